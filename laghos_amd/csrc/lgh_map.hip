// lgh_map.hip — the flow binned onto a fixed Cartesian grid (lgh_map; the driver's `-map`): the point quantities and the
// positions of lgh_profile, deposited into the cells of a box that does not move with the mesh.  lgh_profile is the one-axis
// case.  Point evaluation: ZoneEval (lgh_zone_eval.hpp).  Reduction: the exact binned sums of lgh_binsum.hpp with eight sum
// columns and the density's extremes as the bits of a positive double: the same bits for every zone order, node numbering,
// launch grid and rank count.
//
// What differs from a profile is the fold in front of the atomics.  The points of a wavefront land in a handful of cells whose
// rows are far apart (neighbours along y are n0 rows apart), so there is no range of rows to walk: the wavefront scatters by
// cell (prof_scatter_cells) and after `fold` distinct cells (LGH_MAP_FOLD, default 8) the remaining lanes send their own atomics.
#include "lgh_binsum.hpp"
#include "lgh_zone_eval.hpp"

#include <cmath>
#include <cstdlib>

namespace lgh
{

constexpr int kMapSums = 8; // vol mass ie ke mom_x mom_y mom_z pv: columns 1..8 of a row
static_assert(kMapSums + 3 == LGH_MAP_COLS, "a row: n, the sums, rho_min, rho_max");

struct MapArgs : ZoneArgs
{
   int n[3], fold;
   double lo[3], inv_w[3];
   ProfScratch s;
};

template <int DIM, int PASS>
__global__ void __launch_bounds__(256) map_zones_k(const MapArgs a)
{
   extern __shared__ double sm[];
   ZoneEval<DIM, kProfRed> zn(a, sm);
   const int NE = a.NE, N = a.N, NQ = zn.NQ, nt = zn.nt, t = zn.t, lane = t & 63;
   int E[kMapSums];
   double mx[kMapSums];
#pragma unroll
   for (int k = 0; k < kMapSums; k++)
   {
      E[k] = (PASS == 1) ? prof_window(a.s.neg[k]) : 0;
      mx[k] = 0.0;
   }
   long long n_excl = 0;
   for (int iz = blockIdx.x; iz < NE; iz += gridDim.x)
   {
      const int z = a.zorder ? a.zorder[iz] : iz;
      const int *zmap = a.map + (size_t)z * zn.ND;
      zn.fields(a, z, zmap);
      // ---- the points: every thread of a wavefront walks the loop (the folds below need all 64 lanes)
      const double gm1 = a.gamma[z] - 1.0;
      double xf[DIM];
      for (int c = 0; c < DIM; c++) { xf[c] = a.S[(size_t)c * N + zmap[0]]; }
      for (int q0 = 0; q0 < NQ; q0 += nt)
      {
         const bool live = q0 + t < NQ;
         const int q = live ? q0 + t : NQ - 1;
         double v[DIM], x[DIM], v2;
         bool fin;
         const double e = zn.point(q, xf, v, x, v2, fin);
         const double det = zn.dj[q], w = a.W[q], m = a.m[(size_t)z * NQ + q];
         for (int c = 0; c < DIM; c++) { fin = fin && isfinite(x[c]); }
         const bool ok = live && fin && isfinite(det) && isfinite(e) && det > 0.0;
         if (live && !ok && PASS == 1) { n_excl++; }
         const double wd = w * det, rho = (1.0 / w) * m / det;
         double ad[kMapSums];
         ad[0] = wd;
         ad[1] = m;
         ad[2] = m * e;
         ad[3] = 0.5 * (m * v2);
#pragma unroll
         for (int c = 0; c < 3; c++) { ad[4 + c] = (c < DIM) ? m * v[c < DIM ? c : 0] : 0.0; }
         ad[7] = wd * (gm1 * rho * fmax(e, 0.0));
         if (PASS == 0)
         {
            if (ok)
            {
#pragma unroll
               for (int k = 0; k < kMapSums; k++)
               {
                  const double f = fabs(ad[k]);
                  if (f < INFINITY) { mx[k] = fmax(mx[k], f); }
               }
            }
            continue;
         }
         // the cell: row 0 is "outside"; an index is compared as a double, an x far away overflows no integer
         int row = ok ? 1 : -1;
         {
            bool inside = true;
            int cell = 0, stride = 1;
            for (int c = 0; c < DIM; c++)
            {
               const double b = floor((x[c] - a.lo[c]) * a.inv_w[c]);
               const bool in_c = b >= 0.0 && b < (double)a.n[c];
               inside = inside && in_c;
               cell += stride * (in_c ? (int)b : 0);
               stride *= a.n[c];
            }
            if (ok) { row = inside ? 1 + cell : 0; }
         }
         const unsigned long long rb = (unsigned long long)__double_as_longlong(rho);
         // (columns 4 + DIM .. 6: a momentum component above the dimension, nothing but zeros)
         prof_scatter_cells<kMapSums, 4 + DIM, 7>(a.s, ok, row, ~rb, rb, ad, E, a.fold, lane);
      }
   }
   if (PASS == 0) { prof_store_maxima<kMapSums>(a.s, mx, zn.red); }
   else
   {
      const long long n = wave_sum_i64(n_excl);
      if (lane == 0 && n != 0) { prof_add((long long *)a.s.excl, n); }
   }
}

} // namespace lgh

using namespace lgh;

extern "C" int lgh_map(lgh_ctx *c, const double *S, const lgh_map_spec *spec, double *out, long *n_excluded)
{
   LGH_CHECK_ARG(c && S && spec && out && n_excluded);
   if (!c->setup_done)
   {
      set_error("lgh_map: lgh_setup_rho0detj0 has not been called (rho0DetJ0w is not set)");
      return LGH_ERR_ARG;
   }
   const int dim = c->dim;
   long ncells = 1;
   for (int k = 0; k < 3; k++)
   {
      LGH_CHECK_ARG(spec->n[k] >= 1 && (k < dim || spec->n[k] == 1) && spec->n[k] <= LGH_MAP_MAX_CELLS);
      ncells *= spec->n[k];
      LGH_CHECK_ARG(ncells <= LGH_MAP_MAX_CELLS);
      if (k < dim)
      {
         LGH_CHECK_ARG(std::isfinite(spec->lo[k]) && std::isfinite(spec->hi[k]) && spec->lo[k] < spec->hi[k] && std::isfinite(spec->hi[k] - spec->lo[k]));
      }
   }
   const int R = (int)ncells + 1;
   MapArgs a;
   if (prof_scratch<kMapSums>(c->map_dev, c->map_rows, R, a.s) != LGH_OK)
   {
      (void)hipGetLastError(); // (cleared: the context stays usable, a smaller grid may still fit)
      set_error("lgh_map: cannot allocate %zu bytes of scratch memory for %ld cells", prof_layout<kMapSums>(nullptr, R).bytes, ncells);
      return LGH_ERR_HIP;
   }
   size_t lds = 0;
   LGH_PASS(zone_eval_args(c, "lgh_map", S, kProfRed, a, lds));
   for (int k = 0; k < 3; k++)
   {
      a.n[k] = spec->n[k];
      a.lo[k] = (k < dim) ? spec->lo[k] : 0.0;
      a.inv_w[k] = (k < dim) ? (double)spec->n[k] / (spec->hi[k] - spec->lo[k]) : 1.0;
   }
   a.fold = c->sw.map_fold;
   const unsigned threads = (unsigned)std::min(256, 64 * ceil_div(c->NQ, 64));
   const unsigned grid = (unsigned)std::min(c->NE, kProfMaxGrid);
   auto launch = [&](const int pass) {
      if (dim == 3) { hipLaunchKernelGGL((pass ? map_zones_k<3, 1> : map_zones_k<3, 0>), dim3(grid), dim3(threads), lds, c->stream, a); }
      else if (dim == 2) { hipLaunchKernelGGL((pass ? map_zones_k<2, 1> : map_zones_k<2, 0>), dim3(grid), dim3(threads), lds, c->stream, a); }
      else { hipLaunchKernelGGL((pass ? map_zones_k<1, 1> : map_zones_k<1, 0>), dim3(grid), dim3(threads), lds, c->stream, a); }
   };
   return prof_run<kMapSums, ProfKeyPositive>(c, a.s, R, LGH_KERNEL_MAP, true, launch, out, n_excluded);
}
