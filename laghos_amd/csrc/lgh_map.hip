// lgh_map.hip — the flow binned onto a fixed Cartesian grid (lgh_map; the driver's `-map`): the point quantities and the
// positions of lgh_profile, deposited into the cells of a box that does not move with the mesh.  lgh_profile is the one-axis
// case; everything but the scatter is shared with it through lgh_profile.hpp - the evaluation of a zone (ProfZone), pass 0
// for the column maxima and the windows, the split of an addend into the limbs of two sets, non-returning 64-bit integer
// atomics, the NaN flag per (row, column), pack / sums over the ranks / value.  The cell sums are exact and order-free: the
// same bits for every zone order, node numbering, launch grid and rank count.  No floating-point atomic anywhere.
//
// What differs is the fold in front of the atomics.  The points of a wavefront land in a handful of cells whose rows are far
// apart (neighbours along y are n0 rows apart), so there is no range of rows to walk: while lanes remain, the wavefront takes
// the cell of its first remaining lane, ballots the lanes of that cell, folds them per column and limb (wave_sum_i64) and
// retires them.  The 8 columns x 8 limbs of a row are 64 consecutive words, so lane l keeps the folded word l and the row
// goes out as ONE wave instruction over 512 contiguous bytes (the lanes whose word is 0 stay out).  After `fold` distinct
// cells (LGH_MAP_FOLD, default 8) the remaining lanes send their own atomics, one per non-zero limb; 0 sends everything
// that way.  Integer sums: the same bits either way.
#include "lgh_profile.hpp"

#include <cmath>
#include <cstdlib>

namespace lgh
{

constexpr int kMapSums = 8; // vol mass ie ke mom_x mom_y mom_z pv: columns 1..8 of a row
static_assert(kMapSums + 3 == LGH_MAP_COLS, "a row: n, the sums, rho_min, rho_max");
static_assert(kMapSums * kProfWords == kWave, "one word of a row per lane");

struct MapArgs : ProfZoneArgs
{
   int n[3], fold;
   double lo[3], inv_w[3];
   ProfScratch s;
};

template <int DIM, int PASS>
__global__ void __launch_bounds__(256) map_zones_k(const MapArgs a)
{
   extern __shared__ double sm[];
   ProfZone<DIM> zn(a, sm);
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
         unsigned long long rem = __ballot(ok);
         for (int nf = 0; rem != 0 && nf < a.fold; nf++) // (wave-uniform)
         {
            const int r = __builtin_amdgcn_readlane(row, __ffsll((long long)rem) - 1);
            const bool mine = ok && row == r;
            const unsigned long long in_row = __ballot(mine); // (lanes of one cell retire together: all of them still remain)
            const unsigned long long lo_bits = wave_max_u64(mine ? ~rb : 0ULL), hi_bits = wave_max_u64(mine ? rb : 0ULL);
            if (lane == 0)
            {
               prof_add((long long *)a.s.count + r, (long long)__popcll(in_row));
               prof_max(a.s.rmin + r, lo_bits);
               prof_max(a.s.rmax + r, hi_bits);
            }
            long long keep = 0; // word `lane` of the row, folded over the lanes of the cell
#pragma unroll
            for (int k = 0; k < kMapSums; k++)
            {
               if (k >= 4 + DIM && k < 7) { continue; } // (a momentum component above the dimension: nothing but zeros)
               long long l[kProfWords];
               {
                  long long h4[kLimbs] = {0, 0, 0, 0}, l4[kLimbs] = {0, 0, 0, 0};
                  const bool added = !mine || prof_split(h4, l4, ad[k], E[k]);
                  if (__ballot(!added) != 0 && lane == 0) { prof_max(a.s.flags + (size_t)r * kMapSums + k, 1ULL); }
#pragma unroll
                  for (int j = 0; j < kLimbs; j++) { l[j] = h4[j]; l[kLimbs + j] = l4[j]; }
               }
#pragma unroll
               for (int j = 0; j < kProfWords; j++)
               {
                  if (__ballot(l[j] != 0) == 0) { continue; }
                  const long long s = wave_sum_i64(l[j]);
                  if (lane == k * kProfWords + j) { keep = s; }
               }
            }
            if (keep != 0) { prof_add(a.s.words + (size_t)r * (kMapSums * kProfWords) + lane, keep); }
            rem &= ~in_row;
         }
         if ((rem >> lane) & 1ULL) // what is left after `fold` cells: this lane's own atomics
         {
            prof_add((long long *)a.s.count + row, 1LL);
            prof_max(a.s.rmin + row, ~rb);
            prof_max(a.s.rmax + row, rb);
#pragma unroll
            for (int k = 0; k < kMapSums; k++)
            {
               if (k >= 4 + DIM && k < 7) { continue; }
               long long h4[kLimbs] = {0, 0, 0, 0}, l4[kLimbs] = {0, 0, 0, 0};
               long long *wp = a.s.words + ((size_t)row * kMapSums + k) * kProfWords;
               if (!prof_split(h4, l4, ad[k], E[k])) { prof_max(a.s.flags + (size_t)row * kMapSums + k, 1ULL); continue; }
#pragma unroll
               for (int j = 0; j < kLimbs; j++)
               {
                  if (h4[j] != 0) { prof_add(wp + j, h4[j]); }
                  if (l4[j] != 0) { prof_add(wp + kLimbs + j, l4[j]); }
               }
            }
         }
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
   if (R > c->map_rows)
   {
      c->map_rows = 0;
      const size_t bytes = prof_layout<kMapSums>(nullptr, R).bytes;
      if (c->map_dev.alloc(bytes) != LGH_OK)
      {
         (void)hipGetLastError(); // (cleared: the context stays usable, a smaller grid may still fit)
         set_error("lgh_map: cannot allocate %zu bytes of scratch memory for %ld cells", bytes, ncells);
         return LGH_ERR_HIP;
      }
      c->map_rows = R;
   }
   MapArgs a;
   a.s = prof_layout<kMapSums>(c->map_dev, c->map_rows);
   size_t lds = 0;
   {
      const int rc = prof_zone_args(c, "lgh_map", S, a, lds);
      if (rc) { return rc; }
   }
   for (int k = 0; k < 3; k++)
   {
      a.n[k] = spec->n[k];
      a.lo[k] = (k < dim) ? spec->lo[k] : 0.0;
      a.inv_w[k] = (k < dim) ? (double)spec->n[k] / (spec->hi[k] - spec->lo[k]) : 1.0;
   }
   a.fold = c->sw.map_fold;
   const unsigned threads = (unsigned)std::min(256, 64 * ceil_div(c->NQ, 64));
   const unsigned grid = (unsigned)std::min(c->NE, kProfMaxGrid);
   const bool multi = c->multi != 0 && c->comm;
   {
      KtScope kt(c, LGH_KERNEL_MAP);
      LGH_HIP_CHECK(hipMemsetAsync(c->map_dev, 0, a.s.int_bytes, c->stream));
      if (dim == 3) { hipLaunchKernelGGL((map_zones_k<3, 0>), dim3(grid), dim3(threads), lds, c->stream, a); }
      else if (dim == 2) { hipLaunchKernelGGL((map_zones_k<2, 0>), dim3(grid), dim3(threads), lds, c->stream, a); }
      else { hipLaunchKernelGGL((map_zones_k<1, 0>), dim3(grid), dim3(threads), lds, c->stream, a); }
      LGH_HIP_CHECK(hipGetLastError());
      hipLaunchKernelGGL(prof_window_k<kMapSums>, dim3(1), dim3(64), 0, c->stream, a.s);
      LGH_HIP_CHECK(hipGetLastError());
      if (multi)
      {
         const int rc = allreduce_dev_n(c, a.s.neg, kMapSums, 1);
         if (rc) { return rc; }
      }
      if (dim == 3) { hipLaunchKernelGGL((map_zones_k<3, 1>), dim3(grid), dim3(threads), lds, c->stream, a); }
      else if (dim == 2) { hipLaunchKernelGGL((map_zones_k<2, 1>), dim3(grid), dim3(threads), lds, c->stream, a); }
      else { hipLaunchKernelGGL((map_zones_k<1, 1>), dim3(grid), dim3(threads), lds, c->stream, a); }
      LGH_HIP_CHECK(hipGetLastError());
      // (the kernels behind index by the rows of THIS call; the layout is that of the allocation.  The packed rows cross the
      // ranks through allreduce_dev_n, in pieces of what the transport takes at a time: 8 values on the emulated ones)
      const int rc = prof_finish<kMapSums>(c, a.s, R);
      if (rc) { return rc; }
   }
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   const size_t n_out = (size_t)R * LGH_MAP_COLS;
   LGH_HIP_CHECK(hipMemcpy(out, a.s.out, n_out * sizeof(double), hipMemcpyDeviceToHost));
   double ex = 0.0;
   LGH_HIP_CHECK(hipMemcpy(&ex, a.s.out + n_out, sizeof(double), hipMemcpyDeviceToHost));
   *n_excluded = (long)ex;
   return LGH_OK;
}
