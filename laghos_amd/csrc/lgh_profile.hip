// lgh_profile.hip — binned 1-D profiles of a state (lgh_profile; the driver's `-prof`): the point quantities of
// lgh_diag.hip and the position of every quadrature point, reduced into uniform bins of a coordinate (x, y, z or the
// distance from an origin).  The bin sums are exact and order-free: the same bits for every zone order, node numbering,
// launch grid and rank count.
//
// Point evaluation: ZoneEval (lgh_zone_eval.hpp), one workgroup per zone at a time; the last axis gives the position x_q
// beside v_q and e_q.  Reduction: the exact binned sums of lgh_binsum.hpp, which describes the scheme, with seven sum columns
// and the density's extremes as the bits of a positive double.
//
// What is this file's own is how a wavefront walks its rows.  A zone's points fall into few rows that lie side by side, so
// the wavefront takes the range of its rows by wave_min and folds row after row of it (prof_fold_head, prof_fold_column:
// one atomic per non-zero limb, from lane 0).  A range of `fold` rows or more (LGH_PROFILE_FOLD; one zone under thousands of
// bins) takes one atomic per lane and non-zero limb instead (prof_lane_tail).
#include "lgh_binsum.hpp"
#include "lgh_zone_eval.hpp"

#include <cmath>
#include <cstdlib>

namespace lgh
{

constexpr int kProfSums = 7;           // vol mass ie ke mom pv mxi: columns 1..7 of a row
static_assert(kProfSums + 3 == LGH_PROFILE_COLS, "a row: n, the sums, rho_min, rho_max");

struct ProfArgs : ZoneArgs
{
   int axis, nbins, fold;
   double lo, inv_w, origin[3];
   ProfScratch s;
};

template <int DIM, int PASS>
__global__ void __launch_bounds__(256) prof_zones_k(const ProfArgs a)
{
   extern __shared__ double sm[];
   ZoneEval<DIM, kProfRed> zn(a, sm);
   const int NE = a.NE, N = a.N, NQ = zn.NQ, nt = zn.nt, t = zn.t, lane = t & 63;
   int E[kProfSums];
   double mx[kProfSums];
#pragma unroll
   for (int k = 0; k < kProfSums; k++)
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
         double xi, vn;
         if (a.axis < 3)
         {
            xi = x[0];
            vn = v[0];
            for (int c = 1; c < DIM; c++) { if (a.axis == c) { xi = x[c]; vn = v[c]; } }
         }
         else
         {
            double r2 = 0.0, vd = 0.0;
            for (int c = 0; c < DIM; c++)
            {
               const double d = x[c] - a.origin[c];
               r2 += d * d;
               vd += v[c] * d;
            }
            xi = sqrt(r2);
            vn = (xi > 0.0) ? vd / xi : 0.0;
         }
         const bool ok = live && fin && isfinite(det) && isfinite(e) && isfinite(xi) && det > 0.0;
         if (live && !ok && PASS == 1) { n_excl++; }
         const double wd = w * det, rho = (1.0 / w) * m / det;
         double ad[kProfSums];
         ad[0] = wd;
         ad[1] = m;
         ad[2] = m * e;
         ad[3] = 0.5 * (m * v2);
         ad[4] = m * vn;
         ad[5] = wd * (gm1 * rho * fmax(e, 0.0));
         ad[6] = m * xi;
         if (PASS == 0)
         {
            if (ok)
            {
#pragma unroll
               for (int k = 0; k < kProfSums; k++)
               {
                  const double f = fabs(ad[k]);
                  if (f < INFINITY) { mx[k] = fmax(mx[k], f); }
               }
            }
            continue;
         }
         const double b = floor((xi - a.lo) * a.inv_w);
         const int row = !ok ? -1 : ((b < 0.0) ? 0 : ((b >= (double)a.nbins) ? a.nbins + 1 : 1 + (int)b));
         const double rlo_d = wave_min(ok ? (double)row : INFINITY, lane, kWave);
         if (!(rlo_d < INFINITY)) { continue; } // (wave-uniform: no lane of this wavefront has a point)
         const int rlo = (int)rlo_d, rhi = (int)-wave_min(ok ? -(double)row : INFINITY, lane, kWave);
         const unsigned long long rb = (unsigned long long)__double_as_longlong(rho);
         if (rhi - rlo < a.fold)
         {
            for (int r = rlo; r <= rhi; r++)
            {
               const bool mine = row == r;
               const unsigned long long in_row = __ballot(mine);
               if (in_row == 0) { continue; }
               prof_fold_head(a.s, r, in_row, mine ? ~rb : 0ULL, mine ? rb : 0ULL, lane);
#pragma unroll
               for (int k = 0; k < kProfSums; k++)
               {
                  long long *wp = a.s.words + ((size_t)r * kProfSums + k) * kProfWords;
                  prof_fold_column(mine, ad[k], E[k], a.s.flags + (size_t)r * kProfSums + k, lane, [&](const int j, const long long sum) {
                     if (lane == 0 && sum != 0) { prof_add(wp + j, sum); }
                  });
               }
            }
         }
         else if (ok) { prof_lane_tail<kProfSums, 0, 0>(a.s, row, ~rb, rb, ad, E); }
      }
   }
   if (PASS == 0) { prof_store_maxima<kProfSums>(a.s, mx, zn.red); }
   else
   {
      const long long n = wave_sum_i64(n_excl);
      if (lane == 0 && n != 0) { prof_add((long long *)a.s.excl, n); }
   }
}

} // namespace lgh

using namespace lgh;

extern "C" int lgh_profile(lgh_ctx *c, const double *S, const lgh_profile_spec *spec, double *out, long *n_excluded)
{
   LGH_CHECK_ARG(c && S && spec && out && n_excluded);
   if (!c->setup_done)
   {
      set_error("lgh_profile: lgh_setup_rho0detj0 has not been called (rho0DetJ0w is not set)");
      return LGH_ERR_ARG;
   }
   const int dim = c->dim;
   LGH_CHECK_ARG(spec->axis >= 0 && spec->axis <= 3 && (spec->axis == 3 || spec->axis < dim));
   LGH_CHECK_ARG(spec->nbins >= 1 && spec->nbins <= LGH_PROFILE_MAX_BINS);
   LGH_CHECK_ARG(std::isfinite(spec->lo) && std::isfinite(spec->hi) && spec->lo < spec->hi && std::isfinite(spec->hi - spec->lo));
   if (spec->axis == 3)
   {
      for (int k = 0; k < dim; k++) { LGH_CHECK_ARG(std::isfinite(spec->origin[k])); }
   }
   const int R = spec->nbins + 2;
   ProfArgs a;
   LGH_PASS(prof_scratch<kProfSums>(c->prof_dev, c->prof_rows, R, a.s));
   size_t lds = 0;
   LGH_PASS(zone_eval_args(c, "lgh_profile", S, kProfRed, a, lds));
   a.axis = spec->axis; a.nbins = spec->nbins;
   a.lo = spec->lo;
   a.inv_w = (double)spec->nbins / (spec->hi - spec->lo);
   for (int k = 0; k < 3; k++) { a.origin[k] = (spec->axis == 3 && k < dim) ? spec->origin[k] : 0.0; }
   a.fold = c->sw.profile_fold;
   const unsigned threads = (unsigned)std::min(256, 64 * ceil_div(c->NQ, 64));
   const unsigned grid = (unsigned)std::min(c->NE, kProfMaxGrid);
   auto launch = [&](const int pass) {
      if (dim == 3) { hipLaunchKernelGGL((pass ? prof_zones_k<3, 1> : prof_zones_k<3, 0>), dim3(grid), dim3(threads), lds, c->stream, a); }
      else if (dim == 2) { hipLaunchKernelGGL((pass ? prof_zones_k<2, 1> : prof_zones_k<2, 0>), dim3(grid), dim3(threads), lds, c->stream, a); }
      else { hipLaunchKernelGGL((pass ? prof_zones_k<1, 1> : prof_zones_k<1, 0>), dim3(grid), dim3(threads), lds, c->stream, a); }
   };
   return prof_run<kProfSums, ProfKeyPositive>(c, a.s, R, LGH_KERNEL_PROFILE, true, launch, out, n_excluded);
}
