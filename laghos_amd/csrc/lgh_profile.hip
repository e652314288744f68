// lgh_profile.hip — binned 1-D profiles of a state (lgh_profile; the driver's `-prof`): the point quantities of
// lgh_diag.hip and the position of every quadrature point, reduced into uniform bins of a coordinate (x, y, z or the
// distance from an origin).  The bin sums are exact and order-free: the same bits for every zone order, node numbering,
// launch grid and rank count.
//
// Point evaluation: the sum factorisation of diag_zones_k (lgh_diag.hip), one workgroup per zone at a time, with one
// difference - the arrays of phase A that hold B..B (x - x_first) in front of the last axis are kept (phase B puts v and e
// into the arrays of the gradient, which are free by then), so the last axis gives the position x_q beside v_q and e_q.
// The kernel of lgh_diagnostics is left as it is; the two share diag_dot / ipow_c (lgh_diag.hpp).  The evaluation (ProfZone),
// the split into limbs and the kernels in front of and behind the scatter pass live in lgh_profile.hpp, which lgh_map.hip
// (lgh_map: the cells of a Cartesian grid for the bins of one coordinate) uses too; this file keeps the scatter of a profile.
//
// Reduction, in two passes over the zones:
//   pass 0   the maximum of |addend| of each of the seven sum columns over all points that enter a row and whose addend
//            is finite: integer atomic max on the bit pattern of a non-negative double (one per workgroup and column, 16
//            shards), folded by prof_window_k, max-reduced over the ranks (as a min of the negated values).  A maximum is
//            order-free, so the windows below are the same for every numbering, grid and rank count.
//   pass 1   M < 2^e (frexp) gives the window E = max(e + 2, kProfMinE): every addend is below 2^(E-2), half of what
//            exact_add takes (x < 2^31) - the one bit of margin is there so that the two passes, two instantiations of one
//            template, need not round an addend alike.  Capacity needs none: limb 0 of an accumulator holds 2^33 such
//            addends in 64 bits, more points than a mesh has (exact_add's own limit is 2^31).  An addend v is split exactly into
//            hi = trunc(v 2^-g) 2^g with g = E - 128 and lo = v - hi: hi goes into four limbs under E, lo into four more
//            under E - 96 - together seven limbs, 224 bits below 2^E, so that a row of a quiet region beside one loud zone (addends
//            2^-80 of the largest: e and v 10^-12 of it) keeps every bit of its addends; with the 128 bits of one set such
//            a row would keep 46.  The limbs are added into the 64-bit words of (row, column) by non-returning integer
//            atomics; so are the count and the extremes of rho (bit patterns of positive doubles; the minimum as a maximum
//            of the complement, so that one memset clears everything).  An addend that is not finite sets the flag of its
//            (row, column), which comes out NaN.  No floating-point atomic anywhere.
// A zone's points fall into few rows and same-address atomics serialise, so a wavefront folds its lanes per row first:
// the range of rows by wave_min, per row and limb the lanes of other rows zeroed, wave_sum_i64, one atomic per non-zero
// limb.  A range above `fold` rows (one zone under thousands of bins) takes one atomic per lane and non-zero limb instead.
// prof_pack_k then normalises the words of this rank to |limb| < 2^32 as doubles (exact), the sums over the ranks are
// all-reduces of those (exact in any order for fewer than 2^20 ranks), and prof_value_k joins the two sets, resolves the
// carries, takes the sign out and calls exact_value once for the upper and once for the lower limbs.
#include "lgh_profile.hpp"

#include <cmath>
#include <cstdlib>

namespace lgh
{

constexpr int kProfSums = 7;           // vol mass ie ke mom pv mxi: columns 1..7 of a row
static_assert(kProfSums + 3 == LGH_PROFILE_COLS, "a row: n, the sums, rho_min, rho_max");

struct ProfArgs : ProfZoneArgs
{
   int axis, nbins, fold;
   double lo, inv_w, origin[3];
   ProfScratch s;
};

template <int DIM, int PASS>
__global__ void __launch_bounds__(256) prof_zones_k(const ProfArgs a)
{
   extern __shared__ double sm[];
   ProfZone<DIM> zn(a, sm);
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
               const unsigned long long lo_bits = wave_max_u64(mine ? ~rb : 0ULL), hi_bits = wave_max_u64(mine ? rb : 0ULL);
               if (lane == 0)
               {
                  prof_add((long long *)a.s.count + r, (long long)__popcll(in_row));
                  prof_max(a.s.rmin + r, lo_bits);
                  prof_max(a.s.rmax + r, hi_bits);
               }
#pragma unroll
               for (int k = 0; k < kProfSums; k++)
               {
                  long long l[kProfWords];
                  {
                     long long h4[kLimbs] = {0, 0, 0, 0}, l4[kLimbs] = {0, 0, 0, 0};
                     const bool added = !mine || prof_split(h4, l4, ad[k], E[k]);
                     if (__ballot(!added) != 0 && lane == 0) { prof_max(a.s.flags + (size_t)r * kProfSums + k, 1ULL); }
#pragma unroll
                     for (int j = 0; j < kLimbs; j++) { l[j] = h4[j]; l[kLimbs + j] = l4[j]; }
                  }
                  long long *wp = a.s.words + ((size_t)r * kProfSums + k) * kProfWords;
#pragma unroll
                  for (int j = 0; j < kProfWords; j++)
                  {
                     if (__ballot(l[j] != 0) == 0) { continue; }
                     const long long s = wave_sum_i64(l[j]);
                     if (lane == 0 && s != 0) { prof_add(wp + j, s); }
                  }
               }
            }
         }
         else if (ok)
         {
            prof_add((long long *)a.s.count + row, 1LL);
            prof_max(a.s.rmin + row, ~rb);
            prof_max(a.s.rmax + row, rb);
#pragma unroll
            for (int k = 0; k < kProfSums; k++)
            {
               long long h4[kLimbs] = {0, 0, 0, 0}, l4[kLimbs] = {0, 0, 0, 0};
               long long *wp = a.s.words + ((size_t)row * kProfSums + k) * kProfWords;
               if (!prof_split(h4, l4, ad[k], E[k])) { prof_max(a.s.flags + (size_t)row * kProfSums + k, 1ULL); continue; }
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
   if (R > c->prof_rows)
   {
      c->prof_rows = 0;
      LGH_PASS(c->prof_dev.alloc(prof_layout<kProfSums>(nullptr, R).bytes));
      c->prof_rows = R;
   }
   ProfArgs a;
   a.s = prof_layout<kProfSums>(c->prof_dev, c->prof_rows);
   size_t lds = 0;
   {
      const int rc = prof_zone_args(c, "lgh_profile", S, a, lds);
      if (rc) { return rc; }
   }
   a.axis = spec->axis; a.nbins = spec->nbins;
   a.lo = spec->lo;
   a.inv_w = (double)spec->nbins / (spec->hi - spec->lo);
   for (int k = 0; k < 3; k++) { a.origin[k] = (spec->axis == 3 && k < dim) ? spec->origin[k] : 0.0; }
   a.fold = c->sw.profile_fold;
   const unsigned threads = (unsigned)std::min(256, 64 * ceil_div(c->NQ, 64));
   const unsigned grid = (unsigned)std::min(c->NE, kProfMaxGrid);
   const bool multi = c->multi != 0 && c->comm;
   {
      KtScope kt(c, LGH_KERNEL_PROFILE);
      LGH_HIP_CHECK(hipMemsetAsync(c->prof_dev, 0, a.s.int_bytes, c->stream));
      if (dim == 3) { hipLaunchKernelGGL((prof_zones_k<3, 0>), dim3(grid), dim3(threads), lds, c->stream, a); }
      else if (dim == 2) { hipLaunchKernelGGL((prof_zones_k<2, 0>), dim3(grid), dim3(threads), lds, c->stream, a); }
      else { hipLaunchKernelGGL((prof_zones_k<1, 0>), dim3(grid), dim3(threads), lds, c->stream, a); }
      LGH_HIP_CHECK(hipGetLastError());
      hipLaunchKernelGGL(prof_window_k<kProfSums>, dim3(1), dim3(64), 0, c->stream, a.s);
      LGH_HIP_CHECK(hipGetLastError());
      if (multi)
      {
         const int rc = allreduce_dev_n(c, a.s.neg, kProfSums, 1);
         if (rc) { return rc; }
      }
      if (dim == 3) { hipLaunchKernelGGL((prof_zones_k<3, 1>), dim3(grid), dim3(threads), lds, c->stream, a); }
      else if (dim == 2) { hipLaunchKernelGGL((prof_zones_k<2, 1>), dim3(grid), dim3(threads), lds, c->stream, a); }
      else { hipLaunchKernelGGL((prof_zones_k<1, 1>), dim3(grid), dim3(threads), lds, c->stream, a); }
      LGH_HIP_CHECK(hipGetLastError());
      // (the kernels behind index by the rows of THIS call; the layout is that of the allocation)
      const int rc = prof_finish<kProfSums>(c, a.s, R);
      if (rc) { return rc; }
   }
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   const size_t n_out = (size_t)R * LGH_PROFILE_COLS;
   LGH_HIP_CHECK(hipMemcpy(out, a.s.out, n_out * sizeof(double), hipMemcpyDeviceToHost));
   double ex = 0.0;
   LGH_HIP_CHECK(hipMemcpy(&ex, a.s.out + n_out, sizeof(double), hipMemcpyDeviceToHost));
   *n_excluded = (long)ex;
   return LGH_OK;
}
