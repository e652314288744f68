// lgh_diag.hip — conservation and mesh-health diagnostics of a state: the conserved integrals, the extremes of the point
// values and the counts of bad points, per zone and folded over zones and ranks (the driver's `-hist` time history).
//
//   point quantities ...... those of QUpdateBody, the reference's laghos_solver.cpp:1074-1083: detJ of J = grad x,
//                          rho = (1/w) rho0DetJ0w / detJ, p = (gamma_z - 1) rho max(e, 0)
//   integrals ............. InternalEnergy / KineticEnergy, the reference's laghos_solver.cpp:640-697, and mass, volume,
//                          momentum with the same rule
//
// One workgroup per zone at a time evaluates the zone's points (ZoneEval, lgh_zone_eval.hpp: the sum factorisation that the
// profiles and maps use too; the positions it keeps are not read here) and every thread folds its points into 17 partials:
// fixed order in the thread, DPP tree in the wavefront, wavefronts in order - no atomics, the same bits whatever the grid.
// diag_fold_k then folds each of the 17 zone arrays in ascending zone id with one workgroup of fixed shape.
#include "lgh_common.hpp"
#include "lgh_zone_eval.hpp"

#include <algorithm>
#include <climits>
#include <cmath>

namespace lgh
{

constexpr int kDiagZone = LGH_DIAG_ZONE_COUNT;
constexpr int kDiagFoldThreads = 1024;

struct DiagArgs : ZoneArgs
{
   double *out; // [k * NE + z]
};

// 0 sum, 1 min, 2 max
__host__ __device__ constexpr int diag_kind(const int k)
{
   return (k <= 6 || k >= 14) ? 0 : ((k == 7 || k == 8 || k == 10) ? 1 : 2);
}

template <int DIM>
__global__ void __launch_bounds__(256) diag_zones_k(const DiagArgs a)
{
   extern __shared__ double sm[];
   ZoneEval<DIM, kDiagZone * 4> zn(a, sm);
   const int NE = a.NE, NQ = zn.NQ, nt = zn.nt, t = zn.t, lane = t & 63, wid = t >> 6, nw = nt >> 6;
   double *red = zn.red;
   const double inf = INFINITY;
   for (int iz = blockIdx.x; iz < NE; iz += gridDim.x)
   {
      const int z = a.zorder ? a.zorder[iz] : iz;
      zn.fields(a, z, a.map + (size_t)z * zn.ND);
      // ---- the points of this thread, in ascending order; maxima are kept as minima of the negated values
      double acc[kDiagZone];
#pragma unroll
      for (int k = 0; k < kDiagZone; k++) { acc[k] = (diag_kind(k) == 0) ? 0.0 : inf; }
      const double gm1 = a.gamma[z] - 1.0;
      const double x0[DIM] = {}; // (the positions are not read: offsets from the first node, dropped)
      for (int q = t; q < NQ; q += nt)
      {
         double v[DIM], x[DIM], v2;
         bool finite_v;
         const double e = zn.point(q, x0, v, x, v2, finite_v);
         const double det = zn.dj[q], w = a.W[q], m = a.m[(size_t)z * NQ + q];
         const bool fin = isfinite(det) && isfinite(e) && finite_v, inv = det <= 0.0;
         acc[0] += m;
         acc[1] += w * det;
         acc[2] += m * e;
         acc[3] += m * v2;
         for (int c = 0; c < DIM; c++) { acc[4 + c] += m * v[c]; }
         acc[14] += inv ? 1.0 : 0.0;
         acc[15] += (e < 0.0) ? 1.0 : 0.0;
         acc[16] += fin ? 0.0 : 1.0;
         if (fin)
         {
            acc[7] = fmin(acc[7], det);
            acc[10] = fmin(acc[10], e);
            acc[11] = fmin(acc[11], -e);
            acc[13] = fmin(acc[13], -sqrt(v2));
            if (!inv)
            {
               const double rho = (1.0 / w) * m / det;
               acc[8] = fmin(acc[8], rho);
               acc[9] = fmin(acc[9], -rho);
               acc[12] = fmin(acc[12], -(gm1 * rho * fmax(e, 0.0)));
            }
         }
      }
#pragma unroll
      for (int k = 0; k < kDiagZone; k++)
      {
         const double r = (diag_kind(k) == 0) ? wave_sum(acc[k], lane, kWave) : wave_min(acc[k], lane, kWave);
         if (lane == 0) { red[k * 4 + wid] = r; }
      }
      __syncthreads();
      if (t < kDiagZone)
      {
         const int kind = diag_kind(t);
         double r = red[t * 4];
         for (int w = 1; w < nw; w++) { r = (kind == 0) ? r + red[t * 4 + w] : fmin(r, red[t * 4 + w]); }
         if (t == 3) { r *= 0.5; }
         if (kind == 2) { r = -r; }
         a.out[(size_t)t * NE + z] = r;
      }
   }
}

// Slot k = blockIdx.x of the zone arrays folded in ascending zone id by one workgroup of kDiagFoldThreads threads: every
// thread takes zones t, t + 1024, ... in order, then a binary tree in LDS.  g is packed by operation, for the reductions
// over the ranks: [0..9] sums (slots 0-6, 14-16), [10..12] minima (7, 8, 10), [13..16] NEGATED maxima (9, 11, 12, 13),
// [17] the lowest zone id that holds the minimum of slot 7.
__global__ void __launch_bounds__(kDiagFoldThreads) diag_fold_k(const int NE, const double *__restrict__ zone, double *__restrict__ g)
{
   __shared__ double red[kDiagFoldThreads];
   __shared__ int ridx[kDiagFoldThreads];
   const int k = blockIdx.x, t = threadIdx.x, kind = diag_kind(k);
   const double *v = zone + (size_t)k * NE;
   double s = (kind == 0) ? 0.0 : ((kind == 1) ? INFINITY : -INFINITY);
   int bi = INT_MAX;
   for (int i = t; i < NE; i += kDiagFoldThreads)
   {
      const double x = v[i];
      if (kind == 0) { s += x; }
      else if (kind == 1) { if (x < s) { s = x; bi = i; } } // (ascending i: the first zone that holds the value stays)
      else { s = fmax(s, x); }
   }
   red[t] = s;
   ridx[t] = bi;
   __syncthreads();
   for (int off = kDiagFoldThreads / 2; off > 0; off >>= 1)
   {
      if (t < off)
      {
         const double x = red[t + off];
         if (kind == 0) { red[t] += x; }
         else if (kind == 1)
         {
            if (x < red[t] || (k == 7 && x == red[t] && ridx[t + off] < ridx[t])) { red[t] = x; ridx[t] = ridx[t + off]; } // (the zone id: slot 7 only)
         }
         else { red[t] = fmax(red[t], x); }
      }
      __syncthreads();
   }
   if (t == 0)
   {
      const int pk = (k <= 6) ? k : (k >= 14) ? k - 7 : (k == 7) ? 10 : (k == 8) ? 11 : (k == 10) ? 12 : (k == 9) ? 13 : k + 3;
      g[pk] = (kind == 2) ? -red[0] : red[0];
      if (k == 7) { g[17] = (ridx[0] == INT_MAX) ? 0.0 : (double)ridx[0]; } // (no finite point anywhere: every zone holds +inf, the lowest id)
   }
}

static int diag_ready(lgh_ctx *c, const char *who)
{
   if (!c->setup_done)
   {
      set_error("%s: lgh_setup_rho0detj0 has not been called (rho0DetJ0w is not set)", who);
      return LGH_ERR_ARG;
   }
   return LGH_OK;
}

static int diag_zones(lgh_ctx *c, const double *S, double *zone_out)
{
   const int dim = c->dim;
   DiagArgs a;
   size_t lds = 0;
   LGH_PASS(zone_eval_args(c, "lgh_diagnostics", S, kDiagZone * 4, a, lds));
   a.out = zone_out;
   const unsigned threads = (unsigned)std::min(256, 64 * ceil_div(c->NQ, 64));
   const unsigned grid = (unsigned)std::min(c->NE, 1 << 16);
   KtScope kt(c, LGH_KERNEL_DIAG);
   if (dim == 3) { hipLaunchKernelGGL(diag_zones_k<3>, dim3(grid), dim3(threads), lds, c->stream, a); }
   else if (dim == 2) { hipLaunchKernelGGL(diag_zones_k<2>, dim3(grid), dim3(threads), lds, c->stream, a); }
   else { hipLaunchKernelGGL(diag_zones_k<1>, dim3(grid), dim3(threads), lds, c->stream, a); }
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}

} // namespace lgh

using namespace lgh;

extern "C"
{

int lgh_diagnostics_zones(lgh_ctx *c, const double *S, double *zone_out)
{
   LGH_CHECK_ARG(c && S && zone_out);
   const int rc = diag_ready(c, "lgh_diagnostics_zones");
   if (rc) { return rc; }
   return diag_zones(c, S, zone_out);
}

int lgh_diagnostics(lgh_ctx *c, const double *S, double out[LGH_DIAG_COUNT])
{
   LGH_CHECK_ARG(c && S && out);
   int rc = diag_ready(c, "lgh_diagnostics");
   if (rc) { return rc; }
   if (!c->diag_dev) { LGH_PASS(c->diag_dev.alloc((size_t)kDiagZone * c->NE + 32)); }
   double *g = c->diag_dev, *zone = g + 32;
   rc = diag_zones(c, S, zone);
   if (rc) { return rc; }
   hipLaunchKernelGGL(diag_fold_k, dim3(kDiagZone), dim3(kDiagFoldThreads), 0, c->stream, c->NE, (const double *)zone, g);
   LGH_HIP_CHECK(hipGetLastError());
   double h[18];
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   LGH_HIP_CHECK(hipMemcpy(h, g, sizeof(h), hipMemcpyDeviceToHost));
   double rank = (double)c->rank, zid = h[17];
   if (c->multi != 0 && c->comm)
   {
      // sums through the all-reduce (three at a time: the form every transport takes), minima and negated maxima through
      // the min-reduce; then the argmin: the lowest rank among those that hold the minimum, then its zone
      const double own_min = h[10], own_zone = h[17];
      for (int i = 0; i < 10; i += 3)
      {
         rc = allreduce_dev(c, g + i, std::min(3, 10 - i), 0);
         if (rc) { return rc; }
      }
      rc = allreduce_dev(c, g + 10, 7, 1);
      if (rc) { return rc; }
      LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
      LGH_HIP_CHECK(hipMemcpy(h, g, 17 * sizeof(double), hipMemcpyDeviceToHost));
      rank = (own_min == h[10]) ? (double)c->rank : INFINITY;
      rc = lgh_allreduce(c, &rank, 1);
      if (rc) { return rc; }
      zid = (rank == (double)c->rank) ? own_zone : INFINITY;
      rc = lgh_allreduce(c, &zid, 1);
      if (rc) { return rc; }
   }
   for (int k = 0; k <= 6; k++) { out[k] = h[k]; }
   for (int k = 14; k <= 16; k++) { out[k] = h[k - 7]; }
   out[7] = h[10]; out[8] = h[11]; out[10] = h[12];
   out[9] = -h[13]; out[11] = -h[14]; out[12] = -h[15]; out[13] = -h[16];
   out[17] = zid; out[18] = rank; out[19] = 0.0;
   return LGH_OK;
}
}
