// lgh_diag.hip — conservation and mesh-health diagnostics of a state: the conserved integrals, the extremes of the point
// values and the counts of bad points, per zone and folded over zones and ranks (the driver's `-hist` time history).
//
//   point quantities ...... those of QUpdateBody, the reference's laghos_solver.cpp:1074-1083: detJ of J = grad x,
//                          rho = (1/w) rho0DetJ0w / detJ, p = (gamma_z - 1) rho max(e, 0)
//   integrals ............. InternalEnergy / KineticEnergy, the reference's laghos_solver.cpp:640-697, and mass, volume,
//                          momentum with the same rule
//
// One workgroup per zone at a time.  Phase A gathers the zone's x dofs through h1_map into LDS (as offsets from the zone's
// first node: what the gradient needs, without the cancellation of absolute coordinates) and contracts them with
// the 1-D tables direction by direction (sum factorisation, as lgh_sample.hip: D^dim -> Q D^(dim-1) -> ... with B or G
// per axis); the last axis is contracted by the thread that owns the point, which forms the dim x dim Jacobian in
// registers and leaves detJ in LDS.  Phase B does the same for v and e (through B_l2) and every thread folds its points
// into 17 partials: fixed order in the thread, DPP tree in the wavefront, wavefronts in order - no atomics, the same
// bits whatever the grid.  `TC` dof sets go through the staging buffers at a time (all of them where 64 KB of LDS
// allow, one at Q5Q4 in 3D); every value is the same serial sum either way.
// diag_fold_k then folds each of the 17 zone arrays in ascending zone id with one workgroup of fixed shape.
#include "lgh_common.hpp"
#include "lgh_diag.hpp"

#include <algorithm>
#include <climits>
#include <cmath>

namespace lgh
{

constexpr int kDiagZone = LGH_DIAG_ZONE_COUNT;
constexpr int kDiagFoldThreads = 1024;

struct DiagArgs
{
   const double *S, *B, *G, *Bl, *W, *gamma, *m;
   const int *map, *zorder; // zorder: the library's own order of the zones (nullptr: the caller's)
   double *out;             // [k * NE + z]
   int NE, N, D, Q, L, TC;
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
   const int D = a.D, Q = a.Q, L = a.L, TC = a.TC, N = a.N, NE = a.NE;
   const int ND = ipow_c<DIM>(D), NL = ipow_c<DIM>(L), NQ = ipow_c<DIM>(Q);
   const int Qlow = NQ / Q;                      // points of the axes below the last one
   const int S1 = (DIM == 3) ? D * D * Q : 0;    // one array after the first of two staged axes (3D)
   const int S2 = (DIM == 1) ? ND : D * Qlow;    // one array in front of the last axis: [qlow + Qlow * d]
   double *B = sm, *G = B + Q * D, *Bl = G + Q * D, *dj = Bl + Q * L, *red = dj + NQ, *U = red + kDiagZone * 4;
   double *T1 = U + TC * ND, *P = T1 + 2 * TC * S1;
   const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wid = t >> 6, nw = nt >> 6;
   for (int i = t; i < Q * D; i += nt) { B[i] = a.B[i]; G[i] = a.G[i]; }
   for (int i = t; i < Q * L; i += nt) { Bl[i] = a.Bl[i]; }
   const double inf = INFINITY;
   for (int iz = blockIdx.x; iz < NE; iz += gridDim.x)
   {
      const int z = a.zorder ? a.zorder[iz] : iz;
      const int *zmap = a.map + (size_t)z * ND;
      // ---- phase A: J = grad x -> detJ at every point
      for (int c0 = 0; c0 < DIM; c0 += TC)
      {
         const int nc = min(TC, DIM - c0);
         __syncthreads(); // (the staging buffers are free: their last readers are behind this barrier)
         for (int i = t; i < nc * ND; i += nt)
         {
            const int cc = i / ND, d = i - cc * ND;
            // relative to the zone's first node: J = sum G x is a sum of differences (the rows of G sum to zero), and with x
            // of O(1) and J of O(h) the absolute coordinates would cost J log2(1 / h) bits
            const double *xc = a.S + (size_t)(c0 + cc) * N;
            U[i] = xc[zmap[d]] - xc[zmap[0]];
         }
         __syncthreads();
         if (DIM == 3)
         {
            for (int i = t; i < nc * 2 * S1; i += nt) // x axis: B u and G u, [qx + Q (dy + D dz)]
            {
               const int job = i / S1, o = i - job * S1, cc = job >> 1, r = o % Q, hi = o / Q;
               T1[i] = diag_dot(D, Q, ((job & 1) ? G : B) + r, U + cc * ND + D * hi, 1);
            }
            __syncthreads();
            for (int i = t; i < nc * 3 * S2; i += nt) // y axis: j = 0: B G u (d/dx), 1: G B u (d/dy), 2: B B u, [qx + Q (qy + Q dz)]
            {
               const int job = i / S2, o = i - job * S2, cc = job / 3, j = job - 3 * cc;
               const int lo = o % Q, r = (o / Q) % Q, hi = o / (Q * Q);
               const double *src = T1 + (cc * 2 + (j == 0 ? 1 : 0)) * S1 + lo + Q * D * hi;
               P[((c0 + cc) * 3 + j) * S2 + o] = diag_dot(D, Q, ((j == 1) ? G : B) + r, src, Q);
            }
         }
         else if (DIM == 2)
         {
            for (int i = t; i < nc * 2 * S2; i += nt) // x axis: j = 0: G u (d/dx), 1: B u, [qx + Q dy]
            {
               const int job = i / S2, o = i - job * S2, cc = job >> 1, j = job & 1, r = o % Q, hi = o / Q;
               P[((c0 + cc) * 2 + j) * S2 + o] = diag_dot(D, Q, ((j == 0) ? G : B) + r, U + cc * ND + D * hi, 1);
            }
         }
      }
      __syncthreads();
      for (int q = t; q < NQ; q += nt)
      {
         const int qlow = q % Qlow, qhi = q / Qlow;
         double J[DIM * DIM]; // J[c * DIM + j] = d x_c / d xi_j
         for (int c = 0; c < DIM; c++)
         {
            for (int j = 0; j < DIM; j++)
            {
               const double *src = (DIM == 1) ? U : P + (c * DIM + j) * S2;
               J[c * DIM + j] = diag_dot(D, Q, ((j == DIM - 1) ? G : B) + qhi, src + qlow, Qlow);
            }
         }
         double det;
         if (DIM == 1) { det = J[0]; }
         else if (DIM == 2) { det = J[0] * J[3] - J[1] * J[2]; }
         else
         {
            det = J[0] * (J[4] * J[8] - J[5] * J[7]) - J[1] * (J[3] * J[8] - J[5] * J[6]) + J[2] * (J[3] * J[7] - J[4] * J[6]);
         }
         dj[q] = det;
      }
      // ---- phase B: v and e at every point (fields 0 .. DIM-1: v_c through B_h1, field DIM: e through B_l2)
      for (int f0 = 0; f0 < DIM + 1; f0 += TC)
      {
         const int nf = min(TC, DIM + 1 - f0);
         __syncthreads();
         for (int i = t; i < nf * ND; i += nt)
         {
            const int ff = i / ND, d = i - ff * ND, f = f0 + ff;
            if (f < DIM) { U[i] = a.S[(size_t)(DIM + f) * N + zmap[d]]; }
            else if (d < NL) { U[i] = a.S[(size_t)2 * DIM * N + (size_t)z * NL + d]; }
         }
         if (DIM == 1) { continue; } // (TC = 2 in 1D: one pass, the last axis reads U)
         __syncthreads();
         if (DIM == 3)
         {
            for (int i = t; i < nf * S1; i += nt)
            {
               const int ff = i / S1, o = i - ff * S1, n = (f0 + ff < DIM) ? D : L;
               if (o >= n * n * Q) { continue; }
               const int r = o % Q, hi = o / Q;
               T1[i] = diag_dot(n, Q, ((f0 + ff < DIM) ? B : Bl) + r, U + ff * ND + n * hi, 1);
            }
            __syncthreads();
            for (int i = t; i < nf * S2; i += nt)
            {
               const int ff = i / S2, o = i - ff * S2, n = (f0 + ff < DIM) ? D : L;
               if (o >= n * Q * Q) { continue; }
               const int lo = o % Q, r = (o / Q) % Q, hi = o / (Q * Q);
               P[(f0 + ff) * S2 + o] = diag_dot(n, Q, ((f0 + ff < DIM) ? B : Bl) + r, T1 + ff * S1 + lo + Q * n * hi, Q);
            }
         }
         else
         {
            for (int i = t; i < nf * S2; i += nt)
            {
               const int ff = i / S2, o = i - ff * S2, n = (f0 + ff < DIM) ? D : L;
               if (o >= n * Q) { continue; }
               const int r = o % Q, hi = o / Q;
               P[(f0 + ff) * S2 + o] = diag_dot(n, Q, ((f0 + ff < DIM) ? B : Bl) + r, U + ff * ND + n * hi, 1);
            }
         }
      }
      __syncthreads();
      // ---- the points of this thread, in ascending order; maxima are kept as minima of the negated values
      double acc[kDiagZone];
#pragma unroll
      for (int k = 0; k < kDiagZone; k++) { acc[k] = (diag_kind(k) == 0) ? 0.0 : inf; }
      const double gm1 = a.gamma[z] - 1.0;
      const double *F = (DIM == 1) ? U : P;
      for (int q = t; q < NQ; q += nt)
      {
         const int qlow = q % Qlow, qhi = q / Qlow;
         double v[DIM], v2 = 0.0;
         bool finite_v = true;
         for (int c = 0; c < DIM; c++)
         {
            v[c] = diag_dot(D, Q, B + qhi, F + c * S2 + qlow, Qlow);
            v2 += v[c] * v[c];
            finite_v = finite_v && isfinite(v[c]);
         }
         const double e = diag_dot(L, Q, Bl + qhi, F + DIM * S2 + qlow, Qlow);
         const double det = dj[q], w = a.W[q], m = a.m[(size_t)z * NQ + q];
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
   const int dim = c->dim, D = c->D1D, Q = c->Q1D, L = c->L1D;
   DiagArgs a;
   a.S = S; a.B = c->B; a.G = c->G; a.Bl = c->Bl; a.W = c->W; a.gamma = c->gamma; a.m = c->rho0DetJ0w;
   a.map = c->h1map;
   const MeshOrder *o = mesh_order(c);
   a.zorder = o ? o->zorder_d : nullptr;
   a.out = zone_out;
   a.NE = c->NE; a.N = c->N; a.D = D; a.Q = Q; a.L = L;
   const size_t S1 = (dim == 3) ? (size_t)D * D * Q : 0, S2 = (dim == 1) ? 0 : (size_t)D * (c->NQ / Q);
   const size_t fixed = (size_t)Q * (2 * D + L) + c->NQ + kDiagZone * 4 + (size_t)dim * dim * S2;
   size_t lds = 0;
   for (a.TC = dim + 1; a.TC >= 1; a.TC--) // dof sets in the staging buffers at a time: as many as 64 KB allow
   {
      lds = (fixed + (size_t)a.TC * (c->ND + 2 * S1)) * sizeof(double);
      if (lds <= 64 * 1024 || dim == 1) { break; }
   }
   if (a.TC < 1 || lds > 64 * 1024)
   {
      set_error("lgh_diagnostics: one zone of D1D = %d, Q1D = %d needs %zu bytes of LDS", D, Q, lds);
      return LGH_ERR_UNSUPPORTED;
   }
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
