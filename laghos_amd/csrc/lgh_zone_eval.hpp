// lgh_zone_eval.hpp — the evaluation of one zone's quadrature points by a workgroup, once: detJ of J = grad x, v, e and the
// position x at every point, by sum factorisation.  lgh_diag.hip (lgh_diagnostics), lgh_profile.hip (lgh_profile) and
// lgh_map.hip (lgh_map) loop over zones and points on top of it; what they do with the point values is theirs.
//
// Phase A gathers the zone's x dofs through h1_map into LDS (as offsets from the zone's first node: what the gradient needs,
// without the cancellation of absolute coordinates) and contracts them with the 1-D tables direction by direction (as
// lgh_sample.hip: D^dim -> Q D^(dim-1) -> ... with B or G per axis); the last axis is contracted by the thread that owns the
// point, which forms the dim x dim Jacobian in registers and leaves detJ in LDS.  Phase B does the same for v and e (through
// B_l2) into the arrays of the gradient, which are free by then; the arrays that hold B..B (x - x_first) in front of the last
// axis stay, so the last axis gives x_q beside v_q and e_q.  `TC` dof sets go through the staging buffers at a time (all of
// them where 64 KB of LDS allow, one at Q5Q4 in 3D); every value is the same serial sum either way.
#pragma once
#include "lgh_common.hpp"

namespace lgh
{

template <int DIM>
__device__ __forceinline__ int ipow_c(const int b)
{
   return (DIM == 3) ? b * b * b : (DIM == 2 ? b * b : b);
}

// one contraction of n terms: sum_d T[Q d] u[stride d]
__device__ __forceinline__ double diag_dot(const int n, const int Q, const double *__restrict__ T, const double *__restrict__ u,
                                           const int stride)
{
   double s = 0.0;
   for (int d = 0; d < n; d++) { s += T[Q * d] * u[stride * d]; }
   return s;
}

struct ZoneArgs // what the evaluation of a zone's points reads
{
   const double *S, *B, *G, *Bl, *W, *gamma, *m;
   const int *map, *zorder; // zorder: the library's own order of the zones (nullptr: the caller's)
   int NE, N, D, Q, L, TC;
};

template <int DIM>
__device__ __forceinline__ int zone_fslot(const int f) // the array of P (1D: of U) that phase B puts field f into
{
   return (DIM == 3) ? (f < 2 ? f : f + 1) : (DIM == 2 ? 2 * f : f);
}
template <int DIM>
__device__ __forceinline__ int zone_pslot(const int c) // the array that holds B..B (x_c - x_first) in front of the last axis
{
   return (DIM == 3) ? 3 * c + 2 : (DIM == 2 ? 2 * c + 1 : 2);
}

// One zone at a time: the shape, the LDS arrays (zone_eval_args sizes them), the two phases in front of the last axis
// (fields) and the last axis at one point (point).  RED: the doubles of `red`, the area the caller folds its wavefronts in.
template <int DIM, int RED>
struct ZoneEval
{
   int D, Q, L, TC, N, ND, NL, NQ, Qlow, S1, S2, NU;
   double *B, *G, *Bl, *dj, *red, *U, *T1, *P, *UX;
   int t, nt;

   __device__ __forceinline__ ZoneEval(const ZoneArgs &a, double *sm)
   {
      D = a.D; Q = a.Q; L = a.L; TC = a.TC; N = a.N;
      ND = ipow_c<DIM>(D); NL = ipow_c<DIM>(L); NQ = ipow_c<DIM>(Q);
      Qlow = NQ / Q;                      // points of the axes below the last one
      S1 = (DIM == 3) ? D * D * Q : 0;    // one array after the first of two staged axes (3D)
      S2 = (DIM == 1) ? ND : D * Qlow;    // one array in front of the last axis: [qlow + Qlow * d]
      NU = (DIM == 1) ? 3 : TC;           // 1D: v, e and the x offsets side by side
      B = sm; G = B + Q * D; Bl = G + Q * D; dj = Bl + Q * L; red = dj + NQ; U = red + RED;
      T1 = U + NU * ND; P = T1 + 2 * TC * S1;
      UX = (DIM == 1) ? U + 2 * ND : U; // where phase A stages the x offsets
      t = threadIdx.x; nt = blockDim.x;
      for (int i = t; i < Q * D; i += nt) { B[i] = a.B[i]; G[i] = a.G[i]; }
      for (int i = t; i < Q * L; i += nt) { Bl[i] = a.Bl[i]; }
   }

   // detJ at every point into dj; v, e and the positions in front of the last axis.  Ends with a barrier.
   __device__ __forceinline__ void fields(const ZoneArgs &a, const int z, const int *zmap)
   {
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
            UX[i] = xc[zmap[d]] - xc[zmap[0]];
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
               const double *src = (DIM == 1) ? UX : P + (c * DIM + j) * S2;
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
      // ---- phase B: v and e (fields 0 .. DIM-1: v_c through B_h1, field DIM: e through B_l2), into the arrays of the
      // gradient (zone_fslot): those of the position stay
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
         if (DIM == 1) { continue; } // (one pass: fields 0 and 1 sit in U where the last axis reads them)
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
               P[zone_fslot<DIM>(f0 + ff) * S2 + o] = diag_dot(n, Q, ((f0 + ff < DIM) ? B : Bl) + r, T1 + ff * S1 + lo + Q * n * hi, Q);
            }
         }
         else
         {
            for (int i = t; i < nf * S2; i += nt)
            {
               const int ff = i / S2, o = i - ff * S2, n = (f0 + ff < DIM) ? D : L;
               if (o >= n * Q) { continue; }
               const int r = o % Q, hi = o / Q;
               P[zone_fslot<DIM>(f0 + ff) * S2 + o] = diag_dot(n, Q, ((f0 + ff < DIM) ? B : Bl) + r, U + ff * ND + n * hi, 1);
            }
         }
      }
      __syncthreads();
   }

   // the last axis at point q: v_q, x_q = xf + ..., |v_q|^2, whether every v component is finite; returns e_q
   __device__ __forceinline__ double point(const int q, const double (&xf)[DIM], double (&v)[DIM], double (&x)[DIM], double &v2, bool &fin) const
   {
      const double *F = (DIM == 1) ? U : P;
      const int qlow = q % Qlow, qhi = q / Qlow;
      v2 = 0.0;
      fin = true;
      for (int c = 0; c < DIM; c++)
      {
         v[c] = diag_dot(D, Q, B + qhi, F + zone_fslot<DIM>(c) * S2 + qlow, Qlow);
         x[c] = xf[c] + diag_dot(D, Q, B + qhi, F + zone_pslot<DIM>(c) * S2 + qlow, Qlow);
         v2 += v[c] * v[c];
         fin = fin && isfinite(v[c]);
      }
      return diag_dot(L, Q, Bl + qhi, F + zone_fslot<DIM>(DIM) * S2 + qlow, Qlow);
   }
};

// ---- host side: what every call reads of the context, and the LDS of one zone with `nred` doubles of `red`; the fields go
// through in chunks of TC where all at once do not fit
inline int zone_eval_args(lgh_ctx *c, const char *who, const double *S, const int nred, ZoneArgs &a, size_t &lds)
{
   const int dim = c->dim, D = c->D1D, Q = c->Q1D, L = c->L1D;
   a.S = S; a.B = c->B; a.G = c->G; a.Bl = c->Bl; a.W = c->W; a.gamma = c->gamma; a.m = c->rho0DetJ0w;
   a.map = c->h1map;
   const MeshOrder *o = mesh_order(c);
   a.zorder = o ? o->zorder_d : nullptr;
   a.NE = c->NE; a.N = c->N; a.D = D; a.Q = Q; a.L = L;
   const size_t S1 = (dim == 3) ? (size_t)D * D * Q : 0, S2 = (dim == 1) ? 0 : (size_t)D * (c->NQ / Q);
   const size_t narr = (dim == 3) ? 9 : (dim == 2 ? 5 : 0);
   const size_t fixed = (size_t)Q * (2 * D + L) + c->NQ + nred + narr * S2;
   lds = 0;
   for (a.TC = dim + 1; a.TC >= 1; a.TC--) // dof sets in the staging buffers at a time: as many as 64 KB allow
   {
      lds = (fixed + (size_t)(dim == 1 ? 3 : a.TC) * c->ND + (size_t)a.TC * 2 * S1) * sizeof(double);
      if (lds <= 64 * 1024 || dim == 1) { break; }
   }
   if (a.TC < 1 || lds > 64 * 1024)
   {
      set_error("%s: one zone of D1D = %d, Q1D = %d needs %zu bytes of LDS", who, D, Q, lds);
      return LGH_ERR_UNSUPPORTED;
   }
   return LGH_OK;
}

} // namespace lgh
