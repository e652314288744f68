// lgh_sample.hpp — what the lattice kernels share (lgh_sample.hip: the fields; lgh_derived.hip: their derivatives;
// lgh_faces.hip: both on zone faces): the sizes, the sum-factorisation stages, the point expressions and the host side of a
// launch (the checks of R1 and of the tables, their copy, patches per workgroup, the LDS refusal).  Every sum runs
// over its dofs in ascending order in one thread; one text for each expression is what makes the face values the bits of
// the volume values.
#pragma once
#include "lgh_common.hpp"

#include <algorithm>

namespace lgh
{

constexpr int kSampleMaxTab = 81; // R1 * D1D of the largest lattice table (R1 <= 9, D1D <= 9)
constexpr int kSampleThreads = 256;

// The sum every stage is made of: sum_d T[R1*d] u[d*pre], d ascending from 0 in one thread (T: the table at the lattice point's row)
__device__ __forceinline__ double sample_dot(const int n, const int R1, const int pre, const double *__restrict__ T, const double *__restrict__ u)
{
   double s = 0.0;
   for (int d = 0; d < n; d++) { s += T[R1 * d] * u[d * pre]; }
   return s;
}

// One contraction stage along axis a of every field of a group (n dofs per direction, table T[r + R1*d]):
// out[(hi*R1 + r)*pre + lo] = sum_d T[r + R1*d] in[(hi*n + d)*pre + lo], pre = R1^a points done, post = n^(DIM-1-a) to do.
__device__ __forceinline__ void sample_stage(const int nz, const int nf, const int f0, const int NF, const int n, const int R1,
                                             const int pre, const int post, const double *__restrict__ T,
                                             const double *__restrict__ in, const int sin, double *__restrict__ out, const int sout)
{
   const int cnt = post * R1 * pre, total = nz * nf * cnt;
   for (int i = threadIdx.x; i < total; i += kSampleThreads)
   {
      const int o = i % cnt, zf = i / cnt, f = zf % nf, z = zf / nf;
      const int lo = o % pre, r = (o / pre) % R1, hi = o / (pre * R1);
      const double *u = in + (size_t)(z * NF + f0 + f) * sin + (size_t)hi * n * pre + lo;
      out[(size_t)(z * NF + f0 + f) * sout + o] = sample_dot(n, R1, pre, T + r, u);
   }
}

// the last axis: value of field f of zone z at lattice point p = r*pre + lo
__device__ __forceinline__ double sample_last(const int n, const int R1, const int pre, const int p, const double *__restrict__ T,
                                              const double *__restrict__ u)
{
   const int lo = p % pre, r = p / pre;
   return sample_dot(n, R1, pre, T + r, u + lo);
}

// ---- the point expressions the volume kernels and the face kernel (lgh_faces.hip) share: one text, the same bits -----
// pressure of the equation of state at a point of zone gamma gz
__device__ __forceinline__ double sample_pressure(const double gz, const double rv, const double ev) { return (gz - 1.0) * rv * fmax(ev, 0.0); }
// sound speed there
__device__ __forceinline__ double derived_cs(const double gz, const double ev) { return sqrt((gz * (gz - 1.0)) * fmax(ev, 0.0)); }

// det J, adj(J) (J adj(J) = det J I), entry (i, j) at [i][j]
template <int DIM>
__device__ __forceinline__ double derived_adj(const double (&J)[DIM][DIM], double (&A)[DIM][DIM])
{
   if constexpr (DIM == 1)
   {
      A[0][0] = 1.0;
      return J[0][0];
   }
   else if constexpr (DIM == 2)
   {
      A[0][0] = J[1][1]; A[0][1] = -J[0][1];
      A[1][0] = -J[1][0]; A[1][1] = J[0][0];
      return J[0][0] * J[1][1] - J[0][1] * J[1][0];
   }
   else
   {
      A[0][0] = J[1][1] * J[2][2] - J[1][2] * J[2][1];
      A[0][1] = J[0][2] * J[2][1] - J[0][1] * J[2][2];
      A[0][2] = J[0][1] * J[1][2] - J[0][2] * J[1][1];
      A[1][0] = J[1][2] * J[2][0] - J[1][0] * J[2][2];
      A[1][1] = J[0][0] * J[2][2] - J[0][2] * J[2][0];
      A[1][2] = J[0][2] * J[1][0] - J[0][0] * J[1][2];
      A[2][0] = J[1][0] * J[2][1] - J[1][1] * J[2][0];
      A[2][1] = J[0][1] * J[2][0] - J[0][0] * J[2][1];
      A[2][2] = J[0][0] * J[1][1] - J[0][1] * J[1][0];
      return J[0][0] * A[0][0] + J[0][1] * A[1][0] + J[0][2] * A[2][0];
   }
}

// L = (dv/dxi) adj(J) / det J at point pt of NP and what follows from it, stored where an output is asked for
template <int DIM>
__device__ __forceinline__ void derived_grad(const double (&V)[DIM][DIM], const double (&A)[DIM][DIM], const double det, const size_t pt,
                                             const size_t NP, double *gradv, double *div, double *vort)
{
   double Lm[DIM][DIM];
#pragma unroll
   for (int r = 0; r < DIM; r++)
   {
#pragma unroll
      for (int c = 0; c < DIM; c++)
      {
         double s = V[r][0] * A[0][c];
#pragma unroll
         for (int m = 1; m < DIM; m++) { s += V[r][m] * A[m][c]; }
         Lm[r][c] = s / det;
      }
   }
   if (gradv)
   {
#pragma unroll
      for (int r = 0; r < DIM; r++)
      {
#pragma unroll
         for (int c = 0; c < DIM; c++) { gradv[(size_t)(r * DIM + c) * NP + pt] = Lm[r][c]; }
      }
   }
   if (div)
   {
      double s = Lm[0][0];
#pragma unroll
      for (int m = 1; m < DIM; m++) { s += Lm[m][m]; }
      div[pt] = s;
   }
   if (vort)
   {
      if constexpr (DIM == 2) { vort[pt] = Lm[1][0] - Lm[0][1]; }
      if constexpr (DIM == 3)
      {
         vort[pt] = Lm[2][1] - Lm[1][2];
         vort[NP + pt] = Lm[0][2] - Lm[2][0];
         vort[2 * NP + pt] = Lm[1][0] - Lm[0][1];
      }
   }
}

// ---- the host side of a lattice launch, shared by the entries; each keeps its own refusals, its name in the messages, its timer id -----
// what refuses a lattice of R1 points per direction on this context, or LGH_OK
inline int lattice_refusal(const lgh_ctx *c, const int R1)
{
   if (R1 < 2 || R1 > 9) { return LGH_ERR_ARG; }
   return (R1 * c->D1D > kSampleMaxTab || R1 * c->L1D > kSampleMaxTab) ? LGH_ERR_UNSUPPORTED : LGH_OK;
}
// the range of R1, with the entry's message: among an entry's first refusals
inline int lattice_r1(const char *who, const int R1)
{
   if (R1 >= 2 && R1 <= 9) { return LGH_OK; }
   set_error("%s: R1 = %d lattice points per direction is out of range (2 <= R1 <= 9)", who, R1);
   return LGH_ERR_ARG;
}
// The size of the tables, with the entry's message (`bytes`: the form that names the bytes too), behind the entry's own argument
// checks; then the caller's tables - those that are given - copied into the kernel's argument, where they travel by value
inline int lattice_tables(const char *who, const lgh_ctx *c, const int R1, const double *Bh, const double *Gh, const double *Bl, double *Th_arg,
                          double *Gh_arg, double *Tl_arg, const bool bytes = false)
{
   const int D = c->D1D, L = c->L1D;
   if (R1 * D > kSampleMaxTab || R1 * L > kSampleMaxTab)
   {
      if (!bytes) { set_error("%s: lattice tables of R1 * D1D = %d entries (at most %d)", who, R1 * D, kSampleMaxTab); }
      else { set_error("%s: lattice tables of R1 * D1D = %d entries, %zu bytes (at most %d entries)", who, R1 * D, (size_t)R1 * D * sizeof(double), kSampleMaxTab); }
      return LGH_ERR_UNSUPPORTED;
   }
   if (Bh) { std::copy(Bh, Bh + (size_t)R1 * D, Th_arg); }
   if (Gh) { std::copy(Gh, Gh + (size_t)R1 * D, Gh_arg); }
   if (Bl) { std::copy(Bl, Bl + (size_t)R1 * L, Tl_arg); }
   return LGH_OK;
}
// patches (zones, faces, gauges) per workgroup: as many as fit `threads` threads at `pts` each and 48 KB of LDS, at least one
inline int patches_per_group(const int threads, const int pts, const size_t tab_bytes, const size_t patch_bytes)
{
   const size_t budget = 48 * 1024;
   const int by_lds = tab_bytes + patch_bytes <= budget ? (int)((budget - tab_bytes) / patch_bytes) : 1;
   return std::max(1, std::min(threads / pts, by_lds));
}
// one patch (`what`: "zone", "face of a zone") with the tables has to fit the 64 KB of a workgroup
inline int lattice_lds_fits(const char *who, const char *what, const lgh_ctx *c, const int R1, const size_t bytes)
{
   if (bytes <= 64 * 1024) { return LGH_OK; }
   set_error("%s: one %s of D1D = %d on R1 = %d points needs %zu bytes of LDS", who, what, c->D1D, R1, bytes);
   return LGH_ERR_UNSUPPORTED;
}

} // namespace lgh
