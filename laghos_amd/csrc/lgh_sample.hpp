// lgh_sample.hpp — what the lattice kernels share (lgh_sample.hip: the fields; lgh_derived.hip: their derivatives): the
// sizes, and the sum-factorisation stages.  Every sum runs over its dofs in ascending order in one thread.
#pragma once
#include "lgh_common.hpp"

namespace lgh
{

constexpr int kSampleMaxTab = 81; // R1 * D1D of the largest lattice table (R1 <= 9, D1D <= 9)
constexpr int kSampleThreads = 256;

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
      double s = 0.0;
      for (int d = 0; d < n; d++) { s += T[r + R1 * d] * u[d * pre]; }
      out[(size_t)(z * NF + f0 + f) * sout + o] = s;
   }
}

// the last axis: value of field f of zone z at lattice point p = r*pre + lo
__device__ __forceinline__ double sample_last(const int n, const int R1, const int pre, const int p, const double *__restrict__ T,
                                              const double *__restrict__ u)
{
   const int lo = p % pre, r = p / pre;
   double s = 0.0;
   for (int d = 0; d < n; d++) { s += T[r + R1 * d] * u[d * pre + lo]; }
   return s;
}

inline int ipow(int b, int e)
{
   int r = 1;
   for (int i = 0; i < e; i++) { r *= b; }
   return r;
}

} // namespace lgh
