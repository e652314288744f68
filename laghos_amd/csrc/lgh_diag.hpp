// lgh_diag.hpp — the two helpers of the sum-factorised point evaluation that lgh_diag.hip (lgh_diagnostics) and
// lgh_profile.hip (lgh_profile) share: the size of a tensor array and one contraction with a 1-D table.
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

} // namespace lgh
