// lgh_fingerprint.hip — the state fingerprint of include/lgh_fingerprint.h over a device vector, and the same over host words.
//
// Replaces nothing in the reference: /root/reference/laghos.cpp has no restart, and its checks compare |e| (laghos.cpp:1441-1463).
// The checkpoint / restart of the driver (laghos_amd/host/checkpoint.cpp) uses it to tell a state that arrived
// in HBM intact from one that did not, and `-fp` prints it: "the same bits" as one line.
//
// One pass over the vector, read only: grid-stride over pairs of words with 16-byte loads (a scalar head where the vector
// is only 8-byte aligned, a scalar tail where an odd word is left), per-lane 64-bit sum and xor, a wave64 fold, a workgroup
// fold through LDS; every workgroup stores its two words, and a last pass of one workgroup folds those (two atomics per
// workgroup on the same two addresses were measured first: 4096 arrivals at one L2 line took 50 of the kernel's 58 us at
// the 32^3 Q3Q2 state).  Integer add and xor are associative and commutative: the two words do not depend on the launch
// shape.
#include "lgh_common.hpp"

#include <algorithm>

#include "../../include/lgh_fingerprint.h"

namespace lgh
{

constexpr int kFpThreads = 256;
constexpr int kFpWaves = kFpThreads / kWave;

__device__ __forceinline__ void fp_take(const ulonglong2 w, const unsigned long long pos, unsigned long long &s, unsigned long long &x)
{
   const unsigned long long h0 = lgh_fp_word(w.x, pos), h1 = lgh_fp_word(w.y, pos + 1ULL);
   s += h0 + h1;
   x ^= h0 ^ h1;
}

// sum and xor over the workgroup: wave64 fold (every lane is live), then the waves through LDS; the totals are thread 0's
__device__ __forceinline__ void fp_fold(unsigned long long &s, unsigned long long &x, unsigned long long *red)
{
   for (int d = kWave / 2; d > 0; d >>= 1)
   {
      s += __shfl_down(s, d, kWave);
      x ^= __shfl_down(x, d, kWave);
   }
   const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
   if (lane == 0)
   {
      red[wave] = s;
      red[kFpWaves + wave] = x;
   }
   __syncthreads();
   if (threadIdx.x == 0)
   {
      for (int w = 1; w < kFpWaves; w++)
      {
         s += red[w];
         x ^= red[kFpWaves + w];
      }
   }
}

// words: the n words, the first at position `offset`; head = 1: words[0] is taken alone and the pairs start at words + 1
// (then 16-byte aligned).  part[2 b], part[2 b + 1] = sum, xor of the h_i workgroup b took.
__global__ void __launch_bounds__(kFpThreads) fingerprint_k(const unsigned long long *__restrict__ words, const long n, const int head,
                                                            const unsigned long long offset, unsigned long long *__restrict__ part)
{
   __shared__ unsigned long long red[2 * kFpWaves];
   const long np = (n - head) >> 1; // pairs
   const ulonglong2 *__restrict__ p = reinterpret_cast<const ulonglong2 *>(words + head);
   const unsigned long long base = offset + (unsigned long long)head;
   const long stride = (long)gridDim.x * kFpThreads;
   long i = (long)blockIdx.x * kFpThreads + threadIdx.x;
   unsigned long long s = 0ULL, x = 0ULL;
   for (; i + 3 * stride < np; i += 4 * stride) // four loads in flight per lane
   {
      const ulonglong2 a0 = p[i], a1 = p[i + stride], a2 = p[i + 2 * stride], a3 = p[i + 3 * stride];
      fp_take(a0, base + 2ULL * (unsigned long long)i, s, x);
      fp_take(a1, base + 2ULL * (unsigned long long)(i + stride), s, x);
      fp_take(a2, base + 2ULL * (unsigned long long)(i + 2 * stride), s, x);
      fp_take(a3, base + 2ULL * (unsigned long long)(i + 3 * stride), s, x);
   }
   for (; i < np; i += stride) { fp_take(p[i], base + 2ULL * (unsigned long long)i, s, x); }
   if (blockIdx.x == 0 && threadIdx.x == 0)
   {
      if (head)
      {
         const unsigned long long h = lgh_fp_word(words[0], offset);
         s += h;
         x ^= h;
      }
      if ((n - head) & 1L)
      {
         const unsigned long long h = lgh_fp_word(words[n - 1], offset + (unsigned long long)(n - 1));
         s += h;
         x ^= h;
      }
   }
   fp_fold(s, x, red);
   if (threadIdx.x == 0)
   {
      part[2 * (size_t)blockIdx.x] = s;
      part[2 * (size_t)blockIdx.x + 1] = x;
   }
}

// the last pass: one workgroup folds the nb pairs of part into out[0], out[1]
__global__ void __launch_bounds__(kFpThreads) fingerprint_fold_k(const unsigned long long *__restrict__ part, const int nb,
                                                                 unsigned long long *__restrict__ out)
{
   __shared__ unsigned long long red[2 * kFpWaves];
   unsigned long long s = 0ULL, x = 0ULL;
   for (int b = threadIdx.x; b < nb; b += kFpThreads)
   {
      s += part[2 * (size_t)b];
      x ^= part[2 * (size_t)b + 1];
   }
   fp_fold(s, x, red);
   if (threadIdx.x == 0)
   {
      out[0] = s;
      out[1] = x;
   }
}

// the launch of lgh_vec_fingerprint for n words at x: workgroups, and whether a scalar head is taken
static void fp_shape(lgh_ctx *c, const void *x, long n, long *blocks, int *head, long *cap)
{
   if (c->ncu <= 0)
   {
      hipDeviceProp_t prop;
      c->ncu = (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
   }
   *cap = 8L * c->ncu; // eight workgroups of four waves per CU: every SIMD full; longer vectors take further passes
   *head = (n > 0 && ((uintptr_t)x & 15u) != 0) ? 1 : 0;
   const long np = (n - *head) >> 1;
   *blocks = std::max(1L, std::min(*cap, (np + kFpThreads - 1) / kFpThreads));
}

} // namespace lgh

using namespace lgh;

extern "C"
{

int lgh_fingerprint_host(const void *words, long n, unsigned long long offset, unsigned long long out[2])
{
   if (!out || n < 0 || (n > 0 && !words))
   {
      set_error("lgh_fingerprint_host: bad argument (n = %ld, words %s, out %s)", n, words ? "given" : "NULL", out ? "given" : "NULL");
      return LGH_ERR_ARG;
   }
   if (((uintptr_t)words & 7u) != 0)
   {
      set_error("lgh_fingerprint_host: the words must be 8-byte aligned");
      return LGH_ERR_ARG;
   }
   out[0] = out[1] = 0ULL;
   lgh_fp_accumulate((const unsigned long long *)words, n, offset, out);
   return LGH_OK;
}

int lgh_vec_fingerprint(lgh_ctx *c, const double *x, long n, unsigned long long offset, unsigned long long out[2])
{
   LGH_CHECK_ARG(c && out && n >= 0 && (x || n == 0));
   LGH_CHECK_ARG(((uintptr_t)x & 7u) == 0);
   if (n == 0)
   {
      out[0] = out[1] = 0ULL;
      return LGH_OK;
   }
   long blocks, cap;
   int head;
   fp_shape(c, x, n, &blocks, &head, &cap);
   // fp_dev: the two words of the result, then two per workgroup of the largest grid (the device, and with it cap, is the context's)
   if (!c->fp_dev) { LGH_PASS(c->fp_dev.alloc(2 + 2 * (size_t)cap)); }
   {
      KtScope kt(c, LGH_KERNEL_FINGERPRINT);
      hipLaunchKernelGGL(fingerprint_k, dim3((unsigned)blocks), dim3(kFpThreads), 0, c->stream, (const unsigned long long *)x, n, head,
                         offset, c->fp_dev + 2);
      hipLaunchKernelGGL(fingerprint_fold_k, dim3(1), dim3(kFpThreads), 0, c->stream, c->fp_dev + 2, (int)blocks, c->fp_dev);
   }
   LGH_HIP_CHECK(hipGetLastError());
   unsigned long long h[2] = {0ULL, 0ULL};
   LGH_HIP_CHECK(hipMemcpyAsync(h, c->fp_dev, sizeof(h), hipMemcpyDeviceToHost, c->stream));
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   out[0] = h[0];
   out[1] = h[1];
   return LGH_OK;
}

int lgh_vec_fingerprint_shape(lgh_ctx *c, const double *x, long n, long out[4])
{
   LGH_CHECK_ARG(c && out && n >= 0);
   long blocks, cap;
   int head;
   fp_shape(c, x, n, &blocks, &head, &cap);
   out[0] = n > 0 ? blocks : 0;
   out[1] = kFpThreads;
   out[2] = head;
   out[3] = 2L * kFpThreads * cap; // words one pass of the largest grid takes
   return LGH_OK;
}
}
