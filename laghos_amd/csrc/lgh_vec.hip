// lgh_vec.hip — the small vector kernels, their launchers (vec_*, lgh_common.hpp) and the lgh_vec_* entry points.
#include "lgh_common.hpp"

namespace lgh
{

__global__ void __launch_bounds__(256) vec_set_k(double *y, double a, long n)
{
   for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) { y[i] = a; }
}
__global__ void __launch_bounds__(256)
vec_axpby_k(double *z, double a, const double *x, double b, const double *y, long n)
{
   for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
   {
      z[i] = fma(a, x[i], __dmul_rn(b, y[i])); // (one form in both kernels: same bits whatever the alignment)
   }
}
// the same with 16-byte accesses and two of them in flight per thread (all three pointers 16-byte aligned; the
// scalar kernel takes the odd tail): 3.6-3.9 -> ~5 TB/s on the RK stage updates
__global__ void __launch_bounds__(256)
vec_axpby2_k(double2 *z, double a, const double2 *x, double b, const double2 *y, long n2)
{
   const long stride = (long)gridDim.x * blockDim.x;
   long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
   for (; i + stride < n2; i += 2 * stride)
   {
      const double2 x0 = x[i], y0 = y[i], x1 = x[i + stride], y1 = y[i + stride];
      z[i] = make_double2(fma(a, x0.x, __dmul_rn(b, y0.x)), fma(a, x0.y, __dmul_rn(b, y0.y)));
      z[i + stride] = make_double2(fma(a, x1.x, __dmul_rn(b, y1.x)), fma(a, x1.y, __dmul_rn(b, y1.y)));
   }
   if (i < n2)
   {
      const double2 x0 = x[i], y0 = y[i];
      z[i] = make_double2(fma(a, x0.x, __dmul_rn(b, y0.x)), fma(a, x0.y, __dmul_rn(b, y0.y)));
   }
}
// Two RK stage combinations that share their increment y in one pass (round 5): z1 = a1 x1 + b1 y, z2 = a2 x2 + b2 y with the
// expressions of vec_axpby2_k - the same bits as two calls; z2 may alias x2 (z += b k), z1 and z2 must not overlap.
__global__ void __launch_bounds__(256)
vec_axpby_pair_k(double2 *z1, double a1, const double2 *x1, double b1, double2 *z2, double a2, const double2 *x2, double b2, const double2 *y, long n2)
{
   const long stride = (long)gridDim.x * blockDim.x;
   for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n2; i += stride)
   {
      const double2 y0 = y[i], p = x1[i], q = x2[i];
      z1[i] = make_double2(fma(a1, p.x, __dmul_rn(b1, y0.x)), fma(a1, p.y, __dmul_rn(b1, y0.y)));
      z2[i] = make_double2(fma(a2, q.x, __dmul_rn(b2, y0.x)), fma(a2, q.y, __dmul_rn(b2, y0.y)));
   }
}
__global__ void __launch_bounds__(256) vec_neg_k(double *y, long n)
{
   for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) { y[i] = -y[i]; }
}
__global__ void __launch_bounds__(256) vec_zero_list_k(double *y, const int *list, int n)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i < n) { y[list[i]] = 0.0; }
}
__global__ void __launch_bounds__(256)
vec_dot_k(const double *x, const double *y, const double *w, long n, double *partials,
          unsigned int *ticket, double *out)
{
   __shared__ double red[16];
   double s = 0.0;
   for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
   {
      s += (w ? w[i] : 1.0) * x[i] * y[i];
   }
   const double bsum = block_sum(s, red);
   double total;
   if (grid_sum_last_block(bsum, partials, ticket, red, total))
   {
      if (threadIdx.x == 0) { *out = total; }
   }
}
__global__ void set_double_k(double *p, double v) { *p = v; }

int vec_set(lgh_ctx *c, double *y, double a, long n)
{
   if (n <= 0) { return LGH_OK; }
   hipLaunchKernelGGL(vec_set_k, dim3(grid_for(n)), dim3(256), 0, c->stream, y, a, n);
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}
int vec_axpby(lgh_ctx *c, double *z, double a, const double *x, double b, const double *y, long n)
{
   if (n <= 0) { return LGH_OK; }
   if (n >= 4096 && (((uintptr_t)z | (uintptr_t)x | (uintptr_t)y) & 15u) == 0)
   {
      const long n2 = n / 2;
      hipLaunchKernelGGL(vec_axpby2_k, dim3(grid_for(n2)), dim3(256), 0, c->stream, (double2 *)z, a, (const double2 *)x, b,
                         (const double2 *)y, n2);
      if (n & 1) { hipLaunchKernelGGL(vec_axpby_k, dim3(1), dim3(64), 0, c->stream, z + 2 * n2, a, x + 2 * n2, b, y + 2 * n2, 1L); }
   }
   else { hipLaunchKernelGGL(vec_axpby_k, dim3(grid_for(n)), dim3(256), 0, c->stream, z, a, x, b, y, n); }
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}
int vec_axpby_pair(lgh_ctx *c, double *z1, double a1, const double *x1, double b1, double *z2, double a2, const double *x2, double b2,
                   const double *y, long n)
{
   if (n <= 0) { return LGH_OK; }
   if (n >= 4096 && (((uintptr_t)z1 | (uintptr_t)x1 | (uintptr_t)z2 | (uintptr_t)x2 | (uintptr_t)y) & 15u) == 0)
   {
      const long n2 = n / 2;
      hipLaunchKernelGGL(vec_axpby_pair_k, dim3(grid_for(n2)), dim3(256), 0, c->stream, (double2 *)z1, a1, (const double2 *)x1, b1, (double2 *)z2, a2,
                         (const double2 *)x2, b2, (const double2 *)y, n2);
      LGH_HIP_CHECK(hipGetLastError());
      if (n & 1)
      {
         hipLaunchKernelGGL(vec_axpby_k, dim3(1), dim3(64), 0, c->stream, z1 + 2 * n2, a1, x1 + 2 * n2, b1, y + 2 * n2, 1L);
         hipLaunchKernelGGL(vec_axpby_k, dim3(1), dim3(64), 0, c->stream, z2 + 2 * n2, a2, x2 + 2 * n2, b2, y + 2 * n2, 1L);
      }
      LGH_HIP_CHECK(hipGetLastError());
      return LGH_OK;
   }
   LGH_PASS(vec_axpby(c, z1, a1, x1, b1, y, n));
   return vec_axpby(c, z2, a2, x2, b2, y, n);
}
int vec_neg_inplace(lgh_ctx *c, double *y, long n)
{
   if (n <= 0) { return LGH_OK; }
   hipLaunchKernelGGL(vec_neg_k, dim3(grid_for(n)), dim3(256), 0, c->stream, y, n);
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}
int vec_zero_list(lgh_ctx *c, double *y, const int *list, int n)
{
   if (n <= 0) { return LGH_OK; }
   hipLaunchKernelGGL(vec_zero_list_k, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, y, list, n);
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}
int vec_dot(lgh_ctx *c, const double *x, const double *y, const double *w, long n, double *dev_out)
{
   hipLaunchKernelGGL(vec_dot_k, dim3(grid_for(n)), dim3(256), 0, c->stream, x, y, w, n,
                      c->partials + 3 * (size_t)c->part_stride, c->tickets + 3 * kTicketSlot, dev_out);
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}

} // namespace lgh

using namespace lgh;

extern "C"
{

int lgh_vec_set(lgh_ctx *c, double *y, double a, long n) { LGH_CHECK_ARG(c && y); return vec_set(c, y, a, n); }
int lgh_vec_copy(lgh_ctx *c, double *y, const double *x, long n)
{
   LGH_CHECK_ARG(c && y && x);
   LGH_HIP_CHECK(hipMemcpyAsync(y, x, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
   return LGH_OK;
}
int lgh_vec_axpby(lgh_ctx *c, double *z, double a, const double *x, double b, const double *y, long n)
{
   LGH_CHECK_ARG(c && z && x && y);
   return vec_axpby(c, z, a, x, b, y, n);
}
int lgh_vec_axpby_pair(lgh_ctx *c, double *z1, double a1, const double *x1, double b1, double *z2, double a2, const double *x2, double b2,
                       const double *y, long n)
{
   LGH_CHECK_ARG(c && z1 && x1 && z2 && x2 && y && n >= 0);
   // "the same bits as two lgh_vec_axpby calls" only holds when the first result is not an operand of the second: z1 must not
   // overlap z2, x2 or y (round-5 advisor; z1 may be x1, z2 may be x2 - exact aliases, element i is read before it is written)
   {
      auto overlap = [n](const double *p, const double *q) { return p < q + n && q < p + n; };
      LGH_CHECK_ARG(!overlap(z1, z2) && !overlap(z1, x2) && !overlap(z1, y));
      LGH_CHECK_ARG(!overlap(z2, y) && !overlap(z2, x1) && (z2 == x2 || !overlap(z2, x2)) && (z1 == x1 || !overlap(z1, x1)));
   }
   return vec_axpby_pair(c, z1, a1, x1, b1, z2, a2, x2, b2, y, n);
}
int lgh_vec_dot(lgh_ctx *c, const double *x, const double *y, long n, double *result)
{
   LGH_CHECK_ARG(c && x && y && result);
   LGH_PASS(vec_dot(c, x, y, nullptr, n, c->scal + 1));
   LGH_HIP_CHECK(hipMemcpyAsync(c->host_pinned + kPinDot, c->scal + 1, sizeof(double), hipMemcpyDeviceToHost, c->stream));
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   *result = c->host_pinned[kPinDot];
   return LGH_OK;
}

} // extern "C"
