// lgh_records.hip — running records at material points: peak pressure and its time, the pressure impulse, peak density,
// speed and energy, and the arrival time of a pressure threshold (the driver's `-peaks`).
//
// Replaces nothing in the reference: /root/reference/laghos.cpp writes snapshots only (VisItDataCollection::Save,
// laghos.cpp:845-871).  A lattice point of lgh_sample_fields / lgh_sample_faces is the same particle in every cycle, so a
// record per lattice point needs no point location: the kernel takes the arrays those calls wrote and one block of
// LGH_RECORDS_COLS columns, and folds the sample in.
//
// A streaming kernel: 2 + dim columns read, 8 read and 8 written per point, no reuse, no LDS, no atomics.  One lane takes two
// neighbouring points per trip - one 16-byte load or store per column where the column is 16-byte aligned, two 8-byte ones
// where it is not (with n odd every second column of v and rec starts at 8 mod 16; the choice is per column and uniform over
// the launch, a bit of a kernel argument) - up to 14 loads in flight per lane before the first use; grid-stride over the
// pairs with the grid capped at eight workgroups of four waves per CU; an odd last point is one lane's scalar work.
// Every column but speed_max is formed operation by operation in IEEE double (no contraction: the trapezoid sum
// impulse + h (p_last + p) is an add, a multiply and an add), so that a numpy restatement can hold it to the bit: the file
// is built with -ffp-contract=off (Makefile; the pragma in rec_fold alone did not keep the backend from fusing).
#include "lgh_common.hpp"

#include <algorithm>
#include <cmath>

namespace lgh
{

constexpr int kRecThreads = 256;
constexpr int kRecPerLane = 2; // points per lane per trip: one 16-byte access per column

struct RecordsArgs
{
   const double *p, *rho, *e;
   const double *v[3];
   double *rec[LGH_RECORDS_COLS];
   double t, h, threshold; // h = 0.5 dtr
   long n;
   unsigned aligned; // bit 0..2: p, rho, e; 3..5: v[c]; 6 + c: rec[c]: the column starts at a multiple of 16 bytes
   int first;
};

__device__ __forceinline__ double2 rec_ld2(const double *col, const long i, const bool al)
{
   if (al) { return *reinterpret_cast<const double2 *>(col + i); }
   return make_double2(col[i], col[i + 1]);
}

__device__ __forceinline__ void rec_st2(double *col, const long i, const bool al, const double2 w)
{
   if (al) { *reinterpret_cast<double2 *>(col + i) = w; }
   else
   {
      col[i] = w.x;
      col[i + 1] = w.y;
   }
}

// |v|, squares summed in ascending order (the one column that is not held to the bit: the root is the compiler's)
template <int DIM>
__device__ __forceinline__ double rec_speed(const double v0, const double v1, const double v2)
{
   double s = v0 * v0;
   if (DIM > 1) { s += v1 * v1; }
   if (DIM > 2) { s += v2 * v2; }
   return sqrt(s);
}

// r[c]: the point's record, in and out.  A NaN sample compares false everywhere: no extreme moves, the impulse turns NaN.
__device__ __forceinline__ void rec_fold(const double p, const double rho, const double e, const double speed, const double t, const double h,
                                         const double threshold, double r[LGH_RECORDS_COLS])
{
#pragma clang fp contract(off)
   if (p > r[0])
   {
      r[0] = p;
      r[1] = t;
   }
   const double sum = r[3] + p;
   const double area = h * sum;
   r[2] = r[2] + area;
   r[3] = p;
   if (rho > r[4]) { r[4] = rho; }
   if (speed > r[5]) { r[5] = speed; }
   if (e > r[6]) { r[6] = e; }
   if (r[7] < 0.0 && p >= threshold) { r[7] = t; }
}

__device__ __forceinline__ void rec_start(const double p, const double rho, const double e, const double speed, const double t, const double threshold,
                                          double r[LGH_RECORDS_COLS])
{
   r[0] = p;
   r[1] = t;
   r[2] = 0.0;
   r[3] = p;
   r[4] = rho;
   r[5] = speed;
   r[6] = e;
   r[7] = (p >= threshold) ? t : -1.0;
}

template <int DIM>
__global__ void __launch_bounds__(kRecThreads) records_update_k(const RecordsArgs a)
{
   const long np = a.n >> 1; // pairs
   const long stride = (long)gridDim.x * kRecThreads;
   const unsigned al = a.aligned;
   for (long k = (long)blockIdx.x * kRecThreads + threadIdx.x; k < np; k += stride)
   {
      const long i = 2 * k; // i + 1 <= n - 1
      const double2 p = rec_ld2(a.p, i, al & 1u), rho = rec_ld2(a.rho, i, al & 2u), e = rec_ld2(a.e, i, al & 4u);
      const double2 v0 = rec_ld2(a.v[0], i, al & 8u);
      const double2 v1 = DIM > 1 ? rec_ld2(a.v[1], i, al & 16u) : make_double2(0.0, 0.0);
      const double2 v2 = DIM > 2 ? rec_ld2(a.v[2], i, al & 32u) : make_double2(0.0, 0.0);
      double r0[LGH_RECORDS_COLS], r1[LGH_RECORDS_COLS];
      if (a.first)
      {
         rec_start(p.x, rho.x, e.x, rec_speed<DIM>(v0.x, v1.x, v2.x), a.t, a.threshold, r0);
         rec_start(p.y, rho.y, e.y, rec_speed<DIM>(v0.y, v1.y, v2.y), a.t, a.threshold, r1);
      }
      else
      {
#pragma unroll
         for (int c = 0; c < LGH_RECORDS_COLS; c++)
         {
            const double2 w = rec_ld2(a.rec[c], i, al & (64u << c));
            r0[c] = w.x;
            r1[c] = w.y;
         }
         rec_fold(p.x, rho.x, e.x, rec_speed<DIM>(v0.x, v1.x, v2.x), a.t, a.h, a.threshold, r0);
         rec_fold(p.y, rho.y, e.y, rec_speed<DIM>(v0.y, v1.y, v2.y), a.t, a.h, a.threshold, r1);
      }
#pragma unroll
      for (int c = 0; c < LGH_RECORDS_COLS; c++) { rec_st2(a.rec[c], i, al & (64u << c), make_double2(r0[c], r1[c])); }
   }
   if ((a.n & 1L) && blockIdx.x == 0 && threadIdx.x == 0) // the odd last point
   {
      const long i = a.n - 1;
      const double speed = rec_speed<DIM>(a.v[0][i], DIM > 1 ? a.v[1][i] : 0.0, DIM > 2 ? a.v[2][i] : 0.0);
      double r[LGH_RECORDS_COLS];
      if (a.first) { rec_start(a.p[i], a.rho[i], a.e[i], speed, a.t, a.threshold, r); }
      else
      {
#pragma unroll
         for (int c = 0; c < LGH_RECORDS_COLS; c++) { r[c] = a.rec[c][i]; }
         rec_fold(a.p[i], a.rho[i], a.e[i], speed, a.t, a.h, a.threshold, r);
      }
#pragma unroll
      for (int c = 0; c < LGH_RECORDS_COLS; c++) { a.rec[c][i] = r[c]; }
   }
}

// the launch of lgh_records_update for n points: workgroups, the largest grid, trips of the pair loop
static void rec_shape(lgh_ctx *c, long n, long *blocks, long *cap, long *trips)
{
   if (c->ncu <= 0)
   {
      hipDeviceProp_t prop;
      c->ncu = (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
   }
   *cap = 8L * c->ncu; // eight workgroups of four waves per CU; more points take further trips
   const long np = n / kRecPerLane;
   *blocks = std::max(1L, std::min(*cap, (np + kRecThreads - 1) / kRecThreads));
   *trips = (np + *blocks * kRecThreads - 1) / (*blocks * kRecThreads);
}

} // namespace lgh

using namespace lgh;

extern "C"
{

int lgh_records_update(lgh_ctx *c, long n, int dim, const double *p, const double *rho, const double *e, const double *v, double t, double dtr,
                       double threshold, int first, double *rec)
{
   LGH_CHECK_ARG(c);
   if (n < 0)
   {
      set_error("lgh_records_update: n = %ld points", n);
      return LGH_ERR_ARG;
   }
   if (dim < 1 || dim > 3)
   {
      set_error("lgh_records_update: dim = %d is outside 1..3", dim);
      return LGH_ERR_ARG;
   }
   if (!std::isfinite(t))
   {
      set_error("lgh_records_update: the time t = %g is not finite", t);
      return LGH_ERR_ARG;
   }
   if (!std::isfinite(dtr) || dtr < 0.0)
   {
      set_error("lgh_records_update: the time since the last update dtr = %g must be finite and >= 0", dtr);
      return LGH_ERR_ARG;
   }
   if (first && dtr != 0.0)
   {
      set_error("lgh_records_update: the first update starts the records, but dtr = %g is not 0", dtr);
      return LGH_ERR_ARG;
   }
   if (std::isinf(threshold))
   {
      set_error("lgh_records_update: threshold = %g is infinite (NaN means none)", threshold);
      return LGH_ERR_ARG;
   }
   if (n > 0 && (!p || !rho || !e || !v || !rec))
   {
      set_error("lgh_records_update: %s is NULL with n = %ld", !p ? "p" : !rho ? "rho" : !e ? "e" : !v ? "v" : "rec", n);
      return LGH_ERR_ARG;
   }
   if (n == 0) { return LGH_OK; }
   const void *cols[5] = {p, rho, e, v, rec};
   for (const void *q : cols)
   {
      if (((uintptr_t)q & 7u) != 0)
      {
         set_error("lgh_records_update: the array at %p is not 8-byte aligned", q);
         return LGH_ERR_ARG;
      }
   }
   RecordsArgs a;
   memset(&a, 0, sizeof(a));
   a.p = p; a.rho = rho; a.e = e;
   for (int k = 0; k < 3; k++) { a.v[k] = v + (size_t)std::min(k, dim - 1) * n; } // (the unused ones are never read)
   for (int k = 0; k < LGH_RECORDS_COLS; k++) { a.rec[k] = rec + (size_t)k * n; }
   a.t = t; a.h = 0.5 * dtr; a.threshold = threshold; a.n = n; a.first = first != 0;
   const auto al16 = [](const void *q) { return ((uintptr_t)q & 15u) == 0 ? 1u : 0u; };
   a.aligned = al16(p) | (al16(rho) << 1) | (al16(e) << 2);
   for (int k = 0; k < 3; k++) { a.aligned |= al16(a.v[k]) << (3 + k); }
   for (int k = 0; k < LGH_RECORDS_COLS; k++) { a.aligned |= al16(a.rec[k]) << (6 + k); }
   long blocks, cap, trips;
   rec_shape(c, n, &blocks, &cap, &trips);
   KtScope kt(c, LGH_KERNEL_RECORDS);
   if (dim == 3) { hipLaunchKernelGGL(records_update_k<3>, dim3((unsigned)blocks), dim3(kRecThreads), 0, c->stream, a); }
   else if (dim == 2) { hipLaunchKernelGGL(records_update_k<2>, dim3((unsigned)blocks), dim3(kRecThreads), 0, c->stream, a); }
   else { hipLaunchKernelGGL(records_update_k<1>, dim3((unsigned)blocks), dim3(kRecThreads), 0, c->stream, a); }
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}

int lgh_records_shape(lgh_ctx *c, long n, long out[4])
{
   LGH_CHECK_ARG(c && out && n >= 0);
   long blocks, cap, trips;
   rec_shape(c, n, &blocks, &cap, &trips);
   out[0] = n > 0 ? blocks : 0;
   out[1] = kRecThreads;
   out[2] = kRecPerLane;
   out[3] = n > 0 ? trips : 0;
   return LGH_OK;
}
}
