// lgh_profile.hip — binned 1-D profiles of a state (lgh_profile; the driver's `-prof`): the point quantities of
// lgh_diag.hip and the position of every quadrature point, reduced into uniform bins of a coordinate (x, y, z or the
// distance from an origin).  The bin sums are exact and order-free: the same bits for every zone order, node numbering,
// launch grid and rank count.
//
// Point evaluation: the sum factorisation of diag_zones_k (lgh_diag.hip), one workgroup per zone at a time, with one
// difference - the arrays of phase A that hold B..B (x - x_first) in front of the last axis are kept (phase B puts v and e
// into the arrays of the gradient, which are free by then), so the last axis gives the position x_q beside v_q and e_q.
// The kernel of lgh_diagnostics is left as it is; the two share diag_dot / ipow_c (lgh_diag.hpp).
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
#include "lgh_common.hpp"
#include "lgh_diag.hpp"
#include "lgh_vcg.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace lgh
{

constexpr int kProfSums = 7;           // vol mass ie ke mom pv mxi: columns 1..7 of a row
constexpr int kProfWords = 2 * kLimbs; // per (row, column): the limbs of hi, then those of lo
constexpr int kProfGranule = 128;      // hi is a multiple of 2^(E - 128), the lowest unit of its set; |lo| < 2^(E - 128)
constexpr int kProfLoShift = 96;       // the window of lo is E - 96: its limb j weighs what limb j + 3 of hi weighs (its limb 0 stays
                                       // below one unit per addend), so the two sets are ONE number of seven limbs, 224 bits below 2^E
constexpr int kProfMinE = -760;        // (every scaling of exact_add and of the split stays in range down to the denormals)
constexpr int kProfShards = 16, kProfShardStride = 16; // pass 0: copies of the seven maxima, 128 bytes apart
constexpr int kProfPack = 2 * (kLimbs + 1);            // doubles per (row, column) in the packed form: top, limbs; twice
constexpr int kProfMaxGrid = 2048;

struct ProfScratch // one allocation; the integer part is cleared by one memset per call
{
   long long *words;            // [R * 7 * 8]
   unsigned long long *flags;   // [R * 7]
   unsigned long long *count;   // [R]
   unsigned long long *rmin;    // [R]  max of ~bits(rho): the minimum
   unsigned long long *rmax;    // [R]  max of bits(rho)
   unsigned long long *maxbits; // [kProfShards * kProfShardStride]
   unsigned long long *excl;    // [1]
   size_t int_bytes;
   double *neg;                 // [8]   minus the seven maxima (min-reduced over the ranks)
   double *pk;                  // sums: [R * 7 * kProfPack] limbs, [R * 7] flags, [R] counts, [1] excluded; minima: [R] rho_min, [R] -rho_max
   double *out;                 // [R * 10] + [1] excluded
   size_t bytes;
};

static ProfScratch prof_layout(void *base, const int R)
{
   ProfScratch s;
   char *p = (char *)base;
   auto take = [&](size_t n) { char *q = p; p += (n * 8 + 127) / 128 * 128; return q; };
   s.words = (long long *)take((size_t)R * kProfSums * kProfWords);
   s.flags = (unsigned long long *)take((size_t)R * kProfSums);
   s.count = (unsigned long long *)take(R);
   s.rmin = (unsigned long long *)take(R);
   s.rmax = (unsigned long long *)take(R);
   s.maxbits = (unsigned long long *)take(kProfShards * kProfShardStride);
   s.excl = (unsigned long long *)take(1);
   s.int_bytes = (size_t)(p - (char *)base);
   s.neg = (double *)take(8);
   s.pk = (double *)take((size_t)R * kProfSums * kProfPack + (size_t)R * kProfSums + 3 * (size_t)R + 1);
   s.out = (double *)take((size_t)R * LGH_PROFILE_COLS + 1);
   s.bytes = (size_t)(p - (char *)base);
   return s;
}

struct ProfArgs
{
   const double *S, *B, *G, *Bl, *W, *gamma, *m;
   const int *map, *zorder;
   int NE, N, D, Q, L, TC;
   int axis, nbins, fold;
   double lo, inv_w, origin[3];
   ProfScratch s;
};

__device__ __forceinline__ void prof_add(long long *p, const long long v)
{
   (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void prof_max(unsigned long long *p, const unsigned long long v)
{
   (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int prof_window(const double neg_max)
{
   int e;
   (void)frexp(-neg_max, &e); // M = f 2^e, f in [0.5, 1): M < 2^e; M = 0 gives e = 0
   return max(e + 2, kProfMinE);
}
// maximum of an unsigned 64-bit value over the 64 lanes of a full wavefront (DPP, as wave_sum_i64; 0 is the neutral element)
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
#define LGH_U64_STEP(CTRL_, MASK_)                                                                             \
   {                                                                                                            \
      const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v & 0xffffffffULL), CTRL_, MASK_, 0xF, false); \
      const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL_, MASK_, 0xF, false);           \
      const unsigned long long o = ((unsigned long long)hi << 32) | lo;                                         \
      v = (o > v) ? o : v;                                                                                      \
   }
   LGH_U64_STEP(0x111, 0xF) // row_shr:1
   LGH_U64_STEP(0x112, 0xF) // row_shr:2
   LGH_U64_STEP(0x114, 0xF) // row_shr:4
   LGH_U64_STEP(0x118, 0xF) // row_shr:8
   LGH_U64_STEP(0x142, 0xA) // row_bcast:15 into rows 1 and 3
   LGH_U64_STEP(0x143, 0xC) // row_bcast:31 into rows 2 and 3
#undef LGH_U64_STEP
   const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v & 0xffffffffULL), 63);
   const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
   return ((unsigned long long)hi << 32) | lo;
}
// v -> the limbs of hi under E and of lo under E - 96; false (nothing added) when v is not finite.  |v| < 2^(E-2) by pass 0.
__device__ __forceinline__ bool prof_split(long long (&hi)[kLimbs], long long (&lo)[kLimbs], const double v, const int E)
{
   if (!(fabs(v) < ldexp(1.0, E - 1))) { return false; }
   const int g = E - kProfGranule;
   const double h = ldexp(trunc(ldexp(v, -g)), g); // exact: |v 2^-g| < 2^126, and an underflow of the scaling leaves h = 0
   const bool ok = exact_add(hi, h, E) && exact_add(lo, v - h, E - kProfLoShift);
   return ok;
}

template <int DIM>
__device__ __forceinline__ int prof_fslot(const int f) // the array of P (1D: of U) that phase B puts field f into
{
   return (DIM == 3) ? (f < 2 ? f : f + 1) : (DIM == 2 ? 2 * f : f);
}
template <int DIM>
__device__ __forceinline__ int prof_pslot(const int c) // the array that holds B..B (x_c - x_first) in front of the last axis
{
   return (DIM == 3) ? 3 * c + 2 : (DIM == 2 ? 2 * c + 1 : 2);
}

template <int DIM, int PASS>
__global__ void __launch_bounds__(256) prof_zones_k(const ProfArgs a)
{
   extern __shared__ double sm[];
   const int D = a.D, Q = a.Q, L = a.L, TC = a.TC, N = a.N, NE = a.NE;
   const int ND = ipow_c<DIM>(D), NL = ipow_c<DIM>(L), NQ = ipow_c<DIM>(Q);
   const int Qlow = NQ / Q;
   const int S1 = (DIM == 3) ? D * D * Q : 0;
   const int S2 = (DIM == 1) ? ND : D * Qlow;
   const int NU = (DIM == 1) ? 3 : TC; // 1D: v, e and the x offsets side by side
   double *B = sm, *G = B + Q * D, *Bl = G + Q * D, *dj = Bl + Q * L, *red = dj + NQ, *U = red + 32;
   double *T1 = U + NU * ND, *P = T1 + 2 * TC * S1;
   double *UX = (DIM == 1) ? U + 2 * ND : U; // where phase A stages the x offsets
   const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wid = t >> 6, nw = nt >> 6;
   for (int i = t; i < Q * D; i += nt) { B[i] = a.B[i]; G[i] = a.G[i]; }
   for (int i = t; i < Q * L; i += nt) { Bl[i] = a.Bl[i]; }
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
      const int *zmap = a.map + (size_t)z * ND;
      // ---- phase A: J = grad x -> detJ at every point (as diag_zones_k)
      for (int c0 = 0; c0 < DIM; c0 += TC)
      {
         const int nc = min(TC, DIM - c0);
         __syncthreads();
         for (int i = t; i < nc * ND; i += nt)
         {
            const int cc = i / ND, d = i - cc * ND;
            const double *xc = a.S + (size_t)(c0 + cc) * N;
            UX[i] = xc[zmap[d]] - xc[zmap[0]];
         }
         __syncthreads();
         if (DIM == 3)
         {
            for (int i = t; i < nc * 2 * S1; i += nt)
            {
               const int job = i / S1, o = i - job * S1, cc = job >> 1, r = o % Q, hi = o / Q;
               T1[i] = diag_dot(D, Q, ((job & 1) ? G : B) + r, U + cc * ND + D * hi, 1);
            }
            __syncthreads();
            for (int i = t; i < nc * 3 * S2; i += nt) // j = 0: B G u, 1: G B u, 2: B B u
            {
               const int job = i / S2, o = i - job * S2, cc = job / 3, j = job - 3 * cc;
               const int lo = o % Q, r = (o / Q) % Q, hi = o / (Q * Q);
               const double *src = T1 + (cc * 2 + (j == 0 ? 1 : 0)) * S1 + lo + Q * D * hi;
               P[((c0 + cc) * 3 + j) * S2 + o] = diag_dot(D, Q, ((j == 1) ? G : B) + r, src, Q);
            }
         }
         else if (DIM == 2)
         {
            for (int i = t; i < nc * 2 * S2; i += nt) // j = 0: G u, 1: B u
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
         double J[DIM * DIM];
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
      // ---- phase B: v and e, into the arrays of the gradient (prof_fslot): those of the position stay
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
               P[prof_fslot<DIM>(f0 + ff) * S2 + o] = diag_dot(n, Q, ((f0 + ff < DIM) ? B : Bl) + r, T1 + ff * S1 + lo + Q * n * hi, Q);
            }
         }
         else
         {
            for (int i = t; i < nf * S2; i += nt)
            {
               const int ff = i / S2, o = i - ff * S2, n = (f0 + ff < DIM) ? D : L;
               if (o >= n * Q) { continue; }
               const int r = o % Q, hi = o / Q;
               P[prof_fslot<DIM>(f0 + ff) * S2 + o] = diag_dot(n, Q, ((f0 + ff < DIM) ? B : Bl) + r, U + ff * ND + n * hi, 1);
            }
         }
      }
      __syncthreads();
      // ---- the points: every thread of a wavefront walks the loop (the folds below need all 64 lanes)
      const double gm1 = a.gamma[z] - 1.0;
      const double *F = (DIM == 1) ? U : P;
      double xf[DIM];
      for (int c = 0; c < DIM; c++) { xf[c] = a.S[(size_t)c * N + zmap[0]]; }
      for (int q0 = 0; q0 < NQ; q0 += nt)
      {
         const bool live = q0 + t < NQ;
         const int q = live ? q0 + t : NQ - 1;
         const int qlow = q % Qlow, qhi = q / Qlow;
         double v[DIM], x[DIM], v2 = 0.0;
         bool fin = true;
         for (int c = 0; c < DIM; c++)
         {
            v[c] = diag_dot(D, Q, B + qhi, F + prof_fslot<DIM>(c) * S2 + qlow, Qlow);
            x[c] = xf[c] + diag_dot(D, Q, B + qhi, F + prof_pslot<DIM>(c) * S2 + qlow, Qlow);
            v2 += v[c] * v[c];
            fin = fin && isfinite(v[c]);
         }
         const double e = diag_dot(L, Q, Bl + qhi, F + prof_fslot<DIM>(DIM) * S2 + qlow, Qlow);
         const double det = dj[q], w = a.W[q], m = a.m[(size_t)z * NQ + q];
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
   if (PASS == 0)
   {
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kProfSums; k++)
      {
         const double r = -wave_min(-mx[k], lane, kWave);
         if (lane == 0) { red[k * 4 + wid] = r; }
      }
      __syncthreads();
      if (t < kProfSums)
      {
         double r = red[t * 4];
         for (int w = 1; w < nw; w++) { r = fmax(r, red[t * 4 + w]); }
         if (r > 0.0) { prof_max(a.s.maxbits + (blockIdx.x % kProfShards) * kProfShardStride + t, (unsigned long long)__double_as_longlong(r)); }
      }
   }
   else
   {
      const long long n = wave_sum_i64(n_excl);
      if (lane == 0 && n != 0) { prof_add((long long *)a.s.excl, n); }
   }
}

// minus the maximum of |addend| of column t: what the min-reduce over the ranks takes
__global__ void prof_window_k(const ProfScratch s)
{
   const int t = threadIdx.x;
   if (t >= kProfSums) { return; }
   unsigned long long b = 0;
   for (int sh = 0; sh < kProfShards; sh++) { b = max(b, s.maxbits[sh * kProfShardStride + t]); }
   s.neg[t] = -__longlong_as_double((long long)b);
}

// The words of this rank as doubles: per (row, column) and set the limbs with their carries resolved into [0, 2^32) and the
// rest of limb 0 as a signed `top` (|top| < 2^31 for up to 2^31 addends) - every value converts exactly and sums of them
// over fewer than 2^20 ranks stay exact.  Flags, counts and the excluded points ride with the sums; the extremes go apart.
__global__ void prof_pack_k(const ProfScratch s, const int R)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   const size_t n_rc = (size_t)R * kProfSums;
   double *flags = s.pk + n_rc * kProfPack, *count = flags + n_rc, *excl = count + R, *rmin = excl + 1, *rmax = rmin + R;
   if (i < (int)n_rc)
   {
      for (int set = 0; set < 2; set++)
      {
         long long l[kLimbs];
         for (int j = 0; j < kLimbs; j++) { l[j] = s.words[(size_t)i * kProfWords + set * kLimbs + j]; }
         for (int j = kLimbs - 1; j > 0; j--)
         {
            const long long carry = l[j] >> 32;
            l[j] -= carry * 4294967296LL;
            l[j - 1] += carry;
         }
         const long long top = l[0] >> 32;
         l[0] -= top * 4294967296LL;
         double *o = s.pk + (size_t)i * kProfPack + set * (kLimbs + 1);
         o[0] = (double)top;
         for (int j = 0; j < kLimbs; j++) { o[1 + j] = (double)l[j]; }
      }
      flags[i] = (double)s.flags[i];
   }
   if (i < R)
   {
      const unsigned long long n = s.count[i];
      count[i] = (double)n;
      rmin[i] = n ? __longlong_as_double((long long)~s.rmin[i]) : INFINITY;
      rmax[i] = n ? -__longlong_as_double((long long)s.rmax[i]) : INFINITY; // (negated: a min-reduce takes the maximum)
   }
   if (i == 0) { excl[0] = (double)s.excl[0]; }
}

// The rows: per sum column the limbs back as integers (the sums over the ranks are integers below 2^53) and joined into one
// number of seven limbs; carries, then the SIGN taken out - exact_value adds its limbs in floating point, and a negative total
// in carry-resolved form is a large negative top limb plus positive lower ones, which cancel and leave 2^-59 of 2^E where a
// momentum sum may be far smaller than that; the velocity solve only sums positive quantities - and exact_value once for the
// upper four limbs and once for the lower three: two non-negative parts, added smallest first.
__global__ void prof_value_k(const ProfScratch s, const int R)
{
   const int r = blockIdx.x * blockDim.x + threadIdx.x;
   if (r >= R) { return; }
   const size_t n_rc = (size_t)R * kProfSums;
   const double *flags = s.pk + n_rc * kProfPack, *count = flags + n_rc, *excl = count + R, *rmin = excl + 1, *rmax = rmin + R;
   double *o = s.out + (size_t)r * LGH_PROFILE_COLS;
   o[0] = count[r];
   for (int k = 0; k < kProfSums; k++)
   {
      const size_t i = (size_t)r * kProfSums + k;
      const int E = prof_window(s.neg[k]);
      const double *p = s.pk + i * kProfPack;
      long long c[2 * kLimbs - 1];
      for (int j = 0; j < kLimbs; j++) { c[j] = (long long)p[1 + j]; }
      c[0] += (long long)p[0] * 4294967296LL;
      c[kLimbs - 1] += (long long)p[kLimbs + 2] + (long long)p[kLimbs + 1] * 4294967296LL; // limb 0 of lo and its top
      for (int j = 1; j < kLimbs; j++) { c[kLimbs - 1 + j] = (long long)p[kLimbs + 2 + j]; }
      bool neg = false;
      for (int pass = 0; pass < 2; pass++)
      {
         for (int j = 2 * kLimbs - 2; j > 0; j--)
         {
            const long long carry = c[j] >> 32;
            c[j] -= carry * 4294967296LL;
            c[j - 1] += carry;
         }
         if (pass == 1 || c[0] >= 0) { break; }
         neg = true;
         for (int j = 0; j < 2 * kLimbs - 1; j++) { c[j] = -c[j]; }
      }
      long long top[kLimbs], bot[kLimbs];
      for (int j = 0; j < kLimbs; j++) { top[j] = c[j]; bot[j] = (j < kLimbs - 1) ? c[kLimbs + j] : 0; }
      const double val = exact_value(bot, E - 32 * kLimbs) + exact_value(top, E);
      o[1 + k] = (flags[i] != 0.0) ? __builtin_nan("") : (neg ? -val : val);
   }
   o[8] = rmin[r];
   o[9] = -rmax[r];
   if (r == 0) { s.out[(size_t)R * LGH_PROFILE_COLS] = excl[0]; }
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
   const int dim = c->dim, D = c->D1D, Q = c->Q1D, L = c->L1D;
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
      if (c->prof_dev) { LGH_HIP_CHECK(hipFree(c->prof_dev)); c->prof_dev = nullptr; c->prof_rows = 0; }
      LGH_HIP_CHECK(hipMalloc(&c->prof_dev, prof_layout(nullptr, R).bytes));
      c->prof_rows = R;
   }
   ProfArgs a;
   a.s = prof_layout(c->prof_dev, c->prof_rows);
   a.S = S; a.B = c->B; a.G = c->G; a.Bl = c->Bl; a.W = c->W; a.gamma = c->gamma; a.m = c->rho0DetJ0w;
   a.map = c->h1map;
   const MeshOrder *o = mesh_order(c);
   a.zorder = o ? o->zorder_d : nullptr;
   a.NE = c->NE; a.N = c->N; a.D = D; a.Q = Q; a.L = L;
   a.axis = spec->axis; a.nbins = spec->nbins;
   a.lo = spec->lo;
   a.inv_w = (double)spec->nbins / (spec->hi - spec->lo);
   for (int k = 0; k < 3; k++) { a.origin[k] = (spec->axis == 3 && k < dim) ? spec->origin[k] : 0.0; }
   a.fold = c->sw.profile_fold;
   // LDS: as diag_zones_k, with one more array in front of the last axis in 2D and the x offsets beside v and e in 1D
   const size_t S1 = (dim == 3) ? (size_t)D * D * Q : 0, S2 = (dim == 1) ? 0 : (size_t)D * (c->NQ / Q);
   const size_t narr = (dim == 3) ? 9 : (dim == 2 ? 5 : 0);
   const size_t fixed = (size_t)Q * (2 * D + L) + c->NQ + 32 + narr * S2;
   size_t lds = 0;
   for (a.TC = dim + 1; a.TC >= 1; a.TC--)
   {
      lds = (fixed + (size_t)(dim == 1 ? 3 : a.TC) * c->ND + (size_t)a.TC * 2 * S1) * sizeof(double);
      if (lds <= 64 * 1024 || dim == 1) { break; }
   }
   if (a.TC < 1 || lds > 64 * 1024)
   {
      set_error("lgh_profile: one zone of D1D = %d, Q1D = %d needs %zu bytes of LDS", D, Q, lds);
      return LGH_ERR_UNSUPPORTED;
   }
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
      hipLaunchKernelGGL(prof_window_k, dim3(1), dim3(64), 0, c->stream, a.s);
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
      // (the kernels below index by the rows of THIS call; the layout is that of the allocation)
      const int n_rc = R * kProfSums;
      ProfScratch s = a.s;
      hipLaunchKernelGGL(prof_pack_k, dim3(ceil_div(n_rc, 256)), dim3(256), 0, c->stream, s, R);
      LGH_HIP_CHECK(hipGetLastError());
      if (multi)
      {
         const long n_sum = (long)n_rc * kProfPack + n_rc + R + 1;
         int rc = allreduce_dev_n(c, s.pk, n_sum, 0);
         if (rc) { return rc; }
         rc = allreduce_dev_n(c, s.pk + n_sum, 2L * R, 1);
         if (rc) { return rc; }
      }
      hipLaunchKernelGGL(prof_value_k, dim3(ceil_div(R, 64)), dim3(64), 0, c->stream, s, R);
      LGH_HIP_CHECK(hipGetLastError());
   }
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   const size_t n_out = (size_t)R * LGH_PROFILE_COLS;
   LGH_HIP_CHECK(hipMemcpy(out, a.s.out, n_out * sizeof(double), hipMemcpyDeviceToHost));
   double ex = 0.0;
   LGH_HIP_CHECK(hipMemcpy(&ex, a.s.out + n_out, sizeof(double), hipMemcpyDeviceToHost));
   *n_excluded = (long)ex;
   return LGH_OK;
}
