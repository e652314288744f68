// lgh_profile.hpp — what lgh_profile.hip (lgh_profile: bins of one coordinate) and lgh_map.hip (lgh_map: cells of a fixed
// Cartesian grid) share: the evaluation of one zone's points (ProfZone), the split of an addend into the limbs of the two
// sets, the scratch layout, and the kernels in front of and behind the pass that scatters - window, pack and value -
// over the number NS of sum columns (7 for a profile, 8 for a map).  The comments of lgh_profile.hip describe the scheme.
#pragma once
#include "lgh_common.hpp"
#include "lgh_diag.hpp"
#include "lgh_vcg.hpp"

#include <algorithm>

namespace lgh
{

constexpr int kProfWords = 2 * kLimbs; // per (row, column): the limbs of hi, then those of lo
constexpr int kProfGranule = 128;      // hi is a multiple of 2^(E - 128), the lowest unit of its set; |lo| < 2^(E - 128)
constexpr int kProfLoShift = 96;       // the window of lo is E - 96: its limb j weighs what limb j + 3 of hi weighs (its limb 0 stays
                                       // below one unit per addend), so the two sets are ONE number of seven limbs, 224 bits below 2^E
constexpr int kProfMinE = -760;        // (every scaling of exact_add and of the split stays in range down to the denormals)
constexpr int kProfShards = 16, kProfShardStride = 16; // pass 0: copies of the column maxima, 128 bytes apart
constexpr int kProfPack = 2 * (kLimbs + 1);            // doubles per (row, column) in the packed form: top, limbs; twice
constexpr int kProfMaxGrid = 2048;
constexpr int kProfMaxSums = 8;        // (the maxima of a shard, `neg` and the 32 doubles of `red` hold that many columns)

struct ProfScratch // one allocation; the integer part is cleared by one memset per call
{
   long long *words;            // [R * NS * 8]
   unsigned long long *flags;   // [R * NS]
   unsigned long long *count;   // [R]
   unsigned long long *rmin;    // [R]  max of ~bits(rho): the minimum
   unsigned long long *rmax;    // [R]  max of bits(rho)
   unsigned long long *maxbits; // [kProfShards * kProfShardStride]
   unsigned long long *excl;    // [1]
   size_t int_bytes;
   double *neg;                 // [8]   minus the NS maxima (min-reduced over the ranks)
   double *pk;                  // sums: [R * NS * kProfPack] limbs, [R * NS] flags, [R] counts, [1] excluded; minima: [R] rho_min, [R] -rho_max
   double *out;                 // [R * (NS + 3)] + [1] excluded
   size_t bytes;
};

template <int NS>
static ProfScratch prof_layout(void *base, const size_t R)
{
   static_assert(NS <= kProfMaxSums && NS <= kProfShardStride, "the maxima of pass 0 have room for eight columns");
   ProfScratch s;
   char *p = (char *)base;
   auto take = [&](size_t n) { char *q = p; p += (n * 8 + 127) / 128 * 128; return q; };
   s.words = (long long *)take(R * NS * kProfWords);
   s.flags = (unsigned long long *)take(R * NS);
   s.count = (unsigned long long *)take(R);
   s.rmin = (unsigned long long *)take(R);
   s.rmax = (unsigned long long *)take(R);
   s.maxbits = (unsigned long long *)take(kProfShards * kProfShardStride);
   s.excl = (unsigned long long *)take(1);
   s.int_bytes = (size_t)(p - (char *)base);
   s.neg = (double *)take(8);
   s.pk = (double *)take(R * NS * kProfPack + R * NS + 3 * R + 1);
   s.out = (double *)take(R * (NS + 3) + 1);
   s.bytes = (size_t)(p - (char *)base);
   return s;
}

struct ProfZoneArgs // what the evaluation of a zone's points reads
{
   const double *S, *B, *G, *Bl, *W, *gamma, *m;
   const int *map, *zorder;
   int NE, N, D, Q, L, TC;
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

// The evaluation of one zone at a time by a workgroup: the shape, the LDS arrays (prof_zone_lds sizes them), the two
// phases in front of the last axis (fields) and the last axis at one point (point).
template <int DIM>
struct ProfZone
{
   int D, Q, L, TC, N, ND, NL, NQ, Qlow, S1, S2, NU;
   double *B, *G, *Bl, *dj, *red, *U, *T1, *P, *UX;
   int t, nt;

   __device__ __forceinline__ ProfZone(const ProfZoneArgs &a, double *sm)
   {
      D = a.D; Q = a.Q; L = a.L; TC = a.TC; N = a.N;
      ND = ipow_c<DIM>(D); NL = ipow_c<DIM>(L); NQ = ipow_c<DIM>(Q);
      Qlow = NQ / Q;
      S1 = (DIM == 3) ? D * D * Q : 0;
      S2 = (DIM == 1) ? ND : D * Qlow;
      NU = (DIM == 1) ? 3 : TC; // 1D: v, e and the x offsets side by side
      B = sm; G = B + Q * D; Bl = G + Q * D; dj = Bl + Q * L; red = dj + NQ; U = red + 32;
      T1 = U + NU * ND; P = T1 + 2 * TC * S1;
      UX = (DIM == 1) ? U + 2 * ND : U; // where phase A stages the x offsets
      t = threadIdx.x; nt = blockDim.x;
      for (int i = t; i < Q * D; i += nt) { B[i] = a.B[i]; G[i] = a.G[i]; }
      for (int i = t; i < Q * L; i += nt) { Bl[i] = a.Bl[i]; }
   }

   // detJ at every point into dj; v, e and the positions in front of the last axis.  Ends with a barrier.
   __device__ __forceinline__ void fields(const ProfZoneArgs &a, const int z, const int *zmap)
   {
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
         v[c] = diag_dot(D, Q, B + qhi, F + prof_fslot<DIM>(c) * S2 + qlow, Qlow);
         x[c] = xf[c] + diag_dot(D, Q, B + qhi, F + prof_pslot<DIM>(c) * S2 + qlow, Qlow);
         v2 += v[c] * v[c];
         fin = fin && isfinite(v[c]);
      }
      return diag_dot(L, Q, Bl + qhi, F + prof_fslot<DIM>(DIM) * S2 + qlow, Qlow);
   }
};

// pass 0, the end of a workgroup: the maxima mx of its threads into its shard
template <int NS>
__device__ __forceinline__ void prof_store_maxima(const ProfScratch &s, const double (&mx)[NS], double *red)
{
   const int t = threadIdx.x, lane = t & 63, wid = t >> 6, nw = blockDim.x >> 6;
   __syncthreads();
#pragma unroll
   for (int k = 0; k < NS; k++)
   {
      const double r = -wave_min(-mx[k], lane, kWave);
      if (lane == 0) { red[k * 4 + wid] = r; }
   }
   __syncthreads();
   if (t < NS)
   {
      double r = red[t * 4];
      for (int w = 1; w < nw; w++) { r = fmax(r, red[t * 4 + w]); }
      if (r > 0.0) { prof_max(s.maxbits + (blockIdx.x % kProfShards) * kProfShardStride + t, (unsigned long long)__double_as_longlong(r)); }
   }
}

// minus the maximum of |addend| of column t: what the min-reduce over the ranks takes
template <int NS>
__global__ void prof_window_k(const ProfScratch s)
{
   const int t = threadIdx.x;
   if (t >= NS) { return; }
   unsigned long long b = 0;
   for (int sh = 0; sh < kProfShards; sh++) { b = max(b, s.maxbits[sh * kProfShardStride + t]); }
   s.neg[t] = -__longlong_as_double((long long)b);
}

// The words of this rank as doubles: per (row, column) and set the limbs with their carries resolved into [0, 2^32) and the
// rest of limb 0 as a signed `top` (|top| < 2^31 for up to 2^31 addends) - every value converts exactly and sums of them
// over fewer than 2^20 ranks stay exact.  Flags, counts and the excluded points ride with the sums; the extremes go apart.
template <int NS>
__global__ void prof_pack_k(const ProfScratch s, const int R)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   const size_t n_rc = (size_t)R * NS;
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
template <int NS>
__global__ void prof_value_k(const ProfScratch s, const int R)
{
   const int r = blockIdx.x * blockDim.x + threadIdx.x;
   if (r >= R) { return; }
   const size_t n_rc = (size_t)R * NS;
   const double *flags = s.pk + n_rc * kProfPack, *count = flags + n_rc, *excl = count + R, *rmin = excl + 1, *rmax = rmin + R;
   double *o = s.out + (size_t)r * (NS + 3);
   o[0] = count[r];
   for (int k = 0; k < NS; k++)
   {
      const size_t i = (size_t)r * NS + k;
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
   o[NS + 1] = rmin[r];
   o[NS + 2] = -rmax[r];
   if (r == 0) { s.out[(size_t)R * (NS + 3)] = excl[0]; }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// what every call reads of the context, and the LDS of one zone: as diag_zones_k, with one more array in front of the last
// axis in 2D and the x offsets beside v and e in 1D; the fields go through in chunks of TC where all at once do not fit
inline int prof_zone_args(lgh_ctx *c, const char *who, const double *S, ProfZoneArgs &a, size_t &lds)
{
   const int dim = c->dim, D = c->D1D, Q = c->Q1D, L = c->L1D;
   a.S = S; a.B = c->B; a.G = c->G; a.Bl = c->Bl; a.W = c->W; a.gamma = c->gamma; a.m = c->rho0DetJ0w;
   a.map = c->h1map;
   const MeshOrder *o = mesh_order(c);
   a.zorder = o ? o->zorder_d : nullptr;
   a.NE = c->NE; a.N = c->N; a.D = D; a.Q = Q; a.L = L;
   const size_t S1 = (dim == 3) ? (size_t)D * D * Q : 0, S2 = (dim == 1) ? 0 : (size_t)D * (c->NQ / Q);
   const size_t narr = (dim == 3) ? 9 : (dim == 2 ? 5 : 0);
   const size_t fixed = (size_t)Q * (2 * D + L) + c->NQ + 32 + narr * S2;
   lds = 0;
   for (a.TC = dim + 1; a.TC >= 1; a.TC--)
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

// behind the scatter pass: pack, the sums and minima over the ranks, the values.  s: the layout of the allocation; R: the rows of this call
template <int NS>
inline int prof_finish(lgh_ctx *c, const ProfScratch &s, const int R)
{
   const bool multi = c->multi != 0 && c->comm;
   const long n_rc = (long)R * NS;
   hipLaunchKernelGGL(prof_pack_k<NS>, dim3(ceil_div(n_rc, 256)), dim3(256), 0, c->stream, s, R);
   LGH_HIP_CHECK(hipGetLastError());
   if (multi)
   {
      const long n_sum = n_rc * kProfPack + n_rc + R + 1;
      int rc = allreduce_dev_n(c, s.pk, n_sum, 0);
      if (rc) { return rc; }
      rc = allreduce_dev_n(c, s.pk + n_sum, 2L * R, 1);
      if (rc) { return rc; }
   }
   hipLaunchKernelGGL(prof_value_k<NS>, dim3(ceil_div(R, 64)), dim3(64), 0, c->stream, s, R);
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}

} // namespace lgh
