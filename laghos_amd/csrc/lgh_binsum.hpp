// lgh_binsum.hpp — exact, order-free sums of point quantities into rows (bins, cells, lists of faces), once: the scheme that
// lgh_profile.hip, lgh_map.hip and lgh_loads.hip share.  Each of them forms the addends of its points and chooses how a
// wavefront walks its rows; everything else is here, over the number NS of sum columns (7 for a profile, 8 for a map or loads).
// The sums have the same bits for every zone order, node numbering, launch grid and rank count.
//
// Reduction, in two passes over the points (prof_run):
//   pass 0   the maximum of |addend| of each sum column over all points that enter a row and whose addend is finite: integer
//            atomic max on the bit pattern of a non-negative double (one per workgroup and column, 16 shards:
//            prof_store_maxima), folded by prof_window_k, max-reduced over the ranks (as a min of the negated values).  A
//            maximum is order-free, so the windows below are the same for every numbering, grid and rank count.
//   pass 1   M < 2^e (frexp) gives the window E = max(e + 2, kProfMinE): every addend is below 2^(E-2), half of what
//            exact_add takes (x < 2^31) - the one bit of margin is there so that the two passes, two instantiations of one
//            template, need not round an addend alike.  Capacity needs none: limb 0 of an accumulator holds 2^33 such
//            addends in 64 bits, more points than a mesh has (exact_add's own limit is 2^31).  An addend v is split exactly into
//            hi = trunc(v 2^-g) 2^g with g = E - 128 and lo = v - hi (prof_split): hi goes into four limbs under E, lo into four
//            more under E - 96 - together seven limbs, 224 bits below 2^E, so that a row of a quiet region beside one loud zone
//            (addends 2^-80 of the largest: e and v 10^-12 of it) keeps every bit of its addends; with the 128 bits of one
//            set such a row would keep 46.  The limbs are added into the 64-bit words of (row, column) by non-returning
//            integer atomics; so are the count and the two extreme keys (the minimum as a maximum of the complement, so that
//            one memset clears everything; 0 is "none").  An addend that is not finite sets the flag of its (row, column),
//            which comes out NaN.  No floating-point atomic anywhere.
// Same-address atomics serialise, so a wavefront folds the lanes of one row first: prof_fold_head for the count and the
// extremes, prof_fold_column per column - the lanes of other rows zeroed, prof_wave_sum, one atomic per non-zero limb.  Which
// rows it folds is the caller's strategy (a range of rows in lgh_profile.hip; prof_scatter_cells, the cell of the first
// remaining lane, for lgh_map.hip and lgh_loads.hip); the lanes it does not fold send their own atomics (prof_lane_tail).
// prof_pack_k then normalises the words of this rank to |limb| < 2^32 as doubles (exact), the sums over the ranks are
// all-reduces of those (exact in any order for fewer than 2^20 ranks), and prof_value_k joins the two sets, resolves the
// carries, takes the sign out and calls exact_value once for the upper and once for the lower limbs.
#pragma once
#include "lgh_common.hpp"
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
constexpr int kProfRed = 4 * kProfMaxSums; // the doubles prof_store_maxima folds the wavefronts of a workgroup in

struct ProfScratch // one allocation; the integer part is cleared by one memset per call
{
   long long *words;            // [R * NS * 8]
   unsigned long long *flags;   // [R * NS]
   unsigned long long *count;   // [R]
   unsigned long long *rmin;    // [R]  max of the complemented key: the minimum
   unsigned long long *rmax;    // [R]  max of the key
   unsigned long long *maxbits; // [kProfShards * kProfShardStride]
   unsigned long long *excl;    // [1]
   size_t int_bytes;
   double *neg;                 // [8]   minus the NS maxima (min-reduced over the ranks)
   double *pk;                  // sums: [R * NS * kProfPack] limbs, [R * NS] flags, [R] counts, [1] excluded; minima: [R] min, [R] -max
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

// The two extreme words of a row as doubles: what prof_pack_k decodes them with.  The kernels send a key per point and its
// complement as integer maxima, 0 for "none"; lo is the rmin word, hi the rmax word, n the count of the row.  The maximum
// comes out negated, for the min-reduce over the ranks; a row without a value gives +inf twice.
struct ProfKeyPositive // the bits of a positive double as they are, gated by the count (a density: lgh_profile, lgh_map)
{
   static __device__ __forceinline__ double min_of(const unsigned long long lo, const unsigned long long n)
   {
      return n ? __longlong_as_double((long long)~lo) : INFINITY;
   }
   static __device__ __forceinline__ double neg_max_of(const unsigned long long hi, const unsigned long long n)
   {
      return n ? -__longlong_as_double((long long)hi) : INFINITY;
   }
};
struct ProfKeyOrdered // a key that orders ALL doubles but NaN, gated by a non-zero word (a pressure of either sign: lgh_loads)
{
   // grows with p, never 0 for a number: the bits with the sign bit set for p >= 0, their complement below
   static __device__ __forceinline__ unsigned long long key(const double p)
   {
      const long long b = __double_as_longlong(p);
      return (b < 0) ? ~(unsigned long long)b : ((unsigned long long)b | 0x8000000000000000ULL);
   }
   static __device__ __forceinline__ double unkey(const unsigned long long k)
   {
      return __longlong_as_double((long long)((k & 0x8000000000000000ULL) ? (k ^ 0x8000000000000000ULL) : ~k));
   }
   // (an empty row, or one of NaN values only, has no key)
   static __device__ __forceinline__ double min_of(const unsigned long long lo, const unsigned long long) { return lo ? unkey(~lo) : INFINITY; }
   static __device__ __forceinline__ double neg_max_of(const unsigned long long hi, const unsigned long long) { return hi ? -unkey(hi) : INFINITY; }
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

// ---- pass 1, the lanes of a full wavefront that fall into row r (`mine`; in_row = __ballot(mine), not 0) folded into one
// set of atomics.  The head: the count and the two extreme keys (kmin, kmax: 0 in the lanes that have none, or are not mine).
__device__ __forceinline__ void prof_fold_head(const ProfScratch &s, const int r, const unsigned long long in_row, const unsigned long long kmin,
                                               const unsigned long long kmax, const int lane)
{
   const unsigned long long lo_bits = wave_max_u64(kmin), hi_bits = wave_max_u64(kmax);
   if (lane == 0)
   {
      prof_add((long long *)s.count + r, (long long)__popcll(in_row));
      if (lo_bits != 0) { prof_max(s.rmin + r, lo_bits); } // (a maximum with 0 changes nothing: the words are cleared to 0)
      if (hi_bits != 0) { prof_max(s.rmax + r, hi_bits); }
   }
}
// 64-bit integer sum over the 64 lanes of a full wavefront, the total in every lane: wave_sum_i64 (lgh_vcg.hpp) with the DPP
// step taken on the 64-bit value itself.  There a step is `v + (hi << 32 | lo)` of two 32-bit moves, and the compiler turns that
// into two adds, `(v + lo) + (hi << 32)`, for one more step each time the text is inlined one function deeper (two of six steps
// in a kernel, four behind two helpers: 1 % of a map of 64^3 cells).  Here a step is one add however deep the call sits.
__device__ __forceinline__ long long prof_wave_sum(long long v)
{
   v += __builtin_amdgcn_update_dpp(0LL, v, 0x111, 0xF, 0xF, false); // row_shr:1
   v += __builtin_amdgcn_update_dpp(0LL, v, 0x112, 0xF, 0xF, false); // row_shr:2
   v += __builtin_amdgcn_update_dpp(0LL, v, 0x114, 0xF, 0xF, false); // row_shr:4
   v += __builtin_amdgcn_update_dpp(0LL, v, 0x118, 0xF, 0xF, false); // row_shr:8
   v += __builtin_amdgcn_update_dpp(0LL, v, 0x142, 0xA, 0xF, false); // row_bcast:15 into rows 1 and 3
   v += __builtin_amdgcn_update_dpp(0LL, v, 0x143, 0xC, 0xF, false); // row_bcast:31 into rows 2 and 3
   const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v & 0xffffffffLL), 63); // (readlane takes 32 bits)
   const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(v >> 32), 63);
   return (long long)(((unsigned long long)hi << 32) | lo);
}
// One column: the addend v of every lane of the row split under the window E, `flag` raised when a split fails, and word(j, sum)
// called - by all lanes, with the sum over the row in each - for every word j of the column that some lane has non-zero.
template <typename WORD>
__device__ __forceinline__ void prof_fold_column(const bool mine, const double v, const int E, unsigned long long *flag, const int lane, WORD &&word)
{
   long long l[kProfWords];
   {
      long long h4[kLimbs] = {0, 0, 0, 0}, l4[kLimbs] = {0, 0, 0, 0};
      const bool added = !mine || prof_split(h4, l4, v, E);
      if (__ballot(!added) != 0 && lane == 0) { prof_max(flag, 1ULL); }
#pragma unroll
      for (int j = 0; j < kLimbs; j++) { l[j] = h4[j]; l[kLimbs + j] = l4[j]; }
   }
#pragma unroll
   for (int j = 0; j < kProfWords; j++)
   {
      if (__ballot(l[j] != 0) == 0) { continue; }
      word(j, prof_wave_sum(l[j]));
   }
}
// A lane on its own: the count, its extreme keys and the limbs of its addends, one atomic per non-zero limb.  The columns
// [SKIP_LO, SKIP_HI) hold nothing but zeros (a vector component above the dimension) and are left out.
template <int NS, int SKIP_LO, int SKIP_HI>
__device__ __forceinline__ void prof_lane_tail(const ProfScratch &s, const int row, const unsigned long long kmin, const unsigned long long kmax,
                                               const double (&ad)[NS], const int (&E)[NS])
{
   prof_add((long long *)s.count + row, 1LL);
   if (kmin != 0) { prof_max(s.rmin + row, kmin); }
   if (kmax != 0) { prof_max(s.rmax + row, kmax); }
#pragma unroll
   for (int k = 0; k < NS; k++)
   {
      if (k >= SKIP_LO && k < SKIP_HI) { continue; }
      long long h4[kLimbs] = {0, 0, 0, 0}, l4[kLimbs] = {0, 0, 0, 0};
      long long *wp = s.words + ((size_t)row * NS + k) * kProfWords;
      if (!prof_split(h4, l4, ad[k], E[k])) { prof_max(s.flags + (size_t)row * NS + k, 1ULL); continue; }
#pragma unroll
      for (int j = 0; j < kLimbs; j++)
      {
         if (h4[j] != 0) { prof_add(wp + j, h4[j]); }
         if (l4[j] != 0) { prof_add(wp + kLimbs + j, l4[j]); }
      }
   }
}
// The scatter by cell, for points whose rows are few and far apart, so that there is no range of rows to walk: while lanes
// remain (ok: this lane has a point, in `row`), the wavefront takes the row of its first remaining lane, ballots the lanes of
// that row, folds them and retires them.  The NS = 8 columns x 8 limbs of a row are 64 consecutive words, so lane l keeps the
// folded word l and the row goes out as ONE wave instruction over 512 contiguous bytes (the lanes whose word is 0 stay out).
// After `fold` distinct rows the remaining lanes send their own atomics; 0 sends everything that way.  Integer sums: the
// same bits either way.  Every lane of the wavefront must call.
template <int NS, int SKIP_LO, int SKIP_HI>
__device__ __forceinline__ void prof_scatter_cells(const ProfScratch &s, const bool ok, const int row, const unsigned long long kmin,
                                                   const unsigned long long kmax, const double (&ad)[NS], const int (&E)[NS], const int fold, const int lane)
{
   static_assert(NS * kProfWords == kWave, "one word of a row per lane");
   unsigned long long rem = __ballot(ok);
   for (int nf = 0; rem != 0 && nf < fold; nf++) // (wave-uniform)
   {
      const int r = __builtin_amdgcn_readlane(row, __ffsll((long long)rem) - 1);
      const bool mine = ok && row == r;
      const unsigned long long in_row = __ballot(mine); // (lanes of one row retire together: all of them still remain)
      prof_fold_head(s, r, in_row, mine ? kmin : 0ULL, mine ? kmax : 0ULL, lane);
      long long keep = 0; // word `lane` of the row, folded over the lanes of the row
#pragma unroll
      for (int k = 0; k < NS; k++)
      {
         if (k >= SKIP_LO && k < SKIP_HI) { continue; }
         prof_fold_column(mine, ad[k], E[k], s.flags + (size_t)r * NS + k, lane, [&](const int j, const long long sum) {
            if (lane == k * kProfWords + j) { keep = sum; }
         });
      }
      if (keep != 0) { prof_add(s.words + (size_t)r * (NS * kProfWords) + lane, keep); }
      rem &= ~in_row;
   }
   if ((rem >> lane) & 1ULL) { prof_lane_tail<NS, SKIP_LO, SKIP_HI>(s, row, kmin, kmax, ad, E); }
}

// pass 0, the end of a workgroup: the maxima mx of its threads into its shard (red: kProfRed doubles of LDS)
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
// over fewer than 2^20 ranks stay exact.  Flags, counts and the excluded points ride with the sums; the extremes go apart,
// decoded by KEY, the maximum negated: a min-reduce takes it.
template <int NS, typename KEY>
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
      rmin[i] = KEY::min_of(s.rmin[i], n);
      rmax[i] = KEY::neg_max_of(s.rmax[i], n);
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
// Scratch for at least R rows in `dev`, which holds `rows` of them: regrown only when R is larger.  A failed allocation leaves
// rows = 0 and nothing allocated.
template <int NS>
inline int prof_scratch(DevPtr<char> &dev, int &rows, const int R, ProfScratch &s)
{
   if (R > rows)
   {
      rows = 0;
      LGH_PASS(dev.alloc(prof_layout<NS>(nullptr, R).bytes));
      rows = R;
   }
   s = prof_layout<NS>(dev, rows);
   return LGH_OK;
}

// behind the scatter pass: pack, the sums and minima over the ranks, the values.  s: the layout of the allocation; R: the rows of this call
template <int NS, typename KEY>
inline int prof_finish(lgh_ctx *c, const ProfScratch &s, const int R)
{
   const bool multi = c->multi != 0 && c->comm;
   const long n_rc = (long)R * NS;
   hipLaunchKernelGGL((prof_pack_k<NS, KEY>), dim3(ceil_div(n_rc, 256)), dim3(256), 0, c->stream, s, R);
   LGH_HIP_CHECK(hipGetLastError());
   if (multi)
   {
      // (the packed rows cross the ranks in pieces of what the transport takes at a time: 8 values on the emulated ones)
      const long n_sum = n_rc * kProfPack + n_rc + R + 1;
      LGH_PASS(allreduce_dev_n(c, s.pk, n_sum, 0));
      LGH_PASS(allreduce_dev_n(c, s.pk + n_sum, 2L * R, 1));
   }
   hipLaunchKernelGGL(prof_value_k<NS>, dim3(ceil_div(R, 64)), dim3(64), 0, c->stream, s, R);
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}

// One call from the clear to the rows on the host, under timer slot `slot`: launch(pass) puts the caller's kernel of pass 0
// and of pass 1 on the stream (neither without work: an empty list).  The kernels behind index by the R rows of THIS call;
// the layout s is that of the allocation.  out: R * (NS + 3) doubles.
template <int NS, typename KEY, typename LAUNCH>
inline int prof_run(lgh_ctx *c, const ProfScratch &s, const int R, const int slot, const bool have_work, LAUNCH &&launch, double *out, long *n_excluded)
{
   {
      KtScope kt(c, slot);
      LGH_HIP_CHECK(hipMemsetAsync(s.words, 0, s.int_bytes, c->stream)); // (the words open the allocation)
      if (have_work)
      {
         launch(0);
         LGH_HIP_CHECK(hipGetLastError());
      }
      hipLaunchKernelGGL(prof_window_k<NS>, dim3(1), dim3(64), 0, c->stream, s);
      LGH_HIP_CHECK(hipGetLastError());
      if (c->multi != 0 && c->comm) { LGH_PASS(allreduce_dev_n(c, s.neg, NS, 1)); }
      if (have_work)
      {
         launch(1);
         LGH_HIP_CHECK(hipGetLastError());
      }
      LGH_PASS((prof_finish<NS, KEY>(c, s, R)));
   }
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   const size_t n_out = (size_t)R * (NS + 3);
   LGH_HIP_CHECK(hipMemcpy(out, s.out, n_out * sizeof(double), hipMemcpyDeviceToHost));
   double ex = 0.0;
   LGH_HIP_CHECK(hipMemcpy(&ex, s.out + n_out, sizeof(double), hipMemcpyDeviceToHost));
   *n_excluded = (long)ex;
   return LGH_OK;
}

} // namespace lgh
