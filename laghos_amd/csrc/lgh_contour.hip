// lgh_contour.hip — contours of a lattice scalar: marching tetrahedra (3D) / marching triangles (2D) over the volume lattice of
// lgh_sample_fields, with a deterministic two-pass compaction.  The definition is in include/laghos_hip.h (lgh_contour).
//
// An iso-surface needs no search through the moving mesh: the lattice is zone-local, a plane n.x = d is the contour of the
// lattice scalar n.x (lgh_contour_scalar), and every other array is interpolated along the crossed lattice edges afterwards
// (lgh_contour_gather).
//
// Shape: 256 threads; ZPB consecutive zones per workgroup, their scalar values staged in LDS (ZPB R1^dim doubles, at most
// 8 KB).  A work item is one simplex, numbered (zone, sub-cell, simplex) ascending - the order of the output - and the
// workgroup runs over its items 256 at a time.  An item yields 0, 1 or 2 primitives; its place among the workgroup's is
//   the primitives of the rounds before (a running count every thread keeps)
//   + those of the wavefronts before it in the round (four totals through LDS)
//   + those of the lanes before it in its wavefront (two ballots - "at least one", "two" - and population counts).
// The count pass stores the workgroup's totals; one workgroup scans them; the emit pass recomputes the cases and writes at
// its offset.  No atomic decides a position, so the output is a function of the input alone, whatever the grid.  Consecutive
// lanes write consecutive records.  Reads `scalar`; writes its outputs and the scan scratch of the context.  Off the timed path.
#include "lgh_common.hpp"

#include <climits>

namespace lgh
{

constexpr int kContourThreads = 256;
constexpr int kContourWaves = kContourThreads / kWave;
constexpr int kContourStage = 1024; // doubles of scalar values a workgroup stages where a zone has fewer
constexpr int kContourMaxZpb = 16;

// The cases, from the rules of the header.  Corners 0..dim of a simplex in path order; bit i of the case: corner i inside.
// A word: the number of primitives in bits 24-25, and vertex j of primitive q in the nibble q * dim + j as (lower corner) |
// (upper corner) << 2 - the crossed edge, lower lattice index first (lattice indices ascend along the path).
//   one inside corner a, outside o1 < o2 (< o3):  (a o1, a o2 (, a o3));   one outside corner o: (i1 o, i2 o (, i3 o));
//   3D, inside a < b, outside c < d:              (ac, ad, bd), (ac, bd, bc);
//   the last two vertices are swapped where that order has the other sense (3D: the normal from inside to outside by the
//   right-hand rule; 2D: the inside to the left).  The path of an odd permutation of the axes is the mirror image of the path
//   of an even one, so its sense is the other one in every case: row [1] is row [0] with the swap the other way round.
//   Simplices k = 0, 3, 4 (3D) and k = 0 (2D) are even permutations.
__constant__ unsigned kCaseTet[2][16] = {
   {0x0000000, 0x1000c84, 0x10009d4, 0x29d8dc8, 0x1000e98, 0x2e94ce4, 0x28e4ed4, 0x1000edc, 0x1000dec, 0x2de4e84, 0x2ec49e4, 0x10009e8, 0x2cd8d98,
    0x1000d94, 0x10008c4, 0x0000000},
   {0x0000000, 0x10008c4, 0x1000d94, 0x2d98cd8, 0x10009e8, 0x29e4ec4, 0x2e84de4, 0x1000dec, 0x1000edc, 0x2ed48e4, 0x2ce4e94, 0x1000e98, 0x2dc89d8,
    0x10009d4, 0x1000c84, 0x0000000}};
__constant__ unsigned kCaseTri[2][8] = {{0x0000000, 0x1000084, 0x1000049, 0x1000089, 0x1000098, 0x1000094, 0x1000048, 0x0000000},
                                        {0x0000000, 0x1000048, 0x1000094, 0x1000098, 0x1000089, 0x1000049, 0x1000084, 0x0000000}};

struct ContourArgs
{
   const double *s;            // the lattice scalar
   double iso;
   long long *count, *skip;    // per workgroup: primitives, skipped simplices (count pass)
   const long long *offset;    // per workgroup: primitives of the workgroups before it (emit pass)
   int *edges;
   double *t;
   int *zone;
   int NE, R1, ZPB;
};

// corner c of a simplex on the zone's lattice, from its corner 0: the strides of the path's axes, one more per step
__device__ __forceinline__ int corner_offset(const int c, const int sa, const int sb, const int sc)
{
   return ((c >= 1) ? sa : 0) + ((c >= 2) ? sb : 0) + ((c >= 3) ? sc : 0);
}

template <int DIM, bool EMIT>
__global__ void __launch_bounds__(kContourThreads) contour_k(const ContourArgs a)
{
   extern __shared__ double sv[];
   __shared__ int wtot[2][kContourWaves];
   const int R1 = a.R1, C = R1 - 1, t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
   const int NPZ = (DIM == 3) ? R1 * R1 * R1 : R1 * R1, NSC = (DIM == 3) ? C * C * C : C * C;
   constexpr int NS = (DIM == 3) ? 6 : 2; // simplices of a sub-cell
   const long e0 = (long)blockIdx.x * a.ZPB;
   const int nz = (int)min((long)a.ZPB, (long)a.NE - e0); // zones of this workgroup (the last one may hold fewer)
   const double *src = a.s + (size_t)e0 * NPZ;
   for (int i = t; i < nz * NPZ; i += kContourThreads) { sv[i] = src[i]; }
   __syncthreads();
   const int nitems = nz * NSC * NS;
   const double iso = a.iso;
   long long run = EMIT ? a.offset[blockIdx.x] : 0, nskip = 0;
   for (int i0 = 0; i0 < nitems; i0 += kContourThreads)
   {
      const int i = i0 + t;
      unsigned word = 0;
      int skipped = 0, z = 0, loc0 = 0, sa = 0, sb = 0, sc3 = 0;
      if (i < nitems)
      {
         const int k = i % NS, zs = i / NS, sc = zs % NSC;
         z = zs / NSC;
         const int cx = sc % C, cy = (sc / C) % C, cz = sc / (C * C);
         // the path of the k-th permutation (lexicographic) of the axes, as strides on the zone's lattice
         const int st0 = 1, st1 = R1, st2 = R1 * R1;
         int pa, pb, odd;
         if constexpr (DIM == 3)
         {
            pa = k >> 1;
            const int rest0 = (pa == 0) ? 1 : 0, rest1 = (pa == 2) ? 1 : 2; // the two other axes, ascending
            pb = (k & 1) ? rest1 : rest0;
            odd = (k == 1 || k == 2 || k == 5) ? 1 : 0;
         }
         else { pa = k; pb = 1 - k; odd = k; }
         sa = (pa == 0) ? st0 : ((pa == 1) ? st1 : st2);
         sb = (pb == 0) ? st0 : ((pb == 1) ? st1 : st2);
         sc3 = st0 + st1 + st2 - sa - sb; // (3D: the stride of the last axis of the path)
         loc0 = z * NPZ + cx + R1 * (cy + R1 * cz);
         int mask = 0, fin = 1;
#pragma unroll
         for (int c = 0; c <= DIM; c++)
         {
            const double vc = sv[loc0 + corner_offset(c, sa, sb, sc3)];
            fin &= (__builtin_fabs(vc) <= 1.79769313486231570815e308) ? 1 : 0; // (false for NaN and the infinities)
            mask |= (vc >= iso) ? (1 << c) : 0;
         }
         skipped = 1 - fin;
         if (fin) { word = (DIM == 3) ? kCaseTet[odd][mask] : kCaseTri[odd][mask]; }
      }
      const int np = (int)(word >> 24);
      const unsigned long long b1 = __ballot(np >= 1), b2 = __ballot(np == 2), bs = __ballot(skipped);
      const unsigned long long below = (1ull << lane) - 1ull;
      const int pre = __popcll(b1 & below) + __popcll(b2 & below);
      if (lane == 0)
      {
         wtot[0][wave] = __popcll(b1) + __popcll(b2);
         wtot[1][wave] = __popcll(bs);
      }
      __syncthreads();
      int before = 0, all = 0, allskip = 0;
#pragma unroll
      for (int w = 0; w < kContourWaves; w++)
      {
         before += (w < wave) ? wtot[0][w] : 0;
         all += wtot[0][w];
         allskip += wtot[1][w];
      }
      if constexpr (EMIT)
      {
         const long long at = run + before + pre;
         const long pbase = (long)e0 * NPZ; // (NP fits an int: the host refuses otherwise)
#pragma unroll
         for (int q = 0; q < ((DIM == 3) ? 2 : 1); q++)
         {
            if (q >= np) { break; }
            int *eo = a.edges + (size_t)(at + q) * (2 * DIM);
            double *to = a.t + (size_t)(at + q) * DIM;
#pragma unroll
            for (int j = 0; j < DIM; j++)
            {
               const unsigned nib = (word >> (4 * (q * DIM + j))) & 0xFu;
               const int c0 = (int)(nib & 3u), c1 = (int)(nib >> 2);
               const int l0 = loc0 + corner_offset(c0, sa, sb, sc3), l1 = loc0 + corner_offset(c1, sa, sb, sc3);
               const double s0 = sv[l0], s1 = sv[l1];
               eo[2 * j] = (int)(pbase + l0);
               eo[2 * j + 1] = (int)(pbase + l1);
               to[j] = (iso - s0) / (s1 - s0);
            }
            if (a.zone) { a.zone[at + q] = (int)(e0 + z); }
         }
      }
      run += all;
      nskip += allskip;
      __syncthreads(); // the totals are rewritten in the next round
   }
   if constexpr (!EMIT)
   {
      if (t == 0)
      {
         a.count[blockIdx.x] = run;
         a.skip[blockIdx.x] = nskip;
      }
   }
}

// offset[b] = count[0] + ... + count[b-1]; offset[n] the total, offset[n + 1] the sum of skip.  One workgroup, fixed shape.
__global__ void __launch_bounds__(kContourThreads) contour_scan_k(const long long *count, const long long *skip, long long *offset, const int n)
{
   __shared__ long long sc[2][kContourThreads];
   const int t = threadIdx.x;
   long long run = 0, nskip = 0;
   for (int b0 = 0; b0 < n; b0 += kContourThreads)
   {
      const int b = b0 + t;
      const long long mine = (b < n) ? count[b] : 0;
      sc[0][t] = mine;
      sc[1][t] = (b < n) ? skip[b] : 0;
      __syncthreads();
      for (int d = 1; d < kContourThreads; d <<= 1) // inclusive scan, both rows
      {
         const long long x0 = (t >= d) ? sc[0][t - d] : 0, x1 = (t >= d) ? sc[1][t - d] : 0;
         __syncthreads();
         sc[0][t] += x0;
         sc[1][t] += x1;
         __syncthreads();
      }
      if (b < n) { offset[b] = run + sc[0][t] - mine; }
      run += sc[0][kContourThreads - 1];
      nskip += sc[1][kContourThreads - 1];
      __syncthreads();
   }
   if (t == 0)
   {
      offset[n] = run;
      offset[n + 1] = nskip;
   }
}

__global__ void __launch_bounds__(256) contour_gather_k(const long nv, const int *__restrict__ edges, const double *__restrict__ t, const int ncomp,
                                                        const size_t NP, const double *__restrict__ field, double *__restrict__ out)
{
   for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < nv; k += (long)gridDim.x * blockDim.x)
   {
      const int p0 = edges[2 * k], p1 = edges[2 * k + 1];
      const double w = t[k];
      for (int c = 0; c < ncomp; c++)
      {
         const double x = field[c * NP + p0], y = field[c * NP + p1];
         out[(size_t)c * nv + k] = x + w * (y - x);
      }
   }
}

__global__ void __launch_bounds__(256) contour_scalar_k(const int mode, const size_t NP, const int dim, const double *__restrict__ in, const double c0,
                                                        const double c1, const double c2, double *__restrict__ out)
{
   for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < NP; p += (size_t)gridDim.x * blockDim.x)
   {
      const double x = in[p], y = in[NP + p], z = (dim == 3) ? in[2 * NP + p] : 0.0;
      double r;
      if (mode == 0)
      {
         r = c0 * x + c1 * y;
         if (dim == 3) { r = r + c2 * z; }
      }
      else
      {
         r = x * x + y * y;
         if (dim == 3) { r = r + z * z; }
         r = sqrt(r);
      }
      out[p] = r;
   }
}

static int contour_zpb(const int dim, const int R1) { return std::max(1, std::min(kContourMaxZpb, kContourStage / ipow(R1, dim))); }

static int contour_refuses(const lgh_ctx *c, const char *who, const int R1)
{
   if (c->dim == 1)
   {
      set_error("%s: dim = 1: contours are formed in 2D and 3D", who);
      return LGH_ERR_ARG;
   }
   if (R1 < 2 || R1 > 9)
   {
      set_error("%s: R1 = %d lattice points per direction is out of range (2 <= R1 <= 9)", who, R1);
      return LGH_ERR_ARG;
   }
   return LGH_OK;
}

} // namespace lgh

using namespace lgh;

extern "C"
{

int lgh_contour_zpb(lgh_ctx *c, int R1, int *zpb)
{
   LGH_CHECK_ARG(c && zpb);
   LGH_PASS(contour_refuses(c, "lgh_contour_zpb", R1));
   *zpb = contour_zpb(c->dim, R1);
   return LGH_OK;
}

int lgh_contour(lgh_ctx *c, int R1, const double *scalar, double iso, long capacity, int *edges_out, double *t_out, int *zone_out, long *n_prims,
                long *n_skipped)
{
   LGH_CHECK_ARG(c && n_prims && n_skipped);
   LGH_PASS(contour_refuses(c, "lgh_contour", R1));
   if (!scalar)
   {
      set_error("lgh_contour: scalar is NULL");
      return LGH_ERR_ARG;
   }
   if (capacity < 0 || (capacity > 0 && (!edges_out || !t_out)))
   {
      set_error("lgh_contour: capacity = %ld with %s", capacity, capacity < 0 ? "no meaning" : (!edges_out ? "edges_out NULL" : "t_out NULL"));
      return LGH_ERR_ARG;
   }
   const int dim = c->dim, NPZ = ipow(R1, dim);
   if ((size_t)c->NE * NPZ > (size_t)INT_MAX)
   {
      set_error("lgh_contour: %zu lattice points do not fit the 32-bit indices of edges_out", (size_t)c->NE * NPZ);
      return LGH_ERR_UNSUPPORTED;
   }
   const int ZPB = contour_zpb(dim, R1), grid = ceil_div(c->NE, ZPB);
   if (grid > c->contour_cap)
   {
      LGH_HIP_CHECK(hipStreamSynchronize(c->stream)); // (a kernel of an earlier call may still read the buffer)
      LGH_PASS(c->contour_dev.alloc(3 * (size_t)grid + 2));
      c->contour_cap = grid;
   }
   ContourArgs a;
   memset(&a, 0, sizeof(a));
   a.s = scalar; a.iso = iso;
   a.count = c->contour_dev; a.skip = a.count + grid; a.offset = a.skip + grid;
   a.NE = c->NE; a.R1 = R1; a.ZPB = ZPB;
   const size_t lds = (size_t)ZPB * NPZ * sizeof(double);
   long long totals[2] = {0, 0};
   KtScope kt(c, LGH_KERNEL_CONTOUR);
   if (dim == 3) { hipLaunchKernelGGL((contour_k<3, false>), dim3(grid), dim3(kContourThreads), lds, c->stream, a); }
   else { hipLaunchKernelGGL((contour_k<2, false>), dim3(grid), dim3(kContourThreads), lds, c->stream, a); }
   LGH_HIP_CHECK(hipGetLastError());
   hipLaunchKernelGGL(contour_scan_k, dim3(1), dim3(kContourThreads), 0, c->stream, a.count, a.skip, a.skip + grid, grid);
   LGH_HIP_CHECK(hipGetLastError());
   LGH_HIP_CHECK(hipMemcpyAsync(totals, a.offset + grid, sizeof(totals), hipMemcpyDeviceToHost, c->stream));
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   *n_prims = (long)totals[0];
   *n_skipped = (long)totals[1];
   if (totals[0] == 0 || totals[0] > capacity) { return LGH_OK; } // (nothing is written: the caller sizes the buffers and calls again)
   a.edges = edges_out; a.t = t_out; a.zone = zone_out;
   if (dim == 3) { hipLaunchKernelGGL((contour_k<3, true>), dim3(grid), dim3(kContourThreads), lds, c->stream, a); }
   else { hipLaunchKernelGGL((contour_k<2, true>), dim3(grid), dim3(kContourThreads), lds, c->stream, a); }
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}

int lgh_contour_gather(lgh_ctx *c, long n_verts, const int *edges, const double *t, int ncomp, long NP, const double *field, double *out)
{
   LGH_CHECK_ARG(c && n_verts >= 0 && ncomp >= 0 && NP >= 0);
   if (n_verts == 0 || ncomp == 0) { return LGH_OK; }
   LGH_CHECK_ARG(edges && t && field && out);
   const unsigned grid = (unsigned)std::min<long>(ceil_div(n_verts, 256L), 4096L);
   hipLaunchKernelGGL(contour_gather_k, dim3(grid), dim3(256), 0, c->stream, n_verts, edges, t, ncomp, (size_t)NP, field, out);
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}

int lgh_contour_scalar(lgh_ctx *c, int mode, long NP, int dim, const double *in, const double coef[4], double *out)
{
   LGH_CHECK_ARG(c && in && out && NP >= 0 && (mode == 0 || mode == 1) && (dim == 2 || dim == 3) && (mode == 1 || coef));
   if (NP == 0) { return LGH_OK; }
   const unsigned grid = (unsigned)std::min<long>(ceil_div(NP, 256L), 4096L);
   hipLaunchKernelGGL(contour_scalar_k, dim3(grid), dim3(256), 0, c->stream, mode, (size_t)NP, dim, in, coef ? coef[0] : 0.0, coef ? coef[1] : 0.0,
                      coef ? coef[2] : 0.0, out);
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}
}
