// lgh_vcg_hooks.hip — test hooks and statistics of the lockstep velocity solve (lgh_vcg.hip): single launches of K1 and K2
// as the solve issues them, the exact accumulators of lgh_vcg.hpp on their own, the merged E-vector layout as a test
// or a byte count sees it.  They plan like the solve does (vcg_prepare) and launch its kernels through its launchers.
#include "lgh_vcg.hpp"

namespace lgh
{

__global__ void vcg_test_put_rz_k(long long *set, double v0, double v1, double v2, double s0, double s1, double s2)
{
   const double v[kVC] = {v0, v1, v2}, sc[kVC] = {s0, s1, s2};
   for (int k = 0; k < kVC; k++)
   {
      long long acc[kLimbs] = {0, 0, 0, 0};
      const bool ok = exact_add(acc, v[k], exact_scale(sc[k]));
      for (int j = 0; j < kLimbs; j++) { set[kLimbs * k + j] = acc[j]; }
      if (!ok) { set[kLimbShards * kVC * kLimbs] = 1; }
   }
}
// Test hook (lgh_test_exact_sum): the exact accumulators of lgh_vcg.hpp on their own.  The kernels below call
// exact_scale / exact_add / wave_sum_i64 / exact_value / exact_den / exact_fold / exact_fold_lanes themselves - what a
// test sees through them is what K1 and K2 compute with.
__global__ void __launch_bounds__(256)
vcg_test_exact_split_k(const double *__restrict__ v, const long n, int E, const double *__restrict__ scale, long long *__restrict__ limbs, int *__restrict__ ok)
{
   const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= n) { return; }
   if (scale) { E = exact_scale(*scale); }
   long long acc[kLimbs] = {0, 0, 0, 0};
   ok[i] = exact_add(acc, v[i], E) ? 1 : 0;
   for (int j = 0; j < kLimbs; j++) { limbs[kLimbs * i + j] = acc[j]; }
}
__global__ void __launch_bounds__(256)
vcg_test_exact_value_k(const long long *__restrict__ limbs, const long n, const int E, double *__restrict__ out)
{
   const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= n) { return; }
   long long l4[kLimbs];
   for (int j = 0; j < kLimbs; j++) { l4[j] = limbs[kLimbs * i + j]; }
   out[i] = exact_value(l4, E);
}
__global__ void __launch_bounds__(256)
vcg_test_exact_scale_k(const double *__restrict__ rz, const long n, int *__restrict__ E)
{
   const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
   if (i < n) { E[i] = exact_scale(rz[i]); }
}
// one wavefront per 64 words; every lane's result is returned
__global__ void __launch_bounds__(64)
vcg_test_wave_sum_k(const long long *__restrict__ in, long long *__restrict__ out)
{
   const long i = (long)blockIdx.x * 64 + threadIdx.x;
   out[i] = wave_sum_i64(in[i]);
}
// n addends per component (component k: v[k n + i]) over the workgroups of the grid, then what the tail of the slab K1
// does with a lane's accumulators: wave_sum_i64, LDS, one atomic per word into the workgroup's shard, the flag word
__global__ void __launch_bounds__(256)
vcg_test_exact_grid_k(const double *__restrict__ v, const long n, int E, const double *__restrict__ scale, long long *__restrict__ set)
{
   constexpr int NW = 4;
   const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
   if (scale) { E = exact_scale(*scale); }
   long long acc[kVC][kLimbs];
   for (int k = 0; k < kVC; k++) { for (int j = 0; j < kLimbs; j++) { acc[k][j] = 0; } }
   bool acc_bad = false;
   for (long i = (long)blockIdx.x * 256 + tid; i < n; i += 256L * gridDim.x)
   {
      for (int k = 0; k < kVC; k++) { acc_bad = !exact_add(acc[k], v[(long)k * n + i], E) || acc_bad; }
   }
   __shared__ long long redi[NW][kVC * kLimbs];
   __shared__ int redbad[NW];
#pragma unroll
   for (int k = 0; k < kVC; k++)
   {
#pragma unroll
      for (int j = 0; j < kLimbs; j++)
      {
         const long long tot = wave_sum_i64(acc[k][j]);
         if (lane == 0) { redi[wid][kLimbs * k + j] = tot; }
      }
   }
   const bool anybad = __any(acc_bad);
   if (lane == 0) { redbad[wid] = anybad ? 1 : 0; }
   __syncthreads();
   if (tid < kVC * kLimbs)
   {
      long long sum = 0;
      for (int w = 0; w < NW; w++) { sum += redi[w][tid]; }
      if (sum != 0) { (void)__hip_atomic_fetch_add(&set[(blockIdx.x % kLimbShards) * (kVC * kLimbs) + tid], sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
   }
   if (tid == kVC * kLimbs)
   {
      int bad = 0;
      for (int w = 0; w < NW; w++) { bad |= redbad[w]; }
      if (bad) { (void)__hip_atomic_fetch_or(&set[kLimbShards * kVC * kLimbs], 1LL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
   }
}
// the three folds of a set by one full wavefront: out[k] = exact_den, out[3 + k] = exact_fold, out[6 + k] = exact_fold_lanes
__global__ void __launch_bounds__(64)
vcg_test_exact_fold_k(const long long *__restrict__ set, int E, const double *__restrict__ scale, double rz, double *__restrict__ out)
{
   const int lane = threadIdx.x;
   if (scale) { E = exact_scale(*scale); rz = *scale; }
   const long long w = (lane <= kLimbShards * kVC * kLimbs) ? set[lane] : 0LL; // lane l holds word l
   for (int k = 0; k < kVC; k++)
   {
      const double a = exact_den(set, k, rz), b = exact_fold(set, k, E), f = exact_fold_lanes(w, k, E);
      if (lane == 0) { out[k] = a; out[3 + k] = b; out[6 + k] = f; }
   }
}
int vcg_test_exact_sum(lgh_ctx *c, int mode, long n, int G, int E, const double *scale, const double *v, const long long *w_in,
                       long long *w_out, double *d_out, int *i_out)
{
   DevPtr<char> dv, dw, dd, di, ds;
   auto up = [&](DevPtr<char> &b, const void *src, size_t bytes) -> hipError_t {
      if (b.alloc(bytes) != LGH_OK) { return hipErrorOutOfMemory; }
      return src ? hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice) : hipMemsetAsync(b.p, 0, bytes, c->stream);
   };
   if (scale) { LGH_HIP_CHECK(up(ds, scale, sizeof(double))); }
   const double *dscale = (const double *)ds.p;
   const unsigned nb = (unsigned)((n + 255) / 256);
   const size_t un = (size_t)n;
   size_t w_bytes = 0, d_bytes = 0, i_bytes = 0; // what goes back to w_out, d_out, i_out
   switch (mode)
   {
      case 0: // split
         LGH_HIP_CHECK(up(dv, v, un * sizeof(double)));
         LGH_HIP_CHECK(up(dw, nullptr, w_bytes = kLimbs * un * sizeof(long long)));
         LGH_HIP_CHECK(up(di, nullptr, i_bytes = un * sizeof(int)));
         hipLaunchKernelGGL(vcg_test_exact_split_k, dim3(nb), dim3(256), 0, c->stream, (const double *)dv.p, n, E, dscale, (long long *)dw.p, (int *)di.p);
         break;
      case 1: // value
         LGH_HIP_CHECK(up(dw, w_in, kLimbs * un * sizeof(long long)));
         LGH_HIP_CHECK(up(dd, nullptr, d_bytes = un * sizeof(double)));
         hipLaunchKernelGGL(vcg_test_exact_value_k, dim3(nb), dim3(256), 0, c->stream, (const long long *)dw.p, n, E, (double *)dd.p);
         break;
      case 2: // grid
         LGH_HIP_CHECK(up(dv, v, kVC * un * sizeof(double)));
         LGH_HIP_CHECK(up(dw, nullptr, w_bytes = kLimbWords * sizeof(long long))); // a cleared set
         LGH_HIP_CHECK(up(dd, nullptr, d_bytes = 9 * sizeof(double)));
         hipLaunchKernelGGL(vcg_test_exact_grid_k, dim3((unsigned)G), dim3(256), 0, c->stream, (const double *)dv.p, n, E, dscale, (long long *)dw.p);
         LGH_HIP_CHECK(hipGetLastError());
         hipLaunchKernelGGL(vcg_test_exact_fold_k, dim3(1), dim3(64), 0, c->stream, (const long long *)dw.p, E, dscale, ldexp(0.75, E - 12), (double *)dd.p);
         break;
      case 3: // wave
         LGH_HIP_CHECK(up(dv, w_in, un * sizeof(long long)));
         LGH_HIP_CHECK(up(dw, nullptr, w_bytes = un * sizeof(long long)));
         hipLaunchKernelGGL(vcg_test_wave_sum_k, dim3((unsigned)(n / 64)), dim3(64), 0, c->stream, (const long long *)dv.p, (long long *)dw.p);
         break;
      default: // 4: scale
         LGH_HIP_CHECK(up(dv, v, un * sizeof(double)));
         LGH_HIP_CHECK(up(di, nullptr, i_bytes = un * sizeof(int)));
         hipLaunchKernelGGL(vcg_test_exact_scale_k, dim3(nb), dim3(256), 0, c->stream, (const double *)dv.p, n, (int *)di.p);
         break;
   }
   LGH_HIP_CHECK(hipGetLastError());
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   if (w_bytes) { LGH_HIP_CHECK(hipMemcpy(w_out, dw.p, w_bytes, hipMemcpyDeviceToHost)); }
   if (d_bytes) { LGH_HIP_CHECK(hipMemcpy(d_out, dd.p, d_bytes, hipMemcpyDeviceToHost)); }
   if (i_bytes) { LGH_HIP_CHECK(hipMemcpy(i_out, di.p, i_bytes, hipMemcpyDeviceToHost)); }
   return LGH_OK;
}

// Test hooks and the merged layout: the hooks speak the element-local E-vector ([e][d] per component) on both sides.
// Out of K1: every entry from its place in the plane; the right-hand member of a merged pair reads 0.0 and the sum K1
// formed is reported in the left-hand zone's entry (lgh_test_vcg_merged_faces tells the caller which entries those are).
// Into K2: a merged place receives the sum of its two entries (what K1 would have stored there).
__global__ void __launch_bounds__(256)
vcg_unpack_merged_k(const double *__restrict__ plane, const int *__restrict__ pos, const uint8_t *__restrict__ sec, double *__restrict__ out, const size_t n)
{
   const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
   if (i < n) { out[i] = sec[i] ? 0.0 : plane[pos[i]]; }
}
__global__ void __launch_bounds__(256)
vcg_pack_merged_k(const double *__restrict__ in, const int *__restrict__ pos, const uint8_t *__restrict__ sec, const int ND, double *__restrict__ plane, const size_t n)
{
   const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= n || sec[i]) { return; }
   double v = in[i];
   const size_t j = i + (size_t)ND - 3; // same (dy, dz), dx = 0 of the next zone - the partner of a dx = 3 entry of a chain
   if ((i % 4) == 3 && j < n && sec[j] && pos[j] == pos[i]) { v += in[j]; }
   plane[pos[i]] = v;
}
struct MergedDev { DevPtr<int> pos; DevPtr<uint8_t> sec; };
static int merged_to_device(lgh_ctx *c, const VcgAux *aux, MergedDev &m)
{
   SlabLayout L;
   LGH_PASS(slab_merge_layout(c, aux, L));
   LGH_PASS(m.pos.upload(L.pos.data(), L.pos.size()));
   LGH_PASS(m.sec.upload(L.sec.data(), L.sec.size()));
   return LGH_OK;
}
// lgh_test_vcg_merged_faces: mask[e * ND + d] = 1 where K1 of this context has already summed the entry into its left
// neighbour's (all zero when the layout is element-local: every other form of K1, LGH_SLAB_MERGE=0)
int vcg_test_merged_faces(lgh_ctx *c, unsigned char *mask, long *n_merged)
{
   const size_t nE = (size_t)c->NE * c->ND;
   memset(mask, 0, nE);
   *n_merged = 0;
   if (!vcg_available(c)) { return LGH_OK; }
   VcgPlan plan;
   LGH_PASS(vcg_prepare(c, nullptr, nullptr, 0.0, plan));
   if (!plan.a.settab) { return LGH_OK; }
   SlabLayout L;
   LGH_PASS(slab_merge_layout(c, plan.aux, L));
   // (the layout is that of the order the solve runs in; the caller's E-vector is in the caller's zone order)
   const MeshOrder *ord = plan.aux->ord;
   if (ord)
   {
      const size_t ND = (size_t)c->ND;
      for (size_t i = 0; i < (size_t)c->NE; i++) { memcpy(mask + (size_t)ord->zorder[i] * ND, L.sec.data() + i * ND, ND); }
   }
   else { memcpy(mask, L.sec.data(), nE); }
   *n_merged = (long)L.n_merged;
   return LGH_OK;
}

// lgh_vcg_layout_stats: what K1 hands to K2 in this context, for byte accounting (bench.py's moved_bytes): out[0] = doubles
// per component plane K1 writes and K2 reads (NE * ND element-local; less with the merged layout), out[1] = bytes of the
// ELL table K2 always reads (slots 0..3: 16 per node), out[2] = bytes of its second table (slots 4..7) in the 64-node
// blocks that hold a node with more than four contributions (what the wavefronts of K2 fetch of it, to the granularity
// of a wavefront), out[3] = E-vector entries K1 has summed into a neighbour's (0: element-local layout)
int vcg_layout_stats(lgh_ctx *c, long out[4])
{
   out[0] = (long)c->NE * c->ND; out[1] = 16L * c->N; out[2] = 16L * c->N; out[3] = 0;
   if (!vcg_available(c)) { return LGH_OK; }
   VcgPlan plan;
   LGH_PASS(vcg_prepare(c, nullptr, nullptr, 0.0, plan));
   const VcgArgs &a = plan.a;
   if (a.settab)
   {
      SlabLayout L;
      LGH_PASS(slab_merge_layout(c, plan.aux, L));
      long used = 0;
      for (size_t i = 0; i < L.pos.size(); i++) { used = std::max(used, (long)L.pos[i] + 1); }
      out[0] = used;
      out[3] = (long)L.n_merged;
   }
   const size_t N = (size_t)c->N;
   if (a.deg > 4)
   {
      std::vector<int> row((size_t)(a.deg - 4) * N);
      LGH_HIP_CHECK(hipMemcpy(row.data(), a.ell + 4 * N, row.size() * sizeof(int), hipMemcpyDeviceToHost));
      long blocks = 0;
      for (size_t b = 0; b < N; b += 64)
      {
         bool any = false;
         for (size_t n = b; n < std::min(N, b + 64) && !any; n++) { any = row[n] >= 0; } // (rows hold their contributions first: slot 4 tells)
         blocks += any ? 1 : 0;
      }
      out[2] = 16L * 64 * blocks;
   }
   else { out[2] = 0; }
   return LGH_OK;
}

// Test hook (lgh_test_vcg_k1): ONE launch of K1, in whichever form vcg_solve dispatches for this context, exactly as
// the solve would launch it in its first iteration (first != 0: d = r/diag) or in a later one (d = r/diag + beta d_old
// with beta = rz / rz_prev), on the caller's vectors.  Returns what K1 hands to K2: the element contributions
// A_e d_e of the three components as E-vectors (kVC planes of NE*ND, element-local lexicographic) and (d, A d).
// Single rank.  The vectors of the lockstep solve (r, d) are overwritten; nothing else of the context changes.
int vcg_test_k1(lgh_ctx *c, const double *r, const double *d_old, const double rz[3], const double rz_prev[3],
                int first, double *YE_out, double den_out[3])
{
   if (!vcg_available(c)) { set_error("lgh_test_vcg_k1: no lockstep solve for kernel 0x%x", c->kid); return LGH_ERR_UNSUPPORTED; }
   if (c->multi != 0) { set_error("lgh_test_vcg_k1: single rank only"); return LGH_ERR_ARG; }
   VcgPlan plan;
   LGH_PASS(vcg_prepare(c, nullptr, nullptr, 0.0, plan));
   VcgArgs &a = plan.a;
   const size_t N = (size_t)c->N, nE = (size_t)c->NE * c->ND;
   VcgScalars *ds = (VcgScalars *)c->vcg_s;
   const MeshOrder *ord = plan.aux->ord; // (the solve's own order: the caller's vectors and E-vector go through the permutation)
   if (ord) { LGH_PASS(order_gather_nodes(c, r, a.r, kVC)); }
   else { LGH_HIP_CHECK(hipMemcpyAsync(a.r, r, kVC * N * sizeof(double), hipMemcpyDeviceToDevice, c->stream)); }
   if (first) { LGH_HIP_CHECK(hipMemsetAsync(a.d, 0, kVC * N * sizeof(double), c->stream)); }
   else if (ord) { LGH_PASS(order_gather_nodes(c, d_old, a.d, kVC)); }
   else { LGH_HIP_CHECK(hipMemcpyAsync(a.d, d_old, kVC * N * sizeof(double), hipMemcpyDeviceToDevice, c->stream)); }
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream)); // (vcg_set_tol_k has cleared the accumulators and the set counters)
   VcgScalars h;
   memset(&h, 0, sizeof(h));
   for (int k = 0; k < kVC; k++) { h.rz[k] = rz[k]; h.rz_prev[k] = rz_prev[k]; }
   h.first = first ? 1 : 0;
   if (a.rzl && !first)
   {
      // rz_limbs mode: the second iteration takes (r, z) of the first out of set 1 of the exact accumulators and the
      // one before (which also fixes the scale of that set) out of the scalars
      for (int k = 0; k < kVC; k++) { h.rzh[0][k] = rz_prev[k]; }
   }
   LGH_HIP_CHECK(hipMemcpy(ds, &h, sizeof(h), hipMemcpyHostToDevice));
   if (a.rzl && !first)
   {
      hipLaunchKernelGGL(vcg_test_put_rz_k, dim3(1), dim3(1), 0, c->stream, a.rzl + 1 * kLimbWords, rz[0], rz[1], rz[2], rz_prev[0], rz_prev[1], rz_prev[2]);
      LGH_HIP_CHECK(hipGetLastError());
   }
   a.iter = first ? 1 : 2;
   a.partials = c->vcg_partials + (size_t)kVC * c->vcg_stride;
   a.ticket = c->vcg_tickets + kTicketSlot;
   vcg_launch_k1(c, plan, a);
   LGH_HIP_CHECK(hipGetLastError());
   // (slab form with deferred fold: K2 would form den from the accumulators - the one-workgroup fold of the several-rank path does the same)
   if (a.den_limbs) { vcg_launch_fold_den(c, a); }
   LGH_HIP_CHECK(hipGetLastError());
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   LGH_HIP_CHECK(hipMemcpy(&h, ds, sizeof(h), hipMemcpyDeviceToHost));
   MergedDev md;
   if (a.settab) { LGH_PASS(merged_to_device(c, plan.aux, md)); }
   DevPtr<double> tmp; // (internal order: a plane in the solve's zone order on its way to the caller's)
   if (ord) { LGH_PASS(tmp.alloc(nE)); }
   for (int k = 0; k < kVC; k++)
   {
      den_out[k] = h.den[k];
      double *dst = ord ? tmp.p : YE_out + (size_t)k * nE;
      if (a.settab)
      {
         hipLaunchKernelGGL(vcg_unpack_merged_k, dim3((unsigned)((nE + 255) / 256)), dim3(256), 0, c->stream, a.YE + (size_t)k * a.ye_stride, md.pos, md.sec, dst, nE);
         LGH_HIP_CHECK(hipGetLastError());
      }
      else { LGH_HIP_CHECK(hipMemcpyAsync(dst, a.YE + (size_t)k * a.ye_stride, nE * sizeof(double), hipMemcpyDeviceToDevice, c->stream)); }
      if (ord) { LGH_PASS(order_zone_blocks(c, tmp.p, YE_out + (size_t)k * nE, c->ND, true)); }
   }
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   return LGH_OK;
}

// Test hook (lgh_test_vcg_k2): ONE launch of K2 - the node kernel of the lockstep solve, the largest kernel of the
// step - as the one-rank solve issues it in iteration `it` (1: first, beta = 0; even: the launch that also updates x
// with the terms of two iterations; odd > 1: x untouched), on the caller's vectors: the E-vector K1 would have
// written (kVC planes of NE * ND), r, the old direction d and x (kVC * N each, updated in place), the scalars K1 and
// the iteration before leave: (d, A d), (r, z) after iterations it-1 and it-2, alpha of iteration it-1.  Returns
// (r, z) of the new residual as the solve would see it (ticketed fold, or the exact accumulators folded as the next
// K1 does).  One rank only.
int vcg_test_k2(lgh_ctx *c, int it, const double *YE_in, double *r, double *d, double *x, const double den[3],
                const double rz[3], const double rz_prev[3], const double alpha_prev[3], double rz_out[3], int *deferred_x)
{
   if (!vcg_available(c)) { set_error("lgh_test_vcg_k2: no lockstep solve for kernel 0x%x", c->kid); return LGH_ERR_UNSUPPORTED; }
   if (c->multi != 0 || it < 1) { set_error("lgh_test_vcg_k2: single rank, it >= 1"); return LGH_ERR_ARG; }
   VcgPlan plan;
   LGH_PASS(vcg_prepare(c, nullptr, x, 0.0, plan));
   VcgArgs &a = plan.a;
   const size_t N = (size_t)c->N, nE = (size_t)c->NE * c->ND;
   VcgScalars *ds = (VcgScalars *)c->vcg_s;
   const MeshOrder *ord = plan.aux->ord; // (the solve's own order: the caller's vectors and E-vector go through the permutation)
   if (ord)
   {
      LGH_PASS(order_gather_nodes(c, r, a.r, kVC));
      LGH_PASS(order_gather_nodes(c, d, a.d, kVC));
      LGH_PASS(order_gather_nodes(c, x, a.x, kVC));
   }
   else
   {
      LGH_HIP_CHECK(hipMemcpyAsync(a.r, r, kVC * N * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
      LGH_HIP_CHECK(hipMemcpyAsync(a.d, d, kVC * N * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
   }
   MergedDev md;
   if (a.settab) { LGH_PASS(merged_to_device(c, plan.aux, md)); }
   DevPtr<double> tmp;
   if (ord) { LGH_PASS(tmp.alloc(nE)); }
   for (int k = 0; k < kVC; k++)
   {
      const double *src = YE_in + (size_t)k * nE;
      if (ord) { LGH_PASS(order_zone_blocks(c, src, tmp.p, c->ND, false)); src = tmp.p; }
      if (a.settab)
      {
         hipLaunchKernelGGL(vcg_pack_merged_k, dim3((unsigned)((nE + 255) / 256)), dim3(256), 0, c->stream, src, md.pos, md.sec, c->ND, a.YE + (size_t)k * a.ye_stride, nE);
         LGH_HIP_CHECK(hipGetLastError());
      }
      else { LGH_HIP_CHECK(hipMemcpyAsync(a.YE + (size_t)k * a.ye_stride, src, nE * sizeof(double), hipMemcpyDeviceToDevice, c->stream)); }
   }
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream)); // (vcg_set_tol_k has cleared the accumulators)
   VcgScalars h;
   memset(&h, 0, sizeof(h));
   for (int k = 0; k < kVC; k++)
   {
      h.rz[k] = rz[k];
      h.rz_prev[k] = rz_prev[k];
      h.den[k] = den[k];
      h.alpha_last[k] = alpha_prev[k];
      h.rzh[(it - 1) & 1][k] = rz[k];
      h.rzh[it & 1][k] = rz_prev[k];
      h.alpha_hist[(it - 1) & 1][k] = alpha_prev[k];
      h.nupd[k] = it - 1;
   }
   h.first = (it == 1) ? 1 : 0;
   LGH_HIP_CHECK(hipMemcpy(ds, &h, sizeof(h), hipMemcpyHostToDevice));
   a.den_limbs = 0; // (d, A d) comes from the scalars here - the accumulators K1 fills are its own test's subject
   *deferred_x = plan.mode.k2p ? 1 : 0;
   a.iter = it;
   a.partials = c->vcg_partials;
   a.ticket = c->vcg_tickets;
   if (plan.mode.k2p) { vcg_launch_k2p(c, plan, a, it); }
   else if (plan.mode.direct) { vcg_launch_update(c, a, true); }
   else { set_error("lgh_test_vcg_k2: unusual valence (the unfused gather runs in the solve)"); return LGH_ERR_UNSUPPORTED; }
   LGH_HIP_CHECK(hipGetLastError());
   if (a.rzl && plan.mode.k2p) { vcg_launch_rz_finish(c, a, it, nullptr, nullptr, 0ull); }
   LGH_HIP_CHECK(hipGetLastError());
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   LGH_HIP_CHECK(hipMemcpy(&h, ds, sizeof(h), hipMemcpyDeviceToHost));
   for (int k = 0; k < kVC; k++) { rz_out[k] = (a.rzl && plan.mode.k2p) ? h.rzh[it & 1][k] : h.rz[k]; }
   if (ord)
   {
      LGH_PASS(order_scatter_nodes(c, a.r, r, kVC));
      LGH_PASS(order_scatter_nodes(c, a.d, d, kVC));
      LGH_PASS(order_scatter_nodes(c, a.x, x, kVC));
      LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
      return LGH_OK;
   }
   LGH_HIP_CHECK(hipMemcpy(r, a.r, kVC * N * sizeof(double), hipMemcpyDeviceToDevice));
   LGH_HIP_CHECK(hipMemcpy(d, a.d, kVC * N * sizeof(double), hipMemcpyDeviceToDevice));
   return LGH_OK;
}

} // namespace lgh
