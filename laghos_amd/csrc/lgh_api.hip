// lgh_api.hip — C ABI of liblaghos_hip.so: context life cycle, vector helpers,
// timers, and the operator-level entry points declared in include/laghos_hip.h
// (SolveEnergy and its entry points: lgh_energy.hip).
#include <cstdarg>
#include <cstdlib>
#include <cmath>
#include <algorithm>
#include <limits>

#include "lgh_comm_transport.hpp"
#include "lgh_vcg.hpp"

#include <atomic>
#include <chrono>
#include <dlfcn.h>

namespace lgh
{

static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...)
{
   va_list ap;
   va_start(ap, fmt);
   vsnprintf(g_err, sizeof(g_err), fmt, ap);
   va_end(ap);
}

// ---- small vector kernels ------------------------------------------------------
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
// qdata.dt_est = v: the estimate itself and, behind it, the partial minima the row-form update folds its candidates into
__global__ void __launch_bounds__(256) dt_est_set_k(double *p, double v)
{
   if (threadIdx.x == 0)
   {
      p[0] = v;
      p[kDtHint] = (v >= 0.0) ? fabs(v) : __builtin_inf(); // (the hint is compared as an unsigned bit pattern: +0.0 and up; anything else is "no hint")
   }
   for (int s = threadIdx.x; s < kDtSlots; s += blockDim.x) { p[kDtSlotStride * (1 + s)] = __builtin_inf(); }
}
// ... and the fold in front of every read: estimate = min(estimate, partial minima) in a fixed tree (a minimum does not
// depend on the order anyway); the slots go back to +inf
// host_out (pinned host memory as the device sees it): [0] the estimate, [1] the error word `err` - the host reads them
// after the stream synchronisation it needs anyway, without two copy kernels in front of it
__global__ void __launch_bounds__(256) dt_est_fold_k(double *p, const int *err, double *host_out, const unsigned long long token)
{
   __shared__ double red[16];
   double m = __builtin_inf();
   for (int s = threadIdx.x; s < kDtSlots; s += blockDim.x)
   {
      m = fmin(m, p[kDtSlotStride * (1 + s)]);
      p[kDtSlotStride * (1 + s)] = __builtin_inf();
   }
   m = block_min(m, red);
   if (threadIdx.x == 0)
   {
      const double est = fmin(p[0], m);
      p[0] = est;
      p[kDtHint] = __builtin_inf(); // (the hint word goes back with the slots it summarised)
      host_out[0] = est;
      ((int *)(host_out + 1))[0] = *err;
      __threadfence_system();
      __hip_atomic_store((unsigned long long *)(host_out + 2), token, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); // (host_wait_token)
   }
}

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
   int rc = vec_axpby(c, z1, a1, x1, b1, y, n);
   if (rc) { return rc; }
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

// ---- timers: HIP events around the reference's stopwatch regions -----------------
void timer_start(lgh_ctx *c)
{
   if (!c->timers.enabled) { return; }
   (void)hipEventRecord(c->timers.ev[0], c->stream);
}
void timer_stop(lgh_ctx *c, int which)
{
   if (!c->timers.enabled) { return; }
   (void)hipEventRecord(c->timers.ev[1], c->stream);
   (void)hipEventSynchronize(c->timers.ev[1]);
   float ms = 0.f;
   (void)hipEventElapsedTime(&ms, c->timers.ev[0], c->timers.ev[1]);
   c->timers.t[which] += 1e-3 * ms;
}

// ---- roctx ranges (LGH_ROCTX=1): the library is loaded by the first context created with the switch, for the process
namespace
{
struct Roctx
{
   int (*push)(const char *) = nullptr;
   int (*pop)() = nullptr;
   Roctx()
   {
      void *h = nullptr;
      for (const char *n : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"})
      {
         h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
         if (h) { break; }
      }
      if (!h) { return; }
      push = (int (*)(const char *))dlsym(h, "roctxRangePushA");
      pop = (int (*)())dlsym(h, "roctxRangePop");
      if (!push || !pop) { push = nullptr; pop = nullptr; }
   }
};
std::atomic<const Roctx *> g_roctx{nullptr};
void roctx_enable()
{
   static const Roctx r;
   g_roctx.store(&r);
}

// ---- the environment switches (lgh_common.hpp Switches): the one place that reads them
// a flag: '0...' is 0, '1...' is 1, anything else (and no variable) is `unset`
int env_flag(const char *name, const int unset)
{
   const char *e = getenv(name);
   return (e && (e[0] == '0' || e[0] == '1')) ? e[0] - '0' : unset;
}
// a number; a variable that does not start with one counts as not set
long env_long(const char *name, const long unset)
{
   const char *e = getenv(name);
   char *end = nullptr;
   const long v = e ? strtol(e, &end, 10) : 0;
   return (e && end != e) ? v : unset;
}
double env_double(const char *name, const double unset)
{
   const char *e = getenv(name);
   char *end = nullptr;
   const double v = e ? strtod(e, &end) : 0.0;
   return (e && end != e) ? v : unset;
}
std::string env_string(const char *name)
{
   const char *e = getenv(name);
   return e ? e : "";
}
} // namespace
RoctxRange::RoctxRange(const char *name) : on(false)
{
   const Roctx *r = g_roctx.load();
   on = r && r->push != nullptr;
   if (on) { (void)r->push(name); }
}
RoctxRange::~RoctxRange()
{
   if (on) { (void)g_roctx.load()->pop(); }
}

Switches read_switches()
{
   Switches s;
   s.vcg_variant = (int)env_long("LGH_VCG_VARIANT", -1);
   s.slab_wide = env_flag("LGH_SLAB_WIDE", 1);
   s.slab_exact = env_flag("LGH_SLAB_EXACT", 1);
   s.slab_merge = env_flag("LGH_SLAB_MERGE", 1);
   s.slab_defer = env_flag("LGH_SLAB_DEFER", 1);
   s.slab_ye_wide = env_flag("LGH_SLAB_YE_WIDE", 0);
   s.slab_dyn = env_flag("LGH_SLAB_DYN", -1);
   s.rz_limbs = env_flag("LGH_RZ_LIMBS", 1);
   s.kron_neb = env_flag("LGH_KRON_NEB", 1);
   s.fused_init = env_flag("LGH_FUSED_INIT", 1);
   s.k2p = env_flag("LGH_K2P", 1);
   s.k2_skip = env_flag("LGH_K2_SKIP", 1);
   s.k2_grid = (int)env_long("LGH_K2_GRID", 0);
   s.k2_node_weight = env_long("LGH_K2_NODE_WEIGHT", 5);
   s.order = env_flag("LGH_ORDER", 1);
   s.order_multi = env_flag("LGH_ORDER_MULTI", 1);
   s.comm2 = env_flag("LGH_COMM2", -1);
   s.force_multi = env_flag("LGH_FORCE_MULTI", 0);
   s.halo_piggyback = env_flag("LGH_HALO_PIGGYBACK", 1);
   s.halo_fused_pack = env_flag("LGH_HALO_FUSED_PACK", 1);
   s.overlap = env_flag("LGH_OVERLAP", 1);
   s.energy_lockstep = env_flag("LGH_ENERGY_LOCKSTEP", 1);
   s.spin = env_flag("LGH_SPIN", 1);
   s.mass_sep = env_flag("LGH_MASS_SEP", 1);
   s.mass_kron = env_flag("LGH_MASS_KRON", 1);
   s.mass_rank1 = env_flag("LGH_MASS_RANK1", 1);
   s.mass_rank1_tol = env_double("LGH_MASS_RANK1_TOL", kMassRank1Tol);
   s.l2_neb = env_flag("LGH_L2_NEB", 1);
   s.l2_plane = env_flag("LGH_L2_PLANE", 1);
   s.l2_fused = env_flag("LGH_L2_FUSED", 1);
   s.q_form = env_flag("LGH_Q_FORM", 1);
   s.q_ppt = env_flag("LGH_Q_PPT", 0);
   s.q_swz = (int)env_long("LGH_Q_SWZ", -1);
   s.q_occ4 = env_flag("LGH_Q_OCC4", -1);
   s.q_discard = (int)env_long("LGH_Q_DISCARD", 1);
   s.q_tiny_grad = env_double("LGH_Q_TINY_GRAD", 1e-30); // 0: exact zeros only; -1: off
   s.fused_ftv = env_flag("LGH_FUSED_FTV", 1);
   s.fused_f1 = env_flag("LGH_FUSED_F1", 1);
   s.b_sym = env_flag("LGH_B_SYM", 1);
   s.jac0_compact = env_flag("LGH_JAC0_COMPACT", 1);
   // (a tolerance above 1e-10 would turn curved zones into affine ones: clamped - round-5 advisor)
   s.jac0_tol = std::min(std::max(env_double("LGH_JAC0_TOL", kJac0Tol), 0.0), 1e-10);
   s.profile_fold = (int)std::max(0L, env_long("LGH_PROFILE_FOLD", 8));
   s.map_fold = (int)std::min(std::max(0L, env_long("LGH_MAP_FOLD", 8)), 64L); // (a wavefront has 64 lanes: no more cells than that)
   s.roctx = env_flag("LGH_ROCTX", 0);
   s.vcg_trace = env_string("LGH_VCG_TRACE");
   s.vcg_trace_phases = getenv("LGH_VCG_TRACE_PHASES") != nullptr;
   s.q_trace = env_string("LGH_Q_TRACE");
   s.q_trace_call = (int)env_long("LGH_Q_TRACE_CALL", 40);
   return s;
}

CtxHandles::~CtxHandles()
{
   if (stream2) { (void)hipStreamDestroy(stream2); }
   if (ev_fork) { (void)hipEventDestroy(ev_fork); } // (create_stream2 may have failed between the stream and its events)
   if (ev_join) { (void)hipEventDestroy(ev_join); }
   if (host_pinned) { (void)hipHostFree(host_pinned); }
   if (own_stream) { (void)hipStreamDestroy(stream); }
}

// What a context of any dimension starts with: the header fields, the stream, the tables, the restriction and its transpose
// (handed back as t_off / t_idx: the 2D/3D context forms its ELL copy from them), the essential masks, the reduction scratch,
// the pinned block, the timer events and the dt slots at +inf.  The arguments have been checked by lgh_create.
int create_common(const lgh_config *cfg, lgh_ctx *c, std::vector<int> &t_off, std::vector<int> &t_idx)
{
   const int dim = cfg->dim;
   auto ipow = [dim](const int n) { return dim == 1 ? n : dim == 2 ? n * n : n * n * n; };
   c->dim = dim; c->NE = cfg->NE; c->D1D = cfg->D1D; c->Q1D = cfg->Q1D; c->L1D = cfg->L1D;
   c->ND = ipow(c->D1D); c->NQ = ipow(c->Q1D); c->NL = ipow(c->L1D);
   c->N = cfg->N;
   c->H1V = dim * c->N;
   c->L2V = c->NE * c->NL;
   c->kid = (dim << 8) | (c->D1D << 4) | c->Q1D;
   c->visc = cfg->use_viscosity != 0;
   c->vort = cfg->use_vorticity != 0;
   c->cfl = cfg->cfl;
   c->h1order = (double)cfg->order_v;
   if (cfg->stream) { c->stream = (hipStream_t)cfg->stream; }
   else { LGH_HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; }

   LGH_PASS(ctx_buffer(c->B, (size_t)c->Q1D * c->D1D, cfg->B_h1));
   LGH_PASS(ctx_buffer(c->G, (size_t)c->Q1D * c->D1D, cfg->G_h1));
   LGH_PASS(ctx_buffer(c->Bl, (size_t)c->Q1D * c->L1D, cfg->B_l2));
   LGH_PASS(ctx_buffer(c->W, (size_t)c->NQ, cfg->weights));
   LGH_PASS(ctx_buffer(c->gamma, (size_t)c->NE, cfg->gamma));
   const size_t nmap = (size_t)c->NE * c->ND;
   LGH_PASS(ctx_buffer(c->h1map, nmap, cfg->h1_map));
   LGH_PASS(mesh_order_build(c, cfg->h1_map)); // the library's own zone order and node numbering (lgh_order.hip; the identity below 3D)
   // transpose of the restriction in CSR form (ascending E-vector position per node: the fixed order of every node sum)
   t_off.assign((size_t)c->N + 1, 0);
   t_idx.resize(nmap);
   for (size_t i = 0; i < nmap; i++) { t_off[(size_t)cfg->h1_map[i] + 1]++; }
   for (int n = 0; n < c->N; n++) { t_off[(size_t)n + 1] += t_off[n]; }
   std::vector<int> pos(t_off.begin(), t_off.end() - 1);
   for (size_t i = 0; i < nmap; i++) { t_idx[pos[cfg->h1_map[i]]++] = (int)i; }
   LGH_PASS(ctx_buffer(c->t_off, t_off.size(), t_off.data()));
   LGH_PASS(ctx_buffer(c->t_idx, t_idx.size(), t_idx.data()));
   for (int k = 0; k < (dim == 1 ? 1 : 3); k++) // (a 2D context has the third mask too, empty)
   {
      c->ess_count[k] = (k < dim) ? cfg->ess_count[k] : 0;
      std::vector<uint8_t> mask((size_t)c->N, 0);
      for (int i = 0; i < c->ess_count[k]; i++) { mask[cfg->ess[k][i]] = 1; }
      LGH_PASS(ctx_buffer(c->essmask[k], mask.size(), mask.data()));
      LGH_PASS(ctx_buffer(c->ess[k], (size_t)c->ess_count[k], c->ess_count[k] ? cfg->ess[k] : nullptr));
   }

   const size_t nv = std::max<size_t>((size_t)c->N, (size_t)c->L2V);
   c->part_stride = (int)std::max<size_t>(std::max<size_t>((size_t)c->NE, (nv + 255) / 256), 2048) + (int)kShards;
   LGH_PASS(ctx_buffer(c->partials, 4 * (size_t)c->part_stride));
   LGH_PASS(ctx_buffer(c->tickets, 4 * (size_t)kTicketSlot));
   LGH_PASS(ctx_buffer(c->cgs, 1));
   LGH_PASS(ctx_buffer(c->scal, 16));
   LGH_HIP_CHECK(hipHostMalloc((void **)&c->host_pinned, kPinDoubles * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
   memset(c->host_pinned, 0, kPinDoubles * sizeof(double));
   LGH_HIP_CHECK(hipHostGetDevicePointer((void **)&c->host_pinned_dev, c->host_pinned, 0)); // (the one-thread kernels in front of a host look write there)
   LGH_HIP_CHECK(hipEventCreate(&c->timers.ev[0]));
   LGH_HIP_CHECK(hipEventCreate(&c->timers.ev[1]));
   const std::vector<double> infs((size_t)kDtSlotStride * (1 + kDtSlots), std::numeric_limits<double>::infinity());
   return ctx_buffer(c->dt_est_dev, infs.size(), infs.data());
}

static bool kernel_id_supported(int id)
{
   switch (id)
   {
      case 0x222: case 0x234: case 0x246: case 0x258: case 0x26A:
      case 0x322: case 0x334: case 0x346: case 0x358: case 0x36A:
         return true;
   }
   return false;
}

} // namespace lgh

namespace lgh
{
int host_wait_token(lgh_ctx *c, volatile unsigned long long *word, const unsigned long long token)
{
   if (c->sw.spin)
   {
      // polling for at most ~50 ms (a look normally returns within the tail of the last enqueued kernels: a chunk of
      // iterations, 1-20 ms); a host that would wait longer than that sleeps in the stream synchronisation below instead
      const auto t0 = std::chrono::steady_clock::now();
      for (long i = 0;; i++)
      {
         if (__atomic_load_n((const unsigned long long *)word, __ATOMIC_ACQUIRE) == token) { return LGH_OK; }
         __builtin_ia32_pause();
         if ((i & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) { break; }
      }
   }
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   if (__atomic_load_n((const unsigned long long *)word, __ATOMIC_ACQUIRE) != token) { set_error("host look: the finishing kernel did not report"); return LGH_ERR_HIP; }
   return LGH_OK;
}

// The stress of the current quadrature data is in memory (readers of stressJinvT call this first).
int stress_on_hand(lgh_ctx *c, const char *who)
{
   if (c->stress_current) { return LGH_OK; }
   set_error("%s needs stressJinvT, which the last lgh_qupdate kept in registers (lgh_qupdate_store_stress(ctx, 0)): "
             "only F.1 and F^T v of the state's own velocity are on hand; store the stress (..., 1) and update again", who);
   return LGH_ERR_ARG;
}

} // namespace lgh

using namespace lgh;

extern "C"
{

const char *lgh_last_error(void) { return g_err; }
const char *lgh_version(void) { return "laghos_hip 0.1 (gfx950)"; }

static int create_impl(const lgh_config *cfg, lgh_ctx *c);

int lgh_create(const lgh_config *cfg, lgh_ctx **out)
{
   LGH_CHECK_ARG(cfg && out);
   LGH_CHECK_ARG(cfg->dim == 1 || cfg->dim == 2 || cfg->dim == 3);
   LGH_CHECK_ARG(cfg->NE > 0 && cfg->N > 0);
   LGH_CHECK_ARG(cfg->h1_map && cfg->B_h1 && cfg->G_h1 && cfg->B_l2 && cfg->weights && cfg->gamma);
   // MFEM_VERIFY(L1D==D1D-1) (laghos_assembly.cpp:533, :943)
   if (cfg->L1D != cfg->D1D - 1)
   {
      set_error("L1D!=D1D-1");
      return LGH_ERR_UNSUPPORTED;
   }
   const int kid = (cfg->dim << 8) | (cfg->D1D << 4) | cfg->Q1D;
   if (!(cfg->dim == 1 ? kernel_id_supported_1d(kid) : kernel_id_supported(kid)))
   {
      set_error("Unknown kernel 0x%x", kid);
      return LGH_ERR_UNSUPPORTED;
   }
   int ndev = 0;
   if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
   {
      set_error("no HIP device available: the laghos_hip path requires an MI355X (gfx950) GPU");
      return LGH_ERR_HIP;
   }
   LGH_HIP_CHECK(hipSetDevice(cfg->device));
   // argument errors a caller can trigger are found before anything is allocated
   LGH_CHECK_ARG(cfg->cfl > 0.0); // (the time-step estimate is a minimum over cfl / inv_dt >= 0, folded as such: lgh_qrows.hpp)
   const size_t nd = (cfg->dim == 1) ? cfg->D1D : (cfg->dim == 2) ? cfg->D1D * cfg->D1D : cfg->D1D * cfg->D1D * cfg->D1D;
   for (size_t i = 0, n = (size_t)cfg->NE * nd; i < n; i++)
   {
      if (cfg->h1_map[i] < 0 || cfg->h1_map[i] >= cfg->N) { set_error("h1_map entry out of range"); return LGH_ERR_ARG; }
   }
   for (int k = 0; k < cfg->dim; k++)
   {
      LGH_CHECK_ARG(cfg->ess_count[k] >= 0 && (cfg->ess_count[k] == 0 || cfg->ess[k]));
      for (int i = 0; i < cfg->ess_count[k]; i++)
      {
         if (cfg->ess[k][i] < 0 || cfg->ess[k][i] >= cfg->N) { set_error("essential dof out of range"); return LGH_ERR_ARG; }
      }
   }
   if (cfg->dim == 1 && cfg->owner)
   {
      set_error("a 1D context runs on one rank: several ranks (an owner mask) are not supported in 1D");
      return LGH_ERR_UNSUPPORTED;
   }

   lgh_ctx *c = new lgh_ctx;
   c->sw = read_switches();
   if (c->sw.roctx) { roctx_enable(); }
   c->device = cfg->device;
   // every failure below (HIP errors, out of memory) releases what was built so far
   const int rc_create = (cfg->dim == 1) ? create_1d(cfg, c) : create_impl(cfg, c);
   if (rc_create != LGH_OK)
   {
      lgh_destroy(c);
      return rc_create;
   }
   *out = c;
   return LGH_OK;
}

// C_F = 3 cG cB^2, cB = max_d sum_q |B[q, d]|, cG likewise from G.  An output of F.1 is the sum over the three reference
// directions gd and the points q of stressJinvT w detJ (q, gd, c) * T_z[qz, dz] T_y[qy, dy] T_x[qx, dx], T = G in direction gd
// and B in the other two: its absolute value is at most max_q|stressJinvT w detJ| times the sum of the three products of
// absolute column sums, each <= cG cB^2.  The row form of the update flushes a zone's outputs without computing them where
// that bound lies below eps^2 (lgh_qrows.hpp).
static double q_force_bound(const lgh_config *cfg)
{
   double cB = 0.0, cG = 0.0;
   for (int d = 0; d < cfg->D1D; d++)
   {
      double sb = 0.0, sg = 0.0;
      for (int q = 0; q < cfg->Q1D; q++)
      {
         sb += std::fabs(cfg->B_h1[q + cfg->Q1D * d]);
         sg += std::fabs(cfg->G_h1[q + cfg->Q1D * d]);
      }
      cB = std::max(cB, sb);
      cG = std::max(cG, sg);
   }
   return 3.0 * cG * (cB * cB);
}

static int create_impl(const lgh_config *cfg, lgh_ctx *c)
{
   std::vector<int> off, idx; // the transpose of the restriction on the host
   LGH_PASS(create_common(cfg, c, off, idx));
   const int dim = c->dim;
   c->q_tiny_grad = c->sw.q_tiny_grad;
   c->q_discard = (c->sw.q_discard == 1) ? (kQDiscardDt | kQDiscardF1) : (c->sw.q_discard == 2) ? kQDiscardDt : (c->sw.q_discard == 3) ? kQDiscardF1 : 0;
   c->q_cF = q_force_bound(cfg);
   {
      // mirror symmetry of the tables (every nodal or Bernstein basis on symmetric points has it); LGH_B_SYM=0: assume not
      auto mirror = [&](const double *B, const int n) {
         if (!c->sw.b_sym) { return 0; }
         for (int i = 0; i < n; i++)
         {
            const double u = B[i], v = B[n - 1 - i];
            if (std::fabs(u - v) > 1e-14 * std::max(1.0, std::max(std::fabs(u), std::fabs(v)))) { return 0; } // (1e-15 at order 5)
         }
         return 1;
      };
      c->b_h1_sym = mirror(cfg->B_h1, c->Q1D * c->D1D);
      c->b_l2_sym = mirror(cfg->B_l2, c->Q1D * c->L1D);
   }
   {
      // Tensor-product rule?  w[i] = W[i, 0, 0] / w[0]^(dim - 1) with w[0] = W[0]^(1/dim); every entry of W must be the
      // product of its three factors to 8 ulp.  The plane-form L2 mass apply then takes the weights from Q scalars
      // instead of NQ loads per element batch (compact mass data only: value(q, e) = s_e w[qx] w[qy] w[qz]).
      const int Q = c->Q1D, dim = c->dim;
      std::vector<double> w1((size_t)Q);
      const double w0 = (dim == 3) ? cbrt(cfg->weights[0]) : sqrt(cfg->weights[0]);
      bool ok = std::isfinite(w0) && w0 > 0.0;
      for (int i = 0; ok && i < Q; i++)
      {
         w1[i] = cfg->weights[i] / ((dim == 3) ? w0 * w0 : w0);
         ok = std::isfinite(w1[i]) && w1[i] > 0.0;
      }
      // (the kernels keep half of them in scalar registers: w[i] = w[Q - 1 - i], as every rule on symmetric points has it)
      for (int i = 0; ok && i < Q / 2; i++)
      {
         ok = std::fabs(w1[i] - w1[Q - 1 - i]) <= 8.9e-16 * w1[i];
         w1[Q - 1 - i] = w1[i];
      }
      for (int q = 0; ok && q < c->NQ; q++)
      {
         const int qx = q % Q, qy = (q / Q) % Q, qz = q / (Q * Q);
         const double prod = (dim == 3) ? w1[qx] * w1[qy] * w1[qz] : w1[qx] * w1[qy];
         ok = std::fabs(prod - cfg->weights[q]) <= 1.8e-15 * std::fabs(cfg->weights[q]);
      }
      if (ok && c->sw.mass_sep) { LGH_PASS(c->w1d.upload(w1.data(), (size_t)Q)); } // (LGH_MASS_SEP=0, A/B: weights from the NQ-entry table)
      // 1-D mass tiles of the two bases on this rule, M1[i + n j] = sum_q B[q, i] w[q] B[q, j] (long double sums, rounded
      // once): with compact mass data the element matrices are s_e M1 (x) M1 (x) M1 (lgh_vcg_slab.hip, lgh_mass.hip)
      if (c->w1d && c->sw.mass_kron) // (LGH_MASS_KRON=0, A/B: always contract through the quadrature points)
      {
         auto tile = [&](const double *Bt, const int n, DevPtr<double> &out) -> int {
            std::vector<double> M((size_t)n * n);
            for (int i = 0; i < n; i++)
            {
               for (int j = 0; j < n; j++)
               {
                  long double s = 0.0L;
                  for (int q = 0; q < Q; q++) { s += (long double)Bt[q + Q * i] * (long double)w1[q] * (long double)Bt[q + Q * j]; }
                  M[(size_t)i + (size_t)n * j] = (double)s;
               }
            }
            return out.upload(M.data(), M.size());
         };
         LGH_PASS(tile(cfg->B_h1, c->D1D, c->M1h));
         LGH_PASS(tile(cfg->B_l2, c->L1D, c->M1l));
      }
   }
   const size_t nmap = (size_t)c->NE * c->ND;
   {
      // the transpose in ELL form
      int deg = 0;
      for (int n = 0; n < c->N; n++) { deg = std::max(deg, off[(size_t)n + 1] - off[n]); }
      std::vector<int> ell((size_t)deg * c->N, -1);
      for (int n = 0; n < c->N; n++)
         for (int k = off[n]; k < off[(size_t)n + 1]; k++) { ell[(size_t)(k - off[n]) * c->N + n] = idx[k]; }
      c->t_deg = deg;
      LGH_PASS(ctx_buffer(c->t_ell, ell.size(), ell.data()));
   }
   if (cfg->owner) { LGH_PASS(c->owner.upload(cfg->owner, (size_t)c->N)); }

   const size_t nq = (size_t)c->NE * c->NQ;
   LGH_PASS(ctx_buffer(c->stressJinvT, nq * dim * dim));
   LGH_PASS(ctx_buffer(c->Jac0inv, nq * dim * dim));
   LGH_PASS(ctx_buffer(c->Jac0inv_soa, nq * dim * dim));
   LGH_PASS(ctx_buffer(c->Jac0inv_e, (size_t)cfg->NE * dim * dim));
   LGH_PASS(ctx_buffer(c->rho0DetJ0w, nq));
   LGH_PASS(ctx_buffer(c->massD, nq + 2048)); // (one set of the matrix-core K1 behind the last element: its pipeline prefetches without predicates)
   LGH_PASS(ctx_buffer(c->diagV, (size_t)c->N));
   LGH_PASS(ctx_buffer(c->dinvV, (size_t)c->N));
   {
      if (c->sw.fused_ftv) // (LGH_FUSED_FTV=0, A/B: F^T v always by its own kernel)
      {
         LGH_PASS(ctx_buffer(c->erhs_q, (size_t)c->L2V));
         LGH_PASS(ctx_buffer(c->v_snap, (size_t)c->H1V));
      }
      LGH_PASS(ctx_buffer(c->dev_flags, (size_t)8));
      // (LGH_FUSED_F1=0, A/B: F.1 always by its own kernel)
      if (c->dim == 3 && c->sw.fused_f1) { LGH_PASS(ctx_buffer(c->force_e_q, nmap * dim + (size_t)dim * c->ND)); } // (+ a zero element: vcg_init_force_z_k)
   }
   const size_t ne_nd = nmap * dim;
   LGH_PASS(ctx_buffer(c->XE, std::max<size_t>(ne_nd, (size_t)c->L2V)));
   LGH_PASS(ctx_buffer(c->YE, ne_nd + (size_t)dim * c->ND)); // (+ a zero element: vcg_init_force_z_k)
   const size_t nv = std::max<size_t>((size_t)c->N, (size_t)c->L2V);
   LGH_PASS(ctx_buffer(c->cg_r, nv));
   LGH_PASS(ctx_buffer(c->cg_z, nv));
   LGH_PASS(ctx_buffer(c->cg_d0, nv));
   LGH_PASS(ctx_buffer(c->cg_d1, nv));
   LGH_PASS(ctx_buffer(c->cg_y, nv));
   return LGH_OK;
}

lgh_ctx::lgh_ctx() = default;
lgh_ctx::~lgh_ctx() = default;

int lgh_destroy(lgh_ctx *c)
{
   if (!c) { return LGH_OK; }
   (void)hipSetDevice(c->device);
   (void)hipStreamSynchronize(c->stream);
   if (c->stream2) { (void)hipStreamSynchronize(c->stream2); }
   delete c; // every member releases what it owns (lgh_common.hpp)
   return LGH_OK;
}

int lgh_sync(lgh_ctx *c)
{
   LGH_CHECK_ARG(c);
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   return LGH_OK;
}
void *lgh_stream(lgh_ctx *c) { return c ? (void *)c->stream : nullptr; }

static void invalidate_fused(lgh_ctx *c)
{
   c->fused_ftv_valid = 0;
   c->fused_f1_valid = 0;
   c->qgen++;
}
double *lgh_qdata_stressJinvT(lgh_ctx *c)
{
   // the caller may write through this pointer: F^T v and F.1 of the fused update no longer belong to it
   invalidate_fused(c);
   // default mode: whatever the caller puts there is what the force kernels read from now on.  With the stress kept in
   // registers (explicit opt-in) a request for the pointer does not turn planes nobody wrote into current data: the
   // readers keep refusing until lgh_qupdate_store_stress(ctx, 1) and an update
   if (c->stress_store) { c->stress_current = 1; }
   return c->stressJinvT;
}
// Entry points with no 1D form (the 2D/3D kernel forms, the lockstep solve, E-vector test hooks) refuse a 1D context.
static int no_1d(const lgh_ctx *c, const char *who)
{
   if (c->dim != 1) { return LGH_OK; }
   set_error("%s: not available for a 1D context (lgh_1d.hip has its own kernels)", who);
   return LGH_ERR_UNSUPPORTED;
}
int lgh_qupdate_form(lgh_ctx *c, int *form)
{
   LGH_CHECK_ARG(c && form);
   *form = qupdate_form(c);
   return LGH_OK;
}
int lgh_qupdate_discard(lgh_ctx *c, int *mode, double *C_F)
{
   LGH_CHECK_ARG(c && mode && C_F);
   *mode = c->q_discard;
   *C_F = c->q_cF;
   return LGH_OK;
}
int lgh_qupdate_stores_stress(lgh_ctx *c, int *on)
{
   LGH_CHECK_ARG(c && on);
   // (what the next lgh_qupdate will do: the planes are only left out when both products come out of the update kernel)
   *on = (!c->stress_store && c->erhs_q && c->force_e_q && c->v_snap && !c->fused_forces_off && c->dim == 3) ? 0 : 1;
   return LGH_OK;
}
int lgh_qupdate_store_stress(lgh_ctx *c, int on)
{
   LGH_CHECK_ARG(c);
   if ((on != 0) != (c->stress_store != 0))
   {
      c->stress_store = on ? 1 : 0;
      invalidate_fused(c); // the quadrature data has to be updated again before anything reads it
      c->stress_current = 0;
   }
   return LGH_OK;
}
int lgh_reset_quadrature_data(lgh_ctx *c)
{
   LGH_CHECK_ARG(c);
   invalidate_fused(c);
   return LGH_OK;
}
// The force products of the last lgh_qupdate as vectors: F.1 summed to the H1 L-vector (what SolveVelocity negates into
// its right-hand side), F^T v_state as L2 vector.  LGH_ERR_ARG when the product is not on hand (fusion off, 2D for
// F.1, quadrature data changed since).
int lgh_fused_force_mult(lgh_ctx *c, double *y_h1)
{
   LGH_CHECK_ARG(c && y_h1);
   if (!(c->force_e_q && c->fused_f1_valid)) { set_error("lgh_fused_force_mult: no fused F.1 on hand"); return LGH_ERR_ARG; }
   int rc = h1_transpose_gather(c, c->dim, c->force_e_q, y_h1);
   if (rc == LGH_OK && c->multi != 0) { rc = halo_sum(c, y_h1, c->dim); }
   return rc;
}
int lgh_fused_force_e(lgh_ctx *c, double *y_e)
{
   LGH_CHECK_ARG(c && y_e);
   if (!(c->force_e_q && c->fused_f1_valid)) { set_error("lgh_fused_force_e: no fused F.1 on hand"); return LGH_ERR_ARG; }
   LGH_HIP_CHECK(hipMemcpyAsync(y_e, c->force_e_q, sizeof(double) * (size_t)c->dim * c->NE * c->ND, hipMemcpyDeviceToDevice, c->stream));
   return LGH_OK;
}
int lgh_fused_force_mult_transpose(lgh_ctx *c, double *y_l2)
{
   LGH_CHECK_ARG(c && y_l2);
   if (!(c->erhs_q && c->fused_ftv_valid)) { set_error("lgh_fused_force_mult_transpose: no fused F^T v on hand"); return LGH_ERR_ARG; }
   LGH_HIP_CHECK(hipMemcpyAsync(y_l2, c->erhs_q, sizeof(double) * (size_t)c->L2V, hipMemcpyDeviceToDevice, c->stream));
   return LGH_OK;
}
int lgh_quadrature_generation(lgh_ctx *c, unsigned long *gen, int *f1_valid, int *ftv_valid)
{
   LGH_CHECK_ARG(c && gen && f1_valid && ftv_valid);
   *gen = c->qgen;
   *f1_valid = c->fused_f1_valid;
   *ftv_valid = c->fused_ftv_valid;
   return LGH_OK;
}
double *lgh_qdata_Jac0inv(lgh_ctx *c) { return c->Jac0inv; }
double *lgh_qdata_rho0DetJ0w(lgh_ctx *c) { return c->rho0DetJ0w; }
double *lgh_mass_D(lgh_ctx *c)
{
   c->mass_rank1 = -1; // (the caller may write through this pointer: the compact form of the mass data is looked for again)
   c->mass_gen++;
   return c->massD;
}
int lgh_mass_data_form(lgh_ctx *c, int *form)
{
   LGH_CHECK_ARG(c && form);
   if (c->dim == 1) { *form = 0; return LGH_OK; } // (the 1D kernels read the stored table)
   const double *Dq, *Se;
   int dqs;
   int rc = mass_data(c, &Dq, &dqs, &Se);
   if (rc) { return rc; }
   *form = (c->mass_rank1 == 1) ? 1 : 0;
   return LGH_OK;
}
int lgh_mass_data_changed(lgh_ctx *c)
{
   LGH_CHECK_ARG(c);
   c->mass_rank1 = -1;            // the compact form is looked for again at the next mass apply
   c->mass_gen++;
   if (c->dim == 1) { return mass_changed_1d(c); } // (and the factors of the zone mass matrices of the energy solve)
   return mass_assemble_diag(c);  // operator and Jacobi preconditioner stay consistent (laghos_solver.cpp:266-270)
}
double *lgh_mass_diag(lgh_ctx *c) { return c->diagV; }
int lgh_set_h0(lgh_ctx *c, double h0) { LGH_CHECK_ARG(c); c->h0 = h0; return LGH_OK; }
int lgh_get_h0(lgh_ctx *c, double *h0) { LGH_CHECK_ARG(c && h0); *h0 = c->h0; return LGH_OK; }

int lgh_set_dt_est(lgh_ctx *c, double v)
{
   LGH_CHECK_ARG(c);
   hipLaunchKernelGGL(dt_est_set_k, dim3(1), dim3(256), 0, c->stream, c->dt_est_dev, v);
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}
int lgh_get_dt_est(lgh_ctx *c, double *v)
{
   LGH_CHECK_ARG(c && v);
   const unsigned long long token = ++c->look_token;
   hipLaunchKernelGGL(dt_est_fold_k, dim3(1), dim3(256), 0, c->stream, c->dt_est_dev, c->dev_flags + 4, c->host_pinned_dev + kPinDt, token);
   LGH_HIP_CHECK(hipGetLastError());
   {
      const int rc = host_wait_token(c, (volatile unsigned long long *)(c->host_pinned + kPinDtToken), token);
      if (rc) { return rc; }
   }
   *v = c->host_pinned[kPinDt];
   if (*(const int *)(c->host_pinned + kPinDtFlag) != 0)
   {
      LGH_HIP_CHECK(hipMemsetAsync(c->dev_flags + 4, 0, sizeof(int), c->stream));
      set_error("lgh_solve_energy was given a velocity other than the state's while the stress was kept in registers "
                "(lgh_qupdate_store_stress(ctx, 0)): its right-hand side is NaN");
      return LGH_ERR_ARG;
   }
   return LGH_OK;
}

int lgh_setup_rho0detj0(lgh_ctx *c, const double *x0, const double *rho0_l2, const double *rho0_q,
                        double *volume)
{
   LGH_CHECK_ARG(c && x0 && rho0_l2 && rho0_q && volume);
   invalidate_fused(c);
   c->mass_rank1 = -1; // (new mass data)
   c->mass_gen++;
   int rc = (c->dim == 1) ? setup_1d(c, x0, rho0_l2, rho0_q, volume) // (with the diagonal and the zone mass factors)
                          : setup_rho0detj0(c, x0, rho0_l2, rho0_q, volume);
   if (rc) { return rc; }
   if (c->dim != 1) { rc = mass_assemble_diag(c); }
   if (rc == LGH_OK) { c->setup_done = 1; }
   return rc;
}

int lgh_force_mult(lgh_ctx *c, const double *x_l2, double *y_h1)
{
   LGH_CHECK_ARG(c && x_l2 && y_h1);
   // L2R->Mult is the identity for the lexicographic L2 space (assembly.cpp:559-560)
   int rc = stress_on_hand(c, "lgh_force_mult"); // (a refusal is taken before the timing sample opens)
   if (rc) { return rc; }
   if (c->dim == 1) { return force_mult_1d(c, x_l2, y_h1); }
   kt_begin(c, LGH_KERNEL_FORCE_MULT);
   rc = force_mult_E(c, c->stressJinvT, x_l2, c->YE);
   kt_end(c, LGH_KERNEL_FORCE_MULT);
   if (rc) { return rc; }
   rc = h1_transpose_gather(c, c->dim, c->YE, y_h1); // H1R->MultTranspose (:564)
   if (rc) { return rc; }
   if (c->multi != 0) { rc = halo_sum(c, y_h1, c->dim); }
   return rc;
}
int lgh_force_mult_transpose(lgh_ctx *c, const double *v_h1, double *y_l2)
{
   LGH_CHECK_ARG(c && v_h1 && y_l2);
   const int rc0 = stress_on_hand(c, "lgh_force_mult_transpose");
   if (rc0) { return rc0; }
   if (c->dim == 1) { return force_mult_t_1d(c, v_h1, y_l2); }
   kt_begin(c, LGH_KERNEL_FORCE_MULT_T);
   const int rc = force_mult_t_L(c, c->stressJinvT, v_h1, y_l2);
   kt_end(c, LGH_KERNEL_FORCE_MULT_T);
   return rc;
}

int lgh_mass_set_essential_tdofs(lgh_ctx *c, int comp)
{
   LGH_CHECK_ARG(c && comp >= -1 && comp < c->dim);
   c->cur_ess = comp;
   return LGH_OK;
}
int lgh_mass_eliminate_rhs(lgh_ctx *c, double *b)
{
   LGH_CHECK_ARG(c && b);
   if (c->cur_ess < 0) { return LGH_OK; }
   return vec_zero_list(c, b, c->ess[c->cur_ess], c->ess_count[c->cur_ess]);
}
int lgh_mass_mult(lgh_ctx *c, int space, const double *x, double *y)
{
   LGH_CHECK_ARG(c && x && y && (space == LGH_SPACE_H1 || space == LGH_SPACE_L2));
   if (c->dim == 1) { return mass_apply_1d(c, space, x, y, true); }
   return space == LGH_SPACE_H1 ? mass_apply_h1(c, x, y, true) : mass_apply_l2(c, x, y);
}
int lgh_mass_mult_full(lgh_ctx *c, int space, const double *x, double *y)
{
   LGH_CHECK_ARG(c && x && y && (space == LGH_SPACE_H1 || space == LGH_SPACE_L2));
   if (c->dim == 1) { return mass_apply_1d(c, space, x, y, false); }
   return space == LGH_SPACE_H1 ? mass_apply_h1(c, x, y, false) : mass_apply_l2(c, x, y);
}

int lgh_cg_solve(lgh_ctx *c, int space, const double *b, double *x, double rel_tol, int max_iter,
                 int *iters)
{
   LGH_CHECK_ARG(c && b && x && (space == LGH_SPACE_H1 || space == LGH_SPACE_L2));
   if (c->dim == 1) { return cg_1d(c, space, b, x, rel_tol, max_iter, iters, false); }
   return cg_solve(c, space, b, x, rel_tol, max_iter, iters, false);
}

int lgh_l2_mass_solve_local(lgh_ctx *c, const double *b, double *x)
{
   LGH_CHECK_ARG(c && b && x);
   if (c->dim != 1)
   {
      set_error("lgh_l2_mass_solve_local: the zone-local energy solve belongs to the 1D (full-assembly) path; 2D/3D run the energy CG");
      return LGH_ERR_UNSUPPORTED;
   }
   return l2_solve_local_1d(c, b, x);
}

int lgh_qupdate(lgh_ctx *c, const double *S)
{
   LGH_CHECK_ARG(c && S);
   RoctxRange range("QUpdate-UpdateQuadratureData"); // laghos_solver.cpp:1358
   timer_start(c);
   kt_begin(c, LGH_KERNEL_QUPDATE);
   int rc = (c->dim == 1) ? qupdate_1d(c, S) : qupdate(c, S);
   kt_end(c, LGH_KERNEL_QUPDATE);
   timer_stop(c, 3);
   c->timers.c[2] += c->NE;
   return rc;
}

// The fused update forms F.1 for the constant-one L2 function, which is what SolveVelocity passes
// (laghos_solver.cpp:170-171, :354).  one_l2 == NULL means exactly that - the operator's own `one`, as in the
// reference, whose SolveVelocity takes no such argument - and costs nothing.  A vector passed explicitly is checked
// on every call (a pass over it and a host look): nothing is remembered about an address.
__global__ void __launch_bounds__(256) not_all_ones_k(const double *x, const long n, int *flag)
{
   const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
   if (i < n && x[i] != 1.0) { *flag = 1; }
}
static bool is_the_one_vector(lgh_ctx *c, const double *one_l2)
{
   if (!one_l2) { return true; }
   int *flag = c->dev_flags + 1;
   if (hipMemsetAsync(flag, 0, sizeof(int), c->stream) != hipSuccess) { return false; }
   hipLaunchKernelGGL(not_all_ones_k, dim3(ceil_div(c->L2V, 256)), dim3(256), 0, c->stream, one_l2, (long)c->L2V, flag);
   int h = 1;
   if (hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess) { return false; }
   if (hipStreamSynchronize(c->stream) != hipSuccess) { return false; }
   return h == 0;
}
// the vector ForcePA->Mult is applied to when the kernel has to run: the caller's, or the context's own ones
static int one_vector(lgh_ctx *c, const double *one_l2, const double **out)
{
   if (one_l2) { *out = one_l2; return LGH_OK; }
   if (!c->ones_l2)
   {
      LGH_PASS(c->ones_l2.alloc((size_t)c->L2V));
      const int rc = vec_set(c, c->ones_l2, 1.0, c->L2V);
      if (rc) { return rc; }
   }
   *out = c->ones_l2;
   return LGH_OK;
}

// SolveVelocity, PA branch without acceleration source (laghos_solver.cpp:329-399).
// The caller has already run UpdateQuadratureData(S) if the data was stale (:332).
int lgh_solve_velocity(lgh_ctx *c, const double *S, double *dS_dt, const double *one_l2,
                       double *rhs_h1, double *work_B, double rel_tol, int max_iter, int *h1_iters)
{
   LGH_CHECK_ARG(c && S && dS_dt && rhs_h1 && work_B);
   const int dim = c->dim, N = c->N;
   double *dv = dS_dt + c->H1V;
   int rc;
   if (dim == 1) // the FA branch (laghos_solver.cpp:400-439; lgh_1d.hip)
   {
      LGH_CHECK_ARG(!c->accel_src);
      const double *ones = nullptr;
      rc = one_vector(c, one_l2, &ones);
      if (rc) { return rc; }
      rc = stress_on_hand(c, "lgh_solve_velocity");
      if (rc) { return rc; }
      return solve_velocity_1d(c, ones, dv, rhs_h1, rel_tol, max_iter, h1_iters);
   }
   // One rank, region timers off, no acceleration source: the E->L sum of F.1, the negation,
   // EliminateRHS, dv = 0 and the CG initialisation are one kernel (vcg_init_force_k), with
   // bit-identical results.  With the timers on the reference's regions are kept apart.
   if (!c->timers.enabled && !c->accel_src && vcg_fused_init_ok(c))
   {
      // F.1 up to the E-vector (:354): formed by the fused update for this very state, or by the force kernel
      const double *force_E = c->YE;
      if (c->force_e_q && c->fused_f1_valid && is_the_one_vector(c, one_l2)) { force_E = c->force_e_q; }
      else
      {
         const double *ones = nullptr;
         rc = one_vector(c, one_l2, &ones);
         if (rc) { return rc; }
         rc = stress_on_hand(c, "lgh_solve_velocity (F.1 of a vector other than one, or of changed quadrature data)");
         if (rc) { return rc; }
         kt_begin(c, LGH_KERNEL_FORCE_MULT);
         rc = force_mult_E(c, c->stressJinvT, ones, c->YE);
         kt_end(c, LGH_KERNEL_FORCE_MULT);
         if (rc) { return rc; }
      }
      int its[3] = {0, 0, 0};
      RoctxRange range("SolveVelocity-CGVMass"); // laghos_solver.cpp:387-390 (here: with the E->L sum of F.1 and EliminateRHS in its first kernel)
      rc = vcg_solve(c, rhs_h1, dv, rel_tol, max_iter, its, force_E); // :358-388
      if (rc) { return rc; }
      for (int cc = 0; cc < dim; cc++)
      {
         c->timers.c[0] += its[cc]; // :392
         if (h1_iters) { *h1_iters += its[cc]; }
      }
      c->cur_ess = dim - 1;
      return LGH_OK;
   }
   rc = vec_set(c, dv, 0.0, c->H1V); // dv = 0.0 (:338)
   if (rc) { return rc; }
   {
   RoctxRange range("SolveVelocity-ForcePA"); // laghos_solver.cpp:353-356
   timer_start(c);
   if (c->force_e_q && c->fused_f1_valid && is_the_one_vector(c, one_l2))
   {
      // F.1 of this state from the fused update: only H1R^T (and the sum over the ranks) is left of :354, and
      // the right-hand side has the bits of the fused-init path above
      rc = h1_transpose_gather(c, c->dim, c->force_e_q, rhs_h1);
      if (rc == LGH_OK && c->multi != 0) { rc = halo_sum(c, rhs_h1, c->dim); }
   }
   else
   {
      const double *ones = nullptr;
      rc = one_vector(c, one_l2, &ones);
      if (rc == LGH_OK) { rc = lgh_force_mult(c, ones, rhs_h1); } // :354
   }
   timer_stop(c, 2);
   }
   if (rc) { return rc; }
   rc = vec_neg_inplace(c, rhs_h1, c->H1V); // :358
   if (rc) { return rc; }
   if (c->accel_src) // source_type == 2: B_c += VMassPA->MultFull(accel_c) (:371-380), before EliminateRHS
   {
      for (int cc = 0; cc < dim; cc++)
      {
         rc = mass_apply_h1(c, c->accel_src + (size_t)cc * N, work_B, false);
         if (rc) { return rc; }
         rc = vec_axpby(c, rhs_h1 + (size_t)cc * N, 1.0, rhs_h1 + (size_t)cc * N, 1.0, work_B, N);
         if (rc) { return rc; }
      }
   }
   // the dim component solves in lockstep (lgh_vcg.hip) when the kernel id has it
   {
      for (int cc = 0; cc < dim; cc++)
      {
         // EliminateRHS with c_tdofs[cc] (:383-384); rhs_h1 is caller scratch
         rc = vec_zero_list(c, rhs_h1 + (size_t)cc * N, c->ess[cc], c->ess_count[cc]);
         if (rc) { return rc; }
      }
      int its[3] = {0, 0, 0};
      RoctxRange range("SolveVelocity-CGVMass"); // laghos_solver.cpp:387-390
      timer_start(c);
      rc = vcg_solve(c, rhs_h1, dv, rel_tol, max_iter, its); // :388 for all components
      if (rc == LGH_OK)
      {
         timer_stop(c, 0);
         for (int cc = 0; cc < dim; cc++)
         {
            c->timers.c[0] += its[cc]; // :392
            if (h1_iters) { *h1_iters += its[cc]; }
         }
         c->cur_ess = dim - 1;
         return LGH_OK;
      }
      if (rc != LGH_ERR_UNSUPPORTED) { return rc; }
   }
   for (int cc = 0; cc < dim; cc++)
   {
      // B = rhs_c (Pconf is the identity on a conforming mesh; shared-node sums
      // were already applied by lgh_force_mult) (:368-369)
      LGH_HIP_CHECK(hipMemcpyAsync(work_B, rhs_h1 + (size_t)cc * N, sizeof(double) * N,
                                   hipMemcpyDeviceToDevice, c->stream));
      rc = lgh_mass_set_essential_tdofs(c, cc); // :383
      if (rc) { return rc; }
      rc = lgh_mass_eliminate_rhs(c, work_B); // :384
      if (rc) { return rc; }
      int it = 0;
      timer_start(c);
      rc = cg_solve(c, LGH_SPACE_H1, work_B, dv + (size_t)cc * N, rel_tol, max_iter, &it, true); // :388
      timer_stop(c, 0);
      if (rc) { return rc; }
      c->timers.c[0] += it; // :392
      if (h1_iters) { *h1_iters += it; }
   }
   return LGH_OK;
}

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
   int rc = vec_dot(c, x, y, nullptr, n, c->scal + 1);
   if (rc) { return rc; }
   LGH_HIP_CHECK(hipMemcpyAsync(c->host_pinned + kPinDot, c->scal + 1, sizeof(double), hipMemcpyDeviceToHost, c->stream));
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   *result = c->host_pinned[kPinDot];
   return LGH_OK;
}

int lgh_set_velocity_source(lgh_ctx *c, const double *accel_h1)
{
   LGH_CHECK_ARG(c);
   if (accel_h1)
   {
      const int rc = no_1d(c, "lgh_set_velocity_source"); // (problem 7 has no 1D form)
      if (rc) { return rc; }
   }
   c->accel_src = accel_h1;
   return LGH_OK;
}

int lgh_tg_source_2d(lgh_ctx *c, const double *S, double *e_source)
{
   LGH_CHECK_ARG(c && S && e_source);
   const int rc = no_1d(c, "lgh_tg_source_2d");
   if (rc) { return rc; }
   return tg_source_2d(c, S, e_source);
}

int lgh_internal_energy(lgh_ctx *c, const double *e_l2, double *result)
{
   LGH_CHECK_ARG(c && e_l2 && result);
   if (c->dim == 1) { return energy_1d(c, 0, e_l2, result); }
   return interp_energy(c, 0, e_l2, result);
}
int lgh_kinetic_energy(lgh_ctx *c, const double *v_h1, double *result)
{
   LGH_CHECK_ARG(c && v_h1 && result);
   if (c->dim == 1) { return energy_1d(c, 1, v_h1, result); }
   return interp_energy(c, 1, v_h1, result);
}

int lgh_get_timers(lgh_ctx *c, double t[4], long n[3])
{
   LGH_CHECK_ARG(c && t && n);
   for (int i = 0; i < 4; i++) { t[i] = c->timers.t[i]; }
   for (int i = 0; i < 3; i++) { n[i] = c->timers.c[i]; }
   return LGH_OK;
}
int lgh_reset_timers(lgh_ctx *c)
{
   LGH_CHECK_ARG(c);
   for (int i = 0; i < 4; i++) { c->timers.t[i] = 0; }
   for (int i = 0; i < 3; i++) { c->timers.c[i] = 0; }
   return LGH_OK;
}
int lgh_enable_timers(lgh_ctx *c, int on)
{
   LGH_CHECK_ARG(c);
   c->timers.enabled = on != 0;
   return LGH_OK;
}

int lgh_ktime_begin(lgh_ctx *c, int which, int max_samples)
{
   LGH_CHECK_ARG(c && which >= 0 && max_samples > 0);
   if (!c->ktime) { c->ktime.reset(new KTime()); }
   KTime *k = c->ktime.get();
   while ((int)k->ev.size() < 2 * max_samples)
   {
      hipEvent_t e;
      LGH_HIP_CHECK(hipEventCreate(&e));
      k->ev.push_back(e);
   }
   k->which = which;
   k->max = max_samples;
   k->n = 0;
   return LGH_OK;
}
int lgh_ktime_end(lgh_ctx *c, int *launches, double *mean_seconds)
{
   LGH_CHECK_ARG(c && launches && mean_seconds && c->ktime);
   KTime *k = c->ktime.get();
   LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   double tot = 0.0;
   for (int i = 0; i < k->n; i++)
   {
      float ms = 0.f;
      LGH_HIP_CHECK(hipEventElapsedTime(&ms, k->ev[2 * i], k->ev[2 * i + 1]));
      tot += 1e-3 * ms;
   }
   *launches = k->n;
   *mean_seconds = k->n ? tot / k->n : 0.0;
   k->which = -1;
   return LGH_OK;
}

int lgh_set_fused_forces(lgh_ctx *c, int on)
{
   LGH_CHECK_ARG(c);
   if (c->fused_forces_off == (on ? 0 : 1)) { return LGH_OK; } // (nothing changes: the products on hand stay)
   c->fused_forces_off = on ? 0 : 1;
   invalidate_fused(c);
   return LGH_OK;
}

int lgh_get_fused_forces(lgh_ctx *c, int *f1, int *ftv)
{
   LGH_CHECK_ARG(c && f1 && ftv);
   *f1 = (c->force_e_q && !c->fused_forces_off) ? 1 : 0;
   *ftv = (c->erhs_q && !c->fused_forces_off) ? 1 : 0;
   return LGH_OK;
}

int lgh_qupdate_set_tiny_grad(lgh_ctx *c, double tiny_grad)
{
   LGH_CHECK_ARG(c);
   c->q_tiny_grad = tiny_grad;
   return LGH_OK;
}

int lgh_table_symmetry(lgh_ctx *c, int *h1, int *l2)
{
   LGH_CHECK_ARG(c && h1 && l2);
   *h1 = c->b_h1_sym;
   *l2 = c->b_l2_sym;
   return LGH_OK;
}
int lgh_l2_mass_form(lgh_ctx *c, int *form, int *compact)
{
   LGH_CHECK_ARG(c && form && compact);
   if (c->dim == 1) { *form = 0; *compact = 0; return LGH_OK; } // (l2_mass_1d_k: one zone per lane, the stored table)
   return l2_mass_form(c, form, compact);
}
int lgh_k1_form(lgh_ctx *c, int *form)
{
   LGH_CHECK_ARG(c && form);
   *form = (c->dim == 1) ? -1 : vcg_k1_form(c);
   return LGH_OK;
}

int lgh_test_vcg_k1(lgh_ctx *c, const double *r, const double *d_old, const double rz[3], const double rz_prev[3], int first,
                    double *y_E, double den[3])
{
   LGH_CHECK_ARG(c && r && (first || d_old) && rz && rz_prev && y_E && den);
   const int rc = no_1d(c, "lgh_test_vcg_k1");
   if (rc) { return rc; }
   return vcg_test_k1(c, r, d_old, rz, rz_prev, first, y_E, den);
}
int lgh_jac0inv_form(lgh_ctx *c, int *compact)
{
   LGH_CHECK_ARG(c && compact);
   *compact = (c->jac0_compact == 1) ? 1 : 0;
   return LGH_OK;
}
int lgh_vcg_layout_stats(lgh_ctx *c, long out[4])
{
   LGH_CHECK_ARG(c && out);
   const int rc = no_1d(c, "lgh_vcg_layout_stats");
   if (rc) { return rc; }
   return vcg_layout_stats(c, out);
}
int lgh_test_vcg_merged_faces(lgh_ctx *c, unsigned char *mask, long *n_merged)
{
   LGH_CHECK_ARG(c && mask && n_merged);
   const int rc = no_1d(c, "lgh_test_vcg_merged_faces");
   if (rc) { return rc; }
   return vcg_test_merged_faces(c, mask, n_merged);
}
int lgh_test_vcg_k2(lgh_ctx *c, int it, const double *y_E, double *r, double *d, double *x, const double den[3], const double rz[3],
                    const double rz_prev[3], const double alpha_prev[3], double rz_out[3], int *deferred_x)
{
   LGH_CHECK_ARG(c && it >= 1 && y_E && r && d && x && den && rz && rz_prev && alpha_prev && rz_out && deferred_x);
   const int rc = no_1d(c, "lgh_test_vcg_k2");
   if (rc) { return rc; }
   return vcg_test_k2(c, it, y_E, r, d, x, den, rz, rz_prev, alpha_prev, rz_out, deferred_x);
}
int lgh_test_exact_sum(lgh_ctx *c, int mode, long n, int G, int E, const double *scale, const double *v, const long long *w_in,
                       long long *w_out, double *d_out, int *i_out)
{
   LGH_CHECK_ARG(c && mode >= 0 && mode <= 4 && n >= 1 && n <= (1L << 24) && E >= -1000 && E <= 1000);
   LGH_CHECK_ARG(mode != 0 || (v && w_out && i_out));
   LGH_CHECK_ARG(mode != 1 || (w_in && d_out && !scale));
   LGH_CHECK_ARG(mode != 2 || (v && w_out && d_out && G >= 1 && G <= 1024));
   LGH_CHECK_ARG(mode != 3 || (w_in && w_out && n % 64 == 0));
   LGH_CHECK_ARG(mode != 4 || (v && i_out));
   return vcg_test_exact_sum(c, mode, n, G, E, scale, v, w_in, w_out, d_out, i_out);
}
int lgh_force_mult_E(lgh_ctx *c, const double *sJit, const double *x_E, double *y_E)
{
   LGH_CHECK_ARG(c && sJit && x_E && y_E);
   const int rc = no_1d(c, "lgh_force_mult_E");
   if (rc) { return rc; }
   return force_mult_E(c, sJit, x_E, y_E);
}
int lgh_force_mult_transpose_E(lgh_ctx *c, const double *sJit, const double *v_E, double *y_E)
{
   LGH_CHECK_ARG(c && sJit && v_E && y_E);
   const int rc = no_1d(c, "lgh_force_mult_transpose_E");
   if (rc) { return rc; }
   return force_mult_t_E(c, sJit, v_E, y_E);
}
int lgh_mass_apply_E(lgh_ctx *c, int space, const double *x_E, double *y_E)
{
   LGH_CHECK_ARG(c && x_E && y_E);
   const int rc = no_1d(c, "lgh_mass_apply_E");
   if (rc) { return rc; }
   return mass_apply_E(c, space, x_E, y_E);
}
int lgh_test_eig(lgh_ctx *c, int dim, int n, const double *A, double *lambda, double *vec)
{
   LGH_CHECK_ARG(c && A && lambda && vec && (dim == 2 || dim == 3));
   return test_eig(c, dim, n, A, lambda, vec);
}
int lgh_test_sqrt(lgh_ctx *c, int n, const double *x, double *y)
{
   LGH_CHECK_ARG(c && x && y && n >= 0);
   return test_sqrt(c, n, x, y);
}
int lgh_test_singular(lgh_ctx *c, int dim, int n, const double *A, double *sv)
{
   LGH_CHECK_ARG(c && A && sv && (dim == 2 || dim == 3));
   return test_singular(c, dim, n, A, sv);
}

} // extern "C"
