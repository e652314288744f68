// lgh_context.hip — the life cycle of a context: lgh_create checks its arguments, reads the switches and builds what every
// dimension shares (create_common) and what 2D/3D add (create_2d3d: a sequence of named steps); lgh_destroy deletes it, and
// every member releases what it owns (lgh_common.hpp).
#include <cmath>
#include <limits>

#include "lgh_comm_transport.hpp"
#include "lgh_vcg.hpp"

// (here Comm, VcgAux and MeshOrder are complete types)
lgh_ctx::lgh_ctx() = default;
lgh_ctx::~lgh_ctx() = default;

namespace lgh
{

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
   c->dim = dim; c->NE = cfg->NE; c->D1D = cfg->D1D; c->Q1D = cfg->Q1D; c->L1D = cfg->L1D;
   c->ND = ipow(c->D1D, dim); c->NQ = ipow(c->Q1D, dim); c->NL = ipow(c->L1D, dim);
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

// mirror symmetry of the tables (every nodal or Bernstein basis on symmetric points has it); LGH_B_SYM=0: assume not
static void table_mirror_symmetry(const lgh_config *cfg, lgh_ctx *c)
{
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

// Tensor-product rule?  w[i] = W[i, 0, 0] / w[0]^(dim - 1) with w[0] = W[0]^(1/dim); every entry of W must be the
// product of its three factors to 8 ulp.  The plane-form L2 mass apply then takes the weights from Q scalars
// instead of NQ loads per element batch (compact mass data only: value(q, e) = s_e w[qx] w[qy] w[qz]).
static int tensor_rule_and_mass_tiles(const lgh_config *cfg, lgh_ctx *c)
{
   const int Q = c->Q1D, dim = c->dim;
   std::vector<double> w1((size_t)Q);
   const double w0 = (dim == 3) ? cbrt(cfg->weights[0]) : sqrt(cfg->weights[0]);
   bool ok = std::isfinite(w0) && w0 > 0.0;
   for (int i = 0; ok && i < Q; i++)
   {
      w1[i] = cfg->weights[i] / ipow(w0, dim - 1);
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
   if (!c->w1d || !c->sw.mass_kron) { return LGH_OK; } // (LGH_MASS_KRON=0, A/B: always contract through the quadrature points)
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
   return tile(cfg->B_l2, c->L1D, c->M1l);
}

// the transpose of the restriction (off, idx: its CSR form on the host) in ELL form
static int ell_transpose(lgh_ctx *c, const std::vector<int> &off, const std::vector<int> &idx)
{
   int deg = 0;
   for (int n = 0; n < c->N; n++) { deg = std::max(deg, off[(size_t)n + 1] - off[n]); }
   std::vector<int> ell((size_t)deg * c->N, -1);
   for (int n = 0; n < c->N; n++)
      for (int k = off[n]; k < off[(size_t)n + 1]; k++) { ell[(size_t)(k - off[n]) * c->N + n] = idx[k]; }
   c->t_deg = deg;
   return ctx_buffer(c->t_ell, ell.size(), ell.data());
}

// the quadrature data, the products of the fused update and the scratch of the operators and the CGs
static int quadrature_and_scratch_buffers(lgh_ctx *c)
{
   const int dim = c->dim;
   const size_t nq = (size_t)c->NE * c->NQ, nmap = (size_t)c->NE * c->ND, ne_nd = nmap * dim;
   LGH_PASS(ctx_buffer(c->stressJinvT, nq * dim * dim));
   LGH_PASS(ctx_buffer(c->Jac0inv, nq * dim * dim));
   LGH_PASS(ctx_buffer(c->Jac0inv_soa, nq * dim * dim));
   LGH_PASS(ctx_buffer(c->Jac0inv_e, (size_t)c->NE * dim * dim));
   LGH_PASS(ctx_buffer(c->rho0DetJ0w, nq));
   LGH_PASS(ctx_buffer(c->massD, nq + 2048)); // (one set of the matrix-core K1 behind the last element: its pipeline prefetches without predicates)
   LGH_PASS(ctx_buffer(c->diagV, (size_t)c->N));
   LGH_PASS(ctx_buffer(c->dinvV, (size_t)c->N));
   if (c->sw.fused_ftv) // (LGH_FUSED_FTV=0, A/B: F^T v always by its own kernel)
   {
      LGH_PASS(ctx_buffer(c->erhs_q, (size_t)c->L2V));
      LGH_PASS(ctx_buffer(c->v_snap, (size_t)c->H1V));
   }
   LGH_PASS(ctx_buffer(c->dev_flags, (size_t)8));
   // (LGH_FUSED_F1=0, A/B: F.1 always by its own kernel)
   if (dim == 3 && c->sw.fused_f1) { LGH_PASS(ctx_buffer(c->force_e_q, ne_nd + (size_t)dim * c->ND)); } // (+ a zero element: vcg_init_force_z_k)
   LGH_PASS(ctx_buffer(c->XE, std::max<size_t>(ne_nd, (size_t)c->L2V)));
   LGH_PASS(ctx_buffer(c->YE, ne_nd + (size_t)dim * c->ND)); // (+ a zero element: vcg_init_force_z_k)
   const size_t nv = std::max<size_t>((size_t)c->N, (size_t)c->L2V);
   LGH_PASS(ctx_buffer(c->cg_r, nv));
   LGH_PASS(ctx_buffer(c->cg_z, nv));
   LGH_PASS(ctx_buffer(c->cg_d0, nv));
   LGH_PASS(ctx_buffer(c->cg_d1, nv));
   return ctx_buffer(c->cg_y, nv);
}

// a 2D or 3D context
static int create_2d3d(const lgh_config *cfg, lgh_ctx *c)
{
   std::vector<int> off, idx; // the transpose of the restriction on the host
   LGH_PASS(create_common(cfg, c, off, idx));
   c->q_tiny_grad = c->sw.q_tiny_grad;
   c->q_discard = (c->sw.q_discard == 1) ? (kQDiscardDt | kQDiscardF1) : (c->sw.q_discard == 2) ? kQDiscardDt : (c->sw.q_discard == 3) ? kQDiscardF1 : 0;
   c->q_cF = q_force_bound(cfg);
   table_mirror_symmetry(cfg, c);
   LGH_PASS(tensor_rule_and_mass_tiles(cfg, c));
   LGH_PASS(ell_transpose(c, off, idx));
   if (cfg->owner) { LGH_PASS(c->owner.upload(cfg->owner, (size_t)c->N)); }
   return quadrature_and_scratch_buffers(c);
}

} // namespace lgh

using namespace lgh;

extern "C"
{

int lgh_create(const lgh_config *cfg, lgh_ctx **out)
{
   LGH_CHECK_ARG(cfg && out);
   LGH_CHECK_ARG(cfg->dim == 1 || cfg->dim == 2 || cfg->dim == 3);
   LGH_CHECK_ARG(cfg->NE > 0 && cfg->N > 0);
   LGH_CHECK_ARG(cfg->h1_map && cfg->B_h1 && cfg->G_h1 && cfg->B_l2 && cfg->weights && cfg->gamma);
   // MFEM_VERIFY(L1D==D1D-1) (laghos_assembly.cpp:533, :943)
   if (cfg->L1D != cfg->D1D - 1) { set_error("L1D!=D1D-1"); return LGH_ERR_UNSUPPORTED; }
   const int kid = (cfg->dim << 8) | (cfg->D1D << 4) | cfg->Q1D;
   const bool packed = (cfg->D1D & ~0xF) == 0 && (cfg->Q1D & ~0xF) == 0; // (four bits each: no other sizes alias one of the fifteen ids)
   if (!packed || !order_supported(kid)) { return unknown_kernel(kid); }
   int ndev = 0;
   if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
   {
      set_error("no HIP device available: the laghos_hip path requires an MI355X (gfx950) GPU");
      return LGH_ERR_HIP;
   }
   LGH_HIP_CHECK(hipSetDevice(cfg->device));
   // argument errors a caller can trigger are found before anything is allocated
   LGH_CHECK_ARG(cfg->cfl > 0.0); // (the time-step estimate is a minimum over cfl / inv_dt >= 0, folded as such: lgh_qrows.hpp)
   for (size_t i = 0, n = (size_t)cfg->NE * ipow(cfg->D1D, cfg->dim); i < n; i++)
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
   const int rc_create = (cfg->dim == 1) ? create_1d(cfg, c) : create_2d3d(cfg, c);
   if (rc_create != LGH_OK) { lgh_destroy(c); return rc_create; }
   *out = c;
   return LGH_OK;
}

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

} // extern "C"
