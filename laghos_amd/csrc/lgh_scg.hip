// lgh_scg.hip — the device-resident scalar CG on the mass operators of lgh_mass.hip: one run object (ScalarCg) and three
// steps (scg_begin, scg_enqueue, scg_finish).  cg_solve, the split L2 solve of the energy equation (cg_l2_begin / _end) and
// its lockstep form are written on them.
//
// Replaces the two CGSolver instances configured at laghos_solver.cpp:264-284 (algorithm: SURVEY §3.2).
//
// MI355X design: one CG iteration is two kernels and no host round trip.
//   K1 (element batches): beta = rz/rz_prev; the new direction d = z + beta*d is
//       formed on the fly inside the gather (not stored: elements sharing a node
//       all read the old z, d); y_e = B^T D B d_e with the z contraction in
//       registers and tables in SGPRs; den = sum_e d_e.y_e (the E-vector form of
//       (d, A d), so no extra pass over the L-vector is needed).
//   K2 (nodes): forms the same d = z + beta*d in place (one thread per node, no
//       race), z = sum of element contributions (deterministic gather over an
//       ELL-format transpose, coalesced index loads, no atomics), essential rows
//       zeroed, alpha = rz/den, x += alpha d, r -= alpha z, z = r/diag,
//       betanom = (r,z) with a wave64 shuffle reduction; the last block to
//       finish folds the block partials in fixed order, updates the device
//       scalars and the convergence flag.
// The host only enqueues iterations in chunks and looks at the flag between
// chunks; once `done` is set the remaining kernels of a chunk exit immediately.
#include <algorithm>

#include "lgh_mass.hpp"

namespace lgh
{

// ---------------------------------------------------------------------------
// CG node / vector kernels
// ---------------------------------------------------------------------------
struct CgVecArgs
{
   int n;              // N (H1) or L2V
   const int *ell;     // H1 fused gather (ELL transpose; null: y already an L-vector)
   int deg;
   const double *YE;   // E-vector from K1 (H1) ...
   double *yL;         // ... or the operator result as an L-vector (L2, multi-GPU H1, atomics)
   int d_in_place;     // 1: d already holds the new direction (L2); 0: form z + beta d here
   const uint8_t *ess; // essential mask or null
   const double *dinv; // Jacobi (null: no preconditioner)
   const double *owner;// ownership weights or null
   const double *b;
   double *d;
   double *x, *r, *z;
   CgScalars *cgs;
   double *partials;
   unsigned int *ticket;
   int iter;
   int allreduce_pending; // multi-GPU: the scalar fold is finished by a later kernel
};

// init: r = b - A x (A x supplied in yL/YE, or absent when x == 0), z = M^-1 r,
// nom = (z, r); sets r0, done, rz.
template <bool HAVE_AX>
__global__ void __launch_bounds__(256)
cg_init_k(const CgVecArgs a)
{
   __shared__ double red[16];
   const int n = blockIdx.x * blockDim.x + threadIdx.x;
   double part = 0.0;
   if (n < a.n)
   {
      double rv = a.b[n];
      if (HAVE_AX) { rv -= a.yL[n]; }
      a.r[n] = rv;
      double zv = rv;
      if (a.dinv)
      {
         zv = rv * a.dinv[n];
         a.z[n] = zv;
      }
      part = (a.owner ? a.owner[n] : 1.0) * zv * rv;
   }
   const double bsum = block_sum(part, red);
   double total;
   if (grid_sum_last_block(bsum, a.partials, a.ticket, red, total))
   {
      if (threadIdx.x == 0)
      {
         CgScalars *s = a.cgs;
         s->rz = total;
         s->rz_prev = total;
         s->nom0 = total;
         s->iters = 0;
         s->first = 1;
         if (!a.allreduce_pending)
         {
            s->r0 = fmax(total * s->rel_tol2, 0.0);
            s->done = (total < 0.0 || total <= s->r0) ? 1 : 0;
         }
      }
   }
}

// multi-GPU: after the all-reduce of rz (init) finish the scalar bookkeeping
__global__ void cg_init_finish_k(CgScalars *s)
{
   s->rz_prev = s->rz;
   s->nom0 = s->rz;
   s->r0 = fmax(s->rz * s->rel_tol2, 0.0);
   s->done = (s->rz < 0.0 || s->rz <= s->r0) ? 1 : 0;
}

// K2: see file header.
// U nodes per thread with every load of all U nodes issued before first use: the
// kernel is pure memory latency (PMC: 90 % of wave cycles waiting), so the number
// of independent loads in flight per lane is what sets its speed.
constexpr int kUpdU = 2;
template <bool FUSED_GATHER, int DEG>
__global__ void __launch_bounds__(256)
cg_update_k(const CgVecArgs a)
{
   __shared__ double red[16];
   if (a.cgs->done) { return; }
   if (a.allreduce_pending && cg_pending_den(a.cgs, blockIdx.x == 0 && threadIdx.x == 0)) { return; }
   const double alpha = a.cgs->rz / a.cgs->den;
   // `first` was cleared by K1 of this iteration: iteration 1 is recognised by iter
   const bool it1 = (a.iter == 1);
   const double beta = it1 ? 0.0 : a.cgs->rz / a.cgs->rz_prev;
   const int base = blockIdx.x * (256 * kUpdU) + threadIdx.x;
   int n[kUpdU];
   bool ok[kUpdU];
#pragma unroll
   for (int k = 0; k < kUpdU; k++)
   {
      n[k] = base + 256 * k;
      ok[k] = n[k] < a.n;
      if (!ok[k]) { n[k] = a.n - 1; }
   }
   // ---- phase 1: issue all independent loads
   int pidx[kUpdU][DEG > 0 ? DEG : 1];
   if (FUSED_GATHER)
   {
#pragma unroll
      for (int k = 0; k < kUpdU; k++)
#pragma unroll
         for (int j = 0; j < DEG; j++) { pidx[k][j] = (j < a.deg) ? a.ell[(size_t)j * a.n + n[k]] : -1; }
   }
   double zold[kUpdU], dold[kUpdU], xo[kUpdU], ro[kUpdU], di[kUpdU], ow[kUpdU], zv[kUpdU];
   bool es[kUpdU];
#pragma unroll
   for (int k = 0; k < kUpdU; k++)
   {
      ro[k] = a.r[n[k]];
      xo[k] = a.x[n[k]];
      di[k] = a.dinv ? a.dinv[n[k]] : 1.0;
      zold[k] = a.dinv ? a.z[n[k]] : ro[k];
      dold[k] = (a.d_in_place || !it1) ? a.d[n[k]] : 0.0;
      ow[k] = a.owner ? a.owner[n[k]] : 1.0;
      es[k] = a.ess ? (a.ess[n[k]] != 0) : false;
      if (!FUSED_GATHER) { zv[k] = a.yL[n[k]]; }
   }
   // ---- phase 2: dependent E-vector reads
   if (FUSED_GATHER)
   {
      double ye[kUpdU][DEG > 0 ? DEG : 1];
#pragma unroll
      for (int k = 0; k < kUpdU; k++)
#pragma unroll
         for (int j = 0; j < DEG; j++) { ye[k][j] = (pidx[k][j] >= 0) ? a.YE[pidx[k][j]] : 0.0; }
#pragma unroll
      for (int k = 0; k < kUpdU; k++)
      {
         // ascending contribution order, skipping absent slots (same sum as the CSR loop)
         double s = 0.0;
#pragma unroll
         for (int j = 0; j < DEG; j++) { if (pidx[k][j] >= 0) { s += ye[k][j]; } }
         zv[k] = s;
      }
   }
   // ---- phase 3: updates
   double part = 0.0;
#pragma unroll
   for (int k = 0; k < kUpdU; k++)
   {
      if (!ok[k]) { continue; }
      const double z_ = es[k] ? 0.0 : zv[k];
      double dv;
      if (a.d_in_place) { dv = dold[k]; }
      else
      {
         // same expression as K1's gather: d = z_old + beta * d_old
         dv = zold[k];
         if (!it1) { dv += beta * dold[k]; }
         a.d[n[k]] = dv;
      }
      const double xv = xo[k] + alpha * dv;
      const double rv = ro[k] - alpha * z_;
      a.x[n[k]] = xv;
      a.r[n[k]] = rv;
      double pz = rv;
      if (a.dinv)
      {
         pz = rv * di[k];
         a.z[n[k]] = pz;
      }
      part += ow[k] * rv * pz;
   }
   const double bsum = block_sum(part, red);
   double total;
   if (grid_sum_last_block(bsum, a.partials, a.ticket, red, total))
   {
      if (threadIdx.x == 0)
      {
         CgScalars *s = a.cgs;
         s->rz_prev = s->rz;
         s->rz = total; // betanom
         if (!a.allreduce_pending)
         {
            s->iters = a.iter;
            if (total < 0.0 || total <= s->r0) { s->done = 1; }
         }
      }
   }
}
// (several ranks) a finished solve leaves rz = den = 0: the exchanges of the launches the host enqueued past
// convergence then sum zeros instead of multiplying the global values by the number of ranks each time
__global__ void cg_update_finish_k(CgScalars *s, int iter)
{
   if (s->done) { s->rz = 0.0; s->den = 0.0; return; }
   s->iters = iter;
   if (s->rz < 0.0 || s->rz <= s->r0) { s->done = 1; s->rz = 0.0; s->den = 0.0; }
}

__global__ void cg_set_tol_k(CgScalars *s, double rel_tol2)
{
   s->rel_tol2 = rel_tol2;
   s->done = 0;
   s->first = 1;
   s->iters = 0;
}

// ---------------------------------------------------------------------------
// host side: one run, three steps
// ---------------------------------------------------------------------------
struct ScalarCg
{
   int space;
   CgVecArgs v;
   MassArgs m;
   int it, max_iter; // iterations enqueued so far; the cap
   int nbu;          // grid of cg_update_k (kUpdU nodes per thread)
   int *last;        // the slot of cg_last_iters the chunk schedule starts from and the count goes back to
   bool active;      // begun and not finished
};

// Set-up and initial residual: r = b - A x (iterative_mode for H1; L2 starts from x = 0: solvers.cpp), z = M^-1 r, nom = (z, r).
// No iteration is enqueued.
static int scg_begin(lgh_ctx *c, ScalarCg *r, int space, const double *b, double *x, double rel_tol, int max_iter, bool x_is_zero)
{
   const bool h1 = (space == LGH_SPACE_H1);
   const int n = h1 ? c->N : c->L2V;
   const bool multi = (c->multi != 0); // (the split L2 solve on several ranks: the caller has checked that its stream has a communicator)
   int rc;
   *r = ScalarCg{};
   r->space = space;
   r->max_iter = max_iter;
   r->nbu = ceil_div(n, 256 * kUpdU);
   r->last = &c->cg_last_iters[h1 ? 0 : 1][(h1 && c->cur_ess >= 0) ? c->cur_ess : 0];
   hipLaunchKernelGGL(cg_set_tol_k, dim3(1), dim3(1), 0, c->stream, c->cgs, rel_tol * rel_tol);

   CgVecArgs &v = r->v;
   v.n = n;
   v.b = b;
   v.x = x;
   v.r = c->cg_r;
   v.z = h1 ? c->cg_z : c->cg_r; // no preconditioner: z aliases r
   v.d = c->cg_d0;
   v.d_in_place = h1 ? 0 : 1;
   v.dinv = h1 ? c->dinvV : nullptr;
   v.owner = (h1 && multi) ? c->owner : nullptr;
   v.ess = (h1 && c->cur_ess >= 0) ? c->essmask[c->cur_ess] : nullptr;
   if (h1 && !multi)
   {
      v.ell = c->t_ell;
      v.deg = c->t_deg;
      v.YE = c->YE;
   }
   if (!h1) { v.yL = c->cg_y; }
   v.cgs = c->cgs;
   v.partials = c->partials;
   v.ticket = c->tickets;
   v.allreduce_pending = multi ? 1 : 0;

   const int nb = ceil_div(n, 256);
   if (!h1) { rc = vec_set(c, x, 0.0, n); if (rc) { return rc; } x_is_zero = true; }
   if (!x_is_zero)
   {
      rc = mass_apply_h1(c, x, c->cg_y, true);
      if (rc) { return rc; }
      v.yL = c->cg_y;
      hipLaunchKernelGGL(cg_init_k<true>, dim3(nb), dim3(256), 0, c->stream, v);
   }
   else { hipLaunchKernelGGL(cg_init_k<false>, dim3(nb), dim3(256), 0, c->stream, v); }
   LGH_HIP_CHECK(hipGetLastError());
   if (multi)
   {
      rc = allreduce_dev(c, &c->cgs->rz, 1, 0);
      if (rc) { return rc; }
      hipLaunchKernelGGL(cg_init_finish_k, dim3(1), dim3(1), 0, c->stream, c->cgs);
   }

   MassArgs &m = r->m;
   m = base_args(c, space);
   m.x = h1 ? c->cg_z : c->cg_r;
   m.map = h1 ? c->h1map : nullptr;
   m.y = h1 ? c->YE : c->cg_y;
   m.d = c->cg_d0;
   m.cgs = c->cgs;
   m.partials = c->partials + c->part_stride;
   m.ticket = c->tickets + 1 * kTicketSlot;
   m.multi = multi ? 1 : 0;
   m.no_y = (!h1 && l2_fused_update(c)) ? 1 : 0;
   r->active = true;
   return LGH_OK;
}

// The iteration body: iterations it + 1 .. upto, enqueued only.
static int scg_enqueue(lgh_ctx *c, ScalarCg *r, int upto)
{
   const bool h1 = (r->space == LGH_SPACE_H1);
   const bool multi = (r->m.multi != 0);
   MassArgs &m = r->m;
   CgVecArgs &v = r->v;
   int rc;
   for (; r->it < upto;)
   {
      ++r->it;
      m.iter = r->it;
      v.iter = r->it;
      {
         KtScope kt(c, h1 ? LGH_KERNEL_MASS_CG_H1 : LGH_KERNEL_MASS_CG_L2);
         rc = mass_apply_cg(c, r->space, m);
      }
      if (rc) { return rc; }
      if (h1 && !multi)
      {
         KtScope kt(c, LGH_KERNEL_CG_UPDATE_H1);
         if (c->t_deg <= 4) { hipLaunchKernelGGL((cg_update_k<true, 4>), dim3(r->nbu), dim3(256), 0, c->stream, v); }
         else if (c->t_deg <= 8) { hipLaunchKernelGGL((cg_update_k<true, 8>), dim3(r->nbu), dim3(256), 0, c->stream, v); }
         else
         {
            // unusual valence (not a tensor-product mesh): unfused gather, then update
            rc = mass_gather(c, c->YE, nullptr, c->cg_y);
            if (rc) { return rc; }
            v.yL = c->cg_y;
            hipLaunchKernelGGL((cg_update_k<false, 0>), dim3(r->nbu), dim3(256), 0, c->stream, v);
         }
      }
      else
      {
         if (h1)
         {
            // multi-GPU: assemble the L-vector, sum shared nodes, reduce den
            rc = mass_gather(c, c->YE, nullptr, c->cg_y);
            if (rc) { return rc; }
            rc = halo_sum(c, c->cg_y, 1);
            if (rc) { return rc; }
            v.yL = c->cg_y;
         }
         if (multi)
         {
            rc = allreduce_dev(c, &c->cgs->den, 1, 0); // breakdown is looked at by the update (cg_pending_den)
            if (rc) { return rc; }
         }
         if (!h1 && m.no_y) { rc = mass_l2_fused_update(c, m, v.x, v.r, v.partials, v.ticket); if (rc) { return rc; } } // (the update forms M d of its zones itself)
         else { hipLaunchKernelGGL((cg_update_k<false, 0>), dim3(r->nbu), dim3(256), 0, c->stream, v); }
         if (multi)
         {
            rc = allreduce_dev(c, &c->cgs->rz, 1, 0); // convergence is looked at by the next K1 (cg_pending_update)
            if (rc) { return rc; }
         }
      }
      LGH_HIP_CHECK(hipGetLastError());
   }
   return LGH_OK;
}

// The look loop: looks at the convergence flag, enqueues a chunk, looks again, until the solve has converged or reached its
// cap.  chunk = iterations enqueued between two looks.  The iteration count of a mass solve barely changes from one RK stage
// to the next, so the first chunk is the previous count for this (space, component): the common case costs two host round
// trips and no wasted launches; kernels enqueued past convergence exit on the device-side `done` flag.
// look_first: the first look stands in front of the first chunk (cg_solve: a right-hand side of zero enqueues nothing);
// otherwise the caller has enqueued the first chunk already and that look is folded into the one behind it (the split solve).
static int scg_finish(lgh_ctx *c, ScalarCg *r, bool look_first, int first_chunk, int *iters)
{
   CgScalars *hs = (CgScalars *)c->host_pinned;
   int looks = 0, chunk = first_chunk;
   while (true)
   {
      // several ranks: the outcome of the last enqueued update is still pending (cg_pending_update) - commit it
      if (r->m.multi && r->it > 0) { hipLaunchKernelGGL(cg_update_finish_k, dim3(1), dim3(1), 0, c->stream, c->cgs, r->it); }
      LGH_HIP_CHECK(hipMemcpyAsync(hs, c->cgs, sizeof(CgScalars), hipMemcpyDeviceToHost, c->stream));
      LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
      if (hs->done || r->it >= r->max_iter) { break; }
      // after the first chunk (the previous solve's count): two more iterations per look while the count only creeps, then
      // doubling - a solve whose count jumps (the unpreconditioned L2 CG of the first steps at order 4: 225 -> 300) must not pay
      // a host look every two iterations (round 6: 149 looks per RK step at config 5); launches past convergence return at once
      if (!look_first) { chunk = (++looks <= 2) ? 2 : std::min(64, 2 * chunk); }
      look_first = false;
      const int rc = scg_enqueue(c, r, std::min(r->max_iter, r->it + chunk));
      if (rc) { return rc; }
   }
   // upstream: final_iter = max_iter when the loop runs out without converging
   int fin = hs->iters;
   if (!hs->done && r->it >= r->max_iter) { fin = r->max_iter; }
   *r->last = fin;
   if (iters) { *iters = fin; }
   r->active = false;
   return LGH_OK;
}

int cg_solve(lgh_ctx *c, int space, const double *b, double *x, double rel_tol, int max_iter,
             int *iters, bool x_is_zero)
{
   ScalarCg run;
   const int rc = scg_begin(c, &run, space, b, x, rel_tol, max_iter, x_is_zero);
   if (rc) { return rc; }
   const int last = *run.last;
   return scg_finish(c, &run, true, last > 0 ? last : 8, iters);
}

// ---- the L2 (energy) solve split into an enqueue-only half and a completing half -----
// SolveEnergy (laghos_solver.cpp:400-493) needs only the quadrature data and the
// velocity block of S - not the result of SolveVelocity.  lgh_solve_energy_begin
// enqueues F^T v and the first chunk of CG iterations on the context's second stream
// (the caller swaps the stream in), the velocity solve then runs on the main stream
// with its host round trips, and lgh_solve_energy_end looks at the convergence flag.
// The steps of cg_solve(LGH_SPACE_L2) on the context's run: the iterates are identical,
// only the initial look (rhs == 0) is folded into the first one.
static int cg_l2_begin_impl(lgh_ctx *c, const double *b, double *x, double rel_tol, int max_iter, const bool enqueue)
{
   if (!c->l2run) { c->l2run.reset(new ScalarCg()); }
   ScalarCg *r = c->l2run.get();
   const int rc = scg_begin(c, r, LGH_SPACE_L2, b, x, rel_tol, max_iter, true);
   if (rc || !enqueue) { return rc; } // (lockstep: the velocity solve interleaves the iterations)
   const int last = *r->last;
   return scg_enqueue(c, r, std::min(max_iter, last > 0 ? last : 8));
}
int cg_l2_begin(lgh_ctx *c, const double *b, double *x, double rel_tol, int max_iter) { return cg_l2_begin_impl(c, b, x, rel_tol, max_iter, true); }
int cg_l2_end(lgh_ctx *c, int *iters)
{
   ScalarCg *r = c->l2run.get();
   if (!r || !r->active) { return LGH_ERR_ARG; }
   return scg_finish(c, r, false, 0, iters);
}
void cg_l2_free(ScalarCg *r) { delete r; } // (the deleter of lgh_ctx::l2run: the type is known here only)

// ---- lockstep with the velocity CG (lgh_common.hpp): set-up and initial residual here, one iteration per velocity
// iteration from inside vcg_solve (apply behind K1, update behind K2), the rest - if any - by cg_l2_end as before
bool l2_lockstep_possible(lgh_ctx *c) { return l2_fused_update(c); }
int l2_lockstep_limit(lgh_ctx *c)
{
   const ScalarCg *r = c->l2run.get();
   const int last = c->cg_last_iters[1][0];
   const int want = last > 0 ? last : 8;
   return (r && r->active) ? std::min(want, r->max_iter) : 0; // (never past the cap this solve was given)
}
int cg_l2_begin_lockstep(lgh_ctx *c, const double *b, double *x, double rel_tol, int max_iter) { return cg_l2_begin_impl(c, b, x, rel_tol, max_iter, false); }
int l2_lockstep_apply(lgh_ctx *c, int it, const LockstepWords &prev, double *den_mirror)
{
   ScalarCg *r = c->l2run.get();
   if (!r || !r->active || !r->m.no_y || it != r->it + 1 || it > r->max_iter) { set_error("l2_lockstep_apply: no energy solve set up for iteration %d", it); return LGH_ERR_ARG; }
   ++r->it;
   r->m.iter = r->it;
   r->m.ls = prev;
   r->m.ls_on = 1;
   r->m.ls_den_mirror = den_mirror;
   return mass_apply_cg(c, LGH_SPACE_L2, r->m);
}
int l2_lockstep_update(lgh_ctx *c, int it, const double *den_src, long long *word_out)
{
   ScalarCg *r = c->l2run.get();
   if (!r || !r->active || it != r->it) { set_error("l2_lockstep_update: iteration %d has no apply", it); return LGH_ERR_ARG; }
   r->v.iter = r->it;
   MassArgs m = r->m;
   m.ls_on = 1;
   m.ls_den_src = den_src;
   m.ls_word_out = word_out;
   return mass_l2_fused_update(c, m, r->v.x, r->v.r, r->v.partials, r->v.ticket);
}
__global__ void l2_lockstep_fold_k(CgScalars *s, const int it, const LockstepWords w)
{
   if (s->done) { return; }
   (void)lockstep_pending_update(s, it + 1, lockstep_rz(w), true); // what the apply of iteration it + 1 would commit
}
int l2_lockstep_fold(lgh_ctx *c, int it, const LockstepWords &last)
{
   ScalarCg *r = c->l2run.get();
   if (!r || !r->active || it != r->it) { set_error("l2_lockstep_fold: iteration %d is not the last one enqueued", it); return LGH_ERR_ARG; }
   hipLaunchKernelGGL(l2_lockstep_fold_k, dim3(1), dim3(1), 0, c->stream, c->cgs, it, last);
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}
int cg_l2_end_lockstep(lgh_ctx *c, int *iters)
{
   ScalarCg *r = c->l2run.get();
   if (!r || !r->active) { return LGH_ERR_ARG; }
   r->m.ls_on = 0; // (from here on the solve reduces its scalars itself: the sequence of cg_solve)
   r->m.ls_den_mirror = nullptr;
   const int inside = r->it;
   const int rc = cg_l2_end(c, iters);
   c->ls_stats[0] += 1;
   c->ls_stats[1] += inside;
   c->ls_stats[2] += r->it - inside;
   return rc;
}

} // namespace lgh
