// lgh_api.hip — the operator-level entry points of the C ABI (include/laghos_hip.h) that have no file of their own: errors and
// version, quadrature data, mass and force operators, the dt estimate, the form queries and the lgh_test_* hooks.  (Context:
// lgh_context.hip; SolveVelocity: lgh_velocity.hip; SolveEnergy: lgh_energy.hip; vectors: lgh_vec.hip; timers: lgh_timing.hip.)
#include <chrono>
#include <cstdarg>

#include "lgh_common.hpp"

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
// Entry points with no 1D form (the 2D/3D kernel forms, the lockstep solve, E-vector test hooks) refuse a 1D context.
int no_1d(const lgh_ctx *c, const char *who)
{
   if (c->dim != 1) { return LGH_OK; }
   set_error("%s: not available for a 1D context (lgh_1d.hip has its own kernels)", who);
   return LGH_ERR_UNSUPPORTED;
}

} // namespace lgh

using namespace lgh;

extern "C"
{

const char *lgh_last_error(void) { return g_err; }
const char *lgh_version(void) { return "laghos_hip 0.1 (gfx950)"; }

static void invalidate_fused(lgh_ctx *c)
{
   c->fused_ftv_valid = 0;
   c->fused_f1_valid = 0;
   c->qgen++;
}
// the mass data may have changed: its compact form is looked for again at the next mass apply
static void mass_data_invalidated(lgh_ctx *c)
{
   c->mass_rank1 = -1;
   c->mass_gen++;
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
   mass_data_invalidated(c); // (the caller may write through this pointer)
   return c->massD;
}
int lgh_mass_data_form(lgh_ctx *c, int *form)
{
   LGH_CHECK_ARG(c && form);
   if (c->dim == 1) { *form = 0; return LGH_OK; } // (the 1D kernels read the stored table)
   const double *Dq, *Se;
   int dqs;
   LGH_PASS(mass_data(c, &Dq, &dqs, &Se));
   *form = (c->mass_rank1 == 1) ? 1 : 0;
   return LGH_OK;
}
int lgh_mass_data_changed(lgh_ctx *c)
{
   LGH_CHECK_ARG(c);
   mass_data_invalidated(c);
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
   LGH_PASS(host_wait_token(c, (volatile unsigned long long *)(c->host_pinned + kPinDtToken), token));
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
   mass_data_invalidated(c); // (new mass data)
   if (c->dim == 1) { LGH_PASS(setup_1d(c, x0, rho0_l2, rho0_q, volume)); } // (with the diagonal and the zone mass factors)
   else
   {
      LGH_PASS(setup_rho0detj0(c, x0, rho0_l2, rho0_q, volume));
      LGH_PASS(mass_assemble_diag(c));
   }
   c->setup_done = 1;
   return LGH_OK;
}

int lgh_force_mult(lgh_ctx *c, const double *x_l2, double *y_h1)
{
   LGH_CHECK_ARG(c && x_l2 && y_h1);
   // L2R->Mult is the identity for the lexicographic L2 space (assembly.cpp:559-560)
   LGH_PASS(stress_on_hand(c, "lgh_force_mult")); // (a refusal is taken before the timing sample opens)
   if (c->dim == 1) { return force_mult_1d(c, x_l2, y_h1); }
   kt_begin(c, LGH_KERNEL_FORCE_MULT);
   const int rc = force_mult_E(c, c->stressJinvT, x_l2, c->YE);
   kt_end(c, LGH_KERNEL_FORCE_MULT);
   if (rc) { return rc; }
   LGH_PASS(h1_transpose_gather(c, c->dim, c->YE, y_h1)); // H1R->MultTranspose (:564)
   return (c->multi != 0) ? halo_sum(c, y_h1, c->dim) : LGH_OK;
}
int lgh_force_mult_transpose(lgh_ctx *c, const double *v_h1, double *y_l2)
{
   LGH_CHECK_ARG(c && v_h1 && y_l2);
   LGH_PASS(stress_on_hand(c, "lgh_force_mult_transpose"));
   if (c->dim == 1) { return force_mult_t_1d(c, v_h1, y_l2); }
   KtScope sample(c, LGH_KERNEL_FORCE_MULT_T);
   return force_mult_t_L(c, c->stressJinvT, v_h1, y_l2);
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
static int mass_mult(lgh_ctx *c, int space, const double *x, double *y, bool eliminate)
{
   LGH_CHECK_ARG(c && x && y && (space == LGH_SPACE_H1 || space == LGH_SPACE_L2));
   if (c->dim == 1) { return mass_apply_1d(c, space, x, y, eliminate); }
   return space == LGH_SPACE_H1 ? mass_apply_h1(c, x, y, eliminate) : mass_apply_l2(c, x, y);
}
int lgh_mass_mult(lgh_ctx *c, int space, const double *x, double *y) { return mass_mult(c, space, x, y, true); }
int lgh_mass_mult_full(lgh_ctx *c, int space, const double *x, double *y) { return mass_mult(c, space, x, y, false); }

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

int lgh_tg_source_2d(lgh_ctx *c, const double *S, double *e_source)
{
   LGH_CHECK_ARG(c && S && e_source);
   LGH_PASS(no_1d(c, "lgh_tg_source_2d"));
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
   LGH_PASS(no_1d(c, "lgh_test_vcg_k1"));
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
   LGH_PASS(no_1d(c, "lgh_vcg_layout_stats"));
   return vcg_layout_stats(c, out);
}
int lgh_test_vcg_merged_faces(lgh_ctx *c, unsigned char *mask, long *n_merged)
{
   LGH_CHECK_ARG(c && mask && n_merged);
   LGH_PASS(no_1d(c, "lgh_test_vcg_merged_faces"));
   return vcg_test_merged_faces(c, mask, n_merged);
}
int lgh_test_vcg_k2(lgh_ctx *c, int it, const double *y_E, double *r, double *d, double *x, const double den[3], const double rz[3],
                    const double rz_prev[3], const double alpha_prev[3], double rz_out[3], int *deferred_x)
{
   LGH_CHECK_ARG(c && it >= 1 && y_E && r && d && x && den && rz && rz_prev && alpha_prev && rz_out && deferred_x);
   LGH_PASS(no_1d(c, "lgh_test_vcg_k2"));
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
   LGH_PASS(no_1d(c, "lgh_force_mult_E"));
   return force_mult_E(c, sJit, x_E, y_E);
}
int lgh_force_mult_transpose_E(lgh_ctx *c, const double *sJit, const double *v_E, double *y_E)
{
   LGH_CHECK_ARG(c && sJit && v_E && y_E);
   LGH_PASS(no_1d(c, "lgh_force_mult_transpose_E"));
   return force_mult_t_E(c, sJit, v_E, y_E);
}
int lgh_mass_apply_E(lgh_ctx *c, int space, const double *x_E, double *y_E)
{
   LGH_CHECK_ARG(c && x_E && y_E);
   LGH_PASS(no_1d(c, "lgh_mass_apply_E"));
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
