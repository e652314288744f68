// lgh_velocity.hip — SolveVelocity (laghos_solver.cpp:329-399, PA branch; the 1D FA branch goes to lgh_1d.hip): where F.1 comes
// from (force_one_E), how the right-hand side is formed (inside the first kernel of the lockstep CG, or by separate kernels),
// which CG runs (the lockstep one where the kernel id has it, else one scalar CG per component), one iteration accounting.
#include "lgh_common.hpp"

using namespace lgh;

extern "C"
{

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
      LGH_PASS(vec_set(c, c->ones_l2, 1.0, c->L2V));
   }
   *out = c->ones_l2;
   return LGH_OK;
}
// F.1 up to the E-vector (:354), the one place that decides where it comes from: formed by the fused update for this very
// state, or by the force kernel (into YE)
static int force_one_E(lgh_ctx *c, const double *one_l2, const double **force_E)
{
   *force_E = c->YE;
   if (c->force_e_q && c->fused_f1_valid && is_the_one_vector(c, one_l2)) { *force_E = c->force_e_q; return LGH_OK; }
   const double *ones = nullptr;
   LGH_PASS(one_vector(c, one_l2, &ones));
   LGH_PASS(stress_on_hand(c, "lgh_solve_velocity (F.1 of a vector other than one, or of changed quadrature data)")); // (a refusal is taken before the timing sample opens)
   KtScope sample(c, LGH_KERNEL_FORCE_MULT);
   return force_mult_E(c, c->stressJinvT, ones, c->YE);
}
// The right-hand side by separate kernels, the reference's regions kept apart: dv = 0, F.1 summed to the L-vector, the
// negation, the acceleration source, EliminateRHS (in place: callers read rhs_h1 with its essential rows zeroed).
static int rhs_by_kernels(lgh_ctx *c, const double *one_l2, double *rhs_h1, double *work_B, double *dv)
{
   const int dim = c->dim, N = c->N;
   LGH_PASS(vec_set(c, dv, 0.0, c->H1V)); // dv = 0.0 (:338)
   {
      RoctxRange range("SolveVelocity-ForcePA"); // laghos_solver.cpp:353-356
      timer_start(c);
      const double *force_E = nullptr;
      int rc = force_one_E(c, one_l2, &force_E);
      if (rc == LGH_OK) { rc = h1_transpose_gather(c, dim, force_E, rhs_h1); } // H1R->MultTranspose (:564)
      if (rc == LGH_OK && c->multi != 0) { rc = halo_sum(c, rhs_h1, dim); }
      timer_stop(c, 2);
      if (rc) { return rc; }
   }
   LGH_PASS(vec_neg_inplace(c, rhs_h1, c->H1V)); // :358
   for (int cc = 0; c->accel_src && cc < dim; cc++) // source_type == 2: B_c += VMassPA->MultFull(accel_c) (:371-380), before EliminateRHS
   {
      LGH_PASS(mass_apply_h1(c, c->accel_src + (size_t)cc * N, work_B, false));
      LGH_PASS(vec_axpby(c, rhs_h1 + (size_t)cc * N, 1.0, rhs_h1 + (size_t)cc * N, 1.0, work_B, N));
   }
   for (int cc = 0; cc < dim; cc++)
   {
      LGH_PASS(vec_zero_list(c, rhs_h1 + (size_t)cc * N, c->ess[cc], c->ess_count[cc])); // EliminateRHS with c_tdofs[cc] (:383-384); rhs_h1 is caller scratch
   }
   return LGH_OK;
}

int lgh_set_velocity_source(lgh_ctx *c, const double *accel_h1)
{
   LGH_CHECK_ARG(c);
   if (accel_h1) { LGH_PASS(no_1d(c, "lgh_set_velocity_source")); } // (problem 7 has no 1D form)
   c->accel_src = accel_h1;
   return LGH_OK;
}

// The caller has already run UpdateQuadratureData(S) if the data was stale (:332).
int lgh_solve_velocity(lgh_ctx *c, const double *S, double *dS_dt, const double *one_l2,
                       double *rhs_h1, double *work_B, double rel_tol, int max_iter, int *h1_iters)
{
   LGH_CHECK_ARG(c && S && dS_dt && rhs_h1 && work_B);
   const int dim = c->dim, N = c->N;
   double *dv = dS_dt + c->H1V;
   if (dim == 1) // the FA branch (laghos_solver.cpp:400-439; lgh_1d.hip)
   {
      LGH_CHECK_ARG(!c->accel_src);
      const double *ones = nullptr;
      LGH_PASS(one_vector(c, one_l2, &ones));
      LGH_PASS(stress_on_hand(c, "lgh_solve_velocity"));
      return solve_velocity_1d(c, ones, dv, rhs_h1, rel_tol, max_iter, h1_iters);
   }
   // One rank, region timers off, no acceleration source: the E->L sum of F.1, the negation, EliminateRHS, dv = 0 and the CG
   // initialisation are one kernel (vcg_init_force_k, the first of the lockstep CG), with bit-identical results.
   const double *force_E = nullptr; // (set: the lockstep CG forms the right-hand side from it)
   if (!c->timers.enabled && !c->accel_src && vcg_fused_init_ok(c)) { LGH_PASS(force_one_E(c, one_l2, &force_E)); }
   else { LGH_PASS(rhs_by_kernels(c, one_l2, rhs_h1, work_B, dv)); }
   int its[3] = {0, 0, 0};
   RoctxRange range("SolveVelocity-CGVMass"); // laghos_solver.cpp:387-390
   if (vcg_available(c)) // the dim component solves in lockstep (lgh_vcg.hip) when the kernel id has it
   {
      timer_start(c);
      LGH_PASS(vcg_solve(c, rhs_h1, dv, rel_tol, max_iter, its, force_E)); // :358-388 for all components
      timer_stop(c, 0);
   }
   else
   {
      for (int cc = 0; cc < dim; cc++)
      {
         // B = rhs_c, eliminated above (Pconf is the identity on a conforming mesh; shared-node sums were already applied) (:368-369)
         LGH_HIP_CHECK(hipMemcpyAsync(work_B, rhs_h1 + (size_t)cc * N, sizeof(double) * N, hipMemcpyDeviceToDevice, c->stream));
         LGH_PASS(lgh_mass_set_essential_tdofs(c, cc)); // :383 (the constrained mass apply reads cur_ess)
         timer_start(c);
         const int rc = cg_solve(c, LGH_SPACE_H1, work_B, dv + (size_t)cc * N, rel_tol, max_iter, &its[cc], true); // :388
         timer_stop(c, 0);
         if (rc) { return rc; }
      }
   }
   for (int cc = 0; cc < dim; cc++)
   {
      c->timers.c[0] += its[cc]; // :392
      if (h1_iters) { *h1_iters += its[cc]; }
   }
   c->cur_ess = dim - 1;
   return LGH_OK;
}

} // extern "C"
