// lgh_energy.hip — SolveEnergy (laghos_solver.cpp:400-493, PA branch): the right-hand side F^T v, the L2 mass solve, and
// the three ways the solve runs beside or behind the velocity solve between lgh_solve_energy_begin and _end.  One state
// object (EnergySolve, lgh_common.hpp), one decision (energy_mode).
#include <algorithm>

#include "lgh_common.hpp"

extern "C"
{

// ForcePA->MultTranspose(v, e_rhs) of SolveEnergy (laghos_solver.cpp:473).  The fused QUpdate has formed F^T v for the
// velocity of the state it was called for; it stands in for the kernel exactly when the quadrature data is still that
// of this update AND the v passed now equals that velocity element for element - compared on the device, whatever the
// address (RK2Avg's averaged velocity, or a state changed in place since, go through the kernel, as in the reference).
// No host look: the comparison leaves a flag, the force kernel returns at once when it is 0, the copy when it is not.
__global__ void __launch_bounds__(256) vec_differs_k(const double *__restrict__ a, const double *__restrict__ b, const long n, int *flag)
{
   // (compared as bit patterns: -0.0 vs 0.0 or a NaN payload count as different - the kernel then simply runs)
   // grid-stride, 16-byte loads where both vectors allow them (round 5: one element per thread reached 2 TB/s at 64^3)
   const long stride = (long)gridDim.x * blockDim.x, t = (long)blockIdx.x * blockDim.x + threadIdx.x;
   bool diff = false;
   if (((((uintptr_t)a) | ((uintptr_t)b)) & 15u) == 0)
   {
      const longlong2 *a2 = (const longlong2 *)a, *b2 = (const longlong2 *)b;
      for (long i = t; i < n / 2; i += stride)
      {
         const longlong2 p = a2[i], q = b2[i];
         diff = diff || p.x != q.x || p.y != q.y;
      }
      if ((n & 1) && t == 0) { diff = diff || __double_as_longlong(a[n - 1]) != __double_as_longlong(b[n - 1]); }
   }
   else
   {
      for (long i = t; i < n; i += stride) { diff = diff || __double_as_longlong(a[i]) != __double_as_longlong(b[i]); }
   }
   if (diff) { *flag = 1; }
}
// e_rhs = F^T v of the quadrature update unless the velocity differs from the one it was formed for; then (the stress being in
// registers only) NaN and the error word (rounds 3-4: two launches, poison and copy)
__global__ void __launch_bounds__(256) erhs_take_or_poison_k(double *__restrict__ y, const double *__restrict__ x, const long n, const int *__restrict__ flag, int *err)
{
   const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
   if (*flag != 0)
   {
      if (i < n) { y[i] = __builtin_nan(""); }
      if (i == 0) { *err = 1; }
      return;
   }
   if (i < n) { y[i] = x[i]; }
}
__global__ void __launch_bounds__(256) copy_unless_k(double *__restrict__ y, const double *__restrict__ x, const long n, const int *__restrict__ flag)
{
   if (*flag != 0) { return; }
   const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
   if (i < n) { y[i] = x[i]; }
}

} // extern "C" (the kernels keep the symbol names they have had)

namespace lgh
{

// While one of these lives, `stream` holds the second stream: everything enqueued goes there, and reductions use the
// communicator's second channel (lgh_comm.hip reads on_stream2).  Put back on every way out.
struct Stream2Scope
{
   lgh_ctx *c;
   explicit Stream2Scope(lgh_ctx *c_) : c(c_) { flip(1); }
   ~Stream2Scope() { flip(0); }
   Stream2Scope(const Stream2Scope &) = delete;
   Stream2Scope &operator=(const Stream2Scope &) = delete;

private:
   void flip(const int on)
   {
      std::swap(c->stream, c->stream2);
      c->on_stream2 = on;
   }
};

static int energy_rhs(lgh_ctx *c, const double *v_h1, double *e_rhs)
{
   RoctxRange range("SolveEnergy-ForcePA"); // laghos_solver.cpp:472-475
   if (c->erhs_q && c->fused_ftv_valid)
   {
      int *flag = c->dev_flags + (c->on_stream2 ? 2 : 0);
      LGH_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int), c->stream));
      hipLaunchKernelGGL(vec_differs_k, dim3(grid_for((c->H1V + 1) / 2)), dim3(256), 0, c->stream, v_h1, c->v_snap, (long)c->H1V, flag);
      LGH_HIP_CHECK(hipGetLastError());
      if (c->stress_current)
      {
         const int rc = force_mult_t_L(c, c->stressJinvT, v_h1, e_rhs, flag); // (runs only for a different v)
         if (rc) { return rc; }
         hipLaunchKernelGGL(copy_unless_k, dim3(ceil_div(c->L2V, 256)), dim3(256), 0, c->stream, e_rhs, c->erhs_q, (long)c->L2V, flag);
      }
      else
      {
         // the stress was kept in registers: a velocity other than the state's cannot be served - the right-hand side
         // becomes NaN on the device (nothing downstream can look right) and the next lgh_get_dt_est reports it
         hipLaunchKernelGGL(erhs_take_or_poison_k, dim3(ceil_div(c->L2V, 256)), dim3(256), 0, c->stream, e_rhs, c->erhs_q, (long)c->L2V, flag, c->dev_flags + 4);
      }
      LGH_HIP_CHECK(hipGetLastError());
      return LGH_OK;
   }
   return lgh_force_mult_transpose(c, v_h1, e_rhs);
}
// e_rhs = F^T v (+ e_source); the force region of the timers closes behind F^T v, as the reference's stopwatch does
static int energy_rhs_with_source(lgh_ctx *c, const double *v_h1, double *e_rhs, const double *e_source)
{
   timer_start(c);
   int rc = energy_rhs(c, v_h1, e_rhs); // :473
   timer_stop(c, 2);
   if (rc == LGH_OK && e_source) { rc = vec_axpby(c, e_rhs, 1.0, e_rhs, 1.0, e_source, c->L2V); } // :477
   return rc;
}
// :486 - a solve that took no iteration (a right-hand side of zero) counts as one
static void count_l2(lgh_ctx *c, const int it, int *l2_iters)
{
   const int counted = (it == 0) ? 1 : it;
   c->timers.c[1] += counted;
   if (l2_iters) { *l2_iters += counted; }
}

// The second stream, for the energy solve beside the velocity solve - at the LOWEST priority the device offers (round 6): the
// velocity solve is the longer of the two at every order up to Q4Q3 and its kernels fill the device; the energy solve's small
// kernels then take what is left instead of an equal share of the dispatch slots: 8.81 -> 8.75 ms per step at C2 on one box,
// 8.85 -> 8.78 on another; config 5, where the energy CG is the longer one, does not lose (372 -> 367 ms), the highest priority
// gains nothing anywhere (profiles/r6_stream_priority.txt).
static int create_stream2(lgh_ctx *c)
{
   int least = 0, greatest = 0;
   if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest)
   {
      LGH_HIP_CHECK(hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, least));
   }
   else { LGH_HIP_CHECK(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking)); }
   LGH_HIP_CHECK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
   LGH_HIP_CHECK(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
   return LGH_OK;
}

// ---- which way lgh_solve_energy_begin takes
// SolveEnergy does not depend on SolveVelocity's result (it takes v from S), so LagrangianHydroOperator::Mult may run the
// two concurrently.  That needs a quiet context: region timers and kernel sampling have sequential semantics, as in the
// reference, and a velocity solve by the scalar CG would share its scratch with the energy solve.  LGH_OVERLAP=0 switches
// it off.
static bool energy_quiet(const lgh_ctx *c)
{
   return c->sw.overlap && !c->timers.enabled && !(c->ktime && c->ktime->which >= 0) && vcg_available(c);
}
// the energy solve's reductions have a channel of their own on the second stream (one RCCL communicator must not be driven
// from two streams: lgh_comm_init creates a second one for this)
static bool energy_second_channel_free(const lgh_ctx *c)
{
   return c->multi == 0 || comm_second_channel(c);
}
// Several ranks without a second channel (the default over real RCCL): the energy CG can run in LOCKSTEP with the velocity
// CG on the one stream and communicator - its two dot products per iteration ride on exchanges the velocity iteration makes
// anyway.  (l2_lockstep_possible may look at the mass data on its first call, a kernel and a host look: asked last.)
static bool energy_lockstep_capable(lgh_ctx *c)
{
   return c->multi != 0 && !comm_second_channel(c) && l2_lockstep_possible(c) && vcg_lockstep_ready(c);
}
static EnergySolve::Mode energy_mode(lgh_ctx *c)
{
   if (c->dim == 1) { return EnergySolve::Deferred; } // (no overlap in 1D: _end runs the zone-local solve, after the velocity solve as in the reference)
   if (!energy_quiet(c)) { return EnergySolve::Deferred; }
   if (energy_second_channel_free(c)) { return EnergySolve::Overlapped; }
   return (c->sw.energy_lockstep && energy_lockstep_capable(c)) ? EnergySolve::Lockstep : EnergySolve::Deferred; // (LGH_ENERGY_LOCKSTEP=0: after the velocity solve)
}

// the overlapped solve's host looks and, if it has not converged, its further iterations; the join event behind them
static int energy_overlapped_finish(lgh_ctx *c, int *it)
{
   Stream2Scope on2(c);
   const int rc = cg_l2_end(c, it);
   if (rc) { return rc; }
   LGH_HIP_CHECK(hipEventRecord(c->ev_join, c->stream));
   return LGH_OK;
}
int energy_overlap_poll(lgh_ctx *c)
{
   EnergySolve &e = c->energy;
   if (e.mode != EnergySolve::Overlapped || e.polled) { return LGH_OK; }
   int it = 0;
   const int rc = energy_overlapped_finish(c, &it);
   if (rc) { return rc; }
   e.polled = true;
   e.iters = it;
   return LGH_OK;
}

} // namespace lgh

using namespace lgh;

extern "C"
{

// SolveEnergy, PA branch (laghos_solver.cpp:442-490)
int lgh_solve_energy(lgh_ctx *c, const double *S, const double *v_h1, double *dS_dt, double *e_rhs,
                     const double *e_source, double rel_tol, int max_iter, int *l2_iters)
{
   LGH_CHECK_ARG(c && S && v_h1 && dS_dt && e_rhs);
   (void)S;
   double *de = dS_dt + 2 * (size_t)c->H1V;
   if (c->dim == 1) // the FA branch: zone-local solves with the factors of Me(z), no CG (laghos_solver.cpp:491-516)
   {
      const int rc1 = stress_on_hand(c, "lgh_solve_energy");
      if (rc1) { return rc1; }
      return solve_energy_1d(c, v_h1, de, e_rhs, e_source, l2_iters);
   }
   int rc = energy_rhs_with_source(c, v_h1, e_rhs, e_source);
   if (rc) { return rc; }
   int it = 0;
   RoctxRange range("SolveEnergy-CGEMass"); // laghos_solver.cpp:480-483
   timer_start(c);
   rc = cg_solve(c, LGH_SPACE_L2, e_rhs, de, rel_tol, max_iter, &it, true); // :481
   timer_stop(c, 1);
   if (rc) { return rc; }
   count_l2(c, it, l2_iters);
   return LGH_OK;
}

// _begin / _end around lgh_solve_velocity.  Overlapped: _begin enqueues F^T v and the first chunk of the L2 CG on the second
// stream behind a fork event; the velocity solve completes it from inside (energy_overlap_poll) or _end does; _end joins.
// Lockstep: right-hand side and initial residual in _begin, the iterations inside lgh_solve_velocity, what is left of them
// in _end.  Deferred: the sequential lgh_solve_energy inside _end.
int lgh_solve_energy_begin(lgh_ctx *c, const double *S, const double *v_h1, double *dS_dt, double *e_rhs,
                           const double *e_source, double rel_tol, int max_iter)
{
   LGH_CHECK_ARG(c && S && v_h1 && dS_dt && e_rhs);
   EnergySolve &e = c->energy;
   e = EnergySolve{};
   e.args = {S, v_h1, dS_dt, e_rhs, e_source, rel_tol, max_iter};
   double *de = dS_dt + 2 * (size_t)c->H1V;
   const EnergySolve::Mode mode = energy_mode(c);
   if (mode == EnergySolve::Lockstep)
   {
      int rc = energy_rhs_with_source(c, v_h1, e_rhs, e_source);
      if (rc == LGH_OK) { rc = cg_l2_begin_lockstep(c, e_rhs, de, rel_tol, max_iter); }
      if (rc) { return rc; }
   }
   if (mode == EnergySolve::Overlapped)
   {
      if (!c->stream2)
      {
         const int rc2 = create_stream2(c);
         if (rc2) { return rc2; }
      }
      LGH_HIP_CHECK(hipEventRecord(c->ev_fork, c->stream));
      LGH_HIP_CHECK(hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
      Stream2Scope on2(c); // everything below is enqueued on the second stream
      int rc = energy_rhs_with_source(c, v_h1, e_rhs, e_source);
      if (rc == LGH_OK)
      {
         RoctxRange range("SolveEnergy-CGEMass"); // laghos_solver.cpp:480-483 (first chunk, second stream)
         rc = cg_l2_begin(c, e_rhs, de, rel_tol, max_iter); // :481
      }
      if (rc) { return rc; }
   }
   e.mode = mode;
   return LGH_OK;
}
int lgh_energy_lockstep_stats(lgh_ctx *c, long out[4])
{
   LGH_CHECK_ARG(c && out);
   out[0] = c->ls_stats[0]; out[1] = c->ls_stats[1]; out[2] = c->ls_stats[2];
   out[3] = (vcg_available(c) && energy_lockstep_capable(c)) ? 1 : 0; // (what the mode decision asks, without the switches and timers)
   return LGH_OK;
}
int lgh_solve_energy_end(lgh_ctx *c, int *l2_iters)
{
   LGH_CHECK_ARG(c && c->energy.mode != EnergySolve::Idle);
   const EnergySolve e = c->energy;
   c->energy = EnergySolve{};
   int it = 0;
   switch (e.mode)
   {
      case EnergySolve::Deferred:
         return lgh_solve_energy(c, e.args.S, e.args.v, e.args.dS, e.args.e_rhs, e.args.src, e.args.tol, e.args.maxit, l2_iters);
      case EnergySolve::Lockstep:
      {
         // whatever the velocity solve did not interleave (a solve that needs more iterations than last time, or than the
         // velocity solve took) runs now, reducing its scalars itself; then the look
         const int rc = cg_l2_end_lockstep(c, &it);
         if (rc) { return rc; }
         break;
      }
      case EnergySolve::Overlapped:
         if (e.polled) { it = e.iters; } // completed from inside the velocity solve (energy_overlap_poll): only the join is left
         else
         {
            const int rc = energy_overlapped_finish(c, &it);
            if (rc) { return rc; }
         }
         LGH_HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
         break;
      case EnergySolve::Idle: break; // (refused above)
   }
   count_l2(c, it, l2_iters);
   return LGH_OK;
}

} // extern "C"
