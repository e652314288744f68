// lgh_vcg.hip — the three velocity-component mass solves of SolveVelocity run in
// lockstep on the device: the node kernels, the mode decision, the argument block and vcg_solve.
// (K1: lgh_vcg_k1.hip, lgh_vcg_slab.hip; tables: lgh_vcg_tables.hip; test hooks: lgh_vcg_hooks.hip; shared: lgh_vcg.hpp)
//
// Reference: /root/reference/laghos_solver.cpp:363-398 calls CG_VMass.Mult once
// per velocity component, each a Jacobi-PCG on the same scalar H1 mass operator
// with its own right-hand side and essential-dof list.  Here the dim independent
// CGSolver::Mult recurrences advance together: every component keeps
// its own alpha, beta, residual norms, convergence flag and iteration count, and
// performs exactly the operations of its stand-alone solve in the same order —
// only the kernels are shared.
//
// Why (MI355X): the quadrature data D = w detJ0 rho0 is 63 % of the bytes of a mass
// apply and the element->node maps are another 10 %; applying the operator to the
// three directions in one pass reads them once instead of three times, halves the
// launches, and amortises the grid reduction (one ticket, three sums).
#include "lgh_vcg.hpp"

namespace lgh
{
typedef unsigned v4u_ __attribute__((ext_vector_type(4)));

// base pointer + 32-bit byte offset: one SGPR pair and one VGPR per address
__device__ __forceinline__ double vcg_ld(const double *base, const unsigned off) { return *(const double *)((const char *)base + off); }
__device__ __forceinline__ double *vcg_ptr(double *base, const unsigned off) { return (double *)((char *)base + off); }

// a.reset: the first kernel of a solve does what vcg_set_tol_k did in a launch of its own in front of it (round 6: one
// kernel boundary and a serial one-thread loop over ~400 words less per solve).  Workgroup 0 clears the exact accumulators
// and the set counters (nobody touches them before K1 of the first iteration); the thread that writes the scalars of the
// solve resets them first.
__device__ __forceinline__ void vcg_reset_accumulators(const VcgArgs &a)
{
   if (!a.reset || blockIdx.x != 0) { return; }
   if (a.limbs) { for (int i = threadIdx.x; i < 2 * kLimbWords + 8 * 16; i += blockDim.x) { a.limbs[i] = 0; } }
   if (a.rzl) { for (int i = threadIdx.x; i < 3 * kLimbWords; i += blockDim.x) { a.rzl[i] = 0; } }
}
__device__ __forceinline__ void vcg_reset_scalars(const VcgArgs &a, VcgScalars *s)
{
   if (!a.reset) { return; }
   s->rel_tol2 = a.reset_tol2;
   s->all_done = 0;
   s->first = 1;
   for (int c = 0; c < kVC; c++) { s->done[c] = 0; s->iters[c] = 0; s->nupd[c] = 0; s->alpha_last[c] = 0.0; s->alpha_hist[0][c] = s->alpha_hist[1][c] = 0.0; s->rzh[0][c] = s->rzh[1][c] = 0.0; }
}

// ---- init: r = b (x = 0), z = r/diag, nom_c = (z_c, r_c)
__global__ void __launch_bounds__(256)
vcg_init_k(const VcgArgs a)
{
   vcg_reset_accumulators(a);
   __shared__ double red[48];
   const int n = xcd_swizzle(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x; // as K2 and vcg_init_force_k
   double part[kVC] = {0.0, 0.0, 0.0};
   if (n < a.N)
   {
      const double di = a.dinv[n];
      const double ow = a.owner ? a.owner[n] : 1.0;
#pragma unroll
      for (int c = 0; c < kVC; c++)
      {
         const size_t i = (size_t)c * a.N + n;
         const double rv = a.b[(size_t)c * a.N + (a.ncaller ? a.ncaller[n] : n)]; // (b is the caller's vector)
         a.r[i] = rv;
         part[c] = ow * __dmul_rn(rv, di) * rv; // z = r/diag is recomputed where it is used
      }
   }
   double bp[kVC], total[kVC];
   block_sum3(part[0], part[1], part[2], red, bp);
   if (grid_sum3_last_block(bp, a.partials, a.stride, a.ticket, red, total))
   {
      if (threadIdx.x == 0)
      {
         VcgScalars *s = a.s;
         int all = 1;
         vcg_reset_scalars(a, s);
         for (int c = 0; c < kVC; c++)
         {
            s->rz[c] = s->rz_prev[c] = total[c];
            s->iters[c] = 0;
            if (!a.multi)
            {
               s->r0[c] = fmax(total[c] * s->rel_tol2, 0.0);
               s->done[c] = (total[c] < 0.0 || total[c] <= s->r0[c]) ? 1 : 0;
               all = all && s->done[c];
            }
         }
         s->first = 1;
         if (!a.multi) { s->all_done = all; }
      }
   }
}
// ---- init fused with the tail of ForcePA->Mult(one) (SolveVelocity, laghos_solver.cpp:354-384):
// b = -(H1R^T Y_E) with the essential rows of every component zeroed, x = 0, r = b, nom.  FE is
// the force E-vector in the reference layout (D1D^3, dim, NE) (laghos_assembly.cpp:312); the sum
// runs in the order of h1_transpose_gather_k, so b has the bits of the separate
// gather / negate / EliminateRHS kernels it replaces (four passes over the vectors less).
// ellc: the transpose of the restriction for the FORCE E-vector (slot j of node n at j * N + n), which is in the caller's zone
// order whatever order the solve's own E-vector has
template <int DEG>
__global__ void __launch_bounds__(256)
vcg_init_force_k(const VcgArgs a, const double *__restrict__ FE, const int ND, double *__restrict__ bout, const int *__restrict__ ellc, const int degc)
{
   vcg_reset_accumulators(a);
   __shared__ double red[48];
   const int n = xcd_swizzle(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x; // node ranges of vcg_init_k: same partial sums
   double part[kVC] = {0.0, 0.0, 0.0};
   if (n < a.N)
   {
      long pos[DEG];
#pragma unroll
      for (int j = 0; j < DEG; j++)
      {
         const int p = (j < degc) ? ellc[(size_t)j * a.N + n] : -1; // e*ND + d
         const int e = p / ND;
         pos[j] = (p >= 0) ? (long)kVC * ND * e + (p - e * ND) : -1;
      }
      const double di = a.dinv[n];
#pragma unroll
      for (int c = 0; c < kVC; c++)
      {
         double s = 0.0;
#pragma unroll
         for (int j = 0; j < DEG; j++) { if (pos[j] >= 0) { s += FE[pos[j] + (long)ND * c]; } }
         double bv = -s;
         if (a.ess[c] && a.ess[c][n]) { bv = 0.0; }
         const size_t i = (size_t)c * a.N + n;
         bout[(size_t)c * a.N + (a.ncaller ? a.ncaller[n] : n)] = bv; // (the caller's vector)
         a.r[i] = bv;
         a.x[i] = 0.0;
         part[c] = __dmul_rn(bv, di) * bv;
      }
   }
   double bp[kVC], total[kVC];
   block_sum3(part[0], part[1], part[2], red, bp);
   if (grid_sum3_last_block(bp, a.partials, a.stride, a.ticket, red, total))
   {
      if (threadIdx.x == 0)
      {
         VcgScalars *s = a.s;
         int all = 1;
         vcg_reset_scalars(a, s);
         for (int c = 0; c < kVC; c++)
         {
            s->rz[c] = s->rz_prev[c] = total[c];
            s->iters[c] = 0;
            s->r0[c] = fmax(total[c] * s->rel_tol2, 0.0);
            s->done[c] = (total[c] < 0.0 || total[c] <= s->r0[c]) ? 1 : 0;
            all = all && s->done[c];
         }
         s->first = 1;
         s->all_done = all;
      }
   }
}
// The same kernel over a table of byte offsets into the force E-vector ([e][c][d]; absent contributions point at
// a zero element behind it - element NE, all components): no index arithmetic, no predicates, and slots no node of the wavefront uses are not
// fetched (as in vcg_update_p_k).  Same node -> workgroup map and summation orders as above: the same bits.
__global__ void __launch_bounds__(256)
vcg_init_force_z_k(const VcgArgs a, const double *__restrict__ FE, const unsigned compb_fe, const unsigned *__restrict__ ellf,
                   double *__restrict__ bout)
{
   vcg_reset_accumulators(a);
   __shared__ double red[48];
   const int n = xcd_swizzle(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
   const bool ok = n < a.N;
   const unsigned nn = (unsigned)(ok ? n : a.N - 1);
   const unsigned rowb = 4u * (unsigned)a.N;
   unsigned ix[8];
#pragma unroll
   for (int j = 0; j < 8; j++) { ix[j] = *(const unsigned *)((const char *)ellf + (4u * nn + (unsigned)j * rowb)); }
   const double di = vcg_ld(a.dinv, 8u * nn);
   const unsigned es = a.essbits[nn];
   const unsigned zoff = 8u * (unsigned)kVC * (unsigned)(a.ye_stride - kYePad); // = 8 * kVC * ND * NE
   double fe[kVC][8];
#pragma unroll
   for (int j = 0; j < 8; j++)
   {
      if (j == 0 || __any(ix[j] != zoff))
      {
#pragma unroll
         for (int c = 0; c < kVC; c++) { fe[c][j] = vcg_ld(FE, ix[j] + (unsigned)c * compb_fe); }
      }
      else
      {
#pragma unroll
         for (int c = 0; c < kVC; c++) { fe[c][j] = 0.0; }
      }
   }
   double part[kVC];
#pragma unroll
   for (int c = 0; c < kVC; c++)
   {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < 8; j++) { s += fe[c][j]; }
      double bv = -s;
      if ((es >> c) & 1u) { bv = 0.0; }
      part[c] = ok ? __dmul_rn(bv, di) * bv : 0.0;
      if (ok)
      {
         const size_t i = (size_t)c * a.N + n;
         bout[(size_t)c * a.N + (a.ncaller ? a.ncaller[n] : n)] = bv; // (the caller's vector)
         a.r[i] = bv;
         a.x[i] = 0.0;
      }
   }
   double bp[kVC], total[kVC];
   block_sum3(part[0], part[1], part[2], red, bp);
   if (grid_sum3_last_block(bp, a.partials, a.stride, a.ticket, red, total))
   {
      if (threadIdx.x == 0)
      {
         VcgScalars *s = a.s;
         int all = 1;
         vcg_reset_scalars(a, s);
         for (int c = 0; c < kVC; c++)
         {
            s->rz[c] = s->rz_prev[c] = total[c];
            s->iters[c] = 0;
            s->r0[c] = fmax(total[c] * s->rel_tol2, 0.0);
            s->done[c] = (total[c] < 0.0 || total[c] <= s->r0[c]) ? 1 : 0;
            all = all && s->done[c];
         }
         s->first = 1;
         s->all_done = all;
      }
   }
}
__global__ void vcg_init_finish_k(VcgScalars *s)
{
   int all = 1;
   for (int c = 0; c < kVC; c++)
   {
      s->rz_prev[c] = s->rz[c];
      s->r0[c] = fmax(s->rz[c] * s->rel_tol2, 0.0);
      s->done[c] = (s->rz[c] < 0.0 || s->rz[c] <= s->r0[c]) ? 1 : 0;
      all = all && s->done[c];
   }
   s->all_done = all;
}
__global__ void vcg_set_tol_k(VcgScalars *s, double rel_tol2, long long *limbs, long long *rzl)
{
   if (limbs) { for (int i = 0; i < 2 * kLimbWords + 8 * 16; i++) { limbs[i] = 0; } } // accumulators and the set counters behind them
   if (rzl) { for (int i = 0; i < 3 * kLimbWords; i++) { rzl[i] = 0; } }
   s->rel_tol2 = rel_tol2;
   s->all_done = 0;
   s->first = 1;
   for (int c = 0; c < kVC; c++) { s->done[c] = 0; s->iters[c] = 0; s->nupd[c] = 0; s->alpha_last[c] = 0.0; s->alpha_hist[0][c] = s->alpha_hist[1][c] = 0.0; s->rzh[0][c] = s->rzh[1][c] = 0.0; }
}
// Several ranks: the host enqueues the iteration count of the previous solve without looking at the flags,
// so a few launches may follow convergence.  Their kernels return at once, but the exchanges between them
// still run and would re-sum the (already global) den / rz of a finished component once per surplus
// iteration - growing by the number of ranks each time, to inf after a long solve.  Whoever marks a
// component done (vcg_pending_update / vcg_pending_den inside the kernels, this kernel before the host
// looks) therefore zeroes its scalars: sums of zeros stay zero.  den[c] and rz[c] are undefined (0) once
// done[c] is set; nothing reads them after that.
__global__ void vcg_update_finish_k(VcgScalars *s, int iter, VcgScalars *host_out, unsigned long long *host_token, const unsigned long long token)
{
   int all = 1;
   for (int c = 0; c < kVC; c++)
   {
      if (!s->done[c])
      {
         s->iters[c] = iter;
         if (s->rz[c] < 0.0 || s->rz[c] <= s->r0[c]) { s->done[c] = 1; }
      }
      if (s->done[c]) { s->rz[c] = 0.0; s->den[c] = 0.0; }
      all = all && s->done[c];
   }
   s->all_done = all;
   if (host_out) // (the host looks next: straight into its pinned memory, the token last)
   {
      *host_out = *s;
      __threadfence_system();
      __hip_atomic_store(host_token, token, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
   }
}

// rz_limbs mode: the outcome of the last enqueued iteration `last`, committed for the host (what workgroup 0 of
// K1(last + 1) would write); host_out: pinned host memory the host reads after its stream synchronisation (nullptr: test hook)
__global__ void vcg_rz_finish_k(VcgScalars *s, const long long *rzl, const int last, const long long *peers, const int n_peers, VcgScalars *host_out,
                                unsigned long long *host_token, const unsigned long long token)
{
   // several ranks: own words + the peers' (exchange_words) = the sum over the ranks; folded into a scratch set - the
   // flag word rides along (any rank's overflow turns the sum into NaN on every rank)
   long long set[kLimbWords]; // (a copy: K1(last + 1), if the host enqueues it after its look, folds own + peers itself)
   for (int i = 0; i <= kLimbShards * kVC * kLimbs; i++)
   {
      long long w = rzl[(last % 3) * kLimbWords + i];
      for (int p = 0; p < n_peers; p++) { w += peers[p * kLimbWords + i]; }
      set[i] = w;
   }
   double cur[kVC];
   bool dn[kVC];
   for (int k = 0; k < kVC; k++)
   {
      const double before = (last > 1) ? s->rzh[(last - 1) & 1][k] : s->rz[k];
      cur[k] = exact_fold(set, k, exact_scale(before));
      dn[k] = s->done[k] != 0 || vcg_rz_converged(last + 1, cur[k], s->r0[k]);
   }
   vcg_rz_commit(s, last + 1, cur, dn);
   if (host_out)
   {
      *host_out = *s;
      __threadfence_system();
      __hip_atomic_store(host_token, token, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
   }
}

// ---- K2: per node and component: A d = sum of element contributions, ess rows,
// d = r/diag + beta d, x += alpha d, r -= alpha A d, (r, r/diag).  The preconditioned
// residual z = r/diag is never stored: K1 and K2 recompute it from r (one rounded
// multiply, so both see the same value), which saves a vector read and a write.
template <bool FUSED_GATHER, int DEG>
__global__ void __launch_bounds__(256)
vcg_update_k(const VcgArgs a)
{
   __shared__ double red[48];
   if (a.s->all_done) { return; }
   const bool it1 = (a.iter == 1);
   const int n = xcd_swizzle(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
   const bool ok = n < a.N;
   const int nn = ok ? n : a.N - 1;
   double part[kVC] = {0.0, 0.0, 0.0};
   int pidx[DEG > 0 ? DEG : 1];
   if (FUSED_GATHER)
   {
#pragma unroll
      for (int j = 0; j < DEG; j++) { pidx[j] = (j < a.deg) ? a.ell[(size_t)j * a.N + nn] : -1; }
   }
   const double di = a.dinv[nn];
   const double ow = a.owner ? a.owner[nn] : 1.0;
   const bool shared = FUSED_GATHER && a.hmask && a.hmask[nn];
#pragma unroll 1
   for (int c = 0; c < kVC; c++)
   {
      if (a.s->done[c]) { continue; } // uniform
      if (a.multi && vcg_pending_den(a.s, c, blockIdx.x == 0 && threadIdx.x == 0)) { continue; }
      const double alpha = a.s->rz[c] / a.s->den[c];
      const double beta = it1 ? 0.0 : a.s->rz[c] / a.s->rz_prev[c];
      const size_t i = (size_t)c * a.N + nn;
      double zv;
      if (FUSED_GATHER)
      {
         if (shared) { zv = a.yL[i]; } // summed over the ranks by halo_sum
         else
         {
            const double *yc = a.YE + (size_t)c * a.ye_stride;
            zv = 0.0;
#pragma unroll
            for (int j = 0; j < DEG; j++) { if (pidx[j] >= 0) { zv += yc[pidx[j]]; } }
         }
      }
      else { zv = a.yL[i]; }
      if (a.ess[c] && a.ess[c][nn]) { zv = 0.0; }
      const double ro = a.r[i];
      double dv = __dmul_rn(ro, di); // z of the previous iterate, not stored
      if (!it1) { dv = fma(beta, a.d[i], dv); }
      const double xv = a.x[i] + alpha * dv;
      const double rv = ro - alpha * zv;
      const double pz = __dmul_rn(rv, di);
      if (ok)
      {
         a.d[i] = dv;
         a.x[i] = xv;
         a.r[i] = rv;
         part[c] = ow * rv * pz;
      }
   }
   double bp[kVC], total[kVC];
   block_sum3(part[0], part[1], part[2], red, bp);
   if (grid_sum3_last_block(bp, a.partials, a.stride, a.ticket, red, total))
   {
      if (threadIdx.x == 0)
      {
         VcgScalars *s = a.s;
         int all = 1;
         for (int c = 0; c < kVC; c++)
         {
            if (!s->done[c] && !(a.multi && s->den[c] == 0.0)) // (several ranks: breakdown found by this launch)
            {
               s->rz_prev[c] = s->rz[c];
               s->rz[c] = total[c]; // betanom
               if (!a.multi)
               {
                  s->iters[c] = a.iter;
                  if (total[c] < 0.0 || total[c] <= s->r0[c]) { s->done[c] = 1; }
               }
            }
            all = all && s->done[c];
         }
         if (!a.multi) { s->all_done = all; }
      }
   }
}

// ---- K2, bounded-grid form (one rank) ---------------------------------------------------------------
// The same node update as vcg_update_k, organised the way the node phase of the persistent kernel
// (round 2's persistent-solve experiment, profiles/r2_pcg_trace_*.txt) turned out to run fastest - its measurements carry over to a kernel of its own:
//  * four workgroups of 512 threads per CU (more on large meshes: ranges of at most ~1000 nodes), each with a contiguous node range of equal COST (a node costs a
//    fixed part plus a part per element contribution; with equal counts the ranges that cover
//    element-boundary planes take 40 % longer), all ~35 loads of a node issued before the first use,
//    straight-line code.  One node per thread and pass (106 VGPRs, two workgroups resident per CU) - two
//    (182 VGPRs, one resident; what the persistent kernel's node phase used) lost, 55.4 against 49.7 us
//    at C2 (LGH_K2_GRID=<workgroups per CU> for A/B);
//  * the ELL row holds byte offsets and absent contributions point at a zero slot behind the Y_E plane: no
//    predicated loads, addresses are one SGPR base + a 32-bit VGPR offset;
//  * x is only needed at the end of the solve: it is updated every second iteration with both terms,
//      x = (x + alpha_{it-1} d_{it-1}) + alpha_it d_it     (the roundings of two single updates),
//    and vcg_xfix_k adds the pending term of a component that stopped after an odd number of updates -
//    22 MB less traffic per iteration on average at C2;
//  * 1024 workgroup partials instead of 3566 for the ticketed reduction;
//  * write-through and non-temporal stores of d, r, x were tried (no gain) and are gone.

// MINW (round 5): wavefronts per SIMD the register allocation admits (the second argument of HIP's __launch_bounds__):
// 4 = the budget of rounds 2-4 (up to 128 VGPRs: two workgroups of eight wavefronts per CU), 6 = at most 80 (three).  The kernel is a chain of dependent memory round trips per pass
// (table -> element contributions -> stores), and what hides them is the number of wavefronts a CU holds; the second
// table (slots 4..7) is summed in a branch of its own so that its 24 registers exist only there.
template <bool XU, int MINW>
__global__ void __launch_bounds__(512, MINW)
vcg_update_p_k(const VcgArgs a)
{
   constexpr int NT = 512;
   __shared__ double red[48];
   if (a.s->all_done)
   {
      // (several ranks, pack_rz: the exchange that follows must not carry the sums of an earlier iteration)
      if (a.pack_rz && blockIdx.x == 0 && threadIdx.x < a.hp.n_nbr * kVC) { a.hp.sbuf[(size_t)a.hp.base[threadIdx.x / kVC] + threadIdx.x % kVC] = 0.0; }
      return;
   }
   const int it = a.iter;
   const bool first = (it == 1);
   const int tid = threadIdx.x;
   const int w = xcd_swizzle(blockIdx.x, gridDim.x);
   const int n0 = a.nstart[w], n1 = a.nstart[w + 1];
   bool todo[kVC];
   double alpha[kVC], alpha_prev[kVC], beta[kVC], den[kVC];
   // rz_limbs mode (lgh_vcg.hpp): (r, z) of the last two iterations as workgroup 0 of K1 left them
   double rzc[kVC], rzp[kVC];
   int rzE[kVC] = {0, 0, 0};
#pragma unroll
   for (int k = 0; k < kVC; k++)
   {
      rzc[k] = (a.rzl && it > 1) ? a.s->rzh[(it - 1) & 1][k] : a.s->rz[k];
      rzp[k] = a.rzl ? a.s->rzh[it & 1][k] : a.s->rz_prev[k]; // (only looked at from the second iteration on)
      rzE[k] = exact_scale(rzc[k]);
   }
#pragma unroll
   for (int k = 0; k < kVC; k++) { den[k] = (a.den_limbs == 1) ? exact_den(a.limbs + (it & 1) * kLimbWords, k, rzc[k]) : a.s->den[k]; }
   if (a.den_limbs == 1 && blockIdx.x == 0 && tid < kLimbWords) { a.limbs[((it + 1) & 1) * kLimbWords + tid] = 0; } // the set of the next K1
#pragma unroll
   for (int k = 0; k < kVC; k++)
   {
      todo[k] = a.s->done[k] == 0;
      if (a.den_limbs == 1 && den[k] == 0.0) { todo[k] = false; } // breakdown, as upstream (marked below)
      // (several ranks: breakdown is looked at here, after the sum of (d, A d) over the ranks - vcg_pending_den)
      if (a.multi && todo[k] && vcg_pending_den(a.s, k, blockIdx.x == 0 && tid == 0)) { todo[k] = false; }
      alpha[k] = todo[k] ? rzc[k] / den[k] : 0.0;
      alpha_prev[k] = todo[k] ? (a.rzl ? a.s->alpha_hist[(it - 1) & 1][k] : a.s->alpha_last[k]) : 0.0;
      beta[k] = (first || !todo[k]) ? 0.0 : rzc[k] / rzp[k];
   }
   if (a.rzl && !(todo[0] || todo[1] || todo[2]))
   {
      // nothing iterates any more (launches enqueued past convergence): only the bookkeeping of a breakdown is left
      if (blockIdx.x == 0 && tid == 0)
      {
         for (int k = 0; k < kVC; k++) { if (!a.s->done[k] && den[k] == 0.0) { a.s->done[k] = 1; } }
      }
      return;
   }
   const bool xload = XU && it > 2;
   const unsigned compb = 8u * (unsigned)a.N;
   const unsigned zoff = 8u * (unsigned)(a.ye_stride - kYePad); // byte offset of the zero slot (make_ellz)
   const char *const ellhi = (const char *)a.ellz + (size_t)16 * (size_t)a.N; // slots 4..7
   double part[kVC] = {0.0, 0.0, 0.0};
   for (int base = n0; base < n1; base += NT)
   {
      const int n = base + tid;
      const bool ok = n < n1;
      const unsigned nn = (unsigned)(ok ? n : n0);
      // ELL rows as two tables of four offsets per node (16 bytes each): slots 0..3 with one load per node; slots 4..7 -
      // only a vertex node of the mesh has more than four contributions, with the merged E-vector of the slab K1 only
      // where a set boundary meets an element edge in y and z - are fetched when some node of the wavefront uses them
      // (rows hold their contributions first, so slot 3 tells): a ninth of the wavefronts, 16 of the table's 32 bytes per
      // node for the others
      unsigned ix[4];
      const v4u_ q0 = *(const v4u_ *)((const char *)a.ellz + 16u * nn);
      ix[0] = q0[0]; ix[1] = q0[1]; ix[2] = q0[2]; ix[3] = q0[3];
      const bool hi = !a.k2_skip || __any(q0[3] != zoff);
      double ro[kVC], dol[kVC], xo[kVC];
      const double di = vcg_ld(a.dinv, 8u * nn);
      const unsigned es = a.essbits[nn];
#pragma unroll
      for (int k = 0; k < kVC; k++)
      {
         const unsigned vb = 8u * nn + (unsigned)k * compb;
         ro[k] = vcg_ld(a.r, vb);
         dol[k] = vcg_ld(a.d, vb);
         xo[k] = 0.0;
         if (XU && MINW < 6) { xo[k] = vcg_ld(a.x, vb); }
      }
      // Slot j of the ELL rows is only fetched when some node of the wavefront has a j-th contribution (rows hold
      // their contributions first): a wave of consecutive nodes of a tensor-product mesh rarely needs all 8 (a
      // node needs 1, 2, 4 or 8), and the loads of absent slots - all lanes at the zero slot - still occupy the
      // address path.
      bool need[4];
      need[0] = true;
#pragma unroll
      for (int j = 1; j < 4; j++) { need[j] = !a.k2_skip || __any(ix[j] != zoff); }
      double zsum[kVC]; // ascending contribution order (absent slots add 0.0): the sum of vcg_update_k
      {
         double ye[kVC][4];
#pragma unroll
         for (int j = 0; j < 4; j++)
         {
            if (need[j])
            {
#pragma unroll
               for (int k = 0; k < kVC; k++) { ye[k][j] = vcg_ld(a.YE + (size_t)k * a.ye_stride, ix[j]); }
            }
            else
            {
#pragma unroll
               for (int k = 0; k < kVC; k++) { ye[k][j] = 0.0; }
            }
         }
#pragma unroll
         for (int k = 0; k < kVC; k++) { zsum[k] = ((0.0 + ye[k][0]) + ye[k][1]) + ye[k][2]; zsum[k] += ye[k][3]; }
      }
      if (XU && MINW >= 6 && xload)
      {
         // (six wavefronts per SIMD: x is asked for once the element contributions have been summed - its three registers
         //  per node would otherwise be live beside their 24, and the budget of 80 does not hold both; the other
         //  wavefronts of the SIMD cover the round trip)
#pragma unroll
         for (int k = 0; k < kVC; k++) { asm volatile("" : "+v"(zsum[k])); xo[k] = vcg_ld(a.x, 8u * nn + (unsigned)k * compb); }
      }
      if (hi)
      {
         // contributions 5..8 (a ninth of the wavefronts): second table, then the values, added behind the first four
         const v4u_ q1 = *(const v4u_ *)(ellhi + 16u * nn);
#pragma unroll
         for (int k = 0; k < kVC; k++)
         {
            const double *yc = a.YE + (size_t)k * a.ye_stride;
            const double y4 = vcg_ld(yc, q1[0]), y5 = vcg_ld(yc, q1[1]), y6 = vcg_ld(yc, q1[2]), y7 = vcg_ld(yc, q1[3]);
            zsum[k] = (((zsum[k] + y4) + y5) + y6) + y7;
         }
      }
      // several ranks: a node shared with another rank takes its A d from the L-vector the halo exchange has summed
      double ysh[kVC];
      const bool anysh = a.multi && __any((es >> 3) & 1u);
#pragma unroll
      for (int k = 0; k < kVC; k++) { ysh[k] = anysh ? vcg_ld(a.yL, 8u * nn + (unsigned)k * compb) : 0.0; }
      const double ow = ((es >> 4) & 1u) ? 0.0 : 1.0; // (1 on one rank)
#pragma unroll
      for (int k = 0; k < kVC; k++)
      {
         const unsigned vb = 8u * nn + (unsigned)k * compb;
         double zs = zsum[k];
         if (anysh && ((es >> 3) & 1u)) { zs = ysh[k]; }
         const double z_ = ((es >> k) & 1u) ? 0.0 : zs;
         const double zold = __dmul_rn(ro[k], di); // z of the previous iterate, not stored
         const double dnew = first ? zold : fma(beta[k], dol[k], zold);
         const double rnew = ro[k] - alpha[k] * z_;
         if (ok && todo[k])
         {
            *vcg_ptr(a.d, vb) = dnew;
            *vcg_ptr(a.r, vb) = rnew;
            if (XU)
            {
               const double x0 = xload ? xo[k] : 0.0;
               *vcg_ptr(a.x, vb) = fma(alpha[k], dnew, fma(alpha_prev[k], first ? 0.0 : dol[k], x0));
            }
            part[k] += (a.multi ? ow : 1.0) * rnew * __dmul_rn(rnew, di);
         }
      }
   }
   if (a.rzl)
   {
      // no last workgroup: the share of (r, z) of this workgroup into set it % 3 (exact limbs, fire-and-forget atomics);
      // the next kernels fold it.  Workgroup 0 leaves what K2 of the next iteration and the host read.
      // (the workgroup's share as ONE double per component - a fixed tree: wave sums, then the eight wavefronts in
      //  order - split into limbs by one thread per component: exactness is only needed ACROSS workgroups, whose
      //  atomics arrive in any order.  Round 4, first version: every thread split its own partial and the limbs went
      //  through twelve 64-bit wave sums - 0.5 us more per launch, profiles/r4_k2_tail.txt.)
      const int lane = tid & 63, wid = tid >> 6;
      const double w0 = wave_sum(part[0], lane, 64), w1 = wave_sum(part[1], lane, 64), w2 = wave_sum(part[2], lane, 64);
      if (lane == 0) { red[3 * wid + 0] = w0; red[3 * wid + 1] = w1; red[3 * wid + 2] = w2; }
      __syncthreads();
      long long *L = a.rzl + (it % 3) * kLimbWords;
      if (tid < kVC)
      {
         double t = 0.0;
#pragma unroll
         for (int w = 0; w < NT / 64; w++) { t += red[3 * w + tid]; }
         const bool live = (tid == 0) ? todo[0] : (tid == 1) ? todo[1] : todo[2];
         const int E = (tid == 0) ? rzE[0] : (tid == 1) ? rzE[1] : rzE[2];
         long long acc[kLimbs] = {0, 0, 0, 0};
         const bool bad = live && !exact_add(acc, t, E);
         if (live && !bad)
         {
#pragma unroll
            for (int j = 0; j < kLimbs; j++)
            {
               if (acc[j] != 0) { (void)__hip_atomic_fetch_add(&L[(blockIdx.x % kLimbShards) * (kVC * kLimbs) + kLimbs * tid + j], acc[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
            }
         }
         if (bad) { (void)__hip_atomic_fetch_or(&L[kLimbShards * kVC * kLimbs], 1LL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
      }
      if (blockIdx.x == 0 && tid == 0)
      {
         VcgScalars *s = a.s;
         s->first = 0;
         for (int k = 0; k < kVC; k++)
         {
            if (s->done[k]) { continue; }
            s->den[k] = den[k];
            if (den[k] == 0.0) { s->done[k] = 1; continue; } // breakdown, as upstream
            s->alpha_hist[it & 1][k] = alpha[k]; // (K2 of the next iteration: the deferred update of x)
            s->alpha_last[k] = alpha[k];         // (vcg_xfix_k after the solve)
            s->nupd[k] = it;
         }
      }
      return;
   }
   double bp[kVC], total[kVC];
   block_sum3(part[0], part[1], part[2], red, bp);
   if (grid_sum3_last_block(bp, a.partials, a.stride, a.ticket, red, total))
   {
      if (tid == 0)
      {
         VcgScalars *s = a.s;
         int all = 1;
         if (a.den_limbs == 1) { s->first = 0; }
         for (int k = 0; k < kVC; k++)
         {
            if (a.den_limbs == 1 && !s->done[k])
            {
               s->den[k] = den[k];
               if (den[k] == 0.0) { s->done[k] = 1; }
            }
            if (!s->done[k] && !(a.multi && s->den[k] == 0.0)) // (several ranks: breakdown found by this launch)
            {
               s->alpha_last[k] = s->rz[k] / den[k]; // the alpha this launch used
               s->nupd[k] = it;
               s->rz_prev[k] = s->rz[k];
               s->rz[k] = total[k]; // betanom: on several ranks the local part, summed and looked at by the next K1
               if (!a.multi)
               {
                  s->iters[k] = it;
                  if (total[k] < 0.0 || total[k] <= s->r0[k]) { s->done[k] = 1; }
               }
            }
            all = all && s->done[k];
         }
         if (!a.multi) { s->all_done = all; }
         if (a.pack_rz)
         {
            // the local (r, z) straight into the send buffer of the exchange that sums it over the ranks
            for (int k = 0; k < a.hp.n_nbr; k++)
            {
               for (int e = 0; e < kVC; e++) { a.hp.sbuf[(size_t)a.hp.base[k] + e] = s->rz[e]; }
            }
         }
      }
   }
}
// components whose last update of x is still pending (an odd number of updates)
__global__ void __launch_bounds__(256)
vcg_xfix_k(const VcgArgs a)
{
   const int n = blockIdx.x * blockDim.x + threadIdx.x;
   if (n >= a.N) { return; }
   for (int k = 0; k < kVC; k++)
   {
      if ((a.s->nupd[k] & 1) == 0) { continue; }
      const size_t i = (size_t)k * a.N + n;
      a.x[i] = fma(a.s->alpha_last[k], a.d[i], a.x[i]);
   }
}

// The solve ran in the library's own node numbering (a.ncaller): its solution goes to the caller's vector, with the pending
// update of vcg_xfix_k applied on the way (the same fma: the same bits as fix, then copy)
__global__ void __launch_bounds__(256)
vcg_xout_k(const VcgArgs a, double *__restrict__ X)
{
   const int n = blockIdx.x * blockDim.x + threadIdx.x;
   if (n >= a.N) { return; }
   const int nc = a.ncaller[n];
   for (int k = 0; k < kVC; k++)
   {
      const size_t i = (size_t)k * a.N + n;
      double xv = a.x[i];
      if (a.s->nupd[k] & 1) { xv = fma(a.s->alpha_last[k], a.d[i], xv); }
      X[(size_t)k * a.N + nc] = xv;
   }
}

// unfused E -> L sum of the kVC planes (multi-GPU path, unusual valence)
__global__ void __launch_bounds__(256)
vcg_gather_k(const VcgArgs a)
{
   const int n = blockIdx.x * blockDim.x + threadIdx.x;
   if (n >= a.N) { return; }
   for (int c = 0; c < kVC; c++)
   {
      if (a.s->done[c]) { continue; }
      const double *yc = a.YE + (size_t)c * a.ye_stride;
      double s = 0.0;
      for (int j = 0; j < a.deg; j++)
      {
         const int p = a.ell[(size_t)j * a.N + n];
         if (p >= 0) { s += yc[p]; }
      }
      a.yL[(size_t)c * a.N + n] = s;
   }
}

// Several ranks, slab-form K1 with exact accumulators (den_limbs == 2): the local part of (d, A d) has to exist as a
// double before the exchange that sums it over the ranks - one workgroup (of the kernel that runs between K1 and the
// exchange anyway) folds the set K1 added into and clears the other one for the next K1.  256 threads.
__device__ __forceinline__ void vcg_fold_den(const VcgArgs &a)
{
   const int tid = threadIdx.x, it = a.iter;
   // (the scale of the accumulators is that of (r, z) before this iteration: in rz_limbs mode K1 of this iteration left it in rzh)
   if (tid < kVC && !a.s->done[tid])
   {
      const double ref = (a.rzl && it > 1) ? a.s->rzh[(it - 1) & 1][tid] : a.s->rz[tid];
      __hip_atomic_store(&a.s->den[tid], exact_den(a.limbs + (it & 1) * kLimbWords, tid, ref), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
   }
   if (tid < kLimbWords) { a.limbs[((it + 1) & 1) * kLimbWords + tid] = 0; }
   if (tid == 0) { a.s->first = 0; }
}
__global__ void __launch_bounds__(256)
vcg_fold_den_k(const VcgArgs a) { vcg_fold_den(a); }

// E -> L sum at the listed (rank-shared) nodes only: what the halo exchange needs
// pack_halo: every sum also goes to its places in the send buffer (one per neighbour that shares the node: the CSR the
// combine kernel reads), and workgroup 0 puts the local (d, A d) behind every neighbour's block (nx_den) - the exchange
// then starts without the pack kernel (halo_sum(..., packed)).  Components that are done send zeros.
__global__ void __launch_bounds__(256)
vcg_gather_list_k(const VcgArgs a)
{
   if (blockIdx.x == 0 && (a.den_limbs == 2 || a.nx_den > 0))
   {
      if (a.den_limbs == 2) { vcg_fold_den(a); }
      __syncthreads(); // (den of this workgroup's own fold: visible to its other threads)
      const int t = threadIdx.x;
      if (t < a.hp.n_nbr * a.nx_den)
      {
         const int k = t / a.nx_den, e = t - k * a.nx_den;
         a.hp.sbuf[(size_t)a.hp.base[k] + (size_t)kVC * a.hp.ncnt[k] + e] = __hip_atomic_load(e < kVC ? &a.s->den[e] : &a.s->den_e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
   }
   const int u = blockIdx.x * blockDim.x + threadIdx.x;
   if (u >= a.n_shared) { return; }
   const int n = a.sh_node[u];
   for (int c = 0; c < kVC; c++)
   {
      const bool live = a.s->done[c] == 0;
      double s = 0.0;
      if (live)
      {
         const double *yc = a.YE + (size_t)c * a.ye_stride;
         for (int j = 0; j < a.deg; j++)
         {
            const int p = a.ell[(size_t)j * a.N + n];
            if (p >= 0) { s += yc[p]; }
         }
         a.yL[(size_t)c * a.N + n] = s;
      }
      if (a.pack_halo)
      {
         for (int k = a.hp.sh_off[u]; k < a.hp.sh_off[u + 1]; k++)
         {
            const int j = a.hp.sh_src[k];
            if (j >= 0) { a.hp.sbuf[(size_t)a.hp.pos[j] + (size_t)c * a.hp.cnt[j]] = s; }
         }
      }
   }
}

// ---- host side -----------------------------------------------------------------------
bool vcg_fused_init_ok(const lgh_ctx *c) { return c->sw.fused_init && vcg_available(c) && c->multi == 0 && c->t_deg <= 8; }
bool vcg_lockstep_ready(const lgh_ctx *c) { return c->vcg_aux && c->vcg_aux->ls_ready != 0; }

// ---- launchers of the node kernels the solve and the test hooks share
// one launch of K2 as the one-rank solve issues it in iteration `it`: the bounded-grid kernel, x updated every second iteration
void vcg_launch_k2p(lgh_ctx *c, const VcgPlan &plan, const VcgArgs &a, const int it)
{
   kt_begin(c, LGH_KERNEL_CG_UPDATE_H1);
   // the launch without x: at most 80 registers (six wavefronts per SIMD); the one that updates x would spill there and
   // keeps the budget of rounds 2-4 (profiles/r5_k2_occupancy_grid.txt)
   if (it & 1) { hipLaunchKernelGGL((vcg_update_p_k<false, 6>), dim3(plan.aux->grid2), dim3(512), 0, c->stream, a); }
   else { hipLaunchKernelGGL((vcg_update_p_k<true, 4>), dim3(plan.aux->grid2), dim3(512), 0, c->stream, a); }
   kt_end(c, LGH_KERNEL_CG_UPDATE_H1);
}
// the round-1 K2, one node per thread (LGH_K2P=0, unusual valence): gathering A d itself, or reading it from the L-vector
void vcg_launch_update(lgh_ctx *c, const VcgArgs &a, const bool fused_gather)
{
   const int nb = ceil_div(a.N, 256);
   if (fused_gather) { hipLaunchKernelGGL((vcg_update_k<true, 8>), dim3(nb), dim3(256), 0, c->stream, a); }
   else { hipLaunchKernelGGL((vcg_update_k<false, 0>), dim3(nb), dim3(256), 0, c->stream, a); }
}
void vcg_launch_fold_den(lgh_ctx *c, const VcgArgs &a) { hipLaunchKernelGGL(vcg_fold_den_k, dim3(1), dim3(256), 0, c->stream, a); }
void vcg_launch_rz_finish(lgh_ctx *c, const VcgArgs &a, const int last, VcgScalars *host_out, unsigned long long *host_token, const unsigned long long token)
{
   hipLaunchKernelGGL(vcg_rz_finish_k, dim3(1), dim3(1), 0, c->stream, a.s, a.rzl, last, a.rzl_peers, a.n_rz_peers, host_out, host_token, token);
}

// ---- vcg_prepare, step 1: the work buffers of the context
static int vcg_work_buffers(lgh_ctx *c)
{
   if (c->vcg_tickets) { return LGH_OK; } // (the last one built: a failure on the way leaves the rest to the next call)
   const size_t N = (size_t)c->N;
   LGH_PASS(c->vcg_s.alloc(1, true));
   LGH_PASS(c->vcg_vec.alloc(3 * kVC * N, true)); // r, d, yL (z = r/diag is never stored)
   // block partials of the largest reducing launch: K1 (<= NE batches), vcg_update_k (N/256 blocks), vcg_update_p_k (2 per CU)
   c->vcg_stride = (unsigned)(std::max<size_t>(std::max<size_t>((size_t)c->NE, (N + 255) / 256), 4096) + kShards);
   LGH_PASS(c->vcg_partials.alloc(2 * kVC * (size_t)c->vcg_stride, true));
   LGH_PASS(c->vcg_tickets.alloc(2 * kTicketSlot, true));
   return LGH_OK;
}

// Several ranks: which exchange follows K2 - accumulator words or three doubles - must be the same on every rank, and whether a
// rank CAN use the words depends on its own kernels (the slab K1 is dispatched by the rank's zone count): a MIN over the ranks,
// once per set of tables and per form of K1 (the mass data may change it between solves: rz_words_key).  Whether the energy CG
// can ride on this solve's exchanges (lockstep, DESIGN.md 6: a fourth scalar on the halo messages, whose LENGTH both ends must
// agree on) is asked in the same exchange.  Only vcg_solve, which every rank enters together, may ask (in_solve).
static int vcg_mode_collective(lgh_ctx *c, VcgAux *aux, const VcgK1 &k1, const bool in_solve, VcgMode &m)
{
   const int key = (m.rz_words ? 1 : 0) | (k1.form << 10);
   if (aux->rz_words_key != key) { aux->rz_words_all = -1; }
   if (aux->rz_words_all < 0 && !in_solve) { m.rz_words = false; }
   else if (aux->rz_words_all < 0)
   {
      aux->rz_words_key = key;
      const double mine[2] = {m.rz_words ? 1.0 : 0.0, m.ls_mine ? 1.0 : 0.0};
      LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
      LGH_HIP_CHECK(hipMemcpy(c->scal + 12, mine, sizeof(mine), hipMemcpyHostToDevice)); // (pageable host memory: synchronous copies)
      LGH_PASS(allreduce_dev(c, c->scal + 12, 2, 1));
      double all[2] = {0.0, 0.0};
      LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
      LGH_HIP_CHECK(hipMemcpy(all, c->scal + 12, sizeof(all), hipMemcpyDeviceToHost));
      aux->rz_words_all = (all[0] > 0.5) ? 1 : 0;
      aux->ls_all = (all[0] > 0.5 && all[1] > 0.5) ? 1 : 0;
   }
   m.rz_words = m.rz_words && aux->rz_words_all == 1;
   return LGH_OK;
}

// ---- vcg_prepare, step 3: how this solve runs (VcgMode, lgh_vcg.hpp) - every flag once, here
static int vcg_mode(lgh_ctx *c, VcgAux *aux, const VcgK1 &k1, const bool in_solve, VcgMode &m)
{
   m = VcgMode();
   m.multi = c->multi != 0;
   m.mixed = m.multi && c->t_deg <= 8;
   m.direct = !m.multi && c->t_deg <= 8;
   m.k2p = aux->ellz != nullptr && c->sw.k2p;
   m.limbs = c->sw.slab_exact && m.k2p && k1.form == kK1Slab && aux->limbs != nullptr;
   // rz_limbs mode: one rank, exact accumulators with the deferred fold (LGH_RZ_LIMBS=0: the ticketed fold of (r, z) in K2)
   // (several ranks, round 5: all-pairs partitions, where the words of every rank reach every other in one exchange)
   // (a communicator of size 1 - LGH_FORCE_MULTI - has nobody to exchange with: the words are complete as they are)
   m.rz_words = m.limbs && (!m.multi || ((halo_can_piggyback(c) || c->nranks == 1) && c->t_deg <= 8)) && c->sw.rz_limbs;
   HaloPackTables hp;
   const uint8_t *hmask = nullptr;
   const int *sh_node = nullptr;
   if (m.multi) { comm_shared_nodes(c, &hmask, &sh_node, &m.n_shared); }
   if (m.multi && m.rz_words)
   {
      m.ls_mine = m.k2p && c->t_deg <= 8 && l2_lockstep_possible(c) && comm_ranks_before(c) >= 0 &&
                  (m.n_shared == 0 || (c->sw.halo_fused_pack && halo_can_piggyback(c) && comm_pack_tables(c, &hp)));
   }
   if (m.multi && c->nranks == 1) { aux->ls_all = m.ls_mine ? 1 : 0; }
   if (m.multi && c->nranks > 1) { LGH_PASS(vcg_mode_collective(c, aux, k1, in_solve, m)); }
   m.rzl = m.rz_words && c->sw.slab_defer && aux->rzl != nullptr; // (needs the deferred fold of (d, A d) as well)
   // (LGH_SLAB_DEFER=0, A/B: the last workgroup of K1 folds the accumulators (ticket), K2 reads the result)
   m.den_limbs = (m.limbs && c->sw.slab_defer) ? (m.multi ? 2 : 1) : 0; // (several ranks: folded before the exchange, vcg_fold_den)
   // several ranks, bounded-grid K2: the shared-node gather fills the send buffer of the halo exchange itself (and
   // the local (d, A d) with it where the sums ride on the messages), the last workgroup of K2 the one of the
   // (r, z) exchange - two launches less per iteration (A/B: LGH_HALO_FUSED_PACK=0)
   if (c->sw.halo_fused_pack && m.mixed && m.k2p && m.n_shared > 0 && comm_pack_tables(c, &hp))
   {
      m.pack_halo = 1;
      m.nx_den = halo_can_piggyback(c) ? (c->energy.mode == EnergySolve::Lockstep ? kVC + 1 : kVC) : 0; // (lockstep energy CG: its (d, M d) rides along, VcgScalars::den_e)
      m.pack_rz = (halo_can_piggyback(c) && !m.rzl) ? 1 : 0; // (rz_limbs mode: (r, z) travels as accumulator words, exchange_words)
   }
   if (in_solve)
   {
      // (the collective answer, and nothing of this rank's own has changed since it was given)
      aux->ls_ready = (m.multi && aux->ls_all == 1 && m.ls_mine && m.rzl && (m.n_shared == 0 || (m.pack_halo && halo_can_piggyback(c)))) ? 1 : 0;
   }
   // the energy CG in lockstep (lgh_solve_energy_begin set it up on this stream): see vcg_iterate_exchange
   m.ls = c->energy.mode == EnergySolve::Lockstep && m.multi && m.rzl && aux->ls_ready && (m.n_shared == 0 || m.nx_den == kVC + 1);
   return LGH_OK;
}

// the solve runs in the library's own order: per-zone and per-node data of the context through the permutation (copies,
// refreshed when the mass data or the Jacobi diagonal have changed since they were taken), tables and vectors of that order
static int vcg_fill_internal_order(lgh_ctx *c, VcgAux *aux, const VcgK1 &k1, const VcgMode &m, VcgArgs &a)
{
   const bool need_table = a.dqs != 0 || k1.form == kK1Column; // (the column form of K1 reads the stored table whatever the compact form says)
   if (aux->o_mass_gen != c->mass_gen)
   {
      LGH_PASS(order_gather_nodes(c, c->dinvV, aux->o_dinv, 1));
      if (a.dqs == 0) { LGH_PASS(order_zone_blocks(c, a.Se, aux->o_Se, 1, false)); }
      if (need_table)
      {
         if (!aux->o_massD) { LGH_PASS(aux->o_massD.alloc((size_t)c->NE * c->NQ + 2048, true)); }
         LGH_PASS(order_zone_blocks(c, c->massD, aux->o_massD, c->NQ, false));
      }
      aux->o_mass_gen = c->mass_gen;
   }
   if (a.dqs == 0) { a.Se = aux->o_Se; }
   else { a.Dq = aux->o_massD; } // (a.Se: ones)
   a.DqFull = need_table ? aux->o_massD.p : nullptr;
   a.map = aux->o_map;
   a.ell = aux->o_ell;
   for (int k = 0; k < kVC; k++) { a.ess[k] = aux->o_ess[k]; }
   a.dinv = aux->o_dinv;
   a.owner = m.multi ? aux->o_owner.p : nullptr;
   a.ncaller = aux->ord->ncaller_d;
   a.x = aux->o_x;
   return LGH_OK;
}

// ---- vcg_prepare, step 4: the argument block from the context, the tables and the mode
static int vcg_fill_args(lgh_ctx *c, VcgAux *aux, const VcgK1 &k1, const VcgMode &m, double *B, double *X, const double rel_tol, const bool in_solve, VcgArgs &a)
{
   const size_t N = (size_t)c->N;
   memset(&a, 0, sizeof(a));
   a.NE = c->NE;
   a.N = c->N;
   a.B = c->B;
   a.DqFull = c->massD;
   LGH_PASS(mass_data(c, &a.Dq, &a.dqs, &a.Se));
   a.w1 = (a.dqs == 0) ? c->w1d : nullptr;
   a.M1 = (a.dqs == 0 && c->w1d) ? c->M1h : nullptr; // (nullptr with LGH_MASS_KRON=0)
   a.map = c->h1map;
   a.ell = c->t_ell;
   a.deg = c->t_deg;
   for (int k = 0; k < kVC; k++) { a.ess[k] = c->essmask[k]; }
   a.dinv = c->dinvV;
   a.owner = m.multi ? c->owner : nullptr;
   a.b = B;
   a.x = X;
   if (aux->ord) { LGH_PASS(vcg_fill_internal_order(c, aux, k1, m, a)); }
   a.r = c->vcg_vec;
   a.d = c->vcg_vec + kVC * N;
   a.yL = c->vcg_vec + 2 * kVC * N;
   a.YE = aux->ye;
   a.ye_stride = (size_t)c->NE * c->ND + kYePad;
   a.ye_wide = (a.ye_stride * 8 * kVC >= 0xffffffffull || c->sw.slab_ye_wide) ? 1 : 0; // (LGH_SLAB_YE_WIDE=1, test hook: the per-set 64-bit store base on a mesh that does not need it)
   a.ellz = aux->ellz;
   a.essbits = aux->essbits;
   a.nstart = aux->nstart;
   a.mapb = aux->mapb;
   a.map_xrows = aux->map_xrows;
   if (k1.form == kK1Slab && aux->settab)
   {
      // merged E-vector layout: K1 stores by the set table, everybody who reads Y_E goes through the tables of that layout
      a.settab = aux->settab;
      a.ell = aux->ellm;
      a.deg = aux->degm;
      a.ellz = aux->ellzm;
      a.nstart = aux->nstartm;
   }
   a.limbs = m.limbs ? aux->limbs.p : nullptr;
   a.rzl = m.rzl ? aux->rzl.p : nullptr;
   // (a solve resets its scalars and accumulators in its first kernel; the hooks and statistics entry points, which launch
   //  single kernels on state of their own, had vcg_set_tol_k do it: vcg_prepare)
   a.reset = in_solve ? 1 : 0;
   a.reset_tol2 = rel_tol * rel_tol;
   if (m.rzl && m.multi) { LGH_PASS(comm_word_peers(c, kLimbWords, &a.rzl_peers, &a.n_rz_peers)); }
   a.queue = a.limbs ? (unsigned *)(a.limbs + 2 * kLimbWords) : nullptr;
   a.den_limbs = m.den_limbs;
   a.k2_skip = c->sw.k2_skip;
   a.s = c->vcg_s;
   a.stride = c->vcg_stride;
   a.multi = m.multi ? 1 : 0;
   // debug: LGH_VCG_TRACE=<file> dumps "block start loop_end end (xcc<<32|hw_id)" of the
   // last K1 launch of every solve, in 10 ns ticks
   if (!c->sw.vcg_trace.empty())
   {
      if (!aux->trace) { (void)aux->trace.alloc((size_t)kTraceRec * kTraceBlocks, true); }
      a.trace = aux->trace;
      if (a.trace) { (void)hipMemsetAsync(a.trace, 0, (size_t)kTraceRec * kTraceBlocks * sizeof(unsigned long long), c->stream); }
   }
   if (m.multi)
   {
      comm_shared_nodes(c, &a.hmask, &a.sh_node, &a.n_shared);
      if (aux->ord && a.n_shared > 0) { a.hmask = aux->o_hmask; a.sh_node = aux->o_shnode; } // (the same nodes by their internal numbers)
   }
   if (m.pack_halo) { (void)comm_pack_tables(c, &a.hp); }
   a.pack_halo = m.pack_halo;
   a.nx_den = m.nx_den;
   a.pack_rz = m.pack_rz;
   return LGH_OK;
}

// B, X: dim*N (byNODES).  Everything a launch of the lockstep kernels needs, in four steps: work buffers, tables, mode,
// argument block.  in_solve: the call comes from vcg_solve, which every rank enters together - only there may a collective
// run (vcg_mode_collective); the statistics and test entry points take the conservative answer until a solve has decided.
// They launch single kernels on state of their own: for them vcg_set_tol_k resets scalars and accumulators on the context
// stream (a solve does that in its first kernel, VcgArgs::reset).
int vcg_prepare(lgh_ctx *c, double *B, double *X, double rel_tol, VcgPlan &plan, const bool in_solve)
{
   LGH_PASS(vcg_work_buffers(c));
   if (!c->vcg_aux) { LGH_PASS(vcg_build_aux(c)); } // (first solve, or the communicator has changed since)
   VcgAux *aux = c->vcg_aux.get();
   plan.aux = aux;
   plan.k1 = vcg_resolve_k1(c);
   LGH_PASS(vcg_mode(c, aux, plan.k1, in_solve, plan.mode));
   const VcgMode &m = plan.mode;
   if (!in_solve)
   {
      hipLaunchKernelGGL(vcg_set_tol_k, dim3(1), dim3(1), 0, c->stream, c->vcg_s.p, rel_tol * rel_tol, m.limbs ? aux->limbs.p : nullptr,
                         m.rzl ? aux->rzl.p : nullptr);
   }
   return vcg_fill_args(c, aux, plan.k1, m, B, X, rel_tol, in_solve, plan.a);
}

// ---- vcg_solve in pieces -----------------------------------------------------------------
static_assert((kPinVcg + (sizeof(VcgScalars) + sizeof(double) - 1) / sizeof(double)) <= (size_t)kPinVcgToken, "VcgScalars ends before the token slot of the pinned block");

struct VcgRun // one solve in progress
{
   VcgScalars *ds, *hs;           // the scalars on the device; their copy in the host's pinned block, as of the last look
   const HaloNodeAlias *alias;    // the exchange's node lists in the solve's own numbering (a.yL is numbered that way), or nullptr
   int max_iter, chunk, it = 0, looks = 0;
   bool energy_polled = false;
   int ls_limit, ls_before;       // lockstep energy CG: iterations worth interleaving, peers of lower rank
};

// init (vector kernels use reduction slot 0, the element kernel slot 1)
// force_E != nullptr: B and X are outputs - the init kernel forms B = -(H1R^T force_E) with the essential rows zeroed and
// X = 0 itself (single rank only; see vcg_init_force_k).
static int vcg_start(lgh_ctx *c, VcgPlan &plan, double *B, const double *force_E)
{
   VcgArgs &a = plan.a;
   const VcgAux *aux = plan.aux;
   const int nb = ceil_div(a.N, 256);
   a.partials = c->vcg_partials;
   a.ticket = c->vcg_tickets;
   if (force_E)
   {
      if (!plan.mode.direct) { set_error("vcg_solve: fused init is single-rank, degree <= 8"); return LGH_ERR_ARG; }
      if (aux->ellf && aux->essbits) { hipLaunchKernelGGL(vcg_init_force_z_k, dim3(nb), dim3(256), 0, c->stream, a, force_E, 8u * (unsigned)c->ND, aux->ellf, B); }
      else { hipLaunchKernelGGL(vcg_init_force_k<8>, dim3(nb), dim3(256), 0, c->stream, a, force_E, c->ND, B, aux->o_ellc ? aux->o_ellc : c->t_ell, c->t_deg); }
   }
   else
   {
      if (aux->ord) { LGH_HIP_CHECK(hipMemsetAsync(a.x, 0, kVC * (size_t)a.N * sizeof(double), c->stream)); } // (X = 0 on entry: the solve's own copy as well)
      hipLaunchKernelGGL(vcg_init_k, dim3(nb), dim3(256), 0, c->stream, a);
   }
   LGH_HIP_CHECK(hipGetLastError());
   if (plan.mode.multi)
   {
      LGH_PASS(allreduce_dev(c, a.s->rz, kVC, 0));
      hipLaunchKernelGGL(vcg_init_finish_k, dim3(1), dim3(1), 0, c->stream, a.s);
   }
   return LGH_OK;
}

// The host looks at the scalars: stop is set when every component is done or the iterations have run out; otherwise
// the next chunk is sized.  Several ranks: the outcome of the last enqueued update is still pending (vcg_pending_update) -
// the one-thread kernel that commits it also puts the scalars into the host's pinned memory, the token last: no copy
// kernel between it and the synchronisation.
static int vcg_look(lgh_ctx *c, const VcgPlan &plan, VcgRun &r, bool &stop)
{
   const VcgArgs &a = plan.a;
   VcgScalars *hs_dev = (VcgScalars *)(c->host_pinned_dev + kPinVcg);
   unsigned long long *tok_dev = (unsigned long long *)(c->host_pinned_dev + kPinVcgToken);
   volatile unsigned long long *tok = (volatile unsigned long long *)(c->host_pinned + kPinVcgToken);
   const unsigned long long token = ++c->look_token;
   bool copied = false;
   // the first look of a solve comes after a whole chunk of iterations: the energy solve on the second stream is
   // brought to its end meanwhile (its looks used to wait behind the velocity solve, with the GPU idle)
   if (!r.energy_polled) { r.energy_polled = true; LGH_PASS(energy_overlap_poll(c)); }
   if (plan.mode.multi && !a.rzl && r.it > 0) { hipLaunchKernelGGL(vcg_update_finish_k, dim3(1), dim3(1), 0, c->stream, r.ds, r.it, hs_dev, tok_dev, token); copied = true; }
   if (a.rzl && r.it > 0) { vcg_launch_rz_finish(c, a, r.it, hs_dev, tok_dev, token); copied = true; }
   if (copied)
   {
      // (on several ranks the exchanges that follow are host-synchronous on the loopback transports and enqueue-only over
      //  RCCL: either way nothing of this rank is in flight behind the finishing kernel)
      LGH_PASS(host_wait_token(c, tok, token));
   }
   else
   {
      LGH_HIP_CHECK(hipMemcpyAsync(r.hs, r.ds, sizeof(VcgScalars), hipMemcpyDeviceToHost, c->stream));
      LGH_HIP_CHECK(hipStreamSynchronize(c->stream));
   }
   stop = r.hs->all_done || r.it >= r.max_iter;
   if (!stop) { r.chunk = (++r.looks <= 2) ? 2 : std::min(64, 2 * r.chunk); } // (as scg_finish, lgh_scg.hip)
   return LGH_OK;
}

// K1 of iteration a.iter (reduction slot 1; what follows uses slot 0 again)
static int vcg_step_k1(lgh_ctx *c, const VcgPlan &plan, VcgArgs &a)
{
   a.partials = c->vcg_partials + (size_t)kVC * c->vcg_stride;
   a.ticket = c->vcg_tickets + kTicketSlot;
   kt_begin(c, LGH_KERNEL_MASS_CG_H1);
   vcg_launch_k1(c, plan, a);
   kt_end(c, LGH_KERNEL_MASS_CG_H1);
   LGH_HIP_CHECK(hipGetLastError());
   a.partials = c->vcg_partials;
   a.ticket = c->vcg_tickets;
   return LGH_OK;
}

// one iteration on one rank (valence <= 8): K1, then K2 gathers A d itself
static int vcg_iterate_direct(lgh_ctx *c, const VcgPlan &plan, VcgArgs &a)
{
   LGH_PASS(vcg_step_k1(c, plan, a));
   if (plan.mode.k2p) { vcg_launch_k2p(c, plan, a, a.iter); }
   else { kt_begin(c, LGH_KERNEL_CG_UPDATE_H1); vcg_launch_update(c, a, true); kt_end(c, LGH_KERNEL_CG_UPDATE_H1); }
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}

// One iteration with A d as L-vectors between K1 and K2 - several ranks (only at the nodes shared with other ranks when K2
// can gather the rest itself: mode.mixed), or one rank with an unusual valence: gather, (d, A d) folded, shared nodes and
// (d, A d) summed across ranks, K2, (r, z) summed across ranks - as accumulator words or by an all-reduce.  The energy CG in
// lockstep (mode.ls; lgh_scg.hip) runs one of its iterations per velocity iteration while it has some left of the count it
// needed last time: apply behind K1, update behind K2, its (d, M d) on the halo messages (den_e), its (r, r) in a word of the
// word exchange, and in its last interleaved iteration of a chunk (upto: where the chunk ends) its fold behind that exchange.
static int vcg_iterate_exchange(lgh_ctx *c, const VcgPlan &plan, VcgArgs &a, const VcgRun &r, const int upto)
{
   const VcgMode &m = plan.mode;
   const int it = a.iter, nb = ceil_div(a.N, 256);
   const bool ls_it = m.ls && it <= r.ls_limit;
   auto ls_words = [&](const int set_it) { return LockstepWords{a.rzl + (set_it % 3) * kLimbWords, a.rzl_peers, a.n_rz_peers, r.ls_before}; };
   LGH_PASS(vcg_step_k1(c, plan, a));
   if (ls_it) { LGH_PASS(l2_lockstep_apply(c, it, ls_words(it - 1), &r.ds->den_e)); } // (the messages are packed after this)
   if (m.mixed)
   {
      if (a.n_shared > 0) { hipLaunchKernelGGL(vcg_gather_list_k, dim3(ceil_div(a.n_shared, 256)), dim3(256), 0, c->stream, a); }
      else if (a.den_limbs == 2) { vcg_launch_fold_den(c, a); }
   }
   else
   {
      if (a.den_limbs == 2) { vcg_launch_fold_den(c, a); }
      hipLaunchKernelGGL(vcg_gather_k, dim3(nb), dim3(256), 0, c->stream, a);
   }
   LGH_HIP_CHECK(hipGetLastError());
   if (m.multi)
   {
      // (d, A d): summed over the ranks by the halo messages themselves when every
      // rank is a neighbour of every other, by an all-reduce otherwise
      const bool ride = halo_can_piggyback(c);
      LGH_PASS(halo_sum(c, a.yL, kVC, ride ? r.ds->den : nullptr, ride ? std::max(a.nx_den, kVC) : 0, a.pack_halo != 0, r.alias));
      if (!ride) { LGH_PASS(allreduce_dev(c, r.ds->den, kVC, 0)); }
   }
   // (the bounded-grid K2 knows the shared nodes and the owner weights from its flag bytes)
   if (m.mixed && m.k2p) { vcg_launch_k2p(c, plan, a, it); }
   else { vcg_launch_update(c, a, m.mixed); }
   if (ls_it) { LGH_PASS(l2_lockstep_update(c, it, &r.ds->den_e, a.rzl + (it % 3) * kLimbWords)); } // (reads the summed (d, M d); the word exchange carries its (r, r))
   if (m.multi && a.rzl)
   {
      // exact all-reduce of (r, z): the accumulator words K2 just added into go to every peer as they are - no fold,
      // no pack, no combine kernel; the next K1 (or vcg_rz_finish_k) adds own and peers' words before it folds
      LGH_PASS(exchange_words(c, a.rzl + (it % 3) * kLimbWords, kLimbWords));
      if (ls_it && (it == r.ls_limit || it == upto))
      {
         // the energy CG's last interleaved iteration of this chunk: its outcome is committed now, while the peers'
         // words of THIS exchange are still in the buffer (the next apply, if there is one, finds the same sum)
         LGH_PASS(l2_lockstep_fold(c, it, ls_words(it)));
      }
   }
   else if (m.multi) { LGH_PASS(allreduce_dev(c, r.ds->rz, kVC, 0, a.pack_rz != 0 && m.mixed && m.k2p)); } // convergence is looked at by the next K1 (vcg_pending_update)
   LGH_HIP_CHECK(hipGetLastError());
   return LGH_OK;
}

// the solution to the caller, the trace, iters[k] = GetNumIterations() of component k
static int vcg_finish(lgh_ctx *c, const VcgPlan &plan, const VcgRun &r, double *X, int iters[3])
{
   const VcgArgs &a = plan.a;
   const int nb = ceil_div(a.N, 256);
   if (plan.aux->ord)
   {
      // the solution, in the caller's numbering, into the caller's vector (with the pending update of vcg_xfix_k)
      hipLaunchKernelGGL(vcg_xout_k, dim3(nb), dim3(256), 0, c->stream, a, X);
      LGH_HIP_CHECK(hipGetLastError());
   }
   else if (plan.mode.k2p && ((r.hs->nupd[0] | r.hs->nupd[1] | r.hs->nupd[2]) & 1))
   {
      // x lags one update behind for the components that stopped after an odd number of updates
      hipLaunchKernelGGL(vcg_xfix_k, dim3(nb), dim3(256), 0, c->stream, a);
      LGH_HIP_CHECK(hipGetLastError());
   }
   FILE *f = a.trace ? fopen(c->sw.vcg_trace.c_str(), "w") : nullptr; // debug (LGH_VCG_TRACE=<file>): the last K1 launch, a line per workgroup
   if (f)
   {
      std::vector<unsigned long long> h((size_t)kTraceRec * kTraceBlocks);
      (void)hipMemcpy(h.data(), a.trace, h.size() * 8, hipMemcpyDeviceToHost);
      for (int i = 0; i < kTraceBlocks; i++)
      {
         if (h[(size_t)kTraceRec * i] == 0) { continue; } // (no such workgroup in the last launch)
         fprintf(f, "%d", i);
         for (int k = 0; k < kTraceRec; k++) { fprintf(f, " %llu", h[(size_t)kTraceRec * i + k]); }
         fprintf(f, "\n");
      }
      fclose(f);
   }
   int mx = 0;
   for (int k = 0; k < kVC; k++)
   {
      // upstream: final_iter = max_iter when the loop runs out without converging
      int fin = r.hs->iters[k];
      if (!r.hs->done[k] && r.it >= r.max_iter) { fin = r.max_iter; }
      iters[k] = fin;
      mx = std::max(mx, fin);
   }
   c->vcg_last = mx;
   return LGH_OK;
}

// B, X: dim*N (byNODES).  X must be zero on entry (dv = 0, laghos_solver.cpp:338, :382); force_E: see vcg_start.
// iters[c] = GetNumIterations() of component c.
int vcg_solve(lgh_ctx *c, double *B, double *X, double rel_tol, int max_iter, int iters[3], const double *force_E)
{
   if (!vcg_available(c)) { return LGH_ERR_UNSUPPORTED; }
   VcgPlan plan;
   LGH_PASS(vcg_prepare(c, B, X, rel_tol, plan, true));
   VcgArgs &a = plan.a;
   const VcgMode &m = plan.mode;
   VcgRun r;
   r.ds = a.s;
   r.hs = (VcgScalars *)(c->host_pinned + kPinVcg);
   r.alias = (plan.aux->ord && plan.aux->o_alias.nodes) ? &plan.aux->o_alias : nullptr;
   r.max_iter = max_iter;
   r.chunk = c->vcg_last > 0 ? c->vcg_last : 8; // first chunk = iteration count of the previous velocity solve (see cg_solve, lgh_scg.hip)
   r.ls_limit = m.ls ? std::min(l2_lockstep_limit(c), max_iter) : 0;
   r.ls_before = m.ls ? comm_ranks_before(c) : 0;
   LGH_PASS(vcg_start(c, plan, B, force_E));
   // The first chunk is enqueued without looking at the flag first (an all-zero right-hand side just makes its launches
   // return at once): one host round trip, with the GPU idle meanwhile, less per solve.
   for (bool first_look = true;; first_look = false)
   {
      if (!first_look || max_iter <= 0)
      {
         bool stop = false;
         LGH_PASS(vcg_look(c, plan, r, stop));
         if (stop) { break; }
      }
      const int upto = std::min(max_iter, r.it + r.chunk);
      while (r.it < upto)
      {
         a.iter = ++r.it;
         LGH_PASS(m.direct ? vcg_iterate_direct(c, plan, a) : vcg_iterate_exchange(c, plan, a, r, upto));
      }
   }
   return vcg_finish(c, plan, r, X, iters);
}

} // namespace lgh
