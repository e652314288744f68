// lgh_mass.hpp — what the mass operator (lgh_mass.hip) and the scalar CG on top of it (lgh_scg.hip) share: the argument block
// of the element kernels, the decisions a kernel of the CG takes for the kernel before it on several ranks, and the launchers
// the CG needs.
#pragma once
#include "lgh_common.hpp"

namespace lgh
{

// ---------------------------------------------------------------------------
// element kernel: y_e = B^T diag(D_e) B x_e
//   MODE 0: x is an E-vector (or L2 vector), plain apply
//   MODE 1: x gathered from an L-vector through `map`
//   MODE 2: CG K1 (H1): d = z[map] + beta * d_old[map] (not stored); den
//   MODE 3: CG K1 (L2, no map): d = r + beta*d_old, stored in place (element-local)
// ---------------------------------------------------------------------------
struct MassArgs
{
   int NE;
   const double *B;   // [q + Q*d]
   const double *Dq;  // [q + NQ*e] - mass_apply_l2_plane: value(q, e) = Dq[q + dqs e] * Se[e] (mass_data)
   const double *Se;
   int dqs;
   const double *M1;  // mass_apply_l2_kron: the 1-D mass tile of the L2 basis (L x L)
   const double *w1;  // mass_apply_l2_plane<.., SEP = true>: one-dimensional weights, value(q, e) = Se[e] w1[qx] w1[qy] w1[qz] (compact data of a tensor-product rule)
   const double *x;   // MODE 0/1 input; MODE 2/3: z (H1) or r (L2)
   const int *map;    // NE*ND or null
   double *y;         // E-vector (H1) or L2 vector output
   // CG
   double *d;         // direction vector (read; MODE 3 also writes it in place)
   CgScalars *cgs;
   double *partials;
   unsigned int *ticket;
   int multi; // multi-GPU: den is all-reduced before any decision is taken on it
   int iter;  // CG iteration this launch belongs to (several ranks: see cg_pending_update)
   // mass_apply_l2_kron, fused update of the energy CG (round 6): MODE 3 with no_y does not store M d - MODE 4, the update of the
   // same iteration, forms it again from d (the L2 mass matrix is block diagonal: M d of a zone needs that zone's d only) and
   // updates ux (x) and ur (r) with it: ten vector passes per iteration become eight
   int no_y;
   double *ux, *ur;
   // lockstep with the velocity CG on several ranks (lgh_common.hpp): the rank sums of this solve's two dot products travel with
   // the velocity iteration's exchanges instead of in exchanges of their own
   LockstepWords ls;        // MODE 3: the accumulator-word sets of the iteration before, own and peers': word kLsWord = that rank's (r, r)
   int ls_on;               // 1: MODE 3 takes (r, r) from ls instead of cgs->rz; MODE 4 takes (d, M d) from ls_den_src
   double *ls_den_mirror;   // MODE 3: the local (d, M d) also goes here (VcgScalars::den_e: behind the halo messages)
   const double *ls_den_src;// MODE 4: the rank-summed (d, M d)
   long long *ls_word_out;  // MODE 4: the local (r, r), as bits, into word kLsWord of the set the exchange after K2 sends
};

// lockstep: (r, r) of the iteration before = the ranks' values in rank order (own value between the lower and the higher peers)
__device__ __forceinline__ double lockstep_rz(const LockstepWords &w)
{
   double rz = 0.0;
   for (int p = 0; p < w.before; p++) { const double v = __longlong_as_double(w.peers[(size_t)p * kLsWordsPerSet + kLsWord]); rz = (p == 0) ? v : rz + v; }
   {
      const double v = __longlong_as_double(w.own[kLsWord]);
      rz = (w.before == 0) ? v : rz + v;
   }
   for (int p = w.before; p < w.n_peers; p++) { rz += __longlong_as_double(w.peers[(size_t)p * kLsWordsPerSet + kLsWord]); }
   return rz;
}
// ... and what the next kernel of the sequence does with it (cg_pending_update with the sum formed here): convergence looked at,
// the outcome committed by one thread; returns true when the solve has converged
__device__ __forceinline__ bool lockstep_pending_update(CgScalars *s, const int iter, const double rz, const bool commit)
{
   const bool conv = rz < 0.0 || rz <= s->r0;
   if (commit)
   {
      __hip_atomic_store(&s->iters, iter - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (conv)
      {
         __hip_atomic_store(&s->done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
         __hip_atomic_store(&s->rz, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
         __hip_atomic_store(&s->den, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      else { __hip_atomic_store(&s->rz, rz, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } // (the update of this iteration divides it by (d, M d))
   }
   return conv;
}

// Several ranks: the sums of den and (r, z) over the ranks complete outside the kernels that produce the
// local parts, so the decisions they feed (breakdown, convergence, iteration count) are taken by the NEXT
// kernel of the sequence instead of a single-thread kernel after every exchange: each workgroup evaluates the
// same predicate on the same reduced values, and thread 0 of workgroup 0 also commits the outcome to the
// state.  A commit only writes values under which the predicate stays true (done = 1, rz = den = 0: sums of
// zeros stay zero in the exchanges of launches enqueued past convergence), so a thread that reads the
// state after the commit decides like one that read it before.
// K1 of iteration iter >= 2: outcome of the update of iteration iter - 1.
__device__ __forceinline__ bool cg_pending_update(CgScalars *s, const int iter, const bool commit)
{
   const double rz = s->rz;
   const bool conv = rz < 0.0 || rz <= s->r0;
   if (commit)
   {
      // write-through stores: another XCD's L2 may hold the same line dirty (K1's last workgroup writes den / first)
      __hip_atomic_store(&s->iters, iter - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (conv)
      {
         __hip_atomic_store(&s->done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
         __hip_atomic_store(&s->rz, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
         __hip_atomic_store(&s->den, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
   }
   return conv;
}
// K2: breakdown (den == 0 after the sum over the ranks), as upstream
__device__ __forceinline__ bool cg_pending_den(CgScalars *s, const bool commit)
{
   const bool brk = s->den == 0.0;
   if (brk && commit)
   {
      __hip_atomic_store(&s->done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&s->rz, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
   }
   return brk;
}

// ---- launchers of lgh_mass.hip the scalar CG is written on
MassArgs base_args(lgh_ctx *c, int space);
// K1 of a CG iteration: the apply in CG mode for a space (H1: MODE 2, L2: MODE 3)
int mass_apply_cg(lgh_ctx *c, int space, const MassArgs &m);
int mass_gather(lgh_ctx *c, const double *YE, const uint8_t *ess, double *y); // y[n] = sum of the E-vector's contributions to node n; essential rows zeroed
// The energy CG's update as a second launch of the Kronecker kernel (MODE 4) instead of cg_update_k: when the L2 apply runs in
// its Kronecker form.  LGH_L2_FUSED=0: cg_update_k reads the stored product (rounds 1-5).
bool l2_fused_update(lgh_ctx *c);
// ... its launch: x (ux) and r (ur) of the solve, the reduction slot of its (r, r); the iteration is m.iter
int mass_l2_fused_update(lgh_ctx *c, const MassArgs &m, double *ux, double *ur, double *partials, unsigned int *ticket);

} // namespace lgh
