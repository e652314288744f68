/* laghos_hip.h — C ABI of the MI355X-native Laghos partial-assembly hot path.
 *
 * This is the drop-in boundary: the reference's C++ operator
 * classes keep their shape (laghos_amd/host/) and their Mult / MultTranspose /
 * UpdateQuadratureData bodies become calls into this library of hand-written
 * HIP kernels for gfx950.  Plain C types only; no torch / MFEM types.
 *
 * Conventions
 *  - Every `const double*` / `double*` vector argument is a DEVICE pointer owned
 *    by the caller (the reference's mfem::Vector device memory).  Pointers inside
 *    lgh_config are HOST pointers, copied at creation.
 *  - L-vectors use the reference layouts: H1 vectors are byNODES (component c at
 *    [c*N, (c+1)*N)), element-local dofs lexicographic; L2 dofs are e*L1D^dim + l
 *    (SURVEY A2-A4).  S = [x | v | e] with offsets {0, dim*N, 2*dim*N}
 *    (/root/reference/laghos_solver.cpp:166-169).
 *  - dim = 1 (segments; README run 5) runs the reference's full-assembly path, to which
 *    1D always switches (laghos.cpp:454-462), through the same entry points: S = [x | v | e]
 *    with offsets {0, N, 2N}, stressJinvT[e*NQ+q], Jac0inv[e*NQ+q], L2 dofs e*L1D + l.  The
 *    operators are those of the PA path except the energy solve: zone by zone with the
 *    factored mass matrices Me(z) (lgh_l2_mass_solve_local), no CG.  One rank only.  Entry
 *    points that exist for a 2D/3D kernel form (E-vector hooks, lockstep solve) refuse dim 1.
 *  - All work is enqueued on the context's HIP stream; calls are asynchronous
 *    unless they return a scalar to the host (documented per function).
 *  - Return value: 0 = LGH_OK, non-zero = error; lgh_last_error() gives the text.
 *    The reference aborts on the same conditions (MFEM_ABORT "Unknown kernel",
 *    laghos_assembly.cpp:549-553); the C++ shells turn non-zero into abort().
 *  - Not re-entrant per context; one host thread / one process per GPU.
 */
#ifndef LAGHOS_HIP_H
#define LAGHOS_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define LGH_OK 0
#define LGH_ERR_ARG 1         /* bad argument */
#define LGH_ERR_UNSUPPORTED 2 /* (dim,D1D,Q1D) has no kernel: "Unknown kernel 0x..." */
#define LGH_ERR_HIP 3         /* HIP runtime error */
#define LGH_ERR_COMM 4        /* RCCL error */

#define LGH_SPACE_H1 0 /* scalar H1 space "H1c" (laghos_solver.cpp:121) */
#define LGH_SPACE_L2 1

typedef struct lgh_ctx lgh_ctx;

/* Everything ForcePAOperator / MassPAOperator / QUpdate constructors pull out of
 * the MFEM spaces (laghos_assembly.cpp:123-143, :80-96; laghos_solver.hpp:72-89). */
typedef struct lgh_config
{
   int dim, NE;            /* mesh dimension (1|2|3), local elements */
   int D1D, Q1D, L1D;      /* H1 dofs, quadrature points, L2 dofs per direction */
   int N;                  /* local scalar H1 nodes (H1c.GetVSize()) */
   const int *h1_map;      /* NE*D1D^dim: node of element-local lexicographic dof
                              (ElementRestriction, LEXICOGRAPHIC; assembly.cpp:133) */
   const double *B_h1;     /* Q1D*D1D, B[q + Q1D*d]  (DofToQuad::TENSOR, assembly.cpp:141-142) */
   const double *G_h1;     /* Q1D*D1D, derivative table */
   const double *B_l2;     /* Q1D*L1D */
   const double *weights;  /* NQ = Q1D^dim integration weights (ir.GetWeights()) */
   const double *gamma;    /* NE: order-0 L2 gamma grid function (laghos.cpp:628-632) */
   int ess_count[3];       /* c_tdofs[c].Size()  (laghos_solver.cpp:187-195) */
   const int *ess[3];      /* c_tdofs[c]: scalar nodes with v_c = 0 */
   const double *owner;    /* N, 1.0 where this rank owns the node, 0.0 where a lower
                              rank does (T-vector dot products); NULL = all owned */
   int use_viscosity, use_vorticity;
   double cfl;
   int order_v;            /* H1.GetOrder(0): h1order in QUpdateBody */
   int device;             /* HIP device ordinal */
   void *stream;           /* hipStream_t to use, or NULL to create one */
} lgh_config;

const char *lgh_last_error(void);
const char *lgh_version(void);

int lgh_create(const lgh_config *cfg, lgh_ctx **out);
int lgh_destroy(lgh_ctx *ctx);
int lgh_sync(lgh_ctx *ctx); /* hipStreamSynchronize on the context stream */
void *lgh_stream(lgh_ctx *ctx);

/* ---- QuadratureData (laghos_assembly.hpp:31-62); device arrays owned by ctx.
 *   stressJinvT[(e*NQ+q) + NE*NQ*(gd + dim*vd)]     (laghos_solver.cpp:1160-1167)
 *   Jac0inv[i + dim*(j + dim*(e*NQ+q))]              (laghos_solver.cpp:1195)
 *   rho0DetJ0w[e*NQ+q];  mass_D = w*detJ0*rho0(x_q)  (laghos_assembly.cpp:92-95)
 * Writes: lgh_mass_D() and lgh_qdata_stressJinvT() honour them (see below). Jac0inv is a result: in 2D/3D the update reads its own
 * plane-major and per-zone copies (1D reads the array itself); rho0DetJ0w IS read by the update, the energies and the diagnostics,
 * but the mass data and the diagonal are not derived from it again. */
double *lgh_qdata_stressJinvT(lgh_ctx *ctx);
double *lgh_qdata_Jac0inv(lgh_ctx *ctx);
double *lgh_qdata_rho0DetJ0w(lgh_ctx *ctx);
double *lgh_mass_D(lgh_ctx *ctx);
/* Form of the mass quadrature data the plane / slab mass kernels read: 1 = compact, D[q, e] = W[q] s_e (the data of
 * laghos_assembly.cpp:92-95 whenever rho0 detJ0 is constant within each element - every benchmark mesh of
 * BASELINE.json; the kernels then read one double per element instead of NQ), 0 = the stored table.  The test is made
 * on the device (every entry to 1e-12 relative, the size of the rounding of the stored entries; LGH_MASS_RANK1_TOL) at the first mass apply after lgh_setup_rho0detj0() or after lgh_mass_D() was
 * called: a caller that writes through the lgh_mass_D() pointer calls lgh_mass_D() again after its last write. */
int lgh_mass_data_form(lgh_ctx *ctx, int *form);
/* Form of qdata.Jac0inv (laghos_solver.cpp:1195) the row-form quadrature update reads: *compact = 1: one inverse Jacobian per
 * zone - lgh_setup_rho0detj0 found Jac0inv the same at every point of every zone (each entry against the zone's first point,
 * to 1e-12 of the zone's largest entry; LGH_JAC0_TOL), which is what an affine initial zone has - nine doubles per zone
 * instead of nine per quadrature point (15.5 of the 20.5 KB the update streams per zone at Q3Q2); 0: the point values
 * (a curved initial mesh; LGH_JAC0_COMPACT=0).  The arrays of lgh_qdata_Jac0inv() are written in full either way. */
int lgh_jac0inv_form(lgh_ctx *ctx, int *compact);
/* A caller that keeps the lgh_mass_D() pointer and writes the table after a mass apply has run says so with this call
 * (calling lgh_mass_D() again does the first half too): the compact form is tested for again at the next apply,
 * and the Jacobi diagonal (lgh_mass_diag, OperatorJacobiSmoother of laghos_solver.cpp:266-270) is reassembled from the
 * new table, so that the operator every kernel form applies and its preconditioner stay the same matrix. */
int lgh_mass_data_changed(lgh_ctx *ctx);
double *lgh_mass_diag(lgh_ctx *ctx); /* Jacobi diagonal of the scalar H1 mass (N) */
int lgh_set_h0(lgh_ctx *ctx, double h0);
int lgh_get_h0(lgh_ctx *ctx, double *h0);
/* qdata.dt_est: host-visible scalar; the get synchronises the stream. */
int lgh_set_dt_est(lgh_ctx *ctx, double dt_est);
int lgh_get_dt_est(lgh_ctx *ctx, double *dt_est);

/* Rho0DetJ0Vol (laghos_solver.cpp:1170-1261) + mass PA data + Jacobi diagonal
 * (OperatorJacobiSmoother, laghos_solver.cpp:266-270).  x0: H1 L-vector of the
 * initial nodes; rho0_l2: rho0 grid function (L2 dofs); rho0_q: the function rho0
 * at the NE*NQ physical quadrature points.  Synchronous; returns the local volume. */
int lgh_setup_rho0detj0(lgh_ctx *ctx, const double *x0, const double *rho0_l2,
                        const double *rho0_q, double *volume);

/* ---- ForcePAOperator (laghos_assembly.hpp:94-112) */
/* Mult (laghos_assembly.cpp:557-565): x L2 L-vector -> y H1 L-vector (dim*N). */
int lgh_force_mult(lgh_ctx *ctx, const double *x_l2, double *y_h1);
/* MultTranspose (laghos_assembly.cpp:965-973): v H1 L-vector -> y L2 L-vector. */
int lgh_force_mult_transpose(lgh_ctx *ctx, const double *v_h1, double *y_l2);

/* ---- MassPAOperator (laghos_assembly.hpp:115-131) */
/* SetEssentialTrueDofs(c_tdofs[comp]) (assembly.cpp:98-110); comp = -1 clears. */
int lgh_mass_set_essential_tdofs(lgh_ctx *ctx, int comp);
/* EliminateRHS (assembly.cpp:112-115): b[ess] = 0. */
int lgh_mass_eliminate_rhs(lgh_ctx *ctx, double *b);
/* Mult (assembly.cpp:117-121): y = M x, then y[ess] = 0.  space = LGH_SPACE_*. */
int lgh_mass_mult(lgh_ctx *ctx, int space, const double *x, double *y);
/* MultFull (assembly.hpp:127): no essential-row elimination. */
int lgh_mass_mult_full(lgh_ctx *ctx, int space, const double *x, double *y);

/* ---- CG solves configured at laghos_solver.cpp:264-284 (upstream CGSolver,
 * SURVEY §3.2).  space H1: Jacobi-preconditioned, iterative_mode (x = initial
 * guess), active essential list; space L2: plain CG, x overwritten.  Dot products
 * are wave-shuffle reductions, owner-masked and all-reduced over RCCL when a
 * communicator is attached.  Synchronous; *iters = GetNumIterations(). */
int lgh_cg_solve(lgh_ctx *ctx, int space, const double *b, double *x, double rel_tol,
                 int max_iter, int *iters);
/* 1D only (the FA energy solve, laghos_solver.cpp:203-215, :501-515): x = Me(z)^-1 b zone by zone (L2 vectors, device),
 * with the Cholesky factors of the zone mass matrices formed at lgh_setup_rho0detj0 and again at lgh_mass_data_changed.
 * Asynchronous.  LGH_ERR_UNSUPPORTED for dim 2/3 (they run the energy CG). */
int lgh_l2_mass_solve_local(lgh_ctx *ctx, const double *b, double *x);

/* ---- QUpdate::UpdateQuadratureData (laghos_solver.cpp:1354-1411): fused
 * E-restriction + reference-gradient + QKernel; updates stressJinvT and folds the
 * point-wise dt estimate into qdata.dt_est (device side, no host sync).
 * Work whose result the kernel can prove unused is not done (lgh_qupdate_discard below): dt candidates that cannot
 * lower the folded minimum, F.1 rows that the flush below eps^2 would zero.  Which wavefronts skip their candidates
 * depends on timing; the results - stressJinvT, F.1, F^T v, the folded estimate - do not, to the last bit. */
int lgh_qupdate(lgh_ctx *ctx, const double *S);
/* The viscosity branch of QUpdateBody (laghos_solver.cpp:1086-1134) eigen-decomposes sym(grad v) at every
 * point.  When all 64 points of a wavefront have |sym grad v|_max <= tiny_grad (units 1/time) the kernel takes
 * the decomposition's own result for a tensor without deviatoric part (mu = tr/3, direction e_x) instead:
 * identical for exact zeros; for values below the threshold the stress differs by < visc_coeff * tiny_grad.
 * Default 1e-30 (LGH_Q_TINY_GRAD overrides); 0 = exact zeros only; negative = always decompose. */
int lgh_qupdate_set_tiny_grad(lgh_ctx *ctx, double tiny_grad);
/* lgh_qupdate skips two pieces of work whose result it can PROVE unused before computing it; every output keeps every
 * bit (LGH_Q_DISCARD=0 switches both off, for A/B and tests; 2 / 3: only the first / the second):
 *   - the dt candidate of a wavefront (smallest singular value of J, three divisions).  Its only reader is a global
 *     minimum.  From det J and |J|_F the kernel bounds every candidate of the wavefront from below; where that bound lies
 *     above a value the minimum already holds - the row form keeps one hint word beside the estimate, which only ever
 *     receives deposited values - or the candidate is +inf, the candidates are not computed (contexts with viscosity);
 *   - the F.1 rows of a zone (row form).  |output| <= C_F max|stressJinvT w detJ| over the zone, C_F = 3 cG cB^2 from the
 *     absolute column sums of the basis tables; where 2 C_F max|..| < eps^2 every output would be flushed to +0.0
 *     (laghos_assembly.cpp:495-512), and +0.0 is written without the three contractions.
 * Which wavefronts skip their candidates depends on when they read the hint word, that is on timing; the folded
 * estimate, F.1, F^T v and stressJinvT do not.  mode: bit 0 the dt candidate, bit 1 the F.1 rows. */
int lgh_qupdate_discard(lgh_ctx *ctx, int *mode, double *C_F);
/* lgh_qupdate also forms the two force products of the state it is called for - F.1 as E-vector (3D) and
 * F^T v for the state's own velocity - from the stress values it has in registers; lgh_solve_velocity and
 * lgh_solve_energy use them instead of a pass over stressJinvT each.  When they are used (no address is ever
 * compared):
 *   - both products belong to the quadrature data as lgh_qupdate left it: lgh_reset_quadrature_data, a set-up
 *     call, lgh_set_fused_forces and handing out the mutable lgh_qdata_stressJinvT pointer all discard them;
 *   - F.1 only for the all-ones L2 function (one_l2 == NULL, or a vector that is checked on that call);
 *   - F^T v only for a v whose every element equals the velocity block lgh_qupdate saw (a copy is kept and
 *     compared on the device inside lgh_solve_energy; any other v runs ForceMultTranspose, as
 *     laghos_solver.cpp:473 does for whatever v it is given).
 * on = 0 switches the fusion off: the products then always come from the ForcePAOperator kernels (per-kernel
 * timing, A/B).  Default on. */
int lgh_set_fused_forces(lgh_ctx *ctx, int on);
/* QuadratureData.stressJinvT is the hand-over between UpdateQuadratureData and the two ForcePA products in the
 * reference (laghos_solver.cpp:1158-1167 -> laghos_assembly.cpp:307-308, :859-872).  With both products formed inside
 * lgh_qupdate the nine planes are written and never read in a PA run whose SolveEnergy is always given the state's own
 * velocity (RK1-4, RK6): 43 % of the update's memory traffic.  on = 0: lgh_qupdate keeps the stress in registers and
 * does not write stressJinvT (3D, force fusion on); every reader then refuses with LGH_ERR_ARG instead of using stale
 * data - lgh_force_mult, lgh_force_mult_transpose, lgh_solve_velocity for a vector other than one; a SolveEnergy for a
 * velocity other than the state's (RK2Avg) turns its right-hand side into NaN on the device and the next
 * lgh_get_dt_est returns LGH_ERR_ARG.  lgh_qdata_stressJinvT() still returns the array (for inspection), but planes
 * nobody wrote do not become current by asking for them.
 * Default on = 1 (the reference's behaviour); a change takes effect with the next lgh_qupdate. */
int lgh_qupdate_store_stress(lgh_ctx *ctx, int on);
int lgh_qupdate_stores_stress(lgh_ctx *ctx, int *on);
/* Kernel lgh_qupdate launches for this context: 1 = qrows_kernel (3D up to Q4Q3: contraction stages with row-owning
 * threads, lgh_qrows.hpp), 0 = qpoint_kernel (every thread owns one output of every stage; 2D, Q5Q4, LGH_Q_FORM=0). */
int lgh_qupdate_form(lgh_ctx *ctx, int *form); /* whether the next lgh_qupdate writes stressJinvT (bench.py's byte accounting) */
/* ResetQuadratureData (laghos_solver.hpp: qdata_is_current = false): the state has changed, the quadrature data -
 * and the force products formed with it - are stale.  The shells call it wherever the reference does. */
int lgh_reset_quadrature_data(lgh_ctx *ctx);
/* The two fused products as vectors, for callers (and tests) that want ForcePA->Mult(one) / MultTranspose(v_state)
 * of the current quadrature data without another pass over it: F.1 summed to the H1 L-vector (dim*N), F^T v as
 * L2 vector.  LGH_ERR_ARG when the product is not on hand. */
int lgh_fused_force_mult(lgh_ctx *ctx, double *y_h1);
int lgh_fused_force_mult_transpose(lgh_ctx *ctx, double *y_l2);
/* F.1 as lgh_qupdate left it, before the sum over shared nodes: the E-vector [ND][dim][NE] (tests compare its bits). */
int lgh_fused_force_e(lgh_ctx *ctx, double *y_e);
/* *gen counts lgh_qupdate calls and invalidations; *f1_valid / *ftv_valid: a fused F.1 / F^T v is on hand (tests). */
int lgh_quadrature_generation(lgh_ctx *ctx, unsigned long *gen, int *f1_valid, int *ftv_valid);
/* *f1 / *ftv = 1 when lgh_qupdate forms F.1 / F^T v (what the region timers then see: the "Forces" region of
 * lgh_get_timers only holds the E->L sum and right-hand-side set-up, the products are inside "UpdateQuadData") */
int lgh_get_fused_forces(lgh_ctx *ctx, int *f1, int *ftv);

/* ---- LagrangianHydroOperator pieces kept together for launch efficiency
 * (laghos_solver.cpp:329-399, :442-490).  dS_dt = [dx|dv|de]; one_l2 is the
 * constant-one L2 vector (laghos_solver.cpp:170-171) or NULL for the operator's own (the reference's
 * SolveVelocity takes none: it is a member); rhs_h1 / e_rhs / work are
 * caller scratch (dim*N, L2 size, N).  e_source may be NULL.
 * *h1_iters / *l2_iters accumulate CG iteration counts (timer.H1iter, L2iter). */
int lgh_solve_velocity(lgh_ctx *ctx, const double *S, double *dS_dt, const double *one_l2,
                       double *rhs_h1, double *work_B, double rel_tol, int max_iter,
                       int *h1_iters);
int lgh_solve_energy(lgh_ctx *ctx, const double *S, const double *v_h1, double *dS_dt,
                     double *e_rhs, const double *e_source, double rel_tol, int max_iter,
                     int *l2_iters);
/* The same SolveEnergy split in two so that LagrangianHydroOperator::Mult
 * (laghos_solver.cpp:308-326) can overlap it with SolveVelocity, which it does not
 * depend on: _begin enqueues F^T v and the L2 CG on a second stream, _end completes
 * the solve and joins the context stream.  Call order: _begin, lgh_solve_velocity,
 * _end; all pointers must stay valid until _end returns.  The pair is equivalent to
 * one lgh_solve_energy call (identical iterates) and degrades to it when overlap is
 * not possible (timers on, several ranks, 2D). */
int lgh_solve_energy_begin(lgh_ctx *ctx, const double *S, const double *v_h1, double *dS_dt,
                           double *e_rhs, const double *e_source, double rel_tol, int max_iter);
int lgh_solve_energy_end(lgh_ctx *ctx, int *l2_iters);
/* Several ranks on ONE communicator (no second channel: the default over RCCL): _begin sets the energy CG up on the main stream
 * and lgh_solve_velocity enqueues one of its iterations behind each of its own - the mass apply behind K1, the update behind K2 -
 * with (d, M d) as a fourth scalar on the halo messages and (r, r) in a spare word of the accumulator-word exchange: the energy
 * solve costs no exchange and no host look of its own, as SolveEnergy costs none beside SolveVelocity on one rank.  _end runs
 * what is left (an energy solve that needs more iterations than the velocity solve took).  The iterates are those of
 * lgh_solve_energy up to the order in which the ranks' (r, r) and (d, M d) are added (rank order instead of RCCL's).
 * LGH_ENERGY_LOCKSTEP=0: the energy solve after the velocity solve.  Needs what the velocity solve's word exchange needs (every
 * rank a neighbour of every other, the slab form of K1) and region timers off.
 *   out[0] = energy solves run this way, out[1] = their iterations enqueued inside velocity solves, out[2] = ... after them,
 *   out[3] = 1: the next lgh_solve_energy_begin would take this path.
 * Replaces nothing in the reference (laghos_solver.cpp:400-493 runs the two solves one after the other). */
int lgh_energy_lockstep_stats(lgh_ctx *ctx, long out[4]);

/* ---- vector helpers on the context stream (device pointers) */
int lgh_vec_set(lgh_ctx *ctx, double *y, double a, long n);              /* y = a */
int lgh_vec_copy(lgh_ctx *ctx, double *y, const double *x, long n);      /* y = x */
/* z1 = a1 x1 + b1 y and z2 = a2 x2 + b2 y in one pass over y: the two combinations an explicit RK stage forms from the same
 * increment k (upstream RK4Solver::Step: the next stage state and the running sum of the solution).  The same expressions
 * as lgh_vec_axpby - the same bits as two calls.  z1 may be x1 and z2 may be x2 (the very same vector); any other overlap
 * between a result and an operand of the OTHER combination (z1 with z2, x2 or y; z2 with x1 or y) is refused with
 * LGH_ERR_ARG: two sequential calls would see the first result, the fused pass would not. */
int lgh_vec_axpby_pair(lgh_ctx *ctx, double *z1, double a1, const double *x1, double b1, double *z2, double a2, const double *x2, double b2,
                       const double *y, long n);
int lgh_vec_axpby(lgh_ctx *ctx, double *z, double a, const double *x, double b,
                  const double *y, long n);                                /* z = a x + b y */
int lgh_vec_dot(lgh_ctx *ctx, const double *x, const double *y, long n, double *result); /* sync */
/* The state fingerprint of include/lgh_fingerprint.h over the n doubles at x (device), taken as their bit patterns at
 * positions offset .. offset + n - 1: out[0] = sum, out[1] = xor of the mixed words (mod 2^64).  Integer arithmetic only:
 * the two words do not depend on the launch shape, and the fingerprint of a concatenation is the word-wise combination
 * (add, xor) of the fingerprints of its parts at their offsets.  Synchronous, like lgh_vec_dot.  Reads x, writes nothing of
 * the caller's: the quadrature data, its generation counter and the fused force products are untouched.  All dimensions.
 * n == 0 gives {0, 0} without a launch; n < 0, or x == NULL with n > 0: LGH_ERR_ARG.  x may be any 8-byte aligned address
 * (a slice that starts at an odd element is read with a scalar head). */
int lgh_vec_fingerprint(lgh_ctx *ctx, const double *x, long n, unsigned long long offset, unsigned long long out[2]);
/* The launch lgh_vec_fingerprint makes for (x, n), for tests that want sizes beyond one pass of the grid: out[0] = workgroups
 * (0: no launch), out[1] = threads of a workgroup, out[2] = 1 when a scalar head is taken (x not 16-byte aligned), out[3] =
 * words one pass of the largest grid takes. */
int lgh_vec_fingerprint_shape(lgh_ctx *ctx, const double *x, long n, long out[4]);
/* The same function over n 64-bit words in HOST memory (no GPU, no context): what the checkpoint code computes. */
int lgh_fingerprint_host(const void *words, long n, unsigned long long offset, unsigned long long out[2]);

/* ---- energies (laghos_solver.cpp:640-697); synchronous, all-reduced */
/* Acceleration source of SolveVelocity (source_type == 2, problem 7; laghos_solver.cpp:340-347,
 * :371-380): accel_h1 = nodal projection of RTCoefficient on the H1 space (dim*N, byNODES, device;
 * must stay valid), NULL switches it off.  lgh_solve_velocity then adds VMassPA->MultFull(accel_c)
 * to the right-hand side of every component before EliminateRHS. */
int lgh_set_velocity_source(lgh_ctx *ctx, const double *accel_h1);

/* 2D Taylor-Green energy source (SolveEnergy's source_type == 1 branch,
 * laghos_solver.cpp:448-467 with TaylorCoefficient laghos_solver.hpp:208-218):
 * e_source (L2 size, device) = DomainLFIntegrator(TaylorCoefficient) assembled on the
 * mesh positions in S; pass it to lgh_solve_energy(_begin). */
int lgh_tg_source_2d(lgh_ctx *ctx, const double *S, double *e_source);

int lgh_internal_energy(lgh_ctx *ctx, const double *e_l2, double *result);
int lgh_kinetic_energy(lgh_ctx *ctx, const double *v_h1, double *result);

/* ---- `-err`: density against the exact Sedov blast wave (laghos.cpp:1007-1086) ---------
 * Replaces the host-side SedovSol class (sedov/sedov_sol.hpp:21-76, sedov_sol.cpp),
 * LagrangianHydroOperator::ComputeDensity (laghos_solver.cpp:542-563) and the error loop
 * of the driver.  The solution's parameter block `par` is 21 host doubles:
 *   dim gamma rho0 E omega | a b c d e | alpha0..alpha5 | V0 Vv V2 Vs | alpha
 * (the members of SedovSol, sedov_sol.hpp:24-55). */
/* SedovSol::SedovSol (sedov_sol.cpp:27-117): constants and the energy integral alpha
 * (adaptive 21-point Gauss-Kronrod, host).  omega must be 0 (uniform initial density). */
int lgh_sedov_setup(int dim, double gamma, double rho0, double blast_energy, double omega, double par[21]);
/* SedovSol::SetTime (sedov_sol.cpp:119-130): shock[6] = r2 U rho1 rho2 v2 p2 at time t. */
int lgh_sedov_shock(const double par[21], double t, double shock[6]);
/* SedovSol::EvalSol (sedov_sol.cpp:132-198) at one radius, on the host (scalar API of the class). */
int lgh_sedov_eval_point(const double par[21], double t, double r, double *rho, double *v, double *P);
/* The same for n radii on the GPU: r, rho, v, P are device arrays; asynchronous on the context's stream. */
int lgh_sedov_eval(lgh_ctx *ctx, const double par[21], double t, long n, const double *r, double *rho, double *v,
                   double *P);
/* ComputeDensity (laghos_solver.cpp:542-563): zone-local L2 projection of the density on the
 * mesh positions x_h1 (= S, device) into rho_l2 (L2 size, device).  Needs lgh_setup_rho0detj0. */
int lgh_compute_density(lgh_ctx *ctx, const double *x_h1, double *rho_l2);
/* laghos.cpp:1027-1080: err2 = integral over the current mesh of (rho_exact(|x - origin|, t) - rho_h)^2
 * with the n1d^dim tensor Gauss-Legendre rule given by HOST tables on [0,1]: weights[n1d],
 * B_h1/G_h1 [p + n1d*d] (H1 basis values / derivatives), B_l2 [p + n1d*l] (L2 basis).
 * Summed over the ranks; synchronous. */
int lgh_sedov_density_error(lgh_ctx *ctx, const double *x_h1, const double *rho_l2, const double par[21], double t,
                            const double origin[3], int n1d, const double *weights, const double *B_h1,
                            const double *G_h1, const double *B_l2, double *err2);

/* ---- visualisation sampling (stands in for VisItDataCollection::Save, laghos.cpp:691-701, :845-871; the driver's
 * `-paraview` dumps): x, v, e, the density rho_l2 (lgh_compute_density; may be NULL) and the pressure of the equation of
 * state of QUpdateBody (laghos_solver.cpp:1069-1168), p = (gamma_z - 1) rho max(e, 0), on a lattice of R1 = R + 1 points
 * per direction in every zone (2 <= R1 <= 9).  With NP = NE * R1^dim the point index is pt = e * R1^dim + (rx + R1 * (ry +
 * R1 * rz)), e the CALLER's zone index (the one h1_map uses).  Outputs are device arrays, structure of arrays:
 * x_out[c * NP + pt], v_out[c * NP + pt] (c < dim), e_out[pt], rho_out[pt], p_out[pt]; each may be NULL and is then
 * skipped (the others keep their bits).  B_h1_lat [r + R1 * d] / B_l2_lat [r + R1 * l] are HOST tables of the 1-D H1 / L2
 * bases at the lattice abscissae r / R - lgh_config.B_h1 / B_l2 with Q1D -> R1; they are read during the call, nothing is
 * kept of them.  rho_out or p_out without rho_l2, or an R1 out of range: LGH_ERR_ARG; a lattice table of more than 81 entries
 * (R1 * D1D) or a zone that needs more than 64 KB of LDS (D1D = 9 on R1 = 9 points in 3D): LGH_ERR_UNSUPPORTED.  No kernel is
 * launched in either case.
 * Asynchronous on the context's stream; reads S, rho_l2 and the context's constant data, writes its outputs only: the
 * quadrature data, its generation counter and the fused force products are untouched.  All dimensions (1D included). */
int lgh_sample_fields(lgh_ctx *ctx, const double *S, const double *rho_l2 /* or NULL */,
                      int R1, const double *B_h1_lat /* host, R1*D1D, [r + R1*d] */,
                      const double *B_l2_lat /* host, R1*L1D, [r + R1*l] */,
                      double *x_out, double *v_out, double *e_out, double *rho_out, double *p_out);

/* ---- derived flow fields on the same lattice (the driver's `-paraview -pv-fields`): what needs derivatives of the Q_k fields
 * inside a zone and cannot be recovered from a file of linear cells.  Lattice, point index pt, NP and the table layout are
 * those of lgh_sample_fields; G_h1_lat[r + R1 * d] is the derivative of the H1 Gauss-Lobatto basis function d at r / (R1 - 1)
 * (lgh_config.G_h1 with Q1D -> R1).  Per lattice point, with J_ij = dx_i / dxi_j and V_ij = dv_i / dxi_j from the H1 dofs of
 * the zone:
 *   detj_out[pt]                    det J
 *   gradv_out[(i*dim + j)*NP + pt]  L_ij = dv_i / dx_j = (V adj(J))_ij / det J  (sgrad_v of QUpdateBody before Symmetrize,
 *                                   laghos_solver.cpp: Mult(dV, Jinv)); no branch on the sign of det J: an inverted point has
 *                                   the value of the formula, det J == 0 what IEEE gives
 *   div_out[pt]                     L_00 (+ L_11 (+ L_22)), summed in this order from the entries stored
 *   vort_out                        2D: NP values L_10 - L_01; 3D: 3 NP values (L_21 - L_12, L_02 - L_20, L_10 - L_01),
 *                                   component-major as v_out; 1D: LGH_ERR_ARG when not NULL
 *   cs_out[pt]                      sqrt((gamma_z (gamma_z - 1)) max(e, 0)), the sound speed of QUpdateBody, e the value
 *                                   lgh_sample_fields gives at the point (the same bits)
 * Each output is a device array, may be NULL and is then skipped; the others keep their bits.  Refusals as lgh_sample_fields:
 * R1 out of range, a NULL table, vort_out in 1D: LGH_ERR_ARG; tables of more than 81 entries or a zone that needs more than
 * 64 KB of LDS: LGH_ERR_UNSUPPORTED with the bytes in the message.  No kernel is launched in either case.
 * Asynchronous on the context's stream; reads S and the context's constant data (h1_map, gamma), writes its outputs only: the
 * quadrature data, its generation counter and the fused force products are untouched.  All dimensions. */
int lgh_sample_derived(lgh_ctx *ctx, const double *S, int R1, const double *B_h1_lat /* host, R1*D1D, [r + R1*d] */,
                       const double *G_h1_lat /* host, R1*D1D */, const double *B_l2_lat /* host, R1*L1D */,
                       double *detj_out, double *gradv_out, double *div_out, double *vort_out, double *cs_out);

/* ---- the same fields on zone faces (outer surface, logical cut planes): a face is (zone e, local face f = 2a + s), the side
 * xi_a = s of the caller's zone e, a < dim, s = 0 or 1.  Its lattice is the volume lattice above with one abscissa on axis a:
 * NPF = R1^(dim-1) points over the other axes in ascending order, p = r_b + R1 r_c (3D, b < c), p = r_b (2D).  For the list
 * faces[2k] = e, faces[2k + 1] = f of nfaces faces (a HOST array, read during the call like the tables; a zone may appear any
 * number of times, in any order; the device copy lives in a buffer of the context), NPt = nfaces * NPF and pt = k * NPF + p.
 * Outputs are device arrays, structure of arrays over NPt with NP -> NPt in the layouts above; each may be NULL and is skipped:
 *   x_out, v_out, e_out, rho_out, p_out              as lgh_sample_fields
 *   detj_out, gradv_out, div_out, vort_out, cs_out   as lgh_sample_derived
 *   an_out[c * NPt + pt], c < dim                    the outward area vector per unit reference area (Nanson's formula):
 *                                                    N_i = sgn adj(J)_{a i}, J adj(J) = det J I, sgn = +1 for s = 1, -1 for s = 0;
 *                                                    2D: a length-weighted normal.  No branch looks at the sign of det J.
 * For every finite state each output but an_out has THE BITS the volume functions give at the lattice point with r_a = 0
 * (s = 0) or R1 - 1 (s = 1) and the other indices equal: the same stages in the same order, one table row on axis a.
 * LGH_ERR_ARG: dim == 1, R1 out of range, nfaces < 0, a NULL table an output needs (B_h1_lat: x, v and the derivatives; G_h1_lat:
 * detj, gradv, div, vort, an; B_l2_lat: e, rho, p, cs), rho_out / p_out without rho_l2, a zone outside 0..NE-1, a local face
 * outside 0..2 dim - 1.  LGH_ERR_UNSUPPORTED with the bytes in the message: tables of more than 81 entries, a face that needs
 * more than 64 KB of LDS.  The message names the offending value; nothing is launched.  nfaces == 0, or no output: LGH_OK, no launch.
 * Asynchronous on the context's stream; reads S, rho_l2, h1_map, gamma; writes its outputs only.  2D and 3D. */
int lgh_sample_faces(lgh_ctx *ctx, const double *S, const double *rho_l2 /* or NULL */, int R1,
                     const double *B_h1_lat /* host, R1*D1D, or NULL */, const double *G_h1_lat /* host, R1*D1D, or NULL */,
                     const double *B_l2_lat /* host, R1*L1D, or NULL */, int nfaces, const int *faces /* host, 2*nfaces */,
                     double *x_out, double *v_out, double *e_out, double *rho_out, double *p_out, double *detj_out,
                     double *gradv_out, double *div_out, double *vort_out, double *cs_out, double *an_out);
/* Faces per workgroup of that kernel for lists long enough: as many as fit 256 lattice points and 48 KB of LDS, one where they
 * do not - min(256 / NPF, (48 KB - tables) / face), with (R1 + 2) (2 D1D + L1D) doubles of tables and per face
 * 1 + max(D^dim + 2 R1 D^(dim-1) [+ 3 R1^2 D in 3D], L^dim + R1 L^(dim-1) [+ R1^2 L in 3D]) doubles.  Lists of FPB - 1, FPB, FPB + 1
 * faces are the edges of the launch.  LGH_ERR_ARG where lgh_sample_faces refuses dim or R1. */
int lgh_sample_faces_fpb(lgh_ctx *ctx, int R1, int *fpb);
/* The boundary of a mesh given by its element -> node map alone (no GPU, no context; for callers that hand over a mesh
 * library's numbering): the faces (e, f) whose D1D^(dim-1) nodes are, as a set, the nodes of no other face of any zone, in
 * ascending (e, f), into faces_out[2k], faces_out[2k + 1] (room for 2 * 2 dim NE ints); *nfaces their number.  dim 1..3. */
int lgh_mesh_boundary_faces_host(int dim, int NE, int N, int D1D, const int *h1_map, int *faces_out, int *nfaces);

/* ---- conservation and mesh-health diagnostics (the driver's `-hist` time history; the reference prints one number,
 * "Energy diff", after the last step).  At quadrature point q of zone z, with the context's own tables and rule (those
 * lgh_qupdate uses): J_q = grad x and detJ_q from the x block of S, v_q from the v block, e_q from the e block through
 * B_l2, m_q = rho0DetJ0w[z, q], rho_q = (1 / w_q) m_q / detJ_q, p_q = (gamma_z - 1) rho_q max(e_q, 0) - the expressions
 * of QUpdateBody (laghos_solver.cpp:1074-1083).  A point is NON-FINITE when detJ_q, e_q or a component of v_q is not
 * finite, INVERTED when detJ_q <= 0.  Slot k, per zone and globally:
 *    0 mass = sum m_q            1 volume = sum w_q detJ_q      2 internal energy = sum m_q e_q (laghos_solver.cpp:640-667)
 *    3 kinetic energy = 1/2 sum m_q |v_q|^2 (:669-697)          4-6 momentum = sum m_q v_c(q), 0 for c >= dim
 *    7 detj_min (finite points)  8, 9 rho_min, rho_max (finite, not inverted)   10, 11 e_min, e_max (finite points)
 *   12 p_max (finite, not inverted)   13 v_max = max |v_q| (finite points)
 *   14 n_inverted   15 n_negative_e (e_q < 0)   16 n_nonfinite   (counts, as doubles)
 * Sums run over all points (a NaN in the state makes them NaN); extremes skip the excluded points, and with no point
 * left a minimum is +inf and a maximum -inf.  The global array adds 17 = the zone that holds detj_min (the CALLER's id on
 * its rank, ties to the lowest id), 18 = that zone's rank (ties to the lowest rank), 19 = 0.
 * No floating-point atomics: a zone's points are folded in a fixed shape inside its workgroup, the zones in ascending
 * caller id by one workgroup of fixed shape; the same S and context give the same bits whatever the launch grid.  Over
 * several ranks sums go through the all-reduce, minima through the min-reduce, maxima as negated minima.
 * Both calls read S, rho0DetJ0w, gamma, the tables and h1_map and write their outputs only: the quadrature data, its
 * generation counter, the fused force products, dt_est and the velocity snapshot are untouched.  All dimensions.
 * Before lgh_setup_rho0detj0, or with a NULL argument: LGH_ERR_ARG, no kernel is launched. */
#define LGH_DIAG_ZONE_COUNT 17
#define LGH_DIAG_COUNT 20
/* per zone, structure of arrays: zone_out[k * NE + z], z the CALLER's zone id; device; asynchronous */
int lgh_diagnostics_zones(lgh_ctx *ctx, const double *S, double *zone_out);
/* the same folded over zones and ranks; out is HOST memory; synchronous */
int lgh_diagnostics(lgh_ctx *ctx, const double *S, double out[LGH_DIAG_COUNT]);

/* ---- binned 1-D profiles of the flow (the driver's `-prof`): the point quantities of lgh_diagnostics above, and the
 * position x_q = x_first + sum B (x - x_first), reduced into nbins uniform bins of a coordinate xi_q: x_q[axis], or the
 * distance r_q = |x_q - origin| (axis 3).  n_q is the unit axis vector, or (x_q - origin) / r_q (v.n = 0 where r_q = 0).
 * Bin index b = floor((xi_q - lo) * inv_w), inv_w = nbins / (hi - lo) formed once on the host; b < 0 goes to row 0,
 * b >= nbins to row nbins + 1, else to row 1 + b.  A point that is NON-FINITE (detJ_q, e_q, a component of v_q or xi_q) or
 * INVERTED (detJ_q <= 0) enters no row and is counted in n_excluded (summed over the ranks).  Columns of a row:
 *    0 n (points, exact)   1 vol = sum w_q detJ_q   2 mass = sum m_q   3 ie = sum m_q e_q   4 ke = 1/2 sum m_q |v_q|^2
 *    5 mom = sum m_q (v_q . n_q)   6 pv = sum w_q detJ_q p_q   7 mxi = sum m_q xi_q
 *    8 rho_min, 9 rho_max over the row's points (+inf / -inf for an empty row; m_q > 0 is assumed)
 * Columns 1-7 go through the exact integer accumulators of the velocity solve (lgh_vcg.hpp), counts and extremes through
 * integer atomics: no floating-point atomic, and the same bits for every zone order, node numbering, launch grid and rank
 * count.  An addend that is not finite (an overflowed product of finite factors) turns its (row, column) into NaN.
 * out: HOST, (nbins + 2) rows of LGH_PROFILE_COLS doubles, row-major.  Synchronous; collective over the ranks of the context.
 * Reads S, rho0DetJ0w, gamma, the tables and the maps and writes its outputs only (as lgh_diagnostics).  All dimensions.
 * LGH_ERR_ARG without a launch: before lgh_setup_rho0detj0, a NULL argument, axis outside 0..3 or an axis >= dim, nbins
 * outside 1..LGH_PROFILE_MAX_BINS, lo, hi or hi - lo not finite, lo >= hi, a non-finite origin component < dim for axis 3.
 * LGH_PROFILE_FOLD=n (default 8): wavefronts whose points span more than n rows send one atomic per lane and limb instead
 * of folding their lanes row by row first (0: always); the result has the same bits either way. */
#define LGH_PROFILE_COLS 10
#define LGH_PROFILE_MAX_BINS 4096
typedef struct lgh_profile_spec {
   int axis;          /* 0, 1, 2: the coordinate x, y, z (must be < dim); 3: r = |x_q - origin| */
   int nbins;         /* 1 .. LGH_PROFILE_MAX_BINS */
   double lo, hi;     /* finite, lo < hi; bin b covers [lo + b w, lo + (b+1) w), w = (hi - lo) / nbins */
   double origin[3];  /* used by axis 3 only; components >= dim ignored */
} lgh_profile_spec;
int lgh_profile(lgh_ctx *ctx, const double *S, const lgh_profile_spec *spec, double *out, long *n_excluded);

/* ---- the flow binned onto a fixed Cartesian grid (the driver's `-map`): the point quantities of lgh_profile above - x_q,
 * v_q, e_q, detJ_q, m_q, rho_q, p_q, NON-FINITE and INVERTED as there; a component of x_q below dim that is not finite also
 * makes the point non-finite - deposited into the cells of a box that stays where it is while the mesh moves.  lgh_profile
 * is the one-axis case.  Per axis c < dim: b_c = floor((x_q[c] - lo_c) * inv_w_c), inv_w_c = n_c / (hi_c - lo_c) formed once
 * on the host.  A point with some b_c < 0 or b_c >= n_c goes to row 0 ("outside"), every other one to row
 * 1 + b_0 + n_0 (b_1 + n_1 b_2).  Excluded points enter no row and are counted in *n_excluded (summed over the ranks).
 * Columns of a row: 0 n | 1 vol = sum w detJ | 2 mass = sum m | 3 ie = sum m e | 4 ke = 1/2 sum m |v|^2 |
 *   5-7 mom_c = sum m v_c (exactly +0.0 for c >= dim) | 8 pv = sum w detJ p | 9 rho_min | 10 rho_max (+inf / -inf: empty row).
 * Columns 1-8 go through the two-set exact accumulators of lgh_profile (pass 0 for the column maxima and the windows, hi / lo
 * limbs, non-returning 64-bit integer atomics, the NaN flag per (row, column) for an addend that is not finite), counts and
 * extremes through integer atomics: no floating-point atomic, and the same bits for every zone order, node numbering, launch
 * grid and rank count.  The rows add up to the totals of lgh_diagnostics less the excluded points.
 * out: HOST, (ncells + 1) rows of LGH_MAP_COLS doubles, row-major, ncells = n[0] n[1] n[2].  Synchronous; collective over the
 * ranks of the context.  Reads what lgh_profile reads and writes its outputs only.  All dimensions.
 * LGH_ERR_ARG without a launch: before lgh_setup_rho0detj0, a NULL argument, n[c] < 1, n[c] != 1 for c >= dim, ncells above
 * LGH_MAP_MAX_CELLS, and on an axis below dim lo, hi or hi - lo not finite or lo >= hi.  The scratch memory (about 1.4 KB per
 * cell) is allocated at the first call and regrown only when the cell count grows; when it cannot be had the call returns
 * LGH_ERR_HIP with the byte count in the message and the context stays usable.
 * LGH_MAP_FOLD=n (default 8, at most 64): a wavefront folds the lanes of up to n distinct cells before it sends one atomic
 * per non-zero limb of a cell; the lanes left after that send their own (0: always); the same bits either way. */
#define LGH_MAP_COLS 11
#define LGH_MAP_MAX_CELLS (1 << 20)
typedef struct lgh_map_spec {
   int n[3];               /* cells per axis, >= 1; n[c] must be 1 for c >= dim */
   double lo[3], hi[3];    /* finite, lo < hi, for c < dim; ignored above */
} lgh_map_spec;
int lgh_map(lgh_ctx *ctx, const double *S, const lgh_map_spec *spec,
            double *out /* HOST, (ncells + 1) x LGH_MAP_COLS, row-major */, long *n_excluded);

/* ---- pressure loads on lists of zone faces (the driver's `-loads`): the integral of p n dA over walls and logical planes of
 * the mesh, with the area, the power and the swept volume beside it.  A face is (zone e, local face f = 2a + s) as in
 * lgh_sample_faces, e the CALLER's zone id; faces[3k], faces[3k+1], faces[3k+2] = e, f and the row the face is summed into.
 * A face may be listed any number of times, in any order, under any row in 0..nrows-1.  Its points are the tensor Gauss
 * points of the context's own 1-D rule on the dim - 1 tangential axes (ascending, the lower axis fastest), w the product of
 * the 1-D weights.  At a point: x, v the H1 traces; N the outward area vector per unit reference area (the an_out of
 * lgh_sample_faces: Nanson, sign + for s = 1 and - for s = 0, no branch on a determinant); e, rho the traces of the e block
 * of S and of rho_l2 (the density lgh_compute_density projects) IN ZONE e - the thermodynamic fields are discontinuous, the
 * zone a face is listed under is part of the definition; p = (gamma_e - 1) rho max(e, 0).  Both 1-D bases interpolate at the
 * end points, so every trace is a contraction of the face layer of dofs alone.  Columns of a row:
 *    0 n (points, exact)   1 area = sum w |N|   2-4 force_c = sum w p N_c (exactly +0.0 for c >= dim)   5 pa = sum w p |N|
 *    6 power = sum w p (v.N)   7 flux = sum w (v.N)   8 xn = sum w (x.N) (dim x the enclosed volume over a closed surface)
 *    9 p_min, 10 p_max over the row's points, right for negative and zero p (+inf / -inf for an empty row)
 * A point where a component of x, v or N below dim, or e or rho, is not finite enters no row and is counted in *n_excluded
 * (summed over the ranks).  Columns 1-8 go through the two-set exact accumulators of lgh_profile / lgh_map, counts and
 * extremes through integer atomics: no floating-point atomic, and the same bits for every face order, numbering, launch
 * grid and rank count.  An addend that overflows from finite factors turns its own (row, column) into NaN.
 * out: HOST, nrows rows of LGH_LOADS_COLS doubles, row-major.  Synchronous; collective over the ranks of the context (a rank
 * with nfaces == 0 takes part).  Reads S, rho_l2, h1_map, gamma and the tables and writes its outputs only.  2D and 3D.
 * LGH_ERR_ARG without a launch, the value in the message: dim == 1, a NULL argument, nrows outside 1..LGH_LOADS_MAX_ROWS,
 * nfaces < 0, a zone, local face or row out of range.  LGH_ERR_UNSUPPORTED: a rule that is no tensor product, a face that
 * does not fit 64 KB of LDS (the bytes in the message). */
#define LGH_LOADS_COLS 11
#define LGH_LOADS_MAX_ROWS 64
int lgh_loads(lgh_ctx *ctx, const double *S, const double *rho_l2, int nrows,
              int nfaces, const int *faces /* HOST, 3*nfaces: zone e, local face f = 2a+s, row */,
              double *out /* HOST, nrows x LGH_LOADS_COLS, row-major */, long *n_excluded);
/* Faces per workgroup of that kernel for lists long enough (lists of FPB - 1, FPB, FPB + 1 faces are the edges of the launch):
 * as many as fit 256 points and 48 KB of LDS.  Refuses what lgh_loads refuses of a context. */
int lgh_loads_fpb(lgh_ctx *ctx, int *fpb);

/* ---- contours of a lattice scalar: iso-surfaces, and cut planes that are no zone faces (the plane n.x = d is the contour of the
 * lattice scalar n.x at d).  Marching tetrahedra (3D) / marching triangles (2D) over the volume lattice of lgh_sample_fields;
 * nothing is located in the moving mesh.  2D and 3D.
 * INPUT  scalar[NP], a device array on that lattice: R1 points per direction, 2 <= R1 <= 9, NP = NE * R1^dim,
 *   pt = e * R1^dim + rx + R1 * (ry + R1 * rz), e the CALLER's zone index; and a value iso.
 * INSIDE  a lattice point is inside when scalar[pt] >= iso (a NaN is outside; see SKIPPED).
 * SIMPLICES  a sub-cell is the lattice cell with lower corner (rx, ry, rz), r* < R1 - 1, index rx + (R1-1) * (ry + (R1-1) * rz).
 *   3D: six tetrahedra, the Kuhn split along the diagonal 000-111: tetrahedron k is the path 000 -> e_a -> e_a + e_b -> 111 of
 *   the k-th permutation (a, b, c) of the axes in lexicographic order (012, 021, 102, 120, 201, 210).  2D: two triangles,
 *   k = 0: (00, 10, 11), k = 1: (00, 01, 11) - the paths of (x, y) and (y, x).  Corners are numbered 0..dim along the path; their
 *   lattice indices ascend with it.  The split is translation invariant: neighbouring sub-cells of a zone share diagonals.
 * VERTEX  on a lattice edge (p0, p1) of a simplex whose ends differ in side, always stored with p0 < p1 as lattice indices, with
 *   the weight t = (iso - scalar[p0]) / (scalar[p1] - scalar[p0]) in this form in IEEE double: simplices that share an edge
 *   produce the same (p0, p1, t) to the bit.  A vertex is named by the corners of its edge below: "ab" is the edge of corners a, b.
 * PRIMITIVES of a simplex (triangles in 3D, segments in 2D; `<` is the path order):
 *   one corner a inside, o1 < o2 (< o3) outside:      (a o1, a o2 (, a o3))
 *   one corner o outside, i1 < i2 (< i3) inside:      (i1 o, i2 o (, i3 o))
 *   3D, a < b inside and c < d outside:               the quad (ac, ad, bd, bc) split along ac-bd: (ac, ad, bd), then (ac, bd, bc)
 *   ORIENTATION in reference (lattice) coordinates - 3D: the normal by the right-hand rule points from the inside corners to the
 *   outside ones; 2D: the inside lies to the left of the segment.  Where the order above has the other sense, the LAST TWO
 *   vertices of the primitive are swapped.  Primitives with coincident vertices (t = 0 or 1) are kept.
 * SKIPPED  a simplex with a corner value that is not finite produces nothing and is counted in *n_skipped: no NaN reaches an output.
 * ORDER  ascending (zone in the caller's order, sub-cell, simplex k, primitive as listed): the output is a function of the input
 *   alone, the same for every launch grid, and a second call gives the same bytes.  No atomic decides a position: a count pass,
 *   a scan of the workgroup totals, and an emit pass that recomputes the cases and writes at its offset.
 * OUTPUT per primitive q, device arrays: edges_out[2 dim q + 2 j], [.. + 1] = p0, p1 of vertex j < dim; t_out[dim q + j];
 *   zone_out[q] = e (may be NULL).  Points are not shared between primitives.
 * Synchronous in its counts: *n_prims is always the number the input produces.  If *n_prims > capacity NOTHING is written and
 * the call is still LGH_OK: the caller sizes the buffers and calls again; capacity == 0 with NULL outputs is the counting call.
 * The emit pass is asynchronous on the context's stream.  LGH_ERR_ARG without a launch, the value in the message: dim == 1, R1
 * out of range, scalar NULL, capacity < 0, capacity > 0 with edges_out or t_out NULL.  LGH_ERR_UNSUPPORTED: NP above 2^31 - 1.
 * Reads scalar; writes its outputs and a scratch buffer the context owns (three words per workgroup): the quadrature data,
 * its generation counter and the fused force products are untouched. */
int lgh_contour(lgh_ctx *ctx, int R1, const double *scalar, double iso, long capacity,
                int *edges_out /* 2 dim per primitive */, double *t_out /* dim per primitive */, int *zone_out /* or NULL */,
                long *n_prims, long *n_skipped);
/* Any lattice array at the vertices: out[c * n_verts + k] = a + t[k] * (b - a), in this form, with a = field[c * NP + edges[2k]]
 * and b = field[c * NP + edges[2k + 1]], c < ncomp (exactly a where t == 0).  n_verts = dim * n_prims for the arrays of
 * lgh_contour.  Device arrays; asynchronous on the context's stream. */
int lgh_contour_gather(lgh_ctx *ctx, long n_verts, const int *edges, const double *t, int ncomp, long NP,
                       const double *field /* [c * NP + pt] */, double *out /* [c * n_verts + k] */);
/* The two scalars that are no block of the sampling kernels, from the x or v block `in` ([c * NP + pt], c < dim; dim 2 or 3):
 * mode 0: coef[0] * x + coef[1] * y (+ coef[2] * z), each product rounded, summed in this order (the plane family; x, y, z
 * themselves with unit coefficients); mode 1: sqrt(x^2 + y^2 (+ z^2)) in the same order (|v|; coef may be NULL).  Asynchronous. */
int lgh_contour_scalar(lgh_ctx *ctx, int mode, long NP, int dim, const double *in, const double coef[4], double *out);
/* Zones per workgroup of the count and emit kernels: min(16, 1024 / R1^dim), at least 1.  Grids of ZPB - 1, ZPB, ZPB + 1 zones
 * are the edges of a launch.  LGH_ERR_ARG where lgh_contour refuses dim or R1. */
int lgh_contour_zpb(lgh_ctx *ctx, int R1, int *zpb);

/* ---- running records at material points (the driver's `-peaks`): a lattice point of lgh_sample_fields / lgh_sample_faces is
 * the same particle in every cycle, so what happened THERE over time is kept per lattice point.  p, rho, e (n each) and
 * v[c * n + i], c < dim, are the device arrays those calls wrote at time t; rec[c * n + i], c < LGH_RECORDS_COLS, is the record
 * block (device), columns
 *   0 p_max   1 t_p_max   2 impulse   3 p_last   4 rho_max   5 speed_max   6 e_max   7 t_arrival
 * first != 0 starts the records (dtr must be 0; rec is written, not read): p_max = p_last = p, t_p_max = t, impulse = 0,
 * rho_max = rho, speed_max = |v|, e_max = e, t_arrival = (p >= threshold) ? t : -1.  Otherwise, dtr the time since the last
 * update: p > p_max (strictly: the first attainment keeps its time) sets p_max = p, t_p_max = t; impulse = impulse + (0.5 dtr)
 * (p_last + p), the trapezoid rule with 0.5 dtr formed once on the host; p_last = p; rho_max, speed_max, e_max move by >;
 * t_arrival < 0 && p >= threshold sets t_arrival = t.  threshold NaN: no threshold, t_arrival stays -1.
 * |v| = sqrt(v_0^2 + v_1^2 (+ v_2^2)), summed in ascending order.  A NaN sample moves no extreme (comparisons with it are
 * false) and makes the impulse NaN; nothing is trapped.  Every column but speed_max has the bits of these formulas evaluated
 * operation by operation in IEEE double (no contraction into an fma); speed_max may be contracted.
 * LGH_ERR_ARG with the value in the message, nothing launched: n < 0, a NULL array with n > 0, dim outside 1..3, t not finite,
 * dtr negative or not finite, first with dtr != 0, threshold infinite.  n == 0: LGH_OK, no launch.  The arrays may start at
 * any 8-byte aligned address (with n odd every second column does: such a column is read and written 8 bytes at a time).
 * Asynchronous on the context's stream; reads its inputs, reads and writes rec only: the quadrature data, its generation
 * counter and the fused force products are untouched.  dim is the caller's (the context's mesh is not looked at). */
#define LGH_RECORDS_COLS 8
int lgh_records_update(lgh_ctx *ctx, long n, int dim, const double *p, const double *rho, const double *e,
                       const double *v /* v[c*n + i], c < dim */, double t, double dtr, double threshold /* NaN: none */,
                       int first, double *rec /* rec[c*n + i], c < LGH_RECORDS_COLS */);
/* The launch lgh_records_update makes for n points: out[0] = workgroups (0: no launch), out[1] = threads of a workgroup,
 * out[2] = points a lane takes per trip, out[3] = trips of a lane's loop.  The grid is capped: for n large enough out[0] is
 * the cap and out[0] * out[1] * out[2] the points of one trip. */
int lgh_records_shape(lgh_ctx *ctx, long n, long out[4]);

/* ---- gauges: time series at material points (the driver's `-gauges`).  A gauge is a point (zone, reference coordinates
 * xi in [0, 1]^dim): the same particle in every cycle, so nothing is located after the caller has chosen it.  A set of n
 * gauges is an object of the context (a handle; destroying the context frees it).  The caller hands over the 1-D basis
 * values at xi, as with the lattice tables - the library holds no basis definition:
 *   Bh[(g*dim + a)*D1D + d]  H1 basis function d at xi_a of gauge g      Gh: its derivative
 *   Bl[(g*dim + a)*L1D + l]  L2 basis function l there
 * zone[g] is the caller's zone id on this rank, -1 where another rank owns the gauge.  A sample is one row of LGH_GAUGE_COLS
 * doubles per gauge,
 *   0..2 x   3..5 v   6 rho   7 e   8 p   9 cs   10 det J   11 div v      (components >= dim are 0)
 * contracted with the stages and in the order of lgh_sample_fields / lgh_sample_derived (x axis first, every sum over its dofs
 * ascending in one thread): a gauge at a lattice point, given that lattice's table rows, has the bits those calls hold there.
 * det J = det(dx/dxi), div v = tr((dv/dxi) adj(J) / det J), cs = sqrt(gamma_z (gamma_z - 1) max(e, 0)) as lgh_sample_derived;
 * rho = m_g / det J, ONE division, with m_g = rho0(xi) * det J0(xi) formed once at create from x0_h1 and rho0_l2 (device; the
 * arrays lgh_setup_rho0detj0 took): the scheme's own pointwise density - strong mass conservation, what the quadrature update
 * uses at its points - and not the projected density of the dumps; p = (gamma_z - 1) rho max(e, 0).  No branch looks at the
 * sign of det J and nothing is trapped: an inverted zone gives det J <= 0, a NaN dof NaN, in the rows of its gauges only.
 * lgh_gauges_sample appends one sample of the state S to the set's buffer of `capacity` samples: one kernel on the context's
 * stream, no host wait; it reads S and writes the buffer only (the quadrature data, its generation counter and the fused force
 * products are untouched).  On a full buffer: LGH_ERR_ARG, nothing launched.  lgh_gauges_drain synchronises, copies the pending
 * samples to host_out[(s*n + g)*LGH_GAUGE_COLS + col], oldest first, and empties the buffer; *samples = their number (0: nothing
 * was pending); max_samples below it: LGH_ERR_ARG, nothing drained.  lgh_gauges_mass: m_g (n doubles, host).
 * Several ranks: every rank creates the set with the same n and capacity and samples and drains in step.  A rank fills the rows
 * of gauges it does not own with -0.0 (m_g likewise) and the drain is collective, a SUM all-reduce of the transport: x + (-0.0)
 * has the bits of x for every x, signed zeros included, so the sum is an exact gather and every rank gets every row.  A gauge
 * that no rank owns, or two (on one rank: a zone of -1), is refused at create, on every rank.
 * LGH_ERR_ARG with the value in the message, nothing launched or kept: n < 1, capacity < 1, a NULL argument, a call before
 * lgh_setup_rho0detj0, capacity * n above LGH_GAUGE_MAX_ROWS (these must be the same on every rank), a zone outside -1..NE-1, a
 * table entry that is not finite (these are agreed on between the ranks: all refuse), an unknown handle.  LGH_ERR_UNSUPPORTED: a gauge that needs more than 48 KB
 * of LDS (D1D = 9 in 3D).
 * lgh_gauges_shape: out[0] = gauges per workgroup (one wavefront each), out[1] = workgroups of a sample, out[2] = bytes of LDS
 * of a workgroup, out[3] = its threads. */
#define LGH_GAUGE_COLS 12 /* x0 x1 x2 v0 v1 v2 rho e p cs detj div_v ; components >= dim are 0 */
#define LGH_GAUGE_MAX_ROWS 16777216L /* capacity * n of a set: 1.5 GiB of rows */
int lgh_gauges_create(lgh_ctx *ctx, int n, const int *zone /* caller's zone id on this rank, -1: not this rank's */,
                      const double *Bh /* host, n*dim*D1D: H1 basis values at xi_g, [(g*dim + a)*D1D + d] */,
                      const double *Gh /* their derivatives */, const double *Bl /* n*dim*L1D, L2 basis values */,
                      const double *x0_h1 /* device */, const double *rho0_l2 /* device */, int capacity, int *handle);
int lgh_gauges_sample(lgh_ctx *ctx, int handle, const double *S); /* asynchronous, appends one sample */
int lgh_gauges_pending(lgh_ctx *ctx, int handle, int *samples);
int lgh_gauges_drain(lgh_ctx *ctx, int handle, double *host_out /* [s][g][LGH_GAUGE_COLS] */, int max_samples, int *samples);
int lgh_gauges_mass(lgh_ctx *ctx, int handle, double *host_m /* n */);
int lgh_gauges_shape(lgh_ctx *ctx, int handle, long out[4]); /* gauges per workgroup, workgroups, LDS bytes, threads */
int lgh_gauges_destroy(lgh_ctx *ctx, int handle);

/* ---- timing data (TimingData, laghos_solver.hpp:39-56): seconds measured with
 * HIP events around the same regions as the reference stopwatches.
 * t[0..3] = cgH1, cgL2, force, qdata; c[0..2] = H1iter, L2iter, quad_tstep */
int lgh_get_timers(lgh_ctx *ctx, double t[4], long c[3]);
int lgh_reset_timers(lgh_ctx *ctx);
int lgh_enable_timers(lgh_ctx *ctx, int on);

/* ---- per-kernel timing with HIP events on the context stream (bench.py roofline):
 * between begin and end every launch of kernel `which` is bracketed by an event
 * pair (up to max_samples launches); end synchronises and returns the number of
 * sampled launches and their mean duration in seconds. */
#define LGH_KERNEL_MASS_CG_H1 0   /* K1: gather + B^T D B + (d,Ad), H1 CG */
#define LGH_KERNEL_CG_UPDATE_H1 1 /* K2: transpose gather + vector updates + (r,z) */
#define LGH_KERNEL_QUPDATE 2
#define LGH_KERNEL_FORCE_MULT 3
#define LGH_KERNEL_FORCE_MULT_T 4
#define LGH_KERNEL_MASS_CG_L2 5
#define LGH_KERNEL_HALO 6         /* one shared-node / scalar exchange over RCCL: pack, grouped send/recv, combine */
#define LGH_KERNEL_ALLREDUCE 7    /* one ncclAllReduce of device scalars */
#define LGH_KERNEL_SAMPLE 8       /* lgh_sample_fields */
#define LGH_KERNEL_FINGERPRINT 9  /* lgh_vec_fingerprint */
#define LGH_KERNEL_DIAG 10        /* the zone kernel of lgh_diagnostics_zones / lgh_diagnostics */
#define LGH_KERNEL_PROFILE 11     /* lgh_profile: both passes over the zones and the kernels between and behind them */
#define LGH_KERNEL_DERIVED 12     /* lgh_sample_derived */
#define LGH_KERNEL_MAP 13         /* lgh_map: as LGH_KERNEL_PROFILE */
#define LGH_KERNEL_FACES 14       /* lgh_sample_faces */
#define LGH_KERNEL_LOADS 15       /* lgh_loads: both passes over the faces and the kernels between and behind them */
#define LGH_KERNEL_CONTOUR 16     /* lgh_contour: the count pass, the scan, the look at the totals and the emit pass of one call */
#define LGH_KERNEL_RECORDS 17     /* lgh_records_update */
#define LGH_KERNEL_GAUGES 18      /* lgh_gauges_sample */
int lgh_ktime_begin(lgh_ctx *ctx, int which, int max_samples);
int lgh_ktime_end(lgh_ctx *ctx, int *launches, double *mean_seconds);
/* Whether lgh_create found the 1-D H1 / L2 tables mirror symmetric, B[q,d] = B[Q-1-q, D-1-d] (any nodal or
 * Bernstein basis on symmetric points is): the plane-form mass kernels keep half a table in scalar registers
 * and are only dispatched then (the column forms run otherwise). */
int lgh_table_symmetry(lgh_ctx *ctx, int *h1, int *l2);
/* Which form of the mass-apply kernel K1 the lockstep velocity solve (lgh_solve_velocity) launches for this
 * context: 0 = column form, 2 = plane form, 4 = slab form (sum factorisation in registers, lane-group transposes by v_permlane swaps, Q3Q2 only),
 * 5 = Kronecker form (compact mass data on a tensor-product rule: the element matrix as s_e M1 (x) M1 (x) M1 with the
 * 1-D mass tile M1 = B^T diag(w) B; the slab form applies the same where it is dispatched),
 * -1 = no lockstep solve for this kernel id (the scalar CG runs).  Tests use it to make sure a requested
 * form (LGH_VCG_VARIANT) is the one that ran. */
int lgh_k1_form(lgh_ctx *ctx, int *form);
/* Which kernel MassPAOperator::Mult on the L2 space (the energy CG, laghos_solver.cpp:480-488) launches for this context:
 * 2 = Kronecker form s_e M1l (x) M1l (x) M1l (compact mass data on a tensor-product rule, L1D <= 5), 1 = plane form,
 * 0 = column form; *compact = 1 when that kernel reads one factor per element instead of the NQ-entry table
 * (bench.py's byte accounting follows the kernel that runs, not the kernel id). */
int lgh_l2_mass_form(lgh_ctx *ctx, int *form, int *compact);
/* What the mass-apply kernel K1 of the lockstep velocity solve hands to its node kernel K2 in this context, for byte
 * accounting (bench.py): out[0] = doubles per velocity component of the E-vector between them (NE * D1D^3 in the
 * element-local layout; about a fifth less where the slab form of K1 sums the shared x-faces of a set of five zones
 * itself), out[1] = bytes of the transposed-restriction table K2 always reads (16 per node: contributions 1..4),
 * out[2] = bytes of its second half (contributions 5..8) in the 64-node blocks that need it, out[3] = E-vector entries
 * K1 has summed into a neighbour's.  Replaces nothing in the reference: there the E -> L sum is H1R^T
 * (laghos_assembly.cpp:121) inside every operator apply. */
int lgh_vcg_layout_stats(lgh_ctx *ctx, long out[4]);

/* The order in which the library walks the zones and numbers the nodes of its OWN vectors (the velocity solve's r, d, x,
 * 1/diag, E-vector and tables; the zone order of lgh_qupdate).  The reference hands its operators whatever numbering the mesh
 * library has - H1.GetElementRestriction(LEXICOGRAPHIC) of an MFEM space: vertex, edge, face, interior dofs; zones in the
 * order UniformRefinement leaves them (laghos_assembly.cpp:133-134, laghos.cpp:391) - and only the element-local dof order is
 * part of the interface.  lgh_create therefore finds the structure itself, from h1_map alone: zones are neighbours along a
 * local axis when the D1D x D1D nodes of their facing faces coincide position by position; a flood fill gives the zones of a
 * structured block integer coordinates; zones are then taken row by row and the nodes numbered along those rows.  The
 * caller's vectors keep the caller's numbering: they are read / written through the permutation once per solve.
 *   out[0] = 1: the mesh is a set of structured blocks (else the caller's order is kept: general path);
 *   out[1] = 1: the internal order IS the caller's (nothing is permuted; e.g. a lexicographic Cartesian generator);
 *   out[2] = connected components; out[3..5] = zones of the first component along its local x, y, z.
 * LGH_ORDER=0 keeps the caller's order everywhere (A/B).  Replaces nothing in the reference: MFEM's numbering is what it is. */
int lgh_mesh_order(lgh_ctx *ctx, long out[8]);
/* The same analysis as a host helper (no GPU, no context; tests, and callers that want to look at the order before they
 * create a context): zorder[i] = the caller's zone that comes i-th, nnum[n] = internal number of the caller's node n (both
 * the identity when out[0] == 0 or dim != 3); out as above. */
int lgh_mesh_order_host(int dim, int NE, int N, int D1D, const int *h1_map, int *zorder, int *nnum, long out[8]);

/* ---- multi-GPU: element blocks per rank, shared H1 nodes summed
 * over RCCL, dot products / dt all-reduced.  unique_id is the 128-byte
 * ncclUniqueId produced by lgh_comm_unique_id on rank 0 and broadcast by the
 * caller (e.g. torch.distributed).  Neighbour lists: for each of n_nbr peers,
 * the local node indices shared with that peer, sorted identically on both
 * sides (global lexicographic order). */
int lgh_comm_unique_id(char id_out[128]);
int lgh_comm_init(lgh_ctx *ctx, int nranks, int rank, const char unique_id[128]);
/* An id for the cross-process loopback transport instead of RCCL (tests, `bench.py --transport shm`): the ranks are
 * processes as on a node, but may share one GPU (RCCL refuses that); exchanges are staged through a POSIX
 * shared-memory segment named by the id.  Everything above the transport is the code a multi-GPU node runs. */
int lgh_comm_unique_id_shm(char id_out[128]);
int lgh_comm_set_neighbors(lgh_ctx *ctx, int n_nbr, const int *nbr_rank, const int *nbr_count,
                           const int *const *nbr_nodes);
/* What the exchanges of this rank look like (bench.py's `comm` block): neighbours, nodes of the largest message,
 * distinct shared nodes, whether every rank neighbours every other (sums then ride on the halo messages) and
 * whether the second channel (energy solve beside the velocity solve) is up. */
int lgh_comm_stats(lgh_ctx *ctx, int *n_neighbours, long *max_nodes_per_neighbour, long *shared_nodes, int *all_pairs,
                   int *second_channel);
/* Host helper (no GPU, no context): the `owner` mask of lgh_config and the neighbour lists of
 * lgh_comm_set_neighbors from a description of the shared dofs by GROUPS - the form in which MFEM holds them
 * (ParFiniteElementSpace::GroupComm(): GroupTopology = the rank set and master of every group,
 * GroupLDofTable = its L-dofs in an order common to all members; this is what P / P^T of
 * laghos_solver.cpp:368, :393 are built from).  INTEGRATION.md §4 shows the MFEM side.
 *   group g: ranks  group_ranks[group_off[g] .. group_off[g+1])  (my_rank among them, any order),
 *            master group_master[g] (NULL: the lowest rank of the group),
 *            L-dofs ldofs[ldof_off[g] .. ldof_off[g+1]) in the group's common order.
 * Outputs: owner[N] = 0 for dofs of groups mastered elsewhere, 1 otherwise;  *n_nbr peers in ascending rank
 * order, nbr_rank[k], nbr_count[k], and their node lists concatenated in nbr_nodes (neighbour k starts at the sum
 * of the counts before it).  For a peer the groups are taken in the order of their sorted rank sets (a key that
 * is the same on both sides) and the dofs inside a group in the group's order, so the two ranks of a pair
 * enumerate their shared dofs identically.  Capacities: nbr_rank / nbr_count >= number of distinct peers,
 * nbr_nodes >= sum over the groups of (size - 1) * number of dofs; cap_nbr / cap_nodes are checked. */
int lgh_groups_to_neighbors(int my_rank, int N, int n_groups, const int *group_off, const int *group_ranks,
                            const int *group_master, const int *ldof_off, const int *ldofs, double *owner,
                            int *n_nbr, int *nbr_rank, int *nbr_count, int cap_nbr, int *nbr_nodes, long cap_nodes);
/* in-place sum of shared nodes of an H1 L-vector with ncomp components */
int lgh_halo_sum(lgh_ctx *ctx, double *v_h1, int ncomp);
/* op 0 = sum, 1 = min; synchronous */
int lgh_allreduce(lgh_ctx *ctx, double *value, int op);

/* ---- E-vector level entry points (kernel-granularity parity tests only) */
int lgh_force_mult_E(lgh_ctx *ctx, const double *sJit, const double *x_E, double *y_E);
int lgh_force_mult_transpose_E(lgh_ctx *ctx, const double *sJit, const double *v_E, double *y_E);
int lgh_mass_apply_E(lgh_ctx *ctx, int space, const double *x_E, double *y_E);
/* ONE launch of the mass-apply kernel K1 of the lockstep velocity solve - in whichever form lgh_k1_form() reports
 * (column / plane / slab / Kronecker), i.e. the kernel lgh_solve_velocity spends most of its time in - exactly as
 * the solve launches it: first != 0: the first iteration (d = r/diag), else a later one (d = r/diag + beta d_old,
 * beta = rz[c] / rz_prev[c]).  r, d_old: H1 vectors of 3 components (byNODES, device); rz, rz_prev, den: 3 host
 * doubles; y_E: 3 planes of NE*D1D^3 (device) = the element contributions A_e d_e (MassPAOperator::Mult before the
 * E->L sum, laghos_assembly.cpp:117-121); den[c] = (d_c, A d_c).  rz[c] must be (r_c, r_c/diag) of the vectors
 * given (the slab form scales its exact accumulators by it).  Single rank; synchronous; overwrites the solve's own
 * work vectors only. */
int lgh_test_vcg_k1(lgh_ctx *ctx, const double *r, const double *d_old, const double rz[3], const double rz_prev[3],
                    int first, double *y_E, double den[3]);
/* The slab form of K1 stores a set of five x-neighbouring zones with the shared x-faces already summed (merged E-vector
 * layout, round 5: what K2 reads shrinks by a fifth and comes in whole cache lines).  lgh_test_vcg_k1 then reports such a
 * sum in the LEFT zone's entry (dx = 3) and 0.0 in the right zone's (dx = 0); mask[e * D1D^3 + d] (host, NE * D1D^3
 * bytes) = 1 marks those right-hand entries, *n_merged counts them (0 with every other form of K1 or LGH_SLAB_MERGE=0).
 * lgh_test_vcg_k2 takes the element-local E-vector either way (it forms the sums K1 would have stored). */
int lgh_test_vcg_merged_faces(lgh_ctx *ctx, unsigned char *mask, long *n_merged);
/* ONE launch of the node kernel K2 of the lockstep velocity solve (the kernel with the largest share of the step: the
 * E -> L sum of K1's element contributions, essential rows, r -= alpha A d, d = r_old/diag + beta d, the deferred update
 * of x, (r, r/diag)) exactly as the one-rank solve launches it in iteration it >= 1: y_E = 3 planes of NE*D1D^3
 * (device) as lgh_test_vcg_k1 returns them; r, d, x: H1 vectors of 3 components (device), updated in place - d in: the
 * direction of iteration it-1 (ignored for it = 1), d out: that of iteration it; den[c] = (d_c, A d_c) of this
 * iteration, rz[c] / rz_prev[c] = (r, z) after iterations it-1 / it-2, alpha_prev[c] = alpha of iteration it-1 (host
 * doubles).  rz_out[c] = (r, z) of the new residual.  *deferred_x = 1: the bounded-grid kernel ran - x is updated
 * only in even iterations, with the terms of iterations it and it-1 (it = 2: x := both terms, the old content is not
 * read); 0: the round-1 kernel (LGH_K2P=0), x += alpha d every iteration.  Single rank; synchronous. */
int lgh_test_vcg_k2(lgh_ctx *ctx, int it, const double *y_E, double *r, double *d, double *x, const double den[3],
                    const double rz[3], const double rz_prev[3], const double alpha_prev[3], double rz_out[3],
                    int *deferred_x);
/* The exact integer accumulators every (d, A d) and (r, z) of the lockstep velocity solve goes through (lgh_vcg.hpp), on
 * their own: the probe's kernels call the solve's own device functions.  Host arrays in, host arrays out; synchronous;
 * single rank.  E is the scale of the window, or - scale != NULL - exact_scale(*scale) taken on the device.
 *   mode 0, split: one thread per addend v[i] (n of them): exact_add into zeroed accumulators; w_out[4 i + j] = limb j,
 *           i_out[i] = 1 accepted / 0 refused (accumulators untouched).
 *   mode 1, value: d_out[i] = exact_value of the limb words w_in[4 i .. 4 i + 3] under E (scale must be NULL).
 *   mode 2, grid: n addends per component (v[k n + i], k < 3) over G workgroups of 256 threads as the tail of the slab K1
 *           adds them (per-thread exact_add, wave_sum_i64, LDS, one atomic per word into shard blockIdx % 4, atomic or
 *           into the flag word) into a cleared set; a second launch folds the set: w_out = its 56 raw words,
 *           d_out[k] = exact_den, d_out[3 + k] = exact_fold, d_out[6 + k] = exact_fold_lanes (one full wavefront, word l
 *           in lane l).  exact_den gets *scale, or a value whose exact_scale is E.
 *   mode 3, wave: w_out[64 b + l] = what lane l of wavefront b gets from wave_sum_i64 of w_in[64 b .. 64 b + 63]
 *           (n a multiple of 64).
 *   mode 4, scale: i_out[i] = exact_scale(v[i]).
 * Arguments a mode does not use may be NULL / 0. */
int lgh_test_exact_sum(lgh_ctx *ctx, int mode, long n, int G, int E, const double *scale, const double *v,
                       const long long *w_in, long long *w_out, double *d_out, int *i_out);
/* halo pieces without the RCCL transport (tests emulate the exchange between
 * several contexts on one GPU): rank bookkeeping, pack into / combine from caller
 * buffers of 3*total doubles laid out as the send / receive buffers are. */
int lgh_test_set_rank(lgh_ctx *ctx, int nranks, int rank);
int lgh_test_halo_pack(lgh_ctx *ctx, const double *v_h1, int ncomp, double *sendbuf_out);
int lgh_test_halo_combine(lgh_ctx *ctx, const double *recvbuf_in, double *v_h1, int ncomp);
/* the peer buffer of the exact word exchange (the (r, z) accumulator words of the velocity CG on all-pairs partitions) as
 * the solve would size it for `nwords` words per peer: *capacity_words = peers x nwords.  A second
 * lgh_comm_set_neighbors with more neighbours must grow it (round-5 advisor). */
int lgh_test_word_peers(lgh_ctx *ctx, int nwords, long *capacity_words);
/* grouped ncclSend / ncclRecv of n doubles from this rank to itself on the RCCL communicator (what
 * halo_sum does with its neighbours); *max_abs_diff = max |received - sent| */
int lgh_test_rccl_self_sendrecv(lgh_ctx *ctx, int n, double *max_abs_diff);
/* device small-matrix probes: n matrices (column-major, 9 or 4 doubles each) */
int lgh_test_eig(lgh_ctx *ctx, int dim, int n, const double *A, double *lambda, double *vec);
/* y[i] = the device square root the small-matrix routines use (rsq + Goldschmidt step + correction), n device doubles */
int lgh_test_sqrt(lgh_ctx *ctx, int n, const double *x, double *y);
int lgh_test_singular(lgh_ctx *ctx, int dim, int n, const double *A, double *sv_min);

#ifdef __cplusplus
}
#endif
#endif /* LAGHOS_HIP_H */
