// lgh_common.hpp — context, error handling and device reduction helpers shared by
// the HIP translation units of liblaghos_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/laghos_hip.h"

namespace lgh
{

void set_error(const char *fmt, ...);

#define LGH_HIP_CHECK(expr)                                                              \
   do                                                                                    \
   {                                                                                     \
      hipError_t e_ = (expr);                                                            \
      if (e_ != hipSuccess)                                                              \
      {                                                                                  \
         lgh::set_error("HIP error %s at %s:%d: %s", hipGetErrorName(e_), __FILE__,      \
                        __LINE__, #expr);                                                \
         return LGH_ERR_HIP;                                                             \
      }                                                                                  \
   } while (0)

#define LGH_CHECK_ARG(cond)                                                              \
   do                                                                                    \
   {                                                                                     \
      if (!(cond))                                                                       \
      {                                                                                  \
         lgh::set_error("bad argument: %s (%s:%d)", #cond, __FILE__, __LINE__);          \
         return LGH_ERR_ARG;                                                             \
      }                                                                                  \
   } while (0)

#define LGH_PASS(call) do { const int rc_ = (call); if (rc_ != LGH_OK) { return rc_; } } while (0) // an LGH_* status: passed on

constexpr int kWave = 64;          // gfx950 wavefront

// One device allocation, freed with its owner (move-only): the only place of the library that allocates or frees device
// memory.  alloc and upload release what the pointer holds first, so a buffer regrows by calling them again.
template <typename T> struct DevPtr
{
   T *p = nullptr;
   DevPtr() = default;
   DevPtr(DevPtr &&o) noexcept : p(o.p) { o.p = nullptr; } // (declaring the moves deletes the copies)
   DevPtr &operator=(DevPtr &&o) noexcept { std::swap(p, o.p); return *this; }
   ~DevPtr() { reset(); }
   operator T *() const { return p; }
   T *operator->() const { return p; }
   void reset() { if (p) { (void)hipFree(p); p = nullptr; } } // (an empty one never touches the runtime: host-only entry points hold some)
   int alloc(const size_t n, const bool zero = false) // n elements, uninitialised or zero
   {
      reset();
      LGH_HIP_CHECK(hipMalloc((void **)&p, n * sizeof(T)));
      if (zero)
      {
         LGH_HIP_CHECK(hipMemset(p, 0, n * sizeof(T)));
         LGH_HIP_CHECK(hipStreamSynchronize(nullptr)); // (the fill runs on the null stream; a context's stream does not wait for it)
      }
      return LGH_OK;
   }
   int upload(const T *host, const size_t n) // n elements, copied from the host
   {
      const int rc = alloc(n);
      if (rc != LGH_OK) { return rc; }
      LGH_HIP_CHECK(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
      return LGH_OK;
   }
};
// a buffer of a context's set-up: at least one element, so never null; copied from `src`, or zero without one
template <typename T> int ctx_buffer(DevPtr<T> &d, const size_t n, const T *src = nullptr)
{
   const int rc = d.alloc(std::max<size_t>(n, 1), !src);
   if (rc != LGH_OK || !src || !n) { return rc; }
   LGH_HIP_CHECK(hipMemcpy(d.p, src, n * sizeof(T), hipMemcpyHostToDevice));
   return LGH_OK;
}

// Device-resident scalars of one CG solve (SURVEY §3.2 names).
struct CgScalars
{
   double rz;       // (r, z) current: nom, later betanom
   double rz_prev;  // previous (r, z): denominator of beta
   double den;      // (d, A d)
   double r0;       // max(nom*rel_tol^2, abs_tol^2)
   double nom0;     // initial nom
   double rel_tol2; // rel_tol^2 (set by host before the init kernel)
   int done;        // 1: converged / breakdown, later kernels become no-ops
   int iters;       // final_iter
   int first;       // 1 until the first direction has been formed (beta = 0)
   int pad;
};

// Layout of lgh_ctx::host_pinned in doubles.  A scalar CG stages its CgScalars over the front; between solves the first
// slots take single results.  Everything behind has one user.
constexpr int kPinDoubles = 96;
constexpr int kPinResult = 0;                      // a reduction's result (volume, energy, error norm); CgScalars during a scalar CG
constexpr int kPinDot = 1;                         // lgh_vec_dot
constexpr int kPinReduceOut = 2, kPinReduceIn = 3; // lgh_allreduce: the value on its way back / in
constexpr int kPinDt = 8, kPinDtFlag = 9, kPinDtToken = 10; // the dt estimate, its error word, the token of its look (dt_est_fold_k writes the three in a row)
constexpr int kPinVcg = 32;                        // the velocity CG's scalars at a look (VcgScalars, lgh_vcg.hpp) ...
constexpr int kPinVcgToken = 80;                   // ... and the token of that look
static_assert(sizeof(CgScalars) <= kPinDt * sizeof(double) && kPinDtFlag == kPinDt + 1 && kPinDtToken == kPinDt + 2 && kPinDtToken < kPinVcg &&
              kPinVcgToken < kPinDoubles, "slots of the pinned block: disjoint, inside the allocation");

struct Timers
{
   bool enabled = true;
   hipEvent_t ev[2] = {nullptr, nullptr};
   Timers() = default;
   Timers(const Timers &) = delete;
   Timers &operator=(const Timers &) = delete;
   ~Timers() { for (hipEvent_t e : ev) { if (e) { (void)hipEventDestroy(e); } } }
   double t[4] = {0, 0, 0, 0}; // cgH1, cgL2, force, qdata (seconds)
   long c[3] = {0, 0, 0};      // H1iter, L2iter, quad_tstep
};

// event pairs around the launches of one kernel (lgh_ktime_begin / _end)
struct KTime
{
   int which = -1, max = 0, n = 0;
   std::vector<hipEvent_t> ev; // 2 per sample
   KTime() = default;
   KTime(const KTime &) = delete;
   KTime &operator=(const KTime &) = delete;
   ~KTime() { for (hipEvent_t e : ev) { (void)hipEventDestroy(e); } }
};

struct Comm;       // several ranks: the transport and the neighbour tables (lgh_comm_transport.hpp)
struct VcgScalars; // the device scalars of the velocity CG (lgh_vcg.hpp)
struct VcgAux;     // ... and the tables of its node kernel K2

// The library's own order of the zones and numbering of the nodes (lgh_order.hip): found from the element -> node map at
// lgh_create by face adjacency, nothing about the caller's numbering is assumed.  identity: the caller's order already is
// that order (or no structured block was found, or LGH_ORDER=0) - nothing is permuted anywhere.
struct MeshOrder
{
   bool structured = false, identity = true;
   int components = 0, extent[3] = {0, 0, 0};
   std::vector<int> zorder;   // internal zone i is the caller's zone zorder[i]
   std::vector<int> nnum;     // the caller's node n is internal node nnum[n]
   std::vector<int> ncaller;  // internal node m is the caller's node ncaller[m]
   DevPtr<int> zorder_d, ncaller_d, nnum_d; // the same on the device (nullptr when identity)
};

constexpr double kMassRank1Tol = 1e-12; // relative spread of D / W inside an element up to which the mass data counts as W[q] s_e (mass_rank1_k)
constexpr double kJac0Tol = 1e-12;      // ... of Jac0inv inside a zone up to which it counts as one matrix per zone (jac0_compact_k)

// Every environment switch of the library (DESIGN.md "Environment switches"), read ONCE per context: a context's switches
// are those of the environment at its lgh_create (read_switches, lgh_switches.hip - the only place that asks the environment,
// but for the two properties of the shared-memory transport, LGH_SHM_MB and LGH_SHM_TIMEOUT, read where it is opened: ShmGroup::open, lgh_comm_transport.hip).
// Changing the environment afterwards changes nothing for a context that exists; contexts of one process may differ.
// Flags are 0 / 1; -1 where "not set" is an answer of its own.  Field x holds LGH_X unless noted.
struct Switches
{
   // velocity CG (lgh_vcg*.hip)
   int vcg_variant;      // which K1 form vcg_solve launches; -1: by kernel id and mesh size (vcg_k1_form)
   int slab_wide, slab_exact, slab_merge, slab_defer, slab_ye_wide; // slab-form K1
   int slab_dyn;         // ... sets drawn from a workgroup queue: 0 / 1, -1: by passes per wavefront (launch_vcg_slab)
   int rz_limbs, kron_neb, fused_init;
   int k2p, k2_skip, k2_grid; // K2; k2_grid: node ranges per CU, 0: by mesh size
   long k2_node_weight;  // fixed part of a node's cost in units of half a contribution; < 0: equal counts
   int order, order_multi;
   // several ranks (lgh_comm.hip), energy solve beside the velocity solve (lgh_energy.hip), host looks
   int comm2;            // -1: not set (the loop-back transports then have the second channel, RCCL on more than one rank does not)
   int force_multi, halo_piggyback, halo_fused_pack, overlap, energy_lockstep, spin;
   // mass operators (lgh_mass.hip) and the scalar CG on them (lgh_scg.hip)
   int mass_sep, mass_kron, mass_rank1, l2_neb, l2_plane, l2_fused;
   double mass_rank1_tol; // (default kMassRank1Tol)
   // quadrature update and set-up
   int q_form, q_ppt, q_swz, fused_ftv, fused_f1, b_sym, jac0_compact;
   int q_occ4;           // -1: not set (by viscosity and the form of Jac0inv, launch_qrows)
   int q_discard;        // 1 (default): the update skips work whose result is provably discarded; 0: off; A/B: 2 the dt candidate only, 3 the F.1 rows only
   double q_tiny_grad;   // the threshold a context starts with (lgh_ctx::q_tiny_grad)
   double jac0_tol;      // (default kJac0Tol; at most 1e-10)
   int profile_fold;
   int map_fold;
   // debug
   int roctx, vcg_trace_phases, q_trace_call;
   std::string vcg_trace, q_trace; // files; empty: no trace
};
Switches read_switches();

struct ScalarCg; // one scalar CG solve: what its kernels are launched with, how far it has been enqueued (lgh_scg.hip)
void cg_l2_free(ScalarCg *r);

// The energy solve between lgh_solve_energy_begin and _end (lgh_energy.hip): which way _begin took, and what _end needs for it.
struct EnergySolve
{
   enum Mode
   {
      Idle,       // no solve begun
      Overlapped, // right-hand side and first chunk of the CG enqueued on the second stream, beside the velocity solve
      Deferred,   // nothing enqueued: _end runs the whole of lgh_solve_energy with the saved arguments
      Lockstep    // several ranks, one stream and communicator: set up on the main stream, lgh_solve_velocity interleaves the iterations
   };
   Mode mode = Idle;
   bool polled = false; // Overlapped: completed from inside the velocity solve already (energy_overlap_poll) ...
   int iters = 0;       // ... with this iteration count
   struct { const double *S, *v; double *dS, *e_rhs; const double *src; double tol; int maxit; } args = {}; // Deferred
};

// What a context holds that is not device memory: its streams, the events between them and the pinned block.  The energy
// solve swaps `stream` and `stream2` while it runs, so they stay plain handles; they are released here, in the destructor
// of lgh_ctx's base - after every member of lgh_ctx, so after everything that could still be enqueued on an owned stream.
struct CtxHandles
{
   int device = 0;
   hipStream_t stream = nullptr;
   bool own_stream = false;
   // second stream + fork/join events: the energy solve overlaps the velocity solve (lgh_energy.hip)
   hipStream_t stream2 = nullptr;
   hipEvent_t ev_fork = nullptr, ev_join = nullptr;
   double *host_pinned = nullptr;     // pinned host staging, kPinDoubles doubles; its slots: kPin*
   double *host_pinned_dev = nullptr; // the same memory as the device addresses it: scalars a host look needs are written there by the kernel that
                                      // finishes them (no copy kernel between it and the stream synchronisation)
   CtxHandles() = default;
   CtxHandles(const CtxHandles &) = delete;
   CtxHandles &operator=(const CtxHandles &) = delete;
   ~CtxHandles();
};

// One set of gauges (lgh_gauges.hip): material points (zone, reference coordinates) with their 1-D basis values, the mass
// m_g = rho0 det J0 of each and the rows of the samples taken since the last drain.
struct GaugeSet
{
   int n = 0, capacity = 0, pending = 0; // gauges, samples the buffer holds, samples in it
   DevPtr<int> zone;                     // n: the caller's zone id, -1: another rank's
   DevPtr<double> Bh, Gh, Bl;            // n*dim*D1D, the same, n*dim*L1D
   DevPtr<double> mass;                  // n
   DevPtr<double> rows;                  // capacity * n * LGH_GAUGE_COLS
};

} // namespace lgh

// One context.  Every device buffer is a DevPtr of its element type and every other resource has an owner of its own, so
// deleting the context releases all of it, members in reverse order of declaration, then the base: nothing is freed by
// name anywhere (lgh_destroy).  A new buffer is a DevPtr member and an alloc / upload call where it is first needed.
// Buffers that code branches on (owner, w1d, M1h, M1l, erhs_q, v_snap, force_e_q, the first-use ones) are null until built.
struct lgh_ctx : lgh::CtxHandles
{
   lgh_ctx();
   ~lgh_ctx(); // (out of line, lgh_context.hip: where Comm, VcgAux and MeshOrder are complete types)
   lgh::Switches sw;     // the environment switches as they were at lgh_create
   int dim = 0, NE = 0, D1D = 0, Q1D = 0, L1D = 0, ND = 0, NQ = 0, NL = 0, N = 0, H1V = 0, L2V = 0;
   int kid = 0; // (dim<<8)|(D1D<<4)|Q1D, the reference's kernel id
   bool visc = false, vort = false;
   double cfl = 0.0, h0 = 0.0, h1order = 0.0;
   double q_tiny_grad = 0.0;   // QUpdate: threshold of the wave-uniform eigen-decomposition shortcut (lgh_qupdate.hip)
   int q_discard = 0;      // QUpdate: which provably unused work is skipped (kQDiscardDt | kQDiscardF1, lgh_qpoint.hpp; LGH_Q_DISCARD)
   double q_cF = 0.0;      // ... C_F = 3 cG cB^2: |F.1 output| <= C_F max|stressJinvT w detJ| of the zone (q_force_bound, lgh_context.hip)
   int on_stream2 = 0;     // 1 while `stream` holds the second stream (energy solve beside the velocity solve): reductions use the communicator's second channel
   std::unique_ptr<lgh::ScalarCg, void (*)(lgh::ScalarCg *)> l2run{nullptr, lgh::cg_l2_free}; // the run of a split L2 solve (lgh_scg.hip: cg_l2_begin .. cg_l2_end, cg_l2_free), allocated on first use
   const double *accel_src = nullptr; // dim*N acceleration source of SolveVelocity (source_type 2) or nullptr
   lgh::EnergySolve energy; // the energy solve lgh_solve_energy_begin has begun
   long ls_stats[3] = {0, 0, 0}; // lockstep energy solves; their iterations enqueued inside the velocity solve; ... and after it (lgh_energy_lockstep_stats)

   // tables (device): B_h1/G_h1 [q + Q*d], B_l2 [q + Q*l], weights [NQ]
   lgh::DevPtr<double> B, G, Bl, W, gamma;
   // element restriction: gather map, and its transpose in CSR form
   lgh::DevPtr<int> h1map;  // NE*ND
   lgh::DevPtr<int> t_off;  // N+1   (CSR transpose, used by the multi-component force gather)
   lgh::DevPtr<int> t_idx;  // NE*ND: E-vector positions (e*ND + d) contributing to node
   lgh::DevPtr<int> t_ell;  // t_deg*N: the same in ELL format, [k*N + n], -1 = none
   int t_deg = 0;  // max contributions per node (8 for hexes, 4 for quads)
   lgh::DevPtr<uint8_t> essmask[3]; // N each (0/1)
   lgh::DevPtr<int> ess[3];
   int ess_count[3] = {0, 0, 0};
   lgh::DevPtr<double> owner; // N or nullptr
   int cur_ess = -1;

   // QuadratureData + mass PA data
   lgh::DevPtr<double> stressJinvT, Jac0inv, rho0DetJ0w, massD, diagV, dinvV;
   lgh::DevPtr<double> Jac0inv_soa; // plane-major copy of Jac0inv for coalesced reads in QUpdate
   lgh::DevPtr<double> Jac0inv_e; // dim*dim per zone: Jac0inv where it is the same at every point of a zone (an affine initial zone; jac0_compact)
   int jac0_compact = 0; // 1: the row-form update reads Jac0inv_e (checked at lgh_setup_rho0detj0), 0: the point values
   // Rank-1 form of the mass data: where detJ0 and rho0 are constant inside every element (affine elements, piecewise
   // constant density - every mesh and problem of data/), massD[q + NQ e] = W[q] * massS[e] to the last bit or two;
   // the mass kernels then read 8 bytes per element instead of 8 NQ.  -1: not looked at yet (set-up, lgh_mass_D handed
   // out), 0: no (massD as stored), 1: yes (lgh_mass.hip mass_data).  LGH_MASS_RANK1=0 keeps massD.
   lgh::DevPtr<double> massS, ones_ne;
   lgh::DevPtr<double> M1h, M1l; // 1-D mass tiles B^T diag(w1d) B of the H1 (D1D x D1D) and L2 (L1D x L1D) bases: the Kronecker form of the
                                 // mass operators for compact mass data on a tensor-product rule (nullptr: no such rule, or LGH_MASS_KRON=0)
   lgh::DevPtr<double> w1d; // one-dimensional weights when the rule is a tensor product, W[qx + Q (qy + Q qz)] = w[qx] w[qy] w[qz] (checked by lgh_create; nullptr otherwise)
   int mass_rank1 = -1;
   lgh::DevPtr<double> dt_est_dev; // running min of the point-wise estimate: [0] the estimate, then kDtSlots partial minima 128 bytes apart (the row-form
                                   // update sends its candidates there by non-returning atomic min; lgh_get_dt_est folds them into [0])
   // Force products formed inside the fused QUpdate.  Validity is by construction, not by address: `fused_*_valid` says
   // that the product belongs to the quadrature data as it stands (set by lgh_qupdate, cleared by everything that can
   // change stressJinvT: lgh_reset_quadrature_data, lgh_qdata_stressJinvT, lgh_set_fused_forces, the set-up), and
   // F^T v is only used for a velocity that compares equal, element for element, to the one it was formed from.
   lgh::DevPtr<double> erhs_q; // L2V: F^T v of ...
   lgh::DevPtr<double> v_snap; // ... H1V: the velocity block of the state of the last lgh_qupdate (copy)
   lgh::DevPtr<double> force_e_q; // NE*ND*dim: F.1 as E-vector (3D)
   int fused_ftv_valid = 0, fused_f1_valid = 0;
   unsigned long qgen = 0; // counts lgh_qupdate / invalidations (lgh_quadrature_generation)
   lgh::DevPtr<int> dev_flags; // 8 device ints, one owner each: [0] / [2] "v differs from v_snap" of the current lgh_solve_energy (main /
                               // second stream), [1] "x differs from ones" of lgh_force_mult, [3] "mass table is not W[q]*s_e" (mass_data),
                               // [4] "an energy right-hand side was poisoned" (erhs_take_or_poison_k; read and cleared by lgh_get_dt_est),
                               // [5] "Jac0inv varies inside a zone" (jac0_compact_k, lgh_setup_rho0detj0)
   lgh::DevPtr<double> ones_l2; // L2V ones: the operator's own `one` (laghos_solver.cpp:170-171), allocated on first use
   int stress_store = 1; // lgh_qupdate_store_stress: 1 (default) = lgh_qupdate writes the nine stressJinvT planes; 0 = the stress stays in registers
   int stress_current = 0; // stressJinvT holds the stress of the current quadrature data (consumers refuse it otherwise)
   int fused_forces_off = 0; // lgh_set_fused_forces(ctx, 0): the update forms no force products (measurement / A-B)
   // scratch
   lgh::DevPtr<double> XE; // max(L2V, NE*ND*dim)
   lgh::DevPtr<double> YE; // NE*ND*dim
   lgh::DevPtr<double> cg_r, cg_z, cg_d0, cg_d1, cg_y; // max(N, L2V)
   lgh::DevPtr<double> partials; // 4 reduction slots of part_stride block partials each
   int part_stride = 0; // slot size: >= max #blocks of any reducing launch + kShards
   lgh::DevPtr<unsigned int> tickets;// 4 reduction slots of lgh::kTicketSlot counters (sharded tickets)
   lgh::DevPtr<lgh::CgScalars> cgs;
   lgh::DevPtr<double> scal; // small device scalar pool (16 doubles)
   unsigned long long look_token = 0; // counts the host looks that wait for a token in pinned memory (host_wait_token)

   // lockstep velocity CG (lgh_vcg.hip), allocated on first use
   lgh::DevPtr<lgh::VcgScalars> vcg_s;
   lgh::DevPtr<double> vcg_vec, vcg_partials;
   lgh::DevPtr<unsigned int> vcg_tickets;
   unsigned vcg_stride = 0;
   int vcg_last = 0;
   int vcg_grid = 0;     // persistent grid size of the K1 kernel (one resident wave)
   int b_h1_sym = 0, b_l2_sym = 0; // the 1-D H1 / L2 table is mirror symmetric, B[q,d] = B[Q-1-q, D-1-d] (to 1e-14: the round-off of its evaluation): kernels may hold half of it
   int ncu = 0;          // CUs of this context's device (0: not asked yet)
   std::unique_ptr<lgh::VcgAux> vcg_aux; // tables of the node kernel K2 (lgh_vcg.hpp VcgAux; built and dropped by lgh_vcg_tables.hip), allocated on first use

   lgh::Timers timers;
   std::unique_ptr<lgh::KTime> ktime;
   int cg_last_iters[2][3] = {{0, 0, 0}, {0, 0, 0}}; // iteration count of the previous solve per (space, component)
   std::unique_ptr<lgh::Comm> comm;
   int nranks = 1, rank = 0;
   int multi = 0;        // 1: run the multi-rank code path (nranks > 1, or LGH_FORCE_MULTI=1 for testing on one GPU)
   lgh::DevPtr<unsigned long long> q_trace_dev; // debug (LGH_Q_TRACE): stage stamps of the quadrature update's workgroups, NE records
   int q_trace_n = 0, q_trace_calls = 0;
   std::unique_ptr<lgh::MeshOrder> order; // (lgh_order.hip)
   unsigned long mass_gen = 0; // counts changes of the mass data / Jacobi diagonal (the velocity solve keeps copies in its own numbering)
   lgh::DevPtr<double> me_fac; // 1D: NE * L1D^2, Cholesky factors of the zone mass matrices Me(z) of the energy solve (lgh_1d.hip)
   int setup_done = 0;   // lgh_setup_rho0detj0 has run: rho0DetJ0w holds the masses of the points (lgh_diagnostics refuses before)
   lgh::DevPtr<double> diag_dev; // lgh_diagnostics (lgh_diag.hip): 32 doubles of folded values, then the 17 zone arrays; allocated on first use
   lgh::DevPtr<char> prof_dev; // lgh_profile (lgh_profile.hip): accumulator words, flags, maxima and the packed rows for prof_rows rows;
   int prof_rows = 0;        // allocated at the first call, regrown only when nbins grows
   lgh::DevPtr<char> map_dev;  // lgh_map (lgh_map.hip): the same for map_rows rows of eight sum columns; regrown only when the cell count grows
   int map_rows = 0;
   lgh::DevPtr<int> faces_dev; // lgh_sample_faces (lgh_faces.hip): the device copy of the caller's face list, 2 * faces_cap ints; regrown only when a longer list comes
   int faces_cap = 0;
   lgh::DevPtr<char> loads_dev; // lgh_loads (lgh_loads.hip): the same for loads_rows = LGH_LOADS_MAX_ROWS rows, allocated at the first call
   int loads_rows = 0;
   lgh::DevPtr<int> loads_faces; // ... and the device copy of the caller's list, 3 * loads_cap ints; regrown only when a longer list comes
   int loads_cap = 0;
   lgh::DevPtr<long long> contour_dev; // lgh_contour (lgh_contour.hip): counts, skipped counts and offsets of contour_cap workgroups (3 n + 2 words); regrown only when the grid grows
   int contour_cap = 0;
   lgh::DevPtr<unsigned long long> fp_dev; // lgh_vec_fingerprint (lgh_fingerprint.hip): the two words of the result and the workgroups' partial words, allocated on first use
   std::vector<std::unique_ptr<lgh::GaugeSet>> gauges; // lgh_gauges_create (lgh_gauges.hip): the handle is the index; a destroyed set leaves its slot empty
};

namespace lgh
{

// ---- the orders: THE table of the kernel ids, (dim << 8) | (D1D << 4) | Q1D with dim 1, 2, 3 and the five rows below -----------
// The (order_v, order_e) pairs of the reference's 2D / 3D tables (assembly.cpp:534-548, :944-956; laghos_solver.cpp:1387-1396);
// Q5Q4 is an extension the reference does not instantiate.  D, Q, L: the 1-D sizes of the H1 basis, the quadrature rule and the
// L2 basis (L = D - 1: lgh_create).  Every order-templated kernel family picks its instantiation through visit_order; the
// dimension stays a runtime branch inside the callable.
template <int V> using IC = std::integral_constant<int, V>;
template <class F, class G> auto order_row(const int kid, F &&f, G &&none)
{
   switch (kid & 0xFF)
   {
      case 0x22: return f(IC<2>(), IC<2>(), IC<1>());  // Q1Q0
      case 0x34: return f(IC<3>(), IC<4>(), IC<2>());  // Q2Q1
      case 0x46: return f(IC<4>(), IC<6>(), IC<3>());  // Q3Q2
      case 0x58: return f(IC<5>(), IC<8>(), IC<4>());  // Q4Q3
      case 0x6A: return f(IC<6>(), IC<10>(), IC<5>()); // Q5Q4
   }
   return none();
}
inline int unknown_kernel(const int kid)
{
   set_error("Unknown kernel 0x%x", kid);
   return LGH_ERR_UNSUPPORTED;
}
// f(IC<D>, IC<Q>, IC<L>) for the order of kernel id `kid`: what f returns, an LGH_* status; any other id is the one failure
template <class F> int visit_order(const int kid, F &&f) { return order_row(kid, f, [kid] { return unknown_kernel(kid); }); }
// ... of a 2D / 3D context: a 1D context has kernels of its own (lgh_1d.hip), to the families here its id is unknown as well
template <class F> int visit_order_2d3d(const lgh_ctx *c, F &&f) { return c->dim == 1 ? unknown_kernel(c->kid) : visit_order(c->kid, f); }
// one of the fifteen ids (launches nothing, sets no error)
inline bool order_supported(const int kid)
{
   return kid >= 0x100 && kid < 0x400 && order_row(kid, [](auto, auto, auto) { return true; }, [] { return false; });
}
// zones per workgroup of the kernels whose threads are the (qx, qy) columns of their zones: the force kernels, the column
// forms of the mass operators and of K1, the 2-D point form of the quadrature update
constexpr int zones_per_wg(const int Q) { return (256 / (Q * Q)) > 0 ? (256 / (Q * Q)) : 1; }

// ---- wave / block reductions (wave64, DPP) ----------------------------------
// Workgroups here are Q*Q*NEB threads, not always a multiple of 64, so the last wave may be partial (`nact` live
// lanes, wave-uniform).  The reduction runs on the DPP data path: row_shr 1, 2, 4, 8 inside the rows of 16 lanes,
// then row_bcast 15 / 31 across them - 3 instructions per step instead of the ~13 of a ds_bpermute shuffle with
// its lane guard (these trees are ~80 of the QUpdate's ~2100 vector instructions per wave, and the tail of every
// CG kernel).  A lane whose source lies outside its row, in a masked row or in the dead part of a partial wave takes
// the neutral `old` operand instead, so no guard is needed; the total forms in the last live lane and is read
// from there into every lane.  Fixed order: bit-reproducible.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64(const double old, const double src)
{
   const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(src), CTRL, ROW_MASK, 0xF, false);
   const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(src), CTRL, ROW_MASK, 0xF, false);
   return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_bcast_f64(const double v, const int src_lane /* uniform */)
{
   const int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane);
   const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
   return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum(double v, const int lane, const int nact)
{
   (void)lane;
   v += dpp_f64<0x111, 0xF>(0.0, v); // row_shr:1
   v += dpp_f64<0x112, 0xF>(0.0, v); // row_shr:2
   v += dpp_f64<0x114, 0xF>(0.0, v); // row_shr:4
   v += dpp_f64<0x118, 0xF>(0.0, v); // row_shr:8
   v += dpp_f64<0x142, 0xA>(0.0, v); // row_bcast:15 into rows 1 and 3
   v += dpp_f64<0x143, 0xC>(0.0, v); // row_bcast:31 into rows 2 and 3
   return wave_bcast_f64(v, nact - 1);
}
__device__ __forceinline__ double wave_min(double v, const int lane, const int nact)
{
   (void)lane;
   v = fmin(v, dpp_f64<0x111, 0xF>(v, v));
   v = fmin(v, dpp_f64<0x112, 0xF>(v, v));
   v = fmin(v, dpp_f64<0x114, 0xF>(v, v));
   v = fmin(v, dpp_f64<0x118, 0xF>(v, v));
   v = fmin(v, dpp_f64<0x142, 0xA>(v, v));
   v = fmin(v, dpp_f64<0x143, 0xC>(v, v));
   return wave_bcast_f64(v, nact - 1);
}

// a value that is the same in every lane, moved to scalar registers (an FMA can take it as its SGPR operand)
__device__ __forceinline__ double uniform_f64(const double v)
{
   const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
   const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
   return __hiloint2double(hi, lo);
}

// Sum over the block; result valid in thread 0.  `red` = LDS scratch of >= 16 doubles.
__device__ __forceinline__ double block_sum(double v, double *red)
{
   const int tid = threadIdx.x + blockDim.x * (threadIdx.y + blockDim.y * threadIdx.z);
   const int nthr = blockDim.x * blockDim.y * blockDim.z;
   const int lane = tid & 63, wid = tid >> 6, nw = (nthr + 63) >> 6;
   const int nact = min(64, nthr - (wid << 6));
   v = wave_sum(v, lane, nact);
   __syncthreads();
   if (lane == 0) { red[wid] = v; }
   __syncthreads();
   double s = 0.0;
   if (tid == 0)
   {
      for (int w = 0; w < nw; w++) { s += red[w]; }
   }
   return s;
}
// Three sums at once (the three velocity components of the lockstep CG): one pair of barriers instead of three
// pairs plus separators; the same wave sums added in the same order as three block_sum calls - the same bits.
// `red` = LDS scratch of >= 48 doubles; results valid in thread 0.
__device__ __forceinline__ void block_sum3(const double v0, const double v1, const double v2, double *red, double out[3])
{
   const int tid = threadIdx.x + blockDim.x * (threadIdx.y + blockDim.y * threadIdx.z);
   const int nthr = blockDim.x * blockDim.y * blockDim.z;
   const int lane = tid & 63, wid = tid >> 6, nw = (nthr + 63) >> 6;
   const int nact = min(64, nthr - (wid << 6));
   const double a0 = wave_sum(v0, lane, nact), a1 = wave_sum(v1, lane, nact), a2 = wave_sum(v2, lane, nact);
   __syncthreads();
   if (lane == 0)
   {
      red[3 * wid + 0] = a0;
      red[3 * wid + 1] = a1;
      red[3 * wid + 2] = a2;
   }
   __syncthreads();
   out[0] = out[1] = out[2] = 0.0;
   if (tid == 0)
   {
      for (int w = 0; w < nw; w++)
      {
         out[0] += red[3 * w + 0];
         out[1] += red[3 * w + 1];
         out[2] += red[3 * w + 2];
      }
   }
   __syncthreads(); // red is free again (the grid reductions that follow reuse it)
}
__device__ __forceinline__ double block_min(double v, double *red)
{
   const int tid = threadIdx.x + blockDim.x * (threadIdx.y + blockDim.y * threadIdx.z);
   const int nthr = blockDim.x * blockDim.y * blockDim.z;
   const int lane = tid & 63, wid = tid >> 6, nw = (nthr + 63) >> 6;
   const int nact = min(64, nthr - (wid << 6));
   v = wave_min(v, lane, nact);
   __syncthreads();
   if (lane == 0) { red[wid] = v; }
   __syncthreads();
   double s = v;
   if (tid == 0)
   {
      s = red[0];
      for (int w = 1; w < nw; w++) { s = fmin(s, red[w]); }
   }
   return s;
}

// ---- deterministic grid-wide reductions without a second launch -----------------
// Every block publishes its partial with an agent-scope (write-through) atomic
// store, drains, and takes a ticket; the last block to arrive re-reads all
// partials with agent-scope loads in block order (fixed summation tree ->
// bit-reproducible).  Both sides use 8-byte agent atomics (MI355X guide,
// Guideline 16), so no L2 write-back fence is needed.
//
// One device-scope counter serialises at ~12 ns per arrival (guide: "fanin"), so
// thousands of blocks on ONE counter cost tens of microseconds - measured here as
// the whole duration of the first CG kernels.  The ticket is therefore sharded:
// block b arrives on shard b % kShards (one cache line each); the last arriver of
// a shard arrives on the top counter; the last of those owns the final fold.
// Counters are reset by their last arrivers, so a slot is reusable by the next
// launch on the stream.
//
// Memory ordering.  The partial is published with a relaxed agent-scope 8-byte atomic store (sc1:
// write-through, nothing left in this XCD's L2), then `s_waitcnt vmcnt(0)` completes it before the ticket
// is taken; the last arriver reads the partials with relaxed agent-scope 8-byte atomic loads (sc1: served
// past the L1, and never stale in an L2 - the L2s snoop write-through traffic).  That is the "8-byte agent
// atomics on both sides" form of MI355X_MICROARCH.md / cdna_hip_programming.md Guideline 16; it holds by
// the behaviour of gfx9-family vmcnt (which counts stores) and sc1, not by the C++ memory model.  The
// model-conforming form - a RELEASE fetch_add by the producers and an ACQUIRE one by the last block - costs
// an L2 write-back (buffer_wbl2) per workgroup on gfx950, microseconds for each of the thousands of blocks
// of the node kernels whose vector stores are still dirty in the L2; it is not used.  The guard below keeps
// this file from being built for a target where the argument does not hold (vmcnt does not count stores from
// gfx10 on).
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__) && !defined(__gfx90a__)
#error "lgh_common.hpp: the grid reductions rely on gfx9-family vmcnt / sc1 semantics (see comment)"
#endif
constexpr unsigned kShards = 64;
constexpr unsigned kTicketStride = 32;                               // uints: 128 B apart
constexpr unsigned kTicketSlot = (kShards + 1) * kTicketStride;      // uints per reduction slot

// Returns true in ALL threads of the globally last block; `total` is then valid in
// thread 0.  `partials` must hold gridsize + kShards doubles: block partials, then
// (at offset `shard_off`) one folded partial per shard.  Fold order is fixed:
// shard s folds blocks s, s+kShards, ... through the block tree, the last block
// folds the shard sums in shard order -> bit-reproducible, and the serial tail
// after the last arrival is two memory round trips, not gridsize/blocksize.
template <bool IS_MIN>
__device__ __forceinline__ bool grid_reduce_last_block(double block_partial /* thread 0 */,
                                                       double *partials, const unsigned shard_off,
                                                       unsigned int *ticket, double *red, double &total)
{
   const int tid = threadIdx.x + blockDim.x * (threadIdx.y + blockDim.y * threadIdx.z);
   const int nthr = blockDim.x * blockDim.y * blockDim.z;
   const unsigned int nblk = gridDim.x * gridDim.y * gridDim.z;
   const unsigned int bid = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
   const unsigned s = bid % kShards;
   const unsigned cnt = nblk / kShards + ((s < nblk % kShards) ? 1u : 0u);
   const unsigned nsh = nblk < kShards ? nblk : kShards;
   unsigned int *t1 = ticket + s * kTicketStride;
   unsigned int *t2 = ticket + kShards * kTicketStride;
   const double ident = IS_MIN ? INFINITY : 0.0;
   __shared__ unsigned int s_flag;
   if (tid == 0)
   {
      __hip_atomic_store(&partials[bid], block_partial, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const unsigned a = __hip_atomic_fetch_add(t1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_flag = (a == cnt - 1) ? 1u : 0u;
   }
   __syncthreads();
   if (!s_flag) { return false; }
   // last arriver of shard s: fold the shard's block partials
   double v = ident;
   for (unsigned int i = tid; i < cnt; i += nthr)
   {
      const double p = __hip_atomic_load(&partials[s + kShards * i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      v = IS_MIN ? fmin(v, p) : v + p;
   }
   const double ssum = IS_MIN ? block_min(v, red) : block_sum(v, red);
   __syncthreads();
   if (tid == 0)
   {
      __hip_atomic_store(&partials[shard_off + s], ssum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(t1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned b = __hip_atomic_fetch_add(t2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_flag = (b == nsh - 1) ? 1u : 0u;
      if (s_flag) { __hip_atomic_store(t2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
   }
   __syncthreads();
   if (!s_flag) { return false; }
   v = ident;
   for (unsigned int i = tid; i < nsh; i += nthr)
   {
      const double p = __hip_atomic_load(&partials[shard_off + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      v = IS_MIN ? fmin(v, p) : v + p;
   }
   total = IS_MIN ? block_min(v, red) : block_sum(v, red);
   return true;
}
// The shard sums live right after the block partials of a slot: every reduction
// slot of the context is part_stride + kShards doubles (lgh_create).
__device__ __forceinline__ bool grid_sum_last_block(double bp, double *partials, unsigned int *ticket,
                                                    double *red, double &total)
{
   const unsigned nblk = gridDim.x * gridDim.y * gridDim.z;
   return grid_reduce_last_block<false>(bp, partials, nblk, ticket, red, total);
}
__device__ __forceinline__ bool grid_min_last_block(double bp, double *partials, unsigned int *ticket,
                                                    double *red, double &total)
{
   const unsigned nblk = gridDim.x * gridDim.y * gridDim.z;
   return grid_reduce_last_block<true>(bp, partials, nblk, ticket, red, total);
}

// block index -> work chunk so that blocks resident on one XCD (observed:
// block b runs on XCD b % 8) sweep a contiguous range: neighbouring elements
// share H1 nodes, so their gathers hit the same XCD-private L2.
__device__ __forceinline__ int xcd_swizzle(const int b, const int nblocks)
{
   const int per = nblocks >> 3; // blocks per XCD (floor)
   const int main = per << 3;
   if (b >= main) { return b; } // tail stays in place
   return (b & 7) * per + (b >> 3);
}

inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }
template <typename T> inline T ipow(T b, int e) { T r = 1; for (int i = 0; i < e; i++) { r *= b; } return r; } // b to the power e >= 0
inline int grid_for(long n) { return (int)std::min<long>(std::max<long>((n + 255) / 256, 1), 2048); } // workgroups of 256 for a grid-stride loop over n

// ---- lgh_order.hip
int mesh_order_build(lgh_ctx *c, const int *map_host);
// the internal order when it differs from the caller's, else nullptr
inline const MeshOrder *mesh_order(const lgh_ctx *c)
{
   const MeshOrder *o = c->order.get();
   return (o && !o->identity) ? o : nullptr;
}
int order_gather_nodes(lgh_ctx *c, const double *in, double *out, int ncomp);  // out[k N + m] = in[k N + ncaller[m]]
int order_scatter_nodes(lgh_ctx *c, const double *in, double *out, int ncomp); // out[k N + ncaller[m]] = in[k N + m]
int order_gather_bytes(lgh_ctx *c, const uint8_t *in, uint8_t *out);
int order_zone_blocks(lgh_ctx *c, const double *in, double *out, int per, bool to_caller); // blocks of `per` doubles per zone

// ---- lgh_force.hip, lgh_mass.hip, lgh_qupdate.hip, lgh_qsetup.hip: the operators and the quadrature data
int force_mult_E(lgh_ctx *c, const double *sJit, const double *xE, double *yE);
int force_mult_t_L(lgh_ctx *c, const double *sJit, const double *v_h1, double *y_l2, const int *guard = nullptr);
int force_mult_t_E(lgh_ctx *c, const double *sJit, const double *vE, double *y_l2);
int h1_transpose_gather(lgh_ctx *c, int ncomp, const double *YE, double *yL);
int mass_apply_h1(lgh_ctx *c, const double *x, double *y, bool eliminate);
int mass_apply_l2(lgh_ctx *c, const double *x, double *y);
int mass_apply_E(lgh_ctx *c, int space, const double *xE, double *yE);
int mass_assemble_diag(lgh_ctx *c);
// the quadrature data of the mass operators as (table, element stride in doubles, per-element factor): value(q, e) = Dq[q + dqs e] * Se[e]
int mass_data(lgh_ctx *c, const double **Dq, int *dqs, const double **Se);
int l2_mass_form(lgh_ctx *c, int *form, int *compact); // kernel of the L2 mass apply: 2 Kronecker, 1 plane, 0 column (lgh_l2_mass_form)
int qupdate_form(lgh_ctx *c); // 1: row form of the 3D quadrature update (lgh_qrows.hpp), 0: point form
int qupdate(lgh_ctx *c, const double *S);
int setup_rho0detj0(lgh_ctx *c, const double *x0, const double *rho0_l2, const double *rho0_q,
                    double *volume);
int interp_energy(lgh_ctx *c, int which, const double *vec, double *result);
int tg_source_2d(lgh_ctx *c, const double *S, double *out);
int test_eig(lgh_ctx *c, int dim, int n, const double *A, double *lambda, double *vec);
int test_singular(lgh_ctx *c, int dim, int n, const double *A, double *sv);
int test_sqrt(lgh_ctx *c, int n, const double *x, double *y);
constexpr int kDtSlots = 256, kDtSlotStride = 16; // doubles; slot s at dt_est_dev[kDtSlotStride * (1 + s)]
// dt_est_dev[kDtHint], one of the padding doubles behind the estimate: the hint word of the row-form update.  It only ever
// holds +inf, the estimate itself (lgh_set_dt_est) or a value that was also deposited in a slot, so the folded estimate is
// never above it; a wavefront whose candidates provably lie above it skips them (qpoint_body).  The fold resets it to +inf.
constexpr int kDtHint = 1;
enum { kQDiscardDt = 1, kQDiscardF1 = 2 }; // lgh_ctx::q_discard

// ---- lgh_vcg*.hip: the lockstep velocity CG and its test hooks (lgh_vcg_hooks.hip)
int vcg_solve(lgh_ctx *c, double *B, double *X, double rel_tol, int max_iter, int iters[3],
              const double *force_E = nullptr);
bool vcg_fused_init_ok(const lgh_ctx *c);
bool vcg_available(const lgh_ctx *c);
int vcg_k1_form(lgh_ctx *c); // 0 column, 2 plane, 3 matrix cores, 4 slab, -1 none
bool vcg_lockstep_ready(const lgh_ctx *c); // the velocity solve of this context exchanges accumulator words and packs its halo itself
constexpr int kYePad = 16; // doubles behind every Y_E plane of the CG; the first one (slot NE*ND) stays 0.0
// tables of the node kernel K2 (lgh_vcg_tables.hip)
int partition_nodes_by_cost(lgh_ctx *c, int W, DevPtr<int> &out, const std::vector<int> *valence = nullptr);
int make_ellz(lgh_ctx *c, DevPtr<unsigned> &out, const int *ell = nullptr, int deg = 0);
int make_essbits(lgh_ctx *c, DevPtr<uint8_t> &out);
void vcg_free(lgh_ctx *c); // drops the tables of K2: the next solve builds them again (a communicator has changed)
int vcg_test_merged_faces(lgh_ctx *c, unsigned char *mask, long *n_merged); // lgh_test_vcg_merged_faces
int vcg_layout_stats(lgh_ctx *c, long out[4]); // lgh_vcg_layout_stats
int vcg_test_k1(lgh_ctx *c, const double *r, const double *d_old, const double rz[3], const double rz_prev[3], int first,
                double *YE_out, double den_out[3]); // one launch of K1 (test hook)
int vcg_test_k2(lgh_ctx *c, int it, const double *YE_in, double *r, double *d, double *x, const double den[3], const double rz[3],
                const double rz_prev[3], const double alpha_prev[3], double rz_out[3], int *deferred_x); // one launch of K2 (test hook)
int vcg_test_exact_sum(lgh_ctx *c, int mode, long n, int G, int E, const double *scale, const double *v, const long long *w_in,
                       long long *w_out, double *d_out, int *i_out); // the exact accumulators of lgh_vcg.hpp on their own (test hook)

// ---- lgh_scg.hip, lgh_energy.hip: the scalar CG and the energy solve
int cg_solve(lgh_ctx *c, int space, const double *b, double *x, double rel_tol, int max_iter,
             int *iters, bool x_is_zero);
int cg_l2_begin(lgh_ctx *c, const double *b, double *x, double rel_tol, int max_iter);
int cg_l2_end(lgh_ctx *c, int *iters);
// Completes the energy solve that lgh_solve_energy_begin enqueued on the second stream - its host looks and, if it has not
// converged, its further iterations - from INSIDE the velocity solve, while the main stream still has the velocity
// solve's first chunk of iterations in front of it: lgh_solve_energy_end then only joins the streams (round 6: the looks of
// the energy solve used to sit between the end of the velocity solve and the RK combination, with the GPU idle).
int energy_overlap_poll(lgh_ctx *c);
// Energy CG in lockstep with the velocity CG (several ranks, one stream, one communicator; round 6).  Its two dot products
// per iteration ride on exchanges the velocity iteration makes anyway: (d, M d) as a fourth scalar behind the halo messages
// (VcgScalars::den_e), (r, r) as a double in word kLsWord of the accumulator-word exchange.  No exchange of its own.
constexpr int kLsWord = 50;             // (a padding word of an accumulator set: lgh_vcg.hpp checks it is one)
constexpr int kLsWordsPerSet = 56;      // = kLimbWords (checked there): stride of the peers' sets
struct LockstepWords { const long long *own; const long long *peers; int n_peers, before; }; // before: peers of lower rank
bool l2_lockstep_possible(lgh_ctx *c);  // the L2 apply runs as the Kronecker kernel with the fused update (lgh_scg.hip)
int cg_l2_begin_lockstep(lgh_ctx *c, const double *b, double *x, double rel_tol, int max_iter); // set-up + initial residual, no iteration
int l2_lockstep_limit(lgh_ctx *c);      // iterations worth interleaving: the previous solve's count
int l2_lockstep_apply(lgh_ctx *c, int it, const LockstepWords &prev, double *den_mirror);
int l2_lockstep_update(lgh_ctx *c, int it, const double *den_src, long long *word_out);
int l2_lockstep_fold(lgh_ctx *c, int it, const LockstepWords &last); // commits the outcome of iteration it (what the next apply would)
int cg_l2_end_lockstep(lgh_ctx *c, int *iters); // the rest of the solve on its own (exchanges of its own), the host look

// ---- lgh_comm.hip: several ranks
// multi-rank: flags / list of the nodes shared with other ranks (nullptr / 0 without neighbours)
void comm_shared_nodes(const lgh_ctx *c, const uint8_t **hmask, const int **sh_node, int *n_shared);
int comm_ranks_before(const lgh_ctx *c); // neighbours whose rank is lower than this rank's
// packed: the caller's own kernel has already put the node values / scalars into the send buffer of the main channel
// (HaloPackTables: what it needs for that) - the exchange then starts without a pack kernel
struct HaloNodeAlias { const int *nodes, *sh_node; }; // the exchange's node lists in another numbering of the SAME nodes (the velocity solve's own)
int halo_sum(lgh_ctx *c, double *v, int ncomp, double *extra = nullptr, int nextra = 0, bool packed = false, const HaloNodeAlias *alias = nullptr);
void comm_node_lists(const lgh_ctx *c, const int **nodes, int *total, const int **sh_node, int *n_shared);
struct HaloPackTables
{
   const int *sh_off, *sh_src; // CSR over the unique shared nodes: entries of the concatenated neighbour lists (-1: own value)
   const int *pos, *cnt;       // entry j -> offset of its node value in the buffer (component c at + c * cnt[j])
   const int *base, *ncnt;     // neighbour k -> start of its block, nodes in it (scalars sit behind ncomp * ncnt[k] values)
   double *sbuf;
   int n_nbr;
};
bool comm_pack_tables(const lgh_ctx *c, HaloPackTables *t); // false: no neighbours / no tables
bool halo_can_piggyback(const lgh_ctx *c);
bool comm_second_channel(const lgh_ctx *c); // reductions may run on the context's second stream as well
// Exact all-reduce of integer accumulator words (lgh_vcg.hpp: the (r, z) of the lockstep solve) in ONE message round and
// without a kernel: every rank sends its `nwords` 64-bit words to every peer straight out of the accumulators and
// receives theirs into its peer buffer (comm_word_peers: block k = neighbour k); whoever folds the sum adds own and
// peer words - integers, so every rank gets the same bits whatever the arrival order.  All-pairs partitions only.
int exchange_words(lgh_ctx *c, const long long *src, int nwords);
int comm_word_peers(lgh_ctx *c, int nwords, const long long **peers, int *n_peers); // (allocates the peer buffer on first use)
int allreduce_dev_n(lgh_ctx *c, double *dev, long count, int op); // any count: in pieces of what the transport takes at a time
int allreduce_dev(lgh_ctx *c, double *dev, int count, int op, bool packed = false); // packed: as halo_sum (sums that travel as one exchange with every peer only)

// ---- lgh_vec.hip
int vec_set(lgh_ctx *c, double *y, double a, long n);
int vec_axpby(lgh_ctx *c, double *z, double a, const double *x, double b, const double *y, long n);
int vec_axpby_pair(lgh_ctx *c, double *z1, double a1, const double *x1, double b1, double *z2, double a2, const double *x2, double b2,
                   const double *y, long n);
int vec_neg_inplace(lgh_ctx *c, double *y, long n);
int vec_zero_list(lgh_ctx *c, double *y, const int *list, int n);
int vec_dot(lgh_ctx *c, const double *x, const double *y, const double *w, long n, double *dev_out);

// ---- lgh_api.hip
// Host look without a copy kernel and without the wake-up latency of a blocking stream synchronisation: the one-thread
// kernel that finishes the scalars writes them, then `token`, into pinned host memory (a.k.a. host_pinned_dev); the host
// spins on the token word (falls back to hipStreamSynchronize after a while; LGH_SPIN=0: always synchronise).
int host_wait_token(lgh_ctx *c, volatile unsigned long long *word, unsigned long long token);
int stress_on_hand(lgh_ctx *c, const char *who); // LGH_OK: the stress of the current quadrature data is in memory
int no_1d(const lgh_ctx *c, const char *who);   // LGH_OK: not a 1D context (entry points with no 1D form refuse one)

// ---- lgh_context.hip
int create_common(const lgh_config *cfg, lgh_ctx *c, std::vector<int> &t_off, std::vector<int> &t_idx); // what create_1d and the 2D/3D create share

// ---- lgh_1d.hip: the 1D path (the entry points send a context with dim == 1 there; the 2D/3D kernels never see one)
int create_1d(const lgh_config *cfg, lgh_ctx *c);
int setup_1d(lgh_ctx *c, const double *x0, const double *rho0_l2, const double *rho0_q, double *volume);
int mass_changed_1d(lgh_ctx *c); // Jacobi diagonal and zone mass factors from the current mass data
int force_mult_1d(lgh_ctx *c, const double *x_l2, double *y_h1);
int force_mult_t_1d(lgh_ctx *c, const double *v_h1, double *y_l2);
int mass_apply_1d(lgh_ctx *c, int space, const double *x, double *y, bool eliminate);
int l2_solve_local_1d(lgh_ctx *c, const double *b, double *x);
int cg_1d(lgh_ctx *c, int space, const double *b, double *x, double rel_tol, int max_iter, int *iters, bool x_is_zero);
int qupdate_1d(lgh_ctx *c, const double *S);
int solve_velocity_1d(lgh_ctx *c, const double *ones, double *dv, double *rhs, double rel_tol, int max_iter, int *h1_iters);
int solve_energy_1d(lgh_ctx *c, const double *v_h1, double *de, double *e_rhs, const double *e_source, int *l2_iters);
int density_1d(lgh_ctx *c, const double *x_h1, double *rho_l2);
int energy_1d(lgh_ctx *c, int which, const double *vec, double *result);
int sedov_density_error_1d(lgh_ctx *c, const double *x_h1, const double *rho_l2, const double par[21], double t,
                           const double origin[3], int n1d, const double *weights, const double *B_h1, const double *G_h1,
                           const double *B_l2, double *err2);

// ---- lgh_timing.hip
// bracket one launch of kernel `id` with an event pair when sampling is on
inline void kt_begin(lgh_ctx *c, int id)
{
   KTime *k = c->ktime.get();
   if (k && k->which == id && k->n < k->max) { (void)hipEventRecord(k->ev[2 * k->n], c->stream); }
}
inline void kt_end(lgh_ctx *c, int id)
{
   KTime *k = c->ktime.get();
   if (k && k->which == id && k->n < k->max) { (void)hipEventRecord(k->ev[2 * k->n + 1], c->stream); k->n++; }
}

// one sample around a scope: closed on every way out (error returns included)
struct KtScope
{
   lgh_ctx *c;
   int id;
   KtScope(lgh_ctx *c_, int id_) : c(c_), id(id_) { kt_begin(c, id); }
   ~KtScope() { kt_end(c, id); }
   KtScope(const KtScope &) = delete;
   KtScope &operator=(const KtScope &) = delete;
};

void timer_start(lgh_ctx *c);
void timer_stop(lgh_ctx *c, int which);
void roctx_enable(); // (lgh_create, with LGH_ROCTX=1)
// roctx range around a region of the host timeline, named after the reference's Caliper regions
// (/root/reference/laghos_solver.cpp:353-356 "SolveVelocity-ForcePA", :387-390 "SolveVelocity-CGVMass", :472-475
// "SolveEnergy-ForcePA", :480-483 "SolveEnergy-CGEMass", :1358 "QUpdate-UpdateQuadratureData"): a `rocprofv3 --marker-trace
// --kernel-trace` run then attributes the kernels the way the reference's own profile does.  LGH_ROCTX=1 switches them on
// (librocprofiler-sdk-roctx / libroctx64 resolved with dlopen: no link dependency, nothing happens without the variable).
struct RoctxRange
{
   bool on;
   explicit RoctxRange(const char *name);
   ~RoctxRange();
   RoctxRange(const RoctxRange &) = delete;
   RoctxRange &operator=(const RoctxRange &) = delete;
};

} // namespace lgh
