// laghos_solver.hpp — LagrangianHydroOperator, QUpdate, TimingData and the ODE
// solvers with the reference's API surface (/root/reference/laghos_solver.hpp:36-255),
// re-expressed over the C ABI of the HIP library.
#pragma once
#include <memory>

#include "fem.hpp"
#include "laghos_assembly.hpp"

namespace laghos
{

// The blocks of lgh_sample_derived for NP points, [detJ | grad v | div v | vorticity | sound speed], from where they start
// (the vorticity has 3 components in 3D, 1 in 2D, none in 1D)
template <class T> struct DerivedBlocks
{
   T *detj, *grad, *div, *vort, *cs, *end;
   DerivedBlocks(T *p, int dim, long NP)
      : detj(p), grad(detj + NP), div(grad + (long)dim * dim * NP), vort(div + NP), cs(vort + (dim == 3 ? 3 : (dim == 2 ? 1 : 0)) * NP), end(cs + NP) {}
};

namespace hydrodynamics
{

// laghos_solver.hpp:39-56; times come from HIP events inside the library.
struct TimingData
{
   double sw_cgH1 = 0, sw_cgL2 = 0, sw_force = 0, sw_qdata = 0;
   long L2dof = 0, H1iter = 0, L2iter = 0, quad_tstep = 0;
};

// laghos_solver.hpp:58-93
class QUpdate
{
   lgh_ctx *ctx;

public:
   explicit QUpdate(lgh_ctx *c) : ctx(c) {}
   void UpdateQuadratureData(const Vector &S, QuadratureData &) { LGH_VERIFY(lgh_qupdate(ctx, S.Read())); }
};

// Given a state (x, v, e) evaluates the slopes (dx_dt, dv_dt, de_dt)
// (laghos_solver.hpp:97-205, laghos_solver.cpp:104-540; PA branch, dim >= 2).
class LagrangianHydroOperator
{
protected:
   const Discretization &disc;
   lgh_ctx *ctx;
   const int dim, NE;
   const int H1Vsize, L2Vsize;
   const long H1GTVSize, L2GTVSize;
   const double cg_rel_tol;
   const int cg_max_iter;
   std::unique_ptr<QuadratureData> qdata;
   mutable bool qdata_is_current;
   mutable unsigned long qdata_gen = 0; // lgh_quadrature_generation() after the operator's last update
   std::unique_ptr<ForcePAOperator> ForcePA;
   std::unique_ptr<MassPAOperator> VMassPA, EMassPA;
   std::unique_ptr<QUpdate> qupdate;
   mutable Vector one, rhs, e_rhs, B;
   Vector accel_src;        // source_type == 2 (problem 7 gravity, laghos_solver.cpp:340-347)
   mutable Vector e_source; // source_type == 1 (2D Taylor-Green, laghos_solver.cpp:448-467), else empty
   int source_type = 0;
   mutable TimingData timer;
   double volume;

public:
   // nccl_id: 128-byte unique id for multi-rank runs (nullptr when nranks == 1)
   LagrangianHydroOperator(const Discretization &disc, const std::vector<double> &S0,
                           const std::vector<double> &rho0_l2, const std::vector<double> &gamma,
                           const std::vector<double> &rho0_q, double cfl, double cgt, int cgiter,
                           int device, const char *nccl_id);
   ~LagrangianHydroOperator();

   int Size() const { return 2 * H1Vsize + L2Vsize; }
   int H1VSize() const { return H1Vsize; }
   int L2VSize() const { return L2Vsize; }
   // Solve for dx_dt, dv_dt and de_dt (laghos_solver.cpp:308-327)
   void Mult(const Vector &S, Vector &dS_dt) const;
   void SolveVelocity(const Vector &S, Vector &dS_dt) const;
   void SolveEnergy(const Vector &S, const Vector &v, Vector &dS_dt) const;
   void UpdateMesh(const Vector &) const {} // nodes alias S.x: nothing to move
   void UpdateQuadratureData(const Vector &S) const;
   // Calls UpdateQuadratureData (laghos_solver.cpp:527-535); all-reduce MIN
   double GetTimeStepEstimate(const Vector &S) const;
   void ResetTimeStepEstimate() const;
   // (laghos_solver.hpp:193) - the force products lgh_qupdate formed with the stale data are discarded with it
   void ResetQuadratureData() const { qdata_is_current = false; LGH_VERIFY(lgh_reset_quadrature_data(ctx)); }
   double InternalEnergy(const Vector &S) const;
   double KineticEnergy(const Vector &S) const;
   double ENorm(const Vector &S) const; // ||e||_2, all-reduced (laghos.cpp:794-795)
   // zone-local L2 projection of the density on the current mesh (laghos_solver.cpp:542-563)
   void ComputeDensity(const Vector &S, Vector &rho) const;
   // sqrt of the integral of (rho_exact - rho)^2 against the exact Sedov solution `par` at time t,
   // error rule of order err_order (laghos.cpp:1007-1086); all-reduced
   double SedovDensityError(const Vector &S, const Vector &rho, const double par[21], double t,
                            const double origin[3], int err_order) const;
   // The fields of S and the density rho on the lattice of R + 1 points per direction in every zone (lgh_sample_fields;
   // stands in for the grid-function evaluation behind the reference's data collections, laghos.cpp:691-701, :845-871):
   // out = [x | v | e | rho | p] in blocks of dim, dim, 1, 1, 1 times NE (R+1)^dim values, zones in the caller's order
   // (out is sized anew when it is smaller than that; a larger one keeps what lies behind the blocks).
   // Asynchronous on the context's stream; the quadrature data is not touched.
   void SampleFields(const Vector &S, const Vector &rho, int R, Vector &out) const;
   long SamplePoints(int R) const; // NE (R+1)^dim
   // The derived fields of S on the same lattice (lgh_sample_derived).  With NP = SamplePoints(R) and nv = 0, 1, 3 vorticity
   // components in 1D, 2D, 3D, out holds from `offset` on, whatever the mask:
   //    [detJ | grad v | div v | vorticity | sound speed] in blocks of 1, dim^2, 1, nv, 1 times NP values
   // (DerivedSize(R) in all; grad v entry (i, j) = dv_i/dx_j at block i*dim + j, vorticity component-major), each block in
   // the layout of lgh_sample_derived.  mask: the blocks that are computed (DERIVED_*); the others are left as they are.
   // out is sized anew (contents lost) when it is smaller than offset + DerivedSize(R).  Asynchronous on the context's
   // stream; the quadrature data is not touched.
   enum { DERIVED_DIV = 1, DERIVED_VORT = 2, DERIVED_GRAD = 4, DERIVED_DETJ = 8, DERIVED_CS = 16, DERIVED_ALL = 31 };
   void SampleDerived(const Vector &S, int R, unsigned mask, Vector &out, long offset = 0) const;
   long DerivedSize(int R) const; // (3 + dim^2 + nv) NP
   // All of the above on the lattices of a list of zone faces (lgh_sample_faces; the driver's `-pv-surface` / `-pv-slice`):
   // faces[2k] = zone, faces[2k + 1] = local face 2 axis + side.  With NPt = FacePoints(R, nfaces) = nfaces (R+1)^(dim-1), out holds
   //    [x | v | e | rho | p | detJ | grad v | div v | vorticity | sound speed | area vector]
   // in blocks of dim, dim, 1, 1, 1, 1, dim^2, 1, nv, 1, dim times NPt values (FacesSize(R, nfaces) in all).  The five standing
   // blocks and the area vector are always computed, the derived ones by mask (DERIVED_*).  out is sized anew when it is
   // smaller.  2D and 3D.  Asynchronous on the context's stream; the quadrature data is not touched.
   void SampleFaces(const Vector &S, const Vector &rho, int R, const std::vector<int> &faces, unsigned mask, Vector &out) const;
   long FacePoints(int R, long nfaces) const;
   long FacesSize(int R, long nfaces) const; // (2 dim + 3 + 3 + dim^2 + nv + dim) NPt
   // One update of a block of running records (lgh_records_update; the driver's `-peaks`) at the n = RecordPoints(R,
   // faces) lattice points of the volume (faces == nullptr) or of a face list: p, rho, e and v of S are sampled into `scratch`
   // ([v | e | rho | p], sized anew when smaller than (dim + 3) n) by the sampling calls above - the same bits a dump of this state
   // holds - and folded into rec (LGH_RECORDS_COLS x n, column-major; the caller sizes it) at time t, dtr since the last update;
   // threshold NaN: none; first: start the records (dtr 0).  Asynchronous on the context's stream; the quadrature data is not touched.
   void UpdateRecords(const Vector &S, const Vector &rho, int R, const std::vector<int> *faces, double t, double dtr, double threshold, bool first,
                      Vector &scratch, Vector &rec) const;
   long RecordPoints(int R, const std::vector<int> *faces) const { return faces ? FacePoints(R, (long)faces->size() / 2) : SamplePoints(R); }
   // Gauges: time series at material points (lgh_gauges_*; the driver's `-gauges`).  CreateGauges makes a set of n =
   // zone.size() gauges - zone[g] this rank's zone id or -1 where another rank owns the gauge, xi[g*dim + a] its reference
   // coordinates - from the host copies of the initial state and density dofs (the gauge's mass rho0 detJ0 is formed from them), with
   // a device buffer of `capacity` samples; returns the handle.  SampleGauges appends one sample of S: one kernel on the context's
   // stream, no host wait.  DrainGauges takes the pending samples of the set of n gauges, oldest first, into rows (samples x n x
   // LGH_GAUGE_COLS; sized anew) and returns their number.  Create and drain are collective on several ranks; the quadrature data is
   // not touched.
   int CreateGauges(const std::vector<int> &zone, const std::vector<double> &xi, const std::vector<double> &S0, const std::vector<double> &rho0_l2,
                    int capacity) const;
   void SampleGauges(int handle, const Vector &S) const;
   int DrainGauges(int handle, int n, std::vector<double> &rows) const;
   void DestroyGauges(int handle) const;
   // A contour of the state S, formed on the lattice of R + 1 points per direction (lgh_contour; the driver's `-pv-iso` / `-pv-plane`):
   // the iso-surface field = value of one of the fields below, or - field CONTOUR_PLANE - the cut plane coef . x = value.  Runs, in
   // this order, SampleFields (and SampleDerived where the field or the mask needs it) into `lattice`, the scalar, the counting and
   // the emitting call into `work`, and the gathers: with nv = dim * n_prims vertices (triangles in 3D, segments in 2D, points not
   // shared), out holds
   //    [x | v | e | rho | p | detJ | grad v | div v | vorticity | sound speed]
   // in blocks of dim, dim, 1, 1, 1, 1, dim^2, 1, nv3, 1 times nv values (ContourSize(n_prims) in all), the derived ones where the mask
   // (DERIVED_*) names them; zone (host) the zone of every primitive.  The vectors are sized anew when they are smaller.  2D and
   // 3D.  Synchronous; the quadrature data is not touched.
   enum { CONTOUR_DENSITY, CONTOUR_ENERGY, CONTOUR_PRESSURE, CONTOUR_SPEED, CONTOUR_X, CONTOUR_Y, CONTOUR_Z, CONTOUR_DIV, CONTOUR_DETJ, CONTOUR_CS, CONTOUR_PLANE };
   static int ContourField(const std::string &name); // the id of density, energy, pressure, speed, x, y, z, div_v, detj, sound_speed; -1 otherwise
   static const char *ContourFieldList();
   void Contour(const Vector &S, const Vector &rho, int R, int field, const double coef[3], double value, unsigned mask, Vector &lattice,
                Vector &work, Vector &out, std::vector<int> &zone, long *n_prims, long *n_skipped) const;
   long ContourSize(long n_prims) const; // (2 dim + 3 + 3 + dim^2 + nv3) dim n_prims
   // Conserved integrals, extremes of the point values and counts of bad points of the state S, folded over zones and ranks
   // (lgh_diagnostics; the rows of the driver's `-hist` file).  Synchronous, collective on several ranks; reads S and the
   // set-up data only - the quadrature data, the force products and dt_est stay as they are.
   void Diagnostics(const Vector &S, double out[LGH_DIAG_COUNT]) const;
   // The state S binned along a coordinate (lgh_profile; the driver's `-prof` files): rows = (nbins + 2) x LGH_PROFILE_COLS host
   // doubles.  Synchronous, collective on several ranks; reads what Diagnostics reads and leaves alone what it leaves alone.
   void Profile(const Vector &S, const lgh_profile_spec &spec, double *rows, long *n_excluded) const;
   // The state S binned onto a fixed Cartesian grid (lgh_map; the driver's `-map` files): rows = (ncells + 1) x LGH_MAP_COLS host
   // doubles.  Collective over the ranks.
   void Map(const Vector &S, const lgh_map_spec &spec, double *rows, long *n_excluded) const;
   // Pressure loads of the state S on lists of zone faces (lgh_loads; the driver's `-loads`): faces holds 3 ints per listed face -
   // zone, local face, row; rho the density ComputeDensity projects on the mesh of S; rows: HOST, nrows x LGH_LOADS_COLS doubles.
   // Collective over the ranks (a rank without faces takes part).  Reads S and rho only.
   void Loads(const Vector &S, const Vector &rho, int nrows, const std::vector<int> &faces, double *rows, long *n_excluded) const;
   // The exact Sedov solution `par` at time t at n radii (host arrays in and out; lgh_sedov_eval on the GPU)
   void SedovEval(const double par[21], double t, const std::vector<double> &r, std::vector<double> &rho, std::vector<double> &v,
                  std::vector<double> &p) const;
   void PrintTimingData(bool IamRoot, int steps, bool fom) const;
   const TimingData &Timing() const;
   void ResetTiming();
   void EnableTimers(bool on);
   lgh_ctx *Context() const { return ctx; }
   long GlobalH1Size() const { return H1GTVSize; }
   long GlobalL2Size() const { return L2GTVSize; }
   int Rank() const { return disc.part.rank; }
   int NRanks() const { return disc.part.nranks; }
   double AllReduce(double v, int op) const;
   // z = a x + b y on the context stream
   void Add(Vector &z, double a, const Vector &x, double b, const Vector &y) const;
   // z1 = a1 x1 + b1 y, z2 = a2 x2 + b2 y: two stage combinations of one increment in one pass (the bits of two Adds)
   void Add2(Vector &z1, double a1, const Vector &x1, double b1, Vector &z2, double a2, const Vector &x2, double b2, const Vector &y) const;
   void Copy(Vector &y, const Vector &x) const;
   void Sync() const;
};

} // namespace hydrodynamics

// ODE solvers (upstream MFEM ODESolver API: Init / Step)
class ODESolver
{
protected:
   hydrodynamics::LagrangianHydroOperator *f = nullptr;

public:
   virtual ~ODESolver() {}
   virtual void Init(hydrodynamics::LagrangianHydroOperator &op) { f = &op; }
   virtual void Step(Vector &S, double &t, double &dt) = 0;
   virtual int Stages() const = 0;
};

// upstream ForwardEulerSolver, RK2Solver(0.5) (midpoint) and RK3SSPSolver (laghos.cpp:521-523)
class ForwardEulerSolver : public ODESolver
{
   Vector k;

public:
   void Init(hydrodynamics::LagrangianHydroOperator &op) override;
   void Step(Vector &S, double &t, double &dt) override;
   int Stages() const override { return 1; }
};
class RK2Solver : public ODESolver
{
   Vector k, x1;
   double a;

public:
   explicit RK2Solver(double a_ = 0.5) : a(a_) {}
   void Init(hydrodynamics::LagrangianHydroOperator &op) override;
   void Step(Vector &S, double &t, double &dt) override;
   int Stages() const override { return 2; }
};
class RK3SSPSolver : public ODESolver
{
   Vector k, y;

public:
   void Init(hydrodynamics::LagrangianHydroOperator &op) override;
   void Step(Vector &S, double &t, double &dt) override;
   int Stages() const override { return 3; }
};

// classical RK4 (upstream RK4Solver; laghos.cpp:524)
class RK4Solver : public ODESolver
{
   Vector k, y, z;

public:
   void Init(hydrodynamics::LagrangianHydroOperator &op) override;
   void Step(Vector &S, double &t, double &dt) override;
   int Stages() const override { return 4; }
};

// upstream ExplicitRKSolver: s stages, Butcher tableau (a strictly lower triangular by rows, b, c),
// and RK6Solver (laghos.cpp:525): Verner's 8-stage 6th-order method with upstream's coefficients
class ExplicitRKSolver : public ODESolver
{
   int s;
   const double *a, *b, *c;
   Vector y;
   std::vector<Vector> k;

public:
   ExplicitRKSolver(int s_, const double *a_, const double *b_, const double *c_) : s(s_), a(a_), b(b_), c(c_) {}
   void Init(hydrodynamics::LagrangianHydroOperator &op) override;
   void Step(Vector &S, double &t, double &dt) override;
   int Stages() const override { return s; }
};
class RK6Solver : public ExplicitRKSolver
{
   static const double a[28], b[8], c[7];

public:
   RK6Solver() : ExplicitRKSolver(8, a, b, c) {}
};

// energy-conserving midpoint scheme (laghos_solver.cpp:1436-1487)
class RK2AvgSolver : public ODESolver
{
   Vector V, dS_dt, S0;

public:
   void Init(hydrodynamics::LagrangianHydroOperator &op) override;
   void Step(Vector &S, double &t, double &dt) override;
   int Stages() const override { return 2; }
};

} // namespace laghos
