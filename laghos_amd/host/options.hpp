// options.hpp — the command line of the driver: what it sets, how it is read, and what of it the mesh decides.
//
// Both functions are host work before any GPU call.  A refusal comes back in `err` as the complete line for stderr: the driver's
// own messages carry `laghos: `, the two of `-err` are the reference's and carry nothing.
#pragma once

#include <string>
#include <utility>
#include <vector>

#include "fem.hpp"

namespace laghos
{

struct Options
{
   int dim = 3;
   std::string mesh_file = "default";
   int nx = 2, ny = 2, nz = 2;
   double Sx = 1, Sy = 1, Sz = 1;
   double blast_energy = 1;
   int rs_levels = 2, rp_levels = 0;
   int problem = 1;
   int order_v = 2, order_e = 1, order_q = -1;
   int ode_solver_type = 4;
   double t_final = 0.6, cfl = 0.5, cg_tol = 1e-8;
   int cg_max_iter = 300, max_tsteps = -1;
   bool p_assembly = true;
   int vis_steps = 5;
   bool check = false, fom = false, impose_visc = false;
   bool check_exact_sedov = false; // -err (laghos.cpp:262)
   bool gfprint = false;           // -print (laghos.cpp:283-285)
   std::string basename = "results/Laghos"; // -k (laghos.cpp:286-287)
   // -paraview: VTK dumps of density, velocity, specific internal energy (the reference's VisIt fields, laghos.cpp:691-701,
   // :845-871) and pressure at cycle 0 and every -vs steps, under <basename>_paraview/ with the collection <basename>.pvd
   bool paraview = false;
   bool vis_refine_set = false;
   int vis_refine = 0;             // -vr: lattice cells per zone and direction (default: order_v), 1..8
   // -pv-fields LIST: derived fields in the -paraview dumps (lgh_sample_derived): a comma list of div_v, vorticity,
   // grad_v, detj, sound_speed, or all (which leaves vorticity out in 1D); the DERIVED_* bits of LagrangianHydroOperator
   bool pv_fields_set = false, pv_vort_named = false; // (named: `vorticity` itself, not through `all`)
   unsigned pv_fields = 0;
   // -pv-surface / -pv-slice AXIS K: dumps of zone FACES instead of volumes (lgh_sample_faces) - the boundary of the
   // global mesh, and up to 8 node planes K of the global zone grid along x, y or z (0 <= K <= n: the side-0 faces of zone layer K,
   // for K = n the side-1 faces of the last layer).  They are written when -paraview writes, with or without it, under
   // <basename>_surface/ and <basename>_slice_<axis><K>/ with a collection each; -vr and -pv-fields apply.
   bool pv_surface = false;
   std::vector<std::pair<int, int>> pv_slices; // (axis, K)
   bool FaceDumps() const { return pv_surface || !pv_slices.empty(); }
   // -pv-iso FIELD VALUE / -pv-plane NX NY [NZ] D: contours formed on the GPU (lgh_contour) - the iso-surface
   // FIELD = VALUE of density, energy, pressure, speed, x, y, z, div_v, detj or sound_speed, and the cut plane NX x + NY y (+ NZ z) = D,
   // which need not follow zone faces; up to 8 of each.  Written when -paraview writes, with or without it, under
   // <basename>_iso<k>_<field>/ and <basename>_plane<k>/ (k = 0, 1, ...: the position among the options of its kind) with a
   // collection each; -vr and -pv-fields apply.  2D and 3D.
   struct Contour
   {
      std::string field; // a name of kContourFields, or "plane"
      double value = 0;  // VALUE, or D
      int ncoef = 0;     // plane: the numbers in front of D (the mesh's dimension decides whether they fit)
      double coef[3] = {0, 0, 0};
      std::string tag;   // "iso0_density", "plane1": the directory is <basename>_<tag>
   };
   std::vector<Contour> pv_isos, pv_planes;
   bool ContourDumps() const { return !pv_isos.empty() || !pv_planes.empty(); }
   bool LatticeDumps() const { return FaceDumps() || ContourDumps(); } // what -vr and -pv-fields apply to beside -paraview
   int dev = 0;
   // multi-rank (set by the launcher, not the reference CLI)
   int nranks = 1, rank = 0;
   const char *nccl_id = nullptr;
   bool quiet = false;
   bool store_stress = false;      // -store-stress: qdata.stressJinvT written by every update (the reference's behaviour)
   // -renumber mfem|random|none: hand the operators the mesh in another numbering of its nodes and zones than this
   // generator's lexicographic one (Discretization::Renumber) - "mfem" is what upstream Laghos passes through
   // H1.GetElementRestriction (laghos_assembly.cpp:133-134) after its uniform refinements (laghos.cpp:391).  Not a
   // reference option: the reference has no choice in the matter.
   std::string renumber = "none";
   int renumber_seed = 1;
   // The periodic outputs (Periodic in driver_outputs.hpp has the rule): every N accepted steps and after the last one; all but
   // the checkpoint also at cycle 0.  0: none.
   int ckpt_steps = 0;             // -ckpt N: checkpoints (checkpoint.hpp; the reference has none)
   int ckpt_keep = 2;              // -ckpt-keep K: pieces of this run kept per rank (0: all)
   std::string restart;            // -restart PATH: a checkpoint stem, or "latest" (<basename>_restart/latest)
   int hist_steps = 0;             // -hist N: rows of <basename>_history.csv
   // -prof N: binned 1-D profiles of the flow (lgh_profile) in <basename>_profile_<cycle>.csv; profile.hpp, DESIGN.md §7e
   int prof_steps = 0;
   std::string prof_axis;          // -prof-axis x|y|z|r (default: r for -p 1, else x)
   int prof_bins = 64;             // -prof-bins B
   bool prof_range_set = false;    // -prof-range LO HI (default: from the initial mesh, at cycle 0)
   double prof_lo = 0, prof_hi = 0;
   double prof_origin[3] = {0, 0, 0}; // -prof-origin X [Y [Z]] (default: the blast position of -err, the origin)
   // -map N: the flow binned onto a fixed Cartesian grid (lgh_map) in <basename>_map/cycle_<cycle>.vti; map_output.hpp, DESIGN.md §7g
   int map_steps = 0;
   int map_cells_n = 0, map_cells[3] = {64, 64, 64}; // -map-cells NX [NY [NZ]] (default: 64 per axis of the mesh)
   int map_box_n = 0;                                // -map-box X0 X1 [Y0 Y1 [Z0 Z1]] (default: the extent of the initial mesh)
   double map_box[6] = {0, 0, 0, 0, 0, 0};
   // -loads N: pressure loads (lgh_loads) in <basename>_loads.csv; loads_output.hpp, DESIGN.md §7i.  Per recorded cycle one line for
   // the boundary of the global mesh, one per wall (x0 x1 y0 y1 [z0 z1]) and one per -loads-plane AXIS K (repeatable, at most 8): node
   // plane K of the global zone grid along x, y or z by the -pv-slice rule - 0 <= K <= n, the side-0 faces of zone layer K, for K = n the
   // side-1 faces of the last layer.  The normal on a plane is the OUTWARD normal of the zone a face belongs to: it points towards
   // lower AXIS for K < n, towards higher AXIS for K = n.  2D and 3D.
   int loads_steps = 0;
   std::vector<std::pair<int, int>> loads_planes; // (axis, K)
   // -peaks N: running records at the lattice points of the material dumps that are on (-paraview, -pv-surface, -pv-slice) - peak
   // pressure and its time, the pressure impulse, peak density, speed and energy (lgh_records_update) - updated at cycle
   // 0, every N accepted steps, after the last one and whenever a dump is written, and written into those dumps as PointData.
   // -peaks-arrival P adds the time at which the pressure first reached P.
   int peaks_steps = 0;
   bool peaks_arrival_set = false;
   double peaks_arrival = 0;       // (meaningful with peaks_arrival_set)
   // -gauges N: time series at material points (lgh_gauges_*) in <basename>_gauges.csv - x, v, rho, e, p, cs, detJ and
   // div v at every gauge at cycle 0, every N accepted steps and after the last one.  A gauge is given by its position in the INITIAL
   // mesh: -gauge X [Y [Z]] (repeatable, at most 64) and -gauge-file PATH (one point per line, # comments), 4096 in all, in the order
   // of the command line, then of the file.  -gauge-buffer M: samples held on the device between two drains (default 256).
   int gauge_steps = 0;
   struct GaugePoint
   {
      int n = 0;                   // the numbers given (the mesh's dimension decides whether they fit)
      double x[3] = {0, 0, 0};
      std::string from;            // "-gauge 0.5 0.25", "-gauge-file pts.txt line 3": what the messages call it
   };
   std::vector<GaugePoint> gauge_points, gauge_file_points;
   std::string gauge_file;
   bool gauge_buffer_set = false;
   int gauge_buffer = 256;
   size_t Gauges() const { return gauge_points.size() + gauge_file_points.size(); }
   bool fingerprint = false;       // -fp: rank 0 prints the state fingerprint after the last step and per checkpoint
};

// Reads the command line into o, a later occurrence of an option over an earlier one, and checks what needs no mesh.
bool ParseArgs(int argc, const char *const *argv, Options &o, std::string &err);

// What only the mesh (refined as the run will use it) can decide: o.dim, the 1D switch from -pa to -fa with the reference's
// line on stdout, the defaults that depend on problem and dimension, and every option the mesh's dimension or zone grid refuses.
bool CheckAgainstMesh(Options &o, const CartMesh &mesh, std::string &err);

} // namespace laghos
