// laghos.cpp — driver of the MI355X-native Laghos hot path.
//
// Mirrors the command line, time loop and output format of the reference driver
// (/root/reference/laghos.cpp:119-1092) for the subset this repository supports:
// PA mode (-pa), dim 2/3, problems 0-7 on the structured meshes of data/; in 1D (data/segment01.mesh, -dim 1) the FA path,
// problems 1 and 2, to which -pa switches as in the reference (laghos.cpp:454-462);
// -s 1, 2, 3, 4 (Euler, RK2, RK3 SSP, RK4) and 7 (RK2Avg).  Everything else the reference driver does
// (GLVis sockets, VisIt / MFEM data collections, -fa in 2D/3D, AMR, METIS, Umpire, Caliper) is out of scope
// (SURVEY §2); `-paraview` writes VTK files ParaView and VisIt open directly (vtk_output.hpp).
// Exposed both as the `laghos` executable and as C entry points
// (laghos_sim_*) that bench.py drives through ctypes.
#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sys/stat.h>
#include <iomanip>
#include <iostream>
#include <limits>
#include <memory>
#include <sstream>
#include <string>

#include "laghos_solver.hpp"
#include "sedov_exact.hpp"
#include "vtk_output.hpp"
#include "checkpoint.hpp"
#include "history.hpp"
#include "map_output.hpp"
#include "profile.hpp"

using namespace laghos;

namespace
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
   // checkpoint / restart (checkpoint.hpp; the reference has none)
   int ckpt_steps = 0;             // -ckpt N: a checkpoint after every accepted step with ti % N == 0 and after the last one (0: none)
   int ckpt_keep = 2;              // -ckpt-keep K: pieces of this run kept per rank (0: all)
   std::string restart;            // -restart PATH: a checkpoint stem, or "latest" (<basename>_restart/latest)
   int hist_steps = 0;             // -hist N: a row of <basename>_history.csv at cycle 0, after every accepted step with ti % N == 0 and after the last one (0: none)
   // -prof N: a binned 1-D profile of the flow (lgh_profile) in <basename>_profile_<cycle>.csv at cycle 0, after every accepted step
   // with ti % N == 0 and after the last one (0: none); profile.hpp, DESIGN.md §7e
   int prof_steps = 0;
   std::string prof_axis;          // -prof-axis x|y|z|r (default: r for -p 1, else x)
   int prof_bins = 64;             // -prof-bins B
   bool prof_range_set = false;    // -prof-range LO HI (default: from the initial mesh, at cycle 0)
   double prof_lo = 0, prof_hi = 0;
   double prof_origin[3] = {0, 0, 0}; // -prof-origin X [Y [Z]] (default: the blast position of -err, the origin)
   // -map N: the flow binned onto a fixed Cartesian grid (lgh_map) in <basename>_map/cycle_<cycle>.vti at cycle 0, after every
   // accepted step with ti % N == 0 and after the last one (0: none); map_output.hpp, DESIGN.md §7g
   int map_steps = 0;
   int map_cells_n = 0, map_cells[3] = {64, 64, 64}; // -map-cells NX [NY [NZ]] (default: 64 per axis of the mesh)
   int map_box_n = 0;                                // -map-box X0 X1 [Y0 Y1 [Z0 Z1]] (default: the extent of the initial mesh)
   double map_box[6] = {0, 0, 0, 0, 0, 0};
   bool fingerprint = false;       // -fp: rank 0 prints the state fingerprint after the last step and per checkpoint
};

bool ParseArgs(int argc, const char *const *argv, Options &o, std::string &err)
{
   auto need = [&](int &i) -> const char * {
      if (i + 1 >= argc) { err = std::string("missing value for ") + argv[i]; return nullptr; }
      return argv[++i];
   };
   for (int i = 0; i < argc; i++)
   {
      const std::string a = argv[i];
      const char *v = nullptr;
#define OPT_INT(s, l, field) if (a == s || a == l) { if (!(v = need(i))) { return false; } o.field = std::atoi(v); continue; }
#define OPT_DBL(s, l, field) if (a == s || a == l) { if (!(v = need(i))) { return false; } o.field = std::atof(v); continue; }
      OPT_INT("-dim", "--dimension", dim)
      if (a == "-m" || a == "--mesh") { if (!(v = need(i))) { return false; } o.mesh_file = v; continue; }
      OPT_INT("-nx", "--xelems", nx) OPT_INT("-ny", "--yelems", ny) OPT_INT("-nz", "--zelems", nz)
      OPT_DBL("-E0", "--blast-energy", blast_energy)
      OPT_DBL("-Sx", "--xwidth", Sx) OPT_DBL("-Sy", "--ywidth", Sy) OPT_DBL("-Sz", "--zwidth", Sz)
      OPT_INT("-rs", "--refine-serial", rs_levels) OPT_INT("-rp", "--refine-parallel", rp_levels)
      OPT_INT("-p", "--problem", problem)
      OPT_INT("-ok", "--order-kinematic", order_v) OPT_INT("-ot", "--order-thermo", order_e)
      OPT_INT("-oq", "--order-intrule", order_q)
      OPT_INT("-s", "--ode-solver", ode_solver_type)
      OPT_DBL("-tf", "--t-final", t_final) OPT_DBL("-cfl", "--cfl", cfl) OPT_DBL("-cgt", "--cg-tol", cg_tol)
      OPT_INT("-cgm", "--cg-max-steps", cg_max_iter) OPT_INT("-ms", "--max-steps", max_tsteps)
      OPT_INT("-vs", "--visualization-steps", vis_steps) OPT_INT("-dev", "--dev", dev)
      OPT_INT("-renumber-seed", "--renumber-seed", renumber_seed)
      if (a == "-ckpt" || a == "--checkpoint-steps")
      {
         if (!(v = need(i))) { return false; }
         o.ckpt_steps = std::atoi(v);
         if (o.ckpt_steps < 1) { err = "-ckpt / --checkpoint-steps must be at least 1, got " + std::string(v); return false; }
         continue;
      }
      if (a == "-ckpt-keep" || a == "--checkpoint-keep")
      {
         if (!(v = need(i))) { return false; }
         o.ckpt_keep = std::atoi(v);
         if (o.ckpt_keep < 0) { err = "-ckpt-keep / --checkpoint-keep must be 0 (keep all) or more, got " + std::string(v); return false; }
         continue;
      }
      if (a == "-hist" || a == "--history-steps")
      {
         if (!(v = need(i))) { return false; }
         o.hist_steps = std::atoi(v);
         if (o.hist_steps < 1) { err = "-hist / --history-steps must be at least 1, got " + std::string(v); return false; }
         continue;
      }
      if (a == "-prof" || a == "--profile-steps")
      {
         if (!(v = need(i))) { return false; }
         o.prof_steps = std::atoi(v);
         if (o.prof_steps < 1) { err = "-prof / --profile-steps must be at least 1, got " + std::string(v); return false; }
         continue;
      }
      if (a == "-prof-axis" || a == "--profile-axis")
      {
         if (!(v = need(i))) { return false; }
         o.prof_axis = v;
         if (o.prof_axis != "x" && o.prof_axis != "y" && o.prof_axis != "z" && o.prof_axis != "r") { err = "-prof-axis must be x, y, z or r, got " + o.prof_axis; return false; }
         continue;
      }
      if (a == "-prof-bins" || a == "--profile-bins")
      {
         if (!(v = need(i))) { return false; }
         o.prof_bins = std::atoi(v);
         if (o.prof_bins < 1 || o.prof_bins > LGH_PROFILE_MAX_BINS)
         {
            err = "-prof-bins must be between 1 and " + std::to_string(LGH_PROFILE_MAX_BINS) + ", got " + std::string(v);
            return false;
         }
         continue;
      }
      if (a == "-prof-range" || a == "--profile-range")
      {
         double lh[2];
         for (int k = 0; k < 2; k++)
         {
            if (!(v = need(i))) { return false; }
            char *end = nullptr;
            lh[k] = std::strtod(v, &end);
            if (end == v || *end) { err = "-prof-range needs two numbers, got " + std::string(v); return false; }
         }
         if (!(std::isfinite(lh[0]) && std::isfinite(lh[1]) && std::isfinite(lh[1] - lh[0]) && lh[0] < lh[1]))
         {
            err = "-prof-range LO HI needs finite LO < HI";
            return false;
         }
         o.prof_lo = lh[0]; o.prof_hi = lh[1]; o.prof_range_set = true;
         continue;
      }
      if (a == "-prof-origin" || a == "--profile-origin")
      {
         int n = 0;
         while (n < 3 && i + 1 < argc) // one to three numbers
         {
            char *end = nullptr;
            const double x = std::strtod(argv[i + 1], &end);
            if (end == argv[i + 1] || *end) { break; }
            if (!std::isfinite(x)) { err = "-prof-origin needs finite coordinates"; return false; }
            o.prof_origin[n++] = x;
            i++;
         }
         if (n == 0) { err = "-prof-origin needs one to three numbers"; return false; }
         continue;
      }
      if (a == "-map" || a == "--map-steps")
      {
         if (!(v = need(i))) { return false; }
         o.map_steps = std::atoi(v);
         if (o.map_steps < 1) { err = "-map / --map-steps must be at least 1, got " + std::string(v); return false; }
         continue;
      }
      if (a == "-map-cells" || a == "--map-cells")
      {
         o.map_cells_n = 0;
         while (o.map_cells_n < 3 && i + 1 < argc) // one to three counts
         {
            char *end = nullptr;
            const long k = std::strtol(argv[i + 1], &end, 10);
            if (end == argv[i + 1] || *end) { break; }
            if (k < 1 || k > LGH_MAP_MAX_CELLS) { err = "-map-cells needs counts between 1 and " + std::to_string(LGH_MAP_MAX_CELLS) + ", got " + std::string(argv[i + 1]); return false; }
            o.map_cells[o.map_cells_n++] = (int)k;
            i++;
         }
         if (o.map_cells_n == 0) { err = "-map-cells needs one to three counts"; return false; }
         continue;
      }
      if (a == "-map-box" || a == "--map-box")
      {
         o.map_box_n = 0;
         while (o.map_box_n < 6 && i + 1 < argc) // one pair per axis
         {
            char *end = nullptr;
            const double x = std::strtod(argv[i + 1], &end);
            if (end == argv[i + 1] || *end) { break; }
            o.map_box[o.map_box_n++] = x;
            i++;
         }
         if (o.map_box_n == 0 || o.map_box_n % 2) { err = "-map-box needs a pair LO HI per axis, got " + std::to_string(o.map_box_n) + " numbers"; return false; }
         for (int k = 0; k < o.map_box_n; k += 2)
         {
            const double lo = o.map_box[k], hi = o.map_box[k + 1];
            if (!(std::isfinite(lo) && std::isfinite(hi) && std::isfinite(hi - lo) && lo < hi)) { err = "-map-box needs finite LO < HI on every axis"; return false; }
         }
         continue;
      }
      if (a == "-restart" || a == "--restart")
      {
         if (!(v = need(i))) { return false; }
         o.restart = v;
         if (o.restart.empty()) { err = "-restart needs a checkpoint stem or the word latest"; return false; }
         continue;
      }
      if (a == "-fp" || a == "--fingerprint") { o.fingerprint = true; continue; }
#undef OPT_INT
#undef OPT_DBL
      if (a == "-pa" || a == "--partial-assembly") { o.p_assembly = true; continue; }
      if (a == "-fa" || a == "--full-assembly") { o.p_assembly = false; continue; }
      if (a == "-chk" || a == "--checks") { o.check = true; continue; }
      if (a == "-no-chk" || a == "--no-checks") { o.check = false; continue; }
      if (a == "-iv" || a == "--impose-viscosity") { o.impose_visc = true; continue; }
      if (a == "-niv" || a == "--no-impose-viscosity") { o.impose_visc = false; continue; }
      if (a == "-f" || a == "--fom") { o.fom = true; continue; }
      if (a == "-err" || a == "--exact-error") { o.check_exact_sedov = true; continue; }
      if (a == "-no-err" || a == "--no-exact-error") { o.check_exact_sedov = false; continue; }
      if (a == "-no-fom" || a == "--no-fom") { o.fom = false; continue; }
      if (a == "-q" || a == "--quiet") { o.quiet = true; continue; }
      if (a == "-print" || a == "--print") { o.gfprint = true; continue; }
      if (a == "-paraview" || a == "--paraview") { o.paraview = true; continue; }
      if (a == "-no-paraview" || a == "--no-paraview") { o.paraview = false; continue; }
      if (a == "-vr" || a == "--vis-refine")
      {
         if (!(v = need(i))) { return false; }
         o.vis_refine = std::atoi(v);
         o.vis_refine_set = true;
         continue;
      }
      if (a == "-pv-fields" || a == "--paraview-fields")
      {
         if (!(v = need(i))) { return false; }
         using H = hydrodynamics::LagrangianHydroOperator;
         static const struct { const char *name; unsigned bit; } known[] = {
            {"div_v", H::DERIVED_DIV}, {"vorticity", H::DERIVED_VORT}, {"grad_v", H::DERIVED_GRAD}, {"detj", H::DERIVED_DETJ},
            {"sound_speed", H::DERIVED_CS}};
         const std::string list = v;
         o.pv_fields_set = true;
         o.pv_vort_named = false;
         o.pv_fields = 0;
         for (size_t pos = 0; pos <= list.size();)
         {
            const size_t comma = std::min(list.find(',', pos), list.size());
            const std::string name = list.substr(pos, comma - pos);
            pos = comma + 1;
            if (name.empty()) { continue; }
            unsigned bit = 0;
            if (name == "all") { bit = H::DERIVED_ALL; }
            for (const auto &k : known) { if (name == k.name) { bit = k.bit; } }
            if (!bit)
            {
               err = "-pv-fields: unknown field " + name + " (div_v, vorticity, grad_v, detj, sound_speed or all)";
               return false;
            }
            if (name == "vorticity") { o.pv_vort_named = true; }
            o.pv_fields |= bit;
         }
         if (!o.pv_fields) { err = "-pv-fields needs a list of div_v, vorticity, grad_v, detj, sound_speed, or all: the list is empty"; return false; }
         continue;
      }
      if (a == "-pv-surface" || a == "--paraview-surface") { o.pv_surface = true; continue; }
      if (a == "-pv-slice" || a == "--paraview-slice")
      {
         if (i + 2 >= argc) { err = "missing value for " + a + " AXIS K"; return false; }
         if (!(v = need(i))) { return false; }
         const std::string ax = v;
         if (ax != "x" && ax != "y" && ax != "z") { err = "-pv-slice AXIS K: the axis must be x, y or z, got " + ax; return false; }
         if (!(v = need(i))) { return false; }
         char *end = nullptr;
         const long K = std::strtol(v, &end, 10);
         if (end == v || *end || K < 0 || K > 1000000000L) { err = "-pv-slice " + ax + " K: K must be a node plane 0 <= K <= n of the zone grid, got " + std::string(v); return false; }
         const std::pair<int, int> sl(ax[0] - 'x', (int)K);
         if (std::find(o.pv_slices.begin(), o.pv_slices.end(), sl) != o.pv_slices.end())
         {
            err = "-pv-slice " + ax + " " + std::to_string(K) + " is given twice";
            return false;
         }
         if (o.pv_slices.size() == 8) { err = "-pv-slice " + ax + " " + std::to_string(K) + ": at most 8 slices, this is the ninth"; return false; }
         o.pv_slices.push_back(sl);
         continue;
      }
      if (a == "-store-stress" || a == "--store-stress") { o.store_stress = true; continue; }
      if (a == "-no-store-stress" || a == "--no-store-stress") { o.store_stress = false; continue; }
      if (a == "-renumber" || a == "--renumber") { if (!(v = need(i))) { return false; } o.renumber = v; continue; }
      if (a == "-k" || a == "--outputfilename") { if (!(v = need(i))) { return false; } o.basename = v; continue; }
      if (a == "-d" || a == "--device") { if (!need(i)) { return false; } continue; } // always the HIP path
      if (a == "-no-vis" || a == "--no-visualization" || a == "-no-visit" || a == "-no-print") { continue; }
      err = "unsupported option: " + a;
      return false;
   }
   if (!o.vis_refine_set) { o.vis_refine = o.order_v; }
   if ((o.vis_refine_set || o.paraview || o.FaceDumps()) && (o.vis_refine < 1 || o.vis_refine > 8))
   {
      err = "-vr / --vis-refine must be between 1 and 8, got " + std::to_string(o.vis_refine);
      return false;
   }
   if (o.pv_fields_set && !o.paraview && !o.FaceDumps())
   {
      err = "-pv-fields adds fields to the -paraview dumps: it needs -paraview";
      return false;
   }
   if ((o.map_cells_n > 0 || o.map_box_n > 0) && o.map_steps == 0)
   {
      err = std::string(o.map_cells_n > 0 ? "-map-cells" : "-map-box") + " describes the -map files: it needs -map";
      return false;
   }
   return true;
}

// the reference's --checks table (laghos.cpp:1441-1463), all eight problems
bool CheckNorm(int dim, int problem, int ti, double nrm, int &chk)
{
   struct Row { int dim, p, it; double norm; };
   static const Row rows[] = {
      {2, 0, 5, 6.546538624534384e+00}, {2, 0, 27, 7.588576357792927e+00},
      {2, 1, 5, 3.508254945225794e+00}, {2, 1, 15, 2.756444596823211e+00},
      {2, 2, 5, 1.020745795651244e+01}, {2, 2, 59, 1.721590205901898e+01},
      {2, 3, 5, 8.000000000000000e+00}, {2, 3, 16, 8.000000000000000e+00},
      {2, 4, 5, 3.446324942352448e+01}, {2, 4, 18, 3.446844033767240e+01},
      {2, 5, 5, 1.030899557252528e+01}, {2, 5, 36, 1.057362418574309e+01},
      {2, 6, 5, 8.039707010835693e+00}, {2, 6, 36, 8.316970976817373e+00},
      {2, 7, 5, 1.514929259650760e+01}, {2, 7, 25, 1.514931278155159e+01},
      {3, 0, 5, 1.198510951452527e+03}, {3, 0, 188, 1.199384410059154e+03},
      {3, 1, 5, 6.695818592962833e+00}, {3, 1, 20, 4.267902387082487e+00},
      {3, 2, 5, 2.041491591302486e+01}, {3, 2, 59, 3.443180411803796e+01},
      {3, 3, 5, 1.600000000000000e+01}, {3, 3, 16, 1.600000000000000e+01},
      {3, 4, 5, 6.892649884704898e+01}, {3, 4, 18, 6.893688067534482e+01},
      {3, 5, 5, 2.061984481890964e+01}, {3, 5, 36, 2.114519664792607e+01},
      {3, 6, 5, 1.607988713996459e+01}, {3, 6, 36, 1.662736010353023e+01},
      {3, 7, 5, 3.029858112572883e+01}, {3, 7, 24, 3.029858832743707e+01}};
   bool ok = true;
   for (const Row &r : rows)
   {
      if (r.dim == dim && r.p == problem && r.it == ti)
      {
         chk++;
         // the reference compares at 1e-13 against its own CPU build; this GPU
         // path is held to 1e-10 (north_star: 1e-6)
         const double rel = std::fabs(nrm - r.norm) / r.norm;
         if (!(rel < 1e-10))
         {
            std::printf("check P%d #%d: %.15e vs %.15e (rel %.2e)\n", problem, ti, nrm, r.norm, rel);
            ok = false;
         }
      }
   }
   return ok;
}

} // namespace

// `-print` (laghos.cpp:873-900): basename_<ti>_{mesh,rho,v,e}, 8 significant digits as the
// reference's ofs.precision(8).  The reference writes MFEM's mesh / grid-function text formats in MFEM's
// global dof numbering (PrintAsOne / SaveAsOne); MFEM is not part of this repo, so the files carry the
// same header structure and the same fields but THIS library's numbering: H1 nodes lexicographic over
// the Cartesian node grid (x fastest), vector fields byNODES (Ordering: 0), L2 dofs zone by zone in
// lexicographic Bernstein order.  On several ranks every rank writes its block to <name>.<rank>.
bool WriteFields(const std::string &basename, int ti, const Discretization &d, int nranks, int rank,
                 const std::vector<double> &S, const std::vector<double> &rho)
{
   const size_t slash = basename.find_last_of('/');
   if (slash != std::string::npos)
   {
      // create the directory chain of the base name (the reference leaves that to the user)
      const std::string dir = basename.substr(0, slash);
      for (size_t p = 1; p <= dir.size(); p++)
      {
         if (p == dir.size() || dir[p] == '/') { (void)::mkdir(dir.substr(0, p).c_str(), 0777); }
      }
   }
   auto name = [&](const char *what) {
      std::ostringstream os;
      os << basename << "_" << ti << "_" << what;
      if (nranks > 1) { os << "." << rank; }
      return os.str();
   };
   const int dim = d.dim, ok = d.tab.D1D - 1, ot = d.tab.L1D - 1;
   const long H1V = (long)dim * d.N;
   auto header = [&](std::ofstream &f, const char *fec, int order, int vdim) {
      f << "FiniteElementSpace\nFiniteElementCollection: " << fec << "_" << dim << "D_P" << order << "\nVDim: " << vdim
        << "\nOrdering: 0\n\n";
   };
   {
      std::ofstream f(name("mesh").c_str());
      if (!f) { return false; }
      f.precision(8);
      f << "LGH mesh v1.0\n\n# structured " << (dim == 3 ? "hexahedral" : (dim == 2 ? "quadrilateral" : "segment"))
        << " zones; node ids of a zone in lexicographic order of its (order+1)^dim H1 nodes\n\ndimension\n" << dim
        << "\n\nelements\n" << d.NE << "\n";
      const int geom = (dim == 3) ? 5 : (dim == 2 ? 3 : 1); // MFEM geometry ids: CUBE, SQUARE, SEGMENT
      for (int e = 0; e < d.NE; e++)
      {
         f << 1 << " " << geom;
         for (int k = 0; k < d.ND; k++) { f << " " << d.h1map[(size_t)e * d.ND + k]; }
         f << "\n";
      }
      f << "\nnodes\n";
      header(f, "H1", ok, dim);
      for (long i = 0; i < H1V; i++) { f << S[i] << "\n"; }
   }
   {
      std::ofstream f(name("rho").c_str());
      if (!f) { return false; }
      f.precision(8);
      header(f, "L2_T2", ot, 1); // positive (Bernstein) basis, as the reference's l2_fec
      for (double v : rho) { f << v << "\n"; }
   }
   {
      std::ofstream f(name("v").c_str());
      if (!f) { return false; }
      f.precision(8);
      header(f, "H1", ok, dim);
      for (long i = 0; i < H1V; i++) { f << S[H1V + i] << "\n"; }
   }
   {
      std::ofstream f(name("e").c_str());
      if (!f) { return false; }
      f.precision(8);
      header(f, "L2_T2", ot, 1);
      for (size_t i = 2 * H1V; i < S.size(); i++) { f << S[i] << "\n"; }
   }
   return true;
}

// ---- simulation object driven by main() and by bench.py ------------------------------------
struct laghos_sim
{
   Options opt;
   std::unique_ptr<Discretization> disc;
   std::unique_ptr<hydrodynamics::LagrangianHydroOperator> hydro;
   std::unique_ptr<ODESolver> ode;
   Vector S, S_old;
   double t = 0.0, dt = 0.0, t_old = 0.0;
   int ti = 1, steps = 0, repeats = 0;
   bool last_step = false;
   double energy_init = 0.0;
   int checks = 0;
   bool checks_ok = true;
   std::string error;
   // -paraview: the dumps so far (the .pvd is rewritten after each), scratch, and where the time of a dump goes
   std::vector<double> pv_times;
   std::vector<int> pv_cycles;
   Vector pv_rho, pv_dev;
   std::vector<double> pv_host;
   double pv_seconds[3] = {0, 0, 0}; // density + sampling (GPU), device-to-host copy, file write
   // -pv-surface / -pv-slice: the face lists of this rank (fixed at the start: the mesh is Lagrangian), in the order of the command
   // line with the surface first; scratch; where the time of their dumps goes
   struct FaceSet
   {
      std::string tag;        // "surface", "slice_z3": the directory is <basename>_<tag>
      std::vector<int> faces; // (zone, local face) pairs in ascending order
      Vector dev;
   };
   std::vector<FaceSet> pv_faces;
   double pvf_seconds[3] = {0, 0, 0};
   // -ckpt / -restart: the fingerprint of the set-up arrays, the pieces this run wrote (oldest first; -ckpt-keep removes from
   // this list only), scratch, and where the time of a checkpoint goes
   unsigned long long setup_fp[2] = {0, 0};
   std::vector<std::string> ckpt_mine;
   std::vector<double> ckpt_host;
   int ckpt_count = 0;
   double ckpt_seconds[3] = {0, 0, 0}; // fingerprint (GPU), device-to-host copy, host fingerprint + file write
   // -hist: the file (rank 0) and the last cycle that has its row (a restart: the checkpoint's cycle, which gets none)
   HistoryFile hist;
   int hist_last = -1;
   // -prof: what is binned (axis, range and origin fixed at the start, from the initial mesh), the last cycle that has its file (a
   // restart: the checkpoint's cycle, which gets none), the files of this run, the table, and the exact Sedov solution where it applies
   lgh_profile_spec prof_spec = {};
   char prof_axis = 'x';
   int prof_last = -1, prof_files = 0;
   std::vector<double> prof_rows;
   // -map: the grid (fixed at the start, from the initial mesh), the last cycle that has its file, the files of this run
   lgh_map_spec map_spec = {};
   int map_last = -1, map_files = 0;
   std::vector<double> map_rows;
   bool prof_exact = false;
   double prof_par[21] = {};
   int steps_at_start = 0;             // RK steps the checkpoint of a restart had taken: timing / FOM cover the restarted segment
};

// The derived blocks of a dump as the file holds them, in the order of the table of DESIGN.md §7f: point by point, vectors and
// tensors padded with zeros to 3 and 3 x 3 (the 2D vorticity is the z component).  detj .. cs: the blocks of NP points in the
// layout of lgh_sample_derived; vort_buf / grad_buf hold the padded copies the returned fields point into.
static std::vector<VtuField> DerivedVtuFields(unsigned mask, int dim, long NP, const double *detj, const double *grad, const double *div,
                                              const double *vort, const double *cs, std::vector<double> &vort_buf, std::vector<double> &grad_buf)
{
   using H = hydrodynamics::LagrangianHydroOperator;
   std::vector<VtuField> extra;
   const int nv = (dim == 3) ? 3 : (dim == 2 ? 1 : 0);
   if (mask & H::DERIVED_DIV) { extra.push_back({"div_v", 1, div}); }
   if (mask & H::DERIVED_VORT)
   {
      vort_buf.assign(3 * (size_t)NP, 0.0);
      for (int c = 0; c < nv; c++)
      {
         for (long i = 0; i < NP; i++) { vort_buf[3 * i + (dim == 2 ? 2 : c)] = vort[c * NP + i]; }
      }
      extra.push_back({"vorticity", 3, vort_buf.data()});
   }
   if (mask & H::DERIVED_GRAD)
   {
      grad_buf.assign(9 * (size_t)NP, 0.0);
      for (int a = 0; a < dim; a++)
      {
         for (int b = 0; b < dim; b++)
         {
            for (long i = 0; i < NP; i++) { grad_buf[9 * i + 3 * a + b] = grad[(a * dim + b) * NP + i]; }
         }
      }
      extra.push_back({"velocity_gradient", 9, grad_buf.data()});
   }
   if (mask & H::DERIVED_DETJ) { extra.push_back({"detJ", 1, detj}); }
   if (mask & H::DERIVED_CS) { extra.push_back({"sound_speed", 1, cs}); }
   return extra;
}

// One `-paraview` dump of the state at cycle `cycle` (laghos.cpp:691-701, :845-871): density, lattice values on the GPU, one
// copy to the host, <basename>_paraview/cycle_<cycle>[.<rank>].vtu; rank 0 adds the .pvtu of a multi-rank cycle and
// rewrites <basename>.pvd.  rho: the density of this state where the caller (`-print`) has projected it already.
// (DumpVis below has entered the dump into pv_times / pv_cycles.)
static bool DumpParaview(laghos_sim *s, int cycle, const Vector *rho = nullptr)
{
   using clk = std::chrono::steady_clock;
   auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
   const Options &o = s->opt;
   auto &hydro = *s->hydro;
   const int dim = s->disc->dim, R = o.vis_refine;
   const long NP = hydro.SamplePoints(R);
   const clk::time_point t0 = clk::now();
   if (!rho)
   {
      hydro.ComputeDensity(s->S, s->pv_rho); // rho_gf is refreshed before the output (laghos.cpp:827-830)
      rho = &s->pv_rho;
   }
   const long base = (2 * dim + 3) * NP; // the blocks of SampleFields; those of SampleDerived follow in the same vector
   if (o.pv_fields && s->pv_dev.Size() < base + hydro.DerivedSize(R)) { s->pv_dev.SetSize(base + hydro.DerivedSize(R)); }
   hydro.SampleFields(s->S, *rho, R, s->pv_dev);
   if (o.pv_fields) { hydro.SampleDerived(s->S, R, o.pv_fields, s->pv_dev, base); }
   hydro.Sync();
   const clk::time_point t1 = clk::now();
   s->pv_dev.ToHost(s->pv_host);
   const clk::time_point t2 = clk::now();
   const double *h = s->pv_host.data();
   const std::string dir = o.basename + "_paraview";
   const size_t slash = o.basename.find_last_of('/');
   const std::string rel_dir = (slash == std::string::npos ? o.basename : o.basename.substr(slash + 1)) + "_paraview";
   std::vector<VtuField> extra;
   std::vector<double> pv_vort, pv_grad;
   if (o.pv_fields)
   {
      const int nv = (dim == 3) ? 3 : (dim == 2 ? 1 : 0);
      const double *detj = h + base, *grad = detj + NP, *div = grad + (long)dim * dim * NP, *vort = div + NP, *cs = vort + nv * NP;
      extra = DerivedVtuFields(o.pv_fields, dim, NP, detj, grad, div, vort, cs, pv_vort, pv_grad);
   }
   bool ok = WriteVtuFields(dir, dim, s->disc->NE, R + 1, h, h + dim * NP, h + 2 * dim * NP, h + (2 * dim + 1) * NP,
                            h + (2 * dim + 2) * NP, extra, cycle, s->t, o.rank, o.nranks);
   if (ok && o.rank == 0)
   {
      if (o.nranks > 1) { ok = WritePvtuFields(dir, cycle, s->t, o.nranks, extra); }
      ok = ok && WritePvd(o.basename + ".pvd", rel_dir, s->pv_times, s->pv_cycles, o.nranks);
   }
   const clk::time_point t3 = clk::now();
   s->pv_seconds[0] += secs(t0, t1);
   s->pv_seconds[1] += secs(t1, t2);
   s->pv_seconds[2] += secs(t2, t3);
   if (!ok)
   {
      s->error = "cannot write the -paraview files under " + dir;
      std::fprintf(stderr, "%s\n", s->error.c_str());
   }
   return ok;
}

static std::string FaceSetDir(const std::string &basename, const std::string &tag) { return basename + "_" + tag; }

// The faces of this rank's zones on the boundary of the GLOBAL mesh (axis < 0), or on node plane K of the global zone grid along
// `axis`: from the driver's own structured coordinates - zone j is the structured zone elem_perm[j] of the rank's block, which
// starts at Partition::eoff in the global grid of CartMesh::ne zones - so the selection holds under -renumber and on several
// ranks, and an inter-rank interface is no boundary.  Ascending (zone, face).
static std::vector<int> SelectFaces(const Discretization &d, int axis, int K)
{
   std::vector<int> faces;
   for (int j = 0; j < d.NE; j++)
   {
      int l = d.elem_perm.empty() ? j : d.elem_perm[j], g[3] = {0, 0, 0};
      for (int a = 0; a < d.dim; a++)
      {
         g[a] = l % d.part.ne[a] + d.part.eoff[a];
         l /= d.part.ne[a];
      }
      for (int a = 0; a < d.dim; a++)
      {
         const int n = d.mesh.ne(a);
         if (axis < 0)
         {
            if (g[a] == 0) { faces.push_back(j); faces.push_back(2 * a); }
            if (g[a] == n - 1) { faces.push_back(j); faces.push_back(2 * a + 1); }
         }
         else if (a == axis)
         {
            if (K < n && g[a] == K) { faces.push_back(j); faces.push_back(2 * a); }
            if (K == n && g[a] == n - 1) { faces.push_back(j); faces.push_back(2 * a + 1); }
         }
      }
   }
   return faces;
}

// One face set of the state as it stands into host arrays: the blocks of LagrangianHydroOperator::SampleFaces.
static void SampleFaceSet(laghos_sim *s, laghos_sim::FaceSet &fs, const Vector &rho, int R, unsigned mask, std::vector<double> &host,
                          double seconds[2])
{
   using clk = std::chrono::steady_clock;
   auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
   const clk::time_point t0 = clk::now();
   s->hydro->SampleFaces(s->S, rho, R, fs.faces, mask, fs.dev);
   s->hydro->Sync();
   const clk::time_point t1 = clk::now();
   fs.dev.ToHost(host);
   const clk::time_point t2 = clk::now();
   seconds[0] += secs(t0, t1);
   seconds[1] += secs(t1, t2);
}

// The `-pv-surface` / `-pv-slice` files of the state at cycle `cycle`: per face set the lattice values on the GPU, one copy to
// the host, <basename>_<tag>/cycle_<cycle>[.<rank>].vtu (a rank without faces writes an empty piece); rank 0 adds the .pvtu
// of a multi-rank cycle and rewrites <basename>_<tag>.pvd.
static bool DumpFaces(laghos_sim *s, int cycle, const Vector &rho)
{
   using clk = std::chrono::steady_clock;
   const Options &o = s->opt;
   auto &hydro = *s->hydro;
   const int dim = s->disc->dim, R = o.vis_refine;
   const int nv = (dim == 3) ? 3 : 1;
   for (laghos_sim::FaceSet &fs : s->pv_faces)
   {
      const int nfaces = (int)fs.faces.size() / 2;
      const long NPt = hydro.FacePoints(R, nfaces);
      SampleFaceSet(s, fs, rho, R, o.pv_fields, s->pv_host, s->pvf_seconds);
      const clk::time_point t2 = clk::now();
      const double *h = s->pv_host.data();
      const double *x = h, *v = x + dim * NPt, *e = v + dim * NPt, *r = e + NPt, *p = r + NPt;
      const double *detj = p + NPt, *grad = detj + NPt, *div = grad + (long)dim * dim * NPt, *vort = div + NPt, *cs = vort + nv * NPt, *an = cs + NPt;
      std::vector<double> vort_buf, grad_buf;
      const std::vector<VtuField> extra = DerivedVtuFields(o.pv_fields, dim, NPt, detj, grad, div, vort, cs, vort_buf, grad_buf);
      const std::string dir = FaceSetDir(o.basename, fs.tag);
      const size_t slash = o.basename.find_last_of('/');
      const std::string rel_dir = FaceSetDir(slash == std::string::npos ? o.basename : o.basename.substr(slash + 1), fs.tag);
      bool ok = WriteVtuFaces(dir, dim, nfaces, fs.faces.data(), R + 1, x, v, e, r, p, extra, an, cycle, s->t, o.rank, o.nranks);
      if (ok && o.rank == 0)
      {
         if (o.nranks > 1) { ok = WritePvtuFaces(dir, cycle, s->t, o.nranks, extra); }
         ok = ok && WritePvd(dir + ".pvd", rel_dir, s->pv_times, s->pv_cycles, o.nranks);
      }
      s->pvf_seconds[2] += std::chrono::duration<double>(clk::now() - t2).count();
      if (!ok)
      {
         s->error = "cannot write the -pv-" + std::string(fs.tag == "surface" ? "surface" : "slice") + " files under " + dir;
         std::fprintf(stderr, "%s\n", s->error.c_str());
         return false;
      }
   }
   return true;
}

// Everything that is written when -paraview writes (cycle 0, ti % vs == 0, the last step): the volume dump and the face dumps, one
// entry of pv_times / pv_cycles (which the collections list and a checkpoint carries) and one density projection for all.
static bool DumpVis(laghos_sim *s, int cycle, const Vector *rho = nullptr)
{
   const Options &o = s->opt;
   if (!o.paraview && !o.FaceDumps()) { return true; }
   s->pv_times.push_back(s->t);
   s->pv_cycles.push_back(cycle);
   if (o.FaceDumps() && !rho)
   {
      s->hydro->ComputeDensity(s->S, s->pv_rho); // rho_gf is refreshed before the output (laghos.cpp:827-830)
      rho = &s->pv_rho;
   }
   if (o.paraview && !DumpParaview(s, cycle, rho)) { return false; }
   return !o.FaceDumps() || DumpFaces(s, cycle, *rho);
}

static std::string Hex32(const unsigned long long fp[2])
{
   char buf[40];
   std::snprintf(buf, sizeof(buf), "%016llX%016llX", fp[0], fp[1]);
   return buf;
}

static bool SimFail(laghos_sim *s, const std::string &msg)
{
   s->error = msg;
   std::fprintf(stderr, "laghos: %s\n", msg.c_str());
   return false;
}

// The fingerprint of this rank's state (own, lgh_vec_fingerprint at offset 0) and of the whole run (all): on one rank the
// same two words; on several ranks the two words of every rank are gathered (lgh_allreduce sums of 32-bit halves, every
// rank contributing its own slots: exact in doubles) and `all` is the host fingerprint of the 2 * nranks words in rank
// order.  Collective on several ranks.
static bool StateFingerprint(laghos_sim *s, unsigned long long own[2], unsigned long long all[2])
{
   const Options &o = s->opt;
   auto &hydro = *s->hydro;
   if (lgh_vec_fingerprint(hydro.Context(), s->S.Read(), s->S.Size(), 0ULL, own) != 0)
   {
      return SimFail(s, std::string("lgh_vec_fingerprint: ") + lgh_last_error());
   }
   all[0] = own[0];
   all[1] = own[1];
   if (o.nranks > 1)
   {
      std::vector<unsigned long long> w(2 * (size_t)o.nranks, 0ULL);
      for (int r = 0; r < o.nranks; r++)
      {
         for (int k = 0; k < 2; k++)
         {
            for (int half = 0; half < 2; half++)
            {
               const double mine = (r == o.rank) ? (double)((own[k] >> (32 * half)) & 0xFFFFFFFFULL) : 0.0;
               w[2 * (size_t)r + k] |= (unsigned long long)hydro.AllReduce(mine, 0) << (32 * half);
            }
         }
      }
      all[0] = all[1] = 0ULL;
      FingerprintWords(w.data(), (long)w.size(), 0ULL, all);
   }
   return true;
}

// One checkpoint of the state after accepted step ti_now: fingerprint on the device, one copy to the host, the host fingerprint of the copy (the two must agree), then
// the file of this rank, CheckpointPiece(stem).  On several ranks an all-reduce follows: every rank learns whether all
// pieces are complete.  Collective.
static bool WriteCheckpointPiece(laghos_sim *s, const std::string &stem, int ti_now, std::string *piece_out)
{
   using clk = std::chrono::steady_clock;
   auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
   const Options &o = s->opt;
   const Discretization &d = *s->disc;
   auto &hydro = *s->hydro;
   const clk::time_point t0 = clk::now();
   unsigned long long own[2], all[2];
   if (!StateFingerprint(s, own, all)) { return false; }
   const clk::time_point t1 = clk::now();
   s->S.ToHost(s->ckpt_host);
   const clk::time_point t2 = clk::now();
   unsigned long long hfp[2] = {0ULL, 0ULL};
   FingerprintWords(s->ckpt_host.data(), (long)s->ckpt_host.size(), 0ULL, hfp);
   bool ok = true;
   std::string err;
   if (hfp[0] != own[0] || hfp[1] != own[1])
   {
      ok = false;
      err = "checkpoint: the state gives " + Hex32(own) + " on the device and " + Hex32(hfp) + " after the copy to the host: not written";
   }
   const std::string piece = CheckpointPiece(stem, o.nranks, o.rank);
   if (ok)
   {
      CheckpointHeader h;
      h.dim = d.dim; h.problem = o.problem; h.order_v = o.order_v; h.order_e = o.order_e; h.Q1D = d.tab.Q1D;
      h.NE = d.NE; h.global_NE = d.global_NE; h.N = d.N;
      h.nranks = o.nranks; h.rank = o.rank;
      for (int a = 0; a < 3; a++) { h.pgrid[a] = d.part.pgrid[a]; }
      h.ode_solver = o.ode_solver_type; h.cfl = o.cfl; h.cg_tol = o.cg_tol; h.cg_max_iter = o.cg_max_iter;
      h.t = s->t; h.dt = s->dt; h.ti = ti_now; h.steps = s->steps; h.repeats = s->repeats;
      h.energy_init = s->energy_init; h.checks = s->checks; h.checks_ok = s->checks_ok ? 1 : 0;
      h.setup_fp[0] = s->setup_fp[0]; h.setup_fp[1] = s->setup_fp[1];
      std::vector<long long> cyc(s->pv_cycles.begin(), s->pv_cycles.end());
      ok = WriteCheckpoint(piece, h, s->ckpt_host.data(), (long)s->ckpt_host.size(), s->pv_times.data(), cyc.data(), (long)cyc.size(), err) == CKPT_OK;
   }
   const clk::time_point t3 = clk::now();
   s->ckpt_seconds[0] += secs(t0, t1);
   s->ckpt_seconds[1] += secs(t1, t2);
   s->ckpt_seconds[2] += secs(t2, t3);
   const double complete = hydro.AllReduce(ok ? 1.0 : 0.0, 0);
   if (!ok) { return SimFail(s, err); }
   if (o.nranks > 1 && complete != (double)o.nranks) { return SimFail(s, "checkpoint " + stem + ": another rank could not write its piece"); }
   s->ckpt_count++;
   if (o.fingerprint && o.rank == 0) { std::cout << "State fingerprint: " << Hex32(all) << " (cycle " << ti_now << ")" << std::endl; }
   if (piece_out) { *piece_out = piece; }
   return true;
}

// The `-ckpt` checkpoint after accepted step ti_now: the pieces, then <basename>_restart/latest (rank 0, once all pieces are
// complete), then -ckpt-keep: each rank removes its own older pieces beyond the K newest, from the list of what this run wrote.
static bool PeriodicCheckpoint(laghos_sim *s, int ti_now)
{
   const Options &o = s->opt;
   const std::string dir = CheckpointDir(o.basename), name = CheckpointName(ti_now);
   std::string piece;
   if (!WriteCheckpointPiece(s, dir + "/" + name, ti_now, &piece)) { return false; }
   if (o.rank == 0 && !WriteLatest(dir, name)) { return SimFail(s, "cannot write " + dir + "/latest"); }
   s->ckpt_mine.erase(std::remove(s->ckpt_mine.begin(), s->ckpt_mine.end(), piece), s->ckpt_mine.end()); // (written again: listed once)
   s->ckpt_mine.push_back(piece);
   while (o.ckpt_keep > 0 && (int)s->ckpt_mine.size() > o.ckpt_keep)
   {
      (void)std::remove(s->ckpt_mine.front().c_str());
      s->ckpt_mine.erase(s->ckpt_mine.begin());
   }
   return true;
}

// One row of the `-hist` file for the state as it stands, cycle `cycle`: the diagnostics on the GPU (collective), the line by rank 0,
// flushed.  Every rank learns whether the row was written.
static bool HistoryRecord(laghos_sim *s, int cycle)
{
   const Options &o = s->opt;
   auto &hydro = *s->hydro;
   double d[LGH_DIAG_COUNT];
   hydro.Diagnostics(s->S, d);
   bool ok = true;
   std::string err;
   if (o.rank == 0) { ok = HistoryAppend(s->hist, HistoryRow(cycle, s->t, s->dt, s->steps, s->repeats, d, s->energy_init), err); }
   const bool all_ok = hydro.AllReduce(ok ? 1.0 : 0.0, 1) == 1.0;
   if (!ok) { return SimFail(s, "cannot write the -hist file: " + err); }
   if (!all_ok) { return SimFail(s, "rank 0 could not write the -hist file"); }
   s->hist_last = cycle;
   return true;
}

// Opens the `-hist` file on rank 0: a new one, or - a restart from cycle `resume_cycle` >= 0 - the existing one with its later rows dropped.
static bool HistoryOpen(laghos_sim *s, int resume_cycle)
{
   const Options &o = s->opt;
   bool ok = true;
   std::string err;
   if (o.rank == 0)
   {
      const std::string path = HistoryPath(o.basename);
      ok = (resume_cycle < 0) ? HistoryStart(s->hist, path, err) : HistoryResume(s->hist, path, resume_cycle, err);
   }
   const bool all_ok = s->hydro->AllReduce(ok ? 1.0 : 0.0, 1) == 1.0;
   if (!ok) { return SimFail(s, "cannot write the -hist file: " + err); }
   if (!all_ok) { return SimFail(s, "rank 0 could not open the -hist file"); }
   s->hist_last = resume_cycle;
   return true;
}

// -prof: axis, origin and range of the profiles.  The default range comes from the INITIAL mesh S0 (which a restart rebuilds as
// every run does), over all ranks: the bounding box along an axis, 0 to the largest distance of a node from the origin for r.
static void ProfileSetup(laghos_sim *s, const std::vector<double> &S0)
{
   const Options &o = s->opt;
   const Discretization &d = *s->disc;
   lgh_profile_spec &sp = s->prof_spec;
   s->prof_axis = o.prof_axis[0];
   sp.axis = (s->prof_axis == 'r') ? 3 : s->prof_axis - 'x';
   sp.nbins = o.prof_bins;
   for (int k = 0; k < 3; k++) { sp.origin[k] = (k < d.dim) ? o.prof_origin[k] : 0.0; }
   sp.lo = o.prof_lo; sp.hi = o.prof_hi;
   if (!o.prof_range_set)
   {
      double lo = INFINITY, hi = -INFINITY;
      for (long n = 0; n < d.N; n++)
      {
         double xi;
         if (sp.axis < 3) { xi = S0[(size_t)sp.axis * d.N + n]; }
         else
         {
            double r2 = 0.0;
            for (int c = 0; c < d.dim; c++) { const double dx = S0[(size_t)c * d.N + n] - sp.origin[c]; r2 += dx * dx; }
            xi = std::sqrt(r2);
         }
         lo = std::min(lo, xi); hi = std::max(hi, xi);
      }
      sp.lo = (sp.axis == 3) ? 0.0 : s->hydro->AllReduce(lo, 1);
      sp.hi = -s->hydro->AllReduce(-hi, 1);
   }
   s->prof_rows.assign((size_t)(sp.nbins + 2) * LGH_PROFILE_COLS, 0.0);
   // the exact solution beside the curves: where -err is accepted (problem 1 on the default mesh, blast at the origin) and the axis is r
   s->prof_exact = o.problem == 1 && o.mesh_file.compare(0, 7, "default") == 0 && sp.axis == 3 && sp.origin[0] == 0.0 && sp.origin[1] == 0.0 &&
                   sp.origin[2] == 0.0;
   if (s->prof_exact && o.rank == 0)
   {
      SedovSol asol(o.dim, 1.4, 1.0, o.blast_energy, 0.0);
      std::copy(asol.par, asol.par + 21, s->prof_par);
   }
}

// The `-prof` file of the state as it stands, cycle `cycle`: the table on the GPU (collective), the file by rank 0.  Every rank
// learns whether it was written.
static bool ProfileRecord(laghos_sim *s, int cycle)
{
   const Options &o = s->opt;
   auto &hydro = *s->hydro;
   const lgh_profile_spec &sp = s->prof_spec;
   long n_excl = 0;
   hydro.Profile(s->S, sp, s->prof_rows.data(), &n_excl);
   bool ok = true;
   std::string err;
   if (o.rank == 0)
   {
      const int R = sp.nbins + 2;
      std::vector<double> exact;
      if (s->prof_exact)
      {
         exact.assign((size_t)3 * R, NAN);
         std::vector<int> row;
         std::vector<double> r, rho, v, p;
         for (int k = 0; k < R && s->t > 0.0; k++) // (t = 0: the blast has no extent yet; rows without mass have no xi)
         {
            const double *d = s->prof_rows.data() + (size_t)k * LGH_PROFILE_COLS;
            if (d[2] != 0.0 && std::isfinite(d[7] / d[2])) { row.push_back(k); r.push_back(d[7] / d[2]); }
         }
         if (!r.empty()) { hydro.SedovEval(s->prof_par, s->t, r, rho, v, p); }
         for (size_t j = 0; j < row.size(); j++) { exact[3 * row[j]] = rho[j]; exact[3 * row[j] + 1] = v[j]; exact[3 * row[j] + 2] = p[j]; }
      }
      ok = ProfileWrite(ProfilePath(o.basename, cycle),
                        ProfileText(cycle, s->t, s->prof_axis, sp.origin, sp.lo, sp.hi, sp.nbins, n_excl, s->prof_rows.data(),
                                    s->prof_exact ? exact.data() : nullptr),
                        err);
   }
   const bool all_ok = hydro.AllReduce(ok ? 1.0 : 0.0, 1) == 1.0;
   if (!ok) { return SimFail(s, "cannot write the -prof file: " + err); }
   if (!all_ok) { return SimFail(s, "rank 0 could not write the -prof file"); }
   s->prof_last = cycle;
   s->prof_files++;
   return true;
}

// -map: the grid.  The default box is the extent of the INITIAL mesh S0 per axis over all ranks (as ProfileSetup takes its
// default range: a restart rebuilds S0 as every run does and so reproduces it).
static void MapSetup(laghos_sim *s, const std::vector<double> &S0)
{
   const Options &o = s->opt;
   const Discretization &d = *s->disc;
   lgh_map_spec &sp = s->map_spec;
   size_t ncells = 1;
   for (int c = 0; c < 3; c++)
   {
      sp.n[c] = (c < d.dim) ? o.map_cells[c] : 1;
      sp.lo[c] = 0.0; sp.hi[c] = 1.0;
      ncells *= (size_t)sp.n[c];
      if (c >= d.dim) { continue; }
      if (o.map_box_n > 0) { sp.lo[c] = o.map_box[2 * c]; sp.hi[c] = o.map_box[2 * c + 1]; continue; }
      double lo = INFINITY, hi = -INFINITY;
      for (long n = 0; n < d.N; n++)
      {
         const double x = S0[(size_t)c * d.N + n];
         lo = std::min(lo, x); hi = std::max(hi, x);
      }
      sp.lo[c] = s->hydro->AllReduce(lo, 1);
      sp.hi[c] = -s->hydro->AllReduce(-hi, 1);
   }
   s->map_rows.assign((ncells + 1) * LGH_MAP_COLS, 0.0);
}

// The `-map` file of the state as it stands, cycle `cycle`: the rows on the GPU (collective), the file by rank 0.  Every rank
// learns whether it was written.
static bool MapRecord(laghos_sim *s, int cycle)
{
   const Options &o = s->opt;
   auto &hydro = *s->hydro;
   const lgh_map_spec &sp = s->map_spec;
   long n_excl = 0;
   hydro.Map(s->S, sp, s->map_rows.data(), &n_excl);
   bool ok = true;
   std::string err;
   if (o.rank == 0) { ok = WriteVti(MapDir(o.basename), s->disc->dim, sp.n, sp.lo, sp.hi, s->map_rows.data(), n_excl, cycle, s->t, err); }
   const bool all_ok = hydro.AllReduce(ok ? 1.0 : 0.0, 1) == 1.0;
   if (!ok) { return SimFail(s, "cannot write the -map file: " + err); }
   if (!all_ok) { return SimFail(s, "rank 0 could not write the -map file"); }
   s->map_last = cycle;
   s->map_files++;
   return true;
}

extern "C"
{

const char *laghos_sim_error(laghos_sim *s) { return s ? s->error.c_str() : "null sim"; }

// argv: the reference's command-line options; nranks/rank/nccl_id describe the
// process group (nccl_id: 128 bytes from lgh_comm_unique_id, may be NULL for 1 rank)
laghos_sim *laghos_sim_create(int argc, const char *const *argv, int nranks, int rank,
                              const char *nccl_id)
{
   std::unique_ptr<laghos_sim> s(new laghos_sim());
   Options &o = s->opt;
   o.nranks = nranks;
   o.rank = rank;
   o.nccl_id = nccl_id;
   std::string err;
   if (!ParseArgs(argc, argv, o, err))
   {
      std::fprintf(stderr, "laghos: %s\n", err.c_str());
      return nullptr;
   }
   if (o.check_exact_sedov) // laghos.cpp:303-309
   {
      if (o.problem != 1)
      {
         std::fprintf(stderr, "Can only compare problem 1 (Sedov) against the exact solution\n");
         return nullptr;
      }
      if (o.mesh_file.compare(0, 7, "default") != 0)
      {
         std::fprintf(stderr, "check: mesh_file\n");
         return nullptr;
      }
   }
   try
   {
      CartMesh mesh = (o.mesh_file.compare(0, 7, "default") == 0)
                         ? CartMesh::Cartesian(o.dim, o.nx, o.ny, o.nz, o.Sx, o.Sy, o.Sz)
                         : CartMesh::Named(o.mesh_file);
      for (int l = 0; l < o.rs_levels + o.rp_levels; l++) { mesh.UniformRefinement(); } // laghos.cpp:391, :483
      o.dim = mesh.dim;
      if (o.dim == 1 && o.p_assembly) // laghos.cpp:454-462: 1D runs the FA path
      {
         o.p_assembly = false;
         if (rank == 0 && !o.quiet) { std::cout << "Laghos does not support PA in 1D. Switching to FA." << std::endl; }
      }
      if (o.dim == 1 && (o.pv_fields & hydrodynamics::LagrangianHydroOperator::DERIVED_VORT))
      {
         if (o.pv_vort_named)
         {
            std::fprintf(stderr, "laghos: -pv-fields vorticity: there is no vorticity in 1D\n");
            return nullptr;
         }
         o.pv_fields &= ~(unsigned)hydrodynamics::LagrangianHydroOperator::DERIVED_VORT; // (all)
      }
      if (o.FaceDumps() && o.dim == 1)
      {
         std::fprintf(stderr, "laghos: %s: zone faces are dumped in 2D and 3D, this mesh is 1D (its -paraview dump is small already)\n",
                      o.pv_surface ? "-pv-surface" : "-pv-slice");
         return nullptr;
      }
      for (const auto &sl : o.pv_slices)
      {
         const char ax = (char)('x' + sl.first);
         if (sl.first >= o.dim)
         {
            std::fprintf(stderr, "laghos: -pv-slice %c %d: the mesh has %d dimensions, there is no %c axis\n", ax, sl.second, o.dim, ax);
            return nullptr;
         }
         if (sl.second > mesh.ne(sl.first))
         {
            std::fprintf(stderr, "laghos: -pv-slice %c %d: K is out of range, the zone grid has node planes 0..%d along %c\n", ax, sl.second,
                         mesh.ne(sl.first), ax);
            return nullptr;
         }
      }
      if (o.prof_axis.empty()) { o.prof_axis = (o.problem == 1) ? "r" : "x"; }
      if (o.prof_steps > 0 && o.prof_axis != "r" && o.prof_axis[0] - 'x' >= o.dim)
      {
         std::fprintf(stderr, "laghos: -prof-axis %s needs a mesh of %d dimensions, this one has %d\n", o.prof_axis.c_str(), o.prof_axis[0] - 'x' + 1, o.dim);
         return nullptr;
      }
      if (o.map_steps > 0)
      {
         if (o.map_cells_n > 0 && o.map_cells_n != o.dim)
         {
            std::fprintf(stderr, "laghos: -map-cells has %d counts, the mesh has %d dimensions\n", o.map_cells_n, o.dim);
            return nullptr;
         }
         if (o.map_box_n > 0 && o.map_box_n != 2 * o.dim)
         {
            std::fprintf(stderr, "laghos: -map-box has %d numbers, a mesh of %d dimensions needs %d\n", o.map_box_n, o.dim, 2 * o.dim);
            return nullptr;
         }
         double ncells = 1.0;
         for (int c = 0; c < o.dim; c++) { ncells *= (double)o.map_cells[c]; }
         if (ncells > (double)LGH_MAP_MAX_CELLS)
         {
            std::fprintf(stderr, "laghos: -map-cells asks for %.0f cells, at most %d fit\n", ncells, LGH_MAP_MAX_CELLS);
            return nullptr;
         }
      }
      if (!o.p_assembly && o.dim != 1)
      {
         std::fprintf(stderr, "laghos: only the partial-assembly path (-pa) is implemented\n");
         return nullptr;
      }
      const char *force_multi = std::getenv("LGH_FORCE_MULTI");
      if (o.dim == 1 && force_multi && force_multi[0] == '1')
      {
         std::fprintf(stderr, "laghos: LGH_FORCE_MULTI=1 drives the multi-rank path, which 1D does not have\n");
         return nullptr;
      }
      s->disc.reset(new Discretization(mesh, o.order_v, o.order_e, o.problem, nranks, rank, o.order_q, o.blast_energy));
      s->disc->impose_visc = o.impose_visc;
      s->disc->Renumber(o.renumber, o.rs_levels + o.rp_levels, (unsigned)o.renumber_seed);
   }
   catch (const std::exception &e)
   {
      std::fprintf(stderr, "laghos: %s\n", e.what());
      return nullptr;
   }
   const Discretization &d = *s->disc;
   const bool root = (rank == 0) && !o.quiet;
   if (root)
   {
      std::cout << "Number of zones in the serial mesh: " << d.global_NE << std::endl;
      std::cout << "Number of kinematic (position, velocity) dofs: " << (long)d.dim * d.global_N << std::endl;
      std::cout << "Number of specific internal energy dofs: " << d.global_NE * d.NL << std::endl;
   }
   std::vector<double> S0, rho0_l2, gamma, rho0_q;
   d.InitialState(S0, rho0_l2, gamma, rho0_q);
   // -restart: read and verify the file, compare it with what THIS command line sets up (setup_fp: mesh, refinement, orders,
   // problem, -E0, numbering and partition all end up in these arrays) - host work, before any GPU call
   const bool restarting = !o.restart.empty();
   Checkpoint ck;
   std::string ck_piece;
   if (restarting || o.ckpt_steps > 0) { SetupFingerprint(S0, rho0_l2, gamma, rho0_q, d.h1map, s->setup_fp); }
   if (restarting)
   {
      std::string stem = o.restart, err;
      if (stem == "latest")
      {
         std::string name;
         const std::string dir = CheckpointDir(o.basename);
         if (!ReadLatest(dir, name))
         {
            std::fprintf(stderr, "laghos: -restart latest: cannot read %s/latest\n", dir.c_str());
            return nullptr;
         }
         stem = dir + "/" + name;
      }
      ck_piece = CheckpointPiece(stem, nranks, rank);
      if (ReadCheckpoint(ck_piece, ck, err) != CKPT_OK)
      {
         std::fprintf(stderr, "laghos: -restart: %s\n", err.c_str());
         return nullptr;
      }
      const CheckpointHeader &h = ck.h;
      std::string why;
      if (h.nranks != nranks || h.rank != rank)
      {
         why = "it is the piece of rank " + std::to_string(h.rank) + " of " + std::to_string(h.nranks) + ", this is rank " + std::to_string(rank) + " of " +
               std::to_string(nranks) + " (a restart onto another rank count is not supported)";
      }
      else if (h.pgrid[0] != d.part.pgrid[0] || h.pgrid[1] != d.part.pgrid[1] || h.pgrid[2] != d.part.pgrid[2]) { why = "it was written on another process grid"; }
      else if (h.setup_fp[0] != s->setup_fp[0] || h.setup_fp[1] != s->setup_fp[1])
      {
         why = "setup_fp: its run was set up differently (mesh, refinement, orders, problem, -E0, numbering or partition): the file has " + Hex32(h.setup_fp) +
               ", this command line gives " + Hex32(s->setup_fp);
      }
      else if (h.state_words != (long)S0.size() || h.dim != d.dim || h.NE != d.NE || h.N != d.N || h.global_NE != d.global_NE)
      {
         why = "sizes: its state has " + std::to_string(h.state_words) + " words, this run's " + std::to_string(S0.size());
      }
      if (!why.empty())
      {
         std::fprintf(stderr, "laghos: -restart: checkpoint %s refused: %s\n", ck_piece.c_str(), why.c_str());
         return nullptr;
      }
   }
   s->hydro.reset(new hydrodynamics::LagrangianHydroOperator(d, S0, rho0_l2, gamma, rho0_q, o.cfl, o.cg_tol,
                                                             o.cg_max_iter, o.dev, nccl_id));
   switch (o.ode_solver_type)
   {
      case 1: s->ode.reset(new ForwardEulerSolver); break;
      case 2: s->ode.reset(new RK2Solver(0.5)); break;
      case 3: s->ode.reset(new RK3SSPSolver); break;
      case 4: s->ode.reset(new RK4Solver); break;
      case 6: s->ode.reset(new RK6Solver); break;
      case 7: s->ode.reset(new RK2AvgSolver); break;
      default:
         std::fprintf(stderr, "Unknown ODE solver type: %d\n", o.ode_solver_type); // laghos.cpp:527-531
         return nullptr;
   }
   // RK1-4 / RK6 give every SolveEnergy the velocity block of the state the quadrature data was updated for: F.1 and
   // F^T v both come out of the update kernel and nobody reads qdata.stressJinvT - it is not written then.  RK2Avg
   // (laghos_solver.cpp:1464-1480) solves the energy equation for an averaged velocity: the stress stays in memory.
   // (-store-stress / LGH_STORE_STRESS=1 keep it in memory in any case.)
   {
      const char *senv = std::getenv("LGH_STORE_STRESS");
      const bool keep_in_registers = o.ode_solver_type != 7 && d.dim == 3 && !o.store_stress && !(senv && senv[0] == '1');
      if (keep_in_registers) { LGH_VERIFY(lgh_qupdate_store_stress(s->hydro->Context(), 0)); }
   }
   if (o.prof_steps > 0) { ProfileSetup(s.get(), S0); }
   if (o.map_steps > 0) { MapSetup(s.get(), S0); }
   if (o.pv_surface)
   {
      s->pv_faces.emplace_back();
      s->pv_faces.back().tag = "surface";
      s->pv_faces.back().faces = SelectFaces(d, -1, 0);
   }
   for (const auto &sl : o.pv_slices)
   {
      s->pv_faces.emplace_back();
      s->pv_faces.back().tag = std::string("slice_") + (char)('x' + sl.first) + std::to_string(sl.second);
      s->pv_faces.back().faces = SelectFaces(d, sl.first, sl.second);
   }
   if (restarting)
   {
      // the set-up data came from S0 as in every run; the state now comes from the file and must have arrived in HBM intact
      const CheckpointHeader &h = ck.h;
      s->S.FromHost(ck.S);
      s->S_old.SetSize(s->S.Size());
      s->ode->Init(*s->hydro);
      unsigned long long dfp[2];
      if (lgh_vec_fingerprint(s->hydro->Context(), s->S.Read(), s->S.Size(), 0ULL, dfp) != 0 || dfp[0] != h.state_fp[0] || dfp[1] != h.state_fp[1])
      {
         std::fprintf(stderr, "laghos: -restart: checkpoint %s: the state on the device gives %s, state_fp is %s\n", ck_piece.c_str(),
                      Hex32(dfp).c_str(), Hex32(h.state_fp).c_str());
         return nullptr;
      }
      // the quadrature data current for S, as the end of step ti left it in the uninterrupted run (the estimate itself is not
      // needed: dt comes from the file)
      s->hydro->ResetTimeStepEstimate();
      (void)s->hydro->GetTimeStepEstimate(s->S);
      s->t = h.t; s->dt = h.dt; s->ti = h.ti + 1; s->steps = h.steps; s->repeats = h.repeats;
      s->steps_at_start = h.steps;
      s->energy_init = h.energy_init; s->checks = h.checks; s->checks_ok = h.checks_ok != 0;
      s->pv_times = ck.pv_times;
      s->pv_cycles.assign(ck.pv_cycles.begin(), ck.pv_cycles.end());
      if (nranks > 1) // pieces of different checkpoints?
      {
         const double ti_min = s->hydro->AllReduce((double)h.ti, 1), ti_max = -s->hydro->AllReduce(-(double)h.ti, 1);
         const double t_min = s->hydro->AllReduce(h.t, 1), t_max = -s->hydro->AllReduce(-h.t, 1);
         if (ti_min != ti_max || t_min != t_max)
         {
            std::fprintf(stderr, "laghos: -restart: checkpoint %s refused: the ranks read pieces of different checkpoints (cycles %d .. %d)\n",
                         ck_piece.c_str(), (int)ti_min, (int)ti_max);
            return nullptr;
         }
      }
      if (rank == 0)
      {
         if (h.ode_solver != o.ode_solver_type) { std::cout << "Restart: -s was " << h.ode_solver << " in the checkpoint, continuing with " << o.ode_solver_type << std::endl; }
         if (h.cfl != o.cfl) { std::cout << "Restart: -cfl was " << h.cfl << " in the checkpoint, continuing with " << o.cfl << std::endl; }
         if (h.cg_tol != o.cg_tol) { std::cout << "Restart: -cgt was " << h.cg_tol << " in the checkpoint, continuing with " << o.cg_tol << std::endl; }
         if (h.cg_max_iter != o.cg_max_iter) { std::cout << "Restart: -cgm was " << h.cg_max_iter << " in the checkpoint, continuing with " << o.cg_max_iter << std::endl; }
      }
      if (root)
      {
         std::cout << "Restarting from " << ck_piece << ": cycle " << h.ti << ", t = " << std::setprecision(17) << s->t << ", dt = " << s->dt
                   << std::setprecision(6) << std::endl;
      }
      if (o.hist_steps > 0 && !HistoryOpen(s.get(), h.ti)) { return nullptr; } // (no row for the checkpoint's own state: the run that wrote it has)
      s->prof_last = h.ti;                                                     // (nor a profile)
      s->map_last = h.ti;                                                      // (nor a map)
      // a checkpoint written after the last step: nothing is left to do
      if (s->t >= o.t_final || (o.max_tsteps >= 0 && s->steps > o.max_tsteps)) { s->last_step = true; }
      return s.release();
   }
   s->S.FromHost(S0);
   s->S_old.SetSize(s->S.Size());
   s->ode->Init(*s->hydro);
   s->energy_init = s->hydro->InternalEnergy(s->S) + s->hydro->KineticEnergy(s->S); // laghos.cpp:664
   s->hydro->ResetTimeStepEstimate();                                                // :707
   s->t = 0.0;
   s->dt = s->hydro->GetTimeStepEstimate(s->S);                                      // :708
   if (!DumpVis(s.get(), 0)) { return nullptr; }                                      // :691-701
   if (o.hist_steps > 0 && !(HistoryOpen(s.get(), -1) && HistoryRecord(s.get(), 0))) { return nullptr; }
   if (o.prof_steps > 0 && !ProfileRecord(s.get(), 0)) { return nullptr; }
   if (o.map_steps > 0 && !MapRecord(s.get(), 0)) { return nullptr; }
   return s.release();
}

void laghos_sim_destroy(laghos_sim *s) { delete s; }

// One pass of the reference time loop body (laghos.cpp:742-920): advances one
// ACCEPTED step (repeating with dt*0.85 as needed).  Returns 1 if a step was
// taken, 0 when the run is finished.
int laghos_sim_step(laghos_sim *s)
{
   Options &o = s->opt;
   auto &hydro = *s->hydro;
   const bool root = (o.rank == 0) && !o.quiet;
   while (true)
   {
      if (s->last_step) { return 0; }
      if (s->t + s->dt >= o.t_final)
      {
         s->dt = o.t_final - s->t;
         s->last_step = true;
      }
      if (s->steps == o.max_tsteps) { s->last_step = true; }
      hydro.Copy(s->S_old, s->S);
      s->t_old = s->t;
      hydro.ResetTimeStepEstimate();
      s->ode->Step(s->S, s->t, s->dt);
      s->steps++;
      // Adaptive time step control (laghos.cpp:762-778)
      const double dt_est = hydro.GetTimeStepEstimate(s->S);
      if (dt_est < s->dt)
      {
         s->dt *= 0.85;
         if (s->dt < std::numeric_limits<double>::epsilon())
         {
            s->error = "The time step crashed!";
            std::fprintf(stderr, "%s\n", s->error.c_str());
            return -1;
         }
         s->t = s->t_old;
         hydro.Copy(s->S, s->S_old);
         hydro.ResetQuadratureData();
         s->repeats++;
         if (root) { std::cout << "Repeating step " << s->ti << std::endl; }
         if (s->steps < o.max_tsteps) { s->last_step = false; }
         // The run ends here when its last step was a repeated one (the loop of laghos.cpp:742-778 has no step left to take):
         // the state is that of the last accepted step again, with the shortened dt - the checkpoint "after the last step"
         if (s->last_step && o.ckpt_steps > 0 && s->ti > 1 && !PeriodicCheckpoint(s, s->ti - 1)) { return -1; }
         // ... and the row "after the last step", unless that step has its row already (repeated steps themselves write none)
         if (s->last_step && o.hist_steps > 0 && s->ti - 1 > s->hist_last && !HistoryRecord(s, s->ti - 1)) { return -1; }
         if (s->last_step && o.prof_steps > 0 && s->ti - 1 > s->prof_last && !ProfileRecord(s, s->ti - 1)) { return -1; } // (the same rule)
         if (s->last_step && o.map_steps > 0 && s->ti - 1 > s->map_last && !MapRecord(s, s->ti - 1)) { return -1; }        // (and here)
         continue;
      }
      else if (dt_est > 1.25 * s->dt) { s->dt *= 1.02; }

      if (s->last_step || (s->ti % o.vis_steps) == 0)
      {
         const double sqrt_norm = hydro.ENorm(s->S);
         if (root)
         {
            std::cout << std::fixed;
            std::cout << "step " << std::setw(5) << s->ti << ",\tt = " << std::setw(5) << std::setprecision(4)
                      << s->t << ",\tdt = " << std::setw(5) << std::setprecision(6) << s->dt
                      << ",\t|e| = " << std::setprecision(10) << std::scientific << sqrt_norm;
            std::cout << std::fixed << std::endl;
         }
         Vector rho;
         if (o.gfprint) // laghos.cpp:873-900
         {
            std::vector<double> Sh, rhoh;
            hydro.ComputeDensity(s->S, rho); // laghos.cpp:827-830 (rho_gf is refreshed before the output)
            hydro.Sync();
            s->S.ToHost(Sh);
            rho.ToHost(rhoh);
            if (!WriteFields(o.basename, s->ti, *s->disc, o.nranks, o.rank, Sh, rhoh))
            {
               s->error = "cannot write the -print files under " + o.basename;
               std::fprintf(stderr, "%s\n", s->error.c_str());
               return -1;
            }
         }
         if (!DumpVis(s, s->ti, o.gfprint ? &rho : nullptr)) { return -1; } // laghos.cpp:845-871 (one projection for all)
      }
      if (o.check)
      {
         const double e_norm = hydro.ENorm(s->S);
         s->checks_ok = CheckNorm(o.dim, o.problem, s->ti, e_norm, s->checks) && s->checks_ok;
      }
      if (o.ckpt_steps > 0 && (s->last_step || (s->ti % o.ckpt_steps) == 0) && !PeriodicCheckpoint(s, s->ti)) { return -1; }
      if (o.hist_steps > 0 && (s->last_step || (s->ti % o.hist_steps) == 0) && !HistoryRecord(s, s->ti)) { return -1; }
      if (o.prof_steps > 0 && (s->last_step || (s->ti % o.prof_steps) == 0) && !ProfileRecord(s, s->ti)) { return -1; }
      if (o.map_steps > 0 && (s->last_step || (s->ti % o.map_steps) == 0) && !MapRecord(s, s->ti)) { return -1; }
      s->ti++;
      return 1;
   }
}

// `-err` (laghos.cpp:1007-1086): L2 error of the density against the exact Sedov solution at
// t_final.  Returns a negative value (and sets the error string) when the exact shock has
// reached the boundary of the default mesh.
double laghos_sim_sedov_error(laghos_sim *s)
{
   const Options &o = s->opt;
   const double gamma = 1.4, rho0 = 1, omega = 0;
   SedovSol asol(o.dim, gamma, rho0, o.blast_energy, omega);
   asol.SetTime(o.t_final);
   const double min_r = std::min(std::min(o.Sx, o.Sy), o.Sz);
   if (!(asol.r2 <= min_r))
   {
      s->error = "Solution reflections off boundaries detected, cannot compare against exact solution.";
      std::fprintf(stderr, "%s\n", s->error.c_str());
      return -1.0;
   }
   const int err_order = std::max((std::max(o.order_v, o.order_e) + 1) * 2, o.order_q) * 2;
   const double blast_position[3] = {0.0, 0.0, 0.0};
   Vector rho;
   s->hydro->ComputeDensity(s->S, rho);
   return s->hydro->SedovDensityError(s->S, rho, asol.par, o.t_final, blast_position, err_order);
}

// state / metrics access for bench.py
double laghos_sim_time(laghos_sim *s) { return s->t; }
double laghos_sim_dt(laghos_sim *s) { return s->dt; }
int laghos_sim_steps(laghos_sim *s) { return s->steps; }   // RK steps taken incl. repeated ones
int laghos_sim_ti(laghos_sim *s) { return s->ti - 1; }     // accepted steps
int laghos_sim_repeats(laghos_sim *s) { return s->repeats; } // repeated steps so far
void laghos_sim_checks(laghos_sim *s, int *out) { out[0] = s->checks; out[1] = s->checks_ok ? 1 : 0; } // -chk: cycles compared, all passed
// The state fingerprint `-fp` prints: out[0] = sum, out[1] = xor word (include/lgh_fingerprint.h).  One rank: lgh_vec_fingerprint
// of S at offset 0; several ranks: the rank-ordered combination (collective).  0 = ok.
int laghos_sim_fingerprint(laghos_sim *s, unsigned long long *out)
{
   unsigned long long own[2];
   return StateFingerprint(s, own, out) ? 0 : -1;
}
// A checkpoint of the sim as it stands between two steps, to the stem given (rank r of several writes <stem>.<r>; collective).
// No `latest`, no -ckpt-keep.  0 = written; laghos_sim_error() has the message otherwise.
int laghos_sim_write_checkpoint(laghos_sim *s, const char *stem)
{
   if (!s || !stem || !*stem) { return -1; }
   if (s->setup_fp[0] == 0 && s->setup_fp[1] == 0)
   {
      std::vector<double> S0, rho0_l2, gamma, rho0_q;
      s->disc->InitialState(S0, rho0_l2, gamma, rho0_q);
      SetupFingerprint(S0, rho0_l2, gamma, rho0_q, s->disc->h1map, s->setup_fp);
   }
   return WriteCheckpointPiece(s, stem, s->ti - 1, nullptr) ? 0 : -1;
}
double laghos_sim_enorm(laghos_sim *s) { return s->hydro->ENorm(s->S); }
// The LGH_DIAG_COUNT doubles of lgh_diagnostics for the state as it stands (collective on several ranks)
void laghos_sim_diagnostics(laghos_sim *s, double *out) { s->hydro->Diagnostics(s->S, out); }
// lgh_profile of the state as it stands (collective on several ranks): axis 0..2 or 3 = r, rows = (nbins + 2) x LGH_PROFILE_COLS
// doubles, origin = 3 doubles.  0 = ok; otherwise laghos_sim_error() has the library's message and nothing was written.
int laghos_sim_profile(laghos_sim *s, int axis, int nbins, double lo, double hi, const double *origin, double *rows, long *n_excluded)
{
   lgh_profile_spec sp = {};
   sp.axis = axis; sp.nbins = nbins; sp.lo = lo; sp.hi = hi;
   for (int k = 0; k < 3; k++) { sp.origin[k] = origin ? origin[k] : 0.0; }
   const int rc = lgh_profile(s->hydro->Context(), s->S.Read(), &sp, rows, n_excluded);
   if (rc != 0) { s->error = lgh_last_error(); }
   return rc;
}
// lgh_map of the state as it stands (collective on several ranks): n, lo, hi = 3 values each, rows = (n[0] n[1] n[2] + 1) x
// LGH_MAP_COLS doubles.  0 = ok; otherwise laghos_sim_error() has the library's message and nothing was written.
int laghos_sim_map(laghos_sim *s, const int *n, const double *lo, const double *hi, double *rows, long *n_excluded)
{
   if (!n || !lo || !hi) { s->error = "laghos_sim_map: NULL grid"; return LGH_ERR_ARG; }
   lgh_map_spec sp = {};
   for (int k = 0; k < 3; k++) { sp.n[k] = n[k]; sp.lo[k] = lo[k]; sp.hi[k] = hi[k]; }
   const int rc = lgh_map(s->hydro->Context(), s->S.Read(), &sp, rows, n_excluded);
   if (rc != 0) { s->error = lgh_last_error(); }
   return rc;
}
// lgh_sample_derived of the state as it stands on the lattice of R cells per zone and direction (1 <= R <= 8), into host arrays
// in the layouts of that entry: detj, div, cs NP = NE (R+1)^dim doubles, gradv dim^2 NP, vort NP (2D) or 3 NP (3D); each may be
// NULL.  0 = ok; -1 with laghos_sim_error() set for an R out of range or vort in 1D, and nothing was written.
int laghos_sim_derived_fields(laghos_sim *s, int R, double *detj, double *gradv, double *div, double *vort, double *cs)
{
   using H = hydrodynamics::LagrangianHydroOperator;
   const int dim = s->disc->dim, nv = (dim == 3) ? 3 : (dim == 2 ? 1 : 0);
   if (R < 1 || R > 8) { s->error = "laghos_sim_derived_fields: R = " + std::to_string(R) + " is out of range (1 <= R <= 8)"; return -1; }
   if (vort && dim == 1) { s->error = "laghos_sim_derived_fields: vort: there is no vorticity in 1D"; return -1; }
   const unsigned mask = (detj ? H::DERIVED_DETJ : 0) | (gradv ? H::DERIVED_GRAD : 0) | (div ? H::DERIVED_DIV : 0) | (vort ? H::DERIVED_VORT : 0) |
                         (cs ? H::DERIVED_CS : 0);
   if (!mask) { return 0; }
   const long NP = s->hydro->SamplePoints(R);
   Vector dev;
   std::vector<double> h;
   s->hydro->SampleDerived(s->S, R, mask, dev);
   s->hydro->Sync();
   dev.ToHost(h);
   const double *p = h.data();
   auto take = [&](double *dst, long n) { if (dst) { std::memcpy(dst, p, n * sizeof(double)); } p += n; };
   take(detj, NP); take(gradv, (long)dim * dim * NP); take(div, NP); take(vort, nv * NP); take(cs, NP);
   return 0;
}
// The face lists of the driver's dumps for this rank: kind 0 the boundary of the global mesh (`-pv-surface`), kind 1 node plane K
// along axis 0..2 (`-pv-slice`).  Returns the number of faces, -1 with laghos_sim_error() set for a bad selection; faces (may be
// NULL: count only) takes the (zone, local face) pairs.
int laghos_sim_select_faces(laghos_sim *s, int kind, int axis, int K, int *faces)
{
   const Discretization &d = *s->disc;
   if (d.dim == 1) { s->error = "laghos_sim_select_faces: zone faces are sampled in 2D and 3D"; return -1; }
   if (kind != 0 && (kind != 1 || axis < 0 || axis >= d.dim || K < 0 || K > d.mesh.ne(axis)))
   {
      s->error = "laghos_sim_select_faces: kind " + std::to_string(kind) + ", axis " + std::to_string(axis) + ", K " + std::to_string(K) + " is no surface or slice of this mesh";
      return -1;
   }
   const std::vector<int> f = SelectFaces(d, kind == 0 ? -1 : axis, K);
   if (faces) { std::copy(f.begin(), f.end(), faces); }
   return (int)f.size() / 2;
}
// lgh_sample_faces of the state as it stands on the lattice of R cells per direction (1 <= R <= 8) of nfaces faces, all outputs,
// into one host array of LagrangianHydroOperator::FacesSize doubles in the blocks of SampleFaces.  0 = ok; -1 with
// laghos_sim_error() set.
int laghos_sim_face_fields(laghos_sim *s, int R, int nfaces, const int *faces, double *out)
{
   using H = hydrodynamics::LagrangianHydroOperator;
   const Discretization &d = *s->disc;
   if (R < 1 || R > 8) { s->error = "laghos_sim_face_fields: R = " + std::to_string(R) + " is out of range (1 <= R <= 8)"; return -1; }
   if (d.dim == 1 || nfaces < 0 || (nfaces > 0 && (!faces || !out))) { s->error = "laghos_sim_face_fields: 1D, or a NULL argument"; return -1; }
   for (int k = 0; k < nfaces; k++)
   {
      if (faces[2 * k] < 0 || faces[2 * k] >= d.NE || faces[2 * k + 1] < 0 || faces[2 * k + 1] >= 2 * d.dim)
      {
         s->error = "laghos_sim_face_fields: face " + std::to_string(k) + " = (" + std::to_string(faces[2 * k]) + ", " + std::to_string(faces[2 * k + 1]) + ") is out of range";
         return -1;
      }
   }
   if (nfaces == 0) { return 0; }
   laghos_sim::FaceSet fs;
   fs.faces.assign(faces, faces + 2 * (size_t)nfaces);
   Vector rho;
   s->hydro->ComputeDensity(s->S, rho);
   std::vector<double> h;
   double secs[2] = {0, 0};
   SampleFaceSet(s, fs, rho, R, H::DERIVED_ALL, h, secs);
   std::memcpy(out, h.data(), (size_t)s->hydro->FacesSize(R, nfaces) * sizeof(double));
   return 0;
}
double laghos_sim_energy(laghos_sim *s) { return s->hydro->InternalEnergy(s->S) + s->hydro->KineticEnergy(s->S); }
void laghos_sim_sync(laghos_sim *s) { s->hydro->Sync(); }
void laghos_sim_enable_timers(laghos_sim *s, int on) { s->hydro->EnableTimers(on != 0); }
void laghos_sim_reset_timers(laghos_sim *s) { s->hydro->ResetTiming(); }
// t[0..3] = cgH1, cgL2, force, qdata seconds; c[0..2] = H1iter, L2iter, quad_tstep
void laghos_sim_timers(laghos_sim *s, double *t, long *c)
{
   const auto &tm = s->hydro->Timing();
   t[0] = tm.sw_cgH1; t[1] = tm.sw_cgL2; t[2] = tm.sw_force; t[3] = tm.sw_qdata;
   c[0] = tm.H1iter; c[1] = tm.L2iter; c[2] = tm.quad_tstep;
}
// sizes: [dim, local NE, global NE, local N, global H1 vdofs, global L2 dofs, NQ, D1D, Q1D, L1D]
void laghos_sim_sizes(laghos_sim *s, long *out)
{
   const Discretization &d = *s->disc;
   out[0] = d.dim; out[1] = d.NE; out[2] = d.global_NE; out[3] = d.N;
   out[4] = s->hydro->GlobalH1Size(); out[5] = s->hydro->GlobalL2Size();
   out[6] = d.NQ; out[7] = d.tab.D1D; out[8] = d.tab.Q1D; out[9] = d.tab.L1D;
   for (int a = 0; a < 3; a++)
   {
      out[10 + a] = d.part.pgrid[a];               // process grid
      out[13 + a] = a < d.dim ? d.part.ne[a] : 1;  // local zones per axis
   }
}
// host-only: the process grid Partition picks for an nx x ny x nz zone grid on nranks ranks
// (bench.py derives its weak-scaling mesh from it); returns 0, or -1 if the grid cannot be split evenly
int laghos_host_partition(int dim, int nx, int ny, int nz, int nranks, int *pgrid)
{
   try
   {
      CartMesh m = CartMesh::Cartesian(dim, nx, ny, nz, 1.0, 1.0, 1.0);
      Partition p(m, nranks, 0);
      for (int a = 0; a < 3; a++) { pgrid[a] = p.pgrid[a]; }
      return 0;
   }
   catch (const std::exception &)
   {
      return -1;
   }
}
void *laghos_sim_context(laghos_sim *s) { return s->hydro->Context(); }
long laghos_sim_state_size(laghos_sim *s) { return s->S.Size(); }
void laghos_sim_get_state(laghos_sim *s, double *host) // for tests
{
   std::vector<double> h;
   s->hydro->Sync();
   s->S.ToHost(h);
   std::memcpy(host, h.data(), h.size() * sizeof(double));
}

// host-only probes of the setup code (no GPU): tests compare them with the oracle
int laghos_host_tables(int order_v, int order_e, double *qpts, double *qwts, double *gll, double *B,
                       double *G, double *Bl)
{
   Tables t(order_v, order_e);
   std::memcpy(qpts, t.qpts.data(), t.qpts.size() * sizeof(double));
   std::memcpy(qwts, t.qwts.data(), t.qwts.size() * sizeof(double));
   std::memcpy(gll, t.gll.data(), t.gll.size() * sizeof(double));
   std::memcpy(B, t.B.data(), t.B.size() * sizeof(double));
   std::memcpy(G, t.G.data(), t.G.size() * sizeof(double));
   std::memcpy(Bl, t.Bl.data(), t.Bl.size() * sizeof(double));
   return t.Q1D;
}
// host-only: the 1-D bases at the lattice abscissae r/R of the visualisation sampling, B_h1_lat[r + (R+1)*d] ((R+1)*(order_v+1)),
// B_l2_lat[r + (R+1)*l] ((R+1)*(order_e+1))
int laghos_host_lattice_tables(int order_v, int order_e, int R, double *B_h1_lat, double *B_l2_lat)
{
   if (order_v < 1 || order_e < 0 || R < 1) { return -1; }
   std::vector<double> Bh, Bl;
   LatticeTables(order_v, order_e, R, Bh, Bl);
   std::memcpy(B_h1_lat, Bh.data(), Bh.size() * sizeof(double));
   std::memcpy(B_l2_lat, Bl.data(), Bl.size() * sizeof(double));
   return 0;
}
// host-only: the VTK writers of the `-paraview` dumps (vtk_output.hpp); 0 = written.  The arrays are host arrays in the
// layout of lgh_sample_fields; the piece goes to <dir>/cycle_<6 digits>[.<rank>].vtu
int laghos_host_write_vtu(const char *dir, int dim, int NE, int R1, const double *x, const double *v, const double *e,
                          const double *rho, const double *p, int cycle, double time, int rank, int nranks)
{
   return WriteVtu(dir, dim, NE, R1, x, v, e, rho, p, cycle, time, rank, nranks) ? 0 : -1;
}
// host-only: the writer of the `-map` files (map_output.hpp); 0 = written.  rows: the (n[0] n[1] n[2] + 1) x LGH_MAP_COLS doubles of
// lgh_map; the file goes to <dir>/cycle_<6 digits>.vti
int laghos_host_write_vti(const char *dir, int dim, const int *n, const double *lo, const double *hi, const double *rows, long n_excluded,
                          int cycle, double time)
{
   std::string err;
   return WriteVti(dir, dim, n, lo, hi, rows, n_excluded, cycle, time, err) ? 0 : -1;
}
int laghos_host_write_pvtu(const char *dir, int cycle, double time, int nranks) { return WritePvtu(dir, cycle, time, nranks) ? 0 : -1; }
// ... with n_extra further PointData arrays behind the four standing ones (WriteVtuFields): names[k], comps[k] values per point,
// data[k] point by point
static std::vector<VtuField> HostExtra(int n_extra, const char *const *names, const int *comps, const double *const *data)
{
   std::vector<VtuField> extra;
   for (int k = 0; k < n_extra; k++) { extra.push_back({names[k] ? names[k] : "", comps[k], data ? data[k] : nullptr}); }
   return extra;
}
int laghos_host_write_vtu_fields(const char *dir, int dim, int NE, int R1, const double *x, const double *v, const double *e,
                                 const double *rho, const double *p, int n_extra, const char *const *names, const int *comps,
                                 const double *const *data, int cycle, double time, int rank, int nranks)
{
   return WriteVtuFields(dir, dim, NE, R1, x, v, e, rho, p, HostExtra(n_extra, names, comps, data), cycle, time, rank, nranks) ? 0 : -1;
}
int laghos_host_write_pvtu_fields(const char *dir, int cycle, double time, int nranks, int n_extra, const char *const *names, const int *comps)
{
   return WritePvtuFields(dir, cycle, time, nranks, HostExtra(n_extra, names, comps, nullptr)) ? 0 : -1;
}
// host-only: the writers of the `-pv-surface` / `-pv-slice` pieces (WriteVtuFaces, WritePvtuFaces); 0 = written.  The arrays are
// host arrays in the layout of lgh_sample_faces
int laghos_host_write_vtu_faces(const char *dir, int dim, int nfaces, const int *faces, int R1, const double *x, const double *v, const double *e,
                                const double *rho, const double *p, int n_extra, const char *const *names, const int *comps,
                                const double *const *data, const double *an, int cycle, double time, int rank, int nranks)
{
   return WriteVtuFaces(dir, dim, nfaces, faces, R1, x, v, e, rho, p, HostExtra(n_extra, names, comps, data), an, cycle, time, rank, nranks) ? 0 : -1;
}
int laghos_host_write_pvtu_faces(const char *dir, int cycle, double time, int nranks, int n_extra, const char *const *names, const int *comps)
{
   return WritePvtuFaces(dir, cycle, time, nranks, HostExtra(n_extra, names, comps, nullptr)) ? 0 : -1;
}
// host-only: the derivatives of the H1 basis at the lattice abscissae, G_h1_lat[r + (R+1)*d] ((R+1)*(order_v+1))
int laghos_host_lattice_grad_table(int order_v, int R, double *G_h1_lat)
{
   if (order_v < 1 || R < 1) { return -1; }
   std::vector<double> G;
   LatticeGradTable(order_v, R, G);
   std::memcpy(G_h1_lat, G.data(), G.size() * sizeof(double));
   return 0;
}
int laghos_host_write_pvd(const char *pvd_path, const char *rel_dir, int n, const double *times, const int *cycles, int nranks)
{
   return WritePvd(pvd_path, rel_dir, std::vector<double>(times, times + n), std::vector<int>(cycles, cycles + n), nranks) ? 0 : -1;
}
// host-only: the checkpoint writer and reader (checkpoint.hpp); 0 = done, else a CheckpointError with its message in msg.
//   ints[24]: dim problem order_v order_e Q1D | NE global_NE N | nranks rank pgrid[3] | ode_solver cg_max_iter | ti steps repeats |
//             checks checks_ok | header_bytes state_words paraview_dumps (the last three: set by the reader, ignored by the writer)
//   dbls[5]:  cfl cg_tol t dt energy_init;   fps[4]: setup_fp[2] state_fp[2] (state_fp: set by the reader, the writer computes it)
static void CkptPack(const CheckpointHeader &h, long *ints, double *dbls, unsigned long long *fps)
{
   const long v[24] = {h.dim, h.problem, h.order_v, h.order_e, h.Q1D, h.NE, h.global_NE, h.N, h.nranks, h.rank, h.pgrid[0], h.pgrid[1], h.pgrid[2],
                       h.ode_solver, h.cg_max_iter, h.ti, h.steps, h.repeats, h.checks, h.checks_ok, h.header_bytes, h.state_words, h.pv_dumps, 0};
   std::copy(v, v + 24, ints);
   dbls[0] = h.cfl; dbls[1] = h.cg_tol; dbls[2] = h.t; dbls[3] = h.dt; dbls[4] = h.energy_init;
   fps[0] = h.setup_fp[0]; fps[1] = h.setup_fp[1]; fps[2] = h.state_fp[0]; fps[3] = h.state_fp[1];
}
static void CkptMsg(const std::string &err, char *msg, int msg_len)
{
   if (msg && msg_len > 0) { std::snprintf(msg, (size_t)msg_len, "%s", err.c_str()); }
}
int laghos_host_write_checkpoint(const char *path, const long *ints, const double *dbls, const unsigned long long *setup_fp, const double *S, long nS,
                                 const double *pv_times, const long long *pv_cycles, long npv, char *msg, int msg_len)
{
   CheckpointHeader h;
   h.dim = (int)ints[0]; h.problem = (int)ints[1]; h.order_v = (int)ints[2]; h.order_e = (int)ints[3]; h.Q1D = (int)ints[4];
   h.NE = ints[5]; h.global_NE = ints[6]; h.N = ints[7];
   h.nranks = (int)ints[8]; h.rank = (int)ints[9];
   for (int a = 0; a < 3; a++) { h.pgrid[a] = (int)ints[10 + a]; }
   h.ode_solver = (int)ints[13]; h.cg_max_iter = (int)ints[14]; h.ti = (int)ints[15]; h.steps = (int)ints[16]; h.repeats = (int)ints[17];
   h.checks = (int)ints[18]; h.checks_ok = (int)ints[19];
   h.cfl = dbls[0]; h.cg_tol = dbls[1]; h.t = dbls[2]; h.dt = dbls[3]; h.energy_init = dbls[4];
   h.setup_fp[0] = setup_fp[0]; h.setup_fp[1] = setup_fp[1];
   std::string err;
   const int rc = WriteCheckpoint(path, h, S, nS, pv_times, pv_cycles, npv, err);
   CkptMsg(err, msg, msg_len);
   return rc;
}
// S (capS doubles), pv_times / pv_cycles (cap_pv entries) and the header arrays are written only when every check has passed
int laghos_host_read_checkpoint(const char *path, long *ints, double *dbls, unsigned long long *fps, double *S, long capS, double *pv_times,
                                long long *pv_cycles, long cap_pv, char *msg, int msg_len)
{
   Checkpoint c;
   std::string err;
   int rc = ReadCheckpoint(path, c, err);
   if (rc == CKPT_OK && ((long)c.S.size() > capS || (long)c.pv_times.size() > cap_pv))
   {
      rc = CKPT_ERR_CAPACITY;
      err = std::string("checkpoint ") + path + ": capacity: " + std::to_string(c.S.size()) + " state words and " + std::to_string(c.pv_times.size()) +
            " dumps do not fit the caller's arrays";
   }
   CkptMsg(err, msg, msg_len);
   if (rc != CKPT_OK) { return rc; }
   CkptPack(c.h, ints, dbls, fps);
   std::copy(c.S.begin(), c.S.end(), S);
   std::copy(c.pv_times.begin(), c.pv_times.end(), pv_times);
   std::copy(c.pv_cycles.begin(), c.pv_cycles.end(), pv_cycles);
   return CKPT_OK;
}
// host-only: the `-hist` file logic (history.hpp).  The header line; one formatted row (returns its length, -1 when buf is too
// small); and a whole file operation: keep_upto < 0 starts <path> anew, else the existing file is resumed as a restart from cycle
// keep_upto does; then the lines of `rows` (each with its newline; may be empty) are appended one by one and the file is closed.
// 0 = done and *rows_in_file set, -1 with the reason in msg otherwise.
const char *laghos_host_history_header() { return kHistoryHeader; }
int laghos_host_history_row(long cycle, double t, double dt, long rk_steps, long repeats, const double *diag, double energy_init, char *buf, int len)
{
   const std::string r = HistoryRow(cycle, t, dt, rk_steps, repeats, diag, energy_init);
   if ((int)r.size() + 1 > len) { return -1; }
   std::memcpy(buf, r.c_str(), r.size() + 1);
   return (int)r.size();
}
int laghos_host_history_write(const char *path, long keep_upto, const char *rows, long *rows_in_file, char *msg, int msg_len)
{
   HistoryFile h;
   std::string err;
   bool ok = (keep_upto < 0) ? HistoryStart(h, path, err) : HistoryResume(h, path, keep_upto, err);
   const std::string all = rows ? rows : "";
   for (size_t pos = 0; ok && pos < all.size();)
   {
      const size_t nl = all.find('\n', pos), end = (nl == std::string::npos) ? all.size() : nl + 1;
      ok = HistoryAppend(h, all.substr(pos, end - pos), err);
      pos = end;
   }
   CkptMsg(err, msg, msg_len);
   if (rows_in_file) { *rows_in_file = h.rows; }
   return ok ? 0 : -1;
}
// Builds the discretisation of one rank and returns sizes; arrays are copied out
// by laghos_host_disc_get.  kind: 0 h1map, 1 S0, 2 rho0_l2, 3 gamma, 4 rho0_q,
// 5 ess[0], 6 ess[1], 7 ess[2], 8 owner, 9 W, 10 nbr_rank, 11.. nbr_nodes[k-11]
struct laghos_host_disc
{
   std::unique_ptr<Discretization> d;
   std::vector<double> S0, rho0_l2, gamma, rho0_q;
};
// renumber: NULL / "none", "mfem" or "random" (Discretization::Renumber; kinds 100 / 101 of laghos_host_disc_get then
// return node_perm / elem_perm)
static laghos_host_disc *HostDiscCreate(const char *mesh, const int *zones, int rs, int order_v, int order_e, int problem,
                                        double blast_energy, int nranks, int rank, const char *renumber, int seed)
{
   try
   {
      // zones: a Cartesian grid of zones[0] x zones[1] x zones[2] unit-box zones in zones[3] dimensions (the driver's
      // "default" mesh) instead of a named one
      CartMesh m = zones ? CartMesh::Cartesian(zones[3], zones[0], zones[1], zones[2], 1.0, 1.0, 1.0) : CartMesh::Named(mesh);
      for (int l = 0; l < rs; l++) { m.UniformRefinement(); }
      std::unique_ptr<laghos_host_disc> h(new laghos_host_disc());
      h->d.reset(new Discretization(m, order_v, order_e, problem, nranks, rank, -1, blast_energy));
      if (renumber) { h->d->Renumber(renumber, rs, (unsigned)seed); }
      h->d->InitialState(h->S0, h->rho0_l2, h->gamma, h->rho0_q);
      return h.release();
   }
   catch (const std::exception &e)
   {
      std::fprintf(stderr, "laghos_host_disc_create: %s\n", e.what());
      return nullptr;
   }
}
laghos_host_disc *laghos_host_disc_create_renumbered(const char *mesh, int rs, int order_v, int order_e, int problem,
                                                     double blast_energy, int nranks, int rank, const char *renumber, int seed)
{
   return HostDiscCreate(mesh, nullptr, rs, order_v, order_e, problem, blast_energy, nranks, rank, renumber, seed);
}
// the same on a Cartesian grid of nx x ny x nz zones of the unit box (`-m default -dim .. -nx .. -ny .. -nz ..`)
laghos_host_disc *laghos_host_disc_create_cartesian(int dim, int nx, int ny, int nz, int rs, int order_v, int order_e, int problem,
                                                    double blast_energy, int nranks, int rank, const char *renumber, int seed)
{
   const int zones[4] = {nx, ny, nz, dim};
   return HostDiscCreate(nullptr, zones, rs, order_v, order_e, problem, blast_energy, nranks, rank, renumber, seed);
}
laghos_host_disc *laghos_host_disc_create(const char *mesh, int rs, int order_v, int order_e, int problem,
                                          double blast_energy, int nranks, int rank)
{
   return laghos_host_disc_create_renumbered(mesh, rs, order_v, order_e, problem, blast_energy, nranks, rank, nullptr, 0);
}
void laghos_host_disc_destroy(laghos_host_disc *h) { delete h; }
long laghos_host_disc_size(laghos_host_disc *h, int kind)
{
   const Discretization &d = *h->d;
   switch (kind)
   {
      case 0: return (long)d.h1map.size();
      case 1: return (long)h->S0.size();
      case 2: return (long)h->rho0_l2.size();
      case 3: return (long)h->gamma.size();
      case 4: return (long)h->rho0_q.size();
      case 5: case 6: case 7: return (long)d.ess[kind - 5].size();
      case 8: return (long)d.owner.size();
      case 9: return (long)d.W.size();
      case 10: return (long)d.nbr_rank.size();
      case 100: return (long)d.node_perm.size();
      case 101: return (long)d.elem_perm.size();
      default:
         if (kind - 11 < (int)d.nbr_nodes.size()) { return (long)d.nbr_nodes[kind - 11].size(); }
         return -1;
   }
}
void laghos_host_disc_get(laghos_host_disc *h, int kind, void *out)
{
   const Discretization &d = *h->d;
   auto cp = [&](const void *p, size_t bytes) { std::memcpy(out, p, bytes); };
   switch (kind)
   {
      case 0: cp(d.h1map.data(), d.h1map.size() * sizeof(int)); break;
      case 1: cp(h->S0.data(), h->S0.size() * sizeof(double)); break;
      case 2: cp(h->rho0_l2.data(), h->rho0_l2.size() * sizeof(double)); break;
      case 3: cp(h->gamma.data(), h->gamma.size() * sizeof(double)); break;
      case 4: cp(h->rho0_q.data(), h->rho0_q.size() * sizeof(double)); break;
      case 5: case 6: case 7: cp(d.ess[kind - 5].data(), d.ess[kind - 5].size() * sizeof(int)); break;
      case 8: cp(d.owner.data(), d.owner.size() * sizeof(double)); break;
      case 9: cp(d.W.data(), d.W.size() * sizeof(double)); break;
      case 10: cp(d.nbr_rank.data(), d.nbr_rank.size() * sizeof(int)); break;
      case 100: cp(d.node_perm.data(), d.node_perm.size() * sizeof(int)); break;
      case 101: cp(d.elem_perm.data(), d.elem_perm.size() * sizeof(int)); break;
      default: cp(d.nbr_nodes[kind - 11].data(), d.nbr_nodes[kind - 11].size() * sizeof(int));
   }
}

// the reference main(): returns the process exit code
int laghos_main(int argc, const char *const *argv)
{
   laghos_sim *s = laghos_sim_create(argc, argv, 1, 0, nullptr);
   if (!s) { return 1; }
   const Options &o = s->opt;
   int rc;
   while ((rc = laghos_sim_step(s)) == 1) {}
   if (rc < 0) { laghos_sim_destroy(s); return 1; }
   if (o.fingerprint)
   {
      unsigned long long fp[2];
      if (laghos_sim_fingerprint(s, fp) != 0) { laghos_sim_destroy(s); return 1; }
      std::cout << "State fingerprint: " << Hex32(fp) << " (cycle " << s->ti - 1 << ")" << std::endl;
   }
   int steps = (s->steps - s->steps_at_start) * s->ode->Stages(); // laghos.cpp:928-935 (a restart: the steps of this segment, as the timers)
   s->hydro->PrintTimingData(true, steps, o.fom);
   const double energy_final = laghos_sim_energy(s);
   std::cout << std::endl;
   std::cout << "Energy  diff: " << std::scientific << std::setprecision(2)
             << std::fabs(s->energy_init - energy_final) << std::endl;
   if (o.paraview && !o.quiet)
   {
      std::cout << "ParaView dumps: " << s->pv_cycles.size() << " (sample " << s->pv_seconds[0] << " s, copy " << s->pv_seconds[1]
                << " s, write " << s->pv_seconds[2] << " s) -> " << o.basename << ".pvd" << std::endl;
   }
   if (o.FaceDumps() && !o.quiet)
   {
      std::cout << "Face dumps: " << s->pv_cycles.size() << " x " << s->pv_faces.size() << " (sample " << s->pvf_seconds[0] << " s, copy " << s->pvf_seconds[1]
                << " s, write " << s->pvf_seconds[2] << " s) ->";
      for (const auto &fs : s->pv_faces) { std::cout << " " << FaceSetDir(o.basename, fs.tag) << ".pvd"; }
      std::cout << std::endl;
   }
   if (o.ckpt_steps > 0 && !o.quiet)
   {
      std::cout << "Checkpoints: " << s->ckpt_count << " (fingerprint " << s->ckpt_seconds[0] << " s, copy " << s->ckpt_seconds[1] << " s, write "
                << s->ckpt_seconds[2] << " s) -> " << CheckpointDir(o.basename) << std::endl;
   }
   if (o.hist_steps > 0 && !o.quiet) { std::cout << "History: " << s->hist.path << ", " << s->hist.rows << " rows" << std::endl; }
   if (o.prof_steps > 0 && !o.quiet) { std::cout << "Profiles: " << s->prof_files << " files, " << o.basename << "_profile_*.csv" << std::endl; }
   if (o.map_steps > 0 && !o.quiet) { std::cout << "Maps: " << s->map_files << " files, " << MapDir(o.basename) << "/cycle_*.vti" << std::endl; }
   int ret = 0;
   if (o.check_exact_sedov)
   {
      const double err = laghos_sim_sedov_error(s);
      if (err < 0) { laghos_sim_destroy(s); return 1; }
      // the reference prints this with the stream state left by "Energy diff" (scientific, 2 digits)
      std::cout << "Density L2 error: " << std::scientific << std::setprecision(6) << err << std::endl;
   }
   if (o.check && !(s->checks == 2 && s->checks_ok))
   {
      std::cout << "Check error!" << std::endl; // MFEM_VERIFY(!check || checks == 2) (laghos.cpp:926)
      ret = 1;
   }
   laghos_sim_destroy(s);
   return ret;
}

} // extern "C"

#ifdef LAGHOS_MAIN
int main(int argc, char *argv[]) { return laghos_main(argc - 1, argv + 1); }
#endif
