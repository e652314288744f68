// options.cpp — the driver's command line: ParseArgs and CheckAgainstMesh (options.hpp).
#include "options.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>

#include "laghos_solver.hpp"

namespace laghos
{

namespace
{

using H = hydrodynamics::LagrangianHydroOperator;

bool Refuse(std::string &err, const std::string &why)
{
   err = "laghos: " + why;
   return false;
}

// The options that take one value (atoi / atof: `-ms abc` is 0) or none
template <class T> struct ValueOpt { const char *s, *l; T Options::*field; };
using IntOpt = ValueOpt<int>;
using DblOpt = ValueOpt<double>;
using StrOpt = ValueOpt<std::string>;
struct FlagOpt { const char *s, *l; bool Options::*field; bool value; };
// ... and the counts that have a least value: 1 for the periods of the periodic outputs, 0 for -ckpt-keep
struct CountOpt { const char *s, *l; int Options::*field; int least; };

const IntOpt kInts[] = {
   {"-dim", "--dimension", &Options::dim}, {"-nx", "--xelems", &Options::nx}, {"-ny", "--yelems", &Options::ny}, {"-nz", "--zelems", &Options::nz},
   {"-rs", "--refine-serial", &Options::rs_levels}, {"-rp", "--refine-parallel", &Options::rp_levels}, {"-p", "--problem", &Options::problem},
   {"-ok", "--order-kinematic", &Options::order_v}, {"-ot", "--order-thermo", &Options::order_e}, {"-oq", "--order-intrule", &Options::order_q},
   {"-s", "--ode-solver", &Options::ode_solver_type}, {"-cgm", "--cg-max-steps", &Options::cg_max_iter}, {"-ms", "--max-steps", &Options::max_tsteps},
   {"-vs", "--visualization-steps", &Options::vis_steps}, {"-dev", "--dev", &Options::dev}, {"-renumber-seed", "--renumber-seed", &Options::renumber_seed}};
const DblOpt kDbls[] = {
   {"-E0", "--blast-energy", &Options::blast_energy}, {"-Sx", "--xwidth", &Options::Sx}, {"-Sy", "--ywidth", &Options::Sy}, {"-Sz", "--zwidth", &Options::Sz},
   {"-tf", "--t-final", &Options::t_final}, {"-cfl", "--cfl", &Options::cfl}, {"-cgt", "--cg-tol", &Options::cg_tol}};
const StrOpt kStrs[] = {
   {"-m", "--mesh", &Options::mesh_file}, {"-renumber", "--renumber", &Options::renumber}, {"-k", "--outputfilename", &Options::basename}};
const FlagOpt kFlags[] = {
   {"-fp", "--fingerprint", &Options::fingerprint, true},
   {"-pa", "--partial-assembly", &Options::p_assembly, true}, {"-fa", "--full-assembly", &Options::p_assembly, false},
   {"-chk", "--checks", &Options::check, true}, {"-no-chk", "--no-checks", &Options::check, false},
   {"-iv", "--impose-viscosity", &Options::impose_visc, true}, {"-niv", "--no-impose-viscosity", &Options::impose_visc, false},
   {"-f", "--fom", &Options::fom, true}, {"-no-fom", "--no-fom", &Options::fom, false},
   {"-err", "--exact-error", &Options::check_exact_sedov, true}, {"-no-err", "--no-exact-error", &Options::check_exact_sedov, false},
   {"-q", "--quiet", &Options::quiet, true}, {"-print", "--print", &Options::gfprint, true},
   {"-paraview", "--paraview", &Options::paraview, true}, {"-no-paraview", "--no-paraview", &Options::paraview, false},
   {"-pv-surface", "--paraview-surface", &Options::pv_surface, true},
   {"-store-stress", "--store-stress", &Options::store_stress, true}, {"-no-store-stress", "--no-store-stress", &Options::store_stress, false}};
const CountOpt kCounts[] = {
   {"-ckpt", "--checkpoint-steps", &Options::ckpt_steps, 1}, {"-ckpt-keep", "--checkpoint-keep", &Options::ckpt_keep, 0},
   {"-hist", "--history-steps", &Options::hist_steps, 1}, {"-prof", "--profile-steps", &Options::prof_steps, 1},
   {"-map", "--map-steps", &Options::map_steps, 1}, {"-loads", "--loads-steps", &Options::loads_steps, 1},
   {"-peaks", "--peaks-steps", &Options::peaks_steps, 1}, {"-gauges", "--gauge-steps", &Options::gauge_steps, 1}};

constexpr size_t kGaugesOnCommandLine = 64, kGaugesInAll = 4096;
constexpr double kGaugeBufferBytes = 256.0 * 1024 * 1024;

template <class Opt, size_t N> const Opt *Find(const Opt (&table)[N], const std::string &a)
{
   for (const Opt &k : table) { if (a == k.s || a == k.l) { return &k; } }
   return nullptr;
}

// One to `most` numbers behind argv[i], up to the first token that is not a complete number (integers: not a complete integer);
// i moves over them.  Returns how many there were.
int TakeNumbers(int argc, const char *const *argv, int &i, int most, bool integers, double *out)
{
   int n = 0;
   while (n < most && i + 1 < argc)
   {
      char *end = nullptr;
      const double x = integers ? (double)std::strtol(argv[i + 1], &end, 10) : std::strtod(argv[i + 1], &end);
      if (end == argv[i + 1] || *end) { break; }
      out[n++] = x;
      i++;
   }
   return n;
}

bool FiniteInterval(double lo, double hi) { return std::isfinite(lo) && std::isfinite(hi) && std::isfinite(hi - lo) && lo < hi; }

// -pv-fields LIST
bool ParseFieldList(const std::string &list, Options &o, std::string &err)
{
   static const struct { const char *name; unsigned bit; } known[] = {
      {"div_v", H::DERIVED_DIV}, {"vorticity", H::DERIVED_VORT}, {"grad_v", H::DERIVED_GRAD}, {"detj", H::DERIVED_DETJ},
      {"sound_speed", H::DERIVED_CS}, {"all", H::DERIVED_ALL}};
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
      for (const auto &k : known) { if (name == k.name) { bit = k.bit; } }
      if (!bit) { return Refuse(err, "-pv-fields: unknown field " + name + " (div_v, vorticity, grad_v, detj, sound_speed or all)"); }
      if (name == "vorticity") { o.pv_vort_named = true; }
      o.pv_fields |= bit;
   }
   if (!o.pv_fields) { return Refuse(err, "-pv-fields needs a list of div_v, vorticity, grad_v, detj, sound_speed, or all: the list is empty"); }
   return true;
}

// -pv-slice AXIS K and -loads-plane AXIS K (opt; its planes are `noun`), v = K: one more entry of `planes`
bool ParsePlane(const std::string &opt, const char *noun, const std::string &ax, const char *v, std::vector<std::pair<int, int>> &planes, std::string &err)
{
   char *end = nullptr;
   const long K = std::strtol(v, &end, 10);
   if (end == v || *end || K < 0 || K > 1000000000L) { return Refuse(err, opt + " " + ax + " K: K must be a node plane 0 <= K <= n of the zone grid, got " + v); }
   const std::pair<int, int> sl(ax[0] - 'x', (int)K);
   const std::string which = opt + " " + ax + " " + std::to_string(K);
   if (std::find(planes.begin(), planes.end(), sl) != planes.end()) { return Refuse(err, which + " is given twice"); }
   if (planes.size() == 8) { return Refuse(err, which + ": at most 8 " + noun + ", this is the ninth"); }
   planes.push_back(sl);
   return true;
}

// -gauge-file PATH: one point per line - one to three numbers separated by blanks or tabs -, `#` starts a comment, empty lines are skipped
bool ReadGaugeFile(const std::string &path, std::vector<Options::GaugePoint> &points, std::string &err)
{
   points.clear();
   std::ifstream f(path.c_str());
   if (!f) { return Refuse(err, "-gauge-file " + path + ": cannot read the file"); }
   std::string line;
   for (int no = 1; std::getline(f, line); no++)
   {
      const std::string where = "-gauge-file " + path + " line " + std::to_string(no);
      line = line.substr(0, line.find('#'));
      Options::GaugePoint p;
      p.from = where;
      const char *c = line.c_str();
      while (true)
      {
         while (*c == ' ' || *c == '\t' || *c == '\r') { c++; }
         if (!*c) { break; }
         char *end = nullptr;
         const double x = std::strtod(c, &end);
         if (end == c || (*end && *end != ' ' && *end != '\t' && *end != '\r')) { return Refuse(err, where + ": malformed, a point is one to three numbers, got " + line); }
         if (p.n == 3) { return Refuse(err, where + ": malformed, a point has at most three coordinates"); }
         if (!std::isfinite(x)) { return Refuse(err, where + ": the coordinates must be finite numbers"); }
         p.x[p.n++] = x;
         c = end;
      }
      if (p.n > 0) { points.push_back(p); }
   }
   if (f.bad()) { return Refuse(err, "-gauge-file " + path + ": cannot read the file"); }
   if (points.empty()) { return Refuse(err, "-gauge-file " + path + ": the file holds no point"); }
   return true;
}

} // namespace

bool ParseArgs(int argc, const char *const *argv, Options &o, std::string &err)
{
   auto need = [&](int &i) -> const char * {
      if (i + 1 >= argc) { Refuse(err, std::string("missing value for ") + argv[i]); return nullptr; }
      return argv[++i];
   };
   for (int i = 0; i < argc; i++)
   {
      const std::string a = argv[i];
      const char *v = nullptr;
      double x[6];
      if (const IntOpt *k = Find(kInts, a)) { if (!(v = need(i))) { return false; } o.*k->field = std::atoi(v); continue; }
      if (const DblOpt *k = Find(kDbls, a)) { if (!(v = need(i))) { return false; } o.*k->field = std::atof(v); continue; }
      if (const StrOpt *k = Find(kStrs, a)) { if (!(v = need(i))) { return false; } o.*k->field = v; continue; }
      if (const FlagOpt *k = Find(kFlags, a)) { o.*k->field = k->value; continue; }
      if (const CountOpt *k = Find(kCounts, a))
      {
         if (!(v = need(i))) { return false; }
         o.*k->field = std::atoi(v);
         const char *rule = (k->least == 1) ? " must be at least 1, got " : " must be 0 (keep all) or more, got ";
         if (o.*k->field < k->least) { return Refuse(err, std::string(k->s) + " / " + k->l + rule + v); }
         continue;
      }
      if (a == "-prof-axis" || a == "--profile-axis")
      {
         if (!(v = need(i))) { return false; }
         o.prof_axis = v;
         if (o.prof_axis != "x" && o.prof_axis != "y" && o.prof_axis != "z" && o.prof_axis != "r") { return Refuse(err, "-prof-axis must be x, y, z or r, got " + o.prof_axis); }
         continue;
      }
      if (a == "-prof-bins" || a == "--profile-bins")
      {
         if (!(v = need(i))) { return false; }
         o.prof_bins = std::atoi(v);
         if (o.prof_bins < 1 || o.prof_bins > LGH_PROFILE_MAX_BINS) { return Refuse(err, "-prof-bins must be between 1 and " + std::to_string(LGH_PROFILE_MAX_BINS) + ", got " + v); }
         continue;
      }
      if (a == "-prof-range" || a == "--profile-range")
      {
         for (int k = 0; k < 2; k++)
         {
            if (!(v = need(i))) { return false; }
            char *end = nullptr;
            x[k] = std::strtod(v, &end);
            if (end == v || *end) { return Refuse(err, "-prof-range needs two numbers, got " + std::string(v)); }
         }
         if (!FiniteInterval(x[0], x[1])) { return Refuse(err, "-prof-range LO HI needs finite LO < HI"); }
         o.prof_lo = x[0]; o.prof_hi = x[1]; o.prof_range_set = true;
         continue;
      }
      if (a == "-prof-origin" || a == "--profile-origin")
      {
         const int n = TakeNumbers(argc, argv, i, 3, false, x); // (coordinates it does not name keep what an earlier one gave them)
         if (n == 0) { return Refuse(err, "-prof-origin needs one to three numbers"); }
         for (int k = 0; k < n; k++)
         {
            if (!std::isfinite(x[k])) { return Refuse(err, "-prof-origin needs finite coordinates"); }
            o.prof_origin[k] = x[k];
         }
         continue;
      }
      if (a == "-map-cells" || a == "--map-cells")
      {
         const int first = i + 1;
         o.map_cells_n = TakeNumbers(argc, argv, i, 3, true, x);
         if (o.map_cells_n == 0) { return Refuse(err, "-map-cells needs one to three counts"); }
         for (int k = 0; k < o.map_cells_n; k++)
         {
            if (x[k] < 1 || x[k] > LGH_MAP_MAX_CELLS) { return Refuse(err, "-map-cells needs counts between 1 and " + std::to_string(LGH_MAP_MAX_CELLS) + ", got " + argv[first + k]); }
            o.map_cells[k] = (int)x[k];
         }
         continue;
      }
      if (a == "-map-box" || a == "--map-box")
      {
         o.map_box_n = TakeNumbers(argc, argv, i, 6, false, o.map_box); // one pair per axis
         if (o.map_box_n == 0 || o.map_box_n % 2) { return Refuse(err, "-map-box needs a pair LO HI per axis, got " + std::to_string(o.map_box_n) + " numbers"); }
         for (int k = 0; k < o.map_box_n; k += 2)
         {
            if (!FiniteInterval(o.map_box[k], o.map_box[k + 1])) { return Refuse(err, "-map-box needs finite LO < HI on every axis"); }
         }
         continue;
      }
      if (a == "-peaks-arrival" || a == "--peaks-arrival")
      {
         if (!(v = need(i))) { return false; }
         char *end = nullptr;
         o.peaks_arrival = std::strtod(v, &end);
         o.peaks_arrival_set = true;
         if (end == v || *end || !std::isfinite(o.peaks_arrival)) { return Refuse(err, "-peaks-arrival P: the pressure threshold must be a finite number, got " + std::string(v)); }
         continue;
      }
      if (a == "-gauge" || a == "--gauge")
      {
         Options::GaugePoint p;
         p.n = TakeNumbers(argc, argv, i, 3, false, p.x);
         if (p.n == 0) { return Refuse(err, "-gauge X [Y [Z]] needs one to three numbers"); }
         p.from = "-gauge";
         for (int k = 0; k < p.n; k++) { p.from += std::string(" ") + argv[i - p.n + 1 + k]; }
         for (int k = 0; k < p.n; k++) { if (!std::isfinite(p.x[k])) { return Refuse(err, p.from + ": the coordinates must be finite numbers"); } }
         if (o.gauge_points.size() == kGaugesOnCommandLine) { return Refuse(err, p.from + ": at most 64 gauges on the command line (-gauge-file takes more), this is the 65th"); }
         o.gauge_points.push_back(p);
         continue;
      }
      if (a == "-gauge-file" || a == "--gauge-file")
      {
         if (!(v = need(i))) { return false; }
         o.gauge_file = v;
         if (!ReadGaugeFile(o.gauge_file, o.gauge_file_points, err)) { return false; }
         continue;
      }
      if (a == "-gauge-buffer" || a == "--gauge-buffer")
      {
         if (!(v = need(i))) { return false; }
         char *end = nullptr;
         const long M = std::strtol(v, &end, 10);
         o.gauge_buffer_set = true;
         if (end == v || *end || M < 1 || M > 1000000000L) { return Refuse(err, "-gauge-buffer M: the buffer holds at least 1 sample, got " + std::string(v)); }
         o.gauge_buffer = (int)M;
         continue;
      }
      if (a == "-restart" || a == "--restart")
      {
         if (!(v = need(i))) { return false; }
         o.restart = v;
         if (o.restart.empty()) { return Refuse(err, "-restart needs a checkpoint stem or the word latest"); }
         continue;
      }
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
         if (!ParseFieldList(v, o, err)) { return false; }
         continue;
      }
      const bool slice = a == "-pv-slice" || a == "--paraview-slice";
      if (slice || a == "-loads-plane" || a == "--loads-plane")
      {
         const std::string opt = slice ? "-pv-slice" : "-loads-plane";
         if (i + 2 >= argc) { return Refuse(err, "missing value for " + a + " AXIS K"); }
         const std::string ax = argv[++i];
         if (ax != "x" && ax != "y" && ax != "z") { return Refuse(err, opt + " AXIS K: the axis must be x, y or z, got " + ax); }
         if (!ParsePlane(opt, slice ? "slices" : "planes", ax, argv[++i], slice ? o.pv_slices : o.loads_planes, err)) { return false; }
         continue;
      }
      if (a == "-pv-iso" || a == "--paraview-iso")
      {
         if (i + 2 >= argc) { return Refuse(err, "missing value for " + a + " FIELD VALUE"); }
         Options::Contour c;
         c.field = argv[++i];
         v = argv[++i];
         if (H::ContourField(c.field) < 0) { return Refuse(err, "-pv-iso: unknown field " + c.field + " (" + H::ContourFieldList() + ")"); }
         char *end = nullptr;
         c.value = std::strtod(v, &end);
         const std::string which = "-pv-iso " + c.field + " " + v;
         if (end == v || *end || !std::isfinite(c.value)) { return Refuse(err, which + ": the value must be a finite number"); }
         for (const auto &k : o.pv_isos) { if (k.field == c.field && k.value == c.value) { return Refuse(err, which + " is given twice"); } }
         if (o.pv_isos.size() == 8) { return Refuse(err, which + ": at most 8 iso-surfaces, this is the ninth"); }
         c.tag = "iso" + std::to_string(o.pv_isos.size()) + "_" + c.field;
         o.pv_isos.push_back(c);
         continue;
      }
      if (a == "-pv-plane" || a == "--paraview-plane")
      {
         const int n = TakeNumbers(argc, argv, i, 4, false, x);
         if (n < 3) { return Refuse(err, "-pv-plane NX NY [NZ] D needs three numbers in 2D and four in 3D, got " + std::to_string(n)); }
         Options::Contour c;
         c.field = "plane";
         c.ncoef = n - 1;
         c.value = x[n - 1];
         bool finite = std::isfinite(c.value), zero = true;
         std::string which = "-pv-plane";
         for (int k = 0; k < n; k++)
         {
            if (k < n - 1) { c.coef[k] = x[k]; finite = finite && std::isfinite(x[k]); zero = zero && x[k] == 0.0; }
            which += std::string(" ") + argv[i - n + 1 + k];
         }
         if (!finite) { return Refuse(err, which + ": the normal and D must be finite numbers"); }
         if (zero) { return Refuse(err, which + ": the normal is zero"); }
         for (const auto &k : o.pv_planes)
         {
            if (k.ncoef == c.ncoef && k.value == c.value && std::equal(c.coef, c.coef + 3, k.coef)) { return Refuse(err, which + " is given twice"); }
         }
         if (o.pv_planes.size() == 8) { return Refuse(err, which + ": at most 8 planes, this is the ninth"); }
         c.tag = "plane" + std::to_string(o.pv_planes.size());
         o.pv_planes.push_back(c);
         continue;
      }
      if (a == "-d" || a == "--device") { if (!need(i)) { return false; } continue; } // always the HIP path
      if (a == "-no-vis" || a == "--no-visualization" || a == "-no-visit" || a == "-no-print") { continue; }
      return Refuse(err, "unsupported option: " + a);
   }
   if (!o.vis_refine_set) { o.vis_refine = o.order_v; }
   const bool vr_used = o.vis_refine_set || o.paraview || o.LatticeDumps();
   if (vr_used && (o.vis_refine < 1 || o.vis_refine > 8)) { return Refuse(err, "-vr / --vis-refine must be between 1 and 8, got " + std::to_string(o.vis_refine)); }
   if (o.pv_fields_set && !o.paraview && !o.LatticeDumps()) { return Refuse(err, "-pv-fields adds fields to the -paraview dumps: it needs -paraview"); }
   const char *map_detail = o.map_cells_n > 0 ? "-map-cells" : (o.map_box_n > 0 ? "-map-box" : nullptr);
   if (map_detail && o.map_steps == 0) { return Refuse(err, std::string(map_detail) + " describes the -map files: it needs -map"); }
   if (!o.loads_planes.empty() && o.loads_steps == 0) { return Refuse(err, "-loads-plane adds rows to the -loads file: it needs -loads"); }
   if (o.peaks_arrival_set && o.peaks_steps == 0) { return Refuse(err, "-peaks-arrival adds the arrival time to the -peaks records: it needs -peaks"); }
   if (o.peaks_steps > 0 && !o.paraview && !o.FaceDumps())
   {
      return Refuse(err, "-peaks keeps its records at the points of the material dumps: it needs -paraview, -pv-surface or -pv-slice");
   }
   const char *gauge_detail = !o.gauge_points.empty() ? "-gauge" : (!o.gauge_file.empty() ? "-gauge-file" : (o.gauge_buffer_set ? "-gauge-buffer" : nullptr));
   if (gauge_detail && o.gauge_steps == 0) { return Refuse(err, std::string(gauge_detail) + " describes the gauges of the -gauges file: it needs -gauges"); }
   if (o.gauge_steps > 0)
   {
      const size_t n = o.Gauges();
      if (n == 0) { return Refuse(err, "-gauges records time series at gauges: it needs a point, -gauge X [Y [Z]] or -gauge-file PATH"); }
      if (n > kGaugesInAll) { return Refuse(err, "-gauges: at most 4096 gauges in all, got " + std::to_string(n)); }
      if ((double)o.gauge_buffer * (double)n * (LGH_GAUGE_COLS * sizeof(double)) > kGaugeBufferBytes)
      {
         return Refuse(err, "-gauge-buffer " + std::to_string(o.gauge_buffer) + ": " + std::to_string(o.gauge_buffer) + " samples of " + std::to_string(n) +
                               " gauges need more than 256 MiB on the device");
      }
   }
   if (o.check_exact_sedov) // laghos.cpp:303-309, in the reference's words
   {
      if (o.problem != 1) { err = "Can only compare problem 1 (Sedov) against the exact solution"; return false; }
      if (o.mesh_file.compare(0, 7, "default") != 0) { err = "check: mesh_file"; return false; }
   }
   return true;
}

bool CheckAgainstMesh(Options &o, const CartMesh &mesh, std::string &err)
{
   o.dim = mesh.dim;
   if (o.dim == 1 && o.p_assembly) // laghos.cpp:454-462: 1D runs the FA path
   {
      o.p_assembly = false;
      if (o.rank == 0 && !o.quiet) { std::cout << "Laghos does not support PA in 1D. Switching to FA." << std::endl; }
   }
   if (o.dim == 1 && (o.pv_fields & H::DERIVED_VORT))
   {
      if (o.pv_vort_named) { return Refuse(err, "-pv-fields vorticity: there is no vorticity in 1D"); }
      o.pv_fields &= ~(unsigned)H::DERIVED_VORT; // (all)
   }
   const std::string faces = o.pv_surface ? "-pv-surface" : "-pv-slice";
   if (o.FaceDumps() && o.dim == 1) { return Refuse(err, faces + ": zone faces are dumped in 2D and 3D, this mesh is 1D (its -paraview dump is small already)"); }
   const std::string dims = std::to_string(o.dim);
   for (const auto &sl : o.pv_slices)
   {
      const std::string ax(1, (char)('x' + sl.first)), which = "-pv-slice " + ax + " " + std::to_string(sl.second);
      if (sl.first >= o.dim) { return Refuse(err, which + ": the mesh has " + dims + " dimensions, there is no " + ax + " axis"); }
      const std::string planes = std::to_string(mesh.ne(sl.first));
      if (sl.second > mesh.ne(sl.first)) { return Refuse(err, which + ": K is out of range, the zone grid has node planes 0.." + planes + " along " + ax); }
   }
   if (o.ContourDumps() && o.dim == 1)
   {
      return Refuse(err, std::string(o.pv_isos.empty() ? "-pv-plane" : "-pv-iso") + ": contours are formed in 2D and 3D, this mesh is 1D");
   }
   for (const auto &c : o.pv_isos)
   {
      if (c.field == "z" && o.dim == 2) { return Refuse(err, "-pv-iso z: the mesh has 2 dimensions, there is no z axis"); }
   }
   for (const auto &c : o.pv_planes)
   {
      if (c.ncoef != o.dim)
      {
         return Refuse(err, "-pv-plane (" + c.tag + ") has " + std::to_string(c.ncoef + 1) + " numbers, a mesh of " + dims + " dimensions needs " + std::to_string(o.dim + 1));
      }
   }
   if (o.loads_steps > 0 && o.dim == 1) { return Refuse(err, "-loads: pressure loads are taken on zone faces in 2D and 3D, this mesh is 1D"); }
   for (const auto &pl : o.loads_planes)
   {
      const std::string ax(1, (char)('x' + pl.first)), which = "-loads-plane " + ax + " " + std::to_string(pl.second);
      if (pl.first >= o.dim) { return Refuse(err, which + ": the mesh has " + dims + " dimensions, there is no " + ax + " axis"); }
      if (pl.second > mesh.ne(pl.first)) { return Refuse(err, which + ": K is out of range, the zone grid has node planes 0.." + std::to_string(mesh.ne(pl.first)) + " along " + ax); }
   }
   for (const std::vector<Options::GaugePoint> *list : {&o.gauge_points, &o.gauge_file_points})
   {
      for (const Options::GaugePoint &p : *list)
      {
         if (p.n != o.dim) { return Refuse(err, p.from + ": the point has " + std::to_string(p.n) + " coordinates, the mesh has " + dims + " dimensions"); }
         int ijk[3];
         double xi[3];
         if (!LocateInitial(mesh, p.x, ijk, xi)) { return Refuse(err, p.from + ": the point lies outside the initial mesh"); }
      }
   }
   if (o.prof_axis.empty()) { o.prof_axis = (o.problem == 1) ? "r" : "x"; }
   const int prof_dims = (o.prof_axis == "r") ? 1 : o.prof_axis[0] - 'x' + 1; // the dimensions the axis needs
   if (o.prof_steps > 0 && prof_dims > o.dim) { return Refuse(err, "-prof-axis " + o.prof_axis + " needs a mesh of " + std::to_string(prof_dims) + " dimensions, this one has " + dims); }
   if (o.map_steps > 0)
   {
      const std::string cells_n = std::to_string(o.map_cells_n), box_n = std::to_string(o.map_box_n);
      if (o.map_cells_n > 0 && o.map_cells_n != o.dim) { return Refuse(err, "-map-cells has " + cells_n + " counts, the mesh has " + dims + " dimensions"); }
      if (o.map_box_n > 0 && o.map_box_n != 2 * o.dim) { return Refuse(err, "-map-box has " + box_n + " numbers, a mesh of " + dims + " dimensions needs " + std::to_string(2 * o.dim)); }
      double ncells = 1.0;
      for (int c = 0; c < o.dim; c++) { ncells *= (double)o.map_cells[c]; }
      if (ncells > (double)LGH_MAP_MAX_CELLS)
      {
         char asked[32];
         std::snprintf(asked, sizeof(asked), "%.0f", ncells);
         return Refuse(err, std::string("-map-cells asks for ") + asked + " cells, at most " + std::to_string(LGH_MAP_MAX_CELLS) + " fit");
      }
   }
   if (!o.p_assembly && o.dim != 1) { return Refuse(err, "only the partial-assembly path (-pa) is implemented"); }
   const char *force_multi = std::getenv("LGH_FORCE_MULTI");
   if (o.dim == 1 && force_multi && force_multi[0] == '1') { return Refuse(err, "LGH_FORCE_MULTI=1 drives the multi-rank path, which 1D does not have"); }
   return true;
}

} // namespace laghos
