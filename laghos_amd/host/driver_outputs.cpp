// driver_outputs.cpp — what the driver writes (driver_outputs.hpp).
#include "driver_outputs.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <sys/stat.h>

#include "map_output.hpp"
#include "profile.hpp"
#include "records_sidecar.hpp"
#include "sedov_exact.hpp"
#include "vtk_output.hpp"

namespace laghos
{

using H = hydrodynamics::LagrangianHydroOperator;

bool SimFail(laghos_sim *s, const std::string &msg)
{
   s->error = msg;
   std::fprintf(stderr, "laghos: %s\n", msg.c_str());
   return false;
}

std::string Hex32(const unsigned long long fp[2])
{
   char buf[40];
   std::snprintf(buf, sizeof(buf), "%016llX%016llX", fp[0], fp[1]);
   return buf;
}

// A file is written and every rank learns whether it was (collective): by rank 0, and the least of the ranks' flags tells; or
// - the pieces of a checkpoint - by every rank, and the sum of the flags tells.  A rank that could not write says `mine` and what
// write() left in its err, the others say `others`.
template <class Write>
static bool WriteAndAgree(laghos_sim *s, bool every_rank, const std::string &mine, const std::string &others, Write write)
{
   const Options &o = s->opt;
   bool ok = true;
   std::string err;
   if (every_rank || o.rank == 0) { ok = write(err); }
   const double agreed = s->hydro->AllReduce(ok ? 1.0 : 0.0, every_rank ? 0 : 1);
   if (!ok) { return SimFail(s, mine + err); }
   if (agreed != (every_rank ? (double)o.nranks : 1.0)) { return SimFail(s, others); }
   return true;
}

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
   // a grid function: the header of its space, then one value per line (8 significant digits, as everything here)
   auto values = [&](std::ofstream &f, const char *fec, int order, int vdim, const double *begin, const double *end) {
      f.precision(8);
      f << "FiniteElementSpace\nFiniteElementCollection: " << fec << "_" << dim << "D_P" << order << "\nVDim: " << vdim
        << "\nOrdering: 0\n\n";
      for (const double *v = begin; v != end; v++) { f << *v << "\n"; }
   };
   auto field = [&](const char *what, const char *fec, int order, int vdim, const double *begin, const double *end) {
      std::ofstream f(name(what).c_str());
      if (f) { values(f, fec, order, vdim, begin, end); }
      return (bool)f;
   };
   const double *x = S.data(), *v = x + H1V, *e = v + H1V;
   std::ofstream mesh(name("mesh").c_str());
   if (!mesh) { return false; }
   mesh << "LGH mesh v1.0\n\n# structured " << (dim == 3 ? "hexahedral" : (dim == 2 ? "quadrilateral" : "segment"))
        << " zones; node ids of a zone in lexicographic order of its (order+1)^dim H1 nodes\n\ndimension\n" << dim
        << "\n\nelements\n" << d.NE << "\n";
   const int geom = (dim == 3) ? 5 : (dim == 2 ? 3 : 1); // MFEM geometry ids: CUBE, SQUARE, SEGMENT
   for (int z = 0; z < d.NE; z++)
   {
      mesh << 1 << " " << geom;
      for (int k = 0; k < d.ND; k++) { mesh << " " << d.h1map[(size_t)z * d.ND + k]; }
      mesh << "\n";
   }
   mesh << "\nnodes\n";
   values(mesh, "H1", ok, dim, x, v);
   mesh.close();
   // (L2_T2: the positive (Bernstein) basis, as the reference's l2_fec)
   return field("rho", "L2_T2", ot, 1, rho.data(), rho.data() + rho.size()) && field("v", "H1", ok, dim, v, e) && field("e", "L2_T2", ot, 1, e, x + S.size());
}

// The derived blocks of a dump as the file holds them, in the order of the table of DESIGN.md §7f: point by point, vectors and
// tensors padded with zeros to 3 and 3 x 3 (the 2D vorticity is the z component).  vort_buf / grad_buf hold the padded copies
// the returned fields point into.
static std::vector<VtuField> DerivedVtuFields(unsigned mask, int dim, long NP, const DerivedBlocks<const double> &b, std::vector<double> &vort_buf,
                                              std::vector<double> &grad_buf)
{
   std::vector<VtuField> extra;
   const int nv = (dim == 3) ? 3 : (dim == 2 ? 1 : 0);
   if (mask & H::DERIVED_DIV) { extra.push_back({"div_v", 1, b.div}); }
   if (mask & H::DERIVED_VORT)
   {
      vort_buf.assign(3 * (size_t)NP, 0.0);
      for (int c = 0; c < nv; c++)
      {
         for (long i = 0; i < NP; i++) { vort_buf[3 * i + (dim == 2 ? 2 : c)] = b.vort[c * NP + i]; }
      }
      extra.push_back({"vorticity", 3, vort_buf.data()});
   }
   if (mask & H::DERIVED_GRAD)
   {
      grad_buf.assign(9 * (size_t)NP, 0.0);
      for (int a = 0; a < dim; a++)
      {
         for (int c = 0; c < dim; c++)
         {
            for (long i = 0; i < NP; i++) { grad_buf[9 * i + 3 * a + c] = b.grad[(a * dim + c) * NP + i]; }
         }
      }
      extra.push_back({"velocity_gradient", 9, grad_buf.data()});
   }
   if (mask & H::DERIVED_DETJ) { extra.push_back({"detJ", 1, b.detj}); }
   if (mask & H::DERIVED_CS) { extra.push_back({"sound_speed", 1, b.cs}); }
   return extra;
}

// -peaks: the records of point set `face_set` (-1: the volume) as the PointData arrays of its dump, behind the -pv-fields arrays:
// one copy of the block to `host`, which the returned fields point into.  p_last is not written; arrival_time only with
// -peaks-arrival.  (The caller has synchronised the stream since the last update.)
static void AppendRecordFields(const laghos_sim *s, int face_set, std::vector<double> &host, std::vector<VtuField> &extra)
{
   static const struct { const char *name; int col; } kFields[] = {{"peak_pressure", 0}, {"peak_pressure_time", 1}, {"pressure_impulse", 2}, {"peak_density", 4},
                                                                   {"peak_speed", 5}, {"peak_energy", 6}, {"arrival_time", 7}};
   for (const laghos_sim::RecordSet &rs : s->records)
   {
      if (rs.face_set != face_set) { continue; }
      rs.dev.ToHost(host);
      for (const auto &f : kFields)
      {
         if (f.col == 7 && !s->opt.peaks_arrival_set) { continue; }
         extra.push_back({f.name, 1, host.data() + (size_t)f.col * rs.n});
      }
   }
}

void UpdateRecords(laghos_sim *s, const Vector &rho, bool first)
{
   const Options &o = s->opt;
   const double threshold = o.peaks_arrival_set ? o.peaks_arrival : NAN;
   const double dtr = first ? 0.0 : s->t - s->rec_time; // (the time since the last update, whatever the cadence was)
   for (laghos_sim::RecordSet &rs : s->records)
   {
      s->hydro->UpdateRecords(s->S, rho, o.vis_refine, rs.face_set < 0 ? nullptr : &s->pv_faces[rs.face_set].faces, s->t, dtr, threshold, first, s->rec_scratch,
                              rs.dev);
   }
   s->rec_time = s->t;
   s->rec_updates++;
}

// What a sidecar of this run's records must say about the point sets
static void RecordSetLists(const laghos_sim *s, std::vector<std::string> &tags, std::vector<long> &points)
{
   for (const laghos_sim::RecordSet &rs : s->records)
   {
      tags.push_back(rs.tag);
      points.push_back(rs.n);
   }
}

std::string RecordsFromSidecar(laghos_sim *s, const std::string &piece, const CheckpointHeader &h)
{
   const Options &o = s->opt;
   const std::string path = RecordsSidecarPath(piece);
   if (o.peaks_steps <= 0)
   {
      std::FILE *f = (o.rank == 0) ? std::fopen(path.c_str(), "rb") : nullptr;
      if (f)
      {
         std::fclose(f);
         std::cout << "Restart: " << path << " holds -peaks records; this run has no -peaks and ignores them" << std::endl;
      }
      return "";
   }
   RecordsSidecar sc;
   std::string err;
   std::vector<std::string> tags;
   std::vector<long> points;
   RecordSetLists(s, tags, points);
   int rc = ReadRecordsSidecar(path, sc, err);
   if (rc == REC_OK) { rc = MatchRecordsSidecar(path, sc, h.state_fp, o.vis_refine, o.peaks_arrival_set ? 1 : 0, o.peaks_arrival, tags, points, err); }
   if (rc == REC_OK && sc.ti != h.ti) { rc = REC_ERR_STATE_FP; err = "records sidecar " + path + ": state_fp: it belongs to cycle " + std::to_string(sc.ti) + ", the checkpoint to cycle " + std::to_string(h.ti); }
   const bool all_ok = o.nranks == 1 || s->hydro->AllReduce(rc == REC_OK ? 1.0 : 0.0, 1) == 1.0;
   if (rc != REC_OK) { return "laghos: -restart with -peaks: " + err + ": restart refused"; }
   if (!all_ok) { return "laghos: -restart with -peaks: another rank refused its records sidecar"; }
   for (size_t k = 0; k < s->records.size(); k++)
   {
      if (s->records[k].n > 0) { s->records[k].dev.FromHost(sc.blocks[k]); }
   }
   s->rec_time = sc.time;
   return "";
}

// The sidecar of checkpoint piece `piece` (state fingerprint state_fp, cycle ti_now): the blocks to the host, then the file
static bool WriteRecordsBeside(laghos_sim *s, const std::string &piece, int ti_now, const unsigned long long state_fp[2], std::string &err)
{
   const Options &o = s->opt;
   RecordsSidecar sc;
   sc.state_fp[0] = state_fp[0]; sc.state_fp[1] = state_fp[1];
   sc.ti = ti_now; sc.time = s->rec_time; sc.R = o.vis_refine;
   sc.threshold_set = o.peaks_arrival_set ? 1 : 0; sc.threshold = o.peaks_arrival;
   RecordSetLists(s, sc.tags, sc.points);
   s->hydro->Sync();
   for (const laghos_sim::RecordSet &rs : s->records)
   {
      sc.blocks.emplace_back();
      if (rs.n > 0) { rs.dev.ToHost(sc.blocks.back()); }
   }
   return WriteRecordsSidecar(RecordsSidecarPath(piece), sc, err) == REC_OK;
}

std::string FaceSetDir(const std::string &basename, const std::string &tag) { return basename + "_" + tag; }

// What rank 0 adds to the pieces of a dump under <basename>_<tag>: the .pvtu of a multi-rank cycle, and the collection `pvd`
// rewritten with all dumps so far (it names the pieces relative to its own directory).
enum PieceKind { VOLUME_PIECES, FACE_PIECES, CONTOUR_PIECES };
static bool WriteCollection(const laghos_sim *s, const std::string &tag, const std::string &pvd, PieceKind kind, const std::vector<VtuField> &extra,
                            int cycle)
{
   const Options &o = s->opt;
   if (o.rank != 0) { return true; }
   const std::string dir = FaceSetDir(o.basename, tag);
   const size_t slash = o.basename.find_last_of('/');
   const std::string rel_dir = FaceSetDir(slash == std::string::npos ? o.basename : o.basename.substr(slash + 1), tag);
   if (o.nranks > 1)
   {
      const bool ok = (kind == FACE_PIECES)      ? WritePvtuFaces(dir, cycle, s->t, o.nranks, extra)
                      : (kind == CONTOUR_PIECES) ? WritePvtuContour(dir, cycle, s->t, o.nranks, extra)
                                                 : WritePvtuFields(dir, cycle, s->t, o.nranks, extra);
      if (!ok) { return false; }
   }
   return WritePvd(pvd, rel_dir, s->pv_times, s->pv_cycles, o.nranks);
}

// One `-paraview` dump of the state at cycle `cycle` (laghos.cpp:691-701, :845-871): lattice values on the GPU, one
// copy to the host, <basename>_paraview/cycle_<cycle>[.<rank>].vtu; rank 0 adds the .pvtu of a multi-rank cycle and
// rewrites <basename>.pvd.  rho: the density of this state where the caller has projected it already.
// (DumpVis below has entered the dump into pv_times / pv_cycles.)
static bool DumpParaview(laghos_sim *s, int cycle, const Vector *rho)
{
   const Options &o = s->opt;
   auto &hydro = *s->hydro;
   const int dim = s->disc->dim, R = o.vis_refine;
   const long NP = hydro.SamplePoints(R);
   Laps laps(s->pv_seconds);
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
   laps.Lap();
   s->pv_dev.ToHost(s->pv_host);
   laps.Lap();
   const double *h = s->pv_host.data();
   const std::string dir = FaceSetDir(o.basename, "paraview");
   std::vector<VtuField> extra;
   std::vector<double> vort_buf, grad_buf;
   if (o.pv_fields) { extra = DerivedVtuFields(o.pv_fields, dim, NP, DerivedBlocks<const double>(h + base, dim, NP), vort_buf, grad_buf); }
   AppendRecordFields(s, -1, s->rec_host, extra);
   const bool ok = WriteVtuFields(dir, dim, s->disc->NE, R + 1, h, h + dim * NP, h + 2 * dim * NP, h + (2 * dim + 1) * NP,
                                  h + (2 * dim + 2) * NP, extra, cycle, s->t, o.rank, o.nranks) &&
                   WriteCollection(s, "paraview", o.basename + ".pvd", VOLUME_PIECES, extra, cycle);
   laps.Lap();
   if (!ok)
   {
      s->error = "cannot write the -paraview files under " + dir;
      std::fprintf(stderr, "%s\n", s->error.c_str());
   }
   return ok;
}

// The faces of this rank's zones on the boundary of the GLOBAL mesh (axis < 0), or on node plane K of the global zone grid along
// `axis`: from the driver's own structured coordinates - zone j is the structured zone elem_perm[j] of the rank's block, which
// starts at Partition::eoff in the global grid of CartMesh::ne zones - so the selection holds under -renumber and on several
// ranks, and an inter-rank interface is no boundary.  Ascending (zone, face).
std::vector<int> SelectFaces(const Discretization &d, int axis, int K)
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

void SampleFaceSet(laghos_sim *s, laghos_sim::FaceSet &fs, const Vector &rho, int R, unsigned mask, std::vector<double> &host, Laps &laps)
{
   s->hydro->SampleFaces(s->S, rho, R, fs.faces, mask, fs.dev);
   s->hydro->Sync();
   laps.Lap();
   fs.dev.ToHost(host);
   laps.Lap();
}

// The `-pv-surface` / `-pv-slice` files of the state at cycle `cycle`: per face set the lattice values on the GPU, one copy to
// the host, <basename>_<tag>/cycle_<cycle>[.<rank>].vtu (a rank without faces writes an empty piece); rank 0 adds the .pvtu
// of a multi-rank cycle and rewrites <basename>_<tag>.pvd.
static bool DumpFaces(laghos_sim *s, int cycle, const Vector &rho)
{
   const Options &o = s->opt;
   const int dim = s->disc->dim, R = o.vis_refine;
   for (size_t k = 0; k < s->pv_faces.size(); k++)
   {
      laghos_sim::FaceSet &fs = s->pv_faces[k];
      const int nfaces = (int)fs.faces.size() / 2;
      const long NPt = s->hydro->FacePoints(R, nfaces);
      Laps laps(s->pvf_seconds);
      SampleFaceSet(s, fs, rho, R, o.pv_fields, s->pv_host, laps);
      const double *x = s->pv_host.data(), *v = x + dim * NPt, *e = v + dim * NPt, *r = e + NPt, *p = r + NPt;
      const DerivedBlocks<const double> b(p + NPt, dim, NPt); // (the area vectors follow them)
      std::vector<double> vort_buf, grad_buf;
      std::vector<VtuField> extra = DerivedVtuFields(o.pv_fields, dim, NPt, b, vort_buf, grad_buf);
      AppendRecordFields(s, (int)k, s->rec_host, extra);
      const std::string dir = FaceSetDir(o.basename, fs.tag);
      const bool ok = WriteVtuFaces(dir, dim, nfaces, fs.faces.data(), R + 1, x, v, e, r, p, extra, b.end, cycle, s->t, o.rank, o.nranks) &&
                      WriteCollection(s, fs.tag, dir + ".pvd", FACE_PIECES, extra, cycle);
      laps.Lap();
      if (!ok)
      {
         s->error = "cannot write the -pv-" + std::string(fs.tag == "surface" ? "surface" : "slice") + " files under " + dir;
         std::fprintf(stderr, "%s\n", s->error.c_str());
         return false;
      }
   }
   return true;
}

void SampleContour(laghos_sim *s, const laghos_sim::ContourSet &cs, const Vector &rho, int R, unsigned mask, std::vector<double> &host,
                   std::vector<int> &zone, long *n_prims, long *n_skipped, Laps &laps)
{
   s->hydro->Contour(s->S, rho, R, cs.field, cs.spec.coef, cs.spec.value, mask, s->pvc_lattice, s->pvc_work, s->pvc_dev, zone, n_prims, n_skipped);
   laps.Lap();
   s->pvc_dev.ToHost(host);
   laps.Lap();
}

// The `-pv-iso` / `-pv-plane` files of the state at cycle `cycle`: per contour the lattice values, the contour and the vertex values
// on the GPU, one copy to the host, <basename>_<tag>/cycle_<cycle>[.<rank>].vtu (a rank the surface does not touch writes an
// empty piece); rank 0 adds the .pvtu of a multi-rank cycle and rewrites <basename>_<tag>.pvd.
static bool DumpContours(laghos_sim *s, int cycle, const Vector &rho)
{
   const Options &o = s->opt;
   const int dim = s->disc->dim, R = o.vis_refine;
   s->pvc_prims = 0;
   for (const laghos_sim::ContourSet &cs : s->pv_contours)
   {
      Laps laps(s->pvc_seconds);
      long n = 0, nskip = 0;
      SampleContour(s, cs, rho, R, o.pv_fields, s->pv_host, s->pvc_zone, &n, &nskip, laps);
      s->pvc_prims += n;
      const long nv = dim * n;
      const double *x = s->pv_host.data(), *v = x + dim * nv, *e = v + dim * nv, *r = e + nv, *p = r + nv;
      const DerivedBlocks<const double> b(p + nv, dim, nv);
      std::vector<double> vort_buf, grad_buf;
      const std::vector<VtuField> extra = DerivedVtuFields(o.pv_fields, dim, nv, b, vort_buf, grad_buf);
      const std::string dir = FaceSetDir(o.basename, cs.spec.tag);
      const bool ok = WriteVtuContour(dir, dim, n, s->pvc_zone.data(), x, v, e, r, p, extra, cs.spec.value, cycle, s->t, o.rank, o.nranks) &&
                      WriteCollection(s, cs.spec.tag, dir + ".pvd", CONTOUR_PIECES, extra, cycle);
      laps.Lap();
      if (!ok)
      {
         s->error = "cannot write the -pv-" + std::string(cs.spec.field == "plane" ? "plane" : "iso") + " files under " + dir;
         std::fprintf(stderr, "%s\n", s->error.c_str());
         return false;
      }
   }
   return true;
}

bool DumpVis(laghos_sim *s, int cycle, const Vector *rho)
{
   const Options &o = s->opt;
   if (!o.paraview && !o.LatticeDumps()) { return true; }
   s->pv_times.push_back(s->t);
   s->pv_cycles.push_back(cycle);
   if (o.LatticeDumps() && !rho)
   {
      s->hydro->ComputeDensity(s->S, s->pv_rho); // (one projection for all)
      rho = &s->pv_rho;
   }
   if (o.paraview && !DumpParaview(s, cycle, rho)) { return false; }
   if (o.FaceDumps() && !DumpFaces(s, cycle, *rho)) { return false; }
   return !o.ContourDumps() || DumpContours(s, cycle, *rho);
}

// The fingerprint of this rank's state (own, lgh_vec_fingerprint at offset 0) and of the whole run (all): on one rank the
// same two words; on several ranks the two words of every rank are gathered (lgh_allreduce sums of 32-bit halves, every
// rank contributing its own slots: exact in doubles) and `all` is the host fingerprint of the 2 * nranks words in rank
// order.  Collective on several ranks.
bool StateFingerprint(laghos_sim *s, unsigned long long own[2], unsigned long long all[2])
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

// One checkpoint of the state after accepted step ti_now: fingerprint on the device, one copy to the host, the host fingerprint of
// the copy (the two must agree), then the file of this rank, CheckpointPiece(stem).  On several ranks every rank learns whether
// all pieces are complete.  Collective.
bool WriteCheckpointPiece(laghos_sim *s, const std::string &stem, int ti_now, std::string *piece_out)
{
   const Options &o = s->opt;
   const Discretization &d = *s->disc;
   if (!DrainGauges(s)) { return false; } // -gauges: the file holds every sample up to this cycle before the checkpoint exists
   Laps laps(s->ckpt_seconds);
   unsigned long long own[2], all[2];
   if (!StateFingerprint(s, own, all)) { return false; }
   laps.Lap();
   s->S.ToHost(s->ckpt_host);
   laps.Lap();
   const std::string piece = CheckpointPiece(stem, o.nranks, o.rank);
   const bool ok = WriteAndAgree(s, true, "", "checkpoint " + stem + ": another rank could not write its piece", [&](std::string &err) {
      unsigned long long hfp[2] = {0ULL, 0ULL};
      FingerprintWords(s->ckpt_host.data(), (long)s->ckpt_host.size(), 0ULL, hfp);
      bool written = hfp[0] == own[0] && hfp[1] == own[1];
      if (!written) { err = "checkpoint: the state gives " + Hex32(own) + " on the device and " + Hex32(hfp) + " after the copy to the host: not written"; }
      else
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
         written = WriteCheckpoint(piece, h, s->ckpt_host.data(), (long)s->ckpt_host.size(), s->pv_times.data(), cyc.data(), (long)cyc.size(), err) == CKPT_OK;
         // -peaks: the records beside the piece, before anything (`latest`) names the checkpoint
         if (written && o.peaks_steps > 0) { written = WriteRecordsBeside(s, piece, ti_now, own, err); }
      }
      laps.Lap();
      return written;
   });
   if (!ok) { return false; }
   s->ckpt.Written(ti_now);
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
      if (o.peaks_steps > 0) { (void)std::remove(RecordsSidecarPath(s->ckpt_mine.front()).c_str()); }
      s->ckpt_mine.erase(s->ckpt_mine.begin());
   }
   return true;
}

// One row of the `-hist` file for the state as it stands, cycle `cycle`: the diagnostics on the GPU (collective), the line by rank 0,
// flushed.
static bool HistoryRecord(laghos_sim *s, int cycle)
{
   double d[LGH_DIAG_COUNT];
   s->hydro->Diagnostics(s->S, d);
   const bool ok = WriteAndAgree(s, false, "cannot write the -hist file: ", "rank 0 could not write the -hist file", [&](std::string &err) {
      return HistoryAppend(s->hist, HistoryRow(cycle, s->t, s->dt, s->steps, s->repeats, d, s->energy_init), err);
   });
   if (ok) { s->hist_when.Written(cycle); }
   return ok;
}

// Opens the `-hist` file on rank 0: a new one, or - a restart from cycle `resume_cycle` >= 0 - the existing one with its later rows dropped.
static bool HistoryOpen(laghos_sim *s, int resume_cycle)
{
   return WriteAndAgree(s, false, "cannot write the -hist file: ", "rank 0 could not open the -hist file", [&](std::string &err) {
      const std::string path = HistoryPath(s->opt.basename);
      return (resume_cycle < 0) ? HistoryStart(s->hist, path, err) : HistoryResume(s->hist, path, resume_cycle, err);
   });
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

// The `-prof` file of the state as it stands, cycle `cycle`: the table on the GPU (collective), the file by rank 0.
static bool ProfileRecord(laghos_sim *s, int cycle)
{
   auto &hydro = *s->hydro;
   const lgh_profile_spec &sp = s->prof_spec;
   long n_excl = 0;
   hydro.Profile(s->S, sp, s->prof_rows.data(), &n_excl);
   const bool ok = WriteAndAgree(s, false, "cannot write the -prof file: ", "rank 0 could not write the -prof file", [&](std::string &err) {
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
      return ProfileWrite(ProfilePath(s->opt.basename, cycle),
                          ProfileText(cycle, s->t, s->prof_axis, sp.origin, sp.lo, sp.hi, sp.nbins, n_excl, s->prof_rows.data(),
                                      s->prof_exact ? exact.data() : nullptr),
                          err);
   });
   if (ok) { s->prof_when.Written(cycle); }
   return ok;
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

// The `-map` file of the state as it stands, cycle `cycle`: the rows on the GPU (collective), the file by rank 0.
static bool MapRecord(laghos_sim *s, int cycle)
{
   const lgh_map_spec &sp = s->map_spec;
   long n_excl = 0;
   s->hydro->Map(s->S, sp, s->map_rows.data(), &n_excl);
   const bool ok = WriteAndAgree(s, false, "cannot write the -map file: ", "rank 0 could not write the -map file", [&](std::string &err) {
      return WriteVti(MapDir(s->opt.basename), s->disc->dim, sp.n, sp.lo, sp.hi, s->map_rows.data(), n_excl, cycle, s->t, err);
   });
   if (ok) { s->map_when.Written(cycle); }
   return ok;
}

// The lines of the `-loads` file for the state as it stands, cycle `cycle`: the density and the loads on the GPU (collective; a rank
// without faces takes part), the lines by rank 0, flushed.
static bool LoadsRecord(laghos_sim *s, int cycle)
{
   long n_excl = 0;
   s->hydro->ComputeDensity(s->S, s->loads_rho);
   s->hydro->Loads(s->S, s->loads_rho, (int)s->loads_names.size(), s->loads_faces, s->loads_rows.data(), &n_excl);
   const bool ok = WriteAndAgree(s, false, "cannot write the -loads file: ", "rank 0 could not write the -loads file", [&](std::string &err) {
      return HistoryAppend(s->loads_file, LoadsText(cycle, s->t, s->loads_names, s->loads_rows.data()), err);
   });
   if (ok) { s->loads_when.Written(cycle); }
   return ok;
}

// Opens the `-loads` file on rank 0 as HistoryOpen opens the `-hist` file
static bool LoadsOpen(laghos_sim *s, int resume_cycle)
{
   return WriteAndAgree(s, false, "cannot write the -loads file: ", "rank 0 could not open the -loads file", [&](std::string &err) {
      const std::string path = LoadsPath(s->opt.basename);
      LoadsFileInit(s->loads_file);
      return (resume_cycle < 0) ? HistoryStart(s->loads_file, path, err) : HistoryResume(s->loads_file, path, resume_cycle, err);
   });
}

std::vector<double> GaugePositions(const Options &o)
{
   std::vector<double> pts;
   for (const std::vector<Options::GaugePoint> *list : {&o.gauge_points, &o.gauge_file_points})
   {
      for (const Options::GaugePoint &p : *list) { pts.insert(pts.end(), p.x, p.x + 3); }
   }
   return pts;
}

bool DrainGauges(laghos_sim *s)
{
   if (s->gauges_handle < 0 || s->gauges_pending.empty()) { return true; } // (the ranks sample in step: all or none have samples)
   const int n = s->gauges_n;
   const int got = s->hydro->DrainGauges(s->gauges_handle, n, s->gauges_rows);
   if (got != (int)s->gauges_pending.size()) { return SimFail(s, "-gauges: the device buffer held " + std::to_string(got) + " samples, " + std::to_string(s->gauges_pending.size()) + " were taken"); }
   const bool ok = WriteAndAgree(s, false, "cannot write the -gauges file: ", "rank 0 could not write the -gauges file", [&](std::string &err) {
      std::string text;
      for (int k = 0; k < got; k++) { text += GaugesText(s->gauges_pending[k].first, s->gauges_pending[k].second, n, s->gauges_rows.data() + (size_t)k * n * LGH_GAUGE_COLS); }
      return HistoryAppend(s->gauges_file, text, err);
   });
   s->gauges_pending.clear();
   return ok;
}

// One sample of the `-gauges` series for the state as it stands, cycle `cycle`: one kernel on the stream and a note of (cycle, t) -
// no host wait; the lines are written when the buffer is drained (here once it is full).
static bool GaugesRecord(laghos_sim *s, int cycle)
{
   s->hydro->SampleGauges(s->gauges_handle, s->S);
   s->gauges_pending.emplace_back(cycle, s->t);
   s->gauges_when.Written(cycle);
   return (int)s->gauges_pending.size() < s->opt.gauge_buffer || DrainGauges(s);
}

// Opens the `-gauges` file on rank 0 as HistoryOpen opens the `-hist` file
static bool GaugesOpen(laghos_sim *s, int resume_cycle)
{
   return WriteAndAgree(s, false, "cannot write the -gauges file: ", "rank 0 could not open the -gauges file", [&](std::string &err) {
      const std::string path = GaugesPath(s->opt.basename);
      GaugesFileInit(s->gauges_file);
      return (resume_cycle < 0) ? HistoryStart(s->gauges_file, path, err) : HistoryResume(s->gauges_file, path, resume_cycle, err);
   });
}

// The periodic outputs in the order a step writes them (the gauges first: a checkpoint of the same cycle drains their sample too)
static const struct { Periodic laghos_sim::*when; bool (*write)(laghos_sim *, int cycle); } kPeriodic[] = {
   {&laghos_sim::gauges_when, GaugesRecord}, {&laghos_sim::ckpt, PeriodicCheckpoint}, {&laghos_sim::hist_when, HistoryRecord}, {&laghos_sim::prof_when, ProfileRecord}, {&laghos_sim::map_when, MapRecord},
   {&laghos_sim::loads_when, LoadsRecord}};

void SetUpOutputs(laghos_sim *s, const std::vector<double> &S0, const std::vector<double> &rho0_l2)
{
   const Options &o = s->opt;
   s->gauges_when.every = o.gauge_steps;
   if (o.gauge_steps > 0) // (the options have been held against the mesh: every point lies in it)
   {
      std::vector<int> zone;
      std::vector<double> xi;
      (void)ResolveGauges(*s->disc, GaugePositions(o), zone, xi, nullptr);
      s->gauges_n = (int)zone.size();
      s->gauges_handle = s->hydro->CreateGauges(zone, xi, S0, rho0_l2, o.gauge_buffer);
   }
   s->ckpt.every = o.ckpt_steps;
   s->ckpt.at_start = false;
   s->ckpt.again_after_repeat = true;
   s->hist_when.every = o.hist_steps;
   s->prof_when.every = o.prof_steps;
   s->map_when.every = o.map_steps;
   if (o.prof_steps > 0) { ProfileSetup(s, S0); }
   if (o.map_steps > 0) { MapSetup(s, S0); }
   s->loads_when.every = o.loads_steps;
   if (o.loads_steps > 0)
   {
      LoadsRows(*s->disc, o.loads_planes, s->loads_names, s->loads_faces);
      s->loads_rows.assign(s->loads_names.size() * LGH_LOADS_COLS, 0.0);
   }
   auto face_set = [&](const std::string &tag, int axis, int K) {
      s->pv_faces.emplace_back();
      s->pv_faces.back().tag = tag;
      s->pv_faces.back().faces = SelectFaces(*s->disc, axis, K);
   };
   if (o.pv_surface) { face_set("surface", -1, 0); }
   for (const std::vector<Options::Contour> *list : {&o.pv_isos, &o.pv_planes})
   {
      for (const Options::Contour &c : *list)
      {
         s->pv_contours.emplace_back();
         s->pv_contours.back().spec = c;
         s->pv_contours.back().field = (c.field == "plane") ? (int)H::CONTOUR_PLANE : H::ContourField(c.field);
      }
   }
   for (const auto &sl : o.pv_slices) { face_set(std::string("slice_") + (char)('x' + sl.first) + std::to_string(sl.second), sl.first, sl.second); }
   if (o.peaks_steps > 0) // one record block per material point set, and scratch for the largest (sized once: no allocation between updates)
   {
      long most = 0;
      auto record_set = [&](const std::string &tag, int k) {
         s->records.emplace_back();
         laghos_sim::RecordSet &rs = s->records.back();
         rs.tag = tag;
         rs.face_set = k;
         rs.n = s->hydro->RecordPoints(o.vis_refine, k < 0 ? nullptr : &s->pv_faces[k].faces);
         rs.dev.SetSize(LGH_RECORDS_COLS * rs.n);
         most = std::max(most, rs.n);
      };
      if (o.paraview) { record_set("volume", -1); }
      for (size_t k = 0; k < s->pv_faces.size(); k++) { record_set(s->pv_faces[k].tag, (int)k); }
      s->rec_scratch.SetSize((s->disc->dim + 3) * most);
   }
}

bool OpenPeriodicOutputs(laghos_sim *s, int resume_cycle)
{
   for (const auto &out : kPeriodic) { (s->*out.when).last = resume_cycle; } // (a restart: the run that wrote the checkpoint has them)
   return (s->hist_when.every <= 0 || HistoryOpen(s, resume_cycle)) && (s->loads_when.every <= 0 || LoadsOpen(s, resume_cycle)) &&
          (s->gauges_when.every <= 0 || GaugesOpen(s, resume_cycle));
}

bool WritePeriodicOutputs(laghos_sim *s, Periodic::Moment m, int cycle)
{
   for (const auto &out : kPeriodic)
   {
      if ((s->*out.when).Due(m, cycle, s->last_step) && !out.write(s, cycle)) { return false; }
   }
   return !s->last_step || DrainGauges(s); // (the end of the run)
}

} // namespace laghos
