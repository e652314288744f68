// host_probes.cpp — host-only entry points (laghos_host_*): the set-up code, the file writers and readers of the driver as
// tests and bench.py reach them through ctypes.  None of them sees a simulation object or touches the GPU.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include <vector>

#include "checkpoint.hpp"
#include "fem.hpp"
#include "history.hpp"
#include "gauges_output.hpp"
#include "loads_output.hpp"
#include "map_output.hpp"
#include "records_sidecar.hpp"
#include "vtk_output.hpp"

using namespace laghos;

extern "C"
{

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
// host-only: the writers of the `-pv-iso` / `-pv-plane` pieces (WriteVtuContour, WritePvtuContour); 0 = written.  The arrays are
// host arrays in the layout of LagrangianHydroOperator::Contour over dim * nprims points
int laghos_host_write_vtu_contour(const char *dir, int dim, long nprims, const int *zone, const double *x, const double *v, const double *e,
                                  const double *rho, const double *p, int n_extra, const char *const *names, const int *comps,
                                  const double *const *data, double iso_value, int cycle, double time, int rank, int nranks)
{
   return WriteVtuContour(dir, dim, nprims, zone, x, v, e, rho, p, HostExtra(n_extra, names, comps, data), iso_value, cycle, time, rank, nranks) ? 0 : -1;
}
int laghos_host_write_pvtu_contour(const char *dir, int cycle, double time, int nranks, int n_extra, const char *const *names, const int *comps)
{
   return WritePvtuContour(dir, cycle, time, nranks, HostExtra(n_extra, names, comps, nullptr)) ? 0 : -1;
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
// host-only: the `-peaks` sidecar of a checkpoint piece (records_sidecar.hpp); 0 = done, else a RecordsSidecarError with its message
// in msg.  tags: the nsets tags, blank-separated; points[nsets]; blocks: the record blocks one after the other (LGH_RECORDS_COLS x
// points[k] doubles each).
static std::vector<std::string> SplitBlanks(const char *s)
{
   std::vector<std::string> out;
   const std::string all = s ? s : "";
   for (size_t pos = 0; pos < all.size();)
   {
      const size_t sp = std::min(all.find(' ', pos), all.size());
      if (sp > pos) { out.push_back(all.substr(pos, sp - pos)); }
      pos = sp + 1;
   }
   return out;
}
int laghos_host_write_records_sidecar(const char *path, const unsigned long long *state_fp, long ti, double time, int R, int threshold_set, double threshold,
                                      int nsets, const char *tags, const long *points, const double *blocks, char *msg, int msg_len)
{
   RecordsSidecar r;
   r.state_fp[0] = state_fp[0]; r.state_fp[1] = state_fp[1];
   r.ti = ti; r.time = time; r.R = R; r.threshold_set = threshold_set; r.threshold = threshold;
   r.tags = SplitBlanks(tags);
   std::string err;
   int rc = REC_OK;
   if ((int)r.tags.size() != nsets) { rc = REC_ERR_IO; err = std::string("records sidecar ") + path + ": write: " + std::to_string(r.tags.size()) + " tags for " + std::to_string(nsets) + " point sets"; }
   for (int k = 0; k < nsets && rc == REC_OK; k++)
   {
      const long words = kRecordCols * std::max(points[k], 0L);
      r.points.push_back(points[k]);
      r.blocks.emplace_back(blocks, blocks + words);
      blocks += words;
   }
   if (rc == REC_OK) { rc = WriteRecordsSidecar(path, r, err); }
   CkptMsg(err, msg, msg_len);
   return rc;
}
// ints[4]: ti R threshold_set nsets; dbls[2]: time threshold; tags (tags_len chars) blank-separated; the arrays are written only when
// every check has passed and they fit
int laghos_host_read_records_sidecar(const char *path, unsigned long long *state_fp, long *ints, double *dbls, char *tags, int tags_len, long *points,
                                     int cap_sets, double *blocks, long cap_words, char *msg, int msg_len)
{
   RecordsSidecar r;
   std::string err, all;
   int rc = ReadRecordsSidecar(path, r, err);
   long words = 0;
   for (size_t k = 0; k < r.tags.size(); k++)
   {
      all += (k ? " " : "") + r.tags[k];
      words += (long)r.blocks[k].size();
   }
   if (rc == REC_OK && ((int)r.tags.size() > cap_sets || words > cap_words || (int)all.size() + 1 > tags_len))
   {
      rc = REC_ERR_CAPACITY;
      err = std::string("records sidecar ") + path + ": capacity: " + std::to_string(r.tags.size()) + " point sets and " + std::to_string(words) + " words do not fit the caller's arrays";
   }
   CkptMsg(err, msg, msg_len);
   if (rc != REC_OK) { return rc; }
   state_fp[0] = r.state_fp[0]; state_fp[1] = r.state_fp[1];
   ints[0] = r.ti; ints[1] = r.R; ints[2] = r.threshold_set; ints[3] = (long)r.tags.size();
   dbls[0] = r.time; dbls[1] = r.threshold;
   std::memcpy(tags, all.c_str(), all.size() + 1);
   for (size_t k = 0; k < r.tags.size(); k++)
   {
      points[k] = r.points[k];
      blocks = std::copy(r.blocks[k].begin(), r.blocks[k].end(), blocks);
   }
   return REC_OK;
}
// reads <path> and holds it against what a restarting run expects, as the driver does
int laghos_host_match_records_sidecar(const char *path, const unsigned long long *state_fp, int R, int threshold_set, double threshold, int nsets,
                                      const char *tags, const long *points, char *msg, int msg_len)
{
   RecordsSidecar r;
   std::string err;
   int rc = ReadRecordsSidecar(path, r, err);
   if (rc == REC_OK) { rc = MatchRecordsSidecar(path, r, state_fp, R, threshold_set, threshold, SplitBlanks(tags), std::vector<long>(points, points + nsets), err); }
   CkptMsg(err, msg, msg_len);
   return rc;
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
// host-only: the `-loads` file (loads_output.hpp) the same way.  The header line; the lines of one cycle for nrows rows named by
// `names` (blank-separated) from nrows x LGH_LOADS_COLS doubles (returns the length, -1 when buf is too small); and the file
// operation of laghos_host_history_write on a file with the header of the loads file.
const char *laghos_host_loads_header() { return kLoadsHeader; }
int laghos_host_loads_text(long cycle, double t, const char *names, const double *rows, char *buf, int len)
{
   std::vector<std::string> nm;
   const std::string all = names ? names : "";
   for (size_t pos = 0; pos < all.size();)
   {
      const size_t sp = std::min(all.find(' ', pos), all.size());
      if (sp > pos) { nm.push_back(all.substr(pos, sp - pos)); }
      pos = sp + 1;
   }
   const std::string r = LoadsText(cycle, t, nm, rows);
   if ((int)r.size() + 1 > len) { return -1; }
   std::memcpy(buf, r.c_str(), r.size() + 1);
   return (int)r.size();
}
int laghos_host_loads_write(const char *path, long keep_upto, const char *lines, long *rows_in_file, char *msg, int msg_len)
{
   HistoryFile h;
   LoadsFileInit(h);
   std::string err;
   bool ok = (keep_upto < 0) ? HistoryStart(h, path, err) : HistoryResume(h, path, keep_upto, err);
   const std::string all = lines ? lines : "";
   if (ok && !all.empty()) { ok = HistoryAppend(h, all, err); }
   CkptMsg(err, msg, msg_len);
   if (rows_in_file) { *rows_in_file = h.rows; }
   return ok ? 0 : -1;
}
// host-only: the `-gauges` file (gauges_output.hpp) the same way - the header line and the lines of one sample of n gauges from n x
// LGH_GAUGE_COLS doubles (returns the length, -1 when buf is too small) -, the three 1-D bases at one abscissa (BasisAt: D1D, D1D and
// L1D doubles), and the location of a point in the initial mesh given by its break points (LocateInitial: brk holds nbrk[0] +
// nbrk[1] + nbrk[2] break points, axis by axis; 0 = found, -1 = refused: outside the mesh, not finite, or no mesh).
const char *laghos_host_gauges_header() { return kGaugesHeader; }
int laghos_host_gauges_text(long cycle, double t, int n, const double *rows, char *buf, int len)
{
   const std::string r = GaugesText(cycle, t, n, rows);
   if ((int)r.size() + 1 > len) { return -1; }
   std::memcpy(buf, r.c_str(), r.size() + 1);
   return (int)r.size();
}
int laghos_host_basis_at(int order_v, int order_e, double xi, double *Bh, double *Gh, double *Bl)
{
   if (order_v < 1 || order_e < 0 || !Bh || !Gh || !Bl) { return -1; }
   BasisAt(order_v, order_e, xi, Bh, Gh, Bl);
   return 0;
}
int laghos_host_locate_initial(int dim, const int *nbrk, const double *brk, const double *X, int *zone_ijk, double *xi)
{
   if (dim < 1 || dim > 3 || !nbrk || !brk || !X || !zone_ijk || !xi) { return -1; }
   CartMesh m;
   m.dim = dim;
   for (int a = 0; a < dim; a++)
   {
      if (nbrk[a] < 2) { return -1; }
      m.brk[a].assign(brk, brk + nbrk[a]);
      brk += nbrk[a];
   }
   double x3[3] = {0, 0, 0};
   std::copy(X, X + dim, x3);
   return LocateInitial(m, x3, zone_ijk, xi) ? 0 : -1;
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

} // extern "C"
