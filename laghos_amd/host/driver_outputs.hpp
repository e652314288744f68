// driver_outputs.hpp — the simulation object of the driver and everything it writes: the -paraview / -pv-surface / -pv-slice /
// -pv-iso / -pv-plane dumps, -print, checkpoints, the -hist / -prof / -map / -loads / -gauges recorders with the one cadence they and
// -ckpt share, and the -peaks records that live across steps (in the material dumps, and beside every checkpoint piece).
#pragma once

#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "checkpoint.hpp"
#include "gauges_output.hpp"
#include "history.hpp"
#include "laghos_solver.hpp"
#include "loads_output.hpp"
#include "options.hpp"

// When a periodic output is written: at cycle 0, after every accepted step ti with ti % every == 0, after the last step, and -
// when the run ends on a repeated step, on the state of the last accepted one - once more unless that cycle has its output.  A
// restart resumes from a cycle that has it.  The checkpoint differs in two ways: none at cycle 0, and after a repeated last step
// it is written again in any case, because the shortened dt is part of it.
struct Periodic
{
   enum Moment { START, ACCEPTED_STEP, ENDED_ON_REPEAT };
   int every = 0;  // 0: off
   int last = -1;  // the last cycle that has its output
   int count = 0;  // outputs of this run
   bool at_start = true, again_after_repeat = false;
   bool Due(Moment m, int cycle, bool last_step) const
   {
      if (every <= 0) { return false; }
      if (m == START) { return at_start; }
      if (m == ACCEPTED_STEP) { return last_step || cycle % every == 0; }
      return last_step && (again_after_repeat ? cycle > 0 : cycle > last);
   }
   void Written(int cycle) { last = cycle; count++; }
};

// Three laps of wall-clock time, each added to its slot of sum[3] (a dump: GPU work, copy to the host, file write)
struct Laps
{
   using clk = std::chrono::steady_clock;
   double *sum;
   clk::time_point t = clk::now();
   explicit Laps(double *sum3) : sum(sum3) {}
   void Lap()
   {
      const clk::time_point now = clk::now();
      *sum++ += std::chrono::duration<double>(now - t).count();
      t = now;
   }
};

// ---- simulation object driven by main() and by bench.py ------------------------------------
struct laghos_sim
{
   laghos::Options opt;
   std::unique_ptr<laghos::Discretization> disc;
   std::unique_ptr<laghos::hydrodynamics::LagrangianHydroOperator> hydro;
   std::unique_ptr<laghos::ODESolver> ode;
   laghos::Vector S, S_old;
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
   laghos::Vector pv_rho, pv_dev;
   std::vector<double> pv_host;
   double pv_seconds[3] = {0, 0, 0}; // density + sampling (GPU), device-to-host copy, file write
   // -pv-surface / -pv-slice: the face lists of this rank (fixed at the start: the mesh is Lagrangian), in the order of the command
   // line with the surface first; scratch; where the time of their dumps goes
   struct FaceSet
   {
      std::string tag;        // "surface", "slice_z3": the directory is <basename>_<tag>
      std::vector<int> faces; // (zone, local face) pairs in ascending order
      laghos::Vector dev;
   };
   std::vector<FaceSet> pv_faces;
   double pvf_seconds[3] = {0, 0, 0};
   // -pv-iso / -pv-plane: the contours in the order of the command line, the iso-surfaces first; scratch (lattice values, the
   // contour's own arrays, the gathered vertex values); the primitives of this rank in the last dump; where the time goes
   struct ContourSet
   {
      laghos::Options::Contour spec;
      int field = 0; // LagrangianHydroOperator::CONTOUR_*
   };
   std::vector<ContourSet> pv_contours;
   laghos::Vector pvc_lattice, pvc_work, pvc_dev;
   std::vector<int> pvc_zone;
   long pvc_prims = 0;
   double pvc_seconds[3] = {0, 0, 0};
   // The periodic outputs, each with its cadence (`every` is set by SetUpOutputs)
   // -ckpt / -restart: the fingerprint of the set-up arrays, the pieces this run wrote (oldest first; -ckpt-keep removes from
   // this list only), scratch, and where the time of a checkpoint goes
   Periodic ckpt;
   unsigned long long setup_fp[2] = {0, 0};
   std::vector<std::string> ckpt_mine;
   std::vector<double> ckpt_host;
   double ckpt_seconds[3] = {0, 0, 0}; // fingerprint (GPU), device-to-host copy, host fingerprint + file write
   // -hist: the file (rank 0)
   Periodic hist_when;
   laghos::HistoryFile hist;
   // -prof: what is binned (axis, range and origin fixed at the start, from the initial mesh), the table, and the exact Sedov
   // solution where it applies
   Periodic prof_when;
   lgh_profile_spec prof_spec = {};
   char prof_axis = 'x';
   std::vector<double> prof_rows;
   bool prof_exact = false;
   double prof_par[21] = {};
   // -map: the grid (fixed at the start, from the initial mesh)
   Periodic map_when;
   lgh_map_spec map_spec = {};
   std::vector<double> map_rows;
   // -loads: the file (rank 0), the rows and the faces listed under them (fixed at the start), the table and the density
   Periodic loads_when;
   laghos::HistoryFile loads_file;
   std::vector<std::string> loads_names;
   std::vector<int> loads_faces;
   std::vector<double> loads_rows;
   laghos::Vector loads_rho;
   // -peaks: one block of running records per material point set (the volume lattice of -paraview first, then the face sets in
   // their order), on the device; the time of the last update; scratch (the sampled fields; a block on the host); the updates of
   // this run
   struct RecordSet
   {
      std::string tag;   // "volume", or the tag of the face set
      int face_set = -1; // index into pv_faces, -1: the volume
      long n = 0;        // points
      laghos::Vector dev; // LGH_RECORDS_COLS x n, column-major
   };
   std::vector<RecordSet> records;
   double rec_time = 0.0;
   int rec_updates = 0;
   laghos::Vector rec_scratch;
   std::vector<double> rec_host;
   // -gauges: the file (rank 0), the set on the device (the gauges of every rank, in the order of the file) and, per sample it holds,
   // (cycle, t); scratch; the samples of this run
   Periodic gauges_when;
   laghos::HistoryFile gauges_file;
   int gauges_handle = -1, gauges_n = 0;
   std::vector<std::pair<int, double>> gauges_pending;
   std::vector<double> gauges_rows;
   int steps_at_start = 0;             // RK steps the checkpoint of a restart had taken: timing / FOM cover the restarted segment
};

namespace laghos
{

// Sets s->error, prints `laghos: <msg>` on stderr, returns false
bool SimFail(laghos_sim *s, const std::string &msg);
std::string Hex32(const unsigned long long fp[2]);

// What the options ask for, fixed at the start from the initial state S0: the cadences, the -prof axis and range, the -map grid,
// the face lists (collective on several ranks)
void SetUpOutputs(laghos_sim *s, const std::vector<double> &S0, const std::vector<double> &rho0_l2);
// The first thing the periodic outputs do: a restart resumes from cycle resume_cycle >= 0, which has its outputs; -1 starts anew
bool OpenPeriodicOutputs(laghos_sim *s, int resume_cycle);
// Writes the periodic outputs due at this moment for the state as it stands, cycle `cycle`: -gauges, -ckpt, -hist, -prof, -map, -loads
bool WritePeriodicOutputs(laghos_sim *s, Periodic::Moment m, int cycle);
// -gauges: the samples the device buffer holds become lines of the file (collective; nothing to do without pending samples).  The
// driver drains when the buffer is full, before every checkpoint piece is written and after the last step.
bool DrainGauges(laghos_sim *s);
// The gauges of this run as ResolveGauges takes them: 3 doubles per gauge, the command line's first, then the file's
std::vector<double> GaugePositions(const Options &o);

// `-print`: basename_<ti>_{mesh,rho,v,e} from host copies of the state and the density
bool WriteFields(const std::string &basename, int ti, const Discretization &d, int nranks, int rank, const std::vector<double> &S,
                 const std::vector<double> &rho);
// Everything that is written when -paraview writes (cycle 0, ti % vs == 0, the last step): the volume dump, the face dumps and the contour dumps, one
// entry of pv_times / pv_cycles (which the collections list and a checkpoint carries) and one density projection for all.
// rho: the density of this state where the caller (`-print`) has projected it already.
bool DumpVis(laghos_sim *s, int cycle, const Vector *rho = nullptr);
std::string FaceSetDir(const std::string &basename, const std::string &tag);
// The faces of this rank's zones on the boundary of the GLOBAL mesh (axis < 0), or on node plane K of the global zone grid along `axis`
std::vector<int> SelectFaces(const Discretization &d, int axis, int K);
// One contour of the state as it stands into host arrays: the blocks of LagrangianHydroOperator::Contour and the zones (two laps)
void SampleContour(laghos_sim *s, const laghos_sim::ContourSet &cs, const Vector &rho, int R, unsigned mask, std::vector<double> &host,
                   std::vector<int> &zone, long *n_prims, long *n_skipped, Laps &laps);
// One face set of the state as it stands into host arrays: the blocks of LagrangianHydroOperator::SampleFaces (two laps)
void SampleFaceSet(laghos_sim *s, laghos_sim::FaceSet &fs, const Vector &rho, int R, unsigned mask, std::vector<double> &host, Laps &laps);

// -peaks: one update of every record block with the state as it stands (first: the update that starts them, at cycle 0); rho the
// density of this state.  Asynchronous.
void UpdateRecords(laghos_sim *s, const Vector &rho, bool first);
// -peaks on a restart from checkpoint piece `piece` (header h): reads <piece>.rec, holds it against the checkpoint and this run
// (collective on several ranks) and only then takes the blocks and the time of the last update.  Returns the line for stderr when it
// refuses, "" otherwise.  Without -peaks: one line by rank 0 when a sidecar lies there, nothing else.
std::string RecordsFromSidecar(laghos_sim *s, const std::string &piece, const CheckpointHeader &h);

// The fingerprint of this rank's state (own) and of the whole run (all).  Collective on several ranks.
bool StateFingerprint(laghos_sim *s, unsigned long long own[2], unsigned long long all[2]);
// One checkpoint of the state after accepted step ti_now to CheckpointPiece(stem).  Collective.
bool WriteCheckpointPiece(laghos_sim *s, const std::string &stem, int ti_now, std::string *piece_out);

} // namespace laghos
