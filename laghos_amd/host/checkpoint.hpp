// checkpoint.hpp — checkpoint files of the driver's `-ckpt` / `-restart`.  Host only, no GPU code: like
// vtk_output.cpp it can be compiled and run alone on a CPU.  The reference has no restart (/root/reference/laghos.cpp runs
// every problem from t = 0); nothing here replaces reference code.
//
// One file per rank, little endian:
//   header   ASCII `key value` lines, first line "LGHCKPT 1", last line "end", padded with '\n' to a multiple of 4096 bytes;
//            every double as the 16 hex digits of its bit pattern (a decimal copy after '#' is for the reader's eyes only)
//   payload  S (state_words float64), then the times (float64) and cycles (int64) of the ParaView dumps so far
//   trailer  the fingerprint (include/lgh_fingerprint.h, two uint64) of everything before it, taken as 64-bit words
#pragma once
#include <string>
#include <vector>

namespace laghos
{

struct CheckpointHeader
{
   int dim = 0, problem = 0, order_v = 0, order_e = 0, Q1D = 0;
   long NE = 0, global_NE = 0, N = 0;
   int nranks = 1, rank = 0, pgrid[3] = {1, 1, 1};
   int ode_solver = 0, cg_max_iter = 0;
   double cfl = 0, cg_tol = 0;
   double t = 0, dt = 0;
   int ti = 0;      // accepted steps so far
   int steps = 0;   // RK steps including repeated ones
   int repeats = 0;
   double energy_init = 0;
   int checks = 0, checks_ok = 1;
   unsigned long long setup_fp[2] = {0, 0}; // fingerprint of S0 | rho0_l2 | gamma | rho0_q | h1map (SetupFingerprint)
   unsigned long long state_fp[2] = {0, 0}; // fingerprint of S at offset 0 (the writer computes it from the payload)
   // set by the writer / reader
   long header_bytes = 0, state_words = 0, pv_dumps = 0;
};

struct Checkpoint
{
   CheckpointHeader h;
   std::vector<double> S, pv_times;
   std::vector<long long> pv_cycles;
};

// what failed: every code has its own message (file name + check)
enum CheckpointError
{
   CKPT_OK = 0,
   CKPT_ERR_IO = 1,        // cannot open / write / rename
   CKPT_ERR_MAGIC = 2,     // first line is not "LGHCKPT <n>"
   CKPT_ERR_VERSION = 3,   // a version other than 1
   CKPT_ERR_HEADER = 4,    // header_bytes missing / not a multiple of 4096 / beyond the file; a key missing or unreadable
   CKPT_ERR_TRUNCATED = 5, // the file is shorter than header + payload + trailer
   CKPT_ERR_SIZE = 6,      // the file is longer than state_words and the dump count say
   CKPT_ERR_TRAILER = 7,   // the fingerprint of header + payload is not the trailer
   CKPT_ERR_STATE_FP = 8,  // the fingerprint of S is not the header's state_fp
   CKPT_ERR_CAPACITY = 9   // (host probe) the caller's arrays are too small
};

// "<basename>_restart", "cycle_<ti, 6 digits>.lgr", and the piece of one rank (".<rank>" appended on several ranks)
std::string CheckpointDir(const std::string &basename);
std::string CheckpointName(int ti);
std::string CheckpointPiece(const std::string &stem, int nranks, int rank);

// host fingerprint of n 64-bit words at `offset`, combined into fp (add, xor)
void FingerprintWords(const void *words, long n, unsigned long long offset, unsigned long long fp[2]);
// setup_fp: the fingerprint of the concatenation S0 | rho0_l2 | gamma | rho0_q | h1map (entries widened to 64 bits)
void SetupFingerprint(const std::vector<double> &S0, const std::vector<double> &rho0_l2, const std::vector<double> &gamma,
                      const std::vector<double> &rho0_q, const std::vector<int> &h1map, unsigned long long fp[2]);

// Writes <path>.tmp, flushes it to the disk and renames it to <path>: a killed job never leaves a half-written file under
// a final name.  h.state_fp, header_bytes, state_words and pv_dumps are set from the arrays.  Returns a CheckpointError.
int WriteCheckpoint(const std::string &path, CheckpointHeader h, const double *S, long nS, const double *pv_times,
                    const long long *pv_cycles, long npv, std::string &err);
// Reads and checks <path>, in this order: magic and version, header_bytes, the file size against state_words, the
// trailer, state_fp of the payload.  `out` is only assigned when every check has passed.
int ReadCheckpoint(const std::string &path, Checkpoint &out, std::string &err);

// <dir>/latest: one line, the name of the newest complete checkpoint (written to a .tmp and renamed)
bool WriteLatest(const std::string &dir, const std::string &name);
bool ReadLatest(const std::string &dir, std::string &name);

} // namespace laghos
