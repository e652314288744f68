// history.hpp — the `-hist` time history: <basename>_history.csv, one row of conserved integrals and mesh-health figures
// (lgh_diagnostics) per recorded cycle.  The reference prints one number, "Energy diff", after the last step.
//
// A text file: the header line below, then one line per row, columns separated by one blank in the header's order.
// Integers (cycle, rk_steps, repeats, detj_min_rank, detj_min_zone, the n_* counts) are printed as integers, doubles with
// %.17g (inf, -inf, nan for the non-finite ones): equal bits give equal bytes and every value reads back exactly.  The file
// is flushed after every row, so a killed run leaves at most one partial line behind, which a restart drops.
// File logic only - no GPU, no context; the driver (laghos.cpp) supplies the figures.
//
// The file logic - start, resume, append - knows nothing of the columns but that a line starts with its cycle: HistoryFile
// carries the header line it writes and expects, so the `-loads` file (loads_output.hpp: several lines per cycle) goes the same way.
#pragma once
#include <cstdio>
#include <string>

namespace laghos
{

extern const char *const kHistoryHeader; // the first line, without its newline

std::string HistoryPath(const std::string &basename); // <basename>_history.csv

// One row, with its newline.  diag: the LGH_DIAG_COUNT doubles of lgh_diagnostics; total = ie + ke, d_total = total - energy_init.
std::string HistoryRow(long cycle, double t, double dt, long rk_steps, long repeats, const double *diag, double energy_init);

// what a row is made of: " %.17g" (" nan" for every NaN), " %lld" (no blank in front of the first cell of a line)
void AppendDouble(std::string &s, double v);
void AppendInt(std::string &s, long long v, bool first = false);

struct HistoryFile
{
   const char *header = kHistoryHeader; // the first line of this file, without its newline
   const char *what = "history";        // ... and what the messages call it
   std::string path;
   std::FILE *f = nullptr;
   long rows = 0; // rows in the file: kept by a restart + appended (lines kept + appends)
   ~HistoryFile() { Close(); }
   void Close();
};

// A new file with the header (the directory chain of the path is created); an existing file is replaced.
bool HistoryStart(HistoryFile &h, const std::string &path, std::string &err);
// `-restart` from cycle `keep_upto`: the rows of an existing file with cycle <= keep_upto stay, later ones and a partial last line
// are dropped, and the file is open for appending; a missing (or empty) file is started anew.  A file whose first line is not
// the header is refused.
bool HistoryResume(HistoryFile &h, const std::string &path, long keep_upto, std::string &err);
// Appends one row and flushes; false (with the reason) when the write fails.
bool HistoryAppend(HistoryFile &h, const std::string &row, std::string &err);

} // namespace laghos
