// gauges_output.hpp — the `-gauges` file: <basename>_gauges.csv, the time series at the gauges (lgh_gauges_*) - material points
// given by their position in the initial mesh - per recorded cycle.  DESIGN.md §7l.
//
// A text file: the header line below, then one line per (cycle, gauge), cells separated by one blank in the header's order; the
// gauges of a cycle follow each other in the order of the command line, then of the -gauge-file.  cycle and gauge are printed as
// integers, doubles with %.17g (inf, -inf, nan as they come): equal bits give equal bytes.  The lines are written when the device
// buffer is drained - when it is full, before every checkpoint piece, at the end of the run - and flushed; the file logic - start,
// resume on a restart, append - is that of history.hpp.  No GPU, no context; the driver supplies the figures.
#pragma once
#include <string>
#include <vector>

#include "fem.hpp"
#include "history.hpp"

namespace laghos
{

extern const char *const kGaugesHeader; // the first line, without its newline

std::string GaugesPath(const std::string &basename); // <basename>_gauges.csv

// Where the gauges of a run are, for this rank: points holds 3 doubles per gauge (the position in the initial mesh; entries of
// axes >= dim ignored).  zone[g] = this rank's zone id of the zone LocateInitial names - through elem_perm under -renumber - or -1
// where the partition gives that zone to another rank; xi[g*dim + a] the reference coordinates (the same on every rank).  false,
// with the number of the gauge in *bad, when a point lies outside the mesh.
bool ResolveGauges(const Discretization &d, const std::vector<double> &points, std::vector<int> &zone, std::vector<double> &xi, int *bad);

// The lines of one sample, each with its newline.  rows: n x LGH_GAUGE_COLS doubles of lgh_gauges_drain.
std::string GaugesText(long cycle, double t, int n, const double *rows);

// A HistoryFile that writes and expects the header of this file
void GaugesFileInit(HistoryFile &h);

} // namespace laghos
