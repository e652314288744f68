// loads_output.hpp — the `-loads` file: <basename>_loads.csv, the pressure loads (lgh_loads) on the boundary of the global mesh,
// on each of its walls and on the logical planes of `-loads-plane`, per recorded cycle.  DESIGN.md §7i.
//
// A text file: the header line below, then one line per (cycle, row), cells separated by one blank in the header's order; the rows
// of a cycle follow each other in the order of LoadsRows.  cycle and n are printed as integers, doubles with %.17g (inf, -inf,
// nan for the non-finite ones): equal bits give equal bytes.  p_mean = pa / area, nan for a row without points.  The lines of a
// cycle are written at once and flushed; the file logic - start, resume on a restart, append - is that of history.hpp.
// No GPU, no context; the driver supplies the figures.
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "fem.hpp"
#include "history.hpp"

namespace laghos
{

extern const char *const kLoadsHeader; // the first line, without its newline

std::string LoadsPath(const std::string &basename); // <basename>_loads.csv

// The rows of the driver for this rank's zones: `surface` (every face on the boundary of the global mesh), the walls x0 x1 y0 y1
// [z0 z1] (the same faces split by axis and side: a wall face is listed twice), plane_<axis><K> per (axis, K) of `planes` in their
// order (SelectFaces: the side-0 faces of zone layer K, for K = n the side-1 faces of the last layer - the normal is the outward
// normal of the zone a face belongs to).  names: one per row; faces: 3 ints per listed face - zone, local face, row.
void LoadsRows(const Discretization &d, const std::vector<std::pair<int, int>> &planes, std::vector<std::string> &names, std::vector<int> &faces);

// The lines of one cycle, each with its newline.  rows: names.size() x LGH_LOADS_COLS doubles of lgh_loads.
std::string LoadsText(long cycle, double t, const std::vector<std::string> &names, const double *rows);

// A HistoryFile that writes and expects the header of this file
void LoadsFileInit(HistoryFile &h);

} // namespace laghos
