// map_output.hpp — the `-map` files: <basename>_map/cycle_<6 digits>.vti, one VTK XML ImageData file per recorded cycle with
// the flow binned onto a fixed Cartesian grid (lgh_map): the exact cell sums and the fields derived from them.  File logic
// only, no GPU code.  There is no collection file: viewers group numbered .vti files themselves, and a restarted run then
// has nothing to merge.  DESIGN.md §7g.
#pragma once
#include <string>

namespace laghos
{

std::string MapDir(const std::string &basename); // <basename>_map
std::string MapName(int cycle);                  // cycle_<6 digits>.vti

// <dir>/MapName(cycle).  n, lo, hi: cells and box per axis (n = 1 and ignored bounds above dim); rows: the
// (n[0] n[1] n[2] + 1) x LGH_MAP_COLS doubles of lgh_map.  WholeExtent "0 nx 0 ny 0 nz" (0 for an unused axis), Origin lo and
// Spacing (hi - lo) / n (0 and 1 above dim).  CellData, Float64, x fastest as the rows are: n, vol, mass, ie, ke, momentum (3),
// pv, rho_min, rho_max, then the derived density = mass / vol, specific_internal_energy = ie / mass, velocity = momentum /
// mass (3; 0 above dim) and pressure = pv / vol, NaN where the divisor is 0.  FieldData TIME, CYCLE, N_EXCLUDED, OUTSIDE (the
// 11 values of row 0).  Little endian, UInt64 headers, every array in one raw appended block, as the .vtu writer does.  Equal
// bits give equal bytes.  false with err set when the file cannot be written.
bool WriteVti(const std::string &dir, int dim, const int n[3], const double lo[3], const double hi[3], const double *rows,
              long n_excluded, int cycle, double time, std::string &err);

} // namespace laghos
