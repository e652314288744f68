// profile.hpp — the `-prof` files: <basename>_profile_<cycle, 6 digits>.csv, one file per recorded cycle with the binned
// 1-D profile of the flow (lgh_profile): the exact bin sums and the curves derived from them.
//
// A text file in the style of the `-hist` file (history.hpp): line 1 holds "# cycle t axis origin_x origin_y origin_z lo hi
// nbins n_excluded" and their values, line 2 the column names, then one line per row of the table - row 0 (below lo), the
// nbins bins, row nbins + 1 (at or above hi); the open edges print -inf / inf.  Integers (cycle, nbins, n_excluded, row, n)
// are printed as integers, doubles with %.17g (inf, -inf, nan for the non-finite ones): equal bits give equal bytes.  The
// derived columns rho = mass / vol, e = ie / mass, v = mom / mass, p = pv / vol, xi = mxi / mass are nan where the divisor
// is 0.  With `exact` (3 values per row: the exact Sedov solution at the row's xi) the columns rho_exact v_exact p_exact follow.
// File logic only - no GPU, no context; the driver (laghos.cpp) supplies the figures.
#pragma once
#include <string>

namespace laghos
{

std::string ProfilePath(const std::string &basename, int cycle); // <basename>_profile_<cycle, 6 digits>.csv

// The whole file.  axis: 'x', 'y', 'z' or 'r'; rows: (nbins + 2) x LGH_PROFILE_COLS doubles of lgh_profile; exact: nullptr, or
// (nbins + 2) x 3 doubles.
std::string ProfileText(long cycle, double t, char axis, const double origin[3], double lo, double hi, int nbins, long n_excluded,
                        const double *rows, const double *exact);

// Writes the file (the directory chain of the path is created; an existing file is replaced); false with the reason otherwise.
bool ProfileWrite(const std::string &path, const std::string &text, std::string &err);

} // namespace laghos
