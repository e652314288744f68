// loads_output.cpp — the rows and the text of the `-loads` file (loads_output.hpp).
#include "loads_output.hpp"

#include <cmath>

#include "../../include/laghos_hip.h"
#include "driver_outputs.hpp"

namespace laghos
{

const char *const kLoadsHeader = "cycle t name n area fx fy fz pa p_mean power flux xn p_min p_max";

std::string LoadsPath(const std::string &basename) { return basename + "_loads.csv"; }

void LoadsRows(const Discretization &d, const std::vector<std::pair<int, int>> &planes, std::vector<std::string> &names, std::vector<int> &faces)
{
   names.assign(1, "surface");
   faces.clear();
   for (int f = 0; f < 2 * d.dim; f++) { names.push_back(std::string(1, (char)('x' + f / 2)) + (char)('0' + f % 2)); }
   auto list = [&](const std::vector<int> &zf, int row, bool by_face) {
      for (size_t k = 0; k + 1 < zf.size(); k += 2)
      {
         faces.push_back(zf[k]);
         faces.push_back(zf[k + 1]);
         faces.push_back(by_face ? 1 + zf[k + 1] : row); // (on the boundary local face 2a + s is side s of axis a of the box)
      }
   };
   const std::vector<int> surface = SelectFaces(d, -1, 0);
   list(surface, 0, false);
   list(surface, 0, true);
   for (const auto &pl : planes)
   {
      list(SelectFaces(d, pl.first, pl.second), (int)names.size(), false);
      names.push_back(std::string("plane_") + (char)('x' + pl.first) + std::to_string(pl.second));
   }
}

std::string LoadsText(long cycle, double t, const std::vector<std::string> &names, const double *rows)
{
   std::string s;
   for (size_t r = 0; r < names.size(); r++)
   {
      const double *d = rows + r * LGH_LOADS_COLS;
      AppendInt(s, cycle, true);
      AppendDouble(s, t);
      s += " " + names[r];
      AppendInt(s, (long long)d[0]);
      for (int k = 1; k <= 5; k++) { AppendDouble(s, d[k]); }  // area fx fy fz pa
      AppendDouble(s, d[0] != 0.0 ? d[5] / d[1] : NAN);       // p_mean
      for (int k = 6; k <= 10; k++) { AppendDouble(s, d[k]); } // power flux xn p_min p_max
      s += "\n";
   }
   return s;
}

void LoadsFileInit(HistoryFile &h)
{
   h.header = kLoadsHeader;
   h.what = "loads";
}

} // namespace laghos
