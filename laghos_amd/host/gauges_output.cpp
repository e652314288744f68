// gauges_output.cpp — where the gauges are and the text of the `-gauges` file (gauges_output.hpp).
#include "gauges_output.hpp"

#include "../../include/laghos_hip.h"

namespace laghos
{

const char *const kGaugesHeader = "cycle t gauge x y z vx vy vz rho e p cs detj div_v";

std::string GaugesPath(const std::string &basename) { return basename + "_gauges.csv"; }

bool ResolveGauges(const Discretization &d, const std::vector<double> &points, std::vector<int> &zone, std::vector<double> &xi, int *bad)
{
   const int n = (int)(points.size() / 3);
   zone.assign(n, -1);
   xi.assign((size_t)n * d.dim, 0.0);
   // zone j is the structured zone elem_perm[j] of the rank's block
   std::vector<int> of_structured;
   if (!d.elem_perm.empty())
   {
      of_structured.assign(d.elem_perm.size(), -1);
      for (size_t j = 0; j < d.elem_perm.size(); j++) { of_structured[d.elem_perm[j]] = (int)j; }
   }
   for (int g = 0; g < n; g++)
   {
      int ijk[3];
      double x[3];
      if (!LocateInitial(d.mesh, &points[3 * (size_t)g], ijk, x))
      {
         if (bad) { *bad = g; }
         return false;
      }
      bool mine = true;
      int l = 0, stride = 1;
      for (int a = 0; a < d.dim; a++)
      {
         const int loc = ijk[a] - d.part.eoff[a];
         mine = mine && loc >= 0 && loc < d.part.ne[a];
         l += stride * loc;
         stride *= d.part.ne[a];
         xi[(size_t)g * d.dim + a] = x[a];
      }
      if (mine) { zone[g] = of_structured.empty() ? l : of_structured[l]; }
   }
   return true;
}

std::string GaugesText(long cycle, double t, int n, const double *rows)
{
   std::string s;
   for (int g = 0; g < n; g++)
   {
      AppendInt(s, cycle, true);
      AppendDouble(s, t);
      AppendInt(s, g);
      for (int k = 0; k < LGH_GAUGE_COLS; k++) { AppendDouble(s, rows[(size_t)g * LGH_GAUGE_COLS + k]); }
      s += "\n";
   }
   return s;
}

void GaugesFileInit(HistoryFile &h)
{
   h.header = kGaugesHeader;
   h.what = "gauges";
}

} // namespace laghos
