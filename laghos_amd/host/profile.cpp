// profile.cpp — the file logic of the `-prof` profiles (profile.hpp): name, formatting, writing.
#include "profile.hpp"

#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <sys/stat.h>

#include "../../include/laghos_hip.h"

namespace laghos
{

std::string ProfilePath(const std::string &basename, int cycle)
{
   char buf[32];
   std::snprintf(buf, sizeof(buf), "_profile_%06d.csv", cycle);
   return basename + buf;
}

static void AddDouble(std::string &s, double v)
{
   char buf[40];
   if (std::isnan(v)) { std::snprintf(buf, sizeof(buf), " nan"); } // (one spelling, whatever the sign bit)
   else { std::snprintf(buf, sizeof(buf), " %.17g", v); }
   s += buf;
}
static void AddInt(std::string &s, long long v, bool first = false)
{
   char buf[32];
   std::snprintf(buf, sizeof(buf), first ? "%lld" : " %lld", v);
   s += buf;
}
static double Ratio(double a, double b) { return (b != 0.0) ? a / b : NAN; }

std::string ProfileText(long cycle, double t, char axis, const double origin[3], double lo, double hi, int nbins, long n_excluded,
                        const double *rows, const double *exact)
{
   std::string s = "# cycle t axis origin_x origin_y origin_z lo hi nbins n_excluded";
   AddInt(s, cycle);
   AddDouble(s, t);
   s += ' ';
   s += axis;
   for (int k = 0; k < 3; k++) { AddDouble(s, origin[k]); }
   AddDouble(s, lo);
   AddDouble(s, hi);
   AddInt(s, nbins);
   AddInt(s, n_excluded);
   s += "\nrow lo hi n vol mass ie ke mom pv mxi rho_min rho_max rho e v p xi";
   if (exact) { s += " rho_exact v_exact p_exact"; }
   s += "\n";
   for (int r = 0; r < nbins + 2; r++)
   {
      const double *d = rows + (size_t)r * LGH_PROFILE_COLS;
      // (the edges as Context.profile forms them: lo + (hi - lo) b / nbins)
      const double e0 = (r == 0) ? -INFINITY : lo + (hi - lo) * (double)(r - 1) / (double)nbins;
      const double e1 = (r == nbins + 1) ? INFINITY : lo + (hi - lo) * (double)r / (double)nbins;
      AddInt(s, r, true);
      AddDouble(s, e0);
      AddDouble(s, e1);
      AddInt(s, (long long)d[0]);
      for (int k = 1; k < LGH_PROFILE_COLS; k++) { AddDouble(s, d[k]); }
      AddDouble(s, Ratio(d[2], d[1]));
      AddDouble(s, Ratio(d[3], d[2]));
      AddDouble(s, Ratio(d[5], d[2]));
      AddDouble(s, Ratio(d[6], d[1]));
      AddDouble(s, Ratio(d[7], d[2]));
      if (exact) { for (int k = 0; k < 3; k++) { AddDouble(s, exact[3 * r + k]); } }
      s += "\n";
   }
   return s;
}

bool ProfileWrite(const std::string &path, const std::string &text, std::string &err)
{
   const size_t slash = path.find_last_of('/');
   if (slash != std::string::npos)
   {
      const std::string dir = path.substr(0, slash);
      for (size_t p = 1; p <= dir.size(); p++)
      {
         if (p == dir.size() || dir[p] == '/') { (void)::mkdir(dir.substr(0, p).c_str(), 0777); }
      }
   }
   errno = 0;
   std::FILE *f = std::fopen(path.c_str(), "w");
   bool ok = f != nullptr;
   if (ok) { ok = std::fwrite(text.data(), 1, text.size(), f) == text.size(); }
   if (f) { ok = (std::fclose(f) == 0) && ok; }
   if (!ok) { err = "profile " + path + ": cannot write" + (errno ? std::string(": ") + std::strerror(errno) : std::string()); }
   return ok;
}

} // namespace laghos
