// map_output.cpp — the file logic of the `-map` files (map_output.hpp): name, layout, writing.
#include "map_output.hpp"

#include "../../include/laghos_hip.h"
#include "vtk_output.hpp"

#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <sstream>
#include <vector>

namespace laghos
{

std::string MapDir(const std::string &basename) { return basename + "_map"; }

std::string MapName(int cycle)
{
   char buf[32];
   std::snprintf(buf, sizeof(buf), "cycle_%06d.vti", cycle);
   return buf;
}

bool WriteVti(const std::string &dir, int dim, const int n[3], const double lo[3], const double hi[3], const double *rows,
              long n_excluded, int cycle, double time, std::string &err)
{
   const std::string path = dir + "/" + MapName(cycle);
   if (dim < 1 || dim > 3 || !n || !lo || !hi || !rows) { err = "map " + path + ": bad arguments"; return false; }
   size_t NC = 1;
   for (int c = 0; c < 3; c++)
   {
      if (n[c] < 1 || (c >= dim && n[c] != 1)) { err = "map " + path + ": bad arguments"; return false; }
      NC *= (size_t)n[c];
   }
   const int C = LGH_MAP_COLS;
   const double *cell = rows + C; // row 0 is "outside"
   // the columns as arrays of their own
   std::vector<double> col[C], mom(3 * NC), rho(NC), sie(NC), vel(3 * NC), prs(NC);
   for (int k = 0; k < C; k++) { col[k].resize(NC); }
   for (size_t i = 0; i < NC; i++)
   {
      const double *r = cell + i * C;
      for (int k = 0; k < C; k++) { col[k][i] = r[k]; }
      const double vol = r[1], mass = r[2];
      rho[i] = (vol != 0.0) ? mass / vol : NAN;
      sie[i] = (mass != 0.0) ? r[3] / mass : NAN;
      prs[i] = (vol != 0.0) ? r[8] / vol : NAN;
      for (int c = 0; c < 3; c++)
      {
         mom[3 * i + c] = r[5 + c];
         vel[3 * i + c] = (c >= dim) ? 0.0 : ((mass != 0.0) ? r[5 + c] / mass : NAN);
      }
   }
   const int32_t cyc = cycle;
   const int64_t nex = n_excluded;
   Appended ap;
   std::ostringstream h;
   h << std::setprecision(17);
   h << "<?xml version=\"1.0\"?>\n<VTKFile type=\"ImageData\" version=\"1.0\" byte_order=\"LittleEndian\" header_type=\"UInt64\">\n";
   std::ostringstream ext;
   for (int c = 0; c < 3; c++) { ext << (c ? " " : "") << "0 " << (c < dim ? n[c] : 0); }
   h << "<ImageData WholeExtent=\"" << ext.str() << "\" Origin=\"";
   for (int c = 0; c < 3; c++) { h << (c ? " " : "") << (c < dim ? lo[c] : 0.0); }
   h << "\" Spacing=\"";
   for (int c = 0; c < 3; c++) { h << (c ? " " : "") << (c < dim ? (hi[c] - lo[c]) / n[c] : 1.0); }
   h << "\">\n<FieldData>\n";
   h << ap.Array("Float64", "TIME", 0, &time, sizeof(double), " NumberOfTuples=\"1\"");
   h << ap.Array("Int32", "CYCLE", 0, &cyc, sizeof(int32_t), " NumberOfTuples=\"1\"");
   h << ap.Array("Int64", "N_EXCLUDED", 0, &nex, sizeof(int64_t), " NumberOfTuples=\"1\"");
   h << ap.Array("Float64", "OUTSIDE", 0, rows, C * sizeof(double), " NumberOfTuples=\"11\"");
   h << "</FieldData>\n<Piece Extent=\"" << ext.str() << "\">\n<CellData Scalars=\"density\" Vectors=\"velocity\">\n";
   static const char *names[C] = {"n", "vol", "mass", "ie", "ke", nullptr, nullptr, nullptr, "pv", "rho_min", "rho_max"};
   const uint64_t nb = NC * sizeof(double);
   for (int k = 0; k < C; k++)
   {
      if (k == 5) { h << ap.Array("Float64", "momentum", 3, mom.data(), 3 * nb); }
      if (names[k]) { h << ap.Array("Float64", names[k], 1, col[k].data(), nb); }
   }
   h << ap.Array("Float64", "density", 1, rho.data(), nb);
   h << ap.Array("Float64", "specific_internal_energy", 1, sie.data(), nb);
   h << ap.Array("Float64", "velocity", 3, vel.data(), 3 * nb);
   h << ap.Array("Float64", "pressure", 1, prs.data(), nb);
   h << "</CellData>\n</Piece>\n</ImageData>\n";
   MakeDirs(dir);
   errno = 0;
   std::ofstream f(path.c_str(), std::ios::binary);
   bool ok = (bool)f;
   if (ok)
   {
      f << h.str();
      ap.Write(f);
      f << "</VTKFile>\n";
      f.close();
      ok = !f.fail();
   }
   if (!ok) { err = "map " + path + ": cannot write" + (errno ? std::string(": ") + std::strerror(errno) : std::string()); }
   return ok;
}

} // namespace laghos
