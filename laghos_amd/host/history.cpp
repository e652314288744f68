// history.cpp — the file logic of the `-hist` time history (history.hpp): header, row formatting, trimming on restart.
#include "history.hpp"

#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <sys/stat.h>

#include "../../include/laghos_hip.h"

namespace laghos
{

const char *const kHistoryHeader = "# cycle t dt rk_steps repeats mass volume ie ke total d_total px py pz detj_min detj_min_rank "
                                   "detj_min_zone rho_min rho_max e_min e_max p_max v_max n_inverted n_negative_e n_nonfinite";

std::string HistoryPath(const std::string &basename) { return basename + "_history.csv"; }

void AppendDouble(std::string &s, double v)
{
   char buf[40];
   if (std::isnan(v)) { std::snprintf(buf, sizeof(buf), " nan"); } // (one spelling, whatever the sign bit)
   else { std::snprintf(buf, sizeof(buf), " %.17g", v); }
   s += buf;
}
void AppendInt(std::string &s, long long v, bool first)
{
   char buf[32];
   std::snprintf(buf, sizeof(buf), first ? "%lld" : " %lld", v);
   s += buf;
}

std::string HistoryRow(long cycle, double t, double dt, long rk_steps, long repeats, const double *d, double energy_init)
{
   std::string s;
   AppendInt(s, cycle, true);
   AppendDouble(s, t);
   AppendDouble(s, dt);
   AppendInt(s, rk_steps);
   AppendInt(s, repeats);
   const double total = d[2] + d[3];
   for (int k = 0; k < 4; k++) { AppendDouble(s, d[k]); } // mass volume ie ke
   AppendDouble(s, total);
   AppendDouble(s, total - energy_init);
   for (int k = 4; k <= 7; k++) { AppendDouble(s, d[k]); } // px py pz detj_min
   AppendInt(s, (long long)d[18]);
   AppendInt(s, (long long)d[17]);
   for (int k = 8; k <= 13; k++) { AppendDouble(s, d[k]); } // rho_min rho_max e_min e_max p_max v_max
   for (int k = 14; k <= 16; k++) { AppendInt(s, (long long)d[k]); }
   s += "\n";
   return s;
}

void HistoryFile::Close()
{
   if (f) { std::fclose(f); }
   f = nullptr;
}

static void MakeDirs(const std::string &path)
{
   const size_t slash = path.find_last_of('/');
   if (slash == std::string::npos) { return; }
   const std::string dir = path.substr(0, slash);
   for (size_t p = 1; p <= dir.size(); p++)
   {
      if (p == dir.size() || dir[p] == '/') { (void)::mkdir(dir.substr(0, p).c_str(), 0777); }
   }
}

static bool Fail(HistoryFile &h, std::string &err, const std::string &what)
{
   err = std::string(h.what) + " " + h.path + ": " + what + (errno ? std::string(": ") + std::strerror(errno) : std::string());
   h.Close();
   return false;
}

// the whole content replaces the file (written beside it and renamed: a run killed here leaves the old file); left open for appending
static bool Rewrite(HistoryFile &h, const std::string &content, std::string &err)
{
   const std::string tmp = h.path + ".tmp";
   errno = 0;
   std::FILE *out = std::fopen(tmp.c_str(), "wb");
   if (!out) { return Fail(h, err, "cannot open for writing"); }
   const bool written = std::fwrite(content.data(), 1, content.size(), out) == content.size() && std::fflush(out) == 0;
   if (std::fclose(out) != 0 || !written) { (void)std::remove(tmp.c_str()); return Fail(h, err, "write failed"); }
   if (std::rename(tmp.c_str(), h.path.c_str()) != 0) { (void)std::remove(tmp.c_str()); return Fail(h, err, "cannot replace the file"); }
   h.f = std::fopen(h.path.c_str(), "ab");
   if (!h.f) { return Fail(h, err, "cannot open for appending"); }
   return true;
}

bool HistoryStart(HistoryFile &h, const std::string &path, std::string &err)
{
   h.Close();
   h.path = path;
   h.rows = 0;
   MakeDirs(path);
   return Rewrite(h, std::string(h.header) + "\n", err);
}

bool HistoryResume(HistoryFile &h, const std::string &path, long keep_upto, std::string &err)
{
   h.Close();
   h.path = path;
   h.rows = 0;
   errno = 0;
   std::FILE *in = std::fopen(path.c_str(), "rb");
   if (!in) { return HistoryStart(h, path, err); }
   std::string all;
   char buf[4096];
   size_t n;
   while ((n = std::fread(buf, 1, sizeof(buf), in)) > 0) { all.append(buf, n); }
   const bool read_error = std::ferror(in) != 0;
   std::fclose(in);
   if (read_error) { return Fail(h, err, "cannot read"); }
   // complete lines only: what follows the last newline is a row a killed run did not finish
   std::string keep;
   size_t pos = 0;
   bool first = true;
   while (true)
   {
      const size_t nl = all.find('\n', pos);
      if (nl == std::string::npos) { break; }
      const std::string line = all.substr(pos, nl - pos);
      pos = nl + 1;
      if (first)
      {
         first = false;
         if (line != h.header) { errno = 0; return Fail(h, err, std::string("its first line is not the header of a ") + h.what + " file: not touched"); }
         keep += line + "\n";
         continue;
      }
      char *end = nullptr;
      const long long cycle = std::strtoll(line.c_str(), &end, 10);
      if (end == line.c_str() || (*end != ' ' && *end != '\0')) { errno = 0; return Fail(h, err, "a row does not start with a cycle number: not touched"); }
      if (cycle > keep_upto) { continue; }
      keep += line + "\n";
      h.rows++;
   }
   if (first) { return HistoryStart(h, path, err); } // (not even a complete header)
   return Rewrite(h, keep, err);
}

bool HistoryAppend(HistoryFile &h, const std::string &row, std::string &err)
{
   errno = 0;
   if (!h.f) { return Fail(h, err, "not open"); }
   if (std::fwrite(row.data(), 1, row.size(), h.f) != row.size() || std::fflush(h.f) != 0) { return Fail(h, err, "write failed"); }
   h.rows++;
   return true;
}

} // namespace laghos
