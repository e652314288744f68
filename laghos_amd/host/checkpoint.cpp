// checkpoint.cpp — see checkpoint.hpp.  Host only: no HIP, no MFEM.
#include "checkpoint.hpp"

#include <algorithm>
#include <cerrno>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <sys/stat.h>
#include <unistd.h>

#include "../../include/lgh_fingerprint.h"

namespace laghos
{

namespace
{

constexpr long kHeaderAlign = 4096;
constexpr long kMaxHeader = 1L << 20;

void MakeDirChain(const std::string &dir)
{
   for (size_t p = 1; p <= dir.size(); p++)
   {
      if (p == dir.size() || dir[p] == '/') { (void)::mkdir(dir.substr(0, p).c_str(), 0777); }
   }
}

unsigned long long Bits(double v)
{
   unsigned long long b;
   std::memcpy(&b, &v, sizeof(b));
   return b;
}
double FromBits(unsigned long long b)
{
   double v;
   std::memcpy(&v, &b, sizeof(v));
   return v;
}

std::string Hex(unsigned long long w)
{
   char buf[17];
   std::snprintf(buf, sizeof(buf), "%016llX", w);
   return buf;
}

std::string HeaderText(const CheckpointHeader &h)
{
   std::ostringstream os;
   auto dbl = [&](const char *key, double v) {
      char dec[40];
      std::snprintf(dec, sizeof(dec), "%.17g", v);
      os << key << " " << Hex(Bits(v)) << " # " << dec << "\n";
   };
   os << "LGHCKPT 1\n";
   os << "header_bytes " << h.header_bytes << "\n";
   os << "state_words " << h.state_words << "\n";
   os << "dim " << h.dim << "\nproblem " << h.problem << "\norder_v " << h.order_v << "\norder_e " << h.order_e << "\nQ1D " << h.Q1D << "\n";
   os << "NE " << h.NE << "\nglobal_NE " << h.global_NE << "\nN " << h.N << "\n";
   os << "nranks " << h.nranks << "\nrank " << h.rank << "\npgrid " << h.pgrid[0] << " " << h.pgrid[1] << " " << h.pgrid[2] << "\n";
   os << "ode_solver " << h.ode_solver << "\n";
   dbl("cfl", h.cfl);
   dbl("cg_tol", h.cg_tol);
   os << "cg_max_iter " << h.cg_max_iter << "\n";
   dbl("t", h.t);
   dbl("dt", h.dt);
   os << "ti " << h.ti << "\nsteps " << h.steps << "\nrepeats " << h.repeats << "\n";
   dbl("energy_init", h.energy_init);
   os << "checks " << h.checks << "\nchecks_ok " << h.checks_ok << "\n";
   os << "paraview_dumps " << h.pv_dumps << "\n";
   os << "setup_fp " << Hex(h.setup_fp[0]) << " " << Hex(h.setup_fp[1]) << "\n";
   os << "state_fp " << Hex(h.state_fp[0]) << " " << Hex(h.state_fp[1]) << "\n";
   os << "end\n";
   return os.str();
}

// strict readers: the whole token must be a number
bool ParseLong(const std::string &s, long &v)
{
   if (s.empty()) { return false; }
   char *end = nullptr;
   errno = 0;
   v = std::strtol(s.c_str(), &end, 10);
   return errno == 0 && end && *end == '\0';
}
bool ParseHex(const std::string &s, unsigned long long &v)
{
   if (s.size() != 16) { return false; }
   for (char ch : s)
   {
      if (!((ch >= '0' && ch <= '9') || (ch >= 'A' && ch <= 'F'))) { return false; }
   }
   v = std::strtoull(s.c_str(), nullptr, 16);
   return true;
}

std::vector<std::string> Tokens(const std::string &line)
{
   std::vector<std::string> out;
   std::istringstream is(line);
   std::string tok;
   while (is >> tok)
   {
      if (tok[0] == '#') { break; }
      out.push_back(tok);
   }
   return out;
}

int Fail(int code, const std::string &path, const std::string &what, std::string &err)
{
   err = "checkpoint " + path + ": " + what;
   return code;
}

} // namespace

std::string CheckpointDir(const std::string &basename) { return basename + "_restart"; }
std::string CheckpointName(int ti)
{
   char buf[32];
   std::snprintf(buf, sizeof(buf), "cycle_%06d.lgr", ti);
   return buf;
}
std::string CheckpointPiece(const std::string &stem, int nranks, int rank)
{
   return nranks > 1 ? stem + "." + std::to_string(rank) : stem;
}

void FingerprintWords(const void *words, long n, unsigned long long offset, unsigned long long fp[2])
{
   lgh_fp_accumulate((const unsigned long long *)words, n, offset, fp);
}

void SetupFingerprint(const std::vector<double> &S0, const std::vector<double> &rho0_l2, const std::vector<double> &gamma,
                      const std::vector<double> &rho0_q, const std::vector<int> &h1map, unsigned long long fp[2])
{
   fp[0] = fp[1] = 0ULL;
   unsigned long long off = 0;
   for (const std::vector<double> *v : {&S0, &rho0_l2, &gamma, &rho0_q})
   {
      FingerprintWords(v->data(), (long)v->size(), off, fp);
      off += v->size();
   }
   unsigned long long buf[1024];
   for (size_t i = 0; i < h1map.size(); i += 1024)
   {
      const size_t m = std::min<size_t>(1024, h1map.size() - i);
      for (size_t k = 0; k < m; k++) { buf[k] = (unsigned long long)(long long)h1map[i + k]; }
      FingerprintWords(buf, (long)m, off + i, fp);
   }
}

int WriteCheckpoint(const std::string &path, CheckpointHeader h, const double *S, long nS, const double *pv_times,
                    const long long *pv_cycles, long npv, std::string &err)
{
   if (nS < 0 || npv < 0 || (nS > 0 && !S) || (npv > 0 && (!pv_times || !pv_cycles)))
   {
      return Fail(CKPT_ERR_IO, path, "write: bad arguments", err);
   }
   h.state_words = nS;
   h.pv_dumps = npv;
   h.state_fp[0] = h.state_fp[1] = 0ULL;
   FingerprintWords(S, nS, 0, h.state_fp);
   // header_bytes is part of the text: size the text with a value of the final width, then pad
   h.header_bytes = kHeaderAlign;
   for (int pass = 0; pass < 3; pass++)
   {
      const long need = (long)HeaderText(h).size();
      const long padded = (need + kHeaderAlign - 1) / kHeaderAlign * kHeaderAlign;
      if (padded == h.header_bytes) { break; }
      h.header_bytes = padded;
   }
   std::string head = HeaderText(h);
   if ((long)head.size() > h.header_bytes) { return Fail(CKPT_ERR_IO, path, "write: the header does not fit its padding", err); }
   head.resize((size_t)h.header_bytes, '\n');

   unsigned long long trailer[2] = {0ULL, 0ULL};
   unsigned long long off = 0;
   {
      // (the header is copied: a std::string's bytes need not be 8-byte aligned)
      std::vector<unsigned long long> hw((size_t)h.header_bytes / 8);
      std::memcpy(hw.data(), head.data(), (size_t)h.header_bytes);
      FingerprintWords(hw.data(), (long)hw.size(), off, trailer);
      off += hw.size();
   }
   FingerprintWords(S, nS, off, trailer);
   off += (unsigned long long)nS;
   FingerprintWords(pv_times, npv, off, trailer);
   off += (unsigned long long)npv;
   FingerprintWords(pv_cycles, npv, off, trailer);

   const size_t slash = path.find_last_of('/');
   if (slash != std::string::npos) { MakeDirChain(path.substr(0, slash)); }
   const std::string tmp = path + ".tmp";
   std::FILE *f = std::fopen(tmp.c_str(), "wb");
   if (!f) { return Fail(CKPT_ERR_IO, path, std::string("write: cannot open ") + tmp + " (" + std::strerror(errno) + ")", err); }
   bool ok = std::fwrite(head.data(), 1, head.size(), f) == head.size();
   ok = ok && (nS == 0 || std::fwrite(S, sizeof(double), (size_t)nS, f) == (size_t)nS);
   ok = ok && (npv == 0 || std::fwrite(pv_times, sizeof(double), (size_t)npv, f) == (size_t)npv);
   ok = ok && (npv == 0 || std::fwrite(pv_cycles, sizeof(long long), (size_t)npv, f) == (size_t)npv);
   ok = ok && std::fwrite(trailer, sizeof(unsigned long long), 2, f) == 2;
   ok = ok && std::fflush(f) == 0 && ::fsync(::fileno(f)) == 0;
   ok = (std::fclose(f) == 0) && ok;
   if (!ok)
   {
      (void)std::remove(tmp.c_str());
      return Fail(CKPT_ERR_IO, path, "write: cannot write " + tmp, err);
   }
   if (std::rename(tmp.c_str(), path.c_str()) != 0)
   {
      (void)std::remove(tmp.c_str());
      return Fail(CKPT_ERR_IO, path, std::string("write: cannot rename ") + tmp + " (" + std::strerror(errno) + ")", err);
   }
   err.clear();
   return CKPT_OK;
}

int ReadCheckpoint(const std::string &path, Checkpoint &out, std::string &err)
{
   std::FILE *f = std::fopen(path.c_str(), "rb");
   if (!f) { return Fail(CKPT_ERR_IO, path, std::string("cannot open the file (") + std::strerror(errno) + ")", err); }
   struct Closer
   {
      std::FILE *f;
      ~Closer() { std::fclose(f); }
   } closer{f};
   struct stat st;
   if (::fstat(::fileno(f), &st) != 0) { return Fail(CKPT_ERR_IO, path, "cannot stat the file", err); }
   const long file_bytes = (long)st.st_size;

   // 1. magic and version: the first line
   std::string head((size_t)std::min<long>(file_bytes, kHeaderAlign), '\0');
   if (!head.empty() && std::fread(&head[0], 1, head.size(), f) != head.size()) { return Fail(CKPT_ERR_IO, path, "cannot read the file", err); }
   {
      const size_t nl = head.find('\n');
      const std::vector<std::string> tk = Tokens(head.substr(0, nl == std::string::npos ? head.size() : nl));
      long version = 0;
      if (nl == std::string::npos || tk.size() != 2 || tk[0] != "LGHCKPT" || !ParseLong(tk[1], version))
      {
         return Fail(CKPT_ERR_MAGIC, path, "magic: the first line is not \"LGHCKPT <version>\" - not a checkpoint of this driver", err);
      }
      if (version != 1)
      {
         return Fail(CKPT_ERR_VERSION, path, "version: format version " + std::to_string(version) + ", this driver reads version 1", err);
      }
   }
   // 2. header_bytes: the second line; the header must lie inside the file
   long header_bytes = 0;
   {
      const size_t l1 = head.find('\n') + 1, l2 = head.find('\n', l1);
      const std::vector<std::string> tk = Tokens(l2 == std::string::npos ? std::string() : head.substr(l1, l2 - l1));
      if (tk.size() != 2 || tk[0] != "header_bytes" || !ParseLong(tk[1], header_bytes) || header_bytes < kHeaderAlign ||
          header_bytes % kHeaderAlign != 0 || header_bytes > kMaxHeader)
      {
         return Fail(CKPT_ERR_HEADER, path, "header_bytes: the second line is not \"header_bytes <multiple of 4096>\"", err);
      }
      if (header_bytes > file_bytes)
      {
         return Fail(CKPT_ERR_HEADER, path,
                     "header_bytes: the header is " + std::to_string(header_bytes) + " bytes, the file only " + std::to_string(file_bytes) +
                        " (cut inside the header)",
                     err);
      }
   }
   if (header_bytes > (long)head.size())
   {
      const size_t have = head.size();
      head.resize((size_t)header_bytes);
      if (std::fread(&head[have], 1, head.size() - have, f) != head.size() - have) { return Fail(CKPT_ERR_IO, path, "cannot read the header", err); }
   }
   // the key / value lines up to "end"
   std::map<std::string, std::vector<std::string>> kv;
   bool ended = false;
   {
      std::istringstream is(head);
      std::string line;
      std::getline(is, line); // magic
      while (std::getline(is, line))
      {
         const std::vector<std::string> tk = Tokens(line);
         if (tk.empty()) { continue; }
         if (tk[0] == "end") { ended = true; break; }
         kv[tk[0]] = std::vector<std::string>(tk.begin() + 1, tk.end());
      }
   }
   if (!ended) { return Fail(CKPT_ERR_HEADER, path, "header: no \"end\" line inside header_bytes", err); }
   Checkpoint c;
   CheckpointHeader &h = c.h;
   h.header_bytes = header_bytes;
   std::string bad;
   auto geti = [&](const char *key, size_t idx, size_t count, long &v) {
      auto it = kv.find(key);
      if (it == kv.end() || it->second.size() != count || !ParseLong(it->second[idx], v)) { if (bad.empty()) { bad = key; } }
   };
   auto getint = [&](const char *key, int &v) { long l = 0; geti(key, 0, 1, l); v = (int)l; };
   auto getdbl = [&](const char *key, double &v) {
      auto it = kv.find(key);
      unsigned long long b = 0;
      if (it == kv.end() || it->second.size() != 1 || !ParseHex(it->second[0], b)) { if (bad.empty()) { bad = key; } }
      v = FromBits(b);
   };
   auto getfp = [&](const char *key, unsigned long long fp[2]) {
      auto it = kv.find(key);
      if (it == kv.end() || it->second.size() != 2 || !ParseHex(it->second[0], fp[0]) || !ParseHex(it->second[1], fp[1])) { if (bad.empty()) { bad = key; } }
   };
   geti("state_words", 0, 1, h.state_words);
   geti("paraview_dumps", 0, 1, h.pv_dumps);
   getint("dim", h.dim); getint("problem", h.problem); getint("order_v", h.order_v); getint("order_e", h.order_e); getint("Q1D", h.Q1D);
   geti("NE", 0, 1, h.NE); geti("global_NE", 0, 1, h.global_NE); geti("N", 0, 1, h.N);
   getint("nranks", h.nranks); getint("rank", h.rank);
   for (int a = 0; a < 3; a++) { long l = 1; geti("pgrid", (size_t)a, 3, l); h.pgrid[a] = (int)l; }
   getint("ode_solver", h.ode_solver); getint("cg_max_iter", h.cg_max_iter);
   getdbl("cfl", h.cfl); getdbl("cg_tol", h.cg_tol); getdbl("t", h.t); getdbl("dt", h.dt); getdbl("energy_init", h.energy_init);
   getint("ti", h.ti); getint("steps", h.steps); getint("repeats", h.repeats); getint("checks", h.checks); getint("checks_ok", h.checks_ok);
   getfp("setup_fp", h.setup_fp);
   getfp("state_fp", h.state_fp);
   // 3. the file size against state_words (and the dump count).  An unreadable count is reported here, any other key after the trailer:
   // a damaged header is a trailer failure first.
   if (bad == "state_words" || bad == "paraview_dumps" || h.state_words < 0 || h.pv_dumps < 0 || h.state_words > (1L << 50) || h.pv_dumps > (1L << 40))
   {
      return Fail(CKPT_ERR_HEADER, path, "header: state_words / paraview_dumps missing or unreadable", err);
   }
   const long expect = header_bytes + 8 * (h.state_words + 2 * h.pv_dumps) + 16;
   if (file_bytes < expect)
   {
      return Fail(CKPT_ERR_TRUNCATED, path,
                  "truncated: state_words " + std::to_string(h.state_words) + " and " + std::to_string(h.pv_dumps) + " dumps need " +
                     std::to_string(expect) + " bytes, the file has " + std::to_string(file_bytes),
                  err);
   }
   if (file_bytes != expect)
   {
      return Fail(CKPT_ERR_SIZE, path,
                  "size: state_words " + std::to_string(h.state_words) + " and " + std::to_string(h.pv_dumps) + " dumps make " +
                     std::to_string(expect) + " bytes, the file has " + std::to_string(file_bytes),
                  err);
   }
   c.S.resize((size_t)h.state_words);
   c.pv_times.resize((size_t)h.pv_dumps);
   c.pv_cycles.resize((size_t)h.pv_dumps);
   unsigned long long trailer[2] = {0ULL, 0ULL};
   bool ok = h.state_words == 0 || std::fread(c.S.data(), 8, c.S.size(), f) == c.S.size();
   ok = ok && (h.pv_dumps == 0 || std::fread(c.pv_times.data(), 8, c.pv_times.size(), f) == c.pv_times.size());
   ok = ok && (h.pv_dumps == 0 || std::fread(c.pv_cycles.data(), 8, c.pv_cycles.size(), f) == c.pv_cycles.size());
   ok = ok && std::fread(trailer, 8, 2, f) == 2;
   if (!ok) { return Fail(CKPT_ERR_IO, path, "cannot read the payload", err); }
   // 4. the trailer
   unsigned long long fp[2] = {0ULL, 0ULL}, sfp[2] = {0ULL, 0ULL};
   {
      std::vector<unsigned long long> hw((size_t)header_bytes / 8);
      std::memcpy(hw.data(), head.data(), (size_t)header_bytes);
      unsigned long long off = 0;
      FingerprintWords(hw.data(), (long)hw.size(), off, fp);
      off += hw.size();
      FingerprintWords(c.S.data(), h.state_words, off, fp);
      off += (unsigned long long)h.state_words;
      FingerprintWords(c.pv_times.data(), h.pv_dumps, off, fp);
      off += (unsigned long long)h.pv_dumps;
      FingerprintWords(c.pv_cycles.data(), h.pv_dumps, off, fp);
   }
   FingerprintWords(c.S.data(), h.state_words, 0, sfp);
   const bool state_ok = sfp[0] == h.state_fp[0] && sfp[1] == h.state_fp[1];
   if (fp[0] != trailer[0] || fp[1] != trailer[1])
   {
      const char *where = !bad.empty() ? " (the header is damaged: key " :
                          state_ok     ? " (the state still matches state_fp: the damage is in the header, the ParaView lists or the trailer itself" :
                                         " (the state does not match state_fp either: the damage is in the state";
      return Fail(CKPT_ERR_TRAILER, path,
                  "trailer: the file's contents give " + Hex(fp[0]) + Hex(fp[1]) + ", the trailer says " + Hex(trailer[0]) + Hex(trailer[1]) +
                     where + (bad.empty() ? std::string() : bad) + ")",
                  err);
   }
   if (!bad.empty()) { return Fail(CKPT_ERR_HEADER, path, "header: key " + bad + " missing or unreadable", err); }
   // 5. state_fp of the payload
   if (!state_ok)
   {
      return Fail(CKPT_ERR_STATE_FP, path, "state_fp: the state gives " + Hex(sfp[0]) + Hex(sfp[1]) + ", the header says " + Hex(h.state_fp[0]) + Hex(h.state_fp[1]), err);
   }
   out = std::move(c);
   err.clear();
   return CKPT_OK;
}

bool WriteLatest(const std::string &dir, const std::string &name)
{
   MakeDirChain(dir);
   const std::string path = dir + "/latest", tmp = path + ".tmp";
   std::FILE *f = std::fopen(tmp.c_str(), "wb");
   if (!f) { return false; }
   bool ok = std::fprintf(f, "%s\n", name.c_str()) > 0;
   ok = ok && std::fflush(f) == 0 && ::fsync(::fileno(f)) == 0;
   ok = (std::fclose(f) == 0) && ok;
   ok = ok && std::rename(tmp.c_str(), path.c_str()) == 0;
   if (!ok) { (void)std::remove(tmp.c_str()); }
   return ok;
}

bool ReadLatest(const std::string &dir, std::string &name)
{
   std::FILE *f = std::fopen((dir + "/latest").c_str(), "rb");
   if (!f) { return false; }
   char buf[512] = {0};
   const bool ok = std::fgets(buf, sizeof(buf), f) != nullptr;
   std::fclose(f);
   if (!ok) { return false; }
   name = buf;
   while (!name.empty() && (name.back() == '\n' || name.back() == '\r' || name.back() == ' ')) { name.pop_back(); }
   return !name.empty() && name.find('/') == std::string::npos;
}

} // namespace laghos
