// records_sidecar.cpp — see records_sidecar.hpp.  Host only: no HIP, no MFEM.
#include "records_sidecar.hpp"

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <sys/stat.h>
#include <unistd.h>

#include "checkpoint.hpp"

namespace laghos
{

namespace
{

constexpr long kAlign = 64;
constexpr long kMaxHeader = 1L << 20;

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
std::string Dec(double v)
{
   char buf[40];
   std::snprintf(buf, sizeof(buf), "%.17g", v);
   return buf;
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
   err = "records sidecar " + path + ": " + what;
   return code;
}

std::string HeaderText(const RecordsSidecar &r, long header_bytes)
{
   std::ostringstream os;
   os << "LGHREC 1\n";
   os << "header_bytes " << header_bytes << "\n";
   os << "state_fp " << Hex(r.state_fp[0]) << " " << Hex(r.state_fp[1]) << "\n";
   os << "ti " << r.ti << "\n";
   os << "time " << Hex(Bits(r.time)) << " # " << Dec(r.time) << "\n";
   os << "R " << r.R << "\n";
   os << "threshold " << (r.threshold_set ? 1 : 0) << " " << Hex(Bits(r.threshold_set ? r.threshold : 0.0)) << " # " << Dec(r.threshold_set ? r.threshold : 0.0) << "\n";
   os << "sets " << r.tags.size() << "\n";
   for (size_t k = 0; k < r.tags.size(); k++) { os << "set " << r.tags[k] << " " << r.points[k] << "\n"; }
   os << "end\n";
   return os.str();
}

void FingerprintHeader(const std::string &head, unsigned long long fp[2])
{
   std::vector<unsigned long long> hw(head.size() / 8); // (copied: a std::string's bytes need not be 8-byte aligned)
   std::memcpy(hw.data(), head.data(), hw.size() * 8);
   FingerprintWords(hw.data(), (long)hw.size(), 0ULL, fp);
}

std::string SetList(const std::vector<std::string> &tags, const std::vector<long> &points)
{
   std::string s;
   for (size_t k = 0; k < tags.size(); k++) { s += (k ? ", " : "") + tags[k] + " (" + std::to_string(points[k]) + " points)"; }
   return s.empty() ? "none" : s;
}

} // namespace

std::string RecordsSidecarPath(const std::string &checkpoint_piece) { return checkpoint_piece + ".rec"; }

int WriteRecordsSidecar(const std::string &path, const RecordsSidecar &r, std::string &err)
{
   if (r.tags.size() != r.points.size() || r.tags.size() != r.blocks.size()) { return Fail(REC_ERR_IO, path, "write: bad arguments", err); }
   for (size_t k = 0; k < r.tags.size(); k++)
   {
      if (r.points[k] < 0 || (long)r.blocks[k].size() != kRecordCols * r.points[k] || r.tags[k].empty() || r.tags[k].find_first_of(" \t\n#") != std::string::npos)
      {
         return Fail(REC_ERR_IO, path, "write: bad arguments (point set " + std::to_string(k) + ")", err);
      }
   }
   // header_bytes is part of the text: size the text with a value of the final width, then pad
   long header_bytes = kAlign;
   for (int pass = 0; pass < 3; pass++)
   {
      const long need = (long)HeaderText(r, header_bytes).size();
      const long padded = (need + kAlign - 1) / kAlign * kAlign;
      if (padded == header_bytes) { break; }
      header_bytes = padded;
   }
   std::string head = HeaderText(r, header_bytes);
   if ((long)head.size() > header_bytes) { return Fail(REC_ERR_IO, path, "write: the header does not fit its padding", err); }
   head.resize((size_t)header_bytes, '\n');
   unsigned long long trailer[2] = {0ULL, 0ULL};
   FingerprintHeader(head, trailer);
   unsigned long long off = (unsigned long long)header_bytes / 8;
   for (const std::vector<double> &b : r.blocks)
   {
      FingerprintWords(b.data(), (long)b.size(), off, trailer);
      off += b.size();
   }
   const std::string tmp = path + ".tmp";
   std::FILE *f = std::fopen(tmp.c_str(), "wb");
   if (!f) { return Fail(REC_ERR_IO, path, std::string("write: cannot open ") + tmp + " (" + std::strerror(errno) + ")", err); }
   bool ok = std::fwrite(head.data(), 1, head.size(), f) == head.size();
   for (const std::vector<double> &b : r.blocks) { ok = ok && (b.empty() || std::fwrite(b.data(), sizeof(double), b.size(), f) == b.size()); }
   ok = ok && std::fwrite(trailer, sizeof(unsigned long long), 2, f) == 2;
   ok = ok && std::fflush(f) == 0 && ::fsync(::fileno(f)) == 0;
   ok = (std::fclose(f) == 0) && ok;
   if (!ok)
   {
      (void)std::remove(tmp.c_str());
      return Fail(REC_ERR_IO, path, "write: cannot write " + tmp, err);
   }
   if (std::rename(tmp.c_str(), path.c_str()) != 0)
   {
      (void)std::remove(tmp.c_str());
      return Fail(REC_ERR_IO, path, std::string("write: cannot rename ") + tmp + " (" + std::strerror(errno) + ")", err);
   }
   err.clear();
   return REC_OK;
}

int ReadRecordsSidecar(const std::string &path, RecordsSidecar &out, std::string &err)
{
   std::FILE *f = std::fopen(path.c_str(), "rb");
   if (!f) { return Fail(REC_ERR_IO, path, std::string("missing: cannot open the file (") + std::strerror(errno) + ")", err); }
   struct Closer
   {
      std::FILE *f;
      ~Closer() { std::fclose(f); }
   } closer{f};
   struct stat st;
   if (::fstat(::fileno(f), &st) != 0) { return Fail(REC_ERR_IO, path, "cannot stat the file", err); }
   const long file_bytes = (long)st.st_size;
   std::string head((size_t)std::min<long>(file_bytes, 256), '\0');
   if (!head.empty() && std::fread(&head[0], 1, head.size(), f) != head.size()) { return Fail(REC_ERR_IO, path, "cannot read the file", err); }
   // 1. magic and version, header_bytes: the first two lines
   const size_t l1 = head.find('\n'), l2 = (l1 == std::string::npos) ? l1 : head.find('\n', l1 + 1);
   {
      const std::vector<std::string> tk = Tokens(head.substr(0, l1 == std::string::npos ? head.size() : l1));
      if (l1 == std::string::npos || tk.size() != 2 || tk[0] != "LGHREC" || tk[1] != "1")
      {
         return Fail(REC_ERR_MAGIC, path, "magic: the first line is not \"LGHREC 1\" - not a records sidecar of this driver", err);
      }
   }
   long header_bytes = 0;
   {
      const std::vector<std::string> tk = Tokens(l2 == std::string::npos ? std::string() : head.substr(l1 + 1, l2 - l1 - 1));
      if (tk.size() != 2 || tk[0] != "header_bytes" || !ParseLong(tk[1], header_bytes) || header_bytes < kAlign || header_bytes % kAlign != 0 || header_bytes > kMaxHeader)
      {
         return Fail(REC_ERR_HEADER, path, "header_bytes: the second line is not \"header_bytes <multiple of 64>\"", err);
      }
      if (header_bytes > file_bytes)
      {
         return Fail(REC_ERR_TRUNCATED, path,
                     "truncated: the header is " + std::to_string(header_bytes) + " bytes, the file only " + std::to_string(file_bytes) + " (cut inside the header)", err);
      }
   }
   if (header_bytes > (long)head.size())
   {
      const size_t have = head.size();
      head.resize((size_t)header_bytes);
      if (std::fread(&head[have], 1, head.size() - have, f) != head.size() - have) { return Fail(REC_ERR_IO, path, "cannot read the header", err); }
   }
   else
   {
      head.resize((size_t)header_bytes);
      if (std::fseek(f, header_bytes, SEEK_SET) != 0) { return Fail(REC_ERR_IO, path, "cannot read the file", err); }
   }
   // 2. the key / value lines up to "end"
   RecordsSidecar r;
   std::string bad;
   bool ended = false;
   long nsets = -1;
   {
      std::istringstream is(head);
      std::string line;
      std::getline(is, line); // magic
      std::getline(is, line); // header_bytes
      auto want = [&](bool ok, const char *key) { if (!ok && bad.empty()) { bad = key; } };
      while (std::getline(is, line))
      {
         const std::vector<std::string> tk = Tokens(line);
         if (tk.empty()) { continue; }
         if (tk[0] == "end") { ended = true; break; }
         unsigned long long b = 0;
         long l = 0;
         if (tk[0] == "state_fp") { want(tk.size() == 3 && ParseHex(tk[1], r.state_fp[0]) && ParseHex(tk[2], r.state_fp[1]), "state_fp"); }
         else if (tk[0] == "ti") { want(tk.size() == 2 && ParseLong(tk[1], r.ti), "ti"); }
         else if (tk[0] == "time") { want(tk.size() == 2 && ParseHex(tk[1], b), "time"); r.time = FromBits(b); }
         else if (tk[0] == "R") { want(tk.size() == 2 && ParseLong(tk[1], l), "R"); r.R = (int)l; }
         else if (tk[0] == "threshold")
         {
            want(tk.size() == 3 && ParseLong(tk[1], l) && (l == 0 || l == 1) && ParseHex(tk[2], b), "threshold");
            r.threshold_set = (int)l;
            r.threshold = FromBits(b);
         }
         else if (tk[0] == "sets") { want(tk.size() == 2 && ParseLong(tk[1], nsets) && nsets >= 0 && nsets < 4096, "sets"); }
         else if (tk[0] == "set")
         {
            want(tk.size() == 3 && ParseLong(tk[2], l) && l >= 0 && l < (1L << 48), "set");
            if (tk.size() == 3) { r.tags.push_back(tk[1]); r.points.push_back(l); }
         }
         else { want(false, "(an unknown key)"); }
      }
   }
   if (!ended) { return Fail(REC_ERR_HEADER, path, "header: no \"end\" line inside header_bytes", err); }
   if (bad == "sets" || bad == "set" || nsets != (long)r.tags.size()) { return Fail(REC_ERR_HEADER, path, "header: the list of point sets is missing or unreadable", err); }
   // 3. the file size against the point counts
   long words = 0;
   for (long n : r.points) { words += kRecordCols * n; }
   const long expect = header_bytes + 8 * words + 16;
   if (file_bytes < expect)
   {
      return Fail(REC_ERR_TRUNCATED, path, "truncated: its point sets need " + std::to_string(expect) + " bytes, the file has " + std::to_string(file_bytes), err);
   }
   if (file_bytes != expect)
   {
      return Fail(REC_ERR_SIZE, path, "size: its point sets make " + std::to_string(expect) + " bytes, the file has " + std::to_string(file_bytes), err);
   }
   // 4. the trailer
   unsigned long long fp[2] = {0ULL, 0ULL}, trailer[2] = {0ULL, 0ULL};
   FingerprintHeader(head, fp);
   unsigned long long off = (unsigned long long)header_bytes / 8;
   for (long n : r.points)
   {
      r.blocks.emplace_back((size_t)(kRecordCols * n));
      std::vector<double> &b = r.blocks.back();
      if (!b.empty() && std::fread(b.data(), 8, b.size(), f) != b.size()) { return Fail(REC_ERR_IO, path, "cannot read the records", err); }
      FingerprintWords(b.data(), (long)b.size(), off, fp);
      off += b.size();
   }
   if (std::fread(trailer, 8, 2, f) != 2) { return Fail(REC_ERR_IO, path, "cannot read the trailer", err); }
   if (fp[0] != trailer[0] || fp[1] != trailer[1])
   {
      return Fail(REC_ERR_TRAILER, path, "trailer: the file's contents give " + Hex(fp[0]) + Hex(fp[1]) + ", the trailer says " + Hex(trailer[0]) + Hex(trailer[1]), err);
   }
   if (!bad.empty()) { return Fail(REC_ERR_HEADER, path, "header: key " + bad + " missing or unreadable", err); }
   out = std::move(r);
   err.clear();
   return REC_OK;
}

int MatchRecordsSidecar(const std::string &path, const RecordsSidecar &have, const unsigned long long state_fp[2], int R, int threshold_set, double threshold,
                        const std::vector<std::string> &tags, const std::vector<long> &points, std::string &err)
{
   if (have.state_fp[0] != state_fp[0] || have.state_fp[1] != state_fp[1])
   {
      return Fail(REC_ERR_STATE_FP, path,
                  "state_fp: it belongs to another checkpoint: it names the state " + Hex(have.state_fp[0]) + Hex(have.state_fp[1]) + " (cycle " + std::to_string(have.ti) +
                     "), the checkpoint holds " + Hex(state_fp[0]) + Hex(state_fp[1]),
                  err);
   }
   if (have.R != R) { return Fail(REC_ERR_VR, path, "-vr: its records lie on a lattice of " + std::to_string(have.R) + " cells per zone and direction, this run's -vr is " + std::to_string(R), err); }
   const bool same_threshold = (have.threshold_set != 0) == (threshold_set != 0) && (!threshold_set || Bits(have.threshold) == Bits(threshold));
   if (!same_threshold)
   {
      const std::string was = have.threshold_set ? Dec(have.threshold) : "not given", is = threshold_set ? Dec(threshold) : "not given";
      return Fail(REC_ERR_THRESHOLD, path, "threshold: -peaks-arrival was " + was + " in its run, it is " + is + " in this one", err);
   }
   if (have.tags != tags || have.points != points)
   {
      return Fail(REC_ERR_SETS, path, "point sets: it holds " + SetList(have.tags, have.points) + ", this run keeps " + SetList(tags, points), err);
   }
   err.clear();
   return REC_OK;
}

} // namespace laghos
