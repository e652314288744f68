// records_sidecar.hpp — the `-peaks` records beside a checkpoint piece: <checkpoint piece>.rec.  Host only, no GPU
// code, like checkpoint.cpp; the checkpoint format itself does not change.  The reference has neither restart nor records.
//
// One file per rank, little endian:
//   header   ASCII `key value` lines, first line "LGHREC 1", second "header_bytes <n>", last "end", padded with '\n' to a multiple of
//            64 bytes: state_fp and ti of the checkpoint the records belong to, the time of the last update, R (-vr), whether a
//            threshold is set and its bits, then per point set one line "set <tag> <points>"; doubles as the 16 hex digits of their bits
//   payload  per point set its block, LGH_RECORDS_COLS x points float64 (column-major: rec[c * points + i])
//   trailer  the fingerprint (include/lgh_fingerprint.h, two uint64) of everything before it, taken as 64-bit words
#pragma once
#include <string>
#include <vector>

namespace laghos
{

constexpr int kRecordCols = 8; // LGH_RECORDS_COLS

struct RecordsSidecar
{
   unsigned long long state_fp[2] = {0, 0}; // of the checkpoint piece beside it
   long ti = 0;                             // its cycle
   double time = 0;                         // the time of the last update of the records
   int R = 0;                               // lattice cells per zone and direction
   int threshold_set = 0;                   // -peaks-arrival given
   double threshold = 0;                    // its value (compared by its bits)
   std::vector<std::string> tags;           // "volume", "surface", "slice_x2", ... in the order of the run
   std::vector<long> points;
   std::vector<std::vector<double>> blocks; // kRecordCols * points[k] each
};

enum RecordsSidecarError
{
   REC_OK = 0,
   REC_ERR_IO = 1,        // cannot open / write / rename; on reading: the file is missing
   REC_ERR_MAGIC = 2,     // first line is not "LGHREC 1"
   REC_ERR_HEADER = 3,    // header_bytes or a key missing or unreadable
   REC_ERR_TRUNCATED = 4, // shorter than header + blocks + trailer
   REC_ERR_SIZE = 5,      // longer than that
   REC_ERR_TRAILER = 6,   // the fingerprint of header + blocks is not the trailer
   REC_ERR_STATE_FP = 7,  // the sidecar belongs to another checkpoint
   REC_ERR_VR = 8,        // written with another -vr
   REC_ERR_THRESHOLD = 9, // written with another -peaks-arrival
   REC_ERR_SETS = 10,     // other point sets (tags or point counts)
   REC_ERR_CAPACITY = 11  // (host probe) the caller's arrays are too small
};

std::string RecordsSidecarPath(const std::string &checkpoint_piece); // <piece>.rec

// Writes <path>.tmp, flushes it to the disk and renames it to <path>.  Returns a RecordsSidecarError, its message in err.
int WriteRecordsSidecar(const std::string &path, const RecordsSidecar &rec, std::string &err);
// Reads and checks <path>: magic, header, the file size against the point counts, the trailer.  `out` is only assigned when every
// check has passed.
int ReadRecordsSidecar(const std::string &path, RecordsSidecar &out, std::string &err);
// Whether the sidecar read from <path> is the one this run continues from: the checkpoint's state_fp, -vr, the threshold and the
// point sets, in this order; each refusal has its own message naming the file.
int MatchRecordsSidecar(const std::string &path, const RecordsSidecar &have, const unsigned long long state_fp[2], int R, int threshold_set, double threshold,
                        const std::vector<std::string> &tags, const std::vector<long> &points, std::string &err);

} // namespace laghos
