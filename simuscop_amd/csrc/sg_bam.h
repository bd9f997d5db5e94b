// sg_bam.h -- BGZF inflate (sg_inflate.hip) and BAM records (sg_bam.hip) on the device, shared with the host API.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sg_bgzf.h"   // InflateMember, kBgzfMaxIsize, kBgzfMinMember

namespace sg {

constexpr uint32_t kCrcLaneBytes = 1024;     // inflate_kernel: each of the 64 lanes takes the CRC of 1 KiB of a member
constexpr uint32_t kCrcLevels = 6;           // combine tree over the 64 lanes
constexpr uint32_t kBamSegment = 16384;      // record boundaries: bytes of the stream per speculating thread

// inflate verdicts, one per member (0: inflated, CRC-32 and ISIZE as the trailer says)
enum : uint32_t { kInflOk = 0, kInflBlockType, kInflBadCode, kInflDistance, kInflOverrun, kInflTooLong, kInflIsize, kInflCrc,
                  kInflStoredLen, kInflHeader };
struct InflateJob {
  const uint8_t* src;          // the compressed batch
  uint64_t src_bytes;
  const InflateMember* members;
  uint32_t n;
  uint8_t* out;                // inflated bytes land at out + members[i].dst
  uint32_t* status;            // [n]
  const uint32_t* crc_tab;     // [256] reflected 0xEDB88320
  const uint32_t* crc_shift;   // [kCrcLevels][8][16]: "advance by 1024 * 2^k zero bytes" applied to nibble i holding value v
};
void launch_inflate(const InflateJob& J, hipStream_t s);
// host copies of the CRC tables above (built once)
const uint32_t* inflate_crc_tab();
const uint32_t* inflate_crc_shift();

// ---- records of the decompressed stream ----
struct BamJob {
  const uint8_t* d;            // decompressed stream of this call: [partial record carried in][inflated members]
  uint64_t base, L;            // the first record starts at `base`; bytes [0, L) are valid
  uint32_t n_ref;
  const char* names;           // reference names, NUL terminated, at name_off[i]
  const uint64_t* name_off;
  // boundaries (segment b = [base + b * kBamSegment, base + (b + 1) * kBamSegment))
  uint32_t n_seg;
  uint64_t* guess;             // [n_seg] speculated first record start, then the true one
  uint64_t* exit;              // [n_seg] first chain offset at or behind the segment's end from the guess
  uint32_t* count;             // [n_seg] complete records started in the segment
  uint64_t* first;             // [n_seg] exclusive scan of count
  uint64_t* scan_bsum;
  uint64_t* totals;            // [0] records, [1] text bytes, [2] tail (start of the partial record left), [3] error key
  uint64_t* rec;               // [records] start of every record
  uint64_t n_rec;
  uint32_t* line_len;          // [n_rec] rendered bytes (0: filtered out)
  uint64_t* line_off;          // [n_rec]
  char* text;
};
// error key: (offset in the stream << 8) | code, the least one wins
enum : uint32_t { kBamOk = 0, kBamShort = 1, kBamOpCode = 2, kBamRefId = 3, kBamLengths = 4 };
void launch_bam_guess(const BamJob& J, hipStream_t s);     // speculate: first start and exit of every segment
void launch_bam_verify(const BamJob& J, hipStream_t s);    // exit[b - 1] == entry[b], else walk again; tail, counts
void launch_bam_starts(const BamJob& J, hipStream_t s);    // (after the scan of count) every record start
void launch_bam_measure(const BamJob& J, hipStream_t s);   // filter, check, rendered length
void launch_bam_render(const BamJob& J, hipStream_t s);    // (after the scan of line_len) the eleven fields as text

}  // namespace sg
