// sg_bamindex.h -- the BAI index of the sorted truth BAM (simuReads --truth-index; kernels: sg_bamindex.hip, entry
// points: sg_api_bamindex.cpp, serialiser: host/truth_index.cpp).
//
// The index, stated once (DESIGN.md 10h quotes it).  A BAI as in SAMv1 5.2: min_shift 14, depth 5, magic BAI\1.
//   Fields of a record.  beg = POS; end = POS + the reference length of the CIGAR (M, D, N, =, X), POS + 1 when that
//     length is 0 or the record has FLAG 0x4; bin = truth_reg2bin(beg, end).  end and bin come from the record's bytes,
//     as an indexer takes them; the record's own bin field is not used.
//   Virtual offsets.  A record that starts at uncompressed position u of a compressed text whose first member lies at
//     file offset F has voff = (F + moff[u >> 15]) << 16 | (u & 32767).  A record's end offset is the start offset of the
//     next record in the file (what bgzf_tell gives behind the record, also at a member's end); the last record's is
//     (offset of the end-of-file block) << 16.  So only start offsets are computed, and a record that straddles two
//     members, two tiles or two pass-through chunks needs no special case.
//   Chunks.  A chunk is a maximal run of consecutive records with the same (refID, bin) and refID >= 0; it spans [voff
//     of its first record, end offset of its last).  Within a bin, chunks are in file order; two neighbouring chunks of
//     a bin with end == beg are joined (that can only happen where a run crosses a call boundary).
//   Bins of a reference are written in ascending number.
//   Pseudo-bin 37450 is written last for a reference, and only for one that has records: (voff of the reference's first
//     record, end offset of its last record), then (records without 0x4, records with 0x4).
//   n_no_coor, the number of records with refID -1, is always written.
//   Linear index.  Every record with refID >= 0 enters the windows beg >> 14 .. (end - 1) >> 14 -- a 0x4 record placed
//     at its mate too, as [POS, POS + 1): SAMv1's "treated as length 1".  (An unmapped mate in front of its mapped mate
//     at the same POS can have another bin than the mate; its chunk then ends exactly where the mate begins, and with
//     htslib's rule, mapped records only, a reader's chunk.end > ioffset test would drop it.)  n_intv = last window
//     touched + 1; a window no record touches takes the value of the next touched window on its right (htslib's rule);
//     no entry is left at ~0.
//   A reference without records has n_bin = 0 and n_intv = 0; a stem without records still gets a valid file.
//   Not byte-equal to `samtools index`: htslib also folds small bins into their parents and writes bins in hash order.
//   Limits.  BAI cannot address positions >= 2^29: a reference longer than 2^29 is refused.  No .csi.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sg {

constexpr uint32_t kBaiMaxLen = 1u << 29;     // positions a BAI addresses
constexpr uint32_t kBaiShift = 14;            // a linear window's bases, as a shift
constexpr uint32_t kBaiPseudoBin = 37450;

// SAMv1 5.3 reg2bin for [beg, end), 0 <= beg < end <= 2^29
__host__ __device__ inline uint32_t truth_reg2bin(uint32_t beg, uint32_t end) {
  --end;
  if (beg >> 14 == end >> 14) return 4681u + (beg >> 14);
  if (beg >> 17 == end >> 17) return 585u + (beg >> 17);
  if (beg >> 20 == end >> 20) return 73u + (beg >> 20);
  if (beg >> 23 == end >> 23) return 9u + (beg >> 23);
  if (beg >> 26 == end >> 26) return 1u + (beg >> 26);
  return 0u;
}

// what bamindex_rows_kernel leaves of a record
struct BaiRow {
  int32_t ref, beg, end;
  uint32_t bin_unmapped;   // bin | (FLAG 0x4) << 31
};
// a reference for the kernels: its first slot in the stem's linear index and its length
struct BaiRef {
  uint64_t win_first, len;
};
// bits of *flags: a record that does not parse (its block_size, name and CIGAR do not fit its length); a record outside
// its reference or the references; a record outside the text
constexpr unsigned long long kBaiBadRecord = 1, kBaiBadPlace = 2, kBaiBadOffset = 4;

// What a call indexes.  Record i of m: i < carried is the record begun in an earlier text, whole in `carry`, with the
// start offset carry_voff; the others start at skip + off[i - carried] of `text` (bytes long, followed by 64 readable
// bytes, like carry) and are len[i - carried] bytes long.  moff: the text's member offset table (bytes / 32768 rounded
// up entries), file_off the file offset of its first member.
struct BaiJob {
  const uint8_t* text;
  uint64_t bytes;
  const uint64_t* off;
  const uint32_t* len;
  uint64_t skip;
  const uint8_t* carry;
  uint32_t carry_len, carried;
  uint64_t carry_voff;
  const uint64_t* moff;
  uint64_t file_off;
  uint32_t m;
  const BaiRef* refs;
  uint32_t n_ref;
};

// rows[i], voff[i] of every record; the stem's linear index (u64 atomicMin of voff, slot refs[ref].win_first + window)
// and counts ([3 ref] records without 0x4, [3 ref + 1] with 0x4, [3 ref + 2] smallest voff, [3 n_ref] records with
// refID -1) updated; a record that sets a flag enters neither.
void launch_bamindex_rows(const BaiJob& J, BaiRow* rows, uint64_t* voff, unsigned long long* linear, unsigned long long* counts,
                          unsigned long long* flags, hipStream_t s);
// head[i] = 1 where record i starts a run of equal chunk keys (the key: refID << 32 | bin, n_ref << 32 for refID -1)
void launch_bamindex_heads(const BaiRow* rows, uint32_t m, uint32_t n_ref, uint32_t* head, hipStream_t s);
// rank = exclusive scan of head, *total its sum: chunk `rank` gets its key, its start, and ends the one before it; the
// last one stays open (~0).  *no_coor += chunks of refID -1.  pay[c] = c.
void launch_bamindex_compact(const BaiRow* rows, const uint64_t* voff, const uint32_t* head, const uint64_t* rank, const uint64_t* total, uint32_t m,
                             uint32_t n_ref, uint64_t* ckey, uint64_t* cbeg, uint64_t* cend, uint32_t* pay, unsigned long long* no_coor, hipStream_t s);
// out[3 j ..] = {key, beg, end} of chunk pay[j]
void launch_bamindex_gather(const uint64_t* ckey, const uint32_t* pay, const uint64_t* cbeg, const uint64_t* cend, uint32_t n, uint64_t* out,
                            hipStream_t s);
// u64 cells set to ~0
void launch_bamindex_fill(unsigned long long* p, uint64_t n, hipStream_t s);

}  // namespace sg
