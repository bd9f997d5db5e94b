// sg_eval.h -- truthEval: an aligner's BAM scored against the truth BAM (kernels: sg_eval.hip, entry points: sg_api_eval.cpp,
// command line: host/eval.cpp).  The rule is stated here once; DESIGN.md 10j quotes it.
//
// A read is (QNAME bytes, mate); mate = 1 when FLAG has 0x80, else 0.  Nothing is stripped from the name.
// Its key is eval_key: FNV-1a (64 bit) over the name bytes and then the mate byte, mixed by the finalizer of
// MurmurHash3 so that every bit of the key depends on every byte, and cut to the low key_bits bits.  Equal keys are only
// candidates: a match is equal name bytes and equal mate.
//
// A record's reference interval is [POS, POS + span): span = the sum of its M, D, N, = and X lengths, 1 for a record
// without operations.  The test record's refID is given in the truth's numbering (-1: a contig the truth lacks, or none).
//
// The categories of a scored pair, the first that applies:
//   both_unmapped  test FLAG 4 and truth FLAG 4          lost      test FLAG 4, truth mapped
//   invented       test mapped, truth FLAG 4             wrong_contig  another contig, or none
//   wrong_strand   same contig, other strand (FLAG 0x10)
//   exact          same POS and the same interval end
//   near           overlap >= 1 and overlap * 100 >= pct * min(span_truth, span_test), in u64
//   wrong_place    anything else on the same contig and strand
// The truth class of a pair: plain (the truth CIGAR is one M operation), edited (any other mapped truth), unmapped.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sg {

enum : uint32_t { kEvalExact = 0, kEvalNear, kEvalWrongPlace, kEvalWrongStrand, kEvalWrongContig, kEvalLost, kEvalInvented, kEvalBothUnmapped,
                  kEvalCategories };
enum : uint32_t { kEvalPlain = 0, kEvalEdited, kEvalUnmapped, kEvalClasses };
constexpr uint32_t kEvalMapqs = 256;
constexpr uint32_t kEvalCells = 2 * kEvalClasses * kEvalMapqs * kEvalCategories;   // [mate][class][MAPQ][category]
// the scalar counts behind the table, in the order of sg_eval_counts
enum : uint32_t { kEvalNTest = 0, kEvalNSecondary, kEvalNSupplementary, kEvalNUnknown, kEvalNAmbiguous, kEvalNRepeated, kEvalScalars };
constexpr uint32_t kEvalMissing = 2 * kEvalClasses;   // [mate][class]

__host__ __device__ inline uint32_t eval_cell(uint32_t mate, uint32_t cls, uint32_t mapq, uint32_t cat) {
  return ((mate * kEvalClasses + cls) * kEvalMapqs + mapq) * kEvalCategories + cat;
}

// one side of a pair
struct EvalAln {
  int32_t ref;        // refID in the truth's numbering
  int64_t pos;        // 0-based POS
  uint64_t span;
  uint32_t reverse;   // FLAG 0x10
  uint32_t unmapped;  // FLAG 4
};

__host__ __device__ inline uint32_t eval_classify(const EvalAln& t, const EvalAln& q, uint32_t pct) {
  if (q.unmapped) return t.unmapped ? kEvalBothUnmapped : kEvalLost;
  if (t.unmapped) return kEvalInvented;
  if (q.ref < 0 || q.ref != t.ref) return kEvalWrongContig;
  if ((q.reverse != 0) != (t.reverse != 0)) return kEvalWrongStrand;
  const int64_t t_end = t.pos + (int64_t)t.span, q_end = q.pos + (int64_t)q.span;
  if (q.pos == t.pos && q_end == t_end) return kEvalExact;
  const int64_t lo = t.pos > q.pos ? t.pos : q.pos, hi = t_end < q_end ? t_end : q_end;
  const uint64_t overlap = hi > lo ? (uint64_t)(hi - lo) : 0, least = t.span < q.span ? t.span : q.span;
  if (overlap >= 1 && overlap * 100ull >= (uint64_t)pct * least) return kEvalNear;
  return kEvalWrongPlace;
}

__host__ __device__ inline uint64_t eval_key(const uint8_t* name, uint32_t len, uint32_t mate, uint32_t key_bits) {
  uint64_t h = 0xCBF29CE484222325ull;
  for (uint32_t i = 0; i < len; i++) h = (h ^ name[i]) * 0x100000001B3ull;
  h = (h ^ (uint64_t)(mate & 1u)) * 0x100000001B3ull;
  h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull;
  h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull;
  h ^= h >> 33;
  return key_bits >= 64 ? h : h & ((1ull << key_bits) - 1);
}

// ---- the device side ----
// a truth read, 40 bytes.  bits: [0..7] name bytes (without the NUL), 8 reverse, 9 unmapped, 10..11 class, 12 mate,
// 13 duplicate (another row has the same name and mate: set by the duplicates kernel)
struct EvalRow {
  uint64_t key;
  uint64_t name_off;   // in the arena
  uint64_t span;
  int32_t ref, pos;
  uint32_t bits, pad;
};
constexpr uint32_t kRowReverse = 1u << 8, kRowUnmapped = 1u << 9, kRowMate = 1u << 12, kRowDup = 1u << 13;
__host__ __device__ inline uint32_t row_name_len(uint32_t bits) { return bits & 255u; }
__host__ __device__ inline uint32_t row_class(uint32_t bits) { return (bits >> 10) & 3u; }

// what the look-up kernel says of a test record
enum : uint8_t { kHitRow = 0, kHitUnknown, kHitAmbiguous, kHitSecondary, kHitSupplementary };

struct BamJob;
struct EvalJob {
  uint32_t key_bits, pct;
  // the truth: rows in file order, their names, and after the sort the keys in order with their rows
  EvalRow* rows;
  uint64_t n_rows;          // rows in front of this call's
  uint8_t* arena;
  uint64_t arena_used;      // bytes in front of this call's names
  const uint64_t* keys;     // [n_rows] sorted
  const uint32_t* order;    // [n_rows] row of sorted position j
  unsigned long long* claim;   // [n_rows] least ordinal of a primary test record that found the row (~0: none)
  // a call's records (BamJob.rec / n_rec)
  uint32_t* name_len;       // [n_rec] truth: bytes of the name
  uint64_t* name_at;        // [n_rec] truth: their scan
  uint32_t* hit_row;        // [n_rec] test
  uint8_t* hit;             // [n_rec] test
  uint64_t ordinal0;        // ordinal in the file of the call's first record
  const int32_t* refmap;    // test refID -> truth refID or -1
  unsigned long long* table;     // [kEvalCells] then [kEvalScalars] then [kEvalMissing]
  unsigned long long* error;     // the BamJob's error key (totals[3])
  unsigned long long* dup_count; // rows marked duplicate
};

void launch_eval_truth_rows(const BamJob& B, const EvalJob& E, hipStream_t s);    // check, key, span: a row per record; name_len
void launch_eval_truth_names(const BamJob& B, const EvalJob& E, hipStream_t s);   // (after the scan of name_len) names into the arena
void launch_eval_sort_input(const EvalRow* rows, uint32_t n, uint64_t* keys, uint32_t* vals, hipStream_t s);
void launch_eval_duplicates(const EvalJob& E, uint32_t n, hipStream_t s);         // (after the sort) kRowDup, claim = ~0
void launch_eval_lookup(const BamJob& B, const EvalJob& E, hipStream_t s);
void launch_eval_claim(const BamJob& B, const EvalJob& E, hipStream_t s);
void launch_eval_score(const BamJob& B, const EvalJob& E, hipStream_t s);
void launch_eval_missing(const EvalJob& E, uint64_t n, hipStream_t s);

}  // namespace sg
