// host/truth_sort.h -- --truth-sort: the truth BAM of a stem in coordinate order (the order: sg_bamsort.h).
// Every piece's pass comes off the device sorted (sg_bamsort_pass) and is appended as one run to a spool file beside the
// BAM; at the stem's close the key space is cut into tiles that fit the device (sort_tiles), and tile by tile the runs'
// byte ranges are read back, merged on the device (sg_bamsort_merge) and appended to the BAM as BGZF members.
// Host memory: 12 bytes per record for the stem's keys and lengths (and 8 more while the tiles are cut); disk: the
// record stream once, uncompressed.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "simulate.h"
#include "truth_outputs.h"

namespace simu {

// Default of the bytes of records one tile holds.  A capacity bound, not a tuned number: the device holds a tile's
// records twice (input and output), their members (about a fifth) and 28 bytes per record of keys, payloads and offsets.
// SIMU_SORT_TILE_BYTES overrides it.
constexpr uint64_t kSortTileBytes = 1ull << 30;
// A tile of one key value needs no sort and is passed through in chunks of at most max(budget, kSortMinChunk) bytes.
constexpr uint64_t kSortMinChunk = 1ull << 20;

struct SortTiles {
  std::vector<uint64_t> first;     // ascending; tile i holds the records with first[i] <= key < first[i + 1] (the last: all from first[i] on)
  std::vector<uint8_t> single;     // 1: the tile is one key value that alone exceeds the budget
};
// The cut (simu_sort_tiles, simulate.h).  Run r: n[r] ascending keys and n[r] + 1 prefix sums of its records' bytes.
SortTiles sort_tiles(uint32_t n_runs, const uint64_t* const* keys, const uint64_t* n, const uint64_t* const* prefix, uint64_t budget);

class TruthSort {
 public:
  TruthSort(Engine& eng, simu_stats& st) : eng(eng), st(st) {}
  ~TruthSort() { drop(); }   // the spool goes with its owner on every path
  TruthSort(const TruthSort&) = delete;
  TruthSort& operator=(const TruthSort&) = delete;
  bool active() const { return spool != nullptr; }
  void open(const std::string& bam_path);   // a stem starts: <bam_path>.runs.tmp
  void add_run(uint64_t record_bytes);      // the pass sg_bamsort_pass has just made: its stream to the spool, its index to memory
  void finish(FILE* bam);                   // the stem ends: tiles, merges, members appended to `bam`; the spool is removed
  // --truth-index: every later stem's finish() also writes <bam_path>.bai (the rule: csrc/sg_bamindex.h).  Each compressed
  // text is indexed on the device while it is still there (sg_bamindex_add), behind the merge or the pass-through chunk
  // that made it; nothing about the BAM's bytes changes.
  void index_with(const std::vector<uint64_t>& lens) { indexing = true; ref_len = lens; }

 private:
  struct Run {
    uint64_t at = 0;   // where the run starts in the spool
    std::vector<uint64_t> keys;
    std::vector<uint32_t> lens;
  };
  void drop();
  void read_spool(uint64_t at, uint64_t bytes, uint8_t* dst);
  void put_members(FILE* bam, const uint8_t* p, uint64_t n);
  void flush_stage(FILE* bam);
  void stage_from_run(const Run& run, uint64_t& rec, uint64_t bytes);   // `bytes` more of the run's records are staged, from record `rec` on
  void index_added(uint64_t n_chunks, uint64_t first_voff);            // the rows of the sg_bamindex_add just made
  void write_index();
  bool indexing = false;
  std::vector<uint64_t> ref_len;
  std::vector<sg_bai_chunk> rows;   // the stem's chunk rows in call order
  size_t open_row = SIZE_MAX;       // the one whose end the next call's first record closes
  uint64_t file_at = 0;             // where the next member lands in the BAM file
  uint64_t rec_left = 0, stage_skip = 0;   // pass-through: bytes of the record being staged still to come; those at the stage's front that belong to an earlier one
  std::vector<uint32_t> stage_lens;        // ... lengths of the records that start in the stage
  Engine& eng;
  simu_stats& st;
  std::string path, bam_path;
  FILE* spool = nullptr;
  uint64_t spool_bytes = 0;
  std::vector<Run> runs;
  std::vector<uint8_t> buf, stage, members;
};

}  // namespace simu
