// host/truth_sort.cpp -- see truth_sort.h
#include "truth_sort.h"

#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>

namespace simu {

SortTiles sort_tiles(uint32_t n_runs, const uint64_t* const* keys, const uint64_t* n, const uint64_t* const* prefix, uint64_t budget) {
  SortTiles T;
  const uint64_t tiles = simu_sort_tiles(n_runs, keys, n, prefix, budget, nullptr, nullptr, 0);
  if (tiles == UINT64_MAX) throw Error("Error: the truth BAM's runs cannot be cut into tiles", -1);
  T.first.resize(tiles);
  T.single.resize(tiles);
  simu_sort_tiles(n_runs, keys, n, prefix, budget, T.first.data(), T.single.data(), tiles);
  return T;
}

void TruthSort::drop() {
  if (spool) fclose(spool);
  spool = nullptr;
  if (!path.empty()) unlink(path.c_str());
  path.clear();
  runs.clear();
  spool_bytes = 0;
  rows.clear();
  open_row = SIZE_MAX;
  rec_left = stage_skip = 0;
  stage_lens.clear();
}

void TruthSort::open(const std::string& bam_path) {
  drop();
  this->bam_path = bam_path;
  path = bam_path + ".runs.tmp";
  spool = fopen(path.c_str(), "w+b");
  if (!spool) {
    const std::string p = path;
    path.clear();
    throw Error("Error: can not open the spool file of the sorted truth BAM:\n" + p, -1);
  }
}

void TruthSort::add_run(uint64_t record_bytes) {
  uint64_t n = 0;
  eng.check(sg_bamsort_index(eng.ctx, nullptr, nullptr, 0, &n), "sg_bamsort_index");
  if (!n) return;
  Run run;
  run.at = spool_bytes;
  run.keys.resize(n);
  run.lens.resize(n);
  eng.check(sg_bamsort_index(eng.ctx, run.keys.data(), run.lens.data(), n, &n), "sg_bamsort_index");
  if (buf.size() < record_bytes) buf.resize(record_bytes);
  eng.check(sg_bamsort_fetch(eng.ctx, 0, 0, record_bytes, buf.data()), "sg_bamsort_fetch");
  if (fseeko(spool, (off_t)spool_bytes, SEEK_SET) != 0 || fwrite(buf.data(), 1, record_bytes, spool) != record_bytes)
    throw Error("Error: short write to the spool file of the sorted truth BAM", -1);
  spool_bytes += record_bytes;
  runs.push_back(std::move(run));
}

void TruthSort::read_spool(uint64_t at, uint64_t bytes, uint8_t* dst) {
  if (!bytes) return;
  if (fseeko(spool, (off_t)at, SEEK_SET) != 0 || fread(dst, 1, bytes, spool) != bytes)
    throw Error("Error: short read from the spool file of the sorted truth BAM", -1);
}

void TruthSort::put_members(FILE* bam, const uint8_t* p, uint64_t n) {
  if (n && fwrite(p, 1, n, bam) != n) throw Error("Error: short write to the truth BAM file", -1);
  st.truth_bgzf_bytes += n;
}

// the passed-through bytes waiting in `stage`, compressed and appended
void TruthSort::flush_stage(FILE* bam) {
  if (stage.empty()) return;
  uint64_t n = 0;
  members.resize(std::max<size_t>(members.size(), stage.size() + stage.size() / 2 + 1024 * (stage.size() / 32768 + 2)));
  int rc = sg_deflate_bgzf(eng.ctx, stage.data(), stage.size(), members.data(), members.size(), &n);
  if (rc == SG_ERR_OVERFLOW) {
    members.resize(n);
    rc = sg_deflate_bgzf(eng.ctx, stage.data(), stage.size(), members.data(), members.size(), &n);
  }
  eng.check(rc, "sg_deflate_bgzf");
  if (indexing) {
    Timed acc{st.t_bai};
    uint64_t nc = 0, fv = 0;
    eng.check(sg_bamindex_add(eng.ctx, SG_BAMINDEX_DEFLATE, file_at, stage_skip, stage_lens.data(), stage_lens.size(), &nc, &fv), "sg_bamindex_add");
    index_added(nc, fv);
    stage_skip = rec_left;   // the record cut by this flush ends at the next stage's front
    stage_lens.clear();
  }
  put_members(bam, members.data(), n);
  file_at += n;
  stage.clear();
}

void TruthSort::stage_from_run(const Run& run, uint64_t& rec, uint64_t bytes) {
  while (bytes) {
    if (!rec_left) {
      rec_left = run.lens[rec++];
      stage_lens.push_back((uint32_t)rec_left);
    }
    const uint64_t c = std::min(rec_left, bytes);
    rec_left -= c;
    bytes -= c;
  }
}

void TruthSort::index_added(uint64_t n_chunks, uint64_t first_voff) {
  if (open_row != SIZE_MAX && first_voff != ~0ull) {
    rows[open_row].end = first_voff;
    open_row = SIZE_MAX;
  }
  const size_t old = rows.size();
  rows.resize(old + n_chunks);
  uint64_t n = 0;
  eng.check(sg_bamindex_chunks(eng.ctx, rows.data() + old, n_chunks, &n), "sg_bamindex_chunks");
  for (size_t i = old; i < rows.size(); i++)
    if (rows[i].end == ~0ull) open_row = i;
}

// the .bai goes with its owner unless it was written whole
namespace {
struct BaiFile {
  std::string path;
  FILE* f = nullptr;
  bool whole = false;
  ~BaiFile() {
    if (f) fclose(f);
    if (!whole && !path.empty()) unlink(path.c_str());
  }
};
}  // namespace

void TruthSort::write_index() {
  Timed acc{st.t_bai};
  if (open_row != SIZE_MAX) rows[open_row].end = file_at << 16;   // the end-of-file block follows
  open_row = SIZE_MAX;
  uint64_t n_win = 0;
  for (uint64_t ln : ref_len) n_win += (ln + 16383) >> 14;
  std::vector<uint64_t> linear(n_win + 1), counts(3 * ref_len.size() + 1);
  eng.check(sg_bamindex_finish(eng.ctx, linear.data(), n_win, counts.data()), "sg_bamindex_finish");
  uint64_t bins = 0, chunks = 0;
  const uint64_t need = simu_bai_build((uint32_t)ref_len.size(), ref_len.data(), rows.data(), rows.size(), linear.data(), counts.data(), nullptr, 0,
                                       &bins, &chunks);
  if (need == UINT64_MAX) throw Error("Error: the index rows of the sorted truth BAM do not describe an index", -1);
  std::vector<uint8_t> bai(need);
  simu_bai_build((uint32_t)ref_len.size(), ref_len.data(), rows.data(), rows.size(), linear.data(), counts.data(), bai.data(), need, &bins, &chunks);
  BaiFile out;
  out.path = bam_path + ".bai";
  out.f = fopen(out.path.c_str(), "wb");
  if (!out.f) throw Error("Error: can not open the index file of the sorted truth BAM:\n" + out.path, -1);
  const bool ok = fwrite(bai.data(), 1, bai.size(), out.f) == bai.size();
  const bool closed = fclose(out.f) == 0;
  out.f = nullptr;
  if (!ok || !closed) throw Error("Error: short write to the index file of the sorted truth BAM", -1);
  out.whole = true;
  st.bai_bins += bins;
  st.bai_chunks += chunks;
  st.bai_bytes += bai.size();
}

void TruthSort::finish(FILE* bam) {
  if (!spool) return;
  struct Dropper { TruthSort& s; ~Dropper() { s.drop(); } } dropper{*this};
  const auto t0 = std::chrono::steady_clock::now();
  uint64_t budget = kSortTileBytes;
  if (const char* e = getenv("SIMU_SORT_TILE_BYTES")) budget = std::max<uint64_t>(1, strtoull(e, nullptr, 10));
  const uint64_t chunk = std::max(budget, kSortMinChunk);
  const uint32_t R = (uint32_t)runs.size();
  st.truth_sort_runs += R;
  st.truth_spool_bytes += spool_bytes;
  if (indexing) {
    Timed acc{st.t_bai};
    unlink((bam_path + ".bai").c_str());   // (an index of an earlier run does not outlive a failure of this one)
    const off_t at = ftello(bam);
    if (at < 0) throw Error("Error: can not tell where the truth BAM's records start", -1);
    file_at = (uint64_t)at;
    eng.check(sg_bamindex_begin(eng.ctx, (uint32_t)ref_len.size(), ref_len.data()), "sg_bamindex_begin");
  }
  if (R) {
    if (fflush(spool) != 0) throw Error("Error: short write to the spool file of the sorted truth BAM", -1);
    std::vector<std::vector<uint64_t>> prefix(R);
    std::vector<const uint64_t*> kp(R), pp(R);
    std::vector<uint64_t> n(R);
    for (uint32_t r = 0; r < R; r++) {
      const Run& run = runs[r];
      prefix[r].resize(run.keys.size() + 1);
      prefix[r][0] = 0;
      for (size_t i = 0; i < run.lens.size(); i++) prefix[r][i + 1] = prefix[r][i] + run.lens[i];
      kp[r] = run.keys.data();
      pp[r] = prefix[r].data();
      n[r] = run.keys.size();
    }
    const SortTiles T = sort_tiles(R, kp.data(), n.data(), pp.data(), budget);
    st.truth_sort_tiles += T.first.size();
    std::vector<uint64_t> a(R), b(R), part_bytes(R), part_n(R);
    std::vector<const void*> part_rec(R);
    std::vector<const uint64_t*> part_keys(R);
    std::vector<const uint32_t*> part_lens(R);
    for (uint32_t r = 0; r < R; r++) a[r] = 0;
    for (size_t t = 0; t < T.first.size(); t++) {
      uint64_t tile_bytes = 0;
      for (uint32_t r = 0; r < R; r++) {   // (tiles ascend, so a run's range starts where its last one ended)
        const Run& run = runs[r];
        b[r] = t + 1 < T.first.size() ? (uint64_t)(std::lower_bound(run.keys.begin() + (ptrdiff_t)a[r], run.keys.end(), T.first[t + 1]) - run.keys.begin())
                                      : run.keys.size();
        part_bytes[r] = prefix[r][b[r]] - prefix[r][a[r]];
        part_n[r] = b[r] - a[r];
        tile_bytes += part_bytes[r];
      }
      if (T.single[t]) {   // one key value: the merged order is the runs in order, nothing to sort
        for (uint32_t r = 0; r < R; r++) {
          uint64_t at = runs[r].at + prefix[r][a[r]], left = part_bytes[r], rec = a[r];
          while (left) {
            if (stage.size() >= chunk) flush_stage(bam);
            const uint64_t take = std::min<uint64_t>(left, chunk - stage.size());
            const size_t old = stage.size();
            stage.resize(old + take);
            read_spool(at, take, stage.data() + old);
            if (indexing) stage_from_run(runs[r], rec, take);
            at += take;
            left -= take;
          }
        }
      } else {
        flush_stage(bam);
        if (buf.size() < tile_bytes) buf.resize(tile_bytes);
        uint64_t at = 0;
        for (uint32_t r = 0; r < R; r++) {
          read_spool(runs[r].at + prefix[r][a[r]], part_bytes[r], buf.data() + at);
          part_rec[r] = buf.data() + at;
          part_keys[r] = runs[r].keys.data() + a[r];
          part_lens[r] = runs[r].lens.data() + a[r];
          at += part_bytes[r];
        }
        uint64_t ob = 0, gb = 0;
        eng.check(sg_bamsort_merge(eng.ctx, R, part_rec.data(), part_bytes.data(), part_keys.data(), part_lens.data(), part_n.data(), &ob, &gb),
                  "sg_bamsort_merge");
        if (ob != tile_bytes) throw Error("Error: a merged tile of the truth BAM has another size than its runs", -1);
        if (members.size() < gb) members.resize(gb);
        eng.check(sg_bamsort_fetch(eng.ctx, 1, 0, gb, members.data()), "sg_bamsort_fetch");
        if (indexing) {
          Timed acc{st.t_bai};
          uint64_t nc = 0, fv = 0;
          eng.check(sg_bamindex_add(eng.ctx, SG_BAMINDEX_MERGE, file_at, 0, nullptr, 0, &nc, &fv), "sg_bamindex_add");
          index_added(nc, fv);
        }
        put_members(bam, members.data(), gb);
        file_at += gb;
      }
      a = b;
    }
    flush_stage(bam);
  }
  if (indexing) write_index();
  st.t_truth_sort += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace simu
