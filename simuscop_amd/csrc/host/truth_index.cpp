// host/truth_index.cpp -- simu_bai_build: the bytes of a --truth-index file from what the device left (simulate.h; the
// index: csrc/sg_bamindex.h).  Pure host code: the joins, the ordering and the right-fill.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../../include/simuscop_amd.h"
#include "simulate.h"

namespace {

struct Out {
  std::vector<uint8_t> b;
  void u32(uint32_t v) { for (int i = 0; i < 4; i++) b.push_back((uint8_t)(v >> (8 * i))); }
  void u64(uint64_t v) { for (int i = 0; i < 8; i++) b.push_back((uint8_t)(v >> (8 * i))); }
};

}  // namespace

extern "C" uint64_t simu_bai_build(uint32_t n_ref, const uint64_t* ref_len, const void* rows_in, uint64_t n_rows, const uint64_t* linear,
                                   const uint64_t* counts, void* out, uint64_t cap, uint64_t* bins, uint64_t* chunks) {
  if (bins) *bins = 0;
  if (chunks) *chunks = 0;
  if ((n_ref && !ref_len) || (n_rows && !rows_in) || !counts) return UINT64_MAX;
  std::vector<sg_bai_chunk> rows(n_rows);
  if (n_rows) memcpy(rows.data(), rows_in, n_rows * sizeof(sg_bai_chunk));
  for (const sg_bai_chunk& c : rows)
    if ((c.key >> 32) >= n_ref || (uint32_t)c.key >= 37450u || c.end == ~0ull || c.beg == ~0ull) return UINT64_MAX;
  // all calls' rows by (refID, bin); within a bin they stay in call order, which is file order
  std::stable_sort(rows.begin(), rows.end(), [](const sg_bai_chunk& a, const sg_bai_chunk& b) { return a.key < b.key; });
  Out o;
  o.b.insert(o.b.end(), {'B', 'A', 'I', 1});
  o.u32(n_ref);
  uint64_t n_bins = 0, n_chunks = 0, win_first = 0;
  size_t i = 0;
  std::vector<sg_bai_chunk> joined;
  for (uint32_t r = 0; r < n_ref; r++) {
    joined.clear();
    uint64_t last_end = 0, ref_bins = 0;
    for (; i < rows.size() && (rows[i].key >> 32) == r; i++) {
      last_end = std::max(last_end, rows[i].end);
      if (!joined.empty() && joined.back().key == rows[i].key && joined.back().end == rows[i].beg) {
        joined.back().end = rows[i].end;   // a run that crossed a call boundary
        continue;
      }
      if (joined.empty() || joined.back().key != rows[i].key) ref_bins++;
      joined.push_back(rows[i]);
    }
    const uint64_t n_map = counts[(size_t)3 * r], n_unm = counts[(size_t)3 * r + 1], first = counts[(size_t)3 * r + 2];
    const bool has = n_map + n_unm != 0;
    if (has != !joined.empty() || (has && first == ~0ull)) return UINT64_MAX;
    o.u32((uint32_t)ref_bins + (has ? 1u : 0u));
    for (size_t a = 0; a < joined.size();) {
      size_t b = a;
      while (b < joined.size() && joined[b].key == joined[a].key) b++;
      o.u32((uint32_t)joined[a].key);
      o.u32((uint32_t)(b - a));
      for (; a < b; a++) { o.u64(joined[a].beg); o.u64(joined[a].end); }
    }
    if (has) {
      o.u32(37450u);
      o.u32(2);
      o.u64(first); o.u64(last_end);
      o.u64(n_map); o.u64(n_unm);
    }
    n_bins += ref_bins;
    n_chunks += joined.size();
    // linear index: up to the last window touched; an untouched window takes the next touched one's value
    const uint64_t n_win = (ref_len[r] + 16383) >> 14;
    if (n_win && !linear) return UINT64_MAX;
    uint64_t n_intv = n_win;
    while (n_intv && linear[win_first + n_intv - 1] == ~0ull) n_intv--;
    if (has != (n_intv != 0)) return UINT64_MAX;
    o.u32((uint32_t)n_intv);
    const size_t at = o.b.size();
    o.b.resize(at + n_intv * 8);
    uint64_t right = 0;
    for (uint64_t k = n_intv; k-- > 0;) {
      const uint64_t v = linear[win_first + k];
      if (v != ~0ull) right = v;
      for (int j = 0; j < 8; j++) o.b[at + k * 8 + j] = (uint8_t)(right >> (8 * j));
    }
    win_first += n_win;
  }
  if (i != rows.size()) return UINT64_MAX;
  o.u64(counts[(size_t)3 * n_ref]);
  if (bins) *bins = n_bins;
  if (chunks) *chunks = n_chunks;
  if (out && o.b.size() <= cap) memcpy(out, o.b.data(), o.b.size());
  return o.b.size();
}
