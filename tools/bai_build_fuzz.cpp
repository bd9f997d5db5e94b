// tools/bai_build_fuzz.cpp -- simu_bai_build (host/truth_index.cpp: the bytes of a --truth-index file) over seeded random
// tables, for a sanitizer build on the CPU (tools/bai_build_sanitized.sh).  Every case is a sorted list of records cut
// into calls; it goes through simu_bai_build as the driver hands it over -- per-call chunk rows grouped by key, open ends
// closed, linear cells, counts -- and through a plain serialiser written here that walks the records once, and the two
// must agree byte for byte.  The arrays handed over are exactly as long as the contract says, so a read or write past
// them is the sanitizer's to find.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "../include/simuscop_amd.h"
#include "../simuscop_amd/csrc/host/simulate.h"

namespace {

constexpr uint64_t kOpen = ~0ull;

struct Rec { int32_t ref; uint32_t beg, stop, bin; bool unm; uint64_t voff, end; };

uint32_t reg2bin(uint32_t beg, uint32_t end) {
  --end;
  if (beg >> 14 == end >> 14) return 4681 + (beg >> 14);
  if (beg >> 17 == end >> 17) return 585 + (beg >> 17);
  if (beg >> 20 == end >> 20) return 73 + (beg >> 20);
  if (beg >> 23 == end >> 23) return 9 + (beg >> 23);
  if (beg >> 26 == end >> 26) return 1 + (beg >> 26);
  return 0;
}

void put(std::vector<uint8_t>& o, uint64_t v, int n) { for (int i = 0; i < n; i++) o.push_back((uint8_t)(v >> (8 * i))); }

// the file from the records alone
std::vector<uint8_t> plain(const std::vector<Rec>& recs, const std::vector<uint64_t>& ref_len) {
  std::vector<uint8_t> o = {'B', 'A', 'I', 1};
  put(o, ref_len.size(), 4);
  uint64_t no_coor = 0;
  for (const Rec& r : recs) no_coor += r.ref < 0;
  for (size_t ref = 0; ref < ref_len.size(); ref++) {
    std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins;
    std::vector<uint64_t> lin;
    uint64_t n_map = 0, n_unm = 0, first = kOpen, last = 0;
    int64_t prev = -1;
    for (size_t i = 0; i < recs.size(); i++) {
      const Rec& r = recs[i];
      if (r.ref != (int32_t)ref) { prev = -1; continue; }
      if (prev == (int64_t)r.bin) bins[r.bin].back().second = r.end;
      else bins[r.bin].push_back({r.voff, r.end});
      prev = r.bin;
      (r.unm ? n_unm : n_map)++;
      first = std::min(first, r.voff);
      last = r.end;
      const uint32_t w1 = (r.stop - 1) >> 14;
      if (lin.size() < w1 + 1) lin.resize(w1 + 1, kOpen);
      for (uint32_t w = r.beg >> 14; w <= w1; w++) lin[w] = std::min(lin[w], r.voff);
    }
    put(o, bins.size() + (n_map + n_unm ? 1 : 0), 4);
    for (const auto& b : bins) {
      put(o, b.first, 4);
      put(o, b.second.size(), 4);
      for (const auto& c : b.second) { put(o, c.first, 8); put(o, c.second, 8); }
    }
    if (n_map + n_unm) { put(o, 37450, 4); put(o, 2, 4); put(o, first, 8); put(o, last, 8); put(o, n_map, 8); put(o, n_unm, 8); }
    for (size_t w = lin.size(); w-- > 1;)
      if (lin[w - 1] == kOpen) lin[w - 1] = lin[w];
    put(o, lin.size(), 4);
    for (uint64_t v : lin) put(o, v, 8);
  }
  put(o, no_coor, 8);
  return o;
}

}  // namespace

int main(int argc, char** argv) {
  const int cases = argc > 1 ? atoi(argv[1]) : 2000;
  std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 12345);
  auto pick = [&](uint64_t n) { return (uint64_t)(rng() % n); };
  uint64_t joined = 0, total_chunks = 0;
  for (int c = 0; c < cases; c++) {
    static const uint64_t lens[] = {1, 16384, 16385, 100000, 1ull << 22};
    std::vector<uint64_t> ref_len(1 + pick(4));
    for (uint64_t& l : ref_len) l = lens[pick(5)];
    static const int counts_of[] = {0, 1, 2, 5, 30, 200};
    std::vector<Rec> recs(counts_of[pick(6)]);
    for (Rec& r : recs) {
      r.ref = (int32_t)pick(ref_len.size() + 1) - 1;
      r.unm = pick(7) == 0;
      if (r.ref < 0) { r.beg = 0xFFFFFFFFu; r.stop = 0; r.bin = 0; continue; }
      r.beg = (uint32_t)pick(ref_len[r.ref]);
      if (pick(2)) r.beg = std::min<uint32_t>(r.beg, (uint32_t)pick(40000));
      static const uint32_t spans[] = {1, 2, 100, 16384, 50000};
      r.stop = r.unm ? r.beg + 1 : (uint32_t)std::min<uint64_t>(ref_len[r.ref], (uint64_t)r.beg + spans[pick(5)]);
      r.bin = reg2bin(r.beg, r.stop);
    }
    std::stable_sort(recs.begin(), recs.end(), [](const Rec& a, const Rec& b) {
      return ((uint64_t)(uint32_t)a.ref << 32 | a.beg) < ((uint64_t)(uint32_t)b.ref << 32 | b.beg);
    });
    uint64_t v = 5ull << 16;
    for (Rec& r : recs) { r.voff = v; v += (1 + pick(70000)) << (pick(3) == 0 ? 16 : 0); }
    const uint64_t eof = v + (1ull << 16);
    for (size_t i = 0; i < recs.size(); i++) recs[i].end = i + 1 < recs.size() ? recs[i + 1].voff : eof;
    // the calls, and what the device and the driver make of them
    std::vector<size_t> cuts = {0, recs.size()};
    for (uint64_t k = pick(9); k-- > 0;) cuts.push_back(pick(recs.size() + 1));
    std::sort(cuts.begin(), cuts.end());
    std::vector<sg_bai_chunk> rows;
    for (size_t k = 0; k + 1 < cuts.size(); k++) {
      std::vector<sg_bai_chunk> call;
      uint64_t prev = kOpen;
      for (size_t i = cuts[k]; i < cuts[k + 1]; i++) {
        const Rec& r = recs[i];
        const uint64_t key = r.ref < 0 ? kOpen : (uint64_t)r.ref << 32 | r.bin;
        if (key != kOpen && key == prev) call.back().end = r.end;
        else if (key != kOpen) call.push_back(sg_bai_chunk{key, r.voff, r.end});
        prev = key;
      }
      std::stable_sort(call.begin(), call.end(), [](const sg_bai_chunk& a, const sg_bai_chunk& b) { return a.key < b.key; });
      rows.insert(rows.end(), call.begin(), call.end());
    }
    uint64_t n_win = 0;
    std::vector<uint64_t> win_first;
    for (uint64_t l : ref_len) { win_first.push_back(n_win); n_win += (l + 16383) >> 14; }
    std::vector<uint64_t> linear(n_win, kOpen), counts(3 * ref_len.size() + 1, 0);
    for (size_t r = 0; r < ref_len.size(); r++) counts[3 * r + 2] = kOpen;
    for (const Rec& r : recs) {
      if (r.ref < 0) { counts[3 * ref_len.size()]++; continue; }
      counts[3 * r.ref + (r.unm ? 1 : 0)]++;
      counts[3 * r.ref + 2] = std::min(counts[3 * r.ref + 2], r.voff);
      for (uint32_t w = r.beg >> 14; w <= (r.stop - 1) >> 14; w++) linear[win_first[r.ref] + w] = std::min(linear[win_first[r.ref] + w], r.voff);
    }
    uint64_t bins = 0, chunks = 0;
    const uint64_t need = simu_bai_build((uint32_t)ref_len.size(), ref_len.data(), rows.empty() ? nullptr : rows.data(), rows.size(),
                                         linear.empty() ? nullptr : linear.data(), counts.data(), nullptr, 0, &bins, &chunks);
    const std::vector<uint8_t> want = plain(recs, ref_len);
    if (need != want.size()) { fprintf(stderr, "case %d: %llu bytes, the plain serialiser has %zu\n", c, (unsigned long long)need, want.size()); return 1; }
    std::vector<uint8_t> got(need);
    simu_bai_build((uint32_t)ref_len.size(), ref_len.data(), rows.empty() ? nullptr : rows.data(), rows.size(), linear.empty() ? nullptr : linear.data(),
                   counts.data(), got.data(), need, &bins, &chunks);
    if (got != want) { fprintf(stderr, "case %d: the bytes differ\n", c); return 1; }
    if (need > 1) {   // a buffer one byte short is left alone
      std::vector<uint8_t> small(need - 1, 0xAB);
      simu_bai_build((uint32_t)ref_len.size(), ref_len.data(), rows.empty() ? nullptr : rows.data(), rows.size(), linear.empty() ? nullptr : linear.data(),
                     counts.data(), small.data(), need - 1, nullptr, nullptr);
      for (uint8_t b : small) if (b != 0xAB) { fprintf(stderr, "case %d: wrote into a buffer that is too small\n", c); return 1; }
    }
    joined += rows.size() > chunks;
    total_chunks += chunks;
  }
  printf("%d cases, %llu chunks, %llu cases with joined chunks: all as the plain serialiser has them\n", cases, (unsigned long long)total_chunks,
         (unsigned long long)joined);
  return joined ? 0 : 1;
}
