// tools/sort_tiles_fuzz.cpp -- simu_sort_tiles (host/truth_sort_tiles.cpp: how --truth-sort cuts a stem's key space into
// tiles) over seeded random run sets, for a sanitizer build on the CPU (tools/sort_tiles_sanitized.sh).  Every run set goes
// through simu_sort_tiles and through a brute-force cut written here -- all records in one sorted list, grouped by key
// value, cut greedily -- and the two must agree; the arrays handed over are exactly as long as the contract says, so a
// read or write past them is the sanitizer's to find.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "../simuscop_amd/csrc/host/simulate.h"

namespace {

struct Tile { uint64_t first; bool single; };

std::vector<Tile> brute(const std::vector<std::vector<uint64_t>>& keys, const std::vector<std::vector<uint32_t>>& lens, uint64_t budget) {
  std::map<uint64_t, uint64_t> per_key;
  for (size_t r = 0; r < keys.size(); r++)
    for (size_t i = 0; i < keys[r].size(); i++) per_key[keys[r][i]] += lens[r][i];
  std::vector<Tile> out;
  bool open = false;
  uint64_t first = 0, bytes = 0;
  for (const auto& kv : per_key) {
    if (kv.second > budget) {
      if (open) out.push_back({first, false});
      out.push_back({kv.first, true});
      open = false;
    } else if (!open) {
      open = true; first = kv.first; bytes = kv.second;
    } else if (bytes + kv.second <= budget) {
      bytes += kv.second;
    } else {
      out.push_back({first, false});
      first = kv.first; bytes = kv.second;
    }
  }
  if (open) out.push_back({first, false});
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 3000;
  std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 12345);
  uint64_t tiles_seen = 0, singles = 0;
  for (int it = 0; it < rounds; it++) {
    const uint32_t R = (uint32_t)(rng() % 6);
    const uint64_t spans[4] = {1, 8, 1000, UINT64_MAX};
    const uint64_t span = spans[rng() % 4];
    const uint64_t bases[3] = {0, 1ull << 32, UINT64_MAX - span};
    const uint64_t base = span == UINT64_MAX ? 0 : bases[rng() % 3];
    std::vector<std::vector<uint64_t>> keys(R), prefix(R);
    std::vector<std::vector<uint32_t>> lens(R);
    uint64_t total = 0;
    for (uint32_t r = 0; r < R; r++) {
      const uint32_t counts[5] = {0, 1, 2, 7, 40};
      const uint32_t n = counts[rng() % 5];
      for (uint32_t i = 0; i < n; i++) keys[r].push_back(span == UINT64_MAX ? rng() : base + rng() % (span + 1));
      if (n && rng() % 5 == 0) keys[r].back() = UINT64_MAX;
      std::sort(keys[r].begin(), keys[r].end());
      prefix[r].push_back(0);
      for (uint32_t i = 0; i < n; i++) {
        lens[r].push_back((uint32_t)(1 + rng() % 399));
        prefix[r].push_back(prefix[r].back() + lens[r].back());
      }
      total += prefix[r].back();
      keys[r].shrink_to_fit();
      prefix[r].shrink_to_fit();
    }
    const uint64_t budgets[8] = {1, 50, 399, 400, 1000, std::max<uint64_t>(1, total / 3), std::max<uint64_t>(1, total - 1), total + 1};
    const uint64_t budget = budgets[rng() % 8];
    std::vector<const uint64_t*> kp(R), pp(R);
    std::vector<uint64_t> n(R);
    for (uint32_t r = 0; r < R; r++) { kp[r] = keys[r].data(); pp[r] = prefix[r].data(); n[r] = keys[r].size(); }
    const std::vector<Tile> want = brute(keys, lens, budget);
    const uint64_t t = simu_sort_tiles(R, kp.data(), n.data(), pp.data(), budget, nullptr, nullptr, 0);
    if (t != want.size()) { printf("round %d: %llu tiles, the brute-force cut has %zu\n", it, (unsigned long long)t, want.size()); return 1; }
    std::vector<uint64_t> first(t);        // exactly t entries each
    std::vector<uint8_t> single(t);
    if (simu_sort_tiles(R, kp.data(), n.data(), pp.data(), budget, first.data(), single.data(), t) != t) { printf("round %d: the second call differs\n", it); return 1; }
    for (uint64_t i = 0; i < t; i++)
      if (first[i] != want[i].first || (single[i] != 0) != want[i].single) {
        printf("round %d tile %llu: (%llu, %d), the brute-force cut has (%llu, %d)\n", it, (unsigned long long)i, (unsigned long long)first[i], single[i],
               (unsigned long long)want[i].first, (int)want[i].single);
        return 1;
      }
    if (t > 1) {   // a short array takes only what fits
      std::vector<uint64_t> some(t - 1);
      if (simu_sort_tiles(R, kp.data(), n.data(), pp.data(), budget, some.data(), nullptr, t - 1) != t) { printf("round %d: a short array changes the count\n", it); return 1; }
    }
    tiles_seen += t;
    for (uint64_t i = 0; i < t; i++) singles += single[i];
  }
  printf("%d run sets, %llu tiles (%llu of one heavy key): all as the brute-force cut has them\n", rounds, (unsigned long long)tiles_seen,
         (unsigned long long)singles);
  return 0;
}
