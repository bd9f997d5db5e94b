// host/truth_sort_tiles.cpp -- simu_sort_tiles: how --truth-sort cuts a stem's key space into tiles (truth_sort.h).  Pure
// host code with no engine in it, in a file of its own so that tools/sort_tiles_sanitized.sh can build it alone.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "simulate.h"

namespace {

struct Runs {
  uint32_t n_runs;
  const uint64_t* const* keys;
  const uint64_t* n;
  const uint64_t* const* prefix;
  // index of the first record of run r with key >= K
  uint64_t lower(uint32_t r, uint64_t K) const { return (uint64_t)(std::lower_bound(keys[r], keys[r] + n[r], K) - keys[r]); }
  // bytes(key < K) = sum over the runs of prefix_r[lower_bound(keys_r, K)]: monotone in K
  uint64_t bytes_below(uint64_t K) const {
    uint64_t b = 0;
    for (uint32_t r = 0; r < n_runs; r++) b += prefix[r][lower(r, K)];
    return b;
  }
  // the smallest key >= K that a run holds; false: none
  bool next_key(uint64_t K, uint64_t* out) const {
    bool any = false;
    for (uint32_t r = 0; r < n_runs; r++) {
      const uint64_t i = lower(r, K);
      if (i < n[r] && (!any || keys[r][i] < *out)) { *out = keys[r][i]; any = true; }
    }
    return any;
  }
};

}  // namespace

extern "C" uint64_t simu_sort_tiles(uint32_t n_runs, const uint64_t* const* keys, const uint64_t* n, const uint64_t* const* prefix, uint64_t budget,
                                    uint64_t* splitters, uint8_t* single, uint64_t cap) {
  if (n_runs && (!keys || !n || !prefix)) return UINT64_MAX;
  const Runs R{n_runs, keys, n, prefix};
  uint64_t total = 0, tiles = 0;
  for (uint32_t r = 0; r < n_runs; r++) {
    if (n[r] && (!keys[r] || !prefix[r])) return UINT64_MAX;
    if (n[r]) total += prefix[r][n[r]];
  }
  auto emit = [&](uint64_t first, bool is_single) {
    if (tiles < cap) {
      if (splitters) splitters[tiles] = first;
      if (single) single[tiles] = is_single ? 1 : 0;
    }
    tiles++;
  };
  uint64_t from = 0, first = 0;
  bool more = R.next_key(from, &first);
  while (more) {
    const uint64_t base = R.bytes_below(first);
    if (total - base <= budget) {   // all that is left fits
      emit(first, false);
      break;
    }
    if (first == UINT64_MAX) {   // the largest key alone is left, and it is too heavy
      emit(first, true);
      break;
    }
    if (R.bytes_below(first + 1) - base > budget) {   // this key alone is too heavy: a tile of its own
      emit(first, true);
      from = first + 1;
    } else {   // the largest K in (first, 2^64 - 1] with bytes(first <= key < K) <= budget
      uint64_t lo = first + 1, hi = UINT64_MAX;   // lo holds, hi + 1 would be "everything", which does not fit
      for (uint64_t step = 1; lo <= UINT64_MAX - step; step = step > (UINT64_MAX >> 1) ? UINT64_MAX : step * 2) {   // (neighbours are near: gallop first)
        if (R.bytes_below(lo + step) - base <= budget) lo += step;
        else { hi = lo + step - 1; break; }
      }
      while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2 + 1;
        if (R.bytes_below(mid) - base <= budget) lo = mid;
        else hi = mid - 1;
      }
      emit(first, false);
      from = lo;
    }
    more = R.next_key(from, &first);
  }
  return tiles;
}
