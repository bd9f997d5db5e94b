// host/batch_cut.h -- the two cuts of a (population, chromosome) batch, as pure functions over the planned fragment slots
// of its active segments: the run of segments a rank of a sharded run samples, and the next memory-bounded piece of a run.
// No engine, no driver state (tools/driver_check.cpp checks both against a brute-force restatement).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace simu {

// shard by runs of segments (multi-GPU): contiguous, balanced by planned fragments.  false: nothing for this rank
inline bool shard_cut(const std::vector<uint64_t>& slots, int world, int rank, size_t& a0, size_t& a1) {
  a0 = 0; a1 = slots.size();
  if (world <= 1) return true;
  uint64_t slot = 0;
  for (uint64_t s : slots) slot += s;
  const uint64_t per = (slot + world - 1) / world;
  uint64_t acc = 0;
  a0 = a1 = slots.size();
  bool started = false;
  for (size_t i = 0; i < slots.size(); i++) {
    const int owner = per ? (int)std::min<uint64_t>(acc / per, (uint64_t)world - 1) : 0;
    if (owner == rank) { if (!started) { a0 = i; started = true; } a1 = i + 1; }
    acc += slots[i];
  }
  return started;
}

// the end of the piece that starts at segment c0 of the run [.., a1): whole segments, at least one, at most piece_slots slots
inline size_t piece_end(const std::vector<uint64_t>& slots, size_t c0, size_t a1, uint64_t piece_slots) {
  size_t c1 = c0;
  uint64_t acc = 0;
  while (c1 < a1 && (c1 == c0 || acc + slots[c1] <= piece_slots)) acc += slots[c1++];
  return c1;
}

}  // namespace simu
