// tools/errtab_fuzz.cpp -- the host statement of the true error counts' rule (sg_errtab_observe, sg_api_errors.cpp; the
// walk: errtab_walk, sg_truth.h) over seeded random reads, for a sanitizer build on the CPU (tools/errtab_sanitized.sh).
// Every read goes through sg_errtab_observe and through a base-by-base walk written here; the two tables must agree.
// A third of the reads is damaged (events out of order or outside the template, a wrong length, a quality byte out of
// range, more events than a pass keeps): those must be refused and must add nothing.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../include/simuscop_amd.h"

namespace {

struct Dims { uint32_t cycles, qual_lo, n_qual, L; };
uint64_t cells_of(const Dims& d) { return 8ull * d.cycles * d.n_qual + 40 + 8ull * d.L; }

// the rule, base by base as the issue states it; false: refused
bool naive(const Dims& d, const std::vector<uint8_t>& codes, bool rev, const std::vector<uint32_t>& ev, const std::string& bases,
           const std::string& quals, uint32_t mate, std::vector<uint64_t>& tab) {
  const uint32_t L = d.L, np = (uint32_t)bases.size();
  if (ev.size() > SG_MAX_EVENTS || np > d.cycles) return false;
  for (unsigned char q : quals)
    if (q < 33u + d.qual_lo || q - 33u - d.qual_lo >= d.n_qual) return false;
  std::vector<uint64_t> add(tab.size(), 0);
  auto tq = [&](uint32_t r, uint32_t col) -> uint64_t& { return add[(((uint64_t)mate * d.cycles + r) * d.n_qual + ((unsigned char)quals[r] - 33u - d.qual_lo)) * 4 + col]; };
  const uint64_t s0 = 8ull * d.cycles * d.n_qual, i0 = s0 + 40, d0 = i0 + 4ull * L;
  uint32_t j = 0, r = 0;
  size_t e = 0;
  while (j < L) {
    const bool at = e < ev.size() && (ev[e] & 0xFFFFu) == j;
    const uint32_t k = at ? (ev[e] >> 16) & 0x7FFFu : 0u;
    if (at && k == 0u) return false;
    if (at && (ev[e] >> 31)) {
      const uint32_t kc = k < L - j ? k : L - j;
      add[d0 + ((uint64_t)mate * L + j) * 2] += 1;
      add[d0 + ((uint64_t)mate * L + j) * 2 + 1] += kc;
      j += kc;
      e++;
      continue;
    }
    if (r >= np) return false;
    uint32_t t = codes[rev ? L - 1 - j : j];
    if (rev && t < 4u) t ^= 2u;
    if (t < 4u) {
      const char c = bases[r];
      const uint32_t to = c == 'A' ? 0u : c == 'C' ? 1u : c == 'T' ? 2u : c == 'G' ? 3u : 4u;
      tq(r, 0)++;
      if (to != t) tq(r, 1)++;
      add[s0 + mate * 20 + t * 5 + to]++;
    } else {
      tq(r, 2)++;
    }
    r++;
    if (at) {
      if (r + k > np) return false;
      for (uint32_t i = 0; i < k; i++) tq(r + i, 3)++;
      add[i0 + ((uint64_t)mate * L + j) * 2] += 1;
      add[i0 + ((uint64_t)mate * L + j) * 2 + 1] += k;
      r += k;
      e++;
    }
    j++;
  }
  if (e != ev.size() || r != np) return false;
  for (size_t i = 0; i < tab.size(); i++) tab[i] += add[i];
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  const int n_reads = argc > 1 ? atoi(argv[1]) : 20000;
  std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 12345);
  auto pick = [&](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (hi - lo + 1)); };
  long accepted = 0, refused = 0;
  for (int it = 0; it < n_reads; it++) {
    Dims d;
    d.L = pick(50, 700);
    d.cycles = d.L + pick(0, 160);
    d.qual_lo = pick(0, 5);
    d.n_qual = pick(21, 60);
    std::vector<uint8_t> codes(d.L);
    for (auto& c : codes) c = (uint8_t)(rng() % 40 == 0 ? pick(4, 6) : pick(0, 3));
    const bool rev = rng() & 1;
    const uint32_t mate = (uint32_t)(rng() & 1);
    std::vector<uint32_t> ev;
    uint32_t j = pick(0, d.L / 8), n_ev = rng() % 3 ? pick(0, 32) : 0, np = 0, jj = 0;
    while (ev.size() < n_ev && j < d.L) {
      const uint32_t del = (uint32_t)(rng() & 1), k = rng() % 10 ? pick(1, 5) : pick(6, 40);
      ev.push_back(j | (k << 16) | (del << 31));
      const uint32_t kc = k < d.L - j ? k : d.L - j;
      np += j - jj + (del ? 0 : 1 + k);
      jj = del ? j + kc : j + 1;
      j = jj + pick(0, 2 * d.L / (n_ev + 1));
    }
    np += d.L - jj;
    const int damage = (int)(rng() % 3 == 0 ? pick(1, 6) : 0);
    if (damage == 1 && ev.size() >= 2) std::swap(ev[0], ev[ev.size() - 1]);
    if (damage == 2) ev.push_back(pick(d.L, 0xFFFF) | (1u << 16));
    if (damage == 3) np += pick(1, 3);
    if (damage == 4) while (ev.size() <= SG_MAX_EVENTS) ev.push_back((uint32_t)ev.size() | (1u << 16));
    if (damage == 5 && !ev.empty()) ev[ev.size() / 2] &= 0x8000FFFFu;   // an event of no length
    std::string bases(np, 'A'), quals(np, '!');
    for (auto& c : bases) c = "ACGTN"[rng() % 40 == 0 ? 4 : rng() % 4];
    for (auto& q : quals) q = (char)(33 + d.qual_lo + pick(0, d.n_qual - 1));
    if (damage == 6 && np) quals[rng() % np] = (char)(rng() & 1 ? 33 + d.qual_lo + d.n_qual : 32 + d.qual_lo);
    std::vector<uint64_t> got(cells_of(d), 0), want(cells_of(d), 0);
    const int rc = sg_errtab_observe(codes.data(), d.L, rev, ev.data(), (uint32_t)ev.size(), bases.data(), quals.data(), np, mate, d.cycles, d.qual_lo,
                                     d.n_qual, got.data(), got.size());
    const bool ok = naive(d, codes, rev, ev, bases, quals, mate, want);
    if (ok != (rc == SG_OK) || got != want) {
      fprintf(stderr, "read %d: the engine says %d, the base-by-base walk %s, tables %s (L %u, %zu events, %u bases, damage %d)\n", it, rc,
              ok ? "counts" : "refuses", got == want ? "equal" : "differ", d.L, ev.size(), np, damage);
      return 1;
    }
    (ok ? accepted : refused)++;
  }
  printf("errtab_fuzz: %ld reads counted, %ld refused, all as the base-by-base walk has them\n", accepted, refused);
  return accepted > 0 && refused > 0 ? 0 : 1;
}
