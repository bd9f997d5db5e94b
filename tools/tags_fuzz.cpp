// tools/tags_fuzz.cpp -- the host statement of the truth tags' rule (sg_truth_tags, sg_api_truth_tags.cpp; the walks:
// truth_tags_walk and truth_xe, sg_truth.h) over seeded random records, for a sanitizer build on the CPU
// (tools/tags_sanitized.sh).  Every record goes through sg_truth_tags and through a base-by-base walk written here; NM,
// the MD text (kept or dropped against a random cap) and XE must agree.  The MD buffer is allocated with exactly the
// cap's bytes, so a byte written past the cap is a finding of the sanitizer.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../include/simuscop_amd.h"

namespace {

char letter_of(uint8_t code) { return code < 4 ? "ACTG"[code] : 'N'; }

// XE base by base: the template in read direction, the events in turn; -1: the events do not give the read's length
long naive_xe(const std::vector<uint8_t>& codes, bool rev, const std::vector<uint32_t>& ev, const std::string& read) {
  const uint32_t L = (uint32_t)codes.size(), np = (uint32_t)read.size();
  uint32_t j = 0, r = 0;
  size_t e = 0;
  long xe = 0;
  while (j < L) {
    const bool at = e < ev.size() && (ev[e] & 0xFFFFu) == j;
    const uint32_t k = at ? (ev[e] >> 16) & 0x7FFFu : 0u;
    if (at && (ev[e] >> 31)) {
      const uint32_t kc = k < L - j ? k : L - j;
      xe += kc;
      j += kc;
      e++;
      continue;
    }
    if (r >= np) return -1;
    uint32_t t = codes[rev ? L - 1 - j : j];
    if (rev && t < 4u) t ^= 2u;
    if (t < 4u && read[r] != "ACTG"[t]) xe++;
    r++;
    if (at) {
      if (r + k > np) return -1;
      xe += k;
      r += k;
      e++;
    }
    j++;
  }
  return e == ev.size() && r == np ? xe : -1;
}

}  // namespace

int main(int argc, char** argv) {
  const int n_records = argc > 1 ? atoi(argv[1]) : 20000;
  std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 12345);
  auto pick = [&](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (hi - lo + 1)); };
  long kept = 0, dropped = 0, unmapped = 0, with_xe = 0;
  for (int it = 0; it < n_records; it++) {
    // ---- NM / MD: random operations, SEQ that mostly follows the reference ----
    std::vector<uint32_t> ops;
    std::string seq, md;
    std::vector<uint8_t> ref;
    uint32_t nm = 0, m = 0;
    const uint32_t n_runs = rng() % 12 == 0 ? 0u : pick(1, 9);
    uint32_t last = 99;
    for (uint32_t k = 0; k < n_runs; k++) {
      uint32_t op = k == 0 || k + 1 == n_runs ? (rng() % 4 == 0 ? 4u : 0u) : (uint32_t)(rng() % 3 ? 0u : pick(1, 3));
      if (n_runs == 1) op = 0;
      if (op == last) op = op == 0 ? 1u : 0u;
      last = op;
      const uint32_t len = op == 2 && rng() % 6 == 0 ? pick(30, 300) : op == 3 ? pick(1, 5000) : pick(1, 70);
      ops.push_back((len << 4) | op);
      if (op == 0) {
        for (uint32_t i = 0; i < len; i++) {
          const uint8_t code = (uint8_t)(rng() % 30 == 0 ? pick(4, 6) : pick(0, 3));
          const char s = rng() % 12 == 0 ? "ACGTN"[rng() % 5] : letter_of(code);
          ref.push_back(code);
          seq.push_back(s);
          if (code < 4 && s == letter_of(code)) { m++; continue; }
          md += std::to_string(m) + letter_of(code);
          m = 0;
          nm++;
        }
      } else if (op == 2) {
        md += std::to_string(m) + "^";
        m = 0;
        for (uint32_t i = 0; i < len; i++) {
          ref.push_back((uint8_t)(rng() % 30 == 0 ? pick(4, 6) : pick(0, 3)));
          md.push_back(letter_of(ref.back()));
        }
        nm += len;
      } else if (op == 3) {
        for (uint32_t i = 0; i < len; i++) ref.push_back((uint8_t)pick(0, 6));
      } else {
        for (uint32_t i = 0; i < len; i++) seq.push_back("ACGTN"[rng() % 5]);
        if (op == 1) nm += len;
      }
    }
    md += std::to_string(m);
    // the cap: mostly near the text's length, so that both sides of it are met
    const uint32_t cap = n_runs ? (rng() % 2 ? (uint32_t)md.size() + pick(0, 2) - 1u : pick(0, 400)) : pick(0, 8);
    // ---- XE: a template, events that give the read's length (or, one time in five, no template) ----
    const bool inside = rng() % 5 != 0;
    const bool rev = rng() & 1;
    std::vector<uint8_t> tmpl;
    std::vector<uint32_t> ev;
    std::string read;
    if (inside) {
      const uint32_t L = pick(20, 300);
      tmpl.resize(L);
      for (auto& c : tmpl) c = (uint8_t)(rng() % 30 == 0 ? pick(4, 6) : pick(0, 3));
      uint32_t j = pick(0, L / 4), n_ev = rng() % 2 ? pick(0, 8) : 0, np = 0, jj = 0;
      while (ev.size() < n_ev && j < L) {
        const uint32_t del = (uint32_t)(rng() & 1), k = pick(1, 12);
        ev.push_back(j | (k << 16) | (del << 31));
        const uint32_t kc = k < L - j ? k : L - j;
        np += j - jj + (del ? 0 : 1 + k);
        jj = del ? j + kc : j + 1;
        j = jj + pick(0, L / (n_ev + 1));
      }
      np += L - jj;
      read.assign(np, 'A');
      for (auto& c : read) c = "ACGTN"[rng() % 5];
    }
    std::vector<char> buf(cap);   // exactly the cap's bytes
    uint32_t present = 0, g_nm = 0, g_len = 0, g_xe = 0;
    const int rc = sg_truth_tags(ops.data(), (uint32_t)ops.size(), seq.data(), (uint32_t)seq.size(), ref.data(), ref.size(), cap,
                                 inside ? tmpl.data() : nullptr, (uint32_t)tmpl.size(), rev, ev.data(), (uint32_t)ev.size(), read.data(),
                                 (uint32_t)read.size(), &present, &g_nm, buf.data(), &g_len, &g_xe);
    const long w_xe = inside ? naive_xe(tmpl, rev, ev, read) : 0;
    const bool w_md = n_runs && md.size() <= cap;
    uint32_t want = (n_runs ? SG_TAG_NM : 0u) | (w_md ? SG_TAG_MD : 0u) | (inside ? SG_TAG_XE : 0u);
    bool ok = rc == SG_OK && present == want && w_xe >= 0;
    if (ok && n_runs) ok = g_nm == nm;
    if (ok && w_md) ok = g_len == md.size() && std::string(buf.data(), g_len) == md;
    if (ok && inside) ok = g_xe == (uint32_t)w_xe;
    if (!ok) {
      fprintf(stderr, "record %d: rc %d, tags %u (want %u), NM %u (%u), MD %u bytes (%zu, cap %u), XE %u (%ld)\n", it, rc, present, want, g_nm, nm,
              g_len, md.size(), cap, g_xe, w_xe);
      return 1;
    }
    if (!n_runs) unmapped++;
    else (w_md ? kept : dropped)++;
    with_xe += inside;
  }
  printf("tags_fuzz: %ld MD texts kept, %ld dropped, %ld unmapped records, %ld with XE, all as the base-by-base walk has them\n", kept, dropped,
         unmapped, with_xe);
  return kept > 0 && dropped > 0 && unmapped > 0 && with_xe > 0 ? 0 : 1;
}
