// host/truth_errors.cpp -- the text of a --truth-errors file (truth_errors.h).
#include "truth_errors.h"

#include <cstdio>
#include <cstring>

namespace simu {

std::string errors_format(const uint64_t* table, uint32_t cycles, uint32_t qual_lo, uint32_t n_qual, uint32_t tmpl_len, uint32_t mates,
                          uint64_t* rows) {
  std::string out;
  uint64_t n = 0;
  char buf[160];
  auto u = [](uint64_t v) { return (unsigned long long)v; };
  const uint64_t* Q = table;
  const uint64_t* S = Q + 8ull * cycles * n_qual;
  const uint64_t* I = S + 40;
  const uint64_t* D = I + 4ull * tmpl_len;
  out += "#Q\tmate\tcycle\tqual\tbases\terrors\tother\tinserted\n";
  for (uint32_t m = 0; m < mates; m++)
    for (uint32_t c = 0; c < cycles; c++)
      for (uint32_t q = 0; q < n_qual; q++) {
        const uint64_t* cell = Q + (((uint64_t)m * cycles + c) * n_qual + q) * 4;
        if (!(cell[0] | cell[1] | cell[2] | cell[3])) continue;
        snprintf(buf, sizeof buf, "Q\t%u\t%u\t%u\t%llu\t%llu\t%llu\t%llu\n", m + 1, c + 1, qual_lo + q, u(cell[0]), u(cell[1]), u(cell[2]), u(cell[3]));
        out += buf;
        n++;
      }
  out += "#S\tmate\tfrom\tto\tcount\n";
  static const uint32_t kFrom[4] = {0, 1, 3, 2}, kTo[5] = {0, 1, 3, 2, 4};   // the file's A C G T (N) as the table's codes A0 C1 T2 G3 (N4)
  static const char kLetter[] = "ACGTN";
  for (uint32_t m = 0; m < mates; m++)
    for (uint32_t f = 0; f < 4; f++)
      for (uint32_t t = 0; t < 5; t++) {
        snprintf(buf, sizeof buf, "S\t%u\t%c\t%c\t%llu\n", m + 1, kLetter[f], kLetter[t], u(S[m * 20 + kFrom[f] * 5 + kTo[t]]));
        out += buf;
        n++;
      }
  for (int del = 0; del < 2; del++) {
    out += del ? "#D\tmate\tindex\tevents\tbases\n" : "#I\tmate\tindex\tevents\tbases\n";
    const uint64_t* T = del ? D : I;
    for (uint32_t m = 0; m < mates; m++)
      for (uint32_t j = 0; j < tmpl_len; j++) {
        const uint64_t* row = T + ((uint64_t)m * tmpl_len + j) * 2;
        if (!row[0]) continue;
        snprintf(buf, sizeof buf, "%c\t%u\t%u\t%llu\t%llu\n", del ? 'D' : 'I', m + 1, j + 1, u(row[0]), u(row[1]));
        out += buf;
        n++;
      }
  }
  if (rows) *rows = n;
  return out;
}

}  // namespace simu

extern "C" uint64_t simu_errors_format(const uint64_t* table, uint64_t cells, uint32_t cycles, uint32_t qual_lo, uint32_t n_qual, uint32_t tmpl_len,
                                       uint32_t mates, char* out, uint64_t cap, uint64_t* rows) {
  if (!table || mates < 1 || mates > 2 || cells != 8ull * cycles * n_qual + 40 + 8ull * tmpl_len) return UINT64_MAX;
  const std::string text = simu::errors_format(table, cycles, qual_lo, n_qual, tmpl_len, mates, rows);
  if (out && text.size() <= cap) memcpy(out, text.data(), text.size());
  return text.size();
}
