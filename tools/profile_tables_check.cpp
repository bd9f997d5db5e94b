// profile_tables_check.cpp -- (CPU only) what sg_profile_prepare makes of a list of profiles, one line per case: the
// case's name, the number of table words, a 64-bit FNV-1a over them and every field of the layout (SgTableLayout,
// sg_profile_tables.h); of a refused profile the code and the message.  tests/test_profile_tables_cpu.py compares the
// lines with tests/profile_tables_expected.txt.
//
//   g++ -O2 -std=c++17 -ffp-contract=off tools/profile_tables_check.cpp simuscop_amd/csrc/sg_profile_tables.cpp
//       simuscop_amd/csrc/sg_tables.cpp simuscop_amd/csrc/host/profile.cpp -o profile_tables_check
//   profile_tables_check tests/golden/testData
//
// The shipped profiles are read by the driver's loader (host/profile.cpp).  The synthetic ones come from a seeded
// integer generator: every CDF entry is one division of two integers below 2^53, so the doubles are the same wherever
// IEEE arithmetic is.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../simuscop_amd/csrc/host/profile.h"
#include "../simuscop_amd/csrc/sg_profile_tables.h"

namespace {

void report(const char* name, const sg_profile_cdf* pr) {
  sg_profile_tables* T = nullptr;
  const int rc = sg_profile_prepare(pr, &T);
  if (rc != SG_OK) {
    printf("%s rc=%d err=\"%s\"\n", name, rc, sg_profile_tables_error(T));
    sg_profile_tables_free(T);
    return;
  }
  uint64_t h = 0xcbf29ce484222325ull;
  for (uint32_t w : T->tab)
    for (int b = 0; b < 4; b++) { h ^= (w >> (8 * b)) & 0xFFu; h *= 0x100000001b3ull; }
  const SgTableLayout& L = T->L;
  printf("%s words=%llu fnv=%016llx", name, (unsigned long long)T->tab.size(), (unsigned long long)h);
  printf(" sub_off=%llu sub_rows=%llu alias_off=%llu ins_off=%llu del_off=%llu isz_off=%llu gap_off=%llu", (unsigned long long)L.sub_off,
         (unsigned long long)L.sub_rows, (unsigned long long)L.alias_off, (unsigned long long)L.ins_off, (unsigned long long)L.del_off,
         (unsigned long long)L.isz_off, (unsigned long long)L.gap_off);
  printf(" fast_lds_off=%llu fast_sub_off=%llu fast_alias_off=%llu", (unsigned long long)L.fast_lds_off, (unsigned long long)L.fast_sub_off,
         (unsigned long long)L.fast_alias_off);
  printf(" lgW=%u ins_lg=%u del_lg=%u isz_lg=%u fast_stride=%u remap=%02x inv_remap=%02x packed=%08x", L.lgW, L.ins_lg, L.del_lg, L.isz_lg,
         L.fast_stride, L.remap, L.inv_remap, L.packed);
  printf(" kmer_off=");
  for (int m = 0; m < 8; m++) printf("%s%u", m ? "," : "", L.kmer_off[m]);
  printf(" evA=%016llx evB=%016llx has2=%d has_isz=%d", (unsigned long long)L.evA, (unsigned long long)L.evB, (int)L.has2, (int)L.has_isz);
  printf(" kmer=%d bins=%d read_length=%d min_qual=%d isize_min=%d insert_size=%d n_isize=%d\n", L.kmer, L.bins, L.read_length, L.min_qual,
         L.isize_min, L.insert_size, L.n_isize);
  sg_profile_tables_free(T);
}

struct Rng {   // xorshift64*
  uint64_t s;
  uint32_t next() {
    s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
    return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32);
  }
};

struct Shape {
  const char* name;
  int kmer, bins;
  bool has2;
  const char* bases;
  int n_qual;
  bool all_mass;     // every quality symbol carries mass (else about one in three does)
  int lead_zero;     // leading entries of every row without mass
  double insert_rate, del_rate;
  bool has_isz;
  int read_length;
};

// a CDF row of n entries from integer masses: the first `lead_zero` none, the others `all` ? 1..2^20 : none in two of three
void cdf_row(Rng& g, double* row, int n, int lead_zero, bool all) {
  std::vector<uint64_t> m((size_t)n, 0);
  uint64_t total = 0;
  for (int k = 0; k < n; k++) {
    const uint32_t x = g.next();
    if (k >= lead_zero && (all || x % 3 == 0)) m[k] = 1 + (x >> 12);
    total += m[k];
  }
  if (!total) total = m[n - 1] = 1 + (g.next() >> 12);
  uint64_t cum = 0;
  for (int k = 0; k < n; k++) { cum += m[k]; row[k] = (double)cum / (double)total; }
}

struct Synth {
  std::vector<double> subs1, subs2, qual, ins, del, isz;
  sg_profile_cdf v;
  explicit Synth(const Shape& s, uint64_t seed) {
    Rng g{seed * 0x9E3779B97F4A7C15ull + 1};
    int contexts = 0;
    for (int m = 1, p = 1; m <= s.kmer; m++) { p *= 4; contexts += p; }
    const size_t rows = (size_t)contexts * s.bins;
    subs1.resize(rows * 4);
    for (size_t r = 0; r < rows; r++) cdf_row(g, &subs1[r * 4], 4, s.lead_zero ? (int)(r % 4) : 0, r % 5 != 0);
    if (s.has2) {
      subs2.resize(rows * 4);
      for (size_t r = 0; r < rows; r++) cdf_row(g, &subs2[r * 4], 4, s.lead_zero ? (int)((r + 1) % 4) : 0, r % 7 != 0);
    }
    const size_t qrows = (size_t)16 * s.bins;
    qual.resize(qrows * s.n_qual);
    for (size_t r = 0; r < qrows; r++) cdf_row(g, &qual[r * s.n_qual], s.n_qual, s.lead_zero < s.n_qual ? s.lead_zero : s.n_qual - 1, s.all_mass);
    ins.resize(5); del.resize(3);
    cdf_row(g, ins.data(), 5, s.lead_zero ? 2 : 0, true);
    cdf_row(g, del.data(), 3, s.lead_zero ? 1 : 0, true);
    if (s.has_isz) { isz.resize(37); cdf_row(g, isz.data(), 37, s.lead_zero, true); }
    memset(&v, 0, sizeof v);
    v.n_bases = 4;
    memcpy(v.bases, s.bases, 4);
    v.kmer = s.kmer; v.bins = s.bins; v.read_length = s.read_length; v.n_qual = s.n_qual; v.min_qual = 33;
    v.insert_rate = s.insert_rate; v.del_rate = s.del_rate;
    v.ins_cdf = ins.data(); v.n_ins = 5;
    v.del_cdf = del.data(); v.n_del = 3;
    v.subs_cdf1 = subs1.data();
    v.subs_cdf2 = s.has2 ? subs2.data() : nullptr;
    v.qual_cdf = qual.data();
    v.isize_cdf = s.has_isz ? isz.data() : nullptr;
    v.n_isize = s.has_isz ? 37 : 0;
    v.isize_min = s.read_length;
    v.insert_size = 350;
  }
};

const double R1 = 0.00011, R2 = 0.00023;   // (decimal literals: the compiler's conversion is exact to the nearest double)
const Shape kShapes[] = {
    // name              kmer bins has2   bases  n_qual all   lead  ins    del    isz    L
    {"synth_k1_b1",       1,  1, false, "ACTG",  41, false, 0,  R1,   R2,   false, 100},
    {"synth_k1_b7_two",   1,  7, true,  "GTCA",  41, false, 0,  R1,   R2,   true,  100},
    {"synth_k2_b1_two",   2,  1, true,  "ACTG",  41, false, 0,  R1,   R2,   false, 100},
    {"synth_k2_b7",       2,  7, false, "GTCA",  41, false, 0,  R1,   R2,   true,  100},
    {"synth_k3_b1",       3,  1, false, "ACTG",  41, false, 0,  R1,   R2,   true,  100},
    {"synth_k3_b7_two",   3,  7, true,  "ACTG",  41, false, 0,  R1,   R2,   true,  150},
    {"synth_k3_b7_gtca",  3,  7, true,  "GTCA",  41, false, 0,  R1,   R2,   false, 150},
    {"synth_k3_b1_gtca",  3,  1, false, "GTCA",  41, false, 0,  R1,   R2,   true,  100},
    {"synth_k4_b7",       4,  7, false, "ACTG",  41, false, 0,  R1,   R2,   false, 100},
    {"synth_k4_b1_two",   4,  1, true,  "GTCA",  41, false, 0,  R1,   R2,   true,  100},
    {"synth_k6_b1",       6,  1, false, "ACTG",  41, false, 0,  R1,   R2,   false, 100},
    {"synth_k6_b7_two",   6,  7, true,  "GTCA",  41, false, 0,  R1,   R2,   true,  100},
    {"synth_nq1",         3,  7, true,  "ACTG",   1, true,  0,  R1,   R2,   true,  100},
    {"synth_nq1_k2",      2,  1, false, "GTCA",   1, true,  0,  R1,   R2,   false, 100},
    {"synth_nq128_all",   3,  7, true,  "ACTG", 128, true,  0,  R1,   R2,   true,  100},
    {"synth_nq128_k1",    1,  1, false, "GTCA", 128, true,  0,  R1,   R2,   false, 100},
    {"synth_lead_zero",   3,  7, true,  "ACTG",  41, false, 3,  R1,   R2,   true,  100},
    {"synth_lead_zero_k2",2,  1, false, "GTCA",  41, true,  9,  R1,   R2,   true,  100},
    {"synth_rates_zero",  3,  7, true,  "ACTG",  41, false, 0,  0.0,  0.0,  true,  100},
    {"synth_rates_1e-9",  3,  7, true,  "ACTG",  41, false, 0,  1e-9, 1e-9, true,  100},
    {"synth_rates_ins0",  2,  7, false, "ACTG",  41, false, 0,  0.0,  1e-9, false, 100},
    {"synth_L1_b4",       3,  4, true,  "ACTG",  41, false, 0,  R1,   R2,   true,  1},
    {"synth_L1_b4_k1",    1,  4, false, "GTCA",  41, false, 0,  R1,   R2,   false, 1},
    {"synth_L30000_b4",   3,  4, true,  "ACTG",  41, false, 0,  R1,   R2,   true,  30000},
    {"synth_L30000_b4_k4",4,  4, false, "GTCA",  41, false, 0,  R1,   R2,   false, 30000},
};

// every refusal of the checks once (the alias columns' own refusal cannot be reached: the column count is chosen from the
// rows' symbols, and a row's masses always add up to 2^32)
void refusals() {
  const Shape ok = {"", 3, 7, true, "ACTG", 41, false, 0, R1, R2, true, 100};
  Synth base(ok, 99);
  report("refuse_null_profile", nullptr);
  printf("refuse_null_out rc=%d\n", sg_profile_prepare(&base.v, nullptr));
  auto with = [&](const char* name, void (*edit)(sg_profile_cdf&)) {
    sg_profile_cdf v = base.v;
    edit(v);
    report(name, &v);
  };
  with("refuse_n_bases", [](sg_profile_cdf& v) { v.n_bases = 5; });
  with("refuse_kmer_0", [](sg_profile_cdf& v) { v.kmer = 0; });
  with("refuse_kmer_7", [](sg_profile_cdf& v) { v.kmer = 7; });
  with("refuse_bins_0", [](sg_profile_cdf& v) { v.bins = 0; });
  with("refuse_read_length_0", [](sg_profile_cdf& v) { v.read_length = 0; });
  with("refuse_read_length_30001", [](sg_profile_cdf& v) { v.read_length = 30001; });
  with("refuse_bin_arithmetic", [](sg_profile_cdf& v) { v.read_length = 30000; v.bins = 5; });
  with("refuse_bin_arithmetic_n_ins", [](sg_profile_cdf& v) { v.n_ins = 2045; });
  with("refuse_n_qual_0", [](sg_profile_cdf& v) { v.n_qual = 0; });
  with("refuse_n_qual_129", [](sg_profile_cdf& v) { v.n_qual = 129; });
  with("refuse_no_subs", [](sg_profile_cdf& v) { v.subs_cdf1 = nullptr; });
  with("refuse_no_qual", [](sg_profile_cdf& v) { v.qual_cdf = nullptr; });
  with("refuse_no_ins", [](sg_profile_cdf& v) { v.ins_cdf = nullptr; });
  with("refuse_no_del", [](sg_profile_cdf& v) { v.del_cdf = nullptr; });
  with("refuse_n_ins_0", [](sg_profile_cdf& v) { v.n_ins = 0; });
  with("refuse_n_del_0", [](sg_profile_cdf& v) { v.n_del = 0; });
  with("refuse_bases_acgn", [](sg_profile_cdf& v) { memcpy(v.bases, "ACGN", 4); });
  with("refuse_bases_repeat", [](sg_profile_cdf& v) { memcpy(v.bases, "AATG", 4); });
  with("refuse_insert_rate_negative", [](sg_profile_cdf& v) { v.insert_rate = -0.5; });
  with("refuse_insert_rate_half", [](sg_profile_cdf& v) { v.insert_rate = 0.5; });
  with("refuse_del_rate_half", [](sg_profile_cdf& v) { v.insert_rate = 0.25; v.del_rate = 0.375; });
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s <directory of the shipped profiles>\n", argv[0]); return 2; }
  static const char* const shipped[] = {"Illumina_GenomeAnalyzerIIx", "Illumina_HiSeq2000", "Illumina_HiSeq2500", "Illumina_HiSeqXTen"};
  try {
    for (const char* name : shipped)
      for (int paired = 1; paired >= 0; paired--) {
        simu::Profile p;
        p.train(std::string(argv[1]) + "/" + name + ".profile", paired != 0, 350);
        const sg_profile_cdf v = p.view();
        report((std::string(name) + (paired ? "_pe350" : "_se")).c_str(), &v);
      }
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  uint64_t seed = 1;
  for (const Shape& s : kShapes) {
    Synth y(s, seed++);
    report(s.name, &y.v);
  }
  refusals();
  return 0;
}
