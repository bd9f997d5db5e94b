// tools/vcf_row_fuzz.cpp -- sg::vcf_decide (csrc/sg_vcf.h: the verdict on one fragment of a VCF, the code the device
// kernel runs) over seeded random fragments, for a sanitizer build on the CPU (tools/vcf_row_sanitized.sh).  Every
// fragment goes through vcf_decide and through the parser's loop body as lib/vcfparser/vcfparser.cpp:26-106 has it,
// written here with fgets' NUL-terminated buffer, atoi, atof and atol; a verdict other than "undecided" must be the
// parser's.  The fragment is handed over in a heap block of exactly its length, so a read past it is the sanitizer's to
// find.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../simuscop_amd/csrc/sg_vcf.h"

namespace {

const char* kKeys[] = {"1", "20", "X", "2"};

std::string abbr(std::string chr) {
  size_t i = chr.find("chrom");
  if (i == std::string::npos) {
    i = chr.find("chr");
    if (i != std::string::npos) chr = chr.substr(i + 3);
  } else {
    chr = chr.substr(i + 5);
  }
  return chr;
}

// the parser on one fragment
void parser(const std::string& frag, sg_vcf_record* R) {
  memset(R, 0, sizeof *R);
  std::vector<char> buf(frag.begin(), frag.end());
  buf.push_back('\0');
  if (buf[0] == '#') return;
  char* f[10];
  int nf = 0;
  char* p = buf.data();
  f[nf++] = p;
  while (*p && nf < 10) {
    if (*p == '\t') { *p = '\0'; f[nf++] = p + 1; }
    p++;
  }
  if (nf < 10) { R->kind = SG_VCF_MALFORMED; return; }
  const std::string info = f[7];
  const size_t dp = info.find("DP=");
  if (dp != std::string::npos) {
    const size_t semi = info.find(";", dp);
    if (atoi(info.substr(dp + 3, semi - dp - 3).c_str()) < 10) return;
  }
  if ((float)atof(f[5]) < 20.0f) return;
  const std::string chr = abbr(f[0]);
  const long pos = atol(f[1]);
  std::string gt = f[9];
  gt = gt.substr(0, gt.find(':'));
  for (uint32_t c = 0; c < 4; c++)
    if (chr == kKeys[c]) { R->contig = c; R->flags |= SG_VCF_KNOWN; break; }
  const size_t ref_len = strlen(f[3]), alt_len = strlen(f[4]);
  if (ref_len > 1) { R->kind = SG_VCF_DEL; R->pos = pos + 1; R->value = (int32_t)ref_len - 1; }
  else if (alt_len > 1) { R->kind = SG_VCF_INS; R->pos = pos; R->value = (int32_t)alt_len - 1; }
  else { R->kind = SG_VCF_SNV; R->pos = pos; R->value = (int32_t)f[4][0]; if (gt != "1/1") R->flags |= SG_VCF_HOMO; }
}

template <class Rng>
std::string pick(Rng& g, std::initializer_list<const char*> l) { return *(l.begin() + g() % l.size()); }

template <class Rng>
std::string fragment(Rng& g) {
  const uint32_t r = g() % 100;
  if (r < 3) return "#" + std::string(g() % 40, 'x') + "\n";
  if (r < 5) return "\n";
  if (r < 10) {   // bytes of every value, NUL included
    std::string s(1 + g() % 200, ' ');
    for (char& c : s) c = (char)(g() % 256);
    return s;
  }
  std::string pos = std::to_string(g() % 1000000000);
  if (g() % 20 == 0) pos = pick(g, {"", "-7", "+8", " 9", "12x", "1234567890123456789", "999999999999999999"});
  std::string qual = pick(g, {"50", "19.9", "20", "19.999999", "19.9999999", "19.9999990463256", "19.9999990463257", ".", "", "-0", "1e3", "inf", "NAN",
                              "0x1p5", " 30", "5.e1", "20.", ".5", "+20.000", "0000000000000050", "19.99999904632568359375", "PASS", "30p", "3E", "1e-400"});
  if (g() % 4 == 0) { qual = std::to_string(g() % 40) + "." + std::to_string(g() % 100000000); }
  const std::string info = pick(g, {"DP=30", "DP=9", "DP=10", "AF=0.5;DP=25;MQ=60", "ADP=3;DP=50", "DP=", ".", "AF=1", "DP=+11", "DP=-1", "DP= 30",
                                    "DP=3000000000", "DP=0000000030", "DP=12x;DP=1", "D", "DP", "DP=;"});
  const std::string chrom = pick(g, {"chr1", "1", "chr20", "20", "chrom20", "chrX", "chr9", "", "chr", "chro", "xchrom2", "200"});
  const std::string ref = pick(g, {"A", "C", "", "ACG", "N"}), alt = pick(g, {"A", "T", "", "AT", "ACGT", "<DEL>", "\xc3"});
  const std::string gt = pick(g, {"0/1:3,4", "1/1:9", "1/1", "1/1\n", "1|1", "1/1\t0/1", "", ":", "1/"});
  std::string s = chrom + "\t" + pos + "\t.\t" + ref + "\t" + alt + "\t" + qual + "\tPASS\t" + info + "\tGT\t" + gt;
  if (g() % 3) s += "\n";
  if (g() % 10 == 0) s = s.substr(0, g() % (s.size() + 1));   // cut anywhere: fewer fields
  if (g() % 50 == 0) s += std::string(sg::kVcfFragment - s.size(), 'q');   // the longest fragment
  return s.empty() ? "\n" : s;
}

}  // namespace

int main(int argc, char** argv) {
  const long cases = argc > 1 ? atol(argv[1]) : 20000;
  std::mt19937_64 g(argc > 2 ? strtoull(argv[2], nullptr, 10) : 12345);
  std::vector<char> keys(4 * sg::kVcfKeyBytes, 0);
  for (int c = 0; c < 4; c++) strcpy(&keys[c * sg::kVcfKeyBytes], kKeys[c]);
  long undecided = 0, rows = 0;
  for (long i = 0; i < cases; i++) {
    const std::string s = fragment(g);
    char* block = (char*)malloc(s.size());   // exactly the fragment
    memcpy(block, s.data(), s.size());
    sg_vcf_record got, want;
    memset(&got, 0, sizeof got);
    const uint32_t kind = sg::vcf_decide(block, (uint32_t)s.size(), keys.data(), 4, &got);
    free(block);
    parser(s, &want);
    if (kind == SG_VCF_UNDECIDED) { undecided++; continue; }
    rows += kind >= SG_VCF_SNV && kind <= SG_VCF_DEL;
    if (got.kind != want.kind || got.pos != want.pos || got.contig != want.contig || got.value != want.value || got.flags != want.flags) {
      printf("case %ld differs: kind %u / %u pos %lld / %lld contig %u / %u value %d / %d flags %u / %u\n", i, got.kind, want.kind, (long long)got.pos,
             (long long)want.pos, got.contig, want.contig, got.value, want.value, got.flags, want.flags);
      fwrite(s.data(), 1, s.size() < 300 ? s.size() : 300, stdout);
      printf("\n");
      return 1;
    }
  }
  printf("%ld fragments, %ld rows, %ld undecided: all as the parser has them\n", cases, rows, undecided);
  return 0;
}
