// sg_vcf.h -- the VCF of known variants as the reference's parser reads it (lib/vcfparser/vcfparser.cpp:26-106, restated
// by parse_vcf in host/train.cpp), stated once for the device (sg_vcf.hip) and for the host (sg_vcf_row, sg_api_vcf.cpp).
//
// THE RULE
//   Fragments.  The unit is what one fgets(buf, 20000) returns: at most 19,999 bytes, or through the line break.  A line
//     of n bytes (its '\n' included, if it has one) is the fragments at offsets 0, 19999, 2 * 19999, ... below n.
//     Fragments are numbered from 1 across the whole file: the parser's line_num.  (The #CHROM line of a VCF with
//     thousands of samples is longer than 19,999 bytes; its tail is parsed as a data row.)
//   Per fragment:
//     first byte '#'   skipped
//     fields           split at tabs into ten; the tenth keeps the rest of the fragment, line break included.  Fewer than
//                      ten (an empty line is one field): malformed, counted, nothing else happens to it
//     INFO (field 8)   the first occurrence of "DP=" anywhere in the field ("ADP=" matches); its value is atoi of the text
//                      behind it up to the next ';' or the field's end; a value below 10: skipped
//     QUAL (field 6)   (float)atof(QUAL) < 20.0f: skipped ("." is skipped)
//     contig           abbr_of_chr(CHROM) -- what follows the first "chrom", else the first "chr", else the name -- looked
//                      up among the contig keys
//     position         atol(POS)
//     genotype         field 10 up to its first ':' or its end; heterozygous iff exactly the three bytes "1/1" ("1/1\n",
//                      or "1/1\t..." of a multi-sample row without ':', is not); everything else is homozygous
//     kind             strlen(REF) > 1: deletion (pos + 1, strlen(REF) - 1); else strlen(ALT) > 1: insertion (pos,
//                      strlen(ALT) - 1); else SNV (pos, first byte of ALT -- 0 when ALT is empty --, the homo flag)
//     counts           n_snv / n_ins / n_del count every such row; a row is KEPT only when its contig is known
//     order            kept rows of each kind stay in file order
//   Decided here, exactly:
//     POS   [+-]? and at most 18 digits (no digit: 0)
//     DP    [+-]? and at most 9 digits (no digit: 0)
//     QUAL  [+-]?digits[.digits] or [+-]?.digits with at most 15 digits in all, not followed by an exponent or a hex
//           marker; or a first byte that starts no number (value 0).  The parser's verdict on such a text equals
//           value < 20 - 2^-20 in exact decimal arithmetic: the float nearest below 20 is 20 - 2^-19, the tie at
//           20 - 2^-20 = 19.99999904632568359375 goes to 20.0f, and a decimal of at most 15 digits is never within a
//           double's rounding distance of that number.  With 13 fractional digits that is one integer compare.
//   UNDECIDED (handed back to the host, which runs the parser's own per-fragment code on the bytes): a letter that may
//     begin an exponent, "inf", "nan" or a hex form where QUAL's number ends or would begin; longer digit strings; white
//     space in front of a numeric field; a NUL byte inside the fragment.  The fields are looked at in the parser's order,
//     so a fragment that DP has already skipped is not undecided for its QUAL.
#pragma once
#include <stdint.h>

#include "../../include/simuscop_amd.h"

#if defined(__HIPCC__)
#define SG_VCF_HD __host__ __device__
#else
#define SG_VCF_HD
#endif

namespace sg {

constexpr uint32_t kVcfFragment = 19999;   // fgets(buf, 20000)
constexpr uint32_t kVcfKeyBytes = 64;      // contig key slots (NUL terminated), as sg_train's
constexpr uint64_t kVcfQualCut = 199999990463256ull;   // floor((20 - 2^-20) * 10^13): QUAL * 10^13 at or below it is below 20.0f

SG_VCF_HD inline bool vcf_digit(char c) { return c >= '0' && c <= '9'; }
SG_VCF_HD inline bool vcf_space(char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }   // isspace in the C locale

// atoi / atol on [b, e): false when the text is not of a decided form.  max_digits 9 (atoi) or 18 (atol).
SG_VCF_HD inline bool vcf_int(const char* t, uint32_t b, uint32_t e, uint32_t max_digits, long long* out) {
  if (b < e && vcf_space(t[b])) return false;
  bool neg = false;
  if (b < e && (t[b] == '-' || t[b] == '+')) { neg = t[b] == '-'; b++; }
  long long v = 0;
  uint32_t n = 0;
  while (b < e && vcf_digit(t[b])) {
    if (++n > max_digits) return false;
    v = v * 10 + (t[b] - '0');
    b++;
  }
  *out = neg ? -v : v;
  return true;
}

// (float)atof([b, e)) < 20.0f: 1 below, 0 not below, -1 undecided
SG_VCF_HD inline int vcf_qual_below(const char* t, uint32_t b, uint32_t e) {
  if (b < e && vcf_space(t[b])) return -1;
  bool neg = false;
  if (b < e && (t[b] == '-' || t[b] == '+')) { neg = t[b] == '-'; b++; }
  uint64_t ip = 0, fp = 0;
  uint32_t nd = 0, nfrac = 0;
  const uint32_t b0 = b;
  while (b < e && vcf_digit(t[b])) {
    if (++nd > 15) return -1;
    ip = ip * 10 + (uint64_t)(t[b] - '0');
    b++;
  }
  if (b < e && t[b] == '.' && (nd > 0 || (b + 1 < e && vcf_digit(t[b + 1])))) {
    b++;
    while (b < e && vcf_digit(t[b])) {
      if (++nd > 15) return -1;
      if (nfrac < 13) { fp = fp * 10 + (uint64_t)(t[b] - '0'); nfrac++; }
      b++;
    }
  }
  if (b < e) {   // what may go on as an exponent or a hex form, or begin "inf" / "nan"
    const char c = t[b] | 0x20;
    if (b == b0 ? (c == 'i' || c == 'n') : (c == 'e' || c == 'x' || c == 'p')) return -1;
  }
  if (nd == 0 || neg) return 1;   // no number: 0; a negative number or -0
  if (ip != 19) return ip < 19 ? 1 : 0;
  // 19.f...: the integer part took two of the fifteen digits, so at most thirteen are fractional
  for (; nfrac < 13; nfrac++) fp *= 10;
  return 190000000000000ull + fp <= kVcfQualCut ? 1 : 0;
}

// One fragment [t, t + n), n in 1..19999.  keys: n_keys slots of kVcfKeyBytes.  Fills R (but its fragment number) and
// returns its kind.
SG_VCF_HD inline uint32_t vcf_decide(const char* t, uint32_t n, const char* keys, uint32_t n_keys, sg_vcf_record* R) {
  R->pos = 0; R->contig = 0; R->value = 0; R->kind = SG_VCF_SKIP; R->flags = 0;
  if (t[0] == '#') return SG_VCF_SKIP;
  // the nine tabs that end fields 1-9; a NUL anywhere ends the parser's string early: not decided here
  uint32_t e0 = 0, e1 = 0, e2 = 0, e3 = 0, e4 = 0, e5 = 0, e6 = 0, e7 = 0, e8 = 0, tabs = 0;
  bool nul = false;
  for (uint32_t i = 0; i < n; i++) {
    const char c = t[i];
    if (c == '\0') nul = true;
    if (c == '\t' && tabs < 9) {
      switch (tabs) {
        case 0: e0 = i; break;
        case 1: e1 = i; break;
        case 2: e2 = i; break;
        case 3: e3 = i; break;
        case 4: e4 = i; break;
        case 5: e5 = i; break;
        case 6: e6 = i; break;
        case 7: e7 = i; break;
        default: e8 = i; break;
      }
      tabs++;
    }
  }
  if (nul) { R->kind = SG_VCF_UNDECIDED; return SG_VCF_UNDECIDED; }
  if (tabs < 9) { R->kind = SG_VCF_MALFORMED; return SG_VCF_MALFORMED; }
  // INFO: the first "DP=" and its value
  for (uint32_t i = e6 + 1; i + 3 <= e7; i++) {
    if (t[i] == 'D' && t[i + 1] == 'P' && t[i + 2] == '=') {
      uint32_t s = i + 3;
      while (s < e7 && t[s] != ';') s++;
      long long dp = 0;
      if (!vcf_int(t, i + 3, s, 9, &dp)) { R->kind = SG_VCF_UNDECIDED; return SG_VCF_UNDECIDED; }
      if (dp < 10) return SG_VCF_SKIP;
      break;
    }
  }
  const int below = vcf_qual_below(t, e4 + 1, e5);
  if (below < 0) { R->kind = SG_VCF_UNDECIDED; return SG_VCF_UNDECIDED; }
  if (below) return SG_VCF_SKIP;
  long long pos = 0;
  if (!vcf_int(t, e0 + 1, e1, 18, &pos)) { R->kind = SG_VCF_UNDECIDED; return SG_VCF_UNDECIDED; }
  // abbr_of_chr, then the key
  uint32_t cb = 0;
  bool cut = false;
  for (uint32_t q = 0; q + 5 <= e0 && !cut; q++)
    if (t[q] == 'c' && t[q + 1] == 'h' && t[q + 2] == 'r' && t[q + 3] == 'o' && t[q + 4] == 'm') { cb = q + 5; cut = true; }
  for (uint32_t q = 0; q + 3 <= e0 && !cut; q++)
    if (t[q] == 'c' && t[q + 1] == 'h' && t[q + 2] == 'r') { cb = q + 3; cut = true; }
  for (uint32_t c = 0; c < n_keys; c++) {
    const char* key = keys + (uint64_t)c * kVcfKeyBytes;
    uint32_t i = 0;
    while (cb + i < e0 && key[i] != 0 && key[i] == t[cb + i]) i++;
    if (cb + i == e0 && key[i] == 0) { R->contig = c; R->flags |= SG_VCF_KNOWN; break; }
  }
  // the genotype: field 10 up to its first ':' or the fragment's end
  const uint32_t g = e8 + 1;
  const bool het = n - g >= 3 && t[g] == '1' && t[g + 1] == '/' && t[g + 2] == '1' && (n - g == 3 || t[g + 3] == ':');
  const uint32_t ref_len = e3 - e2 - 1, alt_len = e4 - e3 - 1;
  if (ref_len > 1) { R->kind = SG_VCF_DEL; R->pos = pos + 1; R->value = (int32_t)ref_len - 1; }
  else if (alt_len > 1) { R->kind = SG_VCF_INS; R->pos = pos; R->value = (int32_t)alt_len - 1; }
  else {
    R->kind = SG_VCF_SNV; R->pos = pos; R->value = alt_len ? (int32_t)(signed char)t[e3 + 1] : 0;
    if (!het) R->flags |= SG_VCF_HOMO;
  }
  return R->kind;
}

// ---- the kernels of sg_vcf.hip ----
#if defined(__HIPCC__)
struct VcfJob {
  const char* text;          // [the line the call before left unfinished][this call's text]
  uint64_t bytes;
  uint32_t final_call;       // the file ends here: a last line without a line break is a line
  uint64_t first_number;     // fragments numbered before this call
  const char* keys;
  uint32_t n_keys;
  uint32_t n_blocks;         // 64-byte blocks of the text
  uint32_t* block_breaks;    // [n_blocks] line breaks per block
  uint64_t* block_first;     // their exclusive scan; info[0] = the total
  uint64_t* info;            // [0] line breaks [1] lines [2] where the unfinished line starts [3] fragments
                             // [4..8] rows kept as SNV / insertion / deletion, malformed, undecided  [9..11] n_snv / n_ins / n_del
                             // [12] the longest line above one fragment: its bytes << 32 | where it starts
  uint64_t* line_stop;       // [lines] one past the line's last byte
  uint32_t n_lines;
  uint32_t* frag_count;      // [lines]
  uint64_t* frag_first;      // their exclusive scan; info[3] = the total
  uint32_t n_frags;
  uint64_t* frag_start;      // [fragments]
  uint32_t* frag_len;
  sg_vcf_record* rows;       // [fragments] the verdicts
  uint32_t* flag[5];         // [fragments] 1 where the fragment goes to list k: kept SNV / insertion / deletion, malformed, undecided
  uint64_t* slot[5];         // their exclusive scans; info[4 + k] = the totals
  sg_vcf_record* out[3];     // the kept rows of the session, this call's from out_first[k] on
  uint64_t out_first[3];
  uint64_t* malformed;       // [info[7]] fragment numbers
  sg_vcf_fragment* undecided;   // [info[8]] number, where its bytes start in the text, how many
};
void launch_vcf_breaks(const VcfJob& J, hipStream_t s);      // block_breaks
void launch_vcf_lines(const VcfJob& J, hipStream_t s);       // line_stop, info[1..2] (behind the scan of block_breaks)
void launch_vcf_frag_count(const VcfJob& J, hipStream_t s);  // frag_count
void launch_vcf_rows(const VcfJob& J, hipStream_t s);        // frag_start / frag_len, rows, flag, info[9..11]
void launch_vcf_compact(const VcfJob& J, hipStream_t s);     // out, malformed, undecided (behind the scans of flag)
#endif

}  // namespace sg
