// sg_profile_tables.cpp -- see sg_profile_tables.h: sg_profile_prepare and the table self-check entry points of the C
// ABI.  Pure host arithmetic on top of sg_tables.cpp.
#include "sg_profile_tables.h"

#include <algorithm>
#include <cstring>
#include <stdexcept>

#include "sg_tables.h"

namespace {

void pad4(std::vector<uint32_t>& tab, uint32_t fill) { while (tab.size() % 4) tab.push_back(fill); }

// Substitution row, identity first (sg_tables.h): {D0, D1, D2, j0 | o0<<2 | o1<<4 | o2<<6 | o3<<8}, the outcomes o as
// `code` names them
template <class Code>
void pack_sub_row(uint32_t* o, const sg::SubRow& sr, Code code) {
  o[0] = sr.D[0]; o[1] = sr.D[1]; o[2] = sr.D[2];
  o[3] = sr.j0 | code(sr.order[0]) << 2 | code(sr.order[1]) << 4 | code(sr.order[2]) << 6 | code(sr.order[3]) << 8;
}

// Quality row as alias columns (sg_tables.h): W x {thr, lo | hi << 8}
void pack_alias_row(uint32_t* o, const sg::AliasRow& ar, uint32_t W) {
  for (uint32_t c = 0; c < W; c++) { o[2 * c] = ar.thr[c]; o[2 * c + 1] = (uint32_t)ar.lo[c] | (uint32_t)ar.hi[c] << 8; }
}

// The steps of sg_profile_prepare, in the order in which the words are laid down.  Each writes the layout's fields where
// it computes them.
struct Builder {
  const sg_profile_cdf& pr;
  sg_profile_tables& T;
  SgTableLayout& L = T.L;
  std::vector<uint32_t>& tab = T.tab;
  int n_mates = 1;
  std::vector<sg::SubRow> srows;     // [mate][context][bin]
  std::vector<sg::AliasRow> arows;   // [reference base][called base][bin], profile codes
  int checks(), alias_columns(), gap_row();
  void sub_rows(), length_rows(), fast_tables();
};

int Builder::checks() {
  if (pr.n_bases != 4) return T.fail(SG_ERR_UNSUPPORTED, "sg_load_profile: only 4-letter base alphabets are supported");
  if (pr.kmer < 1 || pr.kmer > 6) return T.fail(SG_ERR_UNSUPPORTED, "sg_load_profile: kmer must be in 1..6");
  if (pr.bins < 1 || pr.read_length < 1 || pr.read_length > 30000) return T.fail(SG_ERR_INVALID, "sg_load_profile: bad bins/read_length");
  // the kernels compute bin = i*bins/n' with a 32-bit reciprocal: exact while i*bins*n' < 2^32
  const uint64_t npmax = (uint64_t)pr.read_length + (uint64_t)SG_MAX_EVENTS * (uint64_t)(pr.n_ins > 0 ? pr.n_ins : 1);
  if (npmax > 0xFFFF || npmax * (uint64_t)pr.bins * npmax >= (1ull << 32))
    return T.fail(SG_ERR_UNSUPPORTED, "sg_load_profile: read_length * bins too large for the 32-bit bin arithmetic");
  if (pr.n_qual < 1 || pr.n_qual > 128) return T.fail(SG_ERR_INVALID, "sg_load_profile: n_qual must be in 1..128 (quality symbols are 7-bit fields)");
  if (!pr.subs_cdf1 || !pr.qual_cdf || !pr.ins_cdf || !pr.del_cdf || pr.n_ins < 1 || pr.n_del < 1)
    return T.fail(SG_ERR_INVALID, "sg_load_profile: missing table");
  // base alphabet must be a permutation of ACGT (the kernels classify haplotype bytes by value)
  const char nat[4] = {'A', 'C', 'T', 'G'};  // natural index = (byte >> 1) & 3
  for (int n = 0; n < 4; n++) {
    int code = -1;
    for (int k = 0; k < 4; k++) if (pr.bases[k] == nat[n]) code = k;
    if (code < 0) return T.fail(SG_ERR_UNSUPPORTED, "sg_load_profile: bases must be a permutation of ACGT");
    L.remap |= (uint32_t)code << (2 * n);
    L.inv_remap |= (uint32_t)n << (2 * code);
  }
  for (int k = 0; k < 4; k++) L.packed |= (uint32_t)(uint8_t)pr.bases[k] << (8 * k);
  L.kmer = pr.kmer; L.bins = pr.bins; L.read_length = pr.read_length; L.min_qual = pr.min_qual;
  L.isize_min = pr.isize_min; L.insert_size = pr.insert_size; L.n_isize = pr.n_isize;
  L.has2 = pr.subs_cdf2 != nullptr;
  L.has_isz = pr.isize_cdf != nullptr && pr.n_isize > 0;
  n_mates = L.has2 ? 2 : 1;
  // contexts with m real bases are numbered in base-4 counting order behind those with fewer (Profile::initKmers,
  // Profile.cpp:70-124)
  uint32_t off = 0, p4 = 1;
  for (int m = 1; m <= pr.kmer; m++) { L.kmer_off[m] = off; p4 *= 4; off += p4; }
  L.sub_rows = (uint64_t)off * pr.bins;
  return SG_OK;
}

void Builder::sub_rows() {
  L.sub_off = tab.size();
  srows.resize((size_t)n_mates * L.sub_rows);
  tab.resize(L.sub_off + srows.size() * 4);
  for (int t = 0; t < n_mates; t++) {
    const double* src = t == 0 ? pr.subs_cdf1 : pr.subs_cdf2;
    for (size_t r = 0; r < L.sub_rows; r++) {
      // the reference base a row is about is its context's last base, the lowest base-4 digit of the context id (every
      // kmer_off is a multiple of 4)
      const sg::SubRow& sr = srows[t * L.sub_rows + r] = sg::encode_sub_row_identity_first(src + r * 4, (int)(r / pr.bins & 3));
      pack_sub_row(&tab[L.sub_off + (t * L.sub_rows + r) * 4], sr, [](uint32_t prof) { return prof; });
    }
  }
}

int Builder::alias_columns() {
  const size_t qrows = (size_t)16 * pr.bins;
  std::vector<std::vector<uint64_t>> qmass(qrows);
  uint32_t most = 1;
  for (size_t r = 0; r < qrows; r++) {
    qmass[r] = sg::row_masses(pr.qual_cdf + r * pr.n_qual, pr.n_qual);
    most = std::max(most, sg::symbols_with_mass(qmass[r]));
  }
  L.lgW = std::max(2u, sg::log2_at_least(most));
  const uint32_t W = 1u << L.lgW;
  arows.resize(qrows);
  try {
    for (size_t r = 0; r < qrows; r++) arows[r] = sg::build_alias_row(qmass[r], L.lgW);
  } catch (const std::exception& e) {
    return T.fail(SG_ERR_INVALID, std::string("sg_load_profile: ") + e.what());
  }
  pad4(tab, 0);
  L.alias_off = tab.size();
  tab.resize(L.alias_off + qrows * W * 2);
  for (size_t r = 0; r < qrows; r++) pack_alias_row(&tab[L.alias_off + r * W * 2], arows[r], W);
  return SG_OK;
}

// the indel-length rows and the insert-size row: threshold rows of sg_tables.h, padded to a power of two
void Builder::length_rows() {
  auto add_row = [&](const double* cdf, int n, uint64_t& off, uint32_t& lg) {
    const sg::Row r = sg::encode_row(cdf, n);
    lg = sg::log2_at_least((uint32_t)r.T.size());
    pad4(tab, 0xFFFFFFFFu);
    off = tab.size();
    tab.resize(off + 1 + (1u << lg), 0xFFFFFFFFu);
    tab[off] = r.k0;
    std::copy(r.T.begin(), r.T.end(), tab.begin() + (long)off + 1);
  };
  add_row(pr.ins_cdf, pr.n_ins, L.ins_off, L.ins_lg);
  add_row(pr.del_cdf, pr.n_del, L.del_off, L.del_lg);
  if (L.has_isz) add_row(pr.isize_cdf, pr.n_isize, L.isz_off, L.isz_lg);
  pad4(tab, 0xFFFFFFFFu);
}

// Sequencing indels by skipping ahead: getIndelSeq tests every template position with `p <= insertRate`, then
// `p < delRate/(1-insertRate)`, p = x/2^32 (Profile.cpp:1560-1570).  cI, cD = the numbers of 32-bit draws that pass;
// a position is a candidate with probability evB / 2^64, evB = cI 2^32 + (2^32 - cI) cD, an insertion with evA / evB,
// evA = cI 2^32.  gap[k] = floor(gap[k-1] * gap[1] / 2^64), gap[1] = 2^64 - evB: P(no candidate in k positions).
int Builder::gap_row() {
  if (pr.insert_rate < 0) return T.fail(SG_ERR_INVALID, "sg_load_profile: negative insert rate");
  const uint64_t ci = sg::count_unit_le(pr.insert_rate);
  const uint64_t cd = sg::count_unit_lt(pr.del_rate / (1 - pr.insert_rate));
  if (ci >= (1ull << 31) || cd >= (1ull << 31)) return T.fail(SG_ERR_UNSUPPORTED, "sg_load_profile: sequencing indel rate >= 0.5");
  L.evA = ci << 32, L.evB = L.evA + ((1ull << 32) - ci) * cd;
  std::vector<uint64_t> gap((size_t)pr.read_length + 1, 0xFFFFFFFFFFFFFFFFull);
  if (L.evB) {
    gap[1] = 0ull - L.evB;
    for (size_t k = 1; k + 1 < gap.size(); k++) gap[k + 1] = (uint64_t)(((unsigned __int128)gap[k] * gap[1]) >> 64);
  }
  pad4(tab, 0);
  L.gap_off = tab.size();
  tab.resize(L.gap_off + 2 * gap.size());
  memcpy(&tab[L.gap_off], gap.data(), gap.size() * 8);
  pad4(tab, 0);
  return SG_OK;
}

// Straight-line kernel tables (kmer 3).  The kernel packs base codes 2 bits each in NATURAL order (A0 C1 T2 G3) with
// the OLDEST base of a context in the lowest digit; the reference numbers a context with its oldest base in the
// highest digit, in `bases` order (Profile::initKmers).  Context ids of the kernel: [0,4) one base, [4,20) two, [20,84)
// three.  Everything below is indexed by the kernel's ids and natural base codes.
void Builder::fast_tables() {
  const uint32_t W = 1u << L.lgW, remap = L.remap, inv_remap = L.inv_remap;
  const int bins = pr.bins;
  std::vector<uint32_t> perm;  // kernel context id -> reference context id
  for (int m = 1; m <= 3; m++)
    for (uint32_t v = 0; v < (1u << (2 * m)); v++) {
      uint32_t src = 0;
      for (int tt = 0; tt < m; tt++) {
        const uint32_t nat = (v >> (2 * tt)) & 3u;  // base at age position tt (0 = oldest)
        src |= ((remap >> (2 * nat)) & 3u) << (2 * (m - 1 - tt));
      }
      perm.push_back(L.kmer_off[m] + src);
    }
  auto nat_of = [&](uint32_t prof) { return (inv_remap >> (2u * prof)) & 3u; };
  auto prof_of = [&](uint32_t nat) { return (remap >> (2u * nat)) & 3u; };
  // Per bin the tables hold 192 context rows addressed by the 6-bit field kv = b[i-2] | b[i-1] << 2 | b[i] << 4 of the
  // packed codes: [0,64) the three-base contexts, [64,128) the two-base contexts (kv >> 2; a read's second base) and
  // [128,192) the one-base contexts (kv >> 4; a read's first base), so that every position uses the same extract.
  auto row_of = [&](int t, uint32_t slot, int b) -> const sg::SubRow& {
    const uint32_t kv = slot & 63u;
    const uint32_t ctx = slot < 64u ? perm[20u + kv] : slot < 128u ? perm[4u + (kv >> 2)] : perm[kv >> 4];
    return srows[t * L.sub_rows + (size_t)ctx * bins + b];
  };
  auto alias_of = [&](uint32_t cdn, uint32_t kn, int b) -> const sg::AliasRow& { return arows[((size_t)prof_of(cdn) * 4 + prof_of(kn)) * bins + b]; };
  L.fast_stride = 192u + 4u * W;
  pad4(tab, 0);
  // (1) the LDS image, per mate and bin: [0,192) keep_h - 1 of the context's row, keep_h = c0 >> 16 (a 16-bit head
  //     below keep_h is certainly "no substitution"); [192, 192 + 4W) the diagonal alias columns (reference base ==
  //     called base) in the order [col][natural base] as  col << (16 - lgW) | thr >> 16  in the low half (the draw's
  //     low half minus it is u_head - thr_head: the column bits cancel),  (lo ^ hi) << 16 | hi << 24  above, lo and hi as
  //     characters (symbol + the profile's lowest quality character)
  L.fast_lds_off = tab.size();
  tab.resize(L.fast_lds_off + (size_t)n_mates * bins * L.fast_stride);
  const uint32_t mq = (uint32_t)pr.min_qual;
  for (int t = 0; t < n_mates; t++)
    for (int b = 0; b < bins; b++) {
      uint32_t* blk = &tab[L.fast_lds_off + ((size_t)t * bins + b) * L.fast_stride];
      for (uint32_t sl = 0; sl < 192; sl++) blk[sl] = (uint32_t)(row_of(t, sl, b).c[0] >> 16) - 1u;
      for (uint32_t cdn = 0; cdn < 4; cdn++) {
        const sg::AliasRow& ar = alias_of(cdn, cdn, b);
        for (uint32_t c = 0; c < W; c++)
          blk[192 + c * 4 + cdn] = (c << (16 - L.lgW)) | (ar.thr[c] >> 16) | (uint32_t)((ar.lo[c] + mq) ^ (ar.hi[c] + mq)) << 16 | (uint32_t)(ar.hi[c] + mq) << 24;
      }
    }
  // (2) full substitution rows for the kernel's fix-up path: [mate][bin][192], the outcomes in natural codes
  pad4(tab, 0);
  L.fast_sub_off = tab.size();
  tab.resize(L.fast_sub_off + (size_t)n_mates * bins * 192 * 4);
  for (int t = 0; t < n_mates; t++)
    for (int b = 0; b < bins; b++)
      for (uint32_t sl = 0; sl < 192; sl++) pack_sub_row(&tab[L.fast_sub_off + (((size_t)t * bins + b) * 192 + sl) * 4], row_of(t, sl, b), nat_of);
  // (3) all alias columns in natural order: [cdn][kn][bins][W]
  L.fast_alias_off = tab.size();
  tab.resize(L.fast_alias_off + arows.size() * W * 2);
  for (uint32_t cdn = 0; cdn < 4; cdn++)
    for (uint32_t kn = 0; kn < 4; kn++)
      for (int b = 0; b < bins; b++) pack_alias_row(&tab[L.fast_alias_off + ((((size_t)cdn * 4 + kn) * bins + b) * W) * 2], alias_of(cdn, kn, b), W);
  pad4(tab, 0);
}

int build_tables(const sg_profile_cdf* pr, sg_profile_tables& T) {
  if (!pr) return T.fail(SG_ERR_INVALID, "sg_profile_prepare: null profile");
  Builder b{*pr, T};
  if (int rc = b.checks()) return rc;
  b.sub_rows();
  if (int rc = b.alias_columns()) return rc;
  b.length_rows();
  if (int rc = b.gap_row()) return rc;
  if (pr->kmer == 3) b.fast_tables();
  return SG_OK;
}

}  // namespace

extern "C" {

int sg_profile_prepare(const sg_profile_cdf* pr, sg_profile_tables** out) {
  if (!out) return SG_ERR_INVALID;
  sg_profile_tables* T = new sg_profile_tables();
  *out = T;
  return build_tables(pr, *T);
}
const char* sg_profile_tables_error(const sg_profile_tables* T) { return T ? T->err.c_str() : "null tables"; }
void sg_profile_tables_free(sg_profile_tables* T) { delete T; }

uint64_t sg_cdf_count_le(double c) { return sg::count_le(c); }

int sg_sub_row_identity_first(const double cdf4[4], int cd, uint64_t cum[3], uint8_t order[4]) {
  if (!cdf4 || !cum || !order || cd < 0 || cd > 3) return SG_ERR_INVALID;
  const sg::SubRow r = sg::encode_sub_row_identity_first(cdf4, cd);
  for (int i = 0; i < 3; i++) cum[i] = r.c[i];
  for (int i = 0; i < 4; i++) order[i] = r.order[i];
  return SG_OK;
}

uint32_t sg_row_symbols(const double* cdf, int n) { return (cdf && n > 0) ? sg::symbols_with_mass(sg::row_masses(cdf, n)) : 0u; }

int sg_alias_row(const double* cdf, int n, uint32_t lgW, uint32_t* thr, uint8_t* lo, uint8_t* hi) {
  if (!cdf || n < 1 || n > 256 || lgW < 2 || lgW > 8 || !thr || !lo || !hi) return SG_ERR_INVALID;
  try {
    const sg::AliasRow r = sg::build_alias_row(sg::row_masses(cdf, n), lgW);
    for (uint32_t c = 0; c < (1u << lgW); c++) { thr[c] = r.thr[c]; lo[c] = r.lo[c]; hi[c] = r.hi[c]; }
  } catch (const std::exception&) {
    return SG_ERR_INVALID;
  }
  return SG_OK;
}

}  // extern "C"
