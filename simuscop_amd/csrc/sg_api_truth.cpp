// sg_api_truth.cpp -- truth alignments and the truth BAM of the C ABI (rule: sg_truth.h, kernels: sg_truth.hip,
// sg_truth_tags.hip): the chains' piece map, the preconditions every truth output shares (sg_pass_prelude), a pass's
// alignments as rows (sg_truth_reads) and as BAM records (sg_pass_records).
#include <algorithm>
#include <cstring>

#include "sg_api.h"
#include "sg_scan.h"
#include "sg_truth.h"

// ---- the piece map's and the pass's preconditions (sg_api.h) ----
static int no_piece_map(sg_ctx* ctx, const char* who) {
  return ctx->fail(SG_ERR_INVALID, std::string(who) + ": the chains have no piece map (they were not made by sg_build_haplotypes)");
}

static int truth_need_map(sg_ctx* ctx, const char* who) {
  if (!ctx->truth.from_build) return no_piece_map(ctx, who);
  if (!ctx->truth.mapped) return ctx->fail(SG_ERR_INVALID, std::string(who) + ": call sg_truth_map first");
  return SG_OK;
}

// the map, then the records of sg_truth_bam
static int truth_need_bam(sg_ctx* ctx, const char* who) {
  if (int rc = truth_need_map(ctx, who)) return rc;
  return ctx->pass.have_bam ? SG_OK : ctx->fail(SG_ERR_INVALID, std::string(who) + ": call sg_truth_bam first");
}

static int rows_need_current(sg_ctx* ctx, const char* who) {
  if (ctx->pass.rows_current) return SG_OK;
  return ctx->fail(SG_ERR_INVALID, std::string(who) + ": the chains or the profile changed since sg_sample");
}

int sg_pass_prelude(sg_ctx* ctx, const char* who, sg::PieceMap* map, bool bam_names) {
  if (int rc = rows_need_current(ctx, who)) return rc;
  if (map)
    if (int rc = truth_need_map(ctx, who)) return rc;
  if (int rc = sg_pass_need(ctx, who, sg_ctx::Pass::Settled)) return rc;
  const sg::DevBatch& B = ctx->B;
  const uint32_t nm = B.paired ? 2 : 1;
  if (map && (uint64_t)B.n_slots * nm >= 0xFFFFFFF0ull) return ctx->fail(SG_ERR_UNSUPPORTED, std::string(who) + ": more than 2^32 reads in one pass");
  if (bam_names && B.prefix_len > 200) return ctx->fail(SG_ERR_UNSUPPORTED, std::string(who) + ": read names longer than a BAM record holds");
  if (B.diag)
    return ctx->fail(SG_ERR_UNSUPPORTED, std::string(who) + ": the pass ran under SG_DIAG (a timing ablation: its reads are not those of their rows)");
  if (map) {
    const size_t n_chains = ctx->hap.len.size();
    map->chain_first = ctx->truth.map.as<uint64_t>();
    map->pieces = (const sg::TruthPiece*)(ctx->truth.map.as<uint8_t>() + sg::truth_map_pieces_at(n_chains));
    map->n_chains = (uint32_t)n_chains;
    map->n_reads = B.n_slots * nm;
  }
  return SG_OK;
}

static_assert(sizeof(sg_truth_read) == sizeof(sg::TruthReadRow), "sg_truth_read is the kernel's row");
static_assert(SG_TAG_NM == sg::kTagNM && SG_TAG_MD == sg::kTagMD && SG_TAG_XE == sg::kTagXE, "SG_TAG_* are the kernels' bits");

// With tags == 0 exactly the kernels of the untagged stream are launched and nothing of the tags is allocated; with
// sorted == false nothing of the sort is launched or allocated.
int sg_pass_records(sg_ctx* ctx, const char* who, uint32_t tags, bool sorted, uint64_t* record_bytes, uint64_t* bgzf_bytes) {
  if (!ctx) return SG_ERR_INVALID;
  if (tags & ~(uint32_t)(SG_TAG_NM | SG_TAG_MD | SG_TAG_XE)) return ctx->fail(SG_ERR_INVALID, "sg_truth_bam_tags: tags is a mask of SG_TAG_NM, SG_TAG_MD and SG_TAG_XE");
  sg::TruthJob J;
  memset(&J, 0, sizeof J);
  if (int rc = sg_pass_prelude(ctx, who, &J.map, true)) return rc;
  sg_ctx::Truth& T = ctx->truth;
  if ((tags & (SG_TAG_NM | SG_TAG_MD)) && (!T.n_refs || !ctx->ref_codes.p))
    return ctx->fail(SG_ERR_INVALID, "sg_truth_bam_tags: NM and MD need the reference's codes (sg_reference_commit)");
  if (tags && (uint32_t)ctx->P.L > sg::kTruthTagMaxL)
    return ctx->fail(SG_ERR_UNSUPPORTED, "sg_truth_bam_tags: reads too long for the tagged record kernel (templates of more than " +
                                             std::to_string(sg::kTruthTagMaxL) + " bases)");
  sg_ctx::Pass& Q = ctx->pass;
  const sg::DevBatch& B = ctx->B;
  const uint32_t N = J.map.n_reads;
  Q.have_bam = Q.bam_sorted = false;
  Q.bam_rec_bytes = Q.bam_gz_bytes = Q.bam_records = Q.bam_unmapped = 0;
  for (uint64_t& v : Q.bam_tags) v = 0;
  hipStream_t s = ctx->stream;
  // the pack kernel's stages: one record's FASTQ text and one record's image, for reads of up to L + 512 bases
  const uint32_t np_cap = (uint32_t)ctx->P.L + 512u;
  J.text_lds = (16u + 256u + 2u * np_cap + 4u + 31u) & ~15u;
  const uint32_t tag_cap = tags ? sg::truth_tag_bytes(tags, sg::kTruthMaxMd) : 0u;
  J.image_lds = (16u + 36u + 256u + 4u * sg::kTruthMaxOps + np_cap + (np_cap + 1u) / 2u + tag_cap + 15u) & ~15u;
  if ((size_t)sg::kTruthWaveOps * 4 + 64 * 9 * 4 + J.text_lds + J.image_lds > 160u * 1024u)
    return ctx->fail(SG_ERR_UNSUPPORTED, std::string(who) + ": reads too long for the record kernel");
  // the call's arrays; the eight counters are zeroed and read back as one: [0] records, [1] unmapped, [2] flags, [4] stream bytes
  uint64_t *rec_off = nullptr, *bsum = nullptr;
  if (int rc = sg_carve(ctx, T.work, [&](SgArena& a) {
        J.counters = a.take<unsigned long long>(8);
        J.rows = a.take<sg::TruthRow>(N);
        J.rec_len = a.take<uint32_t>(N);
        rec_off = a.take<uint64_t>(N);
        bsum = a.take<uint64_t>((size_t)sg::scan_blocks(N) + 8);
      }))
    return rc;
  J.rec_off = rec_off;
  // the tags' job: per-read rows {NM, XE, MD length} and behind them the sizing kernel's eight counters
  sg::TagJob G;
  memset(&G, 0, sizeof G);
  if (tags) {
    const size_t at = sg_counters_at((size_t)N * sizeof(sg::TagRow));
    SG_ENSURE(T.tag_rows, at + 64);
    G.tags = tags;
    G.n_refs = T.n_refs;
    G.refs = T.refs.as<sg::TagRef>();
    G.ref_codes = ctx->ref_codes.as<uint8_t>();
    G.rows = T.tag_rows.as<sg::TagRow>();
    G.counters = (unsigned long long*)(T.tag_rows.as<uint8_t>() + at);
    SG_HIP(hipMemsetAsync(G.counters, 0, 64, s));
  }
  uint64_t c[8] = {};
  int sort_rc = SG_OK;
  if (int rc = sg_run_counted(ctx, J.counters, 8, c, [&]() {
        if (!N) return;
        sg::launch_truth_size(ctx->P, B, J, s);
        if (tags) sg::launch_truth_tag_size(ctx->P, B, J, G, s);
        if (!sorted) sg::launch_scan_u32(J.rec_len, N, bsum, rec_off, (uint64_t*)&J.counters[4], s);
        else sort_rc = bamsort_pass_keys(ctx, J, B.paired != 0);
      }))
    return rc;
  if (sort_rc) return sort_rc;
  if (c[2] & 3) return ctx->fail(SG_ERR_OVERFLOW, std::string(who) + ": an alignment with more than " + std::to_string(sg::kTruthMaxOps) + " operations");
  uint64_t tc[8] = {};
  if (tags) {
    if (int rc = sg_read_back(ctx, tc, G.counters, 64)) return rc;
    if (tc[7] & 1) return ctx->fail(SG_ERR_INVALID, "sg_truth_bam_tags: a read whose events or operations do not end at its length");
    if (tc[7] & 2) return ctx->fail(SG_ERR_INVALID, "sg_truth_bam_tags: an alignment outside its contig of the committed reference");
    if (tc[7] & 4) return ctx->fail(SG_ERR_INVALID, "sg_truth_bam_tags: a record outside its mate's text");
  }
  if (sorted) {   // rec_off by read index from the lengths in key order
    if (int rc = bamsort_pass_order(ctx, J, rec_off, &c[4])) return rc;
  }
  const uint64_t total = c[4];
  if (total) {
    SG_ENSURE(T.rec, total + 64);
    J.out = T.rec.as<uint8_t>();
    J.out_bytes = total;
    if (tags) sg::launch_truth_pack_tags(ctx->P, B, J, G, s);
    else sg::launch_truth_pack(ctx->P, B, J, s);
    uint64_t flags = 0;
    if (int rc = sg_read_back(ctx, &flags, &J.counters[2], 8)) return rc;
    if (flags & 4) return ctx->fail(SG_ERR_UNSUPPORTED, std::string(who) + ": a record does not fit the record kernel's stages");
    if (!sorted)
      if (int rc = deflate_text(ctx, T.rec.as<uint8_t>(), total, T.gz, &Q.bam_gz_bytes, who)) return rc;
  }
  for (int i = 0; i < 7; i++) Q.bam_tags[i] = tc[i];
  Q.bam_rec_bytes = total;
  Q.bam_records = c[0];
  Q.bam_unmapped = c[1];
  Q.have_bam = true;
  Q.bam_sorted = sorted;
  if (record_bytes) *record_bytes = Q.bam_rec_bytes;
  if (bgzf_bytes) *bgzf_bytes = Q.bam_gz_bytes;
  return SG_OK;
}

extern "C" {

int sg_truth_align(const sg_truth_piece* pieces, uint64_t n_pieces, uint64_t tmpl_off, uint32_t tmpl_len, int reverse,
                   const uint32_t* events, uint32_t n_events, int32_t* contig, int64_t* pos0, uint32_t* cigar, uint32_t cap,
                   uint32_t* n_ops) {
  if (!pieces || !n_pieces || !contig || !pos0 || !n_ops || (cap && !cigar) || (n_events && !events) || n_events > SG_MAX_EVENTS ||
      tmpl_len == 0 || tmpl_len > 0xFFFFu)
    return SG_ERR_INVALID;
  std::vector<sg::TruthPiece> tp((size_t)n_pieces);
  for (uint64_t i = 0; i < n_pieces; i++) {
    const sg_truth_piece& p = pieces[i];
    if (p.len == 0 || p.contig > 0x3FFFFFFFu || (i && p.dst != pieces[i - 1].dst + pieces[i - 1].len)) return SG_ERR_INVALID;
    tp[i] = sg::TruthPiece{p.dst, p.src, p.len, sg::truth_meta(p.contig, p.kind, p.seg_first)};
  }
  if (tmpl_off < tp[0].dst || tmpl_off + tmpl_len > tp.back().dst + tp.back().len) return SG_ERR_INVALID;
  uint32_t next = 0;   // events ascend and stay apart: a deletion of [j, j + k) is followed by j + k at the earliest
  for (uint32_t e = 0; e < n_events; e++) {
    const uint32_t j = events[e] & 0xFFFFu, k = (events[e] >> 16) & 0x7FFFu, del = events[e] >> 31;
    if (k == 0 || j < next || j >= tmpl_len || (del && j + k > tmpl_len)) return SG_ERR_INVALID;
    next = del ? j + k : j + 1;
  }
  const uint64_t pi = sg::truth_find_piece(tp.data(), 0, n_pieces, tmpl_off);
  const sg::TruthAln A = sg::truth_walk(tp.data(), n_pieces, pi, tmpl_off, tmpl_len, reverse != 0, events, n_events,
                                        [&](uint32_t i, uint32_t v) { if (i < cap) cigar[i] = v; });
  *contig = A.contig;
  *pos0 = A.pos0;
  *n_ops = A.n_ops;
  return A.n_ops > cap ? SG_ERR_OVERFLOW : SG_OK;
}

int sg_truth_map(sg_ctx* ctx, const sg_hap_piece* pieces, const uint8_t* seg_first, uint64_t n_pieces, const int32_t* ref_ids,
                 uint32_t n_ref_ids) {
  if (!ctx || (n_pieces && (!pieces || !seg_first))) return SG_ERR_INVALID;
  sg_ctx::Truth& T = ctx->truth;
  if (!T.from_build || !ctx->have_haps) return no_piece_map(ctx, "sg_truth_map");
  if (n_pieces != T.n_given) return ctx->fail(SG_ERR_INVALID, "sg_truth_map: the pieces are not those of sg_build_haplotypes (another count)");
  SG_HIP(hipSetDevice(ctx->device));
  const size_t n_chains = ctx->hap.len.size();
  for (uint64_t i = 0; i < n_pieces; i++)
    if (pieces[i].chain >= n_chains) return ctx->fail(SG_ERR_INVALID, "sg_truth_map: piece " + std::to_string(i) + " names a chain that does not exist");
  std::vector<uint64_t> order((size_t)n_pieces);
  for (uint64_t i = 0; i < n_pieces; i++) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
    const sg_hap_piece &x = pieces[a], &y = pieces[b];
    return x.chain != y.chain ? x.chain < y.chain : x.dst < y.dst;
  });
  // Everything is checked and built beside the context's state, which changes only once nothing can fail any more: a
  // refused call leaves an earlier map as it was.  The pieces of a chain must tile it -- no hole, no overlap, none of
  // length 0 (the walk of sg_truth.h takes a piece's first base for granted).
  std::vector<sg_truth_piece> sorted((size_t)n_pieces);
  std::vector<uint64_t> chain_first(n_chains + 1, n_pieces);
  std::vector<sg::TruthPiece> dev((size_t)n_pieces);
  uint32_t chain = 0;
  uint64_t at = 0;   // offset in `chain` up to which it is tiled
  chain_first[0] = 0;
  auto chain_done = [&]() { return at == ctx->hap.len[chain]; };
  for (uint64_t i = 0; i < n_pieces; i++) {
    const sg_hap_piece& p = pieces[order[i]];
    while (chain < p.chain) {
      if (!chain_done()) return ctx->fail(SG_ERR_INVALID, "sg_truth_map: the pieces of chain " + std::to_string(chain) + " do not tile it");
      chain_first[++chain] = i;
      at = 0;
    }
    if (p.len == 0 || p.dst != at)
      return ctx->fail(SG_ERR_INVALID, "sg_truth_map: the pieces of chain " + std::to_string(chain) + " do not tile it (piece " + std::to_string(order[i]) + ")");
    at += p.len;
    sorted[i] = sg_truth_piece{p.dst, p.src, p.len, p.contig, p.kind ? 1u : 0u, seg_first[order[i]] ? 1u : 0u};
    int32_t ref = (int32_t)p.contig;
    if (ref_ids && !p.kind) {
      if (p.contig >= n_ref_ids) return ctx->fail(SG_ERR_INVALID, "sg_truth_map: a piece's contig has no entry in ref_ids");
      ref = ref_ids[p.contig];
    }
    if (ref < 0 || ref > 0x3FFFFFFF) return ctx->fail(SG_ERR_INVALID, "sg_truth_map: reference id out of range");
    dev[i] = sg::TruthPiece{p.dst, p.src, p.len, sg::truth_meta((uint32_t)ref, p.kind, seg_first[order[i]])};
  }
  for (;;) {
    if (n_chains && !chain_done()) return ctx->fail(SG_ERR_INVALID, "sg_truth_map: the pieces of chain " + std::to_string(chain) + " do not tile it");
    if (chain + 1 >= n_chains) break;
    chain_first[++chain] = n_pieces;
    at = 0;
  }
  // the way back for the tag kernels: refID -> the codes of the first contig row that carries it
  std::vector<sg::TagRef> refs;
  for (size_t c = ctx->ref_contigs.size(); c-- > 0;) {
    const int64_t ref = ref_ids ? (c < n_ref_ids ? ref_ids[c] : -1) : (int64_t)c;
    if (ref < 0 || ref >= (int64_t)ctx->ref_contigs.size()) continue;   // (a refID no contig row can hold: its records fail the tagged call)
    if (refs.size() <= (size_t)ref) refs.resize((size_t)ref + 1, sg::TagRef{0, 0});
    refs[(size_t)ref] = sg::TagRef{ctx->ref_contigs[c].code_off, ctx->ref_contigs[c].length};
  }
  T.mapped = false;   // (a copy that fails half-way leaves no map rather than a mixed one)
  ctx->pass.have_bam = false;   // (records of another map)
  T.n_refs = 0;
  if (!refs.empty()) {
    SG_ENSURE(T.refs, refs.size() * sizeof(sg::TagRef));
    SG_HIP(hipMemcpyAsync(T.refs.p, refs.data(), refs.size() * sizeof(sg::TagRef), hipMemcpyHostToDevice, ctx->stream));
  }
  const size_t first_b = sg::truth_map_pieces_at(n_chains);
  SG_ENSURE(T.map, first_b + dev.size() * sizeof(sg::TruthPiece) + 64);
  SG_HIP(hipMemcpyAsync(T.map.p, chain_first.data(), (n_chains + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  if (!dev.empty())
    SG_HIP(hipMemcpyAsync(T.map.as<uint8_t>() + first_b, dev.data(), dev.size() * sizeof(sg::TruthPiece), hipMemcpyHostToDevice, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));   // dev is host memory of this frame
  T.sorted.swap(sorted);
  T.chain_first.swap(chain_first);
  T.n_refs = (uint32_t)refs.size();
  T.mapped = true;
  return SG_OK;
}

int sg_truth_pieces(sg_ctx* ctx, uint32_t chain, sg_truth_piece* out, uint64_t cap, uint64_t* n) {
  if (!ctx || !n || (cap && !out)) return SG_ERR_INVALID;
  if (int rc = truth_need_map(ctx, "sg_truth_pieces")) return rc;
  const sg_ctx::Truth& T = ctx->truth;
  if ((size_t)chain + 1 >= T.chain_first.size()) return ctx->fail(SG_ERR_INVALID, "sg_truth_pieces: chain index out of range");
  const uint64_t a = T.chain_first[chain], b = T.chain_first[chain + 1];
  *n = b - a;
  if (b - a > cap) return ctx->fail(SG_ERR_OVERFLOW, "sg_truth_pieces: the pieces do not fit cap");
  std::copy(T.sorted.begin() + (long)a, T.sorted.begin() + (long)b, out);
  return SG_OK;
}

int sg_truth_reads(sg_ctx* ctx, int mate, uint32_t first_slot, uint32_t n, sg_truth_read* out) {
  if (!ctx || mate < 0 || mate > 1 || (n && !out)) return SG_ERR_INVALID;
  if (int rc = rows_need_current(ctx, "sg_truth_reads")) return rc;
  if (int rc = truth_need_map(ctx, "sg_truth_reads")) return rc;
  if (int rc = sg_pass_need(ctx, "sg_truth_reads", sg_ctx::Pass::Settled)) return rc;
  if (mate == 1 && !ctx->B.paired) return ctx->fail(SG_ERR_INVALID, "sg_truth_reads: a single-end pass has no mate 2");
  if ((uint64_t)first_slot + n > ctx->B.n_slots) return ctx->fail(SG_ERR_INVALID, "sg_truth_reads: slots past the end of the batch");
  if (!n) return SG_OK;
  SG_ENSURE(ctx->truth.rows, (size_t)n * sizeof(sg::TruthReadRow));
  sg::launch_truth_reads(ctx->P, ctx->B, (uint32_t)mate, first_slot, n, ctx->truth.rows.as<sg::TruthReadRow>(), ctx->stream);
  return sg_read_back(ctx, out, ctx->truth.rows.p, (size_t)n * sizeof(sg::TruthReadRow));
}

int sg_truth_bam(sg_ctx* ctx, uint64_t* record_bytes, uint64_t* bgzf_bytes) { return sg_truth_bam_tags(ctx, 0, record_bytes, bgzf_bytes); }

int sg_truth_bam_tags(sg_ctx* ctx, uint32_t tags, uint64_t* record_bytes, uint64_t* bgzf_bytes) {
  return sg_pass_records(ctx, tags ? "sg_truth_bam_tags" : "sg_truth_bam", tags, false, record_bytes, bgzf_bytes);
}

int sg_fetch_truth(sg_ctx* ctx, int compressed, uint64_t offset, uint64_t bytes, void* host_dst) {
  if (!ctx || (bytes && !host_dst)) return SG_ERR_INVALID;
  if (int rc = truth_need_bam(ctx, "sg_fetch_truth")) return rc;
  if (!sg_range_within(offset, bytes, compressed ? ctx->pass.bam_gz_bytes : ctx->pass.bam_rec_bytes))
    return ctx->fail(SG_ERR_INVALID, "sg_fetch_truth: range past the end of the data");
  const uint8_t* src = (compressed ? ctx->truth.gz : ctx->truth.rec).as<uint8_t>() + offset;
  SG_HIP(sg_fetch_bytes(ctx->device, ctx->stream, host_dst, src, bytes));
  return SG_OK;
}

int sg_truth_tag_info(sg_ctx* ctx, sg_truth_tag_counts* out) {
  if (!ctx || !out) return SG_ERR_INVALID;
  if (int rc = truth_need_bam(ctx, "sg_truth_tag_info")) return rc;
  const uint64_t* t = ctx->pass.bam_tags;
  *out = sg_truth_tag_counts{t[0], t[1], t[2], t[3], t[4], t[5], t[6], sg::kTruthMaxMd};
  return SG_OK;
}

int sg_truth_info(sg_ctx* ctx, uint64_t* records, uint64_t* unmapped) {
  if (!ctx) return SG_ERR_INVALID;
  if (int rc = truth_need_bam(ctx, "sg_truth_info")) return rc;
  if (records) *records = ctx->pass.bam_records;
  if (unmapped) *unmapped = ctx->pass.bam_unmapped;
  return SG_OK;
}

}  // extern "C"
