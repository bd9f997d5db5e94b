// sg_api_variants.cpp -- the C ABI of the true allele counts (sg_variants_*, sg_variant_observe; kernel: sg_variants.hip;
// the counting rule: truth_variant_scan, sg_truth.h).  The state is sg_ctx::Variants with its two buffers;
// nothing of it exists before sg_variants_begin.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "sg_api.h"
#include "sg_truth.h"

static_assert(sizeof(sg::VariantRow) == 16, "the scan loads a row as 16 bytes");

namespace {

int variants_need(sg_ctx* ctx, const char* who) { return sg_need_begun(ctx, ctx && ctx->variants.on, who, "sg_variants_begin"); }
// Variants::counts: counts[n][2] u32 | the kernel's counters (3 x u64)
size_t counts_counters(uint64_t n) { return sg_counters_at((size_t)n * 8); }

// The ABI's rows as the scan's; the index of the first row that breaks the rules, or n.
uint64_t variant_rows(const sg_variant* rows, uint64_t n, std::vector<sg::VariantRow>& out) {
  out.resize((size_t)n);
  for (uint64_t i = 0; i < n; i++) {
    const sg_variant& v = rows[i];
    if (v.kind > 2u || v.pos > 0xFFFFFFFFull) return i;
    if (v.kind == 0u ? (v.len != 0u || v.allele == 0u || v.allele > 0xFFu) : (v.len == 0u || v.allele != 0u)) return i;
    if (i) {
      const sg_variant& u = rows[i - 1];
      if (!(std::make_tuple(u.contig, u.pos, u.kind, u.allele, u.len) < std::make_tuple(v.contig, v.pos, v.kind, v.allele, v.len))) return i;
    }
    out[(size_t)i] = sg::VariantRow{sg::variant_key(v.contig, v.pos), v.len, v.kind | (v.kind == 0u ? sg::variant_base_code(v.allele) << 8 : 0u)};
  }
  return n;
}

}  // namespace

extern "C" {

int sg_variants_begin(sg_ctx* ctx, const sg_variant* rows, uint64_t n) {
  if (!ctx || (n && !rows)) return SG_ERR_INVALID;
  if (n >= 0x7FFFFFFFull) return ctx->fail(SG_ERR_UNSUPPORTED, "sg_variants_begin: 2^31 rows or more");
  std::vector<sg::VariantRow> tab;
  const uint64_t bad = variant_rows(rows, n, tab);
  if (bad < n)
    return ctx->fail(SG_ERR_INVALID, "sg_variants_begin: row " + std::to_string(bad) + " is out of range or out of order (contig, pos, kind, allele, len ascending, no two alike)");
  SG_HIP(hipSetDevice(ctx->device));
  ctx->variants = sg_ctx::Variants();
  const size_t cnt = counts_counters(n);
  SG_ENSURE(ctx->variants.rows, (size_t)n * sizeof(sg::VariantRow) + 64);
  SG_ENSURE(ctx->variants.counts, cnt + 64);
  hipStream_t s = ctx->stream;
  SG_HIP(hipMemsetAsync(ctx->variants.counts.p, 0, cnt + 64, s));
  if (n) SG_HIP(hipMemcpyAsync(ctx->variants.rows.p, tab.data(), (size_t)n * sizeof(sg::VariantRow), hipMemcpyHostToDevice, s));
  SG_HIP(hipStreamSynchronize(s));   // tab is host memory of this frame
  ctx->variants.n = n;
  ctx->variants.on = true;
  return SG_OK;
}

int sg_variants_add(sg_ctx* ctx, uint64_t* reads_hit, uint64_t* hits) {
  if (int rc = variants_need(ctx, "sg_variants_add")) return rc;
  sg::VariantJob J;
  memset(&J, 0, sizeof J);
  if (int rc = sg_pass_prelude(ctx, "sg_variants_add", &J.map)) return rc;
  if (reads_hit) *reads_hit = 0;
  if (hits) *hits = 0;
  if (!ctx->variants.n) return SG_OK;
  J.table = ctx->variants.rows.as<sg::VariantRow>();
  J.n_rows = ctx->variants.n;
  J.counts = ctx->variants.counts.as<uint32_t>();
  J.counters = (unsigned long long*)(ctx->variants.counts.as<uint8_t>() + counts_counters(J.n_rows));
  uint64_t c[3] = {0, 0, 0};
  if (int rc = sg_run_counted(ctx, J.counters, 3, c, [&]() { sg::launch_variants_add(ctx->P, ctx->B, J, ctx->stream); })) return rc;
  ctx->variants.reads_hit += c[0];
  ctx->variants.hits += c[1];
  if (reads_hit) *reads_hit = c[0];
  if (hits) *hits = c[1];
  if (c[2] & 1) return ctx->fail(SG_ERR_INVALID, "sg_variants_add: a template's first piece was not found in the piece map (the read was not counted)");
  return SG_OK;
}

int sg_variants_counts(sg_ctx* ctx, uint32_t* out, uint64_t cap, uint64_t* n) {
  if (!ctx || !n || (cap && !out)) return SG_ERR_INVALID;
  if (int rc = variants_need(ctx, "sg_variants_counts")) return rc;
  const uint64_t rows = ctx->variants.n;
  *n = rows;
  if (!cap || !rows) return SG_OK;
  if (rows > cap) return ctx->fail(SG_ERR_OVERFLOW, "sg_variants_counts: the rows do not fit cap");
  SG_HIP(hipSetDevice(ctx->device));
  SG_HIP(hipMemcpyAsync(out, ctx->variants.counts.p, (size_t)rows * 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  for (uint64_t i = 0; i < rows; i++) std::swap(out[2 * i], out[2 * i + 1]);   // the device keeps (total, alt)
  return SG_OK;
}

int sg_variants_reset(sg_ctx* ctx) {
  if (int rc = variants_need(ctx, "sg_variants_reset")) return rc;
  SG_HIP(hipSetDevice(ctx->device));
  SG_HIP(hipMemsetAsync(ctx->variants.counts.p, 0, counts_counters(ctx->variants.n) + 64, ctx->stream));
  ctx->variants.reads_hit = 0;
  ctx->variants.hits = 0;
  return SG_OK;
}

int sg_variants_info(sg_ctx* ctx, uint64_t* n_rows, uint64_t* reads_hit, uint64_t* hits) {
  if (int rc = variants_need(ctx, "sg_variants_info")) return rc;
  if (n_rows) *n_rows = ctx->variants.n;
  if (reads_hit) *reads_hit = ctx->variants.reads_hit;
  if (hits) *hits = ctx->variants.hits;
  return SG_OK;
}

int sg_variants_end(sg_ctx* ctx) {
  if (int rc = variants_need(ctx, "sg_variants_end")) return rc;
  ctx->variants = sg_ctx::Variants();
  return SG_OK;
}

int sg_variant_observe(const sg_truth_piece* pieces, uint64_t n_pieces, const uint8_t* codes, uint64_t tmpl_off, uint32_t tmpl_len,
                       const sg_variant* rows, uint64_t n_rows, uint32_t* hit_row, uint8_t* hit_alt, uint64_t cap, uint64_t* n_hits) {
  if (!pieces || !n_pieces || !codes || !n_hits || (n_rows && !rows) || (cap && (!hit_row || !hit_alt)) || tmpl_len == 0 || tmpl_len > 0xFFFFu ||
      n_rows >= 0x7FFFFFFFull)
    return SG_ERR_INVALID;
  std::vector<sg::TruthPiece> tp((size_t)n_pieces);
  for (uint64_t i = 0; i < n_pieces; i++) {
    const sg_truth_piece& p = pieces[i];
    if (p.len == 0 || p.contig > 0x3FFFFFFFu || (i && p.dst != pieces[i - 1].dst + pieces[i - 1].len)) return SG_ERR_INVALID;
    tp[i] = sg::TruthPiece{p.dst, p.src, p.len, sg::truth_meta(p.contig, p.kind, p.seg_first)};
  }
  if (tmpl_off < tp[0].dst || tmpl_off + tmpl_len > tp.back().dst + tp.back().len) return SG_ERR_INVALID;
  std::vector<sg::VariantRow> tab;
  if (variant_rows(rows, n_rows, tab) < n_rows) return SG_ERR_INVALID;
  const uint64_t pi = sg::truth_find_piece(tp.data(), 0, n_pieces, tmpl_off);
  uint64_t n = 0;
  sg::truth_variant_scan(tp.data(), n_pieces, pi, tmpl_off, tmpl_len, codes, tmpl_off, tab.data(), n_rows, [&](uint64_t row, bool alt) {
    if (n < cap) { hit_row[n] = (uint32_t)row; hit_alt[n] = alt ? 1 : 0; }
    n++;
  });
  *n_hits = n;
  return SG_OK;
}

}  // extern "C"
