// sg_api_errors.cpp -- the C ABI of the true error counts (sg_errtab_*; kernel: sg_errors.hip; the counting rule:
// errtab_walk, sg_truth.h).  The state is sg_ctx::Errtab with its buffer; nothing of it exists before
// sg_errtab_begin.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "sg_api.h"
#include "sg_truth.h"

namespace {

int errtab_need(sg_ctx* ctx, const char* who) { return sg_need_begun(ctx, ctx && ctx->errtab.on, who, "sg_errtab_begin"); }
sg::ErrtabDims dims_of(const sg_ctx::Errtab& E) { return sg::ErrtabDims{E.cycles, E.qual_lo, E.n_qual, E.L}; }
// Errtab::table: the table's cells | the kernel's counters (5 x u64)
size_t table_counters(const sg::ErrtabDims& d) { return sg_counters_at((size_t)sg::errtab_cells(d) * 8); }

bool dims_ok(uint32_t cycles, uint32_t qual_lo, uint32_t n_qual, uint32_t L) {
  return L >= 1u && L <= 0xFFFFu && cycles >= L && cycles <= 0xFFFFu && n_qual >= 1u && n_qual <= 128u && qual_lo + n_qual <= 223u;
}

}  // namespace

extern "C" {

int sg_errtab_begin(sg_ctx* ctx, uint32_t cycles, uint32_t qual_lo, uint32_t n_qual) {
  if (!ctx) return SG_ERR_INVALID;
  if (!ctx->have_profile) return ctx->fail(SG_ERR_INVALID, "sg_errtab_begin: load a profile first (its read length is the template's)");
  const uint32_t L = (uint32_t)ctx->P.L;
  if (!dims_ok(cycles, qual_lo, n_qual, L))
    return ctx->fail(SG_ERR_INVALID, "sg_errtab_begin: cycles must lie in [read length, 65535], n_qual in [1, 128], qual_lo + n_qual below 224");
  SG_HIP(hipSetDevice(ctx->device));
  int cus = 0;
  SG_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  sg_ctx::Errtab E;
  E.cycles = cycles; E.qual_lo = qual_lo; E.n_qual = n_qual; E.L = L; E.cus = (uint32_t)(cus > 0 ? cus : 0);
  const size_t cnt = table_counters(dims_of(E));
  SG_ENSURE(ctx->errtab.table, cnt + 64);
  SG_HIP(hipMemsetAsync(ctx->errtab.table.p, 0, cnt + 64, ctx->stream));
  E.table = std::move(ctx->errtab.table);   // (the state changes only once nothing can fail any more)
  E.on = true;
  ctx->errtab = std::move(E);
  return SG_OK;
}

int sg_errtab_add(sg_ctx* ctx, uint64_t* bases, uint64_t* errors) {
  if (int rc = errtab_need(ctx, "sg_errtab_add")) return rc;
  if (int rc = sg_pass_prelude(ctx, "sg_errtab_add", nullptr)) return rc;   // (the reads meet their templates: no piece map)
  const sg::DevBatch& B = ctx->B;
  sg_ctx::Errtab& E = ctx->errtab;
  if ((uint32_t)ctx->P.L != E.L) return ctx->fail(SG_ERR_INVALID, "sg_errtab_add: the profile's read length is not the one sg_errtab_begin saw");
  if (bases) *bases = 0;
  if (errors) *errors = 0;
  if (!B.n_slots) return SG_OK;
  sg::ErrtabJob J;
  memset(&J, 0, sizeof J);
  J.d = dims_of(E);
  J.win_cycles = sg::errtab_win_cycles(J.d);
  J.table = ctx->errtab.table.as<unsigned long long>();
  J.counters = (unsigned long long*)(ctx->errtab.table.as<uint8_t>() + table_counters(J.d));
  uint64_t c[5] = {0, 0, 0, 0, 0};
  if (int rc = sg_run_counted(ctx, J.counters, 5, c, [&]() { sg::launch_errtab_add(ctx->P, B, J, E.cus, ctx->stream); })) return rc;
  // a failed add folds nothing into the sums: the device's table may hold a part of the pass and is undefined until
  // sg_errtab_reset
  if (c[4] & 2) return ctx->fail(SG_ERR_INVALID, "sg_errtab_add: a read's events do not end at the read's length (the read was not counted)");
  if (c[4] & 4) return ctx->fail(SG_ERR_OVERFLOW, "sg_errtab_add: a read is longer than the table's cycles (the read was not counted)");
  if (c[4] & 8) return ctx->fail(SG_ERR_INVALID, "sg_errtab_add: a quality byte outside the table's range (the base was not counted)");
  if (c[4] & 16) return ctx->fail(SG_ERR_INVALID, "sg_errtab_add: a record lies outside its mate's text (the read was not counted)");
  E.bases += c[0];
  E.errors += c[1];
  E.skipped += c[2];
  E.reads += c[3];
  if (bases) *bases = c[0];
  if (errors) *errors = c[1];
  return SG_OK;
}

int sg_errtab_counts(sg_ctx* ctx, uint64_t* out, uint64_t cap, uint64_t* n) {
  if (!ctx || !n || (cap && !out)) return SG_ERR_INVALID;
  if (int rc = errtab_need(ctx, "sg_errtab_counts")) return rc;
  const uint64_t cells = sg::errtab_cells(dims_of(ctx->errtab));
  *n = cells;
  if (!cap) return SG_OK;
  if (cells > cap) return ctx->fail(SG_ERR_OVERFLOW, "sg_errtab_counts: the table does not fit cap");
  SG_HIP(hipSetDevice(ctx->device));
  SG_HIP(hipMemcpyAsync(out, ctx->errtab.table.p, (size_t)cells * 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

int sg_errtab_reset(sg_ctx* ctx) {
  if (int rc = errtab_need(ctx, "sg_errtab_reset")) return rc;
  SG_HIP(hipSetDevice(ctx->device));
  SG_HIP(hipMemsetAsync(ctx->errtab.table.p, 0, table_counters(dims_of(ctx->errtab)) + 64, ctx->stream));
  ctx->errtab.bases = ctx->errtab.errors = ctx->errtab.skipped = ctx->errtab.reads = 0;
  return SG_OK;
}

int sg_errtab_info(sg_ctx* ctx, sg_errtab_shape* out) {
  if (!ctx || !out) return SG_ERR_INVALID;
  if (int rc = errtab_need(ctx, "sg_errtab_info")) return rc;
  const sg_ctx::Errtab& E = ctx->errtab;
  const sg::ErrtabDims d = dims_of(E);
  out->cycles = E.cycles;
  out->qual_lo = E.qual_lo;
  out->n_qual = E.n_qual;
  out->tmpl_len = E.L;
  out->cells = sg::errtab_cells(d);
  out->bases = E.bases;
  out->errors = E.errors;
  out->skipped = E.skipped;
  out->reads = E.reads;
  out->win_cycles = sg::errtab_win_cycles(d);
  out->lds_bytes = (2u * d.n_qual * out->win_cycles + 20u * 64u) * 4u;
  return SG_OK;
}

int sg_errtab_end(sg_ctx* ctx) {
  if (int rc = errtab_need(ctx, "sg_errtab_end")) return rc;
  ctx->errtab = sg_ctx::Errtab();
  return SG_OK;
}

int sg_errtab_observe(const uint8_t* codes, uint32_t tmpl_len, int reverse, const uint32_t* events, uint32_t n_events, const char* bases,
                      const char* quals, uint32_t read_len, uint32_t mate, uint32_t cycles, uint32_t qual_lo, uint32_t n_qual, uint64_t* table,
                      uint64_t cells) {
  if (!codes || !bases || !quals || !table || (n_events && !events) || mate > 1u || !dims_ok(cycles, qual_lo, n_qual, tmpl_len)) return SG_ERR_INVALID;
  const sg::ErrtabDims d{cycles, qual_lo, n_qual, tmpl_len};
  if (cells != sg::errtab_cells(d)) return SG_ERR_INVALID;
  // the read as a whole first: a refused read counts nowhere
  if (read_len > cycles) return SG_ERR_OVERFLOW;
  if (sg::errtab_walk(events, n_events, tmpl_len, [](uint32_t, uint32_t, uint32_t, uint32_t) {}) != read_len) return SG_ERR_INVALID;
  for (uint32_t r = 0; r < read_len; r++) {
    const uint32_t qb = (uint8_t)quals[r];
    if (qb < 33u + qual_lo || qb - 33u - qual_lo >= n_qual) return SG_ERR_INVALID;
  }
  const bool rev = reverse != 0;
  sg::errtab_walk(events, n_events, tmpl_len, [&](uint32_t kind, uint32_t j0, uint32_t r0, uint32_t n) {
    if (kind == 2u || kind == 1u) {
      uint64_t* row = table + sg::errtab_indel(d, kind == 2u ? 1u : 0u, mate, j0);
      row[0] += 1;
      row[1] += n;
    }
    if (kind == 2u) return;
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t r = r0 + i, q = (uint8_t)quals[r] - 33u - qual_lo;
      uint64_t* cell = table + sg::errtab_q(d, mate, r, q);
      if (kind == 1u) { cell[sg::kErrInserted]++; continue; }
      const uint32_t j = j0 + i;
      const uint32_t tc = sg::errtab_tmpl_code(codes[rev ? tmpl_len - 1u - j : j], rev);
      if (tc >= 4u) { cell[sg::kErrOther]++; continue; }
      const uint32_t rc = sg::errtab_read_code((uint8_t)bases[r]);
      cell[sg::kErrBases]++;
      if (rc != tc) cell[sg::kErrErrors]++;
      table[sg::errtab_s(d, mate, tc, rc)]++;
    }
  });
  return SG_OK;
}

}  // extern "C"
