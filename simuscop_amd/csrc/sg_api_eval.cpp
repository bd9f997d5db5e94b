// sg_api_eval.cpp -- sg_eval_*: an aligner's BAM scored against the truth BAM (truthEval).  The rule is stated in sg_eval.h,
// the kernels are in sg_eval.hip; both files come in through SgBamStream (sg_api.h), the sort is sg_bamsort.hip's.  A session
// lives from sg_eval_begin to sg_eval_end:  truth members .. sg_eval_truth_done .. sg_eval_test_refmap .. test members ..
// sg_eval_finish.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <string>

#include "simuscop_amd.h"
#include "sg_api.h"
#include "sg_bam.h"
#include "sg_bamsort.h"
#include "sg_eval.h"
#include "sg_scan.h"

static_assert(SG_EVAL_CELLS == sg::kEvalCells, "SG_EVAL_CELLS is the table of sg_eval.h");
static_assert(sizeof(sg::EvalRow) == 40, "EvalRow is 40 bytes");

namespace {
using Clock = std::chrono::steady_clock;
double since(Clock::time_point t) { return std::chrono::duration<double>(Clock::now() - t).count(); }
// the sort's tiles are counted in u32: (n + kSortTile - 1) must not wrap
constexpr uint64_t kEvalMaxRows = 0xFFFFFFFFull - sg::kSortTile;
constexpr size_t kTableCells = sg::kEvalCells + sg::kEvalScalars + sg::kEvalMissing + 1;   // (+ the duplicates counter)
}  // namespace

struct sg_eval_session {
  enum Stage { Truth, Sorted, Test, Finished, Broken } stage = Truth;
  uint32_t key_bits = 64, pct = 10;
  SgBamStream truth, test;
  hipStream_t copy_stream = nullptr;
  DevBuf rows, arena, name_len, name_at, keys[2], vals[2], sort_work, claim, table, refmap, hit, hit_row;
  int cur = 0;
  uint64_t n_rows = 0, arena_used = 0, duplicates = 0, ordinal = 0;
  double t_inflate = 0, t_truth = 0, t_sort = 0, t_test = 0;
  ~sg_eval_session() {   // (the buffers go with their members)
    if (copy_stream) { (void)hipStreamSynchronize(copy_stream); (void)hipStreamDestroy(copy_stream); }
  }
  void job(sg::EvalJob& E) {
    memset(&E, 0, sizeof E);
    E.key_bits = key_bits; E.pct = pct;
    E.rows = rows.as<sg::EvalRow>(); E.n_rows = n_rows;
    E.arena = arena.as<uint8_t>(); E.arena_used = arena_used;
    E.keys = keys[cur].as<uint64_t>(); E.order = vals[cur].as<uint32_t>();
    E.claim = claim.as<unsigned long long>();
    E.name_len = name_len.as<uint32_t>(); E.name_at = name_at.as<uint64_t>();
    E.hit_row = hit_row.as<uint32_t>(); E.hit = hit.as<uint8_t>();
    E.ordinal0 = ordinal;
    E.refmap = refmap.as<int32_t>();
    E.table = table.as<unsigned long long>();
    E.dup_count = E.table + kTableCells - 1;
  }
};

namespace {

// One call's members of either file up to the record starts (bam_stream_stage, bam_stream_records), timed.
int feed_front(sg_ctx* ctx, sg_eval_session* S, SgBamStream& B, const char* who, const void* members, uint64_t bytes, sg::BamJob* J) {
  const auto t0 = Clock::now();
  int rc = bam_stream_stage(ctx, B, who, members, bytes, S->copy_stream);
  if (rc != SG_OK) return rc;
  SG_HIP(hipStreamSynchronize(S->copy_stream));   // the caller's buffer is free again when this returns
  rc = bam_stream_records(ctx, B, who, ctx->stream, S->copy_stream, J);
  S->t_inflate += since(t0);
  return rc;
}

}  // namespace

// a session that a refused member or record has ended: every later call but sg_eval_end / sg_eval_begin says so
#define SG_EVAL_NOT_BROKEN(S, who)                                                                                          \
  do {                                                                                                                      \
    if ((S) && (S)->stage == sg_eval_session::Broken)                                                                       \
      return ctx->fail(SG_ERR_INVALID, std::string(who) + ": the session has failed on its input: call sg_eval_end");       \
  } while (0)

extern "C" {

void sg_eval_end(sg_ctx* ctx) {
  if (!ctx || !ctx->eval) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  delete ctx->eval;
  ctx->eval = nullptr;
}

int sg_eval_begin(sg_ctx* ctx, uint32_t n_ref_truth, uint32_t key_bits, uint32_t min_overlap, uint64_t first_record_skip) {
  if (!ctx) return SG_ERR_INVALID;
  if (key_bits < 1 || key_bits > 64) return ctx->fail(SG_ERR_INVALID, "sg_eval_begin: key_bits must be 1..64");
  if (min_overlap < 1 || min_overlap > 100) return ctx->fail(SG_ERR_INVALID, "sg_eval_begin: min_overlap must be 1..100");
  SG_HIP(hipSetDevice(ctx->device));
  sg_eval_end(ctx);
  // the session is built aside and handed to the context only when all of it stands: on any failure below it is dropped
  std::unique_ptr<sg_eval_session> S(new sg_eval_session());
  S->key_bits = key_bits;
  S->pct = min_overlap;
  if (int rc = bam_stream_start(ctx, S->truth, nullptr, n_ref_truth, first_record_skip)) return rc;
  SG_ENSURE(S->table, kTableCells * 8 + 64);
  SG_HIP(hipMemsetAsync(S->table.p, 0, kTableCells * 8, ctx->stream));
  SG_HIP(hipStreamCreateWithFlags(&S->copy_stream, hipStreamNonBlocking));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  ctx->eval = S.release();
  return SG_OK;
}

int sg_eval_truth_bgzf(sg_ctx* ctx, const void* members, uint64_t bytes) {
  if (!ctx || (bytes && !members)) return SG_ERR_INVALID;
  sg_eval_session* S = ctx->eval;
  SG_EVAL_NOT_BROKEN(S, "sg_eval_truth_bgzf");
  if (!S || S->stage != sg_eval_session::Truth) return ctx->fail(SG_ERR_INVALID, "sg_eval_truth_bgzf: call sg_eval_begin first, and feed the truth before sg_eval_truth_done");
  SG_HIP(hipSetDevice(ctx->device));
  const char* who = "sg_eval_truth_bgzf";
  if (!bytes) return bam_stream_close(ctx, S->truth, who);
  const auto t0 = Clock::now();
  hipStream_t s = ctx->stream;
  sg::BamJob J;
  int rc = feed_front(ctx, S, S->truth, who, members, bytes, &J);
  if (rc != SG_OK) { S->stage = sg_eval_session::Broken; return rc; }
  const uint64_t n_rec = J.n_rec;
  if (n_rec) {
    if (S->n_rows + n_rec > kEvalMaxRows) S->stage = sg_eval_session::Broken;
    if (S->n_rows + n_rec > kEvalMaxRows) return ctx->fail(SG_ERR_UNSUPPORTED, "sg_eval_truth_bgzf: more than " + std::to_string(kEvalMaxRows) + " truth records");
    if ((rc = sg_grow_keep(ctx, S->rows, S->n_rows * sizeof(sg::EvalRow), (S->n_rows + n_rec) * sizeof(sg::EvalRow) + 64)) != SG_OK) return rc;
    SG_ENSURE(S->name_len, n_rec * 4 + 64);
    SG_ENSURE(S->name_at, n_rec * 8 + 64);
    sg::EvalJob E;
    S->job(E);
    E.error = (unsigned long long*)(J.totals + 3);
    sg::launch_eval_truth_rows(J, E, s);
    sg::launch_scan_u32(E.name_len, (uint32_t)n_rec, J.scan_bsum, E.name_at, J.totals + 1, s);
    uint64_t h_tot[4];
    if ((rc = bam_stream_totals(ctx, S->truth, who, J, h_tot)) != SG_OK) { S->stage = sg_eval_session::Broken; return rc; }
    const uint64_t name_bytes = h_tot[1];
    if ((rc = sg_grow_keep(ctx, S->arena, S->arena_used, S->arena_used + name_bytes + 64)) != SG_OK) return rc;
    S->job(E);
    E.error = (unsigned long long*)(J.totals + 3);
    sg::launch_eval_truth_names(J, E, s);
    SG_HIP(hipGetLastError());
    S->n_rows += n_rec;
    S->arena_used += name_bytes;
  }
  if ((rc = bam_stream_advance(ctx, S->truth, s)) != SG_OK) return rc;
  SG_HIP(hipStreamSynchronize(s));
  S->t_truth += since(t0);
  return SG_OK;
}

int sg_eval_truth_done(sg_ctx* ctx, uint64_t* records, uint64_t* duplicates) {
  if (!ctx) return SG_ERR_INVALID;
  sg_eval_session* S = ctx->eval;
  SG_EVAL_NOT_BROKEN(S, "sg_eval_truth_done");
  if (!S || S->stage != sg_eval_session::Truth) return ctx->fail(SG_ERR_INVALID, "sg_eval_truth_done: call sg_eval_begin first, once");
  SG_HIP(hipSetDevice(ctx->device));
  const auto t0 = Clock::now();
  hipStream_t s = ctx->stream;
  const uint32_t n = (uint32_t)S->n_rows;
  if (n) {
    for (int i = 0; i < 2; i++) {
      SG_ENSURE(S->keys[i], (size_t)n * 8 + 64);
      SG_ENSURE(S->vals[i], (size_t)n * 4 + 64);
    }
    SG_ENSURE(S->claim, (size_t)n * 8 + 64);
    const uint32_t n_hist = sg::kSortDigits * sg::bamsort_blocks(n);
    uint32_t* hist = nullptr;
    uint64_t *hist_off = nullptr, *bsum = nullptr, *total = nullptr;
    if (int rc = sg_carve(ctx, S->sort_work, [&](SgArena& a) {
          hist = a.take<uint32_t>(n_hist);
          hist_off = a.take<uint64_t>(n_hist);
          bsum = a.take<uint64_t>((size_t)sg::scan_blocks(std::max(n, n_hist)) + 8);
          total = a.take<uint64_t>(8);
        }))
      return rc;
    S->cur = 0;
    sg::launch_eval_sort_input(S->rows.as<sg::EvalRow>(), n, S->keys[0].as<uint64_t>(), S->vals[0].as<uint32_t>(), s);
    const uint64_t mask = S->key_bits >= 64 ? ~0ull : (1ull << S->key_bits) - 1;
    if (int rc = bamsort_sort_pairs(ctx, SgSortBufs{S->keys, S->vals, &S->cur, hist, hist_off, bsum, total}, n, mask, 0)) return rc;
    sg::EvalJob E;
    S->job(E);
    sg::launch_eval_duplicates(E, n, s);
    if (int rc = sg_read_back(ctx, &S->duplicates, E.dup_count, 8)) return rc;
  }
  S->stage = sg_eval_session::Sorted;
  S->t_sort += since(t0);
  if (records) *records = S->n_rows;
  if (duplicates) *duplicates = S->duplicates;
  return SG_OK;
}

int sg_eval_test_refmap(sg_ctx* ctx, const int32_t* map, uint32_t n_ref_test, uint64_t first_record_skip) {
  if (!ctx || (n_ref_test && !map)) return SG_ERR_INVALID;
  sg_eval_session* S = ctx->eval;
  SG_EVAL_NOT_BROKEN(S, "sg_eval_test_refmap");
  if (!S || S->stage != sg_eval_session::Sorted) return ctx->fail(SG_ERR_INVALID, "sg_eval_test_refmap: call sg_eval_truth_done first, once");
  for (uint32_t i = 0; i < n_ref_test; i++)
    if (map[i] < -1 || map[i] >= (int32_t)S->truth.n_ref) return ctx->fail(SG_ERR_INVALID, "sg_eval_test_refmap: entry " + std::to_string(i) + " names no truth reference");
  SG_HIP(hipSetDevice(ctx->device));
  SG_ENSURE(S->refmap, (size_t)n_ref_test * 4 + 64);
  if (n_ref_test) SG_HIP(hipMemcpy(S->refmap.p, map, (size_t)n_ref_test * 4, hipMemcpyHostToDevice));
  if (int rc = bam_stream_start(ctx, S->test, nullptr, n_ref_test, first_record_skip)) return rc;
  S->stage = sg_eval_session::Test;
  return SG_OK;
}

int sg_eval_test_bgzf(sg_ctx* ctx, const void* members, uint64_t bytes) {
  if (!ctx || (bytes && !members)) return SG_ERR_INVALID;
  sg_eval_session* S = ctx->eval;
  SG_EVAL_NOT_BROKEN(S, "sg_eval_test_bgzf");
  if (!S || S->stage != sg_eval_session::Test) return ctx->fail(SG_ERR_INVALID, "sg_eval_test_bgzf: call sg_eval_test_refmap first");
  SG_HIP(hipSetDevice(ctx->device));
  const char* who = "sg_eval_test_bgzf";
  if (!bytes) return bam_stream_close(ctx, S->test, who);
  const auto t0 = Clock::now();
  hipStream_t s = ctx->stream;
  sg::BamJob J;
  int rc = feed_front(ctx, S, S->test, who, members, bytes, &J);
  if (rc != SG_OK) { S->stage = sg_eval_session::Broken; return rc; }
  const uint64_t n_rec = J.n_rec;
  if (n_rec) {
    SG_ENSURE(S->hit, n_rec + 64);
    SG_ENSURE(S->hit_row, n_rec * 4 + 64);
    sg::EvalJob E;
    S->job(E);
    E.error = (unsigned long long*)(J.totals + 3);
    sg::launch_eval_lookup(J, E, s);
    sg::launch_eval_claim(J, E, s);
    sg::launch_eval_score(J, E, s);
    uint64_t h_tot[4];
    if ((rc = bam_stream_totals(ctx, S->test, who, J, h_tot)) != SG_OK) { S->stage = sg_eval_session::Broken; return rc; }
    S->ordinal += n_rec;
  }
  if ((rc = bam_stream_advance(ctx, S->test, s)) != SG_OK) return rc;
  SG_HIP(hipStreamSynchronize(s));
  S->t_test += since(t0);
  return SG_OK;
}

int sg_eval_finish(sg_ctx* ctx, uint64_t* table, uint64_t cap, sg_eval_counts* counts) {
  if (!ctx || !counts) return SG_ERR_INVALID;
  sg_eval_session* S = ctx->eval;
  SG_EVAL_NOT_BROKEN(S, "sg_eval_finish");
  if (!S || (S->stage != sg_eval_session::Test && S->stage != sg_eval_session::Finished))
    return ctx->fail(SG_ERR_INVALID, "sg_eval_finish: call sg_eval_test_refmap and feed the test file first");
  if (table && cap < sg::kEvalCells) return ctx->fail(SG_ERR_OVERFLOW, "sg_eval_finish: the table holds SG_EVAL_CELLS cells");
  SG_HIP(hipSetDevice(ctx->device));
  sg::EvalJob E;
  S->job(E);
  if (S->stage == sg_eval_session::Test) {   // (once: the missing pass adds to the table)
    sg::launch_eval_missing(E, S->n_rows, ctx->stream);
    S->stage = sg_eval_session::Finished;
  }
  std::vector<uint64_t> h(kTableCells);
  if (int rc = sg_read_back(ctx, h.data(), E.table, kTableCells * 8)) return rc;
  if (table) memcpy(table, h.data(), (size_t)sg::kEvalCells * 8);
  const uint64_t* sc = h.data() + sg::kEvalCells;
  memset(counts, 0, sizeof *counts);
  counts->test_records = sc[sg::kEvalNTest];
  counts->secondary = sc[sg::kEvalNSecondary];
  counts->supplementary = sc[sg::kEvalNSupplementary];
  counts->unknown = sc[sg::kEvalNUnknown];
  counts->ambiguous = sc[sg::kEvalNAmbiguous];
  counts->repeated = sc[sg::kEvalNRepeated];
  counts->truth_records = S->n_rows;
  counts->truth_duplicates = S->duplicates;
  for (uint32_t m = 0; m < sg::kEvalMissing; m++) counts->missing[m] = sc[sg::kEvalScalars + m];
  counts->truth_bytes = S->truth.inflated;
  counts->test_bytes = S->test.inflated;
  counts->t_inflate = S->t_inflate;
  counts->t_truth = S->t_truth;
  counts->t_sort = S->t_sort;
  counts->t_test = S->t_test;
  return SG_OK;
}

uint32_t sg_eval_classify(int32_t truth_ref, int64_t truth_pos, uint64_t truth_span, int truth_reverse, int truth_unmapped, int32_t test_ref,
                          int64_t test_pos, uint64_t test_span, int test_reverse, int test_unmapped, uint32_t min_overlap) {
  const sg::EvalAln t{truth_ref, truth_pos, truth_span, truth_reverse ? 1u : 0u, truth_unmapped ? 1u : 0u};
  const sg::EvalAln q{test_ref, test_pos, test_span, test_reverse ? 1u : 0u, test_unmapped ? 1u : 0u};
  return sg::eval_classify(t, q, min_overlap);
}

uint64_t sg_eval_key(const void* name, uint32_t len, uint32_t mate, uint32_t key_bits) {
  return sg::eval_key((const uint8_t*)name, len, mate, key_bits < 1 ? 1 : key_bits);
}

}  // extern "C"
