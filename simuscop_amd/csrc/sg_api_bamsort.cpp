// sg_api_bamsort.cpp -- sg_bamsort_*: the truth BAM in coordinate order (simuReads --truth-sort).  The order is stated in
// sg_bamsort.h, the kernels are in sg_bamsort.hip.  A pass comes out sorted because the pack kernels write each record
// at rec_off[read], and rec_off here is the scan of the lengths taken in key order (sg_pass_records, sg_api_truth.cpp); the
// sorted passes of a stem are merged by sorting their concatenation again (sg_bamsort_merge), which needs no pass, no
// profile and no piece map.
#include <algorithm>
#include <cstring>

#include "simuscop_amd.h"
#include "sg_api.h"
#include "sg_bamsort.h"
#include "sg_scan.h"

static_assert(SG_BAMSORT_TILE == sg::kSortTile, "SG_BAMSORT_TILE is the sort block's keys");

namespace {

// The arrays of one call in ctx->bamsort.work.
struct SortWork {
  unsigned long long* counters;   // 8: [0] live records (the scan's total), [1] OR and [2] AND of the keys, [3] stream bytes, [4] gather flags, [7] unused totals
  uint32_t* blk_count;            // key kernel: live records per 256 reads ...
  uint64_t* blk_off;              // ... and their scan
  uint32_t* hist;                 // [256][sort blocks] of one digit pass ...
  uint64_t* hist_off;             // ... and their scan
  uint64_t* src_off;              // merge: scan of the input lengths
  uint64_t* dst_off;              // scan of the lengths in output order
  uint32_t* in_len;               // merge: the input lengths
  uint64_t* bsum;                 // launch_scan_u32's block sums (the largest of the scans)
};

int carve_work(sg_ctx* ctx, uint32_t n, bool pass, bool merge, SortWork* W) {
  const uint32_t n_hist = sg::kSortDigits * sg::bamsort_blocks(n), n_blk = (n + 255u) / 256u;
  return sg_carve(ctx, ctx->bamsort.work, [&](SgArena& a) {
    W->counters = a.take<unsigned long long>(8);
    W->blk_count = a.take<uint32_t>(pass ? n_blk : 0);
    W->blk_off = a.take<uint64_t>(pass ? n_blk : 0);
    W->hist = a.take<uint32_t>(n_hist);
    W->hist_off = a.take<uint64_t>(n_hist);
    W->src_off = a.take<uint64_t>(merge ? n : 0);
    W->dst_off = a.take<uint64_t>(n);
    W->in_len = a.take<uint32_t>(merge ? n : 0);
    W->bsum = a.take<uint64_t>((size_t)sg::scan_blocks(std::max(n, n_hist)) + 8);
  });
}

// Sorts the n (key, payload) pairs in keys[cur] / vals[cur] stably by key.  A digit that is the same in all keys (the OR
// and the AND of the keys agree on it) moves nothing and is skipped.
int sort_pairs(sg_ctx* ctx, const SortWork& W, uint32_t n, uint64_t k_or, uint64_t k_and) {
  sg_ctx::BamSort& S = ctx->bamsort;
  return bamsort_sort_pairs(ctx, SgSortBufs{S.keys, S.vals, &S.cur, W.hist, W.hist_off, W.bsum, (uint64_t*)&W.counters[7]}, n, k_or, k_and);
}

int ensure_pairs(sg_ctx* ctx, uint32_t n) {
  sg_ctx::BamSort& S = ctx->bamsort;
  for (int i = 0; i < 2; i++) {
    SG_ENSURE(S.keys[i], (size_t)n * 8 + 64);
    SG_ENSURE(S.vals[i], (size_t)n * 4 + 64);
  }
  SG_ENSURE(S.lens, (size_t)n * 4 + 64);
  return SG_OK;
}

}  // namespace

int bamsort_sort_pairs(sg_ctx* ctx, const SgSortBufs& b, uint32_t n, uint64_t k_or, uint64_t k_and) {
  if (n < 2) return SG_OK;
  const uint32_t n_hist = sg::kSortDigits * sg::bamsort_blocks(n);
  for (uint32_t shift = 0; shift < 64; shift += 8) {
    if ((((k_or ^ k_and) >> shift) & 255u) == 0) continue;
    const int from = *b.cur, to = *b.cur ^ 1;
    sg::launch_bamsort_hist(b.keys[from].as<uint64_t>(), n, shift, b.hist, ctx->stream);
    sg::launch_scan_u32(b.hist, n_hist, b.bsum, b.hist_off, b.total, ctx->stream);
    sg::launch_bamsort_scatter(b.keys[from].as<uint64_t>(), b.vals[from].as<uint32_t>(), n, shift, b.hist_off, b.keys[to].as<uint64_t>(),
                               b.vals[to].as<uint32_t>(), ctx->stream);
    *b.cur = to;
  }
  SG_HIP(hipGetLastError());
  return SG_OK;
}

int bamsort_pass_keys(sg_ctx* ctx, const sg::TruthJob& J, bool paired) {
  sg_ctx::BamSort& S = ctx->bamsort;
  const uint32_t N = J.map.n_reads;
  S.have = false;
  S.dst_off = nullptr;
  S.n = S.out_bytes = S.gz_bytes = 0;
  S.cur = 0;
  SortWork W;
  if (int rc = carve_work(ctx, N, true, false, &W)) return rc;
  if (int rc = ensure_pairs(ctx, N)) return rc;
  hipStream_t s = ctx->stream;
  SG_HIP(hipMemsetAsync(W.counters, 0, 64, s));
  SG_HIP(hipMemsetAsync(&W.counters[2], 0xFF, 8, s));
  const uint32_t n_blk = (N + 255u) / 256u;
  sg::launch_bamsort_count(J.rec_len, N, W.blk_count, s);
  sg::launch_scan_u32(W.blk_count, n_blk, W.bsum, W.blk_off, (uint64_t*)&W.counters[0], s);
  sg::launch_bamsort_keys(J.rows, J.rec_len, N, paired ? 1u : 0u, W.blk_off, S.keys[0].as<uint64_t>(), S.vals[0].as<uint32_t>(), W.counters, s);
  return SG_OK;
}

int bamsort_pass_order(sg_ctx* ctx, const sg::TruthJob& J, uint64_t* rec_off, uint64_t* total) {
  sg_ctx::BamSort& S = ctx->bamsort;
  const uint32_t N = J.map.n_reads;
  *total = 0;
  if (!N) return SG_OK;
  SortWork W;
  if (int rc = carve_work(ctx, N, true, false, &W)) return rc;   // (the same arrays as in bamsort_pass_keys: nothing moves)
  uint64_t c[3] = {};
  if (int rc = sg_read_back(ctx, c, W.counters, sizeof c)) return rc;
  if (c[0] > N) return ctx->fail(SG_ERR_INVALID, "sg_bamsort_pass: more keys than reads");
  const uint32_t n = (uint32_t)c[0];
  if (!n) return SG_OK;
  if (int rc = sort_pairs(ctx, W, n, c[1], c[2])) return rc;
  hipStream_t s = ctx->stream;
  const uint32_t* vals = S.vals[S.cur].as<uint32_t>();
  sg::launch_bamsort_lens(J.rec_len, vals, n, S.lens.as<uint32_t>(), s);
  sg::launch_scan_u32(S.lens.as<uint32_t>(), n, W.bsum, W.dst_off, (uint64_t*)&W.counters[3], s);
  sg::launch_bamsort_offsets(W.dst_off, vals, n, rec_off, s);
  if (int rc = sg_read_back(ctx, total, &W.counters[3], 8)) return rc;
  S.n = n;
  S.out_bytes = *total;
  return SG_OK;
}

extern "C" {

int sg_bamsort_pass(sg_ctx* ctx, uint32_t tags, uint64_t* record_bytes, uint64_t* records) {
  if (!ctx) return SG_ERR_INVALID;
  uint64_t rb = 0;
  if (int rc = sg_pass_records(ctx, "sg_bamsort_pass", tags, true, &rb, nullptr)) return rc;
  if (record_bytes) *record_bytes = rb;
  if (records) *records = ctx->bamsort.n;
  return SG_OK;
}

int sg_bamsort_merge(sg_ctx* ctx, uint32_t n_runs, const void* const* records, const uint64_t* record_bytes, const uint64_t* const* keys,
                     const uint32_t* const* lens, const uint64_t* n, uint64_t* out_bytes, uint64_t* bgzf_bytes) {
  if (!ctx) return SG_ERR_INVALID;
  if (n_runs && (!records || !record_bytes || !keys || !lens || !n)) return ctx->fail(SG_ERR_INVALID, "sg_bamsort_merge: null run tables");
  sg_ctx::BamSort& S = ctx->bamsort;
  S.have = false;
  S.dst_off = nullptr;
  S.n = S.out_bytes = S.gz_bytes = 0;
  S.cur = 0;
  ctx->pass.bam_sorted = false;   // the index is this call's from here on
  if (out_bytes) *out_bytes = 0;
  if (bgzf_bytes) *bgzf_bytes = 0;
  uint64_t total_n = 0, total_b = 0, k_or = 0, k_and = ~0ull;
  for (uint32_t r = 0; r < n_runs; r++) {
    if (n[r] && (!keys[r] || !lens[r])) return ctx->fail(SG_ERR_INVALID, "sg_bamsort_merge: run " + std::to_string(r) + " has no keys or lengths");
    if (record_bytes[r] && !records[r]) return ctx->fail(SG_ERR_INVALID, "sg_bamsort_merge: run " + std::to_string(r) + " has no records");
    uint64_t b = 0;
    for (uint64_t i = 0; i < n[r]; i++) {
      b += lens[r][i];
      k_or |= keys[r][i];
      k_and &= keys[r][i];
    }
    if (b != record_bytes[r])
      return ctx->fail(SG_ERR_INVALID, "sg_bamsort_merge: the lengths of run " + std::to_string(r) + " do not add up to its bytes");
    total_n += n[r];
    total_b += b;
  }
  if (total_n >= 0xFFFFFFF0ull) return ctx->fail(SG_ERR_UNSUPPORTED, "sg_bamsort_merge: 2^32 records or more");
  SG_HIP(hipSetDevice(ctx->device));
  const uint32_t N = (uint32_t)total_n;
  if (N) {
    hipStream_t s = ctx->stream;
    SortWork W;
    if (int rc = carve_work(ctx, N, false, true, &W)) return rc;
    if (int rc = ensure_pairs(ctx, N)) return rc;
    SG_ENSURE(S.src, total_b + 64);
    SG_ENSURE(S.out, total_b + 64);
    SG_HIP(hipMemsetAsync(W.counters, 0, 64, s));
    uint64_t at_n = 0, at_b = 0;
    for (uint32_t r = 0; r < n_runs; r++) {   // in run order: ties keep it
      if (n[r]) {
        SG_HIP(hipMemcpyAsync(S.keys[0].as<uint64_t>() + at_n, keys[r], n[r] * 8, hipMemcpyHostToDevice, s));
        SG_HIP(hipMemcpyAsync(W.in_len + at_n, lens[r], n[r] * 4, hipMemcpyHostToDevice, s));
      }
      if (record_bytes[r]) SG_HIP(hipMemcpyAsync(S.src.as<uint8_t>() + at_b, records[r], record_bytes[r], hipMemcpyHostToDevice, s));
      at_n += n[r];
      at_b += record_bytes[r];
    }
    SG_HIP(hipStreamSynchronize(s));   // the caller's slices are its own again
    sg::launch_bamsort_iota(S.vals[0].as<uint32_t>(), N, s);
    sg::launch_scan_u32(W.in_len, N, W.bsum, W.src_off, (uint64_t*)&W.counters[7], s);
    if (int rc = sort_pairs(ctx, W, N, k_or, k_and)) return rc;
    const uint32_t* vals = S.vals[S.cur].as<uint32_t>();
    sg::launch_bamsort_lens(W.in_len, vals, N, S.lens.as<uint32_t>(), s);
    sg::launch_scan_u32(S.lens.as<uint32_t>(), N, W.bsum, W.dst_off, (uint64_t*)&W.counters[3], s);
    sg::launch_bamsort_gather(S.src.as<uint8_t>(), total_b, W.src_off, vals, S.lens.as<uint32_t>(), W.dst_off, N, S.out.as<uint8_t>(), total_b,
                              &W.counters[4], s);
    uint64_t c[2] = {};
    if (int rc = sg_read_back(ctx, c, &W.counters[3], sizeof c)) return rc;
    if (c[0] != total_b || (c[1] & 1)) return ctx->fail(SG_ERR_INVALID, "sg_bamsort_merge: a record outside the stream");
    if (total_b)
      if (int rc = deflate_text(ctx, S.out.as<uint8_t>(), total_b, S.gz, &S.gz_bytes, "sg_bamsort_merge")) return rc;
    S.dst_off = W.dst_off;
  }
  S.n = N;
  S.out_bytes = total_b;
  S.have = true;
  if (out_bytes) *out_bytes = S.out_bytes;
  if (bgzf_bytes) *bgzf_bytes = S.gz_bytes;
  return SG_OK;
}

// whether a merge or the current pass left an index, and whose
static int bamsort_need(sg_ctx* ctx, const char* who, bool* from_pass) {
  *from_pass = !ctx->bamsort.have && ctx->pass.have_bam && ctx->pass.bam_sorted;
  if (ctx->bamsort.have || *from_pass) return SG_OK;
  return ctx->fail(SG_ERR_INVALID, std::string(who) + ": call sg_bamsort_pass or sg_bamsort_merge first");
}

int sg_bamsort_index(sg_ctx* ctx, uint64_t* keys_out, uint32_t* lens_out, uint64_t cap, uint64_t* n) {
  if (!ctx || !n) return SG_ERR_INVALID;
  bool from_pass;
  if (int rc = bamsort_need(ctx, "sg_bamsort_index", &from_pass)) return rc;
  const sg_ctx::BamSort& S = ctx->bamsort;
  *n = S.n;
  if (!keys_out && !lens_out) return SG_OK;
  if (S.n > cap) return ctx->fail(SG_ERR_OVERFLOW, "sg_bamsort_index: the index does not fit cap");
  SG_HIP(hipSetDevice(ctx->device));
  if (S.n && keys_out) SG_HIP(hipMemcpyAsync(keys_out, S.keys[S.cur].p, S.n * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (S.n && lens_out) SG_HIP(hipMemcpyAsync(lens_out, S.lens.p, S.n * 4, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

int sg_bamsort_fetch(sg_ctx* ctx, int compressed, uint64_t offset, uint64_t bytes, void* host_dst) {
  if (!ctx || (bytes && !host_dst)) return SG_ERR_INVALID;
  bool from_pass;
  if (int rc = bamsort_need(ctx, "sg_bamsort_fetch", &from_pass)) return rc;
  sg_ctx::BamSort& S = ctx->bamsort;
  if (from_pass && compressed) return ctx->fail(SG_ERR_INVALID, "sg_bamsort_fetch: a sorted pass is not compressed (its runs are merged first)");
  const uint64_t have = compressed ? S.gz_bytes : S.out_bytes;
  if (offset > have || bytes > have - offset) return ctx->fail(SG_ERR_INVALID, "sg_bamsort_fetch: range past the end of the data");
  SG_HIP(hipSetDevice(ctx->device));
  if (bytes) {
    const uint8_t* src = (from_pass ? ctx->truth.rec : compressed ? S.gz : S.out).as<uint8_t>() + offset;
    SG_HIP(hipMemcpyAsync(host_dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipStreamSynchronize(ctx->stream));
  }
  return SG_OK;
}

}  // extern "C"
