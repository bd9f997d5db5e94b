// sg_api_depth.cpp -- the C ABI of the true coverage (sg_depth_*; kernels: sg_depth.hip; the alignment rule: sg_truth.h).
// The state is sg_ctx::Depth with its four buffers; nothing of it exists before sg_depth_begin.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sg_api.h"
#include "sg_scan.h"
#include "sg_truth.h"

static_assert(sizeof(sg_depth_run) == sizeof(sg::DepthRun), "sg_depth_run is the kernel's row");

namespace {

int depth_need(sg_ctx* ctx, const char* who) { return sg_need_begun(ctx, ctx && ctx->depth.on, who, "sg_depth_begin"); }
int depth_contig(sg_ctx* ctx, const char* who, uint32_t contig) {
  if (int rc = depth_need(ctx, who)) return rc;
  if (contig >= ctx->depth.len.size()) return ctx->fail(SG_ERR_INVALID, std::string(who) + ": contig index out of range");
  return SG_OK;
}
// Depth::meta: contig_off[n] | contig_len[n] | counters (2 x u64)
size_t meta_counters(size_t n) { return sg_counters_at(2 * n * 8); }

sg::DepthJob depth_job(sg_ctx* ctx) {
  sg::DepthJob J;
  memset(&J, 0, sizeof J);
  const size_t n = ctx->depth.len.size();
  J.diff = ctx->depth.diff.as<int32_t>();
  J.contig_off = ctx->depth.meta.as<uint64_t>();
  J.contig_len = J.contig_off + n;
  J.n_contigs = (uint32_t)n;
  J.counters = (unsigned long long*)(ctx->depth.meta.as<uint8_t>() + meta_counters(n));
  J.stage_runs = sg::kDepthStageRuns;
  if (const char* e = getenv("SG_DEPTH_STAGE")) J.stage_runs = std::min(J.stage_runs, (uint32_t)strtoul(e, nullptr, 10));   // (tests: reads that walk twice)
  return J;
}

sg::DepthView depth_view(sg_ctx* ctx, uint32_t contig) {
  sg::DepthView V;
  V.diff = ctx->depth.diff.as<int32_t>() + ctx->depth.off[contig];
  V.len = (uint32_t)ctx->depth.len[contig];
  V.n_tiles = (V.len + sg::kDepthTile - 1) / sg::kDepthTile;
  return V;
}

// Depth::work for a contig of n tiles: tile_sum[n] u32 | tile_starts[n] u32 | tile_base[n] u64 | start_base[n] u64 |
// block sums of the two scans | their totals
struct WorkLayout {
  size_t sum, starts, base, sbase, bs0, bs1, tot, bytes;
  explicit WorkLayout(uint32_t n) {
    auto up = [](size_t v) { return (v + 63) & ~(size_t)63; };
    sum = 0;
    starts = up((size_t)n * 4);
    base = up(starts + (size_t)n * 4);
    sbase = up(base + (size_t)n * 8);
    bs0 = up(sbase + (size_t)n * 8);
    bs1 = up(bs0 + ((size_t)sg::scan_blocks(std::max(n, 1u)) + 8) * 8);
    tot = up(bs1 + ((size_t)sg::scan_blocks(std::max(n, 1u)) + 8) * 8);
    bytes = tot + 64;
  }
};

// the first half of the finishing pass: tile sums, run-start counts and their scans of `contig` into Depth::work
int depth_scan(sg_ctx* ctx, uint32_t contig) {
  sg_ctx::Depth& D = ctx->depth;
  if (D.scanned == (int64_t)contig) return SG_OK;
  D.scanned = -1;
  D.scanned_starts = 0;
  const sg::DepthView V = depth_view(ctx, contig);
  if (V.n_tiles) {
    const WorkLayout W(V.n_tiles);
    SG_ENSURE(ctx->depth.work, W.bytes);
    uint8_t* wk = ctx->depth.work.as<uint8_t>();
    hipStream_t s = ctx->stream;
    SG_HIP(hipMemsetAsync(wk + W.tot, 0, 64, s));
    sg::launch_depth_tiles(V, (uint32_t*)(wk + W.sum), (uint32_t*)(wk + W.starts), s);
    sg::launch_scan_u32((const uint32_t*)(wk + W.sum), V.n_tiles, (uint64_t*)(wk + W.bs0), (uint64_t*)(wk + W.base), (uint64_t*)(wk + W.tot), s);
    sg::launch_scan_u32((const uint32_t*)(wk + W.starts), V.n_tiles, (uint64_t*)(wk + W.bs1), (uint64_t*)(wk + W.sbase), (uint64_t*)(wk + W.tot + 8), s);
    uint64_t tot[2] = {0, 0};
    if (int rc = sg_read_back(ctx, tot, wk + W.tot, sizeof tot)) return rc;
    D.scanned_starts = tot[1];
  }
  D.scanned = (int64_t)contig;
  return SG_OK;
}

// a kernel that adds, and its counters: the M bases to the state, the flags to an error
template <class Launch>
int depth_added(sg_ctx* ctx, const char* who, const sg::DepthJob& J, uint64_t* m_bases, Launch launch) {
  uint64_t c[2] = {0, 0};
  ctx->depth.scanned = -1;
  if (int rc = sg_run_counted(ctx, J.counters, 2, c, launch)) return rc;
  ctx->depth.m_bases += c[0];
  if (m_bases) *m_bases = c[0];
  if (c[1] & 1) return ctx->fail(SG_ERR_INVALID, std::string(who) + ": an alignment lies outside its contig (it was not added)");
  if (c[1] & 2) return ctx->fail(SG_ERR_INVALID, std::string(who) + ": an alignment's runs do not end where the alignment ends");
  return SG_OK;
}

}  // namespace

extern "C" {

int sg_depth_begin(sg_ctx* ctx, const uint64_t* contig_len, uint32_t n_contigs) {
  if (!ctx || (n_contigs && !contig_len)) return SG_ERR_INVALID;
  SG_HIP(hipSetDevice(ctx->device));
  std::vector<uint64_t> len(contig_len, contig_len + n_contigs), off(n_contigs);
  uint64_t slots = 0;
  for (uint32_t c = 0; c < n_contigs; c++) {
    if (len[c] >= 0xFFFFFFF8ull) return ctx->fail(SG_ERR_UNSUPPORTED, "sg_depth_begin: contig " + std::to_string(c) + " has 2^32 - 8 bases or more");
    off[c] = slots;
    slots += (len[c] + 1 + 3) & ~(uint64_t)3;   // every contig starts at a multiple of 16 bytes
  }
  sg_ctx::Depth& D = ctx->depth;
  D = sg_ctx::Depth();
  const size_t bytes = (size_t)slots * 4 + 64;
  if (ctx->depth.diff.ensure(bytes)) {
    (void)hipGetLastError();
    return ctx->fail(SG_ERR_HIP, "sg_depth_begin: the device cannot hold the difference array of " + std::to_string(bytes) +
                                     " bytes (4 bytes per reference base)");
  }
  const size_t cnt = meta_counters(n_contigs);
  SG_ENSURE(ctx->depth.meta, cnt + 64);
  hipStream_t s = ctx->stream;
  SG_HIP(hipMemsetAsync(ctx->depth.diff.p, 0, bytes, s));
  SG_HIP(hipMemsetAsync(ctx->depth.meta.p, 0, cnt + 64, s));
  if (n_contigs) {
    SG_HIP(hipMemcpyAsync(ctx->depth.meta.p, off.data(), (size_t)n_contigs * 8, hipMemcpyHostToDevice, s));
    SG_HIP(hipMemcpyAsync(ctx->depth.meta.as<uint64_t>() + n_contigs, len.data(), (size_t)n_contigs * 8, hipMemcpyHostToDevice, s));
  }
  SG_HIP(hipStreamSynchronize(s));   // len and off are host memory of this frame
  D.len.swap(len);
  D.off.swap(off);
  D.slots = slots;
  D.on = true;
  return SG_OK;
}

int sg_depth_add(sg_ctx* ctx, uint64_t* m_bases) {
  if (int rc = depth_need(ctx, "sg_depth_add")) return rc;
  sg::DepthJob J = depth_job(ctx);
  if (int rc = sg_pass_prelude(ctx, "sg_depth_add", &J.map)) return rc;
  return depth_added(ctx, "sg_depth_add", J, m_bases, [&]() { sg::launch_depth_add(ctx->P, ctx->B, J, ctx->stream); });
}

int sg_depth_add_spans(sg_ctx* ctx, const uint32_t* contig, const uint64_t* start, const uint64_t* end, uint64_t n) {
  if (!ctx || (n && (!contig || !start || !end))) return SG_ERR_INVALID;
  if (int rc = depth_need(ctx, "sg_depth_add_spans")) return rc;
  const sg_ctx::Depth& D = ctx->depth;
  for (uint64_t i = 0; i < n; i++) {
    if (contig[i] >= D.len.size()) return ctx->fail(SG_ERR_INVALID, "sg_depth_add_spans: span " + std::to_string(i) + " names a contig that does not exist");
    if (start[i] > end[i] || end[i] > D.len[contig[i]])
      return ctx->fail(SG_ERR_INVALID, "sg_depth_add_spans: span " + std::to_string(i) + " is not inside its contig");
  }
  if (!n) return SG_OK;
  SG_HIP(hipSetDevice(ctx->device));
  const size_t o_start = ((size_t)n * 4 + 63) & ~(size_t)63, o_end = o_start + (size_t)n * 8;
  SG_ENSURE(ctx->depth.out, o_end + (size_t)n * 8);
  uint8_t* buf = ctx->depth.out.as<uint8_t>();
  hipStream_t s = ctx->stream;
  SG_HIP(hipMemcpyAsync(buf, contig, (size_t)n * 4, hipMemcpyHostToDevice, s));
  SG_HIP(hipMemcpyAsync(buf + o_start, start, (size_t)n * 8, hipMemcpyHostToDevice, s));
  SG_HIP(hipMemcpyAsync(buf + o_end, end, (size_t)n * 8, hipMemcpyHostToDevice, s));
  const sg::DepthJob J = depth_job(ctx);
  return depth_added(ctx, "sg_depth_add_spans", J, nullptr, [&]() {   // (synchronises: the caller's arrays are free again)
    sg::launch_depth_spans(J, (const uint32_t*)buf, (const uint64_t*)(buf + o_start), (const uint64_t*)(buf + o_end), n, s);
  });
}

int sg_depth_bins(sg_ctx* ctx, uint32_t contig, uint64_t bin, uint64_t* sums, uint64_t cap, uint64_t* n) {
  if (!ctx || !n || (cap && !sums)) return SG_ERR_INVALID;
  if (int rc = depth_contig(ctx, "sg_depth_bins", contig)) return rc;
  if (bin < 1) return ctx->fail(SG_ERR_INVALID, "sg_depth_bins: bin must be at least 1");
  const uint64_t len = ctx->depth.len[contig];
  const uint64_t n_bins = (len + bin - 1) / bin;
  *n = n_bins;
  if (!cap || !n_bins) return SG_OK;
  if (n_bins > cap) return ctx->fail(SG_ERR_OVERFLOW, "sg_depth_bins: the bins do not fit cap");
  SG_HIP(hipSetDevice(ctx->device));
  if (int rc = depth_scan(ctx, contig)) return rc;
  SG_ENSURE(ctx->depth.out, (size_t)n_bins * 8);
  hipStream_t s = ctx->stream;
  SG_HIP(hipMemsetAsync(ctx->depth.out.p, 0, (size_t)n_bins * 8, s));
  const sg::DepthView V = depth_view(ctx, contig);
  const WorkLayout W(V.n_tiles);
  sg::launch_depth_bins(V, (const uint64_t*)(ctx->depth.work.as<uint8_t>() + W.base), (uint32_t)std::min<uint64_t>(bin, 0xFFFFFFFFull),
                        ctx->depth.out.as<unsigned long long>(), s);
  return sg_read_back(ctx, sums, ctx->depth.out.p, (size_t)n_bins * 8);
}

int sg_depth_runs(sg_ctx* ctx, uint32_t contig, sg_depth_run* rows, uint64_t cap, uint64_t* n) {
  if (!ctx || !n || (cap && !rows)) return SG_ERR_INVALID;
  if (int rc = depth_contig(ctx, "sg_depth_runs", contig)) return rc;
  SG_HIP(hipSetDevice(ctx->device));
  if (int rc = depth_scan(ctx, contig)) return rc;
  const uint64_t n_rows = ctx->depth.scanned_starts;
  *n = n_rows;
  if (!cap || !n_rows) return SG_OK;
  if (n_rows > cap) return ctx->fail(SG_ERR_OVERFLOW, "sg_depth_runs: the rows do not fit cap");
  SG_ENSURE(ctx->depth.out, (size_t)n_rows * sizeof(sg::DepthRun));
  hipStream_t s = ctx->stream;
  const sg::DepthView V = depth_view(ctx, contig);
  const WorkLayout W(V.n_tiles);
  const uint8_t* wk = ctx->depth.work.as<uint8_t>();
  sg::launch_depth_runs(V, (const uint64_t*)(wk + W.base), (const uint64_t*)(wk + W.sbase), ctx->depth.out.as<sg::DepthRun>(), n_rows, s);
  return sg_read_back(ctx, rows, ctx->depth.out.p, (size_t)n_rows * sizeof(sg::DepthRun));
}

int sg_depth_fetch(sg_ctx* ctx, uint32_t contig, uint64_t first, uint64_t n, uint32_t* depth) {
  if (!ctx || (n && !depth)) return SG_ERR_INVALID;
  if (int rc = depth_contig(ctx, "sg_depth_fetch", contig)) return rc;
  const uint64_t len = ctx->depth.len[contig];
  if (first > len || n > len - first) return ctx->fail(SG_ERR_INVALID, "sg_depth_fetch: range past the end of the contig");
  if (!n) return SG_OK;
  SG_HIP(hipSetDevice(ctx->device));
  if (int rc = depth_scan(ctx, contig)) return rc;
  SG_ENSURE(ctx->depth.out, (size_t)n * 4);
  hipStream_t s = ctx->stream;
  const sg::DepthView V = depth_view(ctx, contig);
  const WorkLayout W(V.n_tiles);
  sg::launch_depth_fetch(V, (const uint64_t*)(ctx->depth.work.as<uint8_t>() + W.base), (uint32_t)first, (uint32_t)n, ctx->depth.out.as<uint32_t>(), s);
  return sg_read_back(ctx, depth, ctx->depth.out.p, (size_t)n * 4);
}

int sg_depth_reset(sg_ctx* ctx) {
  if (int rc = depth_need(ctx, "sg_depth_reset")) return rc;
  SG_HIP(hipSetDevice(ctx->device));
  SG_HIP(hipMemsetAsync(ctx->depth.diff.p, 0, (size_t)ctx->depth.slots * 4, ctx->stream));
  ctx->depth.m_bases = 0;
  ctx->depth.scanned = -1;
  return SG_OK;
}

int sg_depth_info(sg_ctx* ctx, uint32_t* n_contigs, uint64_t* m_bases, uint32_t* tile) {
  if (int rc = depth_need(ctx, "sg_depth_info")) return rc;
  if (n_contigs) *n_contigs = (uint32_t)ctx->depth.len.size();
  if (m_bases) *m_bases = ctx->depth.m_bases;
  if (tile) *tile = sg::kDepthTile;
  return SG_OK;
}

int sg_depth_end(sg_ctx* ctx) {
  if (int rc = depth_need(ctx, "sg_depth_end")) return rc;
  ctx->depth = sg_ctx::Depth();
  return SG_OK;
}

}  // extern "C"
