// sg_api_bamindex.cpp -- sg_bamindex_*: the BAI index of the sorted truth BAM (simuReads --truth-index).  The index is
// stated in sg_bamindex.h, the kernels are in sg_bamindex.hip.  A call indexes the records of one compressed text while
// that text and the member offset table of its compression are still on the device: the output of the last
// sg_bamsort_merge, or the text of the last sg_deflate_bgzf.  It leaves the call's chunk rows grouped by (refID, bin) --
// sorted by the sort of sg_bamsort_* -- and adds to the stem's linear index and counts.
#include <algorithm>
#include <cstring>

#include "simuscop_amd.h"
#include "sg_api.h"
#include "sg_bamindex.h"
#include "sg_bamsort.h"
#include "sg_deflate.h"
#include "sg_scan.h"

static_assert(sizeof(sg_bai_chunk) == 24, "a chunk row is three u64");
static_assert(sg::kGzChunk == 32768, "a virtual offset's member is u >> 15");

namespace {

// The arrays of one call in ctx->bamindex.work.
struct IndexWork {
  unsigned long long* counters;   // 8: [0] flags, [1] chunks (the scan's total), [2] chunks of refID -1, [7] unused totals
  sg::BaiRow* rows;
  uint64_t* voff;
  uint32_t* head;
  uint64_t* rank;
  uint64_t* cbeg;
  uint64_t* cend;
  uint32_t* in_len;               // a text of sg_deflate_bgzf: the caller's lengths ...
  uint64_t* in_off;               // ... and their scan
  uint32_t* hist;
  uint64_t* hist_off;
  uint64_t* bsum;
};

int carve_work(sg_ctx* ctx, uint32_t m, uint32_t n_in, IndexWork* W) {
  const uint32_t n_hist = sg::kSortDigits * sg::bamsort_blocks(m);
  return sg_carve(ctx, ctx->bamindex.work, [&](SgArena& a) {
    W->counters = a.take<unsigned long long>(8);
    W->rows = a.take<sg::BaiRow>(m);
    W->voff = a.take<uint64_t>(m);
    W->head = a.take<uint32_t>(m);
    W->rank = a.take<uint64_t>(m);
    W->cbeg = a.take<uint64_t>(m);
    W->cend = a.take<uint64_t>(m);
    W->in_len = a.take<uint32_t>(n_in);
    W->in_off = a.take<uint64_t>(n_in);
    W->hist = a.take<uint32_t>(n_hist);
    W->hist_off = a.take<uint64_t>(n_hist);
    W->bsum = a.take<uint64_t>((size_t)sg::scan_blocks(std::max(std::max(m, n_in), n_hist)) + 8);
  });
}

int need_index(sg_ctx* ctx, const char* who) {
  if (int rc = sg_need_begun(ctx, ctx && ctx->bamindex.on, who, "sg_bamindex_begin")) return rc;
  if (ctx->bamindex.broken) return ctx->fail(SG_ERR_INVALID, std::string(who) + ": an earlier sg_bamindex_add failed; call sg_bamindex_begin again");
  return SG_OK;
}

}  // namespace

extern "C" {

int sg_bamindex_begin(sg_ctx* ctx, uint32_t n_ref, const uint64_t* ref_len) {
  if (!ctx) return SG_ERR_INVALID;
  if (n_ref && !ref_len) return ctx->fail(SG_ERR_INVALID, "sg_bamindex_begin: null reference lengths");
  if (n_ref >= 0x7FFFFFFFu) return ctx->fail(SG_ERR_UNSUPPORTED, "sg_bamindex_begin: 2^31 references or more");
  for (uint32_t r = 0; r < n_ref; r++)
    if (ref_len[r] > sg::kBaiMaxLen)
      return ctx->fail(SG_ERR_UNSUPPORTED, "sg_bamindex_begin: reference " + std::to_string(r) + " is longer than 2^29 bases, which a BAI cannot address");
  SG_HIP(hipSetDevice(ctx->device));
  sg_ctx::BamIndex& B = ctx->bamindex;
  B.on = B.broken = false;
  B.n_chunks = 0;
  B.carry_have = B.carry_need = 0;
  B.ref_len.assign(ref_len, ref_len + n_ref);
  std::vector<sg::BaiRef> refs(n_ref);
  uint64_t n_win = 0;
  for (uint32_t r = 0; r < n_ref; r++) {
    refs[r] = sg::BaiRef{n_win, ref_len[r]};
    n_win += (ref_len[r] + (1u << sg::kBaiShift) - 1) >> sg::kBaiShift;
  }
  B.n_win = n_win;
  std::vector<uint64_t> counts((size_t)3 * n_ref + 1, 0);
  for (uint32_t r = 0; r < n_ref; r++) counts[(size_t)3 * r + 2] = ~0ull;
  SG_ENSURE(B.refs, (size_t)n_ref * sizeof(sg::BaiRef) + 64);
  SG_ENSURE(B.linear, (size_t)n_win * 8 + 64);
  SG_ENSURE(B.counts, counts.size() * 8 + 64);
  hipStream_t s = ctx->stream;
  if (n_ref) SG_HIP(hipMemcpyAsync(B.refs.p, refs.data(), (size_t)n_ref * sizeof(sg::BaiRef), hipMemcpyHostToDevice, s));
  SG_HIP(hipMemcpyAsync(B.counts.p, counts.data(), counts.size() * 8, hipMemcpyHostToDevice, s));
  sg::launch_bamindex_fill(B.linear.as<unsigned long long>(), n_win, s);
  SG_HIP(hipGetLastError());
  SG_HIP(hipStreamSynchronize(s));   // refs and counts are host-owned
  B.on = true;
  return SG_OK;
}

int sg_bamindex_add(sg_ctx* ctx, int source, uint64_t file_offset, uint64_t skip, const uint32_t* lens, uint64_t n, uint64_t* n_chunks,
                    uint64_t* first_voff) {
  if (int rc = need_index(ctx, "sg_bamindex_add")) return rc;
  sg_ctx::BamIndex& B = ctx->bamindex;
  const sg_ctx::BamSort& S = ctx->bamsort;
  if (n_chunks) *n_chunks = 0;
  if (first_voff) *first_voff = ~0ull;
  B.n_chunks = 0;
  if (file_offset >> 47) return ctx->fail(SG_ERR_UNSUPPORTED, "sg_bamindex_add: a file offset of 2^47 or more");
  sg::BaiJob J;
  memset(&J, 0, sizeof J);
  uint64_t n_whole = 0, tail_at = 0;   // records that lie whole in the text; where the one that runs past it starts
  uint32_t tail_len = 0;               // ... and its length (0: none)
  if (source == SG_BAMINDEX_MERGE) {
    if (!S.have) return ctx->fail(SG_ERR_INVALID, "sg_bamindex_add: call sg_bamsort_merge first");
    if (lens || skip) return ctx->fail(SG_ERR_INVALID, "sg_bamindex_add: a merge brings its own lengths and has nothing to skip");
    if (B.carry_have) return ctx->fail(SG_ERR_INVALID, "sg_bamindex_add: the record the last text left unfinished does not end in a merge");
    n_whole = S.n;
    if (n_whole) {
      if (!S.dst_off || ctx->gz_last.text != S.out.as<uint8_t>() || ctx->gz_last.bytes != S.out_bytes)
        return ctx->fail(SG_ERR_INVALID, "sg_bamindex_add: the merge is not the context's latest compression");
      J.text = S.out.as<uint8_t>();
      J.bytes = S.out_bytes;
      J.off = S.dst_off;
      J.len = S.lens.as<uint32_t>();
    }
  } else if (source == SG_BAMINDEX_DEFLATE) {
    if (!ctx->gz_last.text || ctx->gz_last.text != ctx->defl_src.as<uint8_t>())
      return ctx->fail(SG_ERR_INVALID, "sg_bamindex_add: sg_deflate_bgzf is not the context's latest compression");
    if (n && !lens) return ctx->fail(SG_ERR_INVALID, "sg_bamindex_add: null lengths");
    if (n >= 0xFFFFFFF0ull) return ctx->fail(SG_ERR_UNSUPPORTED, "sg_bamindex_add: 2^32 records or more");
    J.text = ctx->gz_last.text;
    J.bytes = ctx->gz_last.bytes;
    if (skip > J.bytes) return ctx->fail(SG_ERR_UNSUPPORTED, "sg_bamindex_add: a record that spans a whole text");
    if (B.carry_have && skip != B.carry_need)
      return ctx->fail(SG_ERR_INVALID, "sg_bamindex_add: `skip` is not the rest of the record the last text left unfinished");
    uint64_t at = skip;
    n_whole = n;
    for (uint64_t i = 0; i < n; i++) {
      if (at >= J.bytes) return ctx->fail(SG_ERR_INVALID, "sg_bamindex_add: record " + std::to_string(i) + " does not start in the text");
      if (lens[i] > J.bytes - at) {
        if (i + 1 != n) return ctx->fail(SG_ERR_INVALID, "sg_bamindex_add: only the last record may run past the text");
        n_whole = n - 1;
        tail_at = at;
        tail_len = lens[i];
      }
      at += lens[i];
    }
    J.skip = skip;
  } else return ctx->fail(SG_ERR_INVALID, "sg_bamindex_add: unknown source");
  const uint32_t carried = B.carry_have ? 1u : 0u;
  if (n_whole + carried >= 0xFFFFFFF0ull) return ctx->fail(SG_ERR_UNSUPPORTED, "sg_bamindex_add: 2^32 records or more");
  const uint32_t m = (uint32_t)n_whole + carried, n_ref = (uint32_t)B.ref_len.size();
  SG_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  uint64_t first = ~0ull;
  if (m) {
    IndexWork W;
    if (int rc = carve_work(ctx, m, source == SG_BAMINDEX_DEFLATE ? (uint32_t)n_whole : 0u, &W)) return rc;
    for (int i = 0; i < 2; i++) {
      SG_ENSURE(B.keys[i], (size_t)m * 8 + 64);
      SG_ENSURE(B.vals[i], (size_t)m * 4 + 64);
    }
    SG_ENSURE(B.chunks, (size_t)m * sizeof(sg_bai_chunk) + 64);
    SG_HIP(hipMemsetAsync(W.counters, 0, 64, s));
    if (source == SG_BAMINDEX_DEFLATE && n_whole) {
      SG_HIP(hipMemcpyAsync(W.in_len, lens, n_whole * 4, hipMemcpyHostToDevice, s));
      sg::launch_scan_u32(W.in_len, (uint32_t)n_whole, W.bsum, W.in_off, (uint64_t*)&W.counters[7], s);
      J.off = W.in_off;
      J.len = W.in_len;
    }
    if (carried) {   // the rest of the unfinished record is the text's front
      if (B.carry_need) SG_HIP(hipMemcpyAsync(B.carry.as<uint8_t>() + B.carry_have, J.text, B.carry_need, hipMemcpyDeviceToDevice, s));
      J.carry = B.carry.as<uint8_t>();
      J.carry_len = B.carry_have + B.carry_need;
      J.carried = 1;
      J.carry_voff = B.carry_voff;
    }
    J.moff = ctx->gz_last.moff;
    J.file_off = file_offset;
    J.m = m;
    J.refs = B.refs.as<sg::BaiRef>();
    J.n_ref = n_ref;
    B.cur = 0;
    sg::launch_bamindex_rows(J, W.rows, W.voff, B.linear.as<unsigned long long>(), B.counts.as<unsigned long long>(), &W.counters[0], s);
    sg::launch_bamindex_heads(W.rows, m, n_ref, W.head, s);
    sg::launch_scan_u32(W.head, m, W.bsum, W.rank, (uint64_t*)&W.counters[1], s);
    sg::launch_bamindex_compact(W.rows, W.voff, W.head, W.rank, (const uint64_t*)&W.counters[1], m, n_ref, B.keys[0].as<uint64_t>(), W.cbeg, W.cend,
                                B.vals[0].as<uint32_t>(), &W.counters[2], s);
    uint64_t c[3] = {};
    B.broken = true;   // until the call is through: the stem's linear index and counts may hold a part of it
    if (int rc = sg_read_back(ctx, c, W.counters, sizeof c)) return rc;
    if (c[0] & sg::kBaiBadOffset) return ctx->fail(SG_ERR_INVALID, "sg_bamindex_add: a record outside the text");
    if (c[0] & sg::kBaiBadRecord) return ctx->fail(SG_ERR_INVALID, "sg_bamindex_add: a record whose name and CIGAR do not fit its length");
    if (c[0] & sg::kBaiBadPlace) return ctx->fail(SG_ERR_INVALID, "sg_bamindex_add: a record outside its reference");
    if (!c[1] || c[1] > m || c[2] > c[1]) return ctx->fail(SG_ERR_INVALID, "sg_bamindex_add: the chunk count does not fit the records");
    if (int rc = sg_read_back(ctx, &first, W.voff, 8)) return rc;
    const uint32_t n_all = (uint32_t)c[1];
    uint64_t ref_mask = 1;
    while (ref_mask <= n_ref) ref_mask <<= 1;
    if (int rc = bamsort_sort_pairs(ctx, SgSortBufs{B.keys, B.vals, &B.cur, W.hist, W.hist_off, W.bsum, (uint64_t*)&W.counters[7]}, n_all,
                                    ((ref_mask - 1) << 32) | 0xFFFFull, 0))
      return rc;
    sg::launch_bamindex_gather(B.keys[B.cur].as<uint64_t>(), B.vals[B.cur].as<uint32_t>(), W.cbeg, W.cend, n_all, B.chunks.as<uint64_t>(), s);
    SG_HIP(hipGetLastError());
    SG_HIP(hipStreamSynchronize(s));
    B.n_chunks = c[1] - c[2];   // the chunks of refID -1 have the largest key: they are the last rows and are left out
    B.broken = false;
  }
  B.carry_have = B.carry_need = 0;
  if (tail_len) {   // the record that runs past the text waits in `carry` for the next text
    const uint32_t have = (uint32_t)(J.bytes - tail_at);
    uint64_t mo = 0;
    SG_ENSURE(B.carry, (size_t)tail_len + 64);
    SG_HIP(hipMemsetAsync(B.carry.p, 0, (size_t)tail_len + 64, s));
    SG_HIP(hipMemcpyAsync(B.carry.p, J.text + tail_at, have, hipMemcpyDeviceToDevice, s));
    if (int rc = sg_read_back(ctx, &mo, ctx->gz_last.moff + (tail_at >> 15), 8)) return rc;
    B.carry_have = have;
    B.carry_need = tail_len - have;
    B.carry_voff = ((file_offset + mo) << 16) | (tail_at & 32767u);
  }
  if (n_chunks) *n_chunks = B.n_chunks;
  if (first_voff) *first_voff = first;
  return SG_OK;
}

int sg_bamindex_chunks(sg_ctx* ctx, sg_bai_chunk* rows, uint64_t cap, uint64_t* n) {
  if (!n) return SG_ERR_INVALID;
  if (int rc = need_index(ctx, "sg_bamindex_chunks")) return rc;
  const sg_ctx::BamIndex& B = ctx->bamindex;
  *n = B.n_chunks;
  if (!rows) return SG_OK;
  if (B.n_chunks > cap) return ctx->fail(SG_ERR_OVERFLOW, "sg_bamindex_chunks: the rows do not fit cap");
  SG_HIP(hipSetDevice(ctx->device));
  if (B.n_chunks) {
    SG_HIP(hipMemcpyAsync(rows, B.chunks.p, B.n_chunks * sizeof(sg_bai_chunk), hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipStreamSynchronize(ctx->stream));
  }
  return SG_OK;
}

int sg_bamindex_finish(sg_ctx* ctx, uint64_t* linear, uint64_t cap, uint64_t* counts) {
  if (int rc = need_index(ctx, "sg_bamindex_finish")) return rc;
  const sg_ctx::BamIndex& B = ctx->bamindex;
  if (B.carry_have) return ctx->fail(SG_ERR_INVALID, "sg_bamindex_finish: the last text left a record unfinished");
  if ((B.n_win && !linear) || !counts) return ctx->fail(SG_ERR_INVALID, "sg_bamindex_finish: null tables");
  if (B.n_win > cap) return ctx->fail(SG_ERR_OVERFLOW, "sg_bamindex_finish: the linear index does not fit cap");
  SG_HIP(hipSetDevice(ctx->device));
  if (B.n_win) SG_HIP(hipMemcpyAsync(linear, B.linear.p, B.n_win * 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipMemcpyAsync(counts, B.counts.p, (B.ref_len.size() * 3 + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

int sg_bamindex_end(sg_ctx* ctx) {
  if (!ctx) return SG_ERR_INVALID;
  ctx->bamindex = sg_ctx::BamIndex();
  return SG_OK;
}

}  // extern "C"
