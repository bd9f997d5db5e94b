// sg_api_vcf.cpp -- the C ABI of the VCF input (kernels: sg_vcf.hip; the rule: sg_vcf.h).  A session lives in ctx->vcf from
// sg_vcf_begin to sg_vcf_end.  A feed is synchronous: when it returns, its rows are in place and its undecided fragments
// can be fetched.  Nothing of a call is committed before its last step has succeeded.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "sg_api.h"
#include "sg_bam.h"
#include "sg_scan.h"
#include "sg_vcf.h"

namespace {

constexpr uint64_t kVcfMaxCall = 1ull << 30;    // bytes of text a call may bring
constexpr uint64_t kVcfMaxLine = 64ull << 20;   // bytes of a line, finished or left unfinished by a call

// a device buffer grown with what it holds kept
int vcf_grow_keep(sg_ctx* ctx, DevBuf& buf, size_t keep_bytes, size_t want_bytes) {
  if (want_bytes <= buf.cap) return SG_OK;
  DevBuf bigger;
  SG_ENSURE(bigger, want_bytes + want_bytes / 2);
  if (keep_bytes) SG_HIP(hipMemcpyAsync(bigger.p, buf.p, keep_bytes, hipMemcpyDeviceToDevice, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  buf = std::move(bigger);
  return SG_OK;
}

int vcf_pack_keys(const char* const* contig_keys, uint32_t n, std::vector<char>& keys) {
  keys.assign((size_t)std::max<uint32_t>(n, 1) * sg::kVcfKeyBytes, 0);
  for (uint32_t c = 0; c < n; c++) {
    if (!contig_keys[c]) return SG_ERR_INVALID;
    if (strlen(contig_keys[c]) >= sg::kVcfKeyBytes) return SG_ERR_UNSUPPORTED;
    strcpy(&keys[(size_t)c * sg::kVcfKeyBytes], contig_keys[c]);
  }
  return SG_OK;
}

// The kernels over text[cur][0, L): the carried line and `fresh` new bytes behind it.  Commits the call.
int vcf_run(sg_ctx* ctx, uint64_t L, bool final_call, uint64_t fresh, const char* who) {
  sg_ctx::Vcf& V = ctx->vcf;
  hipStream_t s = ctx->stream;
  if (L >= (1ull << 31)) return ctx->fail(SG_ERR_INVALID, std::string(who) + ": more than 2 GiB of text in one call: feed less at a time");
  uint64_t info[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t firsts[11];
  uint64_t n_first = 0;
  uint64_t tail = 0;
  const sg_vcf_fragment* und_list = nullptr;
  if (L) {
    sg::VcfJob J;
    memset(&J, 0, sizeof J);
    J.text = V.text[V.cur].as<char>();
    J.bytes = L;
    J.final_call = final_call ? 1u : 0u;
    J.first_number = V.fragments;
    J.keys = V.keys.as<char>();
    J.n_keys = V.n_keys;
    J.n_blocks = (uint32_t)((L + 63) / 64);
    SG_ENSURE(V.info, 16 * 8 + 64);
    J.info = V.info.as<uint64_t>();
    SG_HIP(hipMemsetAsync(J.info, 0, 16 * 8, s));
    // ---- line breaks ----
    int rc = sg_carve(ctx, V.work, [&](SgArena& a) {
      J.block_breaks = a.take<uint32_t>(J.n_blocks);
      J.block_first = a.take<uint64_t>(J.n_blocks);
    });
    if (rc != SG_OK) return rc;
    SG_ENSURE(V.scan, (size_t)(sg::scan_blocks(J.n_blocks) + 1) * 8 + 64);
    sg::launch_vcf_breaks(J, s);
    sg::launch_scan_u32(J.block_breaks, J.n_blocks, V.scan.as<uint64_t>(), J.block_first, J.info + 0, s);
    if ((rc = sg_read_back(ctx, info, J.info, 8)) != SG_OK) return rc;
    // ---- lines and their fragments (one line more than line breaks: the last one of the text may have none) ----
    J.n_lines = (uint32_t)info[0] + 1;
    rc = sg_carve(ctx, V.lines, [&](SgArena& a) {
      J.line_stop = a.take<uint64_t>(J.n_lines);
      J.frag_count = a.take<uint32_t>(J.n_lines);
      J.frag_first = a.take<uint64_t>(J.n_lines);
    });
    if (rc != SG_OK) return rc;
    SG_ENSURE(V.scan, (size_t)(sg::scan_blocks(J.n_lines) + 1) * 8 + 64);
    sg::launch_vcf_lines(J, s);
    sg::launch_vcf_frag_count(J, s);
    sg::launch_scan_u32(J.frag_count, J.n_lines, V.scan.as<uint64_t>(), J.frag_first, J.info + 3, s);
    if ((rc = sg_read_back(ctx, info, J.info, 16 * 8)) != SG_OK) return rc;
    tail = info[2];
    if (tail > L || info[1] > J.n_lines) return ctx->fail(SG_ERR_INVALID, std::string(who) + ": internal: line table out of range");
    if ((info[12] >> 32) > kVcfMaxLine)   // (a finished line: one lane would walk all its fragments)
      return ctx->fail(SG_ERR_INVALID, std::string(who) + ": the line at text offset " + std::to_string(V.text_off + (info[12] & 0xFFFFFFFFull)) +
                                           " is longer than 64 MiB");
    if (L - tail > kVcfMaxLine)
      return ctx->fail(SG_ERR_INVALID, std::string(who) + ": the line at text offset " + std::to_string(V.text_off + tail) +
                                           " is longer than 64 MiB: it does not fit one call's text");
    if (info[3] >= (1ull << 32)) return ctx->fail(SG_ERR_INVALID, std::string(who) + ": too many fragments in one call");
    J.n_frags = (uint32_t)info[3];
    if (J.n_frags) {
      // ---- verdicts, the five lists ----
      const size_t nf = J.n_frags;
      rc = sg_carve(ctx, V.frags, [&](SgArena& a) {
        J.frag_start = a.take<uint64_t>(nf);
        J.frag_len = a.take<uint32_t>(nf);
        J.rows = a.take<sg_vcf_record>(nf);
        for (int k = 0; k < 5; k++) J.flag[k] = a.take<uint32_t>(nf);
        for (int k = 0; k < 5; k++) J.slot[k] = a.take<uint64_t>(nf);
      });
      if (rc != SG_OK) return rc;
      SG_ENSURE(V.scan, (size_t)(sg::scan_blocks(J.n_frags) + 1) * 8 + 64);
      sg::launch_vcf_rows(J, s);
      for (int k = 0; k < 5; k++) sg::launch_scan_u32(J.flag[k], J.n_frags, V.scan.as<uint64_t>(), J.slot[k], J.info + 4 + k, s);
      if ((rc = sg_read_back(ctx, info, J.info, 16 * 8)) != SG_OK) return rc;
      for (int k = 0; k < 5; k++)
        if (info[4 + k] > nf) return ctx->fail(SG_ERR_INVALID, std::string(who) + ": internal: list longer than the fragments");
      for (int k = 0; k < 3; k++) {
        if ((rc = vcf_grow_keep(ctx, V.rows[k], V.kept[k] * sizeof(sg_vcf_record), (V.kept[k] + info[4 + k]) * sizeof(sg_vcf_record) + 64)) != SG_OK) return rc;
        J.out[k] = V.rows[k].as<sg_vcf_record>();
        J.out_first[k] = V.kept[k];
      }
      rc = sg_carve(ctx, V.lists, [&](SgArena& a) {
        J.malformed = a.take<uint64_t>(info[7] + 1);
        J.undecided = a.take<sg_vcf_fragment>(info[8] + 1);
      });
      if (rc != SG_OK) return rc;
      sg::launch_vcf_compact(J, s);
      n_first = std::min<uint64_t>(info[7], 11 - std::min<uint64_t>(V.malformed, 11));
      if ((rc = sg_read_back(ctx, firsts, J.malformed, std::max<uint64_t>(n_first, 1) * 8)) != SG_OK) return rc;
      und_list = J.undecided;
    }
    // ---- the unfinished line leads the next call ----
    const uint64_t left = L - tail;
    DevBuf& N = V.text[V.cur ^ 1];
    SG_ENSURE(N, left + 64);
    if (left) SG_HIP(hipMemcpyAsync(N.p, V.text[V.cur].as<char>() + tail, left, hipMemcpyDeviceToDevice, s));
    SG_HIP(hipStreamSynchronize(s));
    V.cur ^= 1;
    V.carry = left;
    V.text_off += tail;
  }
  for (uint64_t i = 0; i < n_first; i++) V.malformed_first[std::min<uint64_t>(V.malformed, 11) + i] = firsts[i];
  V.fragments += info[3];
  for (int k = 0; k < 3; k++) { V.kept[k] += info[4 + k]; V.n_kind[k] += info[9 + k]; }
  V.malformed += info[7];
  V.undecided += info[8];
  V.last_undecided = info[8];
  V.last_list = und_list;
  V.text_bytes += fresh;
  if (final_call) V.finished = true;
  return SG_OK;
}

int vcf_need(sg_ctx* ctx, const char* who, bool feeding) {
  if (!ctx) return SG_ERR_INVALID;
  const int rc = sg_need_begun(ctx, ctx->vcf.on, who, "sg_vcf_begin");
  if (rc != SG_OK) return rc;
  if (feeding && ctx->vcf.finished) return ctx->fail(SG_ERR_INVALID, std::string(who) + ": the text has been finished (sg_vcf_finish)");
  return SG_OK;
}

}  // namespace

extern "C" {

int sg_vcf_begin(sg_ctx* ctx, const char* const* contig_keys, uint32_t n_contigs) {
  if (!ctx || (n_contigs && !contig_keys)) return SG_ERR_INVALID;
  if (ctx->vcf.on) return ctx->fail(SG_ERR_INVALID, "sg_vcf_begin: a session is open: call sg_vcf_end first");
  std::vector<char> keys;
  const int rc = vcf_pack_keys(contig_keys, n_contigs, keys);
  if (rc == SG_ERR_UNSUPPORTED) return ctx->fail(rc, "sg_vcf_begin: contig name too long");
  if (rc != SG_OK) return rc;
  SG_HIP(hipSetDevice(ctx->device));
  sg_ctx::Vcf V;
  SG_ENSURE(V.keys, keys.size() + 64);
  SG_ENSURE(V.text[0], 64);
  SG_HIP(hipMemcpy(V.keys.p, keys.data(), keys.size(), hipMemcpyHostToDevice));
  V.on = true;
  V.n_keys = n_contigs;
  ctx->vcf = std::move(V);
  return SG_OK;
}

int sg_vcf_feed(sg_ctx* ctx, const char* text, uint64_t bytes) {
  int rc = vcf_need(ctx, "sg_vcf_feed", true);
  if (rc != SG_OK) return rc;
  if (bytes && !text) return SG_ERR_INVALID;
  if (bytes > kVcfMaxCall) return ctx->fail(SG_ERR_INVALID, "sg_vcf_feed: more than 1 GiB of text in one call");
  sg_ctx::Vcf& V = ctx->vcf;
  V.last_undecided = 0;
  if (!bytes) return SG_OK;
  SG_HIP(hipSetDevice(ctx->device));
  const uint64_t L = V.carry + bytes;
  if ((rc = vcf_grow_keep(ctx, V.text[V.cur], V.carry, L + 64)) != SG_OK) return rc;
  SG_HIP(hipMemcpyAsync(V.text[V.cur].as<char>() + V.carry, text, bytes, hipMemcpyHostToDevice, ctx->stream));
  return vcf_run(ctx, L, false, bytes, "sg_vcf_feed");
}

int sg_vcf_feed_bgzf(sg_ctx* ctx, const void* members, uint64_t bytes) {
  int rc = vcf_need(ctx, "sg_vcf_feed_bgzf", true);
  if (rc != SG_OK) return rc;
  if (bytes && !members) return SG_ERR_INVALID;
  sg_ctx::Vcf& V = ctx->vcf;
  V.last_undecided = 0;
  if (!bytes) return SG_OK;
  SG_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  std::vector<sg::InflateMember> mem;
  uint64_t n = 0, whole = 0, total = 0;
  std::string err;
  if (bgzf_walk((const uint8_t*)members, bytes, V.file_off, ~0ull, &mem, &n, &whole, &err) != SG_OK)
    return ctx->fail(SG_ERR_INVALID, "sg_vcf_feed_bgzf: " + err);
  if (whole != bytes)
    return ctx->fail(SG_ERR_INVALID, "sg_vcf_feed_bgzf: BGZF member at file offset " + std::to_string(V.file_off + whole) +
                                         " is cut short (truncated file?)");
  for (sg::InflateMember& m : mem) { m.dst += V.carry; total += m.isize; }
  const uint64_t L = V.carry + total;
  if (L >= (1ull << 31)) return ctx->fail(SG_ERR_INVALID, "sg_vcf_feed_bgzf: more than 2 GiB of text in one call: feed fewer members at a time");
  SG_ENSURE(V.src, bytes + 64);
  SG_HIP(hipMemcpyAsync(V.src.p, members, bytes, hipMemcpyHostToDevice, s));
  if ((rc = vcf_grow_keep(ctx, V.text[V.cur], V.carry, L + 64)) != SG_OK) return rc;
  if (n) {
    if ((rc = inflate_launch(ctx, V.src.as<uint8_t>(), bytes, mem, V.meta, V.text[V.cur].as<uint8_t>(), s, s)) != SG_OK) return rc;
    SG_HIP(hipStreamSynchronize(s));
    if ((rc = inflate_verdicts(ctx, mem, V.meta, "sg_vcf_feed_bgzf")) != SG_OK) return rc;
  }
  if ((rc = vcf_run(ctx, L, false, total, "sg_vcf_feed_bgzf")) != SG_OK) return rc;
  V.file_off += bytes;
  return SG_OK;
}

int sg_vcf_undecided(sg_ctx* ctx, sg_vcf_fragment* rows, uint64_t cap, uint64_t* n, char* bytes, uint64_t bytes_cap, uint64_t* n_bytes) {
  int rc = vcf_need(ctx, "sg_vcf_undecided", false);
  if (rc != SG_OK) return rc;
  if (!n || !n_bytes) return SG_ERR_INVALID;
  sg_ctx::Vcf& V = ctx->vcf;
  *n = V.last_undecided;
  *n_bytes = 0;
  if (!V.last_undecided) return SG_OK;
  SG_HIP(hipSetDevice(ctx->device));
  std::vector<sg_vcf_fragment> list(V.last_undecided);
  SG_HIP(hipMemcpy(list.data(), V.last_list, list.size() * sizeof(sg_vcf_fragment), hipMemcpyDeviceToHost));
  uint64_t need = 0, lo = ~0ull, hi = 0;
  for (const sg_vcf_fragment& f : list) { need += f.len; lo = std::min(lo, f.offset); hi = std::max(hi, f.offset + f.len); }
  *n_bytes = need;
  if (list.size() > cap || need > bytes_cap) return ctx->fail(SG_ERR_OVERFLOW, "sg_vcf_undecided: the fragments do not fit cap / bytes_cap");
  if (!rows || !bytes) return SG_ERR_INVALID;
  // (the text of the last feed is in the buffer the carried line was copied out of)
  const char* text = V.text[V.cur ^ 1].as<char>();
  if (hi > V.text[V.cur ^ 1].cap) return ctx->fail(SG_ERR_INVALID, "sg_vcf_undecided: internal: fragment outside the text");
  std::vector<char> span;
  if (list.size() > 32) {
    span.resize(hi - lo);
    SG_HIP(hipMemcpy(span.data(), text + lo, hi - lo, hipMemcpyDeviceToHost));
  }
  uint64_t at = 0;
  for (size_t i = 0; i < list.size(); i++) {
    if (span.empty()) SG_HIP(hipMemcpy(bytes + at, text + list[i].offset, list[i].len, hipMemcpyDeviceToHost));
    else memcpy(bytes + at, span.data() + (list[i].offset - lo), list[i].len);
    rows[i] = sg_vcf_fragment{list[i].number, at, list[i].len, 0u};
    at += list[i].len;
  }
  return SG_OK;
}

int sg_vcf_finish(sg_ctx* ctx, sg_vcf_counts* counts) {
  int rc = vcf_need(ctx, "sg_vcf_finish", false);
  if (rc != SG_OK) return rc;
  if (!counts) return SG_ERR_INVALID;
  sg_ctx::Vcf& V = ctx->vcf;
  if (!V.finished) {
    SG_HIP(hipSetDevice(ctx->device));
    V.last_undecided = 0;
    if ((rc = vcf_run(ctx, V.carry, true, 0, "sg_vcf_finish")) != SG_OK) return rc;
  }
  memset(counts, 0, sizeof *counts);
  counts->fragments = V.fragments;
  counts->n_snv = V.n_kind[0]; counts->n_ins = V.n_kind[1]; counts->n_del = V.n_kind[2];
  counts->kept_snv = V.kept[0]; counts->kept_ins = V.kept[1]; counts->kept_del = V.kept[2];
  counts->malformed = V.malformed;
  for (uint64_t i = 0; i < std::min<uint64_t>(V.malformed, 11); i++) counts->malformed_first[i] = V.malformed_first[i];
  counts->undecided = V.undecided;
  counts->text_bytes = V.text_bytes;
  return SG_OK;
}

int sg_vcf_rows(sg_ctx* ctx, uint32_t kind, uint64_t first, uint64_t n, sg_vcf_record* rows) {
  const int rc = vcf_need(ctx, "sg_vcf_rows", false);
  if (rc != SG_OK) return rc;
  if (kind < SG_VCF_SNV || kind > SG_VCF_DEL) return ctx->fail(SG_ERR_INVALID, "sg_vcf_rows: kind is SG_VCF_SNV, SG_VCF_INS or SG_VCF_DEL");
  sg_ctx::Vcf& V = ctx->vcf;
  const int k = (int)kind - 1;
  if (!sg_range_within(first, n, V.kept[k])) return ctx->fail(SG_ERR_INVALID, "sg_vcf_rows: rows outside those kept");
  if (!n) return SG_OK;
  if (!rows) return SG_ERR_INVALID;
  const hipError_t e = sg_fetch_bytes(ctx->device, ctx->stream, rows, V.rows[k].as<sg_vcf_record>() + first, n * sizeof(sg_vcf_record));
  return e == hipSuccess ? SG_OK : ctx->hipfail(e, "sg_vcf_rows");
}

int sg_vcf_end(sg_ctx* ctx) {
  if (!ctx) return SG_ERR_INVALID;
  if (!ctx->vcf.on) return SG_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  ctx->vcf = sg_ctx::Vcf();
  return SG_OK;
}

int sg_vcf_row(const char* fragment, uint32_t len, const char* const* contig_keys, uint32_t n_contigs, sg_vcf_record* row) {
  if (!fragment || !row || len < 1 || len > sg::kVcfFragment || (n_contigs && !contig_keys)) return SG_ERR_INVALID;
  std::vector<char> keys;
  const int rc = vcf_pack_keys(contig_keys, n_contigs, keys);
  if (rc != SG_OK) return rc;
  row->fragment = 0;
  sg::vcf_decide(fragment, len, keys.data(), n_contigs, row);
  return SG_OK;
}

}  // extern "C"
