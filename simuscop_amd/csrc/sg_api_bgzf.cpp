// sg_api_bgzf.cpp -- BGZF / BAM input on the device (kernels: sg_inflate.hip, sg_bam.hip; the member walk: sg_bgzf.h): members
// inflated (inflate_launch, inflate_verdicts), a BAM file fed as whole members (SgBamStream, the bam_stream_* calls) and the
// two calls of the ABI that need no session, sg_bgzf_members and sg_inflate_bgzf.  The training session (sg_api_train.cpp),
// the VCF input (sg_api_vcf.cpp) and the two files of truthEval (sg_api_eval.cpp) come in through here; sg_api.h declares it.
#define SG_BGZF_IMPLEMENTATION   // bgzf_walk is defined here (sg_bgzf.h)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "sg_api.h"
#include "sg_bam.h"
#include "sg_scan.h"

namespace {
const char* inflate_verdict(uint32_t v) {
  static const char* what[] = {"", "block type 3", "over-subscribed, incomplete or unused Huffman code", "distance beyond the output",
                               "DEFLATE data runs past the member", "more than 64 KiB of output", "ISIZE does not match the output",
                               "CRC-32 does not match the output", "stored block length does not match its complement", "header longer than the member"};
  return v < sizeof what / sizeof what[0] ? what[v] : "malformed";
}
const char* bam_verdict(uint32_t v) {
  switch (v) {
    case sg::kBamShort: return "block_size smaller than its fixed fields";
    case sg::kBamOpCode: return "CIGAR operation code above 8";
    case sg::kBamRefId: return "reference id outside the header's list";
    default: return "l_read_name of 0 or a negative l_seq";
  }
}

}  // namespace

// Members of `src` (already on the device) inflated to d_out + member.dst; the verdicts land in meta behind the member table.
int inflate_launch(sg_ctx* ctx, const uint8_t* d_src, uint64_t src_bytes, const std::vector<sg::InflateMember>& mem, DevBuf& meta, uint8_t* d_out,
                   hipStream_t s, hipStream_t copy) {
  if (!ctx->infl_crc.p) {
    SG_ENSURE(ctx->infl_crc, (256 + sg::kCrcLevels * 128) * 4);
    SG_HIP(hipMemcpy(ctx->infl_crc.p, sg::inflate_crc_tab(), 256 * 4, hipMemcpyHostToDevice));
    SG_HIP(hipMemcpy(ctx->infl_crc.as<uint32_t>() + 256, sg::inflate_crc_shift(), sg::kCrcLevels * 128 * 4, hipMemcpyHostToDevice));
  }
  const size_t tab = mem.size() * sizeof(sg::InflateMember);
  SG_ENSURE(meta, tab + mem.size() * 4 + 64);
  SG_HIP(hipMemcpyAsync(meta.p, mem.data(), tab, hipMemcpyHostToDevice, copy));
  SG_HIP(hipStreamSynchronize(copy));
  sg::InflateJob J;
  J.src = d_src;
  J.src_bytes = src_bytes;
  J.members = meta.as<sg::InflateMember>();
  J.n = (uint32_t)mem.size();
  J.out = d_out;
  J.status = (uint32_t*)(meta.as<uint8_t>() + tab);
  J.crc_tab = ctx->infl_crc.as<uint32_t>();
  J.crc_shift = J.crc_tab + 256;
  sg::launch_inflate(J, s);
  SG_HIP(hipGetLastError());
  return SG_OK;
}
// the verdicts of inflate_launch (after the stream has been synchronised); the first member that failed names the error
int inflate_verdicts(sg_ctx* ctx, const std::vector<sg::InflateMember>& mem, const DevBuf& meta, const char* who) {
  std::vector<uint32_t> st(mem.size());
  if (mem.empty()) return SG_OK;
  SG_HIP(hipMemcpy(st.data(), meta.as<uint8_t>() + mem.size() * sizeof(sg::InflateMember), mem.size() * 4, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < mem.size(); i++)
    if (st[i])
      return ctx->fail(SG_ERR_INVALID, std::string(who) + ": BGZF member at file offset " + std::to_string(mem[i].file_off) + ": " + inflate_verdict(st[i]));
  return SG_OK;
}

// ---- SgBamStream (sg_api.h): what sg_train_feed_bgzf and the sg_eval_*_bgzf calls share ----
int bam_stream_start(sg_ctx* ctx, SgBamStream& B, const char* const* ref_names, uint32_t n_ref, uint64_t first_record_skip) {
  std::string names;
  std::vector<uint64_t> off(n_ref + 1, 0);
  for (uint32_t i = 0; i < n_ref; i++) {
    if (ref_names && !ref_names[i]) return SG_ERR_INVALID;
    off[i] = names.size();
    if (ref_names) names += ref_names[i];
    names += '\0';
  }
  off[n_ref] = names.size();
  SG_ENSURE(B.names, names.size() + 64);
  SG_ENSURE(B.name_off, off.size() * 8 + 64);
  if (!names.empty()) SG_HIP(hipMemcpy(B.names.p, names.data(), names.size(), hipMemcpyHostToDevice));
  SG_HIP(hipMemcpy(B.name_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice));
  SG_ENSURE(B.totals, 64);
  B.n_ref = n_ref;
  B.skip = first_record_skip;
  B.carry = B.file_off = B.stream_off = B.records = B.inflated = 0;
  B.scur = 0;
  return SG_OK;
}

int bam_stream_stage(sg_ctx* ctx, SgBamStream& B, const char* who, const void* members, uint64_t bytes, hipStream_t copy) {
  uint64_t n = 0, whole = 0;
  std::string err;
  B.mem.clear();
  B.total = 0;
  if (bgzf_walk((const uint8_t*)members, bytes, B.file_off, ~0ull, &B.mem, &n, &whole, &err) != SG_OK)
    return ctx->fail(SG_ERR_INVALID, std::string(who) + ": " + err);
  if (whole != bytes)
    return ctx->fail(SG_ERR_INVALID, std::string(who) + ": BGZF member at file offset " + std::to_string(B.file_off + whole) +
                                         " is cut short (truncated file?)");
  for (sg::InflateMember& m : B.mem) { m.dst += B.carry; B.total += m.isize; }
  B.bytes = bytes;
  SG_ENSURE(B.src, bytes + 64);
  SG_HIP(hipMemcpyAsync(B.src.p, members, bytes, hipMemcpyHostToDevice, copy));
  return SG_OK;
}

int bam_stream_record_error(sg_ctx* ctx, const SgBamStream& B, const char* who, uint64_t key) {
  return ctx->fail(SG_ERR_INVALID, std::string(who) + ": BAM record at decompressed offset " + std::to_string(B.stream_off + (key >> 8)) + ": " +
                                       bam_verdict((uint32_t)(key & 0xFF)));
}

int bam_stream_records(sg_ctx* ctx, SgBamStream& B, const char* who, hipStream_t s, hipStream_t copy, sg::BamJob* job) {
  const uint64_t carry = B.carry, L = carry + B.total;
  DevBuf& S = B.stream[B.scur];
  int rc;
  if ((rc = sg_grow_keep(ctx, S, carry, L + 64)) != SG_OK) return rc;
  if ((rc = inflate_launch(ctx, B.src.as<uint8_t>(), B.bytes, B.mem, B.meta, S.as<uint8_t>(), s, copy)) != SG_OK) return rc;
  // ---- record boundaries ----
  uint64_t base = 0;
  if (B.skip) {   // (the header: nothing is carried while it lasts)
    base = std::min(B.skip, L);
    B.skip -= base;
  }
  const uint32_t n_seg = L > base ? (uint32_t)((L - base + sg::kBamSegment - 1) / sg::kBamSegment) : 0;
  SG_ENSURE(B.seg, (size_t)n_seg * 28 + 64);
  SG_ENSURE(B.scan, (size_t)(sg::scan_blocks(std::max<uint32_t>(n_seg, 1)) + 1) * 8 + 64);
  sg::BamJob& J = *job;
  memset(&J, 0, sizeof J);
  J.d = S.as<uint8_t>();
  J.base = base;
  J.L = L;
  J.n_ref = B.n_ref;
  J.names = B.names.as<char>();
  J.name_off = B.name_off.as<uint64_t>();
  J.n_seg = n_seg;
  J.guess = B.seg.as<uint64_t>();
  J.exit = J.guess + n_seg;
  J.first = J.exit + n_seg;
  J.count = (uint32_t*)(J.first + n_seg);
  J.scan_bsum = B.scan.as<uint64_t>();
  J.totals = B.totals.as<uint64_t>();
  uint64_t h_tot[4] = {0, 0, base, ~0ull};
  SG_HIP(hipMemcpyAsync(J.totals, h_tot, 32, hipMemcpyHostToDevice, s));
  if (n_seg) {
    sg::launch_bam_guess(J, s);
    sg::launch_bam_verify(J, s);
    sg::launch_scan_u32(J.count, n_seg, J.scan_bsum, J.first, J.totals, s);
  }
  SG_HIP(hipGetLastError());
  SG_HIP(hipMemcpyAsync(h_tot, J.totals, 32, hipMemcpyDeviceToHost, s));
  SG_HIP(hipStreamSynchronize(s));
  if ((rc = inflate_verdicts(ctx, B.mem, B.meta, who)) != SG_OK) return rc;
  if (h_tot[3] != ~0ull) return bam_stream_record_error(ctx, B, who, h_tot[3]);
  const uint64_t n_rec = h_tot[0];
  B.tail = h_tot[2];
  B.L = L;
  B.n_rec = n_rec;
  if (n_rec) {
    SG_ENSURE(B.rec, n_rec * 8 + 64);
    SG_ENSURE(B.scan, (size_t)(sg::scan_blocks((uint32_t)n_rec) + 1) * 8 + 64);
    J.scan_bsum = B.scan.as<uint64_t>();
    J.rec = B.rec.as<uint64_t>();
    J.n_rec = n_rec;
    sg::launch_bam_starts(J, s);
  }
  return SG_OK;
}

int bam_stream_advance(sg_ctx* ctx, SgBamStream& B, hipStream_t s) {
  // the partial record behind the last whole one goes to the front of the other stream buffer
  const uint64_t left = B.L - B.tail;
  DevBuf& S = B.stream[B.scur];
  DevBuf& N = B.stream[B.scur ^ 1];
  SG_ENSURE(N, left + 64);
  if (left) SG_HIP(hipMemcpyAsync(N.p, S.as<uint8_t>() + B.tail, left, hipMemcpyDeviceToDevice, s));
  B.scur ^= 1;
  B.carry = left;
  B.stream_off += B.tail;
  B.file_off += B.bytes;
  B.records += B.n_rec;
  B.inflated += B.total;
  return SG_OK;
}

int bam_stream_close(sg_ctx* ctx, const SgBamStream& B, const char* who) {
  if (B.carry)
    return ctx->fail(SG_ERR_INVALID, std::string(who) + ": the BAM record at decompressed offset " + std::to_string(B.stream_off) +
                                         " runs past the end of the stream");
  return SG_OK;
}

extern "C" {

int sg_bgzf_members(const void* buf, uint64_t bytes, uint64_t* offsets, uint32_t* bsize, uint32_t* isize, uint64_t cap, uint64_t* n_members,
                    uint64_t* whole_bytes) {
  if ((bytes && !buf) || !n_members || !whole_bytes) return SG_ERR_INVALID;
  std::string err;
  const int rc = bgzf_walk((const uint8_t*)buf, bytes, 0, cap, nullptr, n_members, whole_bytes, &err, offsets, bsize, isize);
  if (rc != SG_OK) g_create_error = "sg_bgzf_members: " + err;
  return rc;
}

int sg_inflate_bgzf(sg_ctx* ctx, const void* members, uint64_t bytes, void* out, uint64_t out_cap, uint64_t* out_bytes) {
  if (!ctx || (bytes && !members) || !out_bytes) return SG_ERR_INVALID;
  SG_HIP(hipSetDevice(ctx->device));
  std::vector<sg::InflateMember> mem;
  uint64_t n = 0, whole = 0, total = 0;
  std::string err;
  if (bgzf_walk((const uint8_t*)members, bytes, 0, ~0ull, &mem, &n, &whole, &err) != SG_OK) return ctx->fail(SG_ERR_INVALID, "sg_inflate_bgzf: " + err);
  if (whole != bytes)
    return ctx->fail(SG_ERR_INVALID, "sg_inflate_bgzf: BGZF member at file offset " + std::to_string(whole) + " is cut short by the end of the buffer");
  for (const sg::InflateMember& m : mem) total += m.isize;
  *out_bytes = total;
  if (total > out_cap) return ctx->fail(SG_ERR_OVERFLOW, "sg_inflate_bgzf: the inflated bytes do not fit out_cap");
  if (!n) return SG_OK;
  if (!out) return SG_ERR_INVALID;
  hipStream_t s = ctx->stream;
  SG_ENSURE(ctx->infl_src, bytes + 64);
  SG_ENSURE(ctx->infl_out, total + 64);
  SG_HIP(hipMemcpyAsync(ctx->infl_src.p, members, bytes, hipMemcpyHostToDevice, s));
  int rc = inflate_launch(ctx, ctx->infl_src.as<uint8_t>(), bytes, mem, ctx->infl_meta, ctx->infl_out.as<uint8_t>(), s, s);
  if (rc != SG_OK) return rc;
  SG_HIP(hipStreamSynchronize(s));
  if ((rc = inflate_verdicts(ctx, mem, ctx->infl_meta, "sg_inflate_bgzf")) != SG_OK) return rc;
  SG_HIP(hipMemcpy(out, ctx->infl_out.p, total, hipMemcpyDeviceToHost));
  return SG_OK;
}

}  // extern "C"
