// sg_api_deflate.cpp -- the block-gzip sink of the C ABI (kernels: sg_deflate.hip, code construction: sg_deflate.cpp):
// deflate_text, which every BGZF output of the engine goes through, and the calls that hand it a pass's FASTQ text
// (sg_compress) or a caller's bytes (sg_deflate_bgzf).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sg_api.h"
#include "sg_deflate.h"
#include "sg_scan.h"

int deflate_text(sg_ctx* ctx, const uint8_t* text, uint64_t bytes, DevBuf& gz, uint64_t* gz_total, const char* who) {
  hipStream_t s = ctx->stream;
  ctx->gz_last = sg_ctx::GzLast();
  if (bytes / sg::kGzChunk >= 0xFFFFFFF0ull) return ctx->fail(SG_ERR_UNSUPPORTED, std::string(who) + ": text too large");
  const uint32_t n_chunks = (uint32_t)((bytes + sg::kGzChunk - 1) / sg::kGzChunk);
  // The head is zeroed as one: hist[320] u64, the scan's total at byte 2560, the kernels' chunk counters at byte 2576.
  // The tables are uploaded as one: code[288] | len_tok | dist_code[32] | crc_tab[1024] | crc_shift | prefix (<= 256 words).
  const size_t head_bytes = 320 * 8 + 64;
  const size_t tab_words = 288 + sg::kGzLenTokens + 32 + 1024 + sg::kGzLevels * 128 + 256;
  uint8_t* head = nullptr;
  uint32_t* dev_tab = nullptr;
  uint64_t *moff = nullptr, *bsum = nullptr;
  sg::DevDeflate D;
  memset(&D, 0, sizeof D);
  if (int rc = sg_carve(ctx, ctx->gz_work, [&](SgArena& a) {
        head = a.take<uint8_t>(head_bytes);
        dev_tab = a.take<uint32_t>(tab_words);
        D.msize = a.take<uint32_t>(n_chunks);
        moff = a.take<uint64_t>(n_chunks);
        bsum = a.take<uint64_t>((size_t)sg::scan_blocks(n_chunks) + 8);
        D.lbits = a.take<uint32_t>((size_t)n_chunks * sg::kGzThreads);
        D.rec = a.take<uint4>((size_t)n_chunks * sg::kGzThreads * 2);
      }))
    return rc;
  uint64_t* dev_total = (uint64_t*)(head + 320 * 8);
  D.text = text; D.bytes = bytes; D.n_chunks = n_chunks;
  D.min_run = sg::kGzMinRun;
  D.min_copy = sg::kGzMinGramMatch;
  if (const char* e = getenv("SG_GZ_MINCOPY")) D.min_copy = (uint32_t)std::max(8, atoi(e));   // (experiments)
  if (const char* e = getenv("SG_GZ_MINRUN")) D.min_run = (uint32_t)std::max(3, atoi(e));   // (experiments)
  D.hist = (unsigned long long*)head;
  D.next = (uint32_t*)(head + 320 * 8 + 16);
  D.moff = moff;
  // 1. token histogram of every 16th member -> the two Huffman codes, member prefix, CRC tables (host)
  SG_HIP(hipMemsetAsync(head, 0, head_bytes, s));
  sg::launch_gz_hist(D, n_chunks, s);
  uint64_t hist[320];
  if (int rc = sg_read_back(ctx, hist, head, sizeof hist)) return rc;
  sg::DeflatePlan plan;
  sg::deflate_build_plan(hist, hist + 288, &plan);
  if (plan.prefix.size() > 256) return ctx->fail(SG_ERR_UNSUPPORTED, std::string(who) + ": block header longer than expected");
  if (getenv("SG_GZ_TRACE")) {   // where the sampled members' bits go: literals by character, matches by length / distance symbol
    double lit_bits[256], tot_lit = 0, tot_len = 0, tot_dist = 0, n_match = 0, n_lit = 0, match_bytes = 0;
    static const int lbase[29] = {3,4,5,6,7,8,9,10,11,13,15,17,19,23,27,31,35,43,51,59,67,83,99,115,131,163,195,227,258};
    static const int lext[29] = {0,0,0,0,0,0,0,0,1,1,1,1,2,2,2,2,3,3,3,3,4,4,4,4,5,5,5,5,0};
    for (int c = 0; c < 256; c++) { lit_bits[c] = (double)hist[c] * plan.lit_len[c]; tot_lit += lit_bits[c]; n_lit += (double)hist[c]; }
    for (int i = 0; i < 29; i++) { tot_len += (double)hist[257 + i] * (plan.lit_len[257 + i] + lext[i]); n_match += (double)hist[257 + i];
                                   match_bytes += (double)hist[257 + i] * (lbase[i] + (i + 1 < 29 ? (lbase[i + 1] - lbase[i] - 1) / 2.0 : 0)); }
    for (int i = 0; i < 30; i++) tot_dist += (double)hist[288 + i] * (plan.dist_len[i] + (i < 4 ? 0 : (i - 2) / 2));
    const double members = (double)hist[256], all = tot_lit + tot_len + tot_dist;
    fprintf(stderr, "[gz] per member: %.0f literals %.0f bits, %.0f matches (~%.0f bytes) %.0f length bits + %.0f distance bits; total %.0f bits = %.0f bytes\n",
            n_lit / members, tot_lit / members, n_match / members, match_bytes / members, tot_len / members, tot_dist / members, all / members, all / members / 8);
    fprintf(stderr, "[gz] literal bits per member by character:");
    for (int c = 0; c < 256; c++)
      if (lit_bits[c] / members >= 20) fprintf(stderr, " '%c'x%.0f(%d b)=%.0f", c >= 32 && c < 127 ? c : '?', hist[c] / members, plan.lit_len[c], lit_bits[c] / members);
    fprintf(stderr, "\n[gz] matches per member by length symbol:");
    for (int i = 0; i < 29; i++) if (hist[257 + i] / members >= 1) fprintf(stderr, " %d+:%0.f(%d b)", lbase[i], hist[257 + i] / members, plan.lit_len[257 + i] + lext[i]);
    fprintf(stderr, "\n[gz] distance symbols:");
    for (int i = 0; i < 30; i++) if (hist[288 + i] / members >= 1) fprintf(stderr, " %d:%.0f(%d b)", i, hist[288 + i] / members, plan.dist_len[i] + (i < 4 ? 0 : (i - 2) / 2));
    fprintf(stderr, "\n");
  }
  std::vector<uint32_t> tab(tab_words, 0);
  for (int i = 0; i < sg::kGzLitSyms; i++) tab[i] = plan.lit_code[i] | ((uint32_t)plan.lit_len[i] << 16);
  memcpy(&tab[288], plan.len_token, sizeof plan.len_token);
  for (int i = 0; i < sg::kGzDistSyms; i++) tab[288 + sg::kGzLenTokens + i] = plan.dist_code[i] | ((uint32_t)plan.dist_len[i] << 16);
  const size_t t_crc = 288 + sg::kGzLenTokens + 32;
  memcpy(&tab[t_crc], plan.crc_table, sizeof plan.crc_table);
  memcpy(&tab[t_crc + 1024], plan.crc_shift, sizeof plan.crc_shift);
  memcpy(&tab[t_crc + 1024 + sg::kGzLevels * 128], plan.prefix.data(), plan.prefix.size() * 4);
  SG_HIP(hipMemcpyAsync(dev_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, s));
  D.code = dev_tab;
  D.len_tok = D.code + 288;
  D.dist_code = D.len_tok + sg::kGzLenTokens;
  D.crc_tab = D.dist_code + 32;
  D.crc_shift = D.crc_tab + 1024;
  D.prefix = D.crc_shift + sg::kGzLevels * 128;
  D.prefix_words = (uint32_t)plan.prefix.size();
  D.prefix_bits = plan.prefix_bits;
  D.crc_init_full = plan.crc_init_full;
  const uint64_t last = bytes - (uint64_t)(n_chunks - 1) * sg::kGzChunk;
  D.crc_init_last = sg::crc_advance(plan, 0xFFFFFFFFu, last);
  // 2. tokens, member sizes -> offsets
  sg::launch_gz_match(D, n_chunks, s);
  sg::launch_scan_u32(D.msize, n_chunks, bsum, moff, dev_total, s);
  uint64_t total = 0;
  if (int rc = sg_read_back(ctx, &total, dev_total, 8)) return rc;
  SG_ENSURE(gz, total + 64);
  D.out = gz.as<uint8_t>();
  // 3. encode
  sg::launch_gz_encode(D, n_chunks, plan.prefix_bits, s);
  SG_HIP(hipGetLastError());
  SG_HIP(hipStreamSynchronize(s));  // tab / plan are host-owned
  *gz_total = total;
  ctx->gz_last.text = text;
  ctx->gz_last.bytes = bytes;
  ctx->gz_last.moff = D.moff;
  return SG_OK;
}

extern "C" {

int sg_bgzf_eof(uint8_t out[28]) {
  static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (!out) return SG_ERR_INVALID;
  memcpy(out, eof, 28);
  return SG_OK;
}

uint32_t sg_deflate_plan(const uint64_t lit_counts[286], const uint64_t dist_counts[30], uint8_t lit_lens[286], uint32_t lit_codes[286],
                         uint8_t dist_lens[30], uint32_t dist_codes[30], uint32_t len_tokens[260], uint32_t* prefix_words, uint32_t cap) {
  if (!lit_counts || !dist_counts || !lit_lens || !lit_codes || !dist_lens || !dist_codes || !len_tokens || !prefix_words) return 0;
  sg::DeflatePlan plan;
  sg::deflate_build_plan(lit_counts, dist_counts, &plan);
  if (plan.prefix.size() > cap) return 0;
  memcpy(lit_lens, plan.lit_len, sizeof plan.lit_len);
  memcpy(lit_codes, plan.lit_code, sizeof plan.lit_code);
  memcpy(dist_lens, plan.dist_len, sizeof plan.dist_len);
  memcpy(dist_codes, plan.dist_code, sizeof plan.dist_code);
  memcpy(len_tokens, plan.len_token, sizeof plan.len_token);
  memcpy(prefix_words, plan.prefix.data(), plan.prefix.size() * 4);
  return plan.prefix_bits;
}

int sg_compress(sg_ctx* ctx, uint64_t* gz_bytes_r1, uint64_t* gz_bytes_r2) {
  if (int rc = sg_pass_need(ctx, "sg_compress", sg_ctx::Pass::Settled)) return rc;
  sg_ctx::Pass& Q = ctx->pass;
  const int nm = ctx->B.paired ? 2 : 1;
  Q.have_gz = false;   // (a call that fails half-way leaves no members and no sizes)
  Q.gz_bytes[0] = Q.gz_bytes[1] = 0;
  uint64_t gz[2] = {0, 0};
  for (int m = 0; m < nm; m++) {
    const uint64_t bytes = Q.host_totals[m];
    if (!bytes) continue;
    if (int rc = deflate_text(ctx, ctx->out.text[m].as<uint8_t>(), bytes, ctx->out.gz[m], &gz[m], "sg_compress")) return rc;
  }
  Q.have_gz = true;
  Q.gz_bytes[0] = gz[0];
  Q.gz_bytes[1] = gz[1];
  if (gz_bytes_r1) *gz_bytes_r1 = Q.gz_bytes[0];
  if (gz_bytes_r2) *gz_bytes_r2 = Q.gz_bytes[1];
  return SG_OK;
}

int sg_deflate_bgzf(sg_ctx* ctx, const void* text, uint64_t bytes, void* out, uint64_t out_cap, uint64_t* out_bytes) {
  if (!ctx || (bytes && !text) || !out_bytes) return SG_ERR_INVALID;
  *out_bytes = 0;
  if (!bytes) return SG_OK;
  SG_HIP(hipSetDevice(ctx->device));
  SG_ENSURE(ctx->defl_src, bytes + 64);
  SG_HIP(hipMemcpyAsync(ctx->defl_src.p, text, bytes, hipMemcpyHostToDevice, ctx->stream));
  uint64_t total = 0;
  const int rc = deflate_text(ctx, ctx->defl_src.as<uint8_t>(), bytes, ctx->defl_out, &total, "sg_deflate_bgzf");
  if (rc != SG_OK) return rc;
  *out_bytes = total;
  if (total > out_cap) return ctx->fail(SG_ERR_OVERFLOW, "sg_deflate_bgzf: the members do not fit out_cap");
  if (!out) return SG_ERR_INVALID;
  SG_HIP(hipMemcpy(out, ctx->defl_out.p, total, hipMemcpyDeviceToHost));
  return SG_OK;
}

int sg_fetch_compressed(sg_ctx* ctx, int mate, uint64_t offset, uint64_t bytes, void* host_dst) {
  if (!ctx || mate < 0 || mate > 1 || (bytes && !host_dst)) return SG_ERR_INVALID;
  if (!ctx->pass.have_gz) return ctx->fail(SG_ERR_INVALID, "sg_fetch_compressed: call sg_compress first");
  if (!sg_range_within(offset, bytes, ctx->pass.gz_bytes[mate])) return ctx->fail(SG_ERR_INVALID, "sg_fetch_compressed: range past the end of the compressed text");
  SG_HIP(sg_fetch_bytes(ctx->device, ctx->stream, host_dst, ctx->out.gz[mate].as<uint8_t>() + offset, bytes));
  return SG_OK;
}

}  // extern "C"
