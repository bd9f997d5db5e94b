// sg_api_haplotypes.cpp -- reference ingest and haplotype assembly on the device (kernels: sg_haplotypes.hip): the FASTA
// image and its contigs' codes (sg_reference_*), the chains from a copy list (sg_build_haplotypes) or from strings
// (sg_upload_haplotypes), their padded layout and 2-bit copies.
#include <algorithm>

#include "sg_api.h"
#include "sg_hap_check.h"

namespace chk = sg::hapcheck;

// 2-bit copies of the chains buffer (`total` bytes, a multiple of 1024) for the straight-line emit kernel
static int pack_chains(sg_ctx* ctx, size_t total) {
  const size_t q = total / 4, badb = total / 64 / 8;
  SG_ENSURE(ctx->chains2, 2 * q + badb + 64);
  uint8_t* p = ctx->chains2.as<uint8_t>();
  sg::launch_pack2(ctx->chains.as<uint8_t>(), total, (uint32_t*)p, (uint32_t*)(p + q), (uint16_t*)(p + 2 * q), ctx->stream);
  ctx->B.chains2_fwd = p;
  ctx->B.chains2_rc = p + q;
  ctx->B.chains_bad = (const uint16_t*)(p + 2 * q);
  ctx->B.chains_total = total;
  return SG_OK;
}

// The padded layout of the chains buffer (sg_upload_haplotypes, sg_build_haplotypes): a guard of 256 bytes in front of
// every chain and behind the last one (kernels read up to 16 bytes around a fragment, the emit kernel up to 11 before its
// start), every chain rounded up to 64 bytes, the whole to 1024 (pack_chains).
static sg_ctx::ChainLayout chain_layout(int32_t n_chains, const uint64_t* lens) {
  const size_t PAD = 256;
  sg_ctx::ChainLayout L;
  L.len.assign(lens, lens + n_chains);
  L.total = PAD;
  for (int c = 0; c < n_chains; c++) {
    L.off.push_back(L.total);
    L.total += (lens[c] + PAD + 63) & ~(size_t)63;
  }
  L.total = (L.total + PAD + 1023) & ~(size_t)1023;
  return L;
}

// The chains of layout L are in place in ctx->chains: the layout goes to chain_meta (offsets, then lengths) and to
// ctx->hap, the 2-bit copies are made, and the batch reads the new chains from now on.
static int commit_chains(sg_ctx* ctx, sg_ctx::ChainLayout&& L) {
  std::vector<uint64_t> meta(L.off);
  meta.insert(meta.end(), L.len.begin(), L.len.end());
  meta.resize(meta.size() + 2, 0);
  SG_ENSURE(ctx->chain_meta, meta.size() * 8);
  SG_HIP(hipMemcpyAsync(ctx->chain_meta.p, meta.data(), meta.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  if (int rc = pack_chains(ctx, L.total)) return rc;
  SG_HIP(hipGetLastError());
  SG_HIP(hipStreamSynchronize(ctx->stream));  // (meta is host memory of this frame, the callers' staging likewise)
  ctx->B.chains = ctx->chains.as<uint8_t>();
  ctx->B.chain_off = ctx->chain_meta.as<uint64_t>();
  ctx->B.chain_len = ctx->chain_meta.as<uint64_t>() + L.len.size();
  ctx->hap = std::move(L);
  ctx->have_haps = true;
  retire_plan(ctx);
  return SG_OK;
}

extern "C" {

int sg_reference_begin(sg_ctx* ctx, uint64_t raw_bytes) {
  if (!ctx) return SG_ERR_INVALID;
  SG_HIP(hipSetDevice(ctx->device));
  SG_ENSURE(ctx->ref_raw, raw_bytes + 64);
  SG_HIP(hipMemsetAsync((uint8_t*)ctx->ref_raw.p + raw_bytes, '\n', 64, ctx->stream));  // the scan reads whole 16-byte words
  ctx->ref_raw_bytes = raw_bytes;
  ctx->ref_contigs.clear();
  return SG_OK;
}

int sg_reference_chunk(sg_ctx* ctx, uint64_t offset, const void* host, uint64_t bytes) {
  if (!ctx || (!host && bytes)) return SG_ERR_INVALID;
  if (auto v = chk::chunk(ctx->ref_raw.p != nullptr, ctx->ref_raw_bytes, offset, bytes)) return ctx->fail(v.code, v.msg);
  SG_HIP(hipSetDevice(ctx->device));
  if (bytes) SG_HIP(hipMemcpyAsync((uint8_t*)ctx->ref_raw.p + offset, host, bytes, hipMemcpyHostToDevice, ctx->stream));
  return SG_OK;
}

int sg_reference_scan(sg_ctx* ctx, uint64_t* header_offsets, uint32_t cap, uint32_t* n_found, uint32_t* flags) {
  if (!ctx || !n_found || (cap && !header_offsets)) return SG_ERR_INVALID;
  if (auto v = chk::need_image(ctx->ref_raw.p != nullptr, "sg_reference_scan")) return ctx->fail(v.code, v.msg);
  SG_HIP(hipSetDevice(ctx->device));
  SG_ENSURE(ctx->hap_work, (size_t)cap * 8 + 64);
  uint32_t* counters = (uint32_t*)((uint8_t*)ctx->hap_work.p + (size_t)cap * 8);
  SG_HIP(hipMemsetAsync(counters, 0, 8, ctx->stream));
  sg::launch_ref_scan(ctx->ref_raw.as<uint8_t>(), ctx->ref_raw_bytes, ctx->hap_work.as<uint64_t>(), cap, counters, counters + 1, ctx->stream);
  uint32_t host_c[2] = {0, 0};
  if (int rc = sg_read_back(ctx, host_c, counters, 8)) return rc;
  *n_found = host_c[0];
  if (flags) *flags = host_c[1];
  const uint32_t n = host_c[0] < cap ? host_c[0] : cap;
  if (n) SG_HIP(hipMemcpy(header_offsets, ctx->hap_work.p, (size_t)n * 8, hipMemcpyDeviceToHost));
  return SG_OK;
}

int sg_reference_commit(sg_ctx* ctx, const sg_contig* contigs, uint32_t n_contigs) {
  if (!ctx || (n_contigs && !contigs)) return SG_ERR_INVALID;
  if (auto v = chk::need_image(ctx->ref_raw.p != nullptr, "sg_reference_commit")) return ctx->fail(v.code, v.msg);
  SG_HIP(hipSetDevice(ctx->device));
  std::vector<sg::DevContig> tab(n_contigs);
  uint64_t code_off = 0, blocks = 0;
  for (uint32_t c = 0; c < n_contigs; c++) {
    const sg_contig& k = contigs[c];
    if (auto v = chk::contig(k, c, ctx->ref_raw_bytes)) return ctx->fail(v.code, v.msg);   // line shape, 32-bit length, extent
    tab[c] = sg::DevContig{k.raw_offset, code_off, k.length, k.line_bases, k.line_width, blocks};
    blocks += (k.length + 15) / 16;
    code_off += ((k.length + 15) / 16) * 16 + 64;
  }
  SG_ENSURE(ctx->ref_codes, code_off + 64);
  SG_ENSURE(ctx->ref_meta, (size_t)n_contigs * sizeof(sg::DevContig) + 64);
  uint32_t* flags = (uint32_t*)((uint8_t*)ctx->ref_meta.p + (size_t)n_contigs * sizeof(sg::DevContig));
  SG_HIP(hipMemsetAsync(flags, 0, 4, ctx->stream));
  if (n_contigs) SG_HIP(hipMemcpyAsync(ctx->ref_meta.p, tab.data(), (size_t)n_contigs * sizeof(sg::DevContig), hipMemcpyHostToDevice, ctx->stream));
  sg::launch_ref_ingest(ctx->ref_raw.as<uint8_t>(), ctx->ref_codes.as<uint8_t>(), ctx->ref_meta.as<sg::DevContig>(), n_contigs, blocks, flags, ctx->stream);
  uint32_t host_flags = 0;
  if (int rc = sg_read_back(ctx, &host_flags, flags, 4)) return rc;
  if (host_flags & 2u) return ctx->fail(SG_ERR_FORMAT, "sg_reference_commit: a contig's lines are not of one width");
  ctx->ref_contigs = tab;
  ctx->ref_raw.release();  // the file image is not needed again
  ctx->ref_raw_bytes = 0;
  return SG_OK;
}

int sg_build_haplotypes(sg_ctx* ctx, int32_t n_chains, const uint64_t* lens, const sg_hap_piece* pieces, uint64_t n_pieces,
                        const char* literals, uint64_t n_literal_bytes, const sg_hap_patch* patches, uint64_t n_patches) {
  if (!ctx || n_chains < 0 || (n_chains && !lens) || (n_pieces && !pieces) || (n_patches && !patches) ||
      (n_literal_bytes && !literals))
    return SG_ERR_INVALID;
  if (auto v = chk::need_contigs(!ctx->ref_contigs.empty(), n_pieces)) return ctx->fail(v.code, v.msg);
  SG_HIP(hipSetDevice(ctx->device));
  sg_ctx::ChainLayout L = chain_layout(n_chains, lens);
  // absolute offsets, long pieces split so that every workgroup moves <= 64 KB; each piece is checked against its chain
  // and its source, then the list as a tiling of every chain (sg_hap_check.h)
  const uint32_t kSplit = 1u << 16;
  std::vector<sg::DevPiece> dp;
  dp.reserve((size_t)n_pieces + L.total / kSplit + 16);
  auto contig_length = [&](uint32_t k) { return ctx->ref_contigs[k].length; };
  for (uint64_t i = 0; i < n_pieces; i++) {
    const sg_hap_piece& p = pieces[i];
    if (auto v = chk::piece(p, i, n_chains, lens, contig_length, ctx->ref_contigs.size(), n_literal_bytes)) return ctx->fail(v.code, v.msg);
    const uint64_t src = p.kind == 0 ? ctx->ref_contigs[p.contig].code_off + p.src : p.src;
    for (uint32_t o = 0; o < p.len; o += kSplit)
      dp.push_back(sg::DevPiece{L.off[p.chain] + p.dst + o, src + o, std::min<uint32_t>(kSplit, p.len - o), p.kind ? 1u : 0u});
  }
  if (auto v = chk::tiling(n_chains, lens, pieces, n_pieces)) return ctx->fail(v.code, v.msg);
  std::vector<sg::DevPatch> pt((size_t)n_patches);
  for (uint64_t i = 0; i < n_patches; i++) {
    const sg_hap_patch& q = patches[i];
    if (auto v = chk::patch(q, i, n_chains, lens)) return ctx->fail(v.code, v.msg);
    pt[i] = sg::DevPatch{L.off[q.chain] + q.dst, q.base, 0};
  }
  SG_ENSURE(ctx->chains, L.total);
  const size_t pieces_b = (dp.size() * sizeof(sg::DevPiece) + 63) & ~(size_t)63, patches_b = (pt.size() * sizeof(sg::DevPatch) + 63) & ~(size_t)63;
  SG_ENSURE(ctx->hap_work, pieces_b + patches_b + n_literal_bytes + 64);
  uint8_t* wk = ctx->hap_work.as<uint8_t>();
  SG_HIP(hipMemsetAsync(ctx->chains.p, 4, L.total, ctx->stream));  // guard bytes read as 'N'
  if (!dp.empty()) SG_HIP(hipMemcpyAsync(wk, dp.data(), dp.size() * sizeof(sg::DevPiece), hipMemcpyHostToDevice, ctx->stream));
  if (!pt.empty()) SG_HIP(hipMemcpyAsync(wk + pieces_b, pt.data(), pt.size() * sizeof(sg::DevPatch), hipMemcpyHostToDevice, ctx->stream));
  if (n_literal_bytes) {
    SG_HIP(hipMemcpyAsync(wk + pieces_b + patches_b, literals, n_literal_bytes, hipMemcpyHostToDevice, ctx->stream));
    sg::launch_encode_bytes(wk + pieces_b + patches_b, n_literal_bytes, ctx->stream);
  }
  sg::launch_hap_copy(ctx->chains.as<uint8_t>(), ctx->ref_codes.as<uint8_t>(), wk + pieces_b + patches_b, (const sg::DevPiece*)wk, dp.size(), ctx->stream);
  sg::launch_hap_patch(ctx->chains.as<uint8_t>(), (const sg::DevPatch*)(wk + pieces_b), pt.size(), ctx->stream);
  const int rc = commit_chains(ctx, std::move(L));   // (synchronises: dp / pt are stack-owned host memory)
  ctx->truth.forget();
  if (rc == SG_OK) {   // chains with a copy list: sg_truth_map may be given it (nothing of it is kept here)
    ctx->truth.n_given = n_pieces;
    ctx->truth.from_build = true;
  }
  return rc;
}

int sg_haplotype_codes(sg_ctx* ctx, uint32_t chain, uint64_t offset, uint64_t n, uint8_t* codes_out) {
  if (!ctx || (n && !codes_out)) return SG_ERR_INVALID;
  if (auto v = chk::codes(ctx->have_haps, ctx->hap.len.data(), ctx->hap.len.size(), chain, offset, n)) return ctx->fail(v.code, v.msg);
  SG_HIP(hipSetDevice(ctx->device));
  if (n) SG_HIP(hipMemcpy(codes_out, ctx->B.chains + ctx->hap.off[chain] + offset, n, hipMemcpyDeviceToHost));
  return SG_OK;
}

int sg_upload_haplotypes(sg_ctx* ctx, int32_t n_chains, const char* const* chains, const uint64_t* lens) {
  if (!ctx || n_chains < 0 || (n_chains && (!chains || !lens))) return SG_ERR_INVALID;
  SG_HIP(hipSetDevice(ctx->device));
  sg_ctx::ChainLayout L = chain_layout(n_chains, lens);
  SG_ENSURE(ctx->chains, L.total);
  SG_HIP(hipMemsetAsync(ctx->chains.p, 'N', L.total, ctx->stream));
  for (int c = 0; c < n_chains; c++)
    if (lens[c]) SG_HIP(hipMemcpyAsync((uint8_t*)ctx->chains.p + L.off[c], chains[c], lens[c], hipMemcpyHostToDevice, ctx->stream));
  // ASCII -> base codes, in place (A0 C1 T2 G3, N=4, other=5): the kernels never see ASCII
  sg::launch_encode((uint8_t*)ctx->chains.p, L.total, ctx->stream);
  ctx->truth.forget();   // strings have no copy list
  return commit_chains(ctx, std::move(L));
}

}  // extern "C"
