// sg_truth.hip -- truth alignments of a sampled pass as BAM records (simuReads --truth-bam), gfx950.
//
// After a pass the device still holds where every read came from: the fragment's chain offset and strand and the read's
// sequencing indels (the reads' meta rows, DevBatch::events).  With the chains' piece map (the copy list of
// sg_build_haplotypes) that is the read's true alignment (truth_walk, sg_truth.h).  Two kernels turn it into the record
// stream of a BAM file, in FASTQ order (slot by slot, mate 1 then mate 2):
//   truth_size_kernel   lane = read: the walk, counting operations -> a row {contig, pos, end, n_ops} and the record's
//                       length per read (launch_scan_u32 turns the lengths into offsets);
//   truth_pack_kernel   wave = 64 consecutive records.  Phase A, lane = read: the walk again, the operations into the
//                       wave's LDS, the nine fixed words of the record (the mate's row gives RNEXT / PNEXT / TLEN and
//                       the 0x8 / 0x20 flag bits).  Phase B, record by record, the whole wave: the record's FASTQ text
//                       comes in as 16-byte pieces, its image is put together byte by byte in LDS (name, operations,
//                       4-bit bases, qualities; turned round for a reverse read), and leaves as 16-byte pieces --
//                       records are ~300 unaligned bytes, stored by their own lanes every store instruction would
//                       touch 64 cache lines (the reason fragment_kernel's rows leave through LDS); only the bytes an
//                       image shares a 16-byte piece with its neighbours' go out singly.  truth_pack_kernel<true>
//                       (simuReads --truth-tags) appends the NM, XE and MD tags that truth_tag_size_kernel
//                       (sg_truth_tags.hip) has sized; truth_pack_kernel<false> is the kernel without them.
#include <type_traits>

#include "sg_truth_tags.h"

namespace sg {
namespace {

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t qname_len(const DevBatch& B, uint32_t hdr) { return hdr - 2u - (B.paired ? 2u : 0u); }

__global__ __launch_bounds__(256) void truth_size_kernel(DevProfile P, DevBatch B, TruthJob J) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  const PassRead R = pass_read(B, idx, J.map.n_reads);
  ReadGeom g = {};
  if (R.in_range) g = read_geom(P, B, R.t, R.m);
  TruthRow row = {-1, -1, -1, 0u};
  uint32_t len = 0, flags = 0;
  if (g.live) {
    if (g.inside && g.chain < J.map.n_chains) {
      const uint64_t pi = truth_find_piece(J.map.pieces, J.map.chain_first[g.chain], J.map.chain_first[g.chain + 1], g.tmpl_off);
      const TruthAln A = truth_walk(J.map.pieces, J.map.chain_first[g.chain + 1], pi, g.tmpl_off, (uint32_t)P.L, g.reverse != 0u, g.events, g.nev,
                                    [](uint32_t, uint32_t) {});
      if (A.n_ops > kTruthMaxOps) flags |= 1u;
      else if (A.n_ops) row = TruthRow{A.contig, (int32_t)A.pos0, (int32_t)A.end, A.n_ops};
    }
    len = 36u + qname_len(B, g.hdr) + 1u + 4u * row.n_ops + (g.np + 1u) / 2u + g.np;
  }
  if (R.in_range) {
    J.rows[idx] = row;
    J.rec_len[idx] = len;
  }
  uint32_t ops = row.n_ops;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) ops += __shfl_xor(ops, d, 64);
  if (ops > kTruthWaveOps) flags |= 2u;
  const unsigned long long lm = __ballot(g.live), um = __ballot(g.live && row.n_ops == 0u), fm = __ballot(flags != 0u);
  if ((threadIdx.x & 63u) == 0u) {
    if (lm) atomicAdd(&J.counters[0], (unsigned long long)__popcll(lm));
    if (um) atomicAdd(&J.counters[1], (unsigned long long)__popcll(um));
  }
  if (fm && flags) atomicOr(&J.counters[2], (unsigned long long)flags);
}

// 4-bit base code of SAMv1 section 4.2 ("=ACMGRSVTWYHKDBN"); the complement for a read that is turned round
__device__ __forceinline__ uint32_t nt16(uint32_t ch, bool comp) {
  const uint32_t c = ch == 'A' ? 1u : ch == 'C' ? 2u : ch == 'G' ? 4u : ch == 'T' ? 8u : 15u;
  if (!comp || c == 15u) return c;
  return c == 1u ? 8u : c == 8u ? 1u : c == 2u ? 4u : 2u;
}

// The record kernel.  kTags = false is the kernel as it has always been, its own instantiation with nothing of the tags
// in it (a body shared through a wrapper comes out with other register counts); kTags = true appends the record's tags
// behind the qualities (T: the job of truth_tag_size_kernel, whose rows say what each record gets).
struct NoTagJob {};
template <bool kTags>
__global__ __launch_bounds__(64) void truth_pack_kernel(DevProfile P, DevBatch B, TruthJob J, std::conditional_t<kTags, TagJob, NoTagJob> T) {
  extern __shared__ uint4 lds16[];
  uint32_t* const cig = (uint32_t*)lds16;                       // [kTruthWaveOps]
  uint32_t* const fix = cig + kTruthWaveOps;                    // [64][9] the records' fixed words
  uint8_t* const text = (uint8_t*)(fix + 64 * 9 + 0);           // [text_lds]   (64 * 9 * 4 = 2304: a multiple of 16)
  uint8_t* const image = text + J.text_lds;                     // [image_lds]
  const uint32_t lane = threadIdx.x;
  const uint32_t idx = blockIdx.x * 64u + lane;
  const uint32_t nm = B.paired ? 2u : 1u;
  // ---- phase A: lane = read ----
  const PassRead R = pass_read(B, idx, J.map.n_reads);
  const uint32_t t = R.t, m = R.m;
  ReadGeom g = {};
  TruthRow row = {-1, -1, -1, 0u};
  uint32_t rec_len = 0;
  uint64_t rec_off = 0, toff = 0;
  if (R.in_range) {
    rec_len = J.rec_len[idx];
    if (rec_len) {
      g = read_geom(P, B, t, m);
      row = J.rows[idx];
      rec_off = J.rec_off[idx];
      toff = text_offset(B, m, t);
    }
  }
  const bool live = rec_len != 0u && g.live;
  TagRow tag = {0u, 0u, 0u};
  if constexpr (kTags) {
    if (live) tag = T.rows[idx];
  }
  uint32_t cig_base = row.n_ops;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(cig_base, d, 64);
    if ((int)lane >= d) cig_base += up;
  }
  cig_base -= row.n_ops;
  const bool mapped = row.n_ops != 0u;
  if (live && mapped && cig_base + row.n_ops <= kTruthWaveOps) {
    const uint64_t pi = truth_find_piece(J.map.pieces, J.map.chain_first[g.chain], J.map.chain_first[g.chain + 1], g.tmpl_off);
    const uint32_t n_ops = row.n_ops;
    uint32_t* const mine = cig + cig_base;
    truth_walk(J.map.pieces, J.map.chain_first[g.chain + 1], pi, g.tmpl_off, (uint32_t)P.L, g.reverse != 0u, g.events, g.nev,
               [=](uint32_t i, uint32_t v) { if (i < n_ops) mine[i] = v; });
  }
  if (live) {
    TruthRow mate = {-1, -1, -1, 0u};
    const bool has_mate = nm == 2u && J.rec_len[idx ^ 1u] != 0u;
    if (has_mate) mate = J.rows[idx ^ 1u];
    const bool mate_mapped = mate.n_ops != 0u;
    // the mate's strand: PE mate 1 is forward, mate 2 reverse
    uint32_t flag = 0;
    if (nm == 2u) {
      flag = 1u | (m == 0u ? 0x40u : 0x80u);
      if (mapped && mate_mapped) flag |= 2u;
      if (!mate_mapped) flag |= 8u;
      else if (m == 0u) flag |= 0x20u;   // mate 2 is the reverse read
    }
    if (mapped) { if (g.reverse) flag |= 0x10u; } else flag |= 4u;
    int32_t ref = row.contig, pos = row.pos, end = row.end;
    if (!mapped) { ref = mate_mapped ? mate.contig : -1; pos = mate_mapped ? mate.pos : -1; end = pos + 1; }
    int32_t nref = -1, npos = -1, tlen = 0;
    if (nm == 2u) {
      if (mate_mapped) { nref = mate.contig; npos = mate.pos; }
      else { nref = ref; npos = pos; }
      if (mapped && mate_mapped && mate.contig == row.contig) {
        const int32_t left = min(row.pos, mate.pos), right = max(row.end, mate.end);
        const bool leftmost = row.pos < mate.pos || (row.pos == mate.pos && m == 0u);
        tlen = leftmost ? right - left : left - right;
      }
    }
    const uint32_t bin = pos >= 0 ? truth_reg2bin(pos, mapped ? end : pos + 1) : 4680u;
    uint32_t* w = fix + lane * 9u;
    w[0] = rec_len - 4u;
    w[1] = (uint32_t)ref;
    w[2] = (uint32_t)pos;
    w[3] = (qname_len(B, g.hdr) + 1u) | ((mapped ? 60u : 0u) << 8) | (bin << 16);
    w[4] = row.n_ops | (flag << 16);
    w[5] = g.np;
    w[6] = (uint32_t)nref;
    w[7] = (uint32_t)npos;
    w[8] = (uint32_t)tlen;
  }
  wave_lds_sync();
  // ---- phase B: record by record, lane = byte ----
  const unsigned long long todo = __ballot(live && cig_base + row.n_ops <= kTruthWaveOps);
  for (uint32_t r = 0; r < 64u; r++) {
    if (!((todo >> r) & 1ull)) continue;
    const uint32_t r_len = __shfl(rec_len, r, 64), r_np = __shfl(g.np, r, 64), r_hdr = __shfl(g.hdr, r, 64);
    const uint32_t r_ops = __shfl(row.n_ops, r, 64), r_cig = __shfl(cig_base, r, 64), r_m = __shfl(m, r, 64);
    const bool flip = __shfl((uint32_t)(mapped && g.reverse), r, 64) != 0u;
    const uint64_t r_off = ((uint64_t)__shfl((uint32_t)(rec_off >> 32), r, 64) << 32) | __shfl((uint32_t)rec_off, r, 64);
    const uint64_t r_toff = ((uint64_t)__shfl((uint32_t)(toff >> 32), r, 64) << 32) | __shfl((uint32_t)toff, r, 64);
    const uint32_t tlen = r_hdr + 2u * r_np + 4u;
    const uint32_t dt = (uint32_t)(r_toff & 15u), h = (uint32_t)(r_off & 15u);
    const uint64_t ta = r_toff - dt;
    const uint32_t n16 = (dt + tlen + 15u) >> 4;
    if (n16 * 16u > J.text_lds || h + r_len > J.image_lds || ta + (uint64_t)n16 * 16u > B.out_cap[r_m] || r_off + r_len > J.out_bytes) {
      if (lane == 0u) atomicOr(&J.counters[2], 4ull);   // (the host sizes both stages; reported, nothing is written)
      continue;
    }
    const uint4* src = (const uint4*)(B.out[r_m] + ta);
    for (uint32_t q = lane; q < n16; q += 64u) ((uint4*)text)[q] = src[q];
    wave_lds_sync();
    const uint32_t lq = qname_len(B, r_hdr), seq_b = (r_np + 1u) / 2u;
    const uint32_t o_cig = 36u + lq + 1u, o_seq = o_cig + 4u * r_ops, o_qual = o_seq + seq_b;
    const uint8_t* tx = text + dt;
    const uint32_t img_len = kTags ? o_qual + r_np : r_len;   // the record without its tags
    uint32_t present = 0u, r_md = 0u;
    if constexpr (kTags) {
      r_md = __shfl(tag.md_len, r, 64);
      present = tags_present(T.tags, r_ops != 0u, __shfl((uint32_t)g.inside, r, 64) != 0u, r_md);
      if (img_len + truth_tag_bytes(present, r_md) != r_len) {   // (the sizing kernel's row and this record disagree: nothing is written)
        if (lane == 0u) atomicOr(&J.counters[2], 4ull);
        continue;
      }
    }
    for (uint32_t k = lane; k < img_len; k += 64u) {
      uint32_t b;
      if (k < 36u) {
        b = fix[r * 9u + (k >> 2)] >> (8u * (k & 3u));
      } else if (k < o_cig) {
        b = k - 36u < lq ? tx[1u + (k - 36u)] : 0u;
      } else if (k < o_seq) {
        b = cig[r_cig + ((k - o_cig) >> 2)] >> (8u * ((k - o_cig) & 3u));
      } else if (k < o_qual) {
        const uint32_t i0 = 2u * (k - o_seq), i1 = i0 + 1u;
        const uint32_t c0 = nt16(tx[r_hdr + (flip ? r_np - 1u - i0 : i0)], flip);
        const uint32_t c1 = i1 < r_np ? nt16(tx[r_hdr + (flip ? r_np - 1u - i1 : i1)], flip) : 0u;
        b = (c0 << 4) | c1;
      } else {
        const uint32_t i = k - o_qual;
        b = tx[r_hdr + r_np + 3u + (flip ? r_np - 1u - i : i)] - 33u;
      }
      image[h + k] = (uint8_t)b;
    }
    if constexpr (kTags) {   // NM:I, XE:I, MD:Z behind the qualities
      const uint32_t r_nm = __shfl(tag.nm, r, 64), r_xe = __shfl(tag.xe, r, 64);
      uint8_t* tp = image + h + img_len;
      if (present & kTagNM) {
        if (lane < 7u) tp[lane] = (uint8_t)(lane == 0u ? 'N' : lane == 1u ? 'M' : lane == 2u ? 'I' : r_nm >> (8u * (lane - 3u)));
        tp += 7;
      }
      if (present & kTagXE) {
        if (lane < 7u) tp[lane] = (uint8_t)(lane == 0u ? 'X' : lane == 1u ? 'E' : lane == 2u ? 'I' : r_xe >> (8u * (lane - 3u)));
        tp += 7;
      }
      if (present & kTagMD) {
        if (lane < 3u) tp[lane] = (uint8_t)(lane == 0u ? 'M' : lane == 1u ? 'D' : 'Z');
        if (lane == 3u) tp[3u + r_md] = 0u;
        const uint32_t ref = fix[r * 9u + 1u], pos = fix[r * 9u + 2u];
        const uint64_t len = ref < T.n_refs ? T.refs[ref].length : 0ull;
        if (pos <= len) {   // (the sizing kernel has checked the span; a record it refused fails the call)
          const WaveSeq S = {tx + r_hdr, r_np, flip};
          wave_tags_walk<true>(cig + r_cig, r_ops, S, T.ref_codes + T.refs[ref].code_off + pos, len - pos, lane, tp + 3, r_md);
        }
      }
    }
    wave_lds_sync();
    uint8_t* const dst = J.out + (r_off - h);   // 16-byte aligned: the stream's buffer is, and r_off - h is a multiple of 16
    const uint32_t e = h + r_len, p16 = (e + 15u) >> 4;
    for (uint32_t p = lane; p < p16; p += 64u) {
      const uint32_t lo = p * 16u, hi = lo + 16u;
      if (lo >= h && hi <= e) {
        ((uint4*)dst)[p] = ((const uint4*)image)[p];
      } else {   // a piece shared with the neighbouring record
        for (uint32_t i = max(lo, h); i < min(hi, e); i++) dst[i] = image[i];
      }
    }
    wave_lds_sync();
  }
}

// sg_truth_reads: one row per read of mate `mate`, slots [first, first + n)
__global__ __launch_bounds__(256) void truth_reads_kernel(DevProfile P, DevBatch B, uint32_t mate, uint32_t first, uint32_t n, TruthReadRow* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ReadGeom g = read_geom(P, B, first + i, mate);
  TruthReadRow& r = out[i];   // (written in place: a row in registers would be indexed by the event loop)
  r.live = g.live ? 1u : 0u;
  r.chain = g.chain;
  r.reverse = g.reverse;
  r.read_len = g.np;
  r.tmpl_off = g.tmpl_off;
  r.n_events = g.nev;
  r.inside = g.inside ? 1u : 0u;
  for (uint32_t e = 0; e < SG_MAX_EVENTS; e++) r.events[e] = e < g.nev ? g.events[e] : 0u;
}

}  // namespace

void launch_truth_size(const DevProfile& P, const DevBatch& B, const TruthJob& J, hipStream_t s) {
  if (!J.map.n_reads) return;
  hipLaunchKernelGGL(truth_size_kernel, dim3((J.map.n_reads + 255u) / 256u), dim3(256), 0, s, P, B, J);
}
void launch_truth_pack(const DevProfile& P, const DevBatch& B, const TruthJob& J, hipStream_t s) {
  if (!J.map.n_reads) return;
  const size_t lds = (size_t)kTruthWaveOps * 4 + 64 * 9 * 4 + J.text_lds + J.image_lds;
  (void)hipFuncSetAttribute((const void*)truth_pack_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(truth_pack_kernel<false>, dim3((J.map.n_reads + 63u) / 64u), dim3(64), lds, s, P, B, J, NoTagJob{});
}
void launch_truth_pack_tags(const DevProfile& P, const DevBatch& B, const TruthJob& J, const TagJob& T, hipStream_t s) {
  if (!J.map.n_reads) return;
  const size_t lds = (size_t)kTruthWaveOps * 4 + 64 * 9 * 4 + J.text_lds + J.image_lds;
  (void)hipFuncSetAttribute((const void*)truth_pack_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(truth_pack_kernel<true>, dim3((J.map.n_reads + 63u) / 64u), dim3(64), lds, s, P, B, J, T);
}
void launch_truth_reads(const DevProfile& P, const DevBatch& B, uint32_t mate, uint32_t first_slot, uint32_t n, TruthReadRow* out, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(truth_reads_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, P, B, mate, first_slot, n, out);
}

}  // namespace sg
