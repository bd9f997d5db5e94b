// sg_truth_tags.hip -- what the NM, MD and XE tags of a pass's truth BAM records come to (simuReads --truth-tags), gfx950.
//
// The rule is truth_tags_walk / truth_xe (sg_truth.h, DESIGN.md "Truth tags"); sg_truth_tags.h holds the wave's form of
// it.  The tags make a record longer, so they are sized between truth_size_kernel and the scan of the records' lengths:
//   truth_tag_size_kernel   wave = 64 consecutive records, as the record kernel takes them.  Phase A, lane = read: the
//                           geometry, where the read's text and its template start, its row of truth_size_kernel, the
//                           walk's operations into the wave's LDS.  Phase B, record by record, lane = base: 64
//                           consecutive text bytes with their reference codes (NM, the MD text's length: the mismatches
//                           of a chunk come from one ballot, and only they are walked one by one) and with their chain
//                           codes (XE).  Per read a row {NM, XE, MD length or dropped} stays for the record kernel, and
//                           the tag bytes are added to the record's length.  No MD text is kept: the record kernel
//                           makes it again from the text stage it holds anyway.
#include "sg_truth_tags.h"

namespace sg {
namespace {

__global__ __launch_bounds__(64) void truth_tag_size_kernel(DevProfile P, DevBatch B, TruthJob J, TagJob T) {
  __shared__ uint32_t cig[kTruthWaveOps];
  const uint32_t lane = threadIdx.x;
  const uint32_t idx = blockIdx.x * 64u + lane;
  const uint32_t L = (uint32_t)P.L;
  // ---- phase A: lane = read ----
  const PassRead R = pass_read(B, idx, J.map.n_reads);
  ReadGeom g = {};
  TruthRow row = {-1, -1, -1, 0u};
  uint32_t rec_len = 0;
  uint64_t toff = 0, coff = 0;
  if (R.in_range) {
    rec_len = J.rec_len[idx];
    if (rec_len) {
      g = read_geom(P, B, R.t, R.m);
      row = J.rows[idx];
      toff = text_offset(B, R.m, R.t);
      if (g.inside) coff = B.chain_off[g.chain] + g.tmpl_off;
    }
  }
  const bool live = rec_len != 0u && g.live;
  uint32_t cig_base = row.n_ops;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(cig_base, d, 64);
    if ((int)lane >= d) cig_base += up;
  }
  cig_base -= row.n_ops;
  const bool mapped = row.n_ops != 0u;
  const bool fits = cig_base + row.n_ops <= kTruthWaveOps;   // (truth_size_kernel has flagged the wave otherwise: the call fails)
  if (live && mapped && fits && (T.tags & (kTagNM | kTagMD))) {
    const uint64_t pi = truth_find_piece(J.map.pieces, J.map.chain_first[g.chain], J.map.chain_first[g.chain + 1], g.tmpl_off);
    const uint32_t n_ops = row.n_ops;
    uint32_t* const mine = cig + cig_base;
    truth_walk(J.map.pieces, J.map.chain_first[g.chain + 1], pi, g.tmpl_off, L, g.reverse != 0u, g.events, g.nev,
               [=](uint32_t i, uint32_t v) { if (i < n_ops) mine[i] = v; });
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  // ---- phase B: record by record, lane = base ----
  TagRow mine = {0u, 0u, 0u};
  uint32_t flags = 0;
  unsigned long long todo = __ballot(live && fits);
  while (todo) {
    const uint32_t r = (uint32_t)__ffsll((long long)todo) - 1u;
    todo &= todo - 1ull;
    const uint32_t r_np = __shfl(g.np, r, 64), r_hdr = __shfl(g.hdr, r, 64), r_nev = __shfl(g.nev, r, 64), r_m = __shfl(R.m, r, 64);
    const uint32_t r_ops = __shfl(row.n_ops, r, 64), r_cig = __shfl(cig_base, r, 64);
    const bool r_rev = __shfl(g.reverse, r, 64) != 0u, r_inside = __shfl((uint32_t)g.inside, r, 64) != 0u;
    const int32_t r_contig = __shfl(row.contig, r, 64), r_pos = __shfl(row.pos, r, 64), r_end = __shfl(row.end, r, 64);
    const uint64_t r_toff = ((uint64_t)__shfl((uint32_t)(toff >> 32), r, 64) << 32) | __shfl((uint32_t)toff, r, 64);
    const uint64_t r_coff = ((uint64_t)__shfl((uint32_t)(coff >> 32), r, 64) << 32) | __shfl((uint32_t)coff, r, 64);
    if (r_toff + r_hdr + 2ull * r_np + 4ull > B.out_cap[r_m]) {
      flags |= 4u;
      continue;
    }
    const uint8_t* bases = B.out[r_m] + r_toff + r_hdr;
    TagRow tr = {0u, 0u, 0u};
    if (r_ops && (T.tags & (kTagNM | kTagMD))) {
      const uint64_t len = (uint32_t)r_contig < T.n_refs ? T.refs[r_contig].length : 0ull;
      if (r_pos < 0 || r_end < r_pos || (uint64_t)r_end > len) {
        flags |= 2u;
        continue;
      }
      const WaveSeq S = {bases, r_np, r_rev};
      const TagWalk W = wave_tags_walk<false>(cig + r_cig, r_ops, S, T.ref_codes + T.refs[r_contig].code_off + (uint64_t)r_pos, len - (uint64_t)r_pos,
                                              lane, nullptr, 0u);
      if (W.q_end != r_np || W.r_end != (uint64_t)(r_end - r_pos)) {
        flags |= 1u;
        continue;
      }
      tr.nm = W.nm;
      tr.md_len = W.md_len > kTruthMaxMd ? kMdDropped : W.md_len;
    }
    if (r_inside && (T.tags & kTagXE)) {
      const uint32_t* ev = B.events + ((size_t)r_m * B.n_slots + (blockIdx.x * 64u + r) / (B.paired ? 2u : 1u)) * SG_MAX_EVENTS;
      tr.xe = wave_xe(ev, r_nev, L, r_np, r_rev, B.chains + r_coff, bases, lane);
      if (tr.xe == kErrWalkBad) {
        flags |= 1u;
        continue;
      }
    }
    if (lane == r) mine = tr;
  }
  // ---- the rows, the records' lengths, the call's sums ----
  const bool counted = live && fits;
  const uint32_t present = counted ? tags_present(T.tags, mapped, g.inside, mine.md_len) : 0u;
  const uint32_t bytes = truth_tag_bytes(present, mine.md_len);
  if (counted) {
    T.rows[idx] = mine;
    J.rec_len[idx] = rec_len + bytes;
  }
  const unsigned long long has_nm = __ballot((present & kTagNM) != 0u), has_md = __ballot((present & kTagMD) != 0u);
  const unsigned long long has_xe = __ballot((present & kTagXE) != 0u);
  const unsigned long long dropped = __ballot(counted && mapped && (T.tags & kTagMD) && mine.md_len == kMdDropped);
  unsigned long long s_nm = (present & kTagNM) ? mine.nm : 0u, s_xe = (present & kTagXE) ? mine.xe : 0u, s_bytes = bytes;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    s_nm += __shfl_xor(s_nm, d, 64);
    s_xe += __shfl_xor(s_xe, d, 64);
    s_bytes += __shfl_xor(s_bytes, d, 64);
  }
  if (lane == 0u) {
    if (has_nm) atomicAdd(&T.counters[0], (unsigned long long)__popcll(has_nm));
    if (has_md) atomicAdd(&T.counters[1], (unsigned long long)__popcll(has_md));
    if (has_xe) atomicAdd(&T.counters[2], (unsigned long long)__popcll(has_xe));
    if (s_nm) atomicAdd(&T.counters[3], s_nm);
    if (s_xe) atomicAdd(&T.counters[4], s_xe);
    if (dropped) atomicAdd(&T.counters[5], (unsigned long long)__popcll(dropped));
    if (s_bytes) atomicAdd(&T.counters[6], s_bytes);
    if (flags) atomicOr(&T.counters[7], (unsigned long long)flags);
  }
}

}  // namespace

void launch_truth_tag_size(const DevProfile& P, const DevBatch& B, const TruthJob& J, const TagJob& T, hipStream_t s) {
  if (!J.map.n_reads) return;
  hipLaunchKernelGGL(truth_tag_size_kernel, dim3((J.map.n_reads + 63u) / 64u), dim3(64), 0, s, P, B, J, T);
}

}  // namespace sg
