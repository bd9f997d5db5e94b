// sg_errors.hip -- true error counts per cycle and quality (simuReads --truth-errors), gfx950.
//
// After a pass the device holds every read's text, the haplotype bases it was cut from and its sequencing indels; the
// rule that lays one over the other is errtab_walk (sg_truth.h, DESIGN.md "True error counts").  Counts add up over
// passes, chromosomes and populations, so nothing is sorted and nothing is kept per read.
//   errtab_add_kernel   grid (x, cycle window, mate), 1024 threads.  A wave takes 64 consecutive slots of its mate at a
//                       time.  Phase A, lane = read: the read's geometry (read_geom), where its text starts, where its
//                       template starts in the chains.  Phase B, read by read, lane = cycle: the wave-uniform walk over
//                       the read's events (usually none) tells lane i which template base read position 64c + i pairs
//                       with; the lane loads its base byte, its quality byte (64 consecutive bytes each) and its chain
//                       code and bumps one cell of the workgroup's LDS slabs hit[q][cycle] / miss[q][cycle].  Within
//                       a wave every lane owns its own bank (the slab's rows are a multiple of 64 cells), so the LDS
//                       adds never conflict; waves share the slabs, hence ds_add and not a plain store.  The
//                       substitution matrix is staged the same way in sub[cell][lane].  All of it leaves once per
//                       workgroup as 64-bit global adds of the cells that are not zero.  What is sparse goes to global
//                       memory at once: `other`, `inserted`, the indel rows, cycles behind the last window's slab.
//                       A window stages win_cycles cycles; the windows tile [0, L), the last one also takes the
//                       positions insertions push beyond it.
#include <algorithm>

#include "sg_truth.h"

namespace sg {
namespace {

constexpr uint32_t kErrThreads = 1024;
constexpr uint32_t kErrSubCells = 20;

__global__ __launch_bounds__(kErrThreads) void errtab_add_kernel(DevProfile P, DevBatch B, ErrtabJob J) {
  extern __shared__ uint32_t err_lds[];
  const uint32_t W = J.win_cycles, nq = J.d.n_qual, L = J.d.L;
  uint32_t* const hit = err_lds;               // [nq][W] paired bases that show their template's letter
  uint32_t* const miss = hit + nq * W;         // [nq][W] ... that do not
  uint32_t* const sub = miss + nq * W;         // [20][64] from * 5 + to, a column per lane
  const uint32_t n_lds = 2u * nq * W + kErrSubCells * 64u;
  for (uint32_t i = threadIdx.x; i < n_lds; i += blockDim.x) err_lds[i] = 0u;
  __syncthreads();

  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  const uint32_t m = blockIdx.z, w0 = blockIdx.y * W;
  const bool first = blockIdx.y == 0u, last = blockIdx.y + 1u == gridDim.y;
  const uint32_t n_groups = (B.n_slots + 63u) >> 6;
  uint32_t n_bases = 0, n_errors = 0, n_reads = 0, n_skipped = 0, flags = 0;

  for (uint32_t g = blockIdx.x * waves + wave; g < n_groups; g += gridDim.x * waves) {
    // ---- phase A: lane = read ----
    const uint32_t t = g * 64u + lane;
    ReadGeom geo = {};
    if (t < B.n_slots) geo = read_geom(P, B, t, m);
    const bool use = geo.live && geo.inside;
    uint64_t toff = 0, coff = 0;
    if (use) {
      toff = text_offset(B, m, t);
      coff = B.chain_off[geo.chain] + geo.tmpl_off;
    }
    const uint32_t packed = row::pack_y(geo.np, geo.nev, geo.hdr);   // 16 + 6 + 10 bits, as the meta row holds them
    unsigned long long todo = __ballot(use);
    const unsigned long long outside = __ballot(geo.live && !geo.inside);
    if (first && lane == 0u) n_skipped += (uint32_t)__popcll(outside);
    // ---- phase B: read by read, lane = cycle ----
    while (todo) {
      const uint32_t r = (uint32_t)__ffsll((long long)todo) - 1u;
      todo &= todo - 1ull;
      const uint32_t pk = __shfl(packed, r, 64), rev = __shfl(geo.reverse, r, 64);
      const uint64_t r_toff = ((uint64_t)__shfl((uint32_t)(toff >> 32), r, 64) << 32) | __shfl((uint32_t)toff, r, 64);
      const uint64_t r_coff = ((uint64_t)__shfl((uint32_t)(coff >> 32), r, 64) << 32) | __shfl((uint32_t)coff, r, 64);
      const uint32_t np = row::np(pk), nev = row::nev(pk), hdr = row::hdr_len(pk);
      const uint32_t* ev = B.events + ((size_t)m * B.n_slots + (g * 64u + r)) * SG_MAX_EVENTS;
      // the read as a whole: a read refused here counts nowhere (a quality byte outside the range refuses its base alone,
      // below; either way the call fails and the table is undefined until it is reset)
      uint32_t bad = 0;
      if (np > J.d.cycles) bad = 4u;
      else if (r_toff + hdr + 2ull * np + 4ull > B.out_cap[m]) bad = 16u;
      else if (errtab_walk(ev, nev, L, [](uint32_t, uint32_t, uint32_t, uint32_t) {}) != np) bad = 2u;
      if (bad) {
        flags |= bad;
        continue;
      }
      if (first) {
        n_reads += lane == 0u ? 1u : 0u;
        if (nev && lane == 0u)   // the indel rows: sparse, one lane
          errtab_walk(ev, nev, L, [&](uint32_t kind, uint32_t j, uint32_t, uint32_t n) {
            if (kind == 0u) return;
            unsigned long long* row = J.table + errtab_indel(J.d, kind == 2u ? 1u : 0u, m, j);
            atomicAdd(row, 1ull);
            atomicAdd(row + 1, (unsigned long long)n);
          });
      }
      const uint8_t* text = B.out[m] + r_toff + hdr;
      const uint32_t c_end = last ? np : min(np, w0 + W);
      for (uint32_t c = w0; c < c_end; c += 64u) {
        const uint32_t pos = c + lane;
        if (pos >= np) continue;
        const uint32_t ch = text[pos], qb = text[np + 3u + pos];
        uint32_t cls = 2u, j = 0u;
        errtab_walk(ev, nev, L, [&](uint32_t kind, uint32_t j0, uint32_t r0, uint32_t n) {
          if (kind < 2u && pos - r0 < n) { cls = kind; j = j0 + (pos - r0); }   // (pos < r0 wraps to a large number)
        });
        const uint32_t q = qb - 33u - J.d.qual_lo;
        if (qb < 33u + J.d.qual_lo || q >= nq) {
          flags |= 8u;
        } else if (cls == 1u) {
          atomicAdd(J.table + errtab_q(J.d, m, pos, q) + kErrInserted, 1ull);
        } else if (cls == 0u && j < L) {
          const uint32_t tc = errtab_tmpl_code(B.chains[r_coff + (rev ? L - 1u - j : j)], rev != 0u);
          if (tc >= 4u) {
            atomicAdd(J.table + errtab_q(J.d, m, pos, q) + kErrOther, 1ull);
          } else {
            const uint32_t rc = errtab_read_code(ch);
            const bool wrong = rc != tc;
            if (pos - w0 < W) {
              atomicAdd((wrong ? miss : hit) + q * W + (pos - w0), 1u);
            } else {   // behind the last window's slab: a read that insertions made longer
              unsigned long long* cell = J.table + errtab_q(J.d, m, pos, q);
              atomicAdd(cell + kErrBases, 1ull);
              if (wrong) atomicAdd(cell + kErrErrors, 1ull);
            }
            atomicAdd(sub + (tc * 5u + rc) * 64u + lane, 1u);
            n_bases++;
            n_errors += wrong ? 1u : 0u;
          }
        }
      }
    }
  }

  // ---- the workgroup's counts leave ----
  unsigned long long s_bases = n_bases, s_errors = n_errors;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    s_bases += __shfl_xor(s_bases, d, 64);
    s_errors += __shfl_xor(s_errors, d, 64);
  }
  if (lane == 0u) {
    if (s_bases) atomicAdd(&J.counters[0], s_bases);
    if (s_errors) atomicAdd(&J.counters[1], s_errors);
    if (n_skipped) atomicAdd(&J.counters[2], (unsigned long long)n_skipped);
    if (n_reads) atomicAdd(&J.counters[3], (unsigned long long)n_reads);
  }
  if (flags) atomicOr(&J.counters[4], (unsigned long long)flags);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < nq * W; i += blockDim.x) {
    const uint32_t a = hit[i], b = miss[i];
    if (!(a | b)) continue;
    const uint32_t cyc = w0 + i % W;
    if (cyc >= J.d.cycles) continue;   // (no read that long was counted)
    unsigned long long* cell = J.table + errtab_q(J.d, m, cyc, i / W);
    atomicAdd(cell + kErrBases, (unsigned long long)a + b);
    if (b) atomicAdd(cell + kErrErrors, (unsigned long long)b);
  }
  if (threadIdx.x < kErrSubCells) {
    unsigned long long sum = 0;
    for (uint32_t l = 0; l < 64u; l++) sum += sub[threadIdx.x * 64u + l];
    if (sum) atomicAdd(J.table + errtab_s(J.d, m, threadIdx.x / 5u, threadIdx.x % 5u), sum);
  }
}

}  // namespace

// the cycles a workgroup stages: all of the template when the budget allows, else the most whole 64-cycle chunks that fit
uint32_t errtab_win_cycles(const ErrtabDims& d) {
  const uint32_t want = (d.L + 63u) & ~63u;
  const uint32_t room = ((kErrLdsBudget - kErrSubCells * 64u * 4u) / (8u * d.n_qual)) & ~63u;
  return want < room ? want : room;
}

void launch_errtab_add(const DevProfile& P, const DevBatch& B, const ErrtabJob& J, uint32_t n_cus, hipStream_t s) {
  if (!B.n_slots || !J.win_cycles) return;
  const uint32_t nm = B.paired ? 2u : 1u, windows = (J.d.L + J.win_cycles - 1u) / J.win_cycles;
  const uint32_t groups = (B.n_slots + 63u) >> 6, waves = kErrThreads / 64u;
  const uint32_t fill = (2u * (n_cus ? n_cus : 256u) + windows * nm - 1u) / (windows * nm);   // two workgroups a CU over all of the grid
  const uint32_t gx = std::max(1u, std::min((groups + waves - 1u) / waves, fill));
  const size_t lds = ((size_t)2 * J.d.n_qual * J.win_cycles + kErrSubCells * 64u) * 4;
  (void)hipFuncSetAttribute((const void*)errtab_add_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(errtab_add_kernel, dim3(gx, windows, nm), dim3(kErrThreads), lds, s, P, B, J);
}

}  // namespace sg
