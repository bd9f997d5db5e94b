// sg_variants.hip -- true allele counts per variant (simuReads --truth-variants), gfx950.
//
// For every row of a sorted variant table two uint32 counters: the reads whose template covers the site (total) and
// those whose haplotype shows the allele (alt); the rule is truth_variant_scan (sg_truth.h, DESIGN.md "True allele
// counts").  Counts add up over passes, chromosomes and populations, so nothing is sorted and nothing is kept per read.
//   variants_add_kernel   lane = read (index = slot * mates + mate, as truth_size_kernel): the read's geometry, the
//                         piece that holds its template's first base, the scan; a hit is one atomic add on the row's
//                         total and one on its alt when the read carries the allele.  Most reads hit nothing, and
//                         the hits of one site come from reads of different waves: scattered single dwords, sparse,
//                         so there is no LDS stage and nothing to merge inside a wave.  Per wave two 64-bit sums
//                         (reads with a hit, hits) go to the job's counters.
#include "sg_truth.h"

namespace sg {
namespace {

constexpr uint32_t kVarThreads = 256;

__global__ __launch_bounds__(kVarThreads) void variants_add_kernel(DevProfile P, DevBatch B, VariantJob J) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  const PassRead R = pass_read(B, idx, J.map.n_reads);
  ReadGeom g = {};
  if (R.in_range) g = read_geom(P, B, R.t, R.m);
  uint32_t hits = 0, flags = 0;
  if (g.live && g.inside && g.chain < J.map.n_chains) {
    const uint64_t first = J.map.chain_first[g.chain], last = J.map.chain_first[g.chain + 1];
    const uint64_t pi = first < last ? truth_find_piece(J.map.pieces, first, last, g.tmpl_off) : last;
    if (pi >= last || J.map.pieces[pi].dst > g.tmpl_off || g.tmpl_off - J.map.pieces[pi].dst >= J.map.pieces[pi].len) {
      flags = 1u;
    } else {
      const uint8_t* codes = B.chains + B.chain_off[g.chain];
      truth_variant_scan(J.map.pieces, last, pi, g.tmpl_off, (uint32_t)P.L, codes, 0, J.table, J.n_rows, [&](uint64_t row, bool alt) {
        atomicAdd(&J.counts[row * 2], 1u);
        if (alt) atomicAdd(&J.counts[row * 2 + 1], 1u);
        hits++;
      });
    }
  }
  unsigned long long n_hits = hits, n_reads = hits ? 1u : 0u;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    n_hits += __shfl_xor(n_hits, d, 64);
    n_reads += __shfl_xor(n_reads, d, 64);
  }
  if ((threadIdx.x & 63u) == 0u && n_hits) {
    atomicAdd(&J.counters[0], n_reads);
    atomicAdd(&J.counters[1], n_hits);
  }
  if (flags) atomicOr(&J.counters[2], (unsigned long long)flags);
}

}  // namespace

void launch_variants_add(const DevProfile& P, const DevBatch& B, const VariantJob& J, hipStream_t s) {
  if (!J.map.n_reads || !J.n_rows) return;
  hipLaunchKernelGGL(variants_add_kernel, dim3((J.map.n_reads + kVarThreads - 1u) / kVarThreads), dim3(kVarThreads), 0, s, P, B, J);
}

}  // namespace sg
