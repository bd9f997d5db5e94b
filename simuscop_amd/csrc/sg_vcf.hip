// sg_vcf.hip -- a VCF of known variants on the device: the text of one call (the unfinished line of the call before in
// front) -> the parser's fragments -> their verdicts -> the kept rows of each kind in file order.  The rule is sg_vcf.h's.
//
//   vcf_breaks_kernel      thread = 64 bytes of text: its line breaks (the count the first scan runs over)
//   vcf_lines_kernel       thread = 64 bytes of text: one past every line break -> line_stop, in order
//   vcf_lines_info_kernel  one thread: how many lines the call has, where the unfinished one starts; at the end of the
//                          text a last line without a line break is a line
//   vcf_frag_count_kernel  lane = line: ceil(bytes / 19999) fragments (the count the second scan runs over)
//   vcf_rows_kernel        lane = line: its fragments' starts and lengths, and for every one vcf_decide -- the kind, the
//                          known-contig flag, the row's values --, the five list flags, and the three counts summed over the wave
//   (five scans)           launch_scan_u32 over the list flags: kept SNV / insertion / deletion, malformed, undecided
//   vcf_compact_kernel     lane = fragment: its row, number or (number, start, length) to its slot
// Integer work throughout.  Lane = line, as the SAM field kernel: a line is a few hundred bytes, its bytes are read once.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sg_vcf.h"

namespace sg {

namespace {

__device__ __forceinline__ uint32_t breaks_in_word(uint32_t w) {
  const uint32_t x = w ^ 0x0A0A0A0Au;                                            // zero bytes where a line break stands
  return (uint32_t)__popc(~((((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) | 0x7F7F7F7Fu));   // 0x80 in exactly those bytes
}

__global__ __launch_bounds__(256) void vcf_breaks_kernel(VcfJob J) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= J.n_blocks) return;
  const uint64_t a = (uint64_t)i * 64, e = a + 64 < J.bytes ? a + 64 : J.bytes;
  uint32_t c = 0;
  if (e - a == 64) {   // (the text buffer is 16-byte aligned)
    const uint4* p = (const uint4*)(J.text + a);
    for (int q = 0; q < 4; q++) {
      const uint4 v = p[q];
      c += breaks_in_word(v.x) + breaks_in_word(v.y) + breaks_in_word(v.z) + breaks_in_word(v.w);
    }
  } else {
    for (uint64_t b = a; b < e; b++) c += J.text[b] == '\n';
  }
  J.block_breaks[i] = c;
}

__global__ __launch_bounds__(256) void vcf_lines_kernel(VcfJob J) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= J.n_blocks || !J.block_breaks[i]) return;
  const uint64_t a = (uint64_t)i * 64, e = a + 64 < J.bytes ? a + 64 : J.bytes;
  uint64_t k = J.block_first[i];
  for (uint64_t b = a; b < e; b++)
    if (J.text[b] == '\n') J.line_stop[k++] = b + 1;
}

__global__ void vcf_lines_info_kernel(VcfJob J) {
  if (blockIdx.x || threadIdx.x) return;
  const uint64_t n = J.info[0];
  const uint64_t tail = n ? J.line_stop[n - 1] : 0;
  uint64_t lines = n;
  if (J.final_call && tail < J.bytes) { J.line_stop[n] = J.bytes; lines = n + 1; }
  J.info[1] = lines;
  J.info[2] = lines > n ? J.bytes : tail;
}

__global__ __launch_bounds__(256) void vcf_frag_count_kernel(VcfJob J) {
  const uint32_t li = blockIdx.x * blockDim.x + threadIdx.x;
  if (li >= J.n_lines) return;
  if (li >= J.info[1]) { J.frag_count[li] = 0; return; }   // (n_lines is the host's bound: the line breaks + 1)
  const uint64_t len = J.line_stop[li] - (li ? J.line_stop[li - 1] : 0);
  J.frag_count[li] = (uint32_t)((len + kVcfFragment - 1) / kVcfFragment);
  // the longest line and where it starts (both below 2^31): the host refuses one that is too long before any lane walks it
  if (len > kVcfFragment) atomicMax((unsigned long long*)J.info + 12, (unsigned long long)((len << 32) | (J.line_stop[li] - len)));
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {   // the sum over the wave's 64 lanes, in lane 0
  for (int off = 32; off; off >>= 1) v += __shfl_down(v, off);
  return v;
}

__global__ __launch_bounds__(256) void vcf_rows_kernel(VcfJob J) {
  const uint32_t li = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = li < J.n_lines && li < J.info[1];   // (no early return: every lane takes part in the sums below)
  const uint64_t start = live && li ? J.line_stop[li - 1] : 0, stop = live ? J.line_stop[li] : 0;
  uint64_t f = live ? J.frag_first[li] : 0;
  uint32_t n_snv = 0, n_ins = 0, n_del = 0;
  for (uint64_t a = start; a < stop; a += kVcfFragment, f++) {
    const uint32_t len = stop - a < kVcfFragment ? (uint32_t)(stop - a) : kVcfFragment;
    sg_vcf_record R;
    const uint32_t kind = vcf_decide(J.text + a, len, J.keys, J.n_keys, &R);
    R.fragment = J.first_number + f + 1;
    const bool known = (R.flags & SG_VCF_KNOWN) != 0;
    J.frag_start[f] = a;
    J.frag_len[f] = len;
    J.rows[f] = R;
    J.flag[0][f] = kind == SG_VCF_SNV && known;
    J.flag[1][f] = kind == SG_VCF_INS && known;
    J.flag[2][f] = kind == SG_VCF_DEL && known;
    J.flag[3][f] = kind == SG_VCF_MALFORMED;
    J.flag[4][f] = kind == SG_VCF_UNDECIDED;
    n_snv += kind == SG_VCF_SNV;
    n_ins += kind == SG_VCF_INS;
    n_del += kind == SG_VCF_DEL;
  }
  n_snv = wave_sum(n_snv); n_ins = wave_sum(n_ins); n_del = wave_sum(n_del);   // one atomic per wave and kind
  if ((threadIdx.x & 63u) == 0) {
    if (n_snv) atomicAdd((unsigned long long*)J.info + 9, (unsigned long long)n_snv);
    if (n_ins) atomicAdd((unsigned long long*)J.info + 10, (unsigned long long)n_ins);
    if (n_del) atomicAdd((unsigned long long*)J.info + 11, (unsigned long long)n_del);
  }
}

__global__ __launch_bounds__(256) void vcf_compact_kernel(VcfJob J) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= J.n_frags) return;
  for (int k = 0; k < 3; k++)
    if (J.flag[k][f]) J.out[k][J.out_first[k] + J.slot[k][f]] = J.rows[f];
  if (J.flag[3][f]) J.malformed[J.slot[3][f]] = J.rows[f].fragment;
  if (J.flag[4][f]) J.undecided[J.slot[4][f]] = sg_vcf_fragment{J.rows[f].fragment, J.frag_start[f], J.frag_len[f], 0u};
}

inline dim3 grid_of(uint32_t n) { return dim3((n + 255) / 256); }

}  // namespace

void launch_vcf_breaks(const VcfJob& J, hipStream_t s) {
  if (J.n_blocks) hipLaunchKernelGGL(vcf_breaks_kernel, grid_of(J.n_blocks), dim3(256), 0, s, J);
}
void launch_vcf_lines(const VcfJob& J, hipStream_t s) {
  if (J.n_blocks) hipLaunchKernelGGL(vcf_lines_kernel, grid_of(J.n_blocks), dim3(256), 0, s, J);
  hipLaunchKernelGGL(vcf_lines_info_kernel, dim3(1), dim3(64), 0, s, J);
}
void launch_vcf_frag_count(const VcfJob& J, hipStream_t s) {
  if (J.n_lines) hipLaunchKernelGGL(vcf_frag_count_kernel, grid_of(J.n_lines), dim3(256), 0, s, J);
}
void launch_vcf_rows(const VcfJob& J, hipStream_t s) {
  if (J.n_lines) hipLaunchKernelGGL(vcf_rows_kernel, grid_of(J.n_lines), dim3(256), 0, s, J);
}
void launch_vcf_compact(const VcfJob& J, hipStream_t s) {
  if (J.n_frags) hipLaunchKernelGGL(vcf_compact_kernel, grid_of(J.n_frags), dim3(256), 0, s, J);
}

}  // namespace sg
