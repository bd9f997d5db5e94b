// sg_bam.hip -- BAM records of an inflated stream on the device (SAMv1 section 4.2), turned into the lines
// `samtools view -F 0xD04 -q 20` prints, for the training kernels of sg_train.hip.
//
// Record boundaries, exactly and without a serial walk over the records:
//   bam_guess_kernel   thread = 16 KiB segment of the stream: the first offset of the segment that looks like a record
//                      start (strict checks on the fixed fields, the name and the next record), then the chain of
//                      block_size from there to the segment's end: its exit and the records it started
//   bam_verify_kernel  one workgroup: the true chain enters segment b where it left segment b - 1.  Segments whose guess
//                      is that entry keep their exit and count; the others are walked again from the true entry (only
//                      where the guess was wrong: the serial part is O(segments), the segment walks are rare).  Where
//                      the chain stops (a record the stream does not hold whole) is the tail, carried into the next call
//   bam_starts_kernel  (after a scan of the counts) thread = segment: every record start, in stream order
// Then the lines:
//   bam_measure_kernel thread = record: the checks (block_size against the fixed fields, op codes, reference ids), the
//                      filter (flag & 0xD04) == 0 && mapq >= 20, the length of the rendered line (0: no line)
//   bam_render_kernel  (after a scan of the lengths) thread = record: QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL,
//                      tab separated, one line break; a CIGAR of more than 65,535 operations comes from its CG:B:I tag as
//                      htslib's bam_tag2cigar takes it
// Every read of the stream stays inside [0, L); a record is only read once its block_size says it lies there whole.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sg_bam.h"
#include "sg_bam_record.h"

namespace sg {

namespace {

// offset o starts something that looks like a record (a guess only: the verify pass decides)
__device__ bool plausible(const BamJob& J, uint64_t o) {
  const uint8_t* d = J.d;
  if (o + 36 > J.L) return false;
  const uint32_t bs = rd32(d, o);
  if (bs < 32 || bs > (1u << 28)) return false;
  const int32_t ref = (int32_t)rd32(d, o + 4), pos = (int32_t)rd32(d, o + 8), nref = (int32_t)rd32(d, o + 24), npos = (int32_t)rd32(d, o + 28);
  if (ref < -1 || ref >= (int32_t)J.n_ref || nref < -1 || nref >= (int32_t)J.n_ref || pos < -1 || npos < -1) return false;
  const uint32_t lname = d[o + 12], ncig = rd16(d, o + 16);
  const int32_t lseq = (int32_t)rd32(d, o + 20);
  if (lname < 1 || lseq < 0) return false;
  if (32ull + lname + 4ull * ncig + ((uint64_t)lseq + 1) / 2 + (uint64_t)lseq > bs) return false;
  const uint64_t nm = o + 36;
  if (nm + lname <= J.L) {
    if (d[nm + lname - 1] != 0) return false;
    for (uint32_t i = 0; i + 1 < lname; i++)
      if (d[nm + i] < 33 || d[nm + i] > 126) return false;
    const uint64_t cg = nm + lname;
    for (uint32_t i = 0; i < ncig && i < 16 && cg + 4 * i + 4 <= J.L; i++)
      if ((d[cg + 4 * i] & 15u) > 8) return false;
  }
  const uint64_t o2 = o + 4 + bs;   // the next record, where the stream holds its fixed fields
  if (o2 + 36 <= J.L) {
    const uint32_t bs2 = rd32(d, o2);
    const int32_t ref2 = (int32_t)rd32(d, o2 + 4);
    if (bs2 < 32 || bs2 > (1u << 28) || ref2 < -1 || ref2 >= (int32_t)J.n_ref || d[o2 + 12] < 1) return false;
  }
  return true;
}

// the chain of block_size from p up to `hi`: records it starts that the stream holds whole
__device__ __forceinline__ uint64_t walk(const BamJob& J, uint64_t p, uint64_t hi, uint32_t* cnt) {
  uint32_t n = 0;
  while (p < hi && p + 4 <= J.L) {
    const uint32_t bs = rd32(J.d, p);
    if (bs < 32 || p + 4 + bs > J.L) break;
    n++;
    p += 4 + bs;
  }
  *cnt = n;
  return p;
}

__device__ __forceinline__ void seg_range(const BamJob& J, uint32_t b, uint64_t* lo, uint64_t* hi) {
  *lo = J.base + (uint64_t)b * kBamSegment;
  *hi = *lo + kBamSegment < J.L ? *lo + kBamSegment : J.L;
}

__global__ __launch_bounds__(256) void bam_guess_kernel(BamJob J) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= J.n_seg) return;
  uint64_t lo, hi;
  seg_range(J, b, &lo, &hi);
  uint64_t g = ~0ull, p = ~0ull;
  uint32_t cnt = 0;
  if (b == 0) g = J.base;
  else
    for (uint64_t o = lo; o < hi; o++)
      if (plausible(J, o)) { g = o; break; }
  if (g != ~0ull) p = walk(J, g, hi, &cnt);
  J.guess[b] = g;
  J.exit[b] = p;
  J.count[b] = cnt;
}

constexpr uint32_t kVerifyTile = 1024;

__global__ __launch_bounds__(kVerifyTile) void bam_verify_kernel(BamJob J) {
  __shared__ uint64_t sg[kVerifyTile], se[kVerifyTile];
  __shared__ uint32_t sc[kVerifyTile];
  __shared__ uint64_t s_cur;
  __shared__ uint32_t s_ended;
  const uint32_t t = threadIdx.x;
  if (t == 0) { s_cur = J.base; s_ended = 0; }
  for (uint32_t t0 = 0; t0 < J.n_seg; t0 += kVerifyTile) {
    const uint32_t n = J.n_seg - t0 < kVerifyTile ? J.n_seg - t0 : kVerifyTile;
    if (t < n) { sg[t] = J.guess[t0 + t]; se[t] = J.exit[t0 + t]; sc[t] = J.count[t0 + t]; }
    __syncthreads();
    if (t == 0) {
      uint64_t cur = s_cur;
      uint32_t ended = s_ended;
      for (uint32_t j = 0; j < n; j++) {
        uint64_t lo, hi;
        seg_range(J, t0 + j, &lo, &hi);
        if (ended || cur >= hi) { sg[j] = cur; se[j] = cur; sc[j] = 0; continue; }   // no record starts here
        if (cur != sg[j]) {   // a wrong guess: the segment's records from the true entry
          uint32_t c;
          se[j] = walk(J, cur, hi, &c);
          sg[j] = cur;
          sc[j] = c;
        }
        cur = se[j];
        if (cur < hi) ended = 1;   // the chain stops inside this segment
      }
      s_cur = cur;
      s_ended = ended;
    }
    __syncthreads();
    if (t < n) { J.guess[t0 + t] = sg[t]; J.count[t0 + t] = sc[t]; }
    __syncthreads();
  }
  if (t == 0) {
    const uint64_t tail = s_cur;
    J.totals[2] = tail;
    if (tail + 4 <= J.L && rd32(J.d, tail) < 32) atomicMin((unsigned long long*)&J.totals[3], (unsigned long long)((tail << 8) | kBamShort));
  }
}

__global__ __launch_bounds__(256) void bam_starts_kernel(BamJob J) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= J.n_seg) return;
  uint64_t p = J.guess[b];
  const uint64_t f = J.first[b];
  const uint32_t n = J.count[b];
  for (uint32_t i = 0; i < n; i++) {
    J.rec[f + i] = p;
    p += 4 + rd32(J.d, p);
  }
}

struct Sink {
  char* out;
  uint64_t n;
  __device__ __forceinline__ void put(char c) {
    if (out) out[n] = c;
    n++;
  }
  __device__ void num(int64_t v) {
    if (v < 0) { put('-'); v = -v; }
    uint64_t u = (uint64_t)v, t = 1;
    uint32_t k = 1;
    while (u / t >= 10) { t *= 10; k++; }
    if (out)
      for (uint32_t i = 0; i < k; i++) { out[n + i] = (char)('0' + (u / t) % 10); t /= 10; }
    n += k;
  }
  __device__ void name(const BamJob& J, int32_t ref) {
    if (ref < 0) { put('*'); return; }
    const uint64_t a = J.name_off[ref], b = J.name_off[ref + 1] - 1;
    if (out)
      for (uint64_t i = a; i < b; i++) out[n + i - a] = J.names[i];
    n += b - a;
  }
};

__device__ uint64_t render(const BamJob& J, const Rec& R, char* out) {
  const uint8_t* d = J.d;
  Sink s{out, 0};
  for (uint32_t i = 0; i + 1 < R.lname && d[R.name + i]; i++) s.put((char)d[R.name + i]);
  s.put('\t');
  s.num(R.flag); s.put('\t');
  s.name(J, R.ref); s.put('\t');
  s.num((int64_t)R.pos + 1); s.put('\t');
  s.num(R.mapq); s.put('\t');
  if (!R.nops) s.put('*');
  for (uint32_t i = 0; i < R.nops; i++) {
    const uint32_t c = rd32(d, R.ops + 4ull * i);
    s.num(c >> 4);
    s.put("MIDNSHP=X"[c & 15u]);
  }
  s.put('\t');
  if (R.nref < 0) s.put('*');
  else if (R.nref == R.ref) s.put('=');
  else s.name(J, R.nref);
  s.put('\t');
  s.num((int64_t)R.npos + 1); s.put('\t');
  s.num(R.tlen); s.put('\t');
  const uint32_t L = (uint32_t)R.lseq;
  if (!L) s.put('*');
  if (out)
    for (uint32_t i = 0; i < L; i++) out[s.n + i] = "=ACMGRSVTWYHKDBN"[(d[R.seq + i / 2] >> ((~i & 1u) * 4)) & 15u];
  s.n += L;
  s.put('\t');
  if (!L || d[R.qual] == 0xFF) {
    s.put('*');
  } else {
    if (out)
      for (uint32_t i = 0; i < L; i++) out[s.n + i] = (char)(d[R.qual + i] + 33);
    s.n += L;
  }
  s.put('\n');
  return s.n;
}

__global__ __launch_bounds__(256) void bam_measure_kernel(BamJob J) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= J.n_rec) return;
  const uint64_t o = J.rec[i];
  Rec R;
  const uint32_t code = parse(J, o, R);
  uint32_t len = 0;
  if (code != kBamOk) atomicMin((unsigned long long*)&J.totals[3], (unsigned long long)((o << 8) | code));
  else if ((R.flag & 0xD04u) == 0 && R.mapq >= 20) len = (uint32_t)render(J, R, nullptr);
  J.line_len[i] = len;
}

__global__ __launch_bounds__(256) void bam_render_kernel(BamJob J) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= J.n_rec || !J.line_len[i]) return;
  Rec R;
  parse(J, J.rec[i], R);
  render(J, R, J.text + J.line_off[i]);
}

uint32_t blocks(uint64_t n, uint32_t t) { return (uint32_t)((n + t - 1) / t); }

}  // namespace

void launch_bam_guess(const BamJob& J, hipStream_t s) {
  if (J.n_seg) hipLaunchKernelGGL(bam_guess_kernel, dim3(blocks(J.n_seg, 256)), dim3(256), 0, s, J);
}
void launch_bam_verify(const BamJob& J, hipStream_t s) { hipLaunchKernelGGL(bam_verify_kernel, dim3(1), dim3(kVerifyTile), 0, s, J); }
void launch_bam_starts(const BamJob& J, hipStream_t s) {
  if (J.n_seg) hipLaunchKernelGGL(bam_starts_kernel, dim3(blocks(J.n_seg, 256)), dim3(256), 0, s, J);
}
void launch_bam_measure(const BamJob& J, hipStream_t s) {
  if (J.n_rec) hipLaunchKernelGGL(bam_measure_kernel, dim3(blocks(J.n_rec, 256)), dim3(256), 0, s, J);
}
void launch_bam_render(const BamJob& J, hipStream_t s) {
  if (J.n_rec) hipLaunchKernelGGL(bam_render_kernel, dim3(blocks(J.n_rec, 256)), dim3(256), 0, s, J);
}

}  // namespace sg
