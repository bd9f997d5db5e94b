// sg_eval.hip -- the kernels of truthEval (the rule: sg_eval.h).  Every kernel is lane = record (or row) over the record
// starts that bam_guess / bam_verify / bam_starts left (sg_bam.hip); a record is parsed and checked by sg_bam_record.h's
// parse, as bam_measure_kernel does, and only read inside its own block_size.
//   the truth   eval_truth_rows_kernel   check, key, span, class: one EvalRow per record; the name's length
//               eval_truth_names_kernel  (after the scan of the lengths) the name bytes into the arena
//               eval_sort_input_kernel   (key, row) pairs for the radix passes of sg_bamsort.hip
//               eval_duplicates_kernel   (after the sort) a row whose run of equal keys holds another row of equal name and
//                                        mate is a duplicate; every claim slot starts empty
//   the test    eval_lookup_kernel       binary search of the key, then the run of equal keys against the arena
//               eval_claim_kernel        atomicMin of the record's ordinal in the file into its row's slot
//               eval_score_kernel        the record whose ordinal is in the slot is classified; the others are `repeated`
//   the end     eval_missing_kernel      rows nobody claimed
// Counting: a workgroup counts into a table in LDS (u32 cells: [mate][class][MAPQ][category], 48 KiB, and the scalars behind
// it), walks its records in a grid-stride loop and adds its non-zero cells to the u64 table in memory once, at its end.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sg_bam.h"
#include "sg_bam_record.h"
#include "sg_eval.h"

namespace sg {

namespace {

constexpr uint32_t kScoreThreads = 256, kScoreBlocks = 512;

// bytes of the name in front of its NUL
__device__ __forceinline__ uint32_t name_bytes(const uint8_t* d, const Rec& R) {
  uint32_t n = 0;
  while (n + 1 < R.lname && d[R.name + n]) n++;
  return n;
}
// the record's own operations (a kSmN placeholder has the span of the CIGAR it stands for)
__device__ __forceinline__ uint64_t ref_span(const uint8_t* d, const Rec& R) {
  if (!R.ncig) return 1;
  uint64_t span = 0;
  for (uint32_t i = 0; i < R.ncig; i++) {
    const uint32_t c = rd32(d, R.cig + 4ull * i), op = c & 15u;
    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += c >> 4;
  }
  return span;
}
__device__ __forceinline__ void report(const EvalJob& E, uint64_t o, uint32_t code) {
  atomicMin(E.error, (unsigned long long)((o << 8) | code));
}

__global__ __launch_bounds__(256) void eval_truth_rows_kernel(BamJob B, EvalJob E) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B.n_rec) return;
  const uint64_t o = B.rec[i];
  Rec R;
  const uint32_t code = parse(B, o, R);
  EvalRow row;
  row.key = 0; row.name_off = 0; row.span = 0; row.ref = -1; row.pos = -1; row.bits = 0; row.pad = 0;
  uint32_t len = 0;
  if (code != kBamOk) {
    report(E, o, code);
  } else {
    len = name_bytes(B.d, R);
    const uint32_t mate = (R.flag & 0x80u) ? 1u : 0u, unmapped = (R.flag & 4u) ? 1u : 0u;
    const uint32_t cls = unmapped ? kEvalUnmapped : (R.ncig == 1 && (B.d[R.cig] & 15u) == 0) ? kEvalPlain : kEvalEdited;
    row.key = eval_key(B.d + R.name, len, mate, E.key_bits);
    row.span = ref_span(B.d, R);
    row.ref = R.ref;
    row.pos = R.pos;
    row.bits = len | ((R.flag & 0x10u) ? kRowReverse : 0u) | (unmapped ? kRowUnmapped : 0u) | (cls << 10) | (mate ? kRowMate : 0u);
  }
  E.rows[E.n_rows + i] = row;
  E.name_len[i] = len;
}

__global__ __launch_bounds__(256) void eval_truth_names_kernel(BamJob B, EvalJob E) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B.n_rec) return;
  const uint32_t len = E.name_len[i];
  const uint64_t at = E.arena_used + E.name_at[i], src = B.rec[i] + 36;
  for (uint32_t k = 0; k < len; k++) E.arena[at + k] = B.d[src + k];
  E.rows[E.n_rows + i].name_off = at;
}

__global__ __launch_bounds__(256) void eval_sort_input_kernel(const EvalRow* rows, uint32_t n, uint64_t* keys, uint32_t* vals) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  keys[i] = rows[i].key;
  vals[i] = i;
}

// row r names the read (name bytes at `name`, len, mate)
__device__ __forceinline__ bool same_read(const EvalJob& E, const EvalRow& r, const uint8_t* name, uint32_t len, uint32_t mate) {
  if (row_name_len(r.bits) != len || ((r.bits & kRowMate) ? 1u : 0u) != mate) return false;
  const uint8_t* a = E.arena + r.name_off;
  for (uint32_t k = 0; k < len; k++)
    if (a[k] != name[k]) return false;
  return true;
}

__global__ __launch_bounds__(256) void eval_duplicates_kernel(EvalJob E, uint32_t n) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t r = E.order[j];
  const uint64_t k = E.keys[j];
  const EvalRow me = E.rows[r];
  const uint8_t* name = E.arena + me.name_off;
  const uint32_t len = row_name_len(me.bits), mate = (me.bits & kRowMate) ? 1u : 0u;
  bool dup = false;
  for (uint32_t q = j; !dup && q > 0 && E.keys[q - 1] == k; q--) dup = same_read(E, E.rows[E.order[q - 1]], name, len, mate);
  for (uint32_t q = j + 1; !dup && q < n && E.keys[q] == k; q++) dup = same_read(E, E.rows[E.order[q]], name, len, mate);
  if (dup) {
    atomicOr(&E.rows[r].bits, kRowDup);
    atomicAdd(E.dup_count, 1ull);
  }
  E.claim[r] = ~0ull;
}

__global__ __launch_bounds__(256) void eval_lookup_kernel(BamJob B, EvalJob E) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B.n_rec) return;
  const uint64_t o = B.rec[i];
  Rec R;
  const uint32_t code = parse(B, o, R);
  uint8_t hit = kHitUnknown;
  uint32_t hit_row = 0;
  if (code != kBamOk) {
    report(E, o, code);
  } else if (R.flag & 0x100u) {
    hit = kHitSecondary;
  } else if (R.flag & 0x800u) {
    hit = kHitSupplementary;
  } else {
    const uint32_t len = name_bytes(B.d, R), mate = (R.flag & 0x80u) ? 1u : 0u;
    const uint8_t* name = B.d + R.name;
    const uint64_t k = eval_key(name, len, mate, E.key_bits);
    uint64_t lo = 0, hi = E.n_rows;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (E.keys[mid] < k) lo = mid + 1;
      else hi = mid;
    }
    for (uint64_t q = lo; q < E.n_rows && E.keys[q] == k; q++) {
      const uint32_t r = E.order[q];
      const EvalRow row = E.rows[r];
      if (same_read(E, row, name, len, mate)) {
        hit = (row.bits & kRowDup) ? kHitAmbiguous : kHitRow;
        hit_row = r;
        break;
      }
    }
  }
  E.hit[i] = hit;
  E.hit_row[i] = hit_row;
}

__global__ __launch_bounds__(256) void eval_claim_kernel(BamJob B, EvalJob E) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B.n_rec || E.hit[i] != kHitRow) return;
  atomicMin(&E.claim[E.hit_row[i]], (unsigned long long)(E.ordinal0 + i));
}

constexpr uint32_t kScoreCells = kEvalCells + kEvalScalars;

__global__ __launch_bounds__(kScoreThreads) void eval_score_kernel(BamJob B, EvalJob E) {
  __shared__ uint32_t cells[kScoreCells];
  for (uint32_t c = threadIdx.x; c < kScoreCells; c += kScoreThreads) cells[c] = 0;
  __syncthreads();
  for (uint64_t i = (uint64_t)blockIdx.x * kScoreThreads + threadIdx.x; i < B.n_rec; i += (uint64_t)gridDim.x * kScoreThreads) {
    const uint8_t hit = E.hit[i];
    atomicAdd(&cells[kEvalCells + kEvalNTest], 1u);
    if (hit == kHitSecondary) { atomicAdd(&cells[kEvalCells + kEvalNSecondary], 1u); continue; }
    if (hit == kHitSupplementary) { atomicAdd(&cells[kEvalCells + kEvalNSupplementary], 1u); continue; }
    if (hit == kHitUnknown) { atomicAdd(&cells[kEvalCells + kEvalNUnknown], 1u); continue; }
    if (hit == kHitAmbiguous) { atomicAdd(&cells[kEvalCells + kEvalNAmbiguous], 1u); continue; }
    const uint32_t r = E.hit_row[i];
    if (E.claim[r] != E.ordinal0 + i) { atomicAdd(&cells[kEvalCells + kEvalNRepeated], 1u); continue; }
    Rec R;
    if (parse(B, B.rec[i], R) != kBamOk) continue;   // (the look-up kernel has reported it: the call fails)
    const EvalRow row = E.rows[r];
    EvalAln t, q;
    t.ref = row.ref; t.pos = row.pos; t.span = row.span; t.reverse = (row.bits & kRowReverse) ? 1u : 0u; t.unmapped = (row.bits & kRowUnmapped) ? 1u : 0u;
    q.ref = R.ref < 0 ? -1 : E.refmap[R.ref]; q.pos = R.pos; q.span = ref_span(B.d, R); q.reverse = (R.flag & 0x10u) ? 1u : 0u;
    q.unmapped = (R.flag & 4u) ? 1u : 0u;
    const uint32_t cat = eval_classify(t, q, E.pct);
    atomicAdd(&cells[eval_cell((row.bits & kRowMate) ? 1u : 0u, row_class(row.bits), R.mapq, cat)], 1u);
  }
  __syncthreads();
  for (uint32_t c = threadIdx.x; c < kScoreCells; c += kScoreThreads)
    if (cells[c]) atomicAdd(&E.table[c], (unsigned long long)cells[c]);
}

__global__ __launch_bounds__(kScoreThreads) void eval_missing_kernel(EvalJob E, uint64_t n) {
  __shared__ uint32_t cells[kEvalMissing];
  if (threadIdx.x < kEvalMissing) cells[threadIdx.x] = 0;
  __syncthreads();
  for (uint64_t r = (uint64_t)blockIdx.x * kScoreThreads + threadIdx.x; r < n; r += (uint64_t)gridDim.x * kScoreThreads) {
    const uint32_t bits = E.rows[r].bits;
    if (!(bits & kRowDup) && E.claim[r] == ~0ull) atomicAdd(&cells[((bits & kRowMate) ? 1u : 0u) * kEvalClasses + row_class(bits)], 1u);
  }
  __syncthreads();
  if (threadIdx.x < kEvalMissing && cells[threadIdx.x]) atomicAdd(&E.table[kScoreCells + threadIdx.x], (unsigned long long)cells[threadIdx.x]);
}

uint32_t blocks(uint64_t n, uint32_t t) { return (uint32_t)((n + t - 1) / t); }
uint32_t stride_blocks(uint64_t n) { return (uint32_t)std::min<uint64_t>((n + kScoreThreads - 1) / kScoreThreads, kScoreBlocks); }

}  // namespace

void launch_eval_truth_rows(const BamJob& B, const EvalJob& E, hipStream_t s) {
  if (B.n_rec) hipLaunchKernelGGL(eval_truth_rows_kernel, dim3(blocks(B.n_rec, 256)), dim3(256), 0, s, B, E);
}
void launch_eval_truth_names(const BamJob& B, const EvalJob& E, hipStream_t s) {
  if (B.n_rec) hipLaunchKernelGGL(eval_truth_names_kernel, dim3(blocks(B.n_rec, 256)), dim3(256), 0, s, B, E);
}
void launch_eval_sort_input(const EvalRow* rows, uint32_t n, uint64_t* keys, uint32_t* vals, hipStream_t s) {
  if (n) hipLaunchKernelGGL(eval_sort_input_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, rows, n, keys, vals);
}
void launch_eval_duplicates(const EvalJob& E, uint32_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL(eval_duplicates_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, E, n);
}
void launch_eval_lookup(const BamJob& B, const EvalJob& E, hipStream_t s) {
  if (B.n_rec) hipLaunchKernelGGL(eval_lookup_kernel, dim3(blocks(B.n_rec, 256)), dim3(256), 0, s, B, E);
}
void launch_eval_claim(const BamJob& B, const EvalJob& E, hipStream_t s) {
  if (B.n_rec) hipLaunchKernelGGL(eval_claim_kernel, dim3(blocks(B.n_rec, 256)), dim3(256), 0, s, B, E);
}
void launch_eval_score(const BamJob& B, const EvalJob& E, hipStream_t s) {
  if (B.n_rec) hipLaunchKernelGGL(eval_score_kernel, dim3(stride_blocks(B.n_rec)), dim3(kScoreThreads), 0, s, B, E);
}
void launch_eval_missing(const EvalJob& E, uint64_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL(eval_missing_kernel, dim3(stride_blocks(n)), dim3(kScoreThreads), 0, s, E, n);
}

}  // namespace sg
