// sg_api_train.cpp -- the C ABI of profile training, sg_train_* (kernels: sg_train.hip; the BAM input of sg_train_feed_bgzf
// comes in through SgBamStream, sg_api_bgzf.cpp).  A training session lives from sg_train_begin to sg_train_finish or
// sg_train_end; the context it runs on is sg_api.cpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "sg_api.h"
#include "sg_bam.h"
#include "sg_scan.h"
#include "sg_train.h"

extern "C" {

struct sg_train_session {
  char bases[4] = {0, 0, 0, 0};
  uint32_t kmer = 0, bins = 0, n_isize = 0, n_indel_len = 0, count_gc = 0, window = 1000, wes = 0, remap = 0;
  uint64_t max_reads = 300000000;    // Profile.cpp:236
  bool capped = false;               // the cap was reached: the reference has stopped reading
  uint32_t kc = 0, koff[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  size_t subs_n = 0, kmers_n = 0, qual_n = 0, counters = 0;
  uint32_t n_contigs = 0;
  DevBuf keys, contigs, counts, flags, text[2], line_end, reads, gate, steps, windows, window_rc, carry, scan_work, tgt, known, t_ref,
      t_alt, patch, gc_out;
  // Two text buffers and a copy stream: chunk k travels to text[k & 1] while the kernels of chunk k - 1 read the other one.
  hipStream_t copy_stream = nullptr;
  uint64_t fed = 0;                  // chunks handed to the kernels so far
  bool pending = false;              // a chunk's kernels are queued whose carry / flags have not been looked at yet
  uint64_t pending_lines = 0;
  bool own_codes = false;            // t_ref / t_alt are copies with the SNVs of the VCF in them
  uint64_t code_bytes = 0;
  uint64_t n_tgt = 0, n_ins = 0, n_del = 0;
  int cur = 0;                       // carry[cur] is read by the next chunk, carry[cur ^ 1] written
  uint64_t lines = 0, n_windows = 0; // lines fed / windows opened so far (host copies)
  uint64_t windows_cap = 0;          // rows the window arrays hold
  sg::TrainCarry* mail = nullptr;    // pinned: the carry a chunk left, the flag word behind it
  uint32_t* mail_flags() { return (uint32_t*)(mail + 1); }
  // BAM input (sg_train_bam_start, sg_train_feed_bgzf): the members come in through `in` (SgBamStream, sg_api.h); the lines of
  // its whole records are rendered into the text buffers above
  bool bam = false;
  SgBamStream in;                    // the members, the stream and its record starts (sg_api.h)
  double bam_seconds = 0;
  DevBuf line_len, line_off;
  ~sg_train_session() {   // (the buffers go with their members)
    if (copy_stream) { (void)hipStreamSynchronize(copy_stream); (void)hipStreamDestroy(copy_stream); }
    if (mail) (void)hipHostFree(mail);
  }
};

void sg_train_end(sg_ctx* ctx) {
  if (!ctx || !ctx->train) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  delete ctx->train;
  ctx->train = nullptr;
}

int sg_train_begin(sg_ctx* ctx, const sg_train_setup* st) {
  if (!ctx || !st || !st->bases || (st->n_contigs && !st->contig_keys)) return SG_ERR_INVALID;
  if (ctx->ref_contigs.empty() || st->n_contigs != ctx->ref_contigs.size())
    return ctx->fail(SG_ERR_INVALID, "sg_train_begin: name the contigs of sg_reference_commit, in its order");
  if (strlen(st->bases) != 4 || st->kmer < 1 || st->kmer > 6 || st->bins < 1 || st->n_isize < 1 || st->n_indel_len < 1 || st->window < 1)
    return ctx->fail(SG_ERR_UNSUPPORTED, "sg_train_begin: bases must hold four letters, kmer 1..6, bins >= 1");
  if ((st->n_snv && !(st->snv_contig && st->snv_pos && st->snv_alt && st->snv_homo)) || (st->n_ins && !(st->ins_contig && st->ins_pos && st->ins_len)) ||
      (st->n_del && !(st->del_contig && st->del_pos && st->del_len)) || (st->target_first && !(st->target_spos && st->target_epos)))
    return SG_ERR_INVALID;
  uint32_t remap = 0;
  {
    const char nat[4] = {'A', 'C', 'T', 'G'};
    for (int n = 0; n < 4; n++) {
      int code = -1;
      for (int k = 0; k < 4; k++) if (st->bases[k] == nat[n]) code = k;
      if (code < 0) return ctx->fail(SG_ERR_UNSUPPORTED, "sg_train_begin: bases must be a permutation of ACGT");
      remap |= (uint32_t)code << (2 * n);
    }
  }
  SG_HIP(hipSetDevice(ctx->device));
  sg_train_end(ctx);
  // the session is built aside and handed to the context only when all of it stands: on any failure below it is dropped
  std::unique_ptr<sg_train_session> T(new sg_train_session());
  memcpy(T->bases, st->bases, 4);
  T->kmer = (uint32_t)st->kmer; T->bins = (uint32_t)st->bins; T->n_isize = st->n_isize; T->n_indel_len = st->n_indel_len;
  T->count_gc = st->count_gc ? 1u : 0u; T->window = st->window; T->remap = remap; T->n_contigs = st->n_contigs;
  if (st->max_reads) T->max_reads = st->max_reads;
  {
    uint32_t p4 = 1;
    for (int m = 1; m <= st->kmer; m++) { T->koff[m] = T->kc; p4 *= 4; T->kc += p4; }
  }
  T->subs_n = (size_t)T->kc * T->bins * 4; T->kmers_n = (size_t)T->bins * T->kc; T->qual_n = (size_t)16 * T->bins * 94;
  T->counters = 2 * T->subs_n + T->kmers_n + T->qual_n + T->n_isize + 2 * (size_t)T->n_indel_len + sg::kTrainScalars;
  const uint32_t nc = st->n_contigs;
  hipStream_t s = ctx->stream;
  // ---- contigs, their targets (countGC's windows of an exome: [spos, epos - 1], Profile.cpp:590-593) ----
  std::vector<char> keys((size_t)nc * sg::kTrainKeyBytes, 0);
  std::vector<sg::TrainContig> tc(nc);
  uint64_t code_bytes = 0;
  for (uint32_t c = 0; c < nc; c++) {
    if (!st->contig_keys[c] || strlen(st->contig_keys[c]) >= sg::kTrainKeyBytes) return ctx->fail(SG_ERR_UNSUPPORTED, "sg_train_begin: contig name too long");
    strcpy(&keys[(size_t)c * sg::kTrainKeyBytes], st->contig_keys[c]);
    memset(&tc[c], 0, sizeof tc[c]);
    tc[c].code_off = ctx->ref_contigs[c].code_off;
    tc[c].length = ctx->ref_contigs[c].length;
    const std::string k = st->contig_keys[c];
    tc[c].xym = (k == "X" || k == "Y" || k == "M") ? 1u : 0u;
    code_bytes = std::max<uint64_t>(code_bytes, tc[c].code_off + ((tc[c].length + 15) / 16) * 16 + 64);
  }
  T->code_bytes = code_bytes;
  std::vector<int64_t> tgt;   // left[n], right[n], pmax[n]
  if (st->target_first && st->target_first[nc] > 0) {
    const uint64_t n = st->target_first[nc];
    T->n_tgt = n; T->wes = 1;
    tgt.resize(3 * n);
    for (uint32_t c = 0; c < nc; c++) {
      const uint64_t a = st->target_first[c], b = st->target_first[c + 1];
      if (b < a || b > n || b - a > 0xFFFFFFFFull) return ctx->fail(SG_ERR_INVALID, "sg_train_begin: target_first must ascend");
      tc[c].tgt_first = a; tc[c].tgt_n = (uint32_t)(b - a);
      int64_t pm = INT64_MIN;
      for (uint64_t t = a; t < b; t++) {
        // (loadTargets keeps 1 <= spos and epos <= the contig's length, divideTargets spos <= epos: Genome.cpp:270-279, 690-733)
        if (st->target_spos[t] < 0 || st->target_epos[t] < st->target_spos[t] || (uint64_t)st->target_epos[t] > tc[c].length)
          return ctx->fail(SG_ERR_INVALID, "sg_train_begin: a target leaves its contig");
        tgt[t] = st->target_spos[t];
        tgt[n + t] = st->target_epos[t] - 1;
        pm = std::max(pm, tgt[n + t]);
        tgt[2 * n + t] = pm;
      }
    }
  }
  // ---- known insertions / deletions per contig: file order (running maximum of the positions: where the reference's loop
  // stops, Profile.cpp:314-316) and (position, length) order (is the event there at all, and how early) ----
  std::vector<int64_t> kn64;   // per kind: pmax[n], pos[n]
  std::vector<int32_t> kn32;   // per kind: len[n], first[n] (as int32)
  auto stage_known = [&](uint64_t n, const uint32_t* contig, const int64_t* pos, const int32_t* len, bool ins) -> bool {
    std::vector<std::vector<uint64_t>> rows(nc);
    for (uint64_t i = 0; i < n; i++) {
      if (contig[i] >= nc) return false;
      rows[contig[i]].push_back(i);
    }
    const size_t b64 = kn64.size(), b32 = kn32.size();
    kn64.resize(b64 + 2 * n);
    kn32.resize(b32 + 2 * n);
    uint64_t at = 0;
    for (uint32_t c = 0; c < nc; c++) {
      const std::vector<uint64_t>& r = rows[c];
      if (r.size() > 0x7FFFFFFFull) return false;
      (ins ? tc[c].ins_first : tc[c].del_first) = at;
      (ins ? tc[c].ins_n : tc[c].del_n) = (uint32_t)r.size();
      int64_t pm = INT64_MIN;
      std::vector<uint32_t> order(r.size());
      for (size_t j = 0; j < r.size(); j++) {
        pm = std::max(pm, pos[r[j]]);
        kn64[b64 + at + j] = pm;
        order[j] = (uint32_t)j;
      }
      std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        if (pos[r[x]] != pos[r[y]]) return pos[r[x]] < pos[r[y]];
        return len[r[x]] < len[r[y]];
      });
      for (size_t j = 0; j < r.size(); j++) {
        kn64[b64 + n + at + j] = pos[r[order[j]]];
        kn32[b32 + at + j] = len[r[order[j]]];
        // the least file-order index of this (position, length): stable_sort keeps file order inside equal keys
        const bool same = j > 0 && pos[r[order[j]]] == pos[r[order[j - 1]]] && len[r[order[j]]] == len[r[order[j - 1]]];
        kn32[b32 + n + at + j] = same ? kn32[b32 + n + at + j - 1] : (int32_t)order[j];
      }
      at += r.size();
    }
    return true;
  };
  T->n_ins = st->n_ins; T->n_del = st->n_del;
  if (!stage_known(st->n_ins, st->ins_contig, st->ins_pos, st->ins_len, true) || !stage_known(st->n_del, st->del_contig, st->del_pos, st->del_len, false))
    return ctx->fail(SG_ERR_INVALID, "sg_train_begin: a known insertion / deletion names no contig");
  // ---- SNVs: altSequence takes every one, refSequence the homozygous ones, later rows over earlier (Genome.cpp:469-475) ----
  std::map<uint64_t, char> alt_patch, ref_patch;
  for (uint64_t i = 0; i < st->n_snv; i++) {
    if (st->snv_contig[i] >= nc) return ctx->fail(SG_ERR_INVALID, "sg_train_begin: a known SNV names no contig");
    const sg::TrainContig& C = tc[st->snv_contig[i]];
    // (a position outside the contig writes outside the reference's string: skipped)
    if (st->snv_pos[i] < 1 || (uint64_t)st->snv_pos[i] > C.length) continue;
    const uint64_t off = C.code_off + (uint64_t)(st->snv_pos[i] - 1);
    alt_patch[off] = st->snv_alt[i];
    if (st->snv_homo[i]) ref_patch[off] = st->snv_alt[i];
  }
  // ---- device side ----
  auto up = [&](DevBuf& buf, const void* src, size_t bytes) -> int {
    SG_ENSURE(buf, bytes + 64);
    if (bytes) SG_HIP(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, s));
    return SG_OK;
  };
  int rc;
  if ((rc = up(T->keys, keys.data(), keys.size())) != SG_OK) return rc;
  if ((rc = up(T->contigs, tc.data(), tc.size() * sizeof(sg::TrainContig))) != SG_OK) return rc;
  if ((rc = up(T->tgt, tgt.data(), tgt.size() * 8)) != SG_OK) return rc;
  {
    std::vector<uint8_t> blob(kn64.size() * 8 + kn32.size() * 4);
    if (!kn64.empty()) memcpy(blob.data(), kn64.data(), kn64.size() * 8);
    if (!kn32.empty()) memcpy(blob.data() + kn64.size() * 8, kn32.data(), kn32.size() * 4);
    if ((rc = up(T->known, blob.data(), blob.size())) != SG_OK) return rc;
    SG_HIP(hipStreamSynchronize(s));
  }
  if (!alt_patch.empty()) {
    T->own_codes = true;
    SG_ENSURE(T->t_ref, code_bytes);
    SG_ENSURE(T->t_alt, code_bytes);
    SG_HIP(hipMemcpyAsync(T->t_ref.p, ctx->ref_codes.p, code_bytes, hipMemcpyDeviceToDevice, s));
    SG_HIP(hipMemcpyAsync(T->t_alt.p, ctx->ref_codes.p, code_bytes, hipMemcpyDeviceToDevice, s));
    for (int which = 0; which < 2; which++) {
      const std::map<uint64_t, char>& m = which ? ref_patch : alt_patch;
      if (m.empty()) continue;
      std::vector<uint64_t> off; std::vector<uint8_t> ch;
      off.reserve(m.size()); ch.reserve(m.size());
      for (const auto& kv : m) { off.push_back(kv.first); ch.push_back((uint8_t)kv.second); }
      SG_ENSURE(T->patch, off.size() * 9 + 64);
      uint8_t* d_ch = T->patch.as<uint8_t>() + off.size() * 8;
      SG_HIP(hipMemcpyAsync(T->patch.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, s));
      SG_HIP(hipMemcpyAsync(d_ch, ch.data(), ch.size(), hipMemcpyHostToDevice, s));
      sg::launch_train_patch((which ? T->t_ref : T->t_alt).as<uint8_t>(), T->patch.as<uint64_t>(), d_ch, off.size(), which == 0, s);
      SG_HIP(hipGetLastError());
      SG_HIP(hipStreamSynchronize(s));
    }
  }
  SG_ENSURE(T->counts, T->counters * 8);
  SG_ENSURE(T->flags, 64);
  SG_ENSURE(T->carry, 2 * sizeof(sg::TrainCarry) + 64);
  SG_HIP(hipMemsetAsync(T->counts.p, 0, T->counters * 8, s));
  SG_HIP(hipMemsetAsync(T->flags.p, 0, 64, s));
  SG_HIP(hipMemsetAsync(T->carry.p, 0, 2 * sizeof(sg::TrainCarry), s));
  SG_HIP(hipHostMalloc((void**)&T->mail, sizeof(sg::TrainCarry) + 64, hipHostMallocDefault));
  SG_HIP(hipStreamCreateWithFlags(&T->copy_stream, hipStreamNonBlocking));
  SG_HIP(hipStreamSynchronize(s));
  ctx->train = T.release();
  return SG_OK;
}

namespace {
void train_job(sg_ctx* ctx, sg_train_session* T, sg::TrainJob& J) {
  memset(&J, 0, sizeof J);
  J.keys = T->keys.as<char>();
  J.contigs = T->contigs.as<sg::TrainContig>();
  J.n_contigs = T->n_contigs;
  J.ref_codes = T->own_codes ? T->t_ref.as<uint8_t>() : ctx->ref_codes.as<uint8_t>();
  J.alt_codes = T->own_codes ? T->t_alt.as<uint8_t>() : ctx->ref_codes.as<uint8_t>();
  memcpy(J.bases, T->bases, 4);
  J.remap = T->remap;
  J.kmer = T->kmer; J.bins = T->bins; J.kmer_count = T->kc; J.n_isize = T->n_isize; J.n_indel_len = T->n_indel_len;
  for (int m = 0; m < 8; m++) J.kmer_off[m] = T->koff[m];
  J.count_gc = T->count_gc; J.wes = T->wes; J.window = T->window; J.max_reads = T->max_reads;
  J.tgt_left = T->tgt.as<int64_t>(); J.tgt_right = J.tgt_left + T->n_tgt; J.tgt_pmax = J.tgt_left + 2 * T->n_tgt;
  const int64_t* k64 = T->known.as<int64_t>();
  const int32_t* k32 = (const int32_t*)(T->known.as<uint8_t>() + (2 * T->n_ins + 2 * T->n_del) * 8);
  J.known_ins = sg::TrainKnown{k64, k64 + T->n_ins, k32, (const uint32_t*)(k32 + T->n_ins)};
  J.known_del = sg::TrainKnown{k64 + 2 * T->n_ins, k64 + 2 * T->n_ins + T->n_del, k32 + 2 * T->n_ins, (const uint32_t*)(k32 + 2 * T->n_ins + T->n_del)};
  unsigned long long* c0 = T->counts.as<unsigned long long>();
  J.subs1 = c0; J.subs2 = c0 + T->subs_n; J.kmers = c0 + 2 * T->subs_n; J.quality = J.kmers + T->kmers_n; J.isize = J.quality + T->qual_n;
  J.ins_len = J.isize + T->n_isize; J.del_len = J.ins_len + T->n_indel_len; J.scalars = J.del_len + T->n_indel_len;
  J.flags = T->flags.as<uint32_t>();
  J.carry_in = T->carry.as<sg::TrainCarry>() + T->cur;
  J.carry_out = T->carry.as<sg::TrainCarry>() + (T->cur ^ 1);
}

// What the chunk whose kernels are queued left behind: the malformed-line flag, the cap, the windows opened so far.
int train_settle(sg_ctx* ctx, sg_train_session* T) {
  if (!T->pending) return SG_OK;
  SG_HIP(hipStreamSynchronize(ctx->stream));
  T->pending = false;
  if (*T->mail_flags() & 1u) return ctx->fail(SG_ERR_INVALID, "Error: malformed read , there should be 11 mandatory fields");   // Profile.cpp:246-251
  if (T->mail->cut_line != ~0ull) { T->capped = true; T->lines += T->mail->cut_line + 1; }
  else T->lines += T->pending_lines;
  if (T->count_gc) T->n_windows = T->mail->n_windows;
  return SG_OK;
}

// The kernels of one chunk of whole lines that lies in T->text[T->fed & 1] (the chunk before settled).
int train_run_chunk(sg_ctx* ctx, sg_train_session* T, uint64_t bytes) {
  hipStream_t s = ctx->stream;
  DevBuf& text = T->text[T->fed & 1];
  int rc = SG_OK;
  SG_ENSURE(T->scan_work, sg::train_scan_work_bytes(bytes / 64 + 1));
  sg::TrainJob J;
  train_job(ctx, T, J);
  J.text = text.as<char>();
  J.bytes = bytes;
  J.scan_work = T->scan_work.p;
  sg::launch_train_lines_count(J, s);
  SG_HIP(hipGetLastError());
  SG_HIP(hipMemcpyAsync(T->mail, J.carry_out, sizeof(sg::TrainCarry), hipMemcpyDeviceToHost, s));
  SG_HIP(hipStreamSynchronize(s));
  const uint64_t n_lines = T->mail->n_lines;
  if (!n_lines) return SG_OK;
  SG_ENSURE(T->line_end, n_lines * 8 + 64);
  SG_ENSURE(T->reads, n_lines * sizeof(sg::TrainRead) + 64);
  if (T->count_gc) {
    SG_ENSURE(T->gate, n_lines * sizeof(sg::TrainGate) + 64);
    SG_ENSURE(T->steps, n_lines * sizeof(sg::TrainStep) + 64);
    const uint64_t want = T->n_windows + n_lines + 1;
    if (want > T->windows_cap) {
      const uint64_t cap = want + want / 2;
      if ((rc = sg_grow_keep(ctx, T->windows, T->n_windows * sizeof(sg::TrainWindow), cap * sizeof(sg::TrainWindow))) != SG_OK) return rc;
      if ((rc = sg_grow_keep(ctx, T->window_rc, T->n_windows * 4, cap * 4)) != SG_OK) return rc;
      SG_HIP(hipMemsetAsync(T->window_rc.as<uint32_t>() + T->n_windows, 0, (cap - T->n_windows) * 4, s));
      T->windows_cap = cap;
    }
  }
  SG_ENSURE(T->scan_work, sg::train_scan_work_bytes(std::max<uint64_t>(bytes / 64 + 1, n_lines)));
  if (T->scan_work.p != J.scan_work) {   // (the tile prefixes of the line scan sit in the old block: count again)
    J.scan_work = T->scan_work.p;
    sg::launch_train_lines_count(J, s);
  }
  J.line_end = T->line_end.as<uint64_t>();
  J.n_lines = n_lines;
  J.reads = T->reads.as<sg::TrainRead>();
  J.gate = T->gate.as<sg::TrainGate>();
  J.steps = T->steps.as<sg::TrainStep>();
  J.windows = T->windows.as<sg::TrainWindow>();
  J.window_rc = T->window_rc.as<uint32_t>();
  sg::launch_train_lines_fill(J, s);
  sg::launch_train_chunk(J, s);
  SG_HIP(hipGetLastError());
  SG_HIP(hipMemcpyAsync(T->mail, J.carry_out, sizeof(sg::TrainCarry), hipMemcpyDeviceToHost, s));
  SG_HIP(hipMemcpyAsync(T->mail_flags(), T->flags.p, 4, hipMemcpyDeviceToHost, s));
  T->pending = true;
  T->pending_lines = n_lines;
  T->cur ^= 1;
  T->fed++;
  return SG_OK;
}
}  // namespace

// One chunk of lines. The copy to the device runs on its own stream into the text buffer the previous chunk is not using, so it
// overlaps that chunk's kernels; the call returns with its own kernels queued (sg_train_capped / the malformed-line error of
// chunk k are known when chunk k + 1 is fed or sg_train_finish runs).
int sg_train_feed(sg_ctx* ctx, const char* sam_text, uint64_t sam_bytes) {
  if (!ctx || (sam_bytes && !sam_text)) return SG_ERR_INVALID;
  sg_train_session* T = ctx->train;
  if (!T) return ctx->fail(SG_ERR_INVALID, "sg_train_feed: call sg_train_begin first");
  if (!sam_bytes || T->capped) return SG_OK;   // (behind the cap: Profile::train has left its loop, Profile.cpp:1461-1464)
  SG_HIP(hipSetDevice(ctx->device));
  // A last line without a line break loses its last character, as Profile::train's `buf[strlen(buf)-1] = '\0'` chops it
  // (Profile.cpp:1459): in the device copy that character becomes the line break.
  const bool open_end = sam_text[sam_bytes - 1] != '\n';
  const uint64_t bytes = sam_bytes;
  DevBuf& text = T->text[T->fed & 1];
  SG_ENSURE(text, bytes + 64);
  SG_HIP(hipMemcpyAsync(text.p, sam_text, sam_bytes, hipMemcpyHostToDevice, T->copy_stream));
  if (open_end) SG_HIP(hipMemsetAsync(text.as<char>() + sam_bytes - 1, '\n', 1, T->copy_stream));
  int rc = train_settle(ctx, T);
  SG_HIP(hipStreamSynchronize(T->copy_stream));   // the caller's buffer is free again when this returns
  if (rc != SG_OK) return rc;
  if (T->capped) return SG_OK;
  return train_run_chunk(ctx, T, bytes);
}

// 1 once the cap on counted reads was reached. A chunk's verdict is known when the next one is fed (or at sg_train_finish):
// a caller that stops feeding on it has handed over at most one chunk the reference would not have read, which is dropped.
int sg_train_capped(sg_ctx* ctx) { return ctx && ctx->train && ctx->train->capped ? 1 : 0; }

int sg_train_finish(sg_ctx* ctx, sg_train_counts* out, double* gc, double* rc, uint64_t gc_cap, uint64_t* n_gc) {
  if (!ctx || !out) return SG_ERR_INVALID;
  sg_train_session* T = ctx->train;
  if (!T) return ctx->fail(SG_ERR_INVALID, "sg_train_finish: call sg_train_begin first");
  SG_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  {
    const int settled = train_settle(ctx, T);
    if (settled != SG_OK) return settled;
  }
  // ---- the windows countGC pushed (Profile.cpp:559-570, 623-634): every window but the last one it was in, if its GC
  // content is above zero and it counted a read; in the order they were opened ----
  std::vector<double> h_gc, h_rc;
  std::vector<uint32_t> h_raw;
  const uint64_t nw = T->n_windows;
  if (nw) {
    SG_ENSURE(T->gc_out, nw * 16 + 64);
    sg::TrainJob J;
    train_job(ctx, T, J);
    double* d_gc = T->gc_out.as<double>();
    sg::launch_train_window_gc(T->windows.as<sg::TrainWindow>(), T->window_rc.as<uint32_t>(), nw, J.contigs, J.ref_codes, T->wes, d_gc, d_gc + nw, s);
    SG_HIP(hipGetLastError());
    h_gc.resize(nw); h_rc.resize(nw); h_raw.resize(nw);
    SG_HIP(hipMemcpyAsync(h_gc.data(), d_gc, nw * 8, hipMemcpyDeviceToHost, s));
    SG_HIP(hipMemcpyAsync(h_rc.data(), d_gc + nw, nw * 8, hipMemcpyDeviceToHost, s));
    SG_HIP(hipMemcpyAsync(h_raw.data(), T->window_rc.p, nw * 4, hipMemcpyDeviceToHost, s));
  }
  std::vector<uint64_t> host(T->counters);
  SG_HIP(hipMemcpyAsync(host.data(), T->counts.p, T->counters * 8, hipMemcpyDeviceToHost, s));
  SG_HIP(hipStreamSynchronize(s));
  uint64_t pushed = 0;
  for (uint64_t w = 0; w + 1 < nw; w++)
    if (h_gc[w] > 0 && h_raw[w] > 0) {
      if (pushed < gc_cap && gc && rc) { gc[pushed] = h_gc[w]; rc[pushed] = h_rc[w]; }
      pushed++;
    }
  if (n_gc) *n_gc = pushed;
  if (gc && rc && pushed > gc_cap) return ctx->fail(SG_ERR_OVERFLOW, "sg_train_finish: more (GC, read count) pairs than gc_cap");
  const uint64_t* h = host.data();
  if (out->subs1) memcpy(out->subs1, h, T->subs_n * 8);
  if (out->subs2) memcpy(out->subs2, h + T->subs_n, T->subs_n * 8);
  if (out->kmers) memcpy(out->kmers, h + 2 * T->subs_n, T->kmers_n * 8);
  if (out->quality) memcpy(out->quality, h + 2 * T->subs_n + T->kmers_n, T->qual_n * 8);
  const uint64_t* is = h + 2 * T->subs_n + T->kmers_n + T->qual_n;
  if (out->isize) memcpy(out->isize, is, (size_t)T->n_isize * 8);
  if (out->ins_len) memcpy(out->ins_len, is + T->n_isize, (size_t)T->n_indel_len * 8);
  if (out->del_len) memcpy(out->del_len, is + T->n_isize + T->n_indel_len, (size_t)T->n_indel_len * 8);
  const uint64_t* sc = is + T->n_isize + 2 * (size_t)T->n_indel_len;
  out->lines = T->lines - sc[sg::kTrainEmptyLines];   // (empty lines are no reads: Profile.cpp:229-231)
  out->reads_counted = sc[sg::kTrainReads];
  out->cigar_chars = sc[sg::kTrainCigarChars];
  out->insert_events = sc[sg::kTrainInsEvents];
  out->delete_events = sc[sg::kTrainDelEvents];
  out->isize_overflow = sc[sg::kTrainIsizeOverflow];
  out->indel_len_overflow = sc[sg::kTrainIndelLenOverflow];
  out->skipped_overhang = sc[sg::kTrainOverhang];
  out->gc_rejected = sc[sg::kTrainGcRejected];
  out->gc_windows = nw;
  out->capped = T->capped ? 1 : 0;
  sg_train_end(ctx);
  return SG_OK;
}

int sg_train_count(sg_ctx* ctx, const char* sam_text, uint64_t sam_bytes, const char* const* contig_keys, uint32_t n_contigs,
                   const char* bases, int32_t kmer, int32_t bins, uint32_t n_isize, uint32_t n_indel_len, sg_train_counts* out) {
  if (!ctx || !out) return SG_ERR_INVALID;
  sg_train_setup st;
  memset(&st, 0, sizeof st);
  st.contig_keys = contig_keys; st.n_contigs = n_contigs; st.bases = bases; st.kmer = kmer; st.bins = bins;
  st.n_isize = n_isize; st.n_indel_len = n_indel_len; st.count_gc = 0; st.window = 1000;
  int rc = sg_train_begin(ctx, &st);
  if (rc == SG_OK) rc = sg_train_feed(ctx, sam_text, sam_bytes);
  if (rc == SG_OK) rc = sg_train_finish(ctx, out, nullptr, nullptr, 0, nullptr);
  if (rc != SG_OK) sg_train_end(ctx);
  return rc;
}

int sg_train_bam_start(sg_ctx* ctx, const char* const* ref_names, uint32_t n_ref, uint64_t first_record_skip) {
  if (!ctx || (n_ref && !ref_names)) return SG_ERR_INVALID;
  sg_train_session* T = ctx->train;
  if (!T) return ctx->fail(SG_ERR_INVALID, "sg_train_bam_start: call sg_train_begin first");
  if (T->fed || T->bam) return ctx->fail(SG_ERR_INVALID, "sg_train_bam_start: call it once, before anything is fed");
  SG_HIP(hipSetDevice(ctx->device));
  if (int rc = bam_stream_start(ctx, T->in, ref_names, n_ref, first_record_skip)) return rc;
  T->bam = true;
  return SG_OK;
}

int sg_train_feed_bgzf(sg_ctx* ctx, const void* members, uint64_t bytes) {
  if (!ctx || (bytes && !members)) return SG_ERR_INVALID;
  sg_train_session* T = ctx->train;
  if (!T || !T->bam) return ctx->fail(SG_ERR_INVALID, "sg_train_feed_bgzf: call sg_train_begin and sg_train_bam_start first");
  if (T->capped) return SG_OK;
  SG_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const auto t0 = std::chrono::steady_clock::now();
  if (!bytes) {   // the end of the stream: nothing may be left of a record
    const int rc = train_settle(ctx, T);
    if (rc != SG_OK || T->capped) return rc;
    return bam_stream_close(ctx, T->in, "sg_train_feed_bgzf");
  }
  // stage the members while the chunk before is still counted
  int rc = bam_stream_stage(ctx, T->in, "sg_train_feed_bgzf", members, bytes, T->copy_stream);
  if (rc != SG_OK) return rc;
  rc = train_settle(ctx, T);
  SG_HIP(hipStreamSynchronize(T->copy_stream));   // the caller's buffer is free again when this returns
  if (rc != SG_OK) return rc;
  if (T->capped) return SG_OK;
  sg::BamJob J;
  if ((rc = bam_stream_records(ctx, T->in, "sg_train_feed_bgzf", s, T->copy_stream, &J)) != SG_OK) return rc;
  const uint64_t n_rec = J.n_rec;
  uint64_t text_bytes = 0;
  if (n_rec) {
    SG_ENSURE(T->line_len, n_rec * 4 + 64);
    SG_ENSURE(T->line_off, n_rec * 8 + 64);
    J.line_len = T->line_len.as<uint32_t>();
    J.line_off = T->line_off.as<uint64_t>();
    sg::launch_bam_measure(J, s);
    sg::launch_scan_u32(J.line_len, (uint32_t)n_rec, J.scan_bsum, J.line_off, J.totals + 1, s);
    uint64_t h_tot[4];
    if ((rc = bam_stream_totals(ctx, T->in, "sg_train_feed_bgzf", J, h_tot)) != SG_OK) return rc;
    text_bytes = h_tot[1];
  }
  if (text_bytes) {
    DevBuf& text = T->text[T->fed & 1];
    SG_ENSURE(text, text_bytes + 64);
    J.text = text.as<char>();
    sg::launch_bam_render(J, s);
    SG_HIP(hipGetLastError());
  }
  if ((rc = bam_stream_advance(ctx, T->in, s)) != SG_OK) return rc;
  if (text_bytes) {
    SG_HIP(hipStreamSynchronize(s));
    T->bam_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return train_run_chunk(ctx, T, text_bytes);
  }
  T->bam_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return SG_OK;
}

int sg_train_bam_info(sg_ctx* ctx, uint64_t* records, uint64_t* inflated_bytes, double* seconds) {
  if (!ctx) return SG_ERR_INVALID;
  sg_train_session* T = ctx->train;
  if (!T || !T->bam) return ctx->fail(SG_ERR_INVALID, "sg_train_bam_info: no BAM input in this session");
  if (records) *records = T->in.records;
  if (inflated_bytes) *inflated_bytes = T->in.inflated;
  if (seconds) *seconds = T->bam_seconds;
  return SG_OK;
}

}  // extern "C"
