// sg_api.cpp -- C ABI (include/simuscop_amd.h) on top of the gfx950 kernels: the context, the profile's upload, the
// plan, the sampling pass and its results, detached outputs.  The other subjects have files of their own (sg_api.h
// lists them).
//
// Everything here is host plumbing: grow-only device buffers (sized for a 288 GB HBM3E part: a whole chromosome's
// haplotypes, plan and FASTQ text stay resident), kernel sequencing on one HIP stream.  There is no CPU fallback:
// without a HIP device sg_create fails.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "sg_api.h"
#include "sg_profile_tables.h"

thread_local std::string g_create_error;

struct sg_outputs {
  int device = 0;
  hipStream_t stream = nullptr;
  OutputSet bufs;
  uint64_t text_bytes[2] = {0, 0}, gz_bytes[2] = {0, 0};
  std::string err;
  ~sg_outputs() {
    if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
  }
};

sg_ctx::~sg_ctx() {
  (void)hipSetDevice(device);
  if (stream) (void)hipStreamSynchronize(stream);
  for (sg_outputs* o : spare) delete o;
  if (evs_created)
    for (auto& ev : evs) (void)hipEventDestroy(ev);
  if (own_stream) { (void)hipStreamSynchronize(own_stream); (void)hipStreamDestroy(own_stream); }
  if (mail) (void)hipHostFree(mail);
}

int finish_plan(sg_ctx* ctx, uint64_t nw, uint32_t n_segs, uint32_t n_slots, uint32_t batch_id, uint32_t first_window,
                       uint32_t first_slot, int32_t paired, const char* name_prefix) {
  const size_t plen = name_prefix ? strlen(name_prefix) : 0;
  const uint32_t nm = paired ? 2 : 1;
  SG_ENSURE(ctx->prefix, plen + 16);
  SG_ENSURE(ctx->pairs, ((size_t)n_slots + 1) * sizeof(sg::PairRec));
  SG_ENSURE(ctx->win_namebase, (nw + 1) * 4);
  SG_ENSURE(ctx->win_slot, (nw + 1) * 4);
  SG_ENSURE(ctx->win_flag, (nw + 1) * 4);
  SG_ENSURE(ctx->win_rows, (nw + 1) * sizeof(sg::WinRow));
  SG_ENSURE(ctx->blk_win, ((size_t)(n_slots + 255) / 256 + 1) * 4);
  SG_ENSURE(ctx->seg_flags, ((size_t)n_segs + 1) * 2 * 4);   // seg_flag, seg_lost
  SG_ENSURE(ctx->events, ((size_t)nm * n_slots + 1) * 4 * SG_MAX_EVENTS);
  SG_ENSURE(ctx->recoff, ((size_t)nm * n_slots + 1) * 4);
  SG_ENSURE(ctx->meta, ((size_t)nm * n_slots + 1) * 48);
  SG_ENSURE(ctx->totals, sg::kTotalsBytes);
  SG_ENSURE(ctx->bsum, ((size_t)nm * ((n_slots + 255) / 256) + 1) * 8);
  SG_HIP(hipMemcpyAsync(ctx->prefix.p, name_prefix, plen, hipMemcpyHostToDevice, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));

  sg::DevBatch& B = ctx->B;
  B.windows = ctx->windows.as<sg_window>();
  B.n_windows = nw;
  B.seg_size = ctx->segmeta.as<uint32_t>();
  B.seg_first_window = ctx->segmeta.as<uint32_t>() + n_segs;
  B.n_segs = n_segs;
  B.n_slots = n_slots;
  B.batch_id = batch_id;
  B.win_offset = first_window;
  B.slot_offset = first_slot;
  B.paired = paired ? 1 : 0;
  B.prefix = ctx->prefix.as<uint8_t>();
  B.prefix_len = (uint32_t)plen;
  for (int i = 0; i < 4; i++) B.prefix_w[i] = 0;
  for (size_t i = 0; i < plen && i < 16; i++) B.prefix_w[i / 4] |= (uint32_t)(uint8_t)name_prefix[i] << (8 * (i % 4));
  B.pairs = ctx->pairs.as<sg::PairRec>();
  B.win_namebase = ctx->win_namebase.as<uint32_t>();
  B.win_slot = ctx->win_slot.as<uint32_t>();
  B.win_flag = ctx->win_flag.as<uint32_t>();
  B.win_rows = ctx->win_rows.as<sg::WinRow>();
  B.blk_win = ctx->blk_win.as<uint32_t>();
  B.seg_flag = ctx->seg_flags.as<uint32_t>();
  B.seg_lost = B.seg_flag + n_segs + 1;
  B.events = ctx->events.as<uint32_t>();
  B.recloc = ctx->recoff.as<uint32_t>();
  B.blkbase = ctx->bsum.as<uint64_t>();
  B.seg_shift = sg::record_seg_shift((uint32_t)n_slots);
  B.meta = ctx->meta.as<uint4>();
  B.totals = ctx->totals.as<uint64_t>();
  B.slowq_count = (uint32_t*)(B.totals + 4);
  // the batch's own tables (slot -> window, edge windows, flagged segments), from the windows now on the device and the
  // loaded profile: made once here, read by every pass over the batch
  SG_HIP(hipMemsetAsync(B.seg_flag, 0, ((size_t)n_segs + 1) * 2 * 4, ctx->stream));
  sg::launch_batch_map(ctx->P, B, ctx->stream);
  SG_HIP(hipGetLastError());
  ctx->pass = sg_ctx::Pass(sg_ctx::Pass::Planned);
  return SG_OK;
}

void retire_plan(sg_ctx* ctx) {
  if (ctx->pass.stage <= sg_ctx::Pass::Planned) ctx->pass = sg_ctx::Pass();
  else ctx->pass.rows_current = false;
}

// The pass is over (its outputs were detached, or it failed): back to its plan, if that is still good.
static void restart_pass(sg_ctx* ctx) {
  ctx->pass = sg_ctx::Pass(ctx->pass.rows_current ? sg_ctx::Pass::Planned : sg_ctx::Pass::None);
}

// header + emit kernels of the current batch into the context's output buffers
static int launch_text(sg_ctx* ctx, bool prof) {
  sg::DevBatch& B = ctx->B;
  hipStream_t s = ctx->stream;
  for (int m = 0; m < 2; m++) {
    B.out[m] = ctx->out.text[m].as<uint8_t>();
    B.out_cap[m] = ctx->out.text[m].cap;
  }
  // Queue of the items the fast emit kernel leaves to the generic code (windows with a non-ACGT base,
  // reads with >= 2 sequencing indels): room for every item of ~10 % of the reads.  A batch that
  // needs more is emitted again by the generic kernel (settle_pass), so the size is not a correctness
  // matter.  SG_SLOWQ_CAP overrides it (tests force the overflow path with it).
  B.slowq = nullptr;
  B.slowq_cap = 0;
  if (sg::emit_uses_fast_kernel(ctx->P, B)) {
    uint64_t cap = std::max<uint64_t>(1u << 16, 2ull * B.n_slots);
    if (const char* e = getenv("SG_SLOWQ_CAP")) cap = std::max<uint64_t>(1, strtoull(e, nullptr, 10));
    cap = std::min<uint64_t>(cap, 1ull << 30);
    SG_ENSURE(ctx->slowq, cap * 8 * (B.paired ? 2 : 1));
    B.slowq = ctx->slowq.as<uint2>();
    B.slowq_cap = (uint32_t)cap;
  }
  if (prof) SG_HIP(hipEventRecord(ctx->evs[sg_ctx::EV_TEXT_BEGIN], s));  // after the (first-pass) output allocation
  sg::launch_header(ctx->P, B, s);
  ctx->pass.emit_path = sg::emit_path(ctx->P, B, false);
  sg::launch_emit(ctx->P, B, s, false, prof ? ctx->evs[sg_ctx::EV_MAIN_EMIT_END] : nullptr);
  if (prof) SG_HIP(hipEventRecord(ctx->evs[sg_ctx::EV_TEXT_END], s));
  return SG_OK;
}

// the text buffers at least as large as the pass's totals say
static int grow_text(sg_ctx* ctx) {
  for (int m = 0; m < (ctx->B.paired ? 2 : 1); m++) SG_ENSURE(ctx->out.text[m], ctx->pass.host_totals[m] + 64);
  return SG_OK;
}

// totals[3] & 1: the pass is over
static int refuse_event_overflow(sg_ctx* ctx) {
  restart_pass(ctx);
  return ctx->fail(SG_ERR_OVERFLOW, "sg_sample: a read drew more than SG_MAX_EVENTS sequencing indels");
}

static int run_pass(sg_ctx* ctx) {
  sg_ctx::Pass& Q = ctx->pass = sg_ctx::Pass(sg_ctx::Pass::Planned);   // whatever the last pass left ends here
  sg::DevBatch& B = ctx->B;
  B.k0 = (uint32_t)ctx->seed;
  B.k1 = (uint32_t)(ctx->seed >> 32);
  // timing ablations (outputs are wrong when set): SG_DIAG selects the generic emit kernel, SG_FDIAG keeps the straight-line one
  { const char* dg = getenv("SG_DIAG"); B.diag = dg ? (uint32_t)atoi(dg) : 0u; }
  if (const char* fd = getenv("SG_FDIAG")) B.diag = (uint32_t)atoi(fd);
  hipStream_t s = ctx->stream;
  const bool prof = ctx->profiling;
  if (!B.n_windows) SG_HIP(hipMemsetAsync(B.totals, 0, sg::kTotalsBytes, s));  // (otherwise edge_kernel clears them)
  // (what the intervals between these events are called: settle_pass)
  if (prof) SG_HIP(hipEventRecord(ctx->evs[sg_ctx::EV_EDGE_BEGIN], s));
  sg::launch_edge(ctx->P, B, s);
  if (prof) SG_HIP(hipEventRecord(ctx->evs[sg_ctx::EV_EDGE_END], s));
  if (prof) SG_HIP(hipEventRecord(ctx->evs[sg_ctx::EV_FRAGMENT_BEGIN], s));
  sg::launch_fragment(ctx->P, B, s);
  if (prof) SG_HIP(hipEventRecord(ctx->evs[sg_ctx::EV_FRAGMENT_END], s));
  sg::launch_scan(B, s);
  if (prof) SG_HIP(hipEventRecord(ctx->evs[sg_ctx::EV_SCAN_END], s));
  SG_HIP(hipGetLastError());
  // a released output set (sg_release_outputs): its buffers become this pass's
  if (ctx->out.empty() && !ctx->spare.empty()) std::swap(ctx->out, ctx->spare.back()->bufs);
  // The FASTQ size is only known now, on the device.  When the context already holds output buffers (every pass
  // but a context's first), the emit kernels are launched at once: they compare the size with the buffers' capacity
  // themselves and do nothing but raise a flag when it does not fit (settle_pass then grows the buffers and launches
  // them again).  Otherwise two u64 are read back first -- one stream sync in the middle of the pass.
  Q.speculative = ctx->out.text[0].p != nullptr && (!B.paired || ctx->out.text[1].p != nullptr) && getenv("SG_NO_SPECULATION") == nullptr;
  if (!Q.speculative) {
    sg::launch_mail(B.totals, ctx->mail, s);
    SG_HIP(hipStreamSynchronize(s));
    memcpy(Q.host_totals, ctx->mail, 4 * 8);
    if (Q.host_totals[3] & 1) return refuse_event_overflow(ctx);
    if (int rc = grow_text(ctx)) return rc;
  }
  if (int rc = launch_text(ctx, prof)) return rc;
  sg::launch_mail(B.totals, ctx->mail, s);
  SG_HIP(hipGetLastError());
  Q.stage = sg_ctx::Pass::Queued;
  return SG_OK;
}

// Queued -> Settled.  What the queued pass left: sizes, flags; the emit kernels again if the text did not fit the buffers
// they were given; every item again through the generic kernel if the slow queue overflowed; the kernel times.
static int settle_pass(sg_ctx* ctx) {
  sg_ctx::Pass& Q = ctx->pass;
  sg::DevBatch& B = ctx->B;
  SG_HIP(hipStreamSynchronize(ctx->stream));
  memcpy(Q.host_totals, ctx->mail, 4 * 8);
  Q.host_flags[0] = ctx->mail[3];
  Q.host_flags[1] = ctx->mail[4];
  if (Q.host_totals[3] & 1) return refuse_event_overflow(ctx);
  if (Q.speculative && (Q.host_flags[0] & 4)) {  // the buffers were too small: grow, emit again
    if (int rc = grow_text(ctx)) return rc;
    // what the aborted launch left behind: the flags, the slow-queue counts (a mate whose text did fit has appended its
    // items already) and the read-group counters of both emit kernels (exhausted by that mate); the record offsets' segment
    // bases and the sizes stay
    SG_HIP(hipMemsetAsync(B.totals + 3, 0, 2 * 8, ctx->stream));
    SG_HIP(hipMemsetAsync((uint8_t*)B.totals + 128, 0, sg::kTotalsSegBase - 128, ctx->stream));
    if (int rc = launch_text(ctx, ctx->profiling)) return rc;   // (the kernel times are then those of the launch that counted)
    sg::launch_mail(B.totals, ctx->mail, ctx->stream);
    SG_HIP(hipStreamSynchronize(ctx->stream));
    Q.host_flags[0] = ctx->mail[3];
    Q.host_flags[1] = ctx->mail[4];
  }
  SG_HIP(hipStreamSynchronize(ctx->stream));
  Q.slow_items = (Q.host_flags[1] & 0xFFFFFFFFu) + (Q.host_flags[1] >> 32);
  Q.slow_overflow = (Q.host_flags[0] & 2) != 0;
  if (Q.slow_overflow) {  // headers are in place; every item again through the generic kernel
    sg::launch_emit(ctx->P, B, ctx->stream, true, nullptr);
    SG_HIP(hipGetLastError());
    SG_HIP(hipStreamSynchronize(ctx->stream));
  }
  if (ctx->profiling) {
    // the six intervals of SG_K_NAMES, by the names they got when each was a kernel of its own: "plan" is edge_kernel,
    // "namebase" is empty (the numbers are made in the other two), "indel" is fragment_kernel, "scan" is block_base_kernel
    const hipEvent_t* ev = ctx->evs;
    SG_HIP(hipEventElapsedTime(&ctx->last_ms[SG_K_PLAN], ev[sg_ctx::EV_EDGE_BEGIN], ev[sg_ctx::EV_EDGE_END]));
    SG_HIP(hipEventElapsedTime(&ctx->last_ms[SG_K_NAMEBASE], ev[sg_ctx::EV_EDGE_END], ev[sg_ctx::EV_FRAGMENT_BEGIN]));
    SG_HIP(hipEventElapsedTime(&ctx->last_ms[SG_K_INDEL], ev[sg_ctx::EV_FRAGMENT_BEGIN], ev[sg_ctx::EV_FRAGMENT_END]));
    SG_HIP(hipEventElapsedTime(&ctx->last_ms[SG_K_SCAN], ev[sg_ctx::EV_FRAGMENT_END], ev[sg_ctx::EV_SCAN_END]));
    SG_HIP(hipEventElapsedTime(&ctx->last_ms[SG_K_EMIT], ev[sg_ctx::EV_TEXT_BEGIN], ev[sg_ctx::EV_MAIN_EMIT_END]));
    SG_HIP(hipEventElapsedTime(&ctx->last_ms[SG_K_EMIT_SLOW], ev[sg_ctx::EV_MAIN_EMIT_END], ev[sg_ctx::EV_TEXT_END]));
  }
  Q.stage = sg_ctx::Pass::Settled;
  return SG_OK;
}

int sg_pass_need(sg_ctx* ctx, const char* who, sg_ctx::Pass::Stage at_least, bool settle_now) {
  using Pass = sg_ctx::Pass;
  if (!ctx) return SG_ERR_INVALID;
  static const char* const step[] = {"", "sg_plan", "sg_sample", "sg_result"};
  const Pass::Stage need = settle_now && at_least == Pass::Settled ? Pass::Queued : at_least;   // settling asks no more
  if (ctx->pass.stage < need || (at_least == Pass::Planned && !ctx->pass.rows_current))
    return ctx->fail(SG_ERR_INVALID, std::string(who) + ": call " + step[need] + " first");
  SG_HIP(hipSetDevice(ctx->device));
  return at_least == Pass::Settled && ctx->pass.stage == Pass::Queued ? settle_pass(ctx) : SG_OK;
}

extern "C" {

const char* sg_last_error(const sg_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int sg_create(sg_ctx** out, int device, uint64_t seed) {
  if (!out) { g_create_error = "sg_create: null output pointer"; return SG_ERR_INVALID; }
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    g_create_error = std::string("sg_create: no HIP device available (") + hipGetErrorString(e) +
                     "); this engine has no CPU path";
    return SG_ERR_HIP;
  }
  if (device < 0 || device >= ndev) { g_create_error = "sg_create: device index out of range"; return SG_ERR_INVALID; }
  e = hipSetDevice(device);
  if (e != hipSuccess) { g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e); return SG_ERR_HIP; }
  sg_ctx* ctx = new sg_ctx();
  ctx->device = device;
  ctx->seed = seed;
  e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking);
  if (e != hipSuccess) { g_create_error = std::string("hipStreamCreate: ") + hipGetErrorString(e); delete ctx; return SG_ERR_HIP; }
  ctx->stream = ctx->own_stream;
  e = hipHostMalloc((void**)&ctx->mail, 64, hipHostMallocDefault);
  if (e != hipSuccess) { g_create_error = std::string("hipHostMalloc: ") + hipGetErrorString(e); delete ctx; return SG_ERR_HIP; }
  *out = ctx;
  return SG_OK;
}

void sg_destroy(sg_ctx* ctx) {
  if (!ctx) return;
  sg_train_end(ctx);
  sg_eval_end(ctx);
  delete ctx;
}

int sg_set_stream(sg_ctx* ctx, void* hip_stream) {
  if (!ctx) return SG_ERR_INVALID;
  ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
  return SG_OK;
}

int sg_set_seed(sg_ctx* ctx, uint64_t seed) {
  if (!ctx) return SG_ERR_INVALID;
  ctx->seed = seed;
  return SG_OK;
}

int sg_set_strict_bases(sg_ctx* ctx, int on) {
  if (!ctx) return SG_ERR_INVALID;
  ctx->B.strict_bases = on ? 1u : 0u;   // read by the generic item code of every later pass (template_code, sg_kernels.hip)
  return SG_OK;
}

int sg_set_profiling(sg_ctx* ctx, int enable) {
  if (!ctx) return SG_ERR_INVALID;
  SG_HIP(hipSetDevice(ctx->device));
  if (enable && !ctx->evs_created) {
    for (auto& ev : ctx->evs) SG_HIP(hipEventCreate(&ev));
    ctx->evs_created = true;
  }
  ctx->profiling = enable != 0;
  return SG_OK;
}

int sg_kernel_times(sg_ctx* ctx, float ms[SG_K_COUNT]) {
  if (!ctx || !ms) return SG_ERR_INVALID;
  for (int i = 0; i < SG_K_COUNT; i++) ms[i] = ctx->last_ms[i];
  return SG_OK;
}

int sg_sync(sg_ctx* ctx) {
  if (!ctx) return SG_ERR_INVALID;
  SG_HIP(hipSetDevice(ctx->device));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

// The profile's tables (sg_profile_prepare, sg_profile_tables.h) go to the device as they are; DevProfile points into them.
int sg_load_prepared_profile(sg_ctx* ctx, const sg_profile_tables* T) {
  if (!ctx || !T) return SG_ERR_INVALID;
  if (T->rc != SG_OK) return ctx->fail(T->rc, T->err);
  SG_HIP(hipSetDevice(ctx->device));
  SG_ENSURE(ctx->tab, T->tab.size() * 4);
  SG_HIP(hipMemcpyAsync(ctx->tab.p, T->tab.data(), T->tab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));

  const SgTableLayout& L = T->L;
  sg::DevProfile& P = ctx->P;
  const uint32_t* base = ctx->tab.as<uint32_t>();
  const bool fast = L.kmer == 3;
  P.sub = (const uint4*)(base + L.sub_off);
  P.sub_mate_rows = L.has2 ? (uint32_t)L.sub_rows : 0u;
  P.alias = (const uint2*)(base + L.alias_off);
  P.lgW = L.lgW;
  P.fast_lds = fast ? base + L.fast_lds_off : nullptr;
  P.fast_mate_words = L.has2 ? (uint32_t)L.bins * L.fast_stride : 0u;
  P.fast_stride = L.fast_stride;
  P.fast_sub = fast ? (const uint4*)(base + L.fast_sub_off) : nullptr;
  P.fast_alias = fast ? (const uint2*)(base + L.fast_alias_off) : nullptr;
  P.ins_row = base + L.ins_off; P.ins_lg = L.ins_lg;
  P.del_row = base + L.del_off; P.del_lg = L.del_lg;
  P.isz_row = L.has_isz ? base + L.isz_off : nullptr; P.isz_lg = L.isz_lg;
  P.inv_remap_packed = L.inv_remap;
  P.isz_min = L.isize_min;
  P.fixed_isz = L.insert_size;
  P.isz_lo = L.has_isz ? L.isize_min : L.insert_size;
  P.isz_hi = L.has_isz ? L.isize_min + L.n_isize - 1 : L.insert_size;
  P.evA = L.evA; P.evB = L.evB;
  P.gap_row = (const uint64_t*)(base + L.gap_off);
  P.L = L.read_length; P.bins = L.bins; P.kmer = L.kmer; P.min_qual = L.min_qual;
  P.remap_packed = L.remap; P.bases_packed = L.packed;
  for (int m = 0; m < 8; m++) P.kmer_off[m] = L.kmer_off[m];
  ctx->have_profile = true;
  retire_plan(ctx);
  if (sg::emit_variant(P) != 0) sg::preload_emit_fast();   // (not inside the first pass's timed launch)
  return SG_OK;
}

int sg_load_profile(sg_ctx* ctx, const sg_profile_cdf* pr) {
  if (!ctx || !pr) return SG_ERR_INVALID;
  sg_profile_tables* T = nullptr;
  sg_profile_prepare(pr, &T);
  const int rc = sg_load_prepared_profile(ctx, T);
  sg_profile_tables_free(T);
  return rc;
}

int sg_plan(sg_ctx* ctx, const sg_batch* b) {
  if (!ctx || !b) return SG_ERR_INVALID;
  if (!ctx->have_profile) return ctx->fail(SG_ERR_INVALID, "sg_plan: call sg_load_profile first");
  if (!ctx->have_haps) return ctx->fail(SG_ERR_INVALID, "sg_plan: call sg_upload_haplotypes first");
  if (b->n_windows && (!b->windows || !b->seg_size || !b->seg_first_window)) return ctx->fail(SG_ERR_INVALID, "sg_plan: null arrays");
  if (b->n_windows > 0xFFFFFFFFull) return ctx->fail(SG_ERR_INVALID, "sg_plan: more than 2^32 windows in one batch");
  if (b->batch_id > 0xFFFF) return ctx->fail(SG_ERR_INVALID, "sg_plan: batch_id must fit 16 bits");
  SG_HIP(hipSetDevice(ctx->device));
  // validate the plan on the host: every operand shape the kernels assume
  uint64_t slots = 0;
  const uint64_t nw = b->n_windows;
  for (uint64_t w = 0; w < nw; w++) {
    const sg_window& x = b->windows[w];
    if (x.seg >= b->n_segs) return ctx->fail(SG_ERR_INVALID, "sg_plan: window.seg out of range");
    if (x.slot_base != slots) return ctx->fail(SG_ERR_INVALID, "sg_plan: window.slot_base is not the running prefix sum");
    if (x.len == 0) return ctx->fail(SG_ERR_INVALID, "sg_plan: empty window");
    if (b->seg_size[x.seg] == 0) return ctx->fail(SG_ERR_INVALID, "sg_plan: seg_size 0");
    uint64_t planned = x.n_reads <= 0 ? 0 : (b->paired ? ((uint64_t)x.n_reads + 1) / 2 : (uint64_t)x.n_reads);
    slots += planned;
    if (slots > 0xFFFFFFF0ull) return ctx->fail(SG_ERR_INVALID, "sg_plan: more than 2^32 fragments in one batch");
  }
  for (uint32_t s = 0; s < b->n_segs; s++)
    if (b->seg_first_window[s] > b->seg_first_window[s + 1] || b->seg_first_window[s + 1] > nw)
      return ctx->fail(SG_ERR_INVALID, "sg_plan: seg_first_window not monotone");
  if (b->n_segs && (b->seg_first_window[0] != 0 || b->seg_first_window[b->n_segs] != nw))
    return ctx->fail(SG_ERR_INVALID, "sg_plan: seg_first_window must cover all windows");
  const size_t plen = b->name_prefix ? strlen(b->name_prefix) : 0;
  if (plen == 0 || plen > 990) return ctx->fail(SG_ERR_INVALID, "sg_plan: bad name_prefix (1..990 bytes)");  // header length is a 10-bit field
  for (uint64_t w = 0; w < nw; w++) {
    const sg_window& x = b->windows[w];
    if (x.chain >= ctx->hap.len.size()) return ctx->fail(SG_ERR_INVALID, "sg_plan: window.chain out of range");
    if (x.hap_base + x.spos + x.len > ctx->hap.len[x.chain]) return ctx->fail(SG_ERR_INVALID, "sg_plan: window runs past its chain");
  }
  SG_ENSURE(ctx->windows, (nw + 1) * sizeof(sg_window));
  SG_ENSURE(ctx->segmeta, ((size_t)b->n_segs * 2 + 2) * 4);
  if (nw) SG_HIP(hipMemcpyAsync(ctx->windows.p, b->windows, nw * sizeof(sg_window), hipMemcpyHostToDevice, ctx->stream));
  if (b->n_segs) {
    SG_HIP(hipMemcpyAsync(ctx->segmeta.p, b->seg_size, (size_t)b->n_segs * 4, hipMemcpyHostToDevice, ctx->stream));
    SG_HIP(hipMemcpyAsync(ctx->segmeta.as<uint32_t>() + b->n_segs, b->seg_first_window, ((size_t)b->n_segs + 1) * 4,
                          hipMemcpyHostToDevice, ctx->stream));
  }
  return finish_plan(ctx, nw, b->n_segs, (uint32_t)slots, b->batch_id, b->first_window, b->first_slot, b->paired, b->name_prefix);
}

int sg_sample(sg_ctx* ctx) {
  if (int rc = sg_pass_need(ctx, "sg_sample", sg_ctx::Pass::Planned)) return rc;
  return run_pass(ctx);
}

int sg_emit_variant(sg_ctx* ctx) {
  if (!ctx || !ctx->have_profile) return -1;
  return sg::emit_variant(ctx->P);
}

int sg_emit_path(const sg_ctx* ctx, sg_emit_path_info* info) {
  // (a const context: no message to leave, no device to select, so the stage is tested here and not by sg_pass_need)
  if (!ctx || !info || ctx->pass.stage != sg_ctx::Pass::Settled) return SG_ERR_INVALID;
  const sg::EmitPath& path = ctx->pass.emit_path;
  *info = sg_emit_path_info{path.main_kernel, path.slow_rows_lds, path.lds_bytes, path.clean_cap};
  return SG_OK;
}

int sg_emit_info(sg_ctx* ctx, uint64_t* queued_items, int* requeued) {
  if (int rc = sg_pass_need(ctx, "sg_emit_info", sg_ctx::Pass::Settled)) return rc;
  if (queued_items) *queued_items = ctx->pass.slow_items;
  if (requeued) *requeued = ctx->pass.slow_overflow ? 1 : 0;
  return SG_OK;
}

int sg_result(sg_ctx* ctx, uint64_t* bytes_r1, uint64_t* bytes_r2, uint64_t* n_fragments) {
  if (int rc = sg_pass_need(ctx, "sg_result", sg_ctx::Pass::Settled, true)) return rc;
  const uint64_t* totals = ctx->pass.host_totals;
  if (bytes_r1) *bytes_r1 = totals[0];
  if (bytes_r2) *bytes_r2 = ctx->B.paired ? totals[1] : 0;
  if (n_fragments) *n_fragments = totals[2];
  return SG_OK;
}

int sg_fetch(sg_ctx* ctx, char* host_r1, char* host_r2) {
  if (int rc = sg_pass_need(ctx, "sg_fetch", sg_ctx::Pass::Settled, true)) return rc;
  char* const dst[2] = {host_r1, ctx->B.paired ? host_r2 : nullptr};
  for (int m = 0; m < 2; m++)
    if (dst[m]) SG_HIP(sg_fetch_bytes(ctx->device, ctx->stream, dst[m], ctx->out.text[m].p, ctx->pass.host_totals[m]));
  return SG_OK;
}

int sg_fetch_range(sg_ctx* ctx, int mate, uint64_t offset, uint64_t bytes, char* host_dst) {
  if (!ctx || (bytes && !host_dst) || mate < 0 || mate > 1) return SG_ERR_INVALID;
  if (int rc = sg_pass_need(ctx, "sg_fetch_range", sg_ctx::Pass::Settled, true)) return rc;
  if (mate == 1 && !ctx->B.paired) return ctx->fail(SG_ERR_INVALID, "sg_fetch_range: single-end batch has no mate 2");
  if (!sg_range_within(offset, bytes, ctx->pass.host_totals[mate])) return ctx->fail(SG_ERR_INVALID, "sg_fetch_range: range past the end of the FASTQ text");
  SG_HIP(sg_fetch_bytes(ctx->device, ctx->stream, host_dst, ctx->out.text[mate].as<char>() + offset, bytes));
  return SG_OK;
}

int sg_device_output(sg_ctx* ctx, void** dev_r1, void** dev_r2) {
  // (settled here: a pass queued without its size may still move to larger buffers)
  if (int rc = sg_pass_need(ctx, "sg_device_output", sg_ctx::Pass::Settled, true)) return rc;
  if (dev_r1) *dev_r1 = ctx->out.text[0].p;
  if (dev_r2) *dev_r2 = ctx->B.paired ? ctx->out.text[1].p : nullptr;
  return SG_OK;
}

// ---- detached outputs ----
int sg_detach_outputs(sg_ctx* ctx, sg_outputs** out) {
  if (!out) return SG_ERR_INVALID;
  if (int rc = sg_pass_need(ctx, "sg_detach_outputs", sg_ctx::Pass::Settled)) return rc;
  sg_outputs* o = nullptr;
  if (!ctx->spare.empty()) { o = ctx->spare.back(); ctx->spare.pop_back(); }
  if (!o) {
    o = new sg_outputs();
    o->device = ctx->device;
    hipError_t e = hipStreamCreateWithFlags(&o->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete o; return ctx->hipfail(e, "hipStreamCreate(outputs)"); }
  }
  // whatever the spare still holds goes back to the context (it is empty or smaller than what was just used)
  std::swap(ctx->out, o->bufs);
  const sg_ctx::Pass& Q = ctx->pass;
  o->text_bytes[0] = Q.host_totals[0];
  o->text_bytes[1] = ctx->B.paired ? Q.host_totals[1] : 0;
  o->gz_bytes[0] = Q.gz_bytes[0];   // (0 without sg_compress)
  o->gz_bytes[1] = Q.gz_bytes[1];
  restart_pass(ctx);
  *out = o;
  return SG_OK;
}

int sg_outputs_sizes(const sg_outputs* o, uint64_t text_bytes[2], uint64_t gz_bytes[2]) {
  if (!o) return SG_ERR_INVALID;
  for (int m = 0; m < 2; m++) {
    if (text_bytes) text_bytes[m] = o->text_bytes[m];
    if (gz_bytes) gz_bytes[m] = o->gz_bytes[m];
  }
  return SG_OK;
}

const char* sg_outputs_last_error(const sg_outputs* o) { return o ? o->err.c_str() : ""; }

int sg_outputs_fetch(sg_outputs* o, int mate, int compressed, uint64_t offset, uint64_t bytes, void* host_dst) {
  if (!o || mate < 0 || mate > 1 || (bytes && !host_dst)) return SG_ERR_INVALID;
  if (!sg_range_within(offset, bytes, compressed ? o->gz_bytes[mate] : o->text_bytes[mate])) {
    o->err = "sg_outputs_fetch: range past the end of the data";
    return SG_ERR_INVALID;
  }
  if (!bytes) return SG_OK;
  const uint8_t* src = (compressed ? o->bufs.gz[mate] : o->bufs.text[mate]).as<uint8_t>() + offset;
  const hipError_t e = sg_fetch_bytes(o->device, o->stream, host_dst, src, bytes);
  if (e != hipSuccess) { o->err = std::string("sg_outputs_fetch: ") + hipGetErrorString(e); return SG_ERR_HIP; }
  return SG_OK;
}

int sg_release_outputs(sg_ctx* ctx, sg_outputs* o) {
  if (!ctx || !o) return SG_ERR_INVALID;
  SG_HIP(hipSetDevice(ctx->device));
  SG_HIP(hipStreamSynchronize(o->stream));
  o->text_bytes[0] = o->text_bytes[1] = o->gz_bytes[0] = o->gz_bytes[1] = 0;
  ctx->spare.push_back(o);
  return SG_OK;
}

}  // extern "C"
