// sg_api.cpp -- C ABI (include/simuscop_amd.h) on top of the gfx950 kernels; profile training and BAM input are in
// sg_api_train.cpp, the window planner in sg_api_windows.cpp.
//
// Everything here is host plumbing: table conversion, grow-only device buffers (sized for a
// 288 GB HBM3E part: a whole chromosome's haplotypes, plan and FASTQ text stay resident), kernel
// sequencing on one HIP stream.  There is no CPU fallback: without a HIP device sg_create fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "sg_api.h"
#include "sg_deflate.h"
#include "sg_scan.h"
#include "sg_tables.h"
#include "sg_truth.h"

namespace {

// Device blocks released by a context stay with the process and serve the next request of their size on the same
// device.  A whole-genome run allocates ~60 GB in a few dozen blocks and returns them at its end; the next run of the
// process asked the runtime for the same blocks again, and every dozen runs or so ONE such hipMalloc took 2-5 s
// (`SG_TRACE_ALLOC=1 python tools/c3_steps.py`: "hipMalloc 3455.3 MB: 4925.76 ms" in the thirteenth run, 20-40 ms in the
// others) -- seventeen times the run itself.  Best fit within 1.5x; the cache holds at most SG_BLOCK_CACHE_GB (default: a
// third of the device's memory) and gives everything back through sg_release_cached_memory().  SG_BLOCK_CACHE_GB=0 turns it off.
struct BlockCache {
  struct Block { void* p; size_t cap; int dev; };
  std::mutex mu;
  std::vector<Block> blocks;   // oldest first
  size_t held = 0;
  // Default: a third of the device's memory (MI355X: 96 GB -- a whole-genome run's ~60 GB of blocks fit; what other
  // allocators of the process and other processes on the device may need stays free), SG_BLOCK_CACHE_GB overrides.
  static size_t limit() {
    static const size_t v = [] {
      const char* e = getenv("SG_BLOCK_CACHE_GB");
      if (e) return (size_t)(atof(e) * 1073741824.0);
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || !total_b) return (size_t)(64.0 * 1073741824.0);
      return total_b / 3;
    }();
    return v;
  }
  void* take(size_t want, int dev, size_t* cap) {
    std::lock_guard<std::mutex> lk(mu);
    size_t best = blocks.size();
    for (size_t i = 0; i < blocks.size(); i++)
      if (blocks[i].dev == dev && blocks[i].cap >= want && blocks[i].cap <= want + want / 2 + (64u << 20) &&
          (best == blocks.size() || blocks[i].cap < blocks[best].cap))
        best = i;
    if (best == blocks.size()) return nullptr;
    void* p = blocks[best].p;
    *cap = blocks[best].cap;
    held -= blocks[best].cap;
    blocks.erase(blocks.begin() + (long)best);
    return p;
  }
  void give(void* p, size_t cap, int dev) {
    if (cap > limit()) { (void)hipFree(p); return; }
    // whoever gets the block next may write it at once: nothing of this process may still be using it (hipFree waits
    // likewise)
    int cur = dev;
    (void)hipGetDevice(&cur);
    if (cur != dev) (void)hipSetDevice(dev);
    (void)hipDeviceSynchronize();
    if (cur != dev) (void)hipSetDevice(cur);
    std::vector<Block> drop;
    {
      std::lock_guard<std::mutex> lk(mu);
      blocks.push_back({p, cap, dev});
      held += cap;
      while (held > limit() && !blocks.empty()) {
        drop.push_back(blocks.front());
        held -= blocks.front().cap;
        blocks.erase(blocks.begin());
      }
    }
    for (const Block& b : drop) (void)hipFree(b.p);
  }
  bool any() {
    std::lock_guard<std::mutex> lk(mu);
    return !blocks.empty();
  }
  void trim() {
    std::vector<Block> drop;
    {
      std::lock_guard<std::mutex> lk(mu);
      drop.swap(blocks);
      held = 0;
    }
    for (const Block& b : drop) (void)hipFree(b.p);
  }
};
BlockCache& block_cache() {
  static BlockCache* c = new BlockCache;  // (never destroyed: contexts may outlive static destructors)
  return *c;
}

// Pinned staging buffers are kept for the process like the device blocks (BlockCache above): pinning 64 MB takes ~5 ms, a
// run's two reference-staging buffers 10 ms of a 0.27 s whole-genome run.  Exact sizes only (the callers use a few fixed
// ones), at most 1 GB kept.
struct HostCache {
  struct Block { void* p; uint64_t bytes; };
  std::mutex mu;
  std::vector<Block> blocks;
  std::map<void*, uint64_t> live;   // what sg_host_alloc handed out: sizes for the way back
  uint64_t held = 0;
  void* take(uint64_t bytes) {
    std::lock_guard<std::mutex> lk(mu);
    for (size_t i = 0; i < blocks.size(); i++)
      if (blocks[i].bytes == bytes) {
        void* p = blocks[i].p;
        held -= bytes;
        blocks.erase(blocks.begin() + (long)i);
        live[p] = bytes;
        return p;
      }
    return nullptr;
  }
  void note(void* p, uint64_t bytes) {
    std::lock_guard<std::mutex> lk(mu);
    live[p] = bytes;
  }
  bool give(void* p) {   // false: not one of ours, or no room
    std::lock_guard<std::mutex> lk(mu);
    auto it = live.find(p);
    if (it == live.end()) return false;
    const uint64_t bytes = it->second;
    live.erase(it);
    if (BlockCache::limit() == 0 || held + bytes > (1ull << 30)) return false;
    blocks.push_back({p, bytes});
    held += bytes;
    return true;
  }
  void trim() {
    std::vector<Block> drop;
    {
      std::lock_guard<std::mutex> lk(mu);
      drop.swap(blocks);
      held = 0;
    }
    for (const Block& b : drop) (void)hipHostFree(b.p);
  }
};
HostCache& host_cache() {
  static HostCache* c = new HostCache;
  return *c;
}

}  // namespace

thread_local std::string g_create_error;

int DevBuf::ensure(size_t bytes) {
  if (bytes <= cap) return 0;
  release();
  size_t want = bytes + bytes / 8 + 256;
  static const bool trace = getenv("SG_TRACE_ALLOC") != nullptr;
  (void)hipGetDevice(&dev);
  if ((p = block_cache().take(want, dev, &cap)) != nullptr) return 0;
  const auto t0 = std::chrono::steady_clock::now();
  hipError_t e = hipMalloc(&p, want);
  if (e != hipSuccess) {
    (void)hipGetLastError();   // (reported by the return value: a later SG_HIP(hipGetLastError()) must not see it again)
    if (block_cache().any()) {  // the cache may be what is in the way
      block_cache().trim();
      if ((e = hipMalloc(&p, want)) != hipSuccess) (void)hipGetLastError();
    }
  }
  if (trace)
    fprintf(stderr, "[sg] hipMalloc %.1f MB: %.2f ms\n", want / 1048576.0,
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  if (e != hipSuccess) { p = nullptr; return (int)e; }
  cap = want;
  return 0;
}

void DevBuf::release() {
  if (p) block_cache().give(p, cap, dev);
  p = nullptr; cap = 0;
}

struct sg_outputs {
  int device = 0;
  hipStream_t stream = nullptr;
  DevBuf text[2], gz[2];
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

// Work buffers and DevBatch fields of a planned batch whose windows / segment arrays are already in ctx->windows /
// ctx->segmeta (put there by sg_plan from host arrays, or by sg_plan_range from the device-made table).
int finish_plan(sg_ctx* ctx, uint64_t nw, uint32_t n_segs, uint32_t n_slots, uint32_t batch_id, uint32_t first_window,
                       uint32_t first_slot, int32_t paired, const char* name_prefix) {
  const size_t plen = name_prefix ? strlen(name_prefix) : 0;
  const uint32_t nm = paired ? 2 : 1;
  SG_ENSURE(ctx->prefix, plen + 16);
  SG_ENSURE(ctx->pairs, ((size_t)n_slots + 1) * sizeof(sg::PairRec));
  SG_ENSURE(ctx->win_actual, (nw + 1) * 4);
  SG_ENSURE(ctx->win_namebase, (nw + 1) * 4);
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
  B.win_actual = ctx->win_actual.as<uint32_t>();
  B.win_namebase = ctx->win_namebase.as<uint32_t>();
  B.events = ctx->events.as<uint32_t>();
  B.recloc = ctx->recoff.as<uint32_t>();
  B.blkbase = ctx->bsum.as<uint64_t>();
  B.seg_shift = sg::record_seg_shift((uint32_t)n_slots);
  B.meta = ctx->meta.as<uint4>();
  B.totals = ctx->totals.as<uint64_t>();
  B.slowq_count = (uint32_t*)(B.totals + 4);
  ctx->pass = sg_ctx::Pass(sg_ctx::Pass::Planned);
  return SG_OK;
}

// The chains or the profile changed: the plan is gone, and a pass's rows no longer belong to them (its text stays).
static void retire_plan(sg_ctx* ctx) {
  if (ctx->pass.stage <= sg_ctx::Pass::Planned) ctx->pass = sg_ctx::Pass();
  else ctx->pass.rows_current = false;
}

// The pass is over (its outputs were detached, or it failed): back to its plan, if that is still good.
static void restart_pass(sg_ctx* ctx) {
  ctx->pass = sg_ctx::Pass(ctx->pass.rows_current ? sg_ctx::Pass::Planned : sg_ctx::Pass::None);
}

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

// ---- truth outputs: the piece map's and the pass's preconditions (sg_api.h) ----
static int truth_need_map(sg_ctx* ctx, const char* who) {
  if (!ctx->truth.from_build)
    return ctx->fail(SG_ERR_INVALID, std::string(who) + ": the chains have no piece map (they were not made by sg_build_haplotypes)");
  if (!ctx->truth.mapped) return ctx->fail(SG_ERR_INVALID, std::string(who) + ": call sg_truth_map first");
  return SG_OK;
}

static int rows_need_current(sg_ctx* ctx, const char* who) {
  if (ctx->pass.rows_current) return SG_OK;
  return ctx->fail(SG_ERR_INVALID, std::string(who) + ": the chains or the profile changed since sg_sample");
}

int sg_pass_prelude(sg_ctx* ctx, const char* who, sg::PieceMap* map, bool bam_names) {
  if (int rc = rows_need_current(ctx, who)) return rc;
  if (map)
    if (int rc = truth_need_map(ctx, who)) return rc;
  if (int rc = sg_pass_need(ctx, who, sg_ctx::Pass::Settled)) return rc;
  const sg::DevBatch& B = ctx->B;
  const uint32_t nm = B.paired ? 2 : 1;
  if (map && (uint64_t)B.n_slots * nm >= 0xFFFFFFF0ull) return ctx->fail(SG_ERR_UNSUPPORTED, std::string(who) + ": more than 2^32 reads in one pass");
  if (bam_names && B.prefix_len > 200) return ctx->fail(SG_ERR_UNSUPPORTED, std::string(who) + ": read names longer than a BAM record holds");
  if (B.diag)
    return ctx->fail(SG_ERR_UNSUPPORTED, std::string(who) + ": the pass ran under SG_DIAG (a timing ablation: its reads are not those of their rows)");
  if (map) {
    const size_t n_chains = ctx->hap.len.size();
    map->chain_first = ctx->truth.map.as<uint64_t>();
    map->pieces = (const sg::TruthPiece*)(ctx->truth.map.as<uint8_t>() + sg::truth_map_pieces_at(n_chains));
    map->n_chains = (uint32_t)n_chains;
    map->n_reads = B.n_slots * nm;
  }
  return SG_OK;
}

extern "C" {

uint64_t sg_cdf_count_le(double c) { return sg::count_le(c); }

int sg_sub_row_identity_first(const double cdf4[4], int cd, uint64_t cum[3], uint8_t order[4]) {
  if (!cdf4 || !cum || !order || cd < 0 || cd > 3) return SG_ERR_INVALID;
  const sg::SubRow r = sg::encode_sub_row_identity_first(cdf4, cd);
  for (int i = 0; i < 3; i++) cum[i] = r.c[i];
  for (int i = 0; i < 4; i++) order[i] = r.order[i];
  return SG_OK;
}

uint32_t sg_row_symbols(const double* cdf, int n) { return (cdf && n > 0) ? sg::symbols_with_mass(sg::row_masses(cdf, n)) : 0u; }

int sg_alias_row(const double* cdf, int n, uint32_t lgW, uint32_t* thr, uint8_t* lo, uint8_t* hi) {
  if (!cdf || n < 1 || n > 256 || lgW < 2 || lgW > 8 || !thr || !lo || !hi) return SG_ERR_INVALID;
  try {
    const sg::AliasRow r = sg::build_alias_row(sg::row_masses(cdf, n), lgW);
    for (uint32_t c = 0; c < (1u << lgW); c++) { thr[c] = r.thr[c]; lo[c] = r.lo[c]; hi[c] = r.hi[c]; }
  } catch (const std::exception&) {
    return SG_ERR_INVALID;
  }
  return SG_OK;
}

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

// ------------------------------------------------------------------------------------------------
// The tables of a profile as the engine wants them, made on the host (sg_profile_prepare: no device, any thread) and
// uploaded by sg_load_prepared_profile.  Offsets are in 32-bit words into `tab`.
struct sg_profile_tables {
  std::vector<uint32_t> tab;
  size_t sub_off = 0, sub_rows = 0, alias_off = 0, fast_lds_off = 0, fast_sub_off = 0, fast_alias_off = 0, ins_off = 0, del_off = 0, isz_off = 0,
         gap_off = 0;
  uint32_t lgW = 0, fast_stride = 0, ins_lg = 0, del_lg = 0, isz_lg = 0, inv_remap = 0, remap = 0, packed = 0;
  bool has2 = false, has_isz = false;
  uint64_t evA = 0, evB = 0;
  int kmer = 0, bins = 0, read_length = 0, min_qual = 0, isize_min = 0, insert_size = 0, n_isize = 0;
  int rc = SG_OK;
  std::string err;
  int fail(int code, const std::string& msg) { rc = code; err = msg; return code; }
};

static int build_tables(const sg_profile_cdf* pr, sg_profile_tables& T) {
  if (!pr) return T.fail(SG_ERR_INVALID, "sg_profile_prepare: null profile");
  if (pr->n_bases != 4) return T.fail(SG_ERR_UNSUPPORTED, "sg_load_profile: only 4-letter base alphabets are supported");
  if (pr->kmer < 1 || pr->kmer > 6) return T.fail(SG_ERR_UNSUPPORTED, "sg_load_profile: kmer must be in 1..6");
  if (pr->bins < 1 || pr->read_length < 1 || pr->read_length > 30000) return T.fail(SG_ERR_INVALID, "sg_load_profile: bad bins/read_length");
  {  // the kernels compute bin = i*bins/n' with a 32-bit reciprocal: exact while i*bins*n' < 2^32
    const uint64_t npmax = (uint64_t)pr->read_length + (uint64_t)SG_MAX_EVENTS * (uint64_t)(pr->n_ins > 0 ? pr->n_ins : 1);
    if (npmax > 0xFFFF || npmax * (uint64_t)pr->bins * npmax >= (1ull << 32))
      return T.fail(SG_ERR_UNSUPPORTED, "sg_load_profile: read_length * bins too large for the 32-bit bin arithmetic");
  }
  if (pr->n_qual < 1 || pr->n_qual > 128) return T.fail(SG_ERR_INVALID, "sg_load_profile: n_qual must be in 1..128 (quality symbols are 7-bit fields)");
  if (!pr->subs_cdf1 || !pr->qual_cdf || !pr->ins_cdf || !pr->del_cdf || pr->n_ins < 1 || pr->n_del < 1)
    return T.fail(SG_ERR_INVALID, "sg_load_profile: missing table");
  // base alphabet must be a permutation of ACGT (the kernels classify haplotype bytes by value)
  uint32_t remap = 0, packed = 0;
  {
    const char nat[4] = {'A', 'C', 'T', 'G'};  // natural index = (byte >> 1) & 3
    for (int n = 0; n < 4; n++) {
      int code = -1;
      for (int k = 0; k < 4; k++) if (pr->bases[k] == nat[n]) code = k;
      if (code < 0) return T.fail(SG_ERR_UNSUPPORTED, "sg_load_profile: bases must be a permutation of ACGT");
      remap |= (uint32_t)code << (2 * n);
    }
    for (int k = 0; k < 4; k++) packed |= (uint32_t)(uint8_t)pr->bases[k] << (8 * k);
  }
  int kmer_count = 0;
  {
    int p = 1;
    for (int m = 1; m <= pr->kmer; m++) { p *= 4; kmer_count += p; }
  }
  const int bins = pr->bins;
  const bool has2 = pr->subs_cdf2 != nullptr;

  // context -> index of its last base (the reference base a substitution row is about): contexts with m real bases are
  // numbered in base-4 counting order (Profile::initKmers, Profile.cpp:70-124), so the last base is the lowest digit
  std::vector<uint8_t> ctx_cd((size_t)kmer_count);
  {
    int off = 0, p4 = 1;
    for (int m = 1; m <= pr->kmer; m++) {
      p4 *= 4;
      for (int v = 0; v < p4; v++) ctx_cd[off + v] = (uint8_t)(v & 3);
      off += p4;
    }
  }
  std::vector<uint32_t>& tab = T.tab;
  // substitution rows, identity first (sg_tables.h): {D0, D1, D2, j0 | o0<<2 | o1<<4 | o2<<6 | o3<<8}, o in profile codes
  const size_t sub_rows = (size_t)kmer_count * bins;
  const size_t sub_off = 0;
  const int n_mates = has2 ? 2 : 1;
  std::vector<sg::SubRow> srows((size_t)n_mates * sub_rows);
  tab.resize((size_t)n_mates * sub_rows * 4);
  for (int t = 0; t < n_mates; t++) {
    const double* src = t == 0 ? pr->subs_cdf1 : pr->subs_cdf2;
    for (size_t r = 0; r < sub_rows; r++) {
      const sg::SubRow sr = sg::encode_sub_row_identity_first(src + r * 4, ctx_cd[r / bins]);
      srows[t * sub_rows + r] = sr;
      uint32_t* o = &tab[(t * sub_rows + r) * 4];
      o[0] = sr.D[0]; o[1] = sr.D[1]; o[2] = sr.D[2];
      o[3] = sr.j0 | (uint32_t)sr.order[0] << 2 | (uint32_t)sr.order[1] << 4 | (uint32_t)sr.order[2] << 6 | (uint32_t)sr.order[3] << 8;
    }
  }
  // quality rows as alias columns (sg_tables.h): [16][bins][W] x {thr, lo | hi << 8}
  const size_t qrows = (size_t)16 * bins;
  std::vector<std::vector<uint64_t>> qmass(qrows);
  uint32_t most = 1;
  for (size_t r = 0; r < qrows; r++) {
    qmass[r] = sg::row_masses(pr->qual_cdf + r * pr->n_qual, pr->n_qual);
    most = std::max(most, sg::symbols_with_mass(qmass[r]));
  }
  uint32_t lgW = 2;
  while ((1u << lgW) < most) lgW++;
  const uint32_t W = 1u << lgW;
  std::vector<sg::AliasRow> arows(qrows);
  try {
    for (size_t r = 0; r < qrows; r++) arows[r] = sg::build_alias_row(qmass[r], lgW);
  } catch (const std::exception& e) {
    return T.fail(SG_ERR_INVALID, std::string("sg_load_profile: ") + e.what());
  }
  while (tab.size() % 4) tab.push_back(0);
  const size_t alias_off = tab.size();
  tab.resize(alias_off + qrows * W * 2);
  for (size_t r = 0; r < qrows; r++)
    for (uint32_t c = 0; c < W; c++) {
      tab[alias_off + (r * W + c) * 2] = arows[r].thr[c];
      tab[alias_off + (r * W + c) * 2 + 1] = (uint32_t)arows[r].lo[c] | (uint32_t)arows[r].hi[c] << 8;
    }
  auto add_row = [&](const double* cdf, int n, size_t& off, uint32_t& lg) {
    sg::Row r = sg::encode_row(cdf, n);
    uint32_t W = sg::pow2_at_least((uint32_t)r.T.size());
    lg = sg::log2u(W);
    off = tab.size();
    tab.resize(off + 1 + W, 0xFFFFFFFFu);
    tab[off] = r.k0;
    for (size_t i = 0; i < r.T.size(); i++) tab[off + 1 + i] = r.T[i];
    while (tab.size() % 4) tab.push_back(0xFFFFFFFFu);
  };
  size_t ins_off, del_off, isz_off = 0;
  uint32_t ins_lg, del_lg, isz_lg = 0;
  while (tab.size() % 4) tab.push_back(0xFFFFFFFFu);
  add_row(pr->ins_cdf, pr->n_ins, ins_off, ins_lg);
  add_row(pr->del_cdf, pr->n_del, del_off, del_lg);
  const bool has_isz = pr->isize_cdf != nullptr && pr->n_isize > 0;
  if (has_isz) add_row(pr->isize_cdf, pr->n_isize, isz_off, isz_lg);
  // Sequencing indels by skipping ahead: getIndelSeq tests every template position with `p <= insertRate`, then
  // `p < delRate/(1-insertRate)`, p = x/2^32 (Profile.cpp:1560-1570).  cI, cD = the numbers of 32-bit draws that pass;
  // a position is a candidate with probability evB / 2^64, evB = cI 2^32 + (2^32 - cI) cD, an insertion with evA / evB,
  // evA = cI 2^32.  gap[k] = floor(gap[k-1] * gap[1] / 2^64), gap[1] = 2^64 - evB: P(no candidate in k positions).
  if (pr->insert_rate < 0) return T.fail(SG_ERR_INVALID, "sg_load_profile: negative insert rate");
  const uint64_t ci = sg::count_unit_le(pr->insert_rate);
  const uint64_t cd = sg::count_unit_lt(pr->del_rate / (1 - pr->insert_rate));
  if (ci >= (1ull << 31) || cd >= (1ull << 31)) return T.fail(SG_ERR_UNSUPPORTED, "sg_load_profile: sequencing indel rate >= 0.5");
  const uint64_t evA = ci << 32, evB = evA + ((1ull << 32) - ci) * cd;
  while (tab.size() % 4) tab.push_back(0);
  const size_t gap_off = tab.size();
  {
    const int L = std::max(pr->read_length, 1);
    std::vector<uint64_t> gap((size_t)L + 1, 0xFFFFFFFFFFFFFFFFull);
    if (evB) {
      gap[1] = 0ull - evB;
      for (int k = 1; k < L; k++) gap[(size_t)k + 1] = (uint64_t)(((unsigned __int128)gap[(size_t)k] * gap[1]) >> 64);
    }
    tab.resize(gap_off + 2 * gap.size());
    memcpy(&tab[gap_off], gap.data(), gap.size() * 8);
    while (tab.size() % 4) tab.push_back(0);
  }
  // Straight-line kernel tables (kmer 3).  The kernel packs base codes 2 bits each in NATURAL order (A0 C1 T2 G3) with
  // the OLDEST base of a context in the lowest digit; the reference numbers a context with its oldest base in the
  // highest digit, in `bases` order (Profile::initKmers).  Context ids of the kernel: [0,4) one base, [4,20) two, [20,84)
  // three.  Everything below is indexed by the kernel's ids and natural base codes.
  uint32_t inv_remap = 0;
  for (int n = 0; n < 4; n++) inv_remap |= (uint32_t)n << (2 * ((remap >> (2 * n)) & 3u));
  size_t fast_lds_off = 0, fast_sub_off = 0, fast_alias_off = 0;
  uint32_t fast_stride = 0;
  if (pr->kmer == 3) {
    std::vector<uint32_t> perm;  // kernel context id -> reference context id
    uint32_t off = 0, p4 = 1;
    for (int m = 1; m <= 3; m++) {
      p4 *= 4;
      for (uint32_t v = 0; v < p4; v++) {
        uint32_t src = 0;
        for (int tt = 0; tt < m; tt++) {
          const uint32_t nat = (v >> (2 * tt)) & 3u;  // base at age position tt (0 = oldest)
          src |= ((remap >> (2 * nat)) & 3u) << (2 * (m - 1 - tt));
        }
        perm.push_back(off + src);
      }
      off += p4;
    }
    auto nat_of = [&](uint32_t prof) { return (inv_remap >> (2u * prof)) & 3u; };
    auto prof_of = [&](uint32_t nat) { return (remap >> (2u * nat)) & 3u; };
    // kernel context ids: [0,4) one base, [4,20) two, [20,84) three, the oldest base in the lowest digit.  Per bin the
    // tables hold 192 context rows addressed by the 6-bit field kv = b[i-2] | b[i-1] << 2 | b[i] << 4 of the packed
    // codes: [0,64) the three-base contexts, [64,128) the two-base contexts (kv >> 2; a read's second base) and
    // [128,192) the one-base contexts (kv >> 4; a read's first base), so that every position uses the same extract.
    auto ctx_of = [&](uint32_t slot) -> uint32_t {
      const uint32_t kv = slot & 63u;
      return slot < 64u ? perm[20u + kv] : slot < 128u ? perm[4u + (kv >> 2)] : perm[kv >> 4];
    };
    fast_stride = 192u + 4u * W;
    while (tab.size() % 4) tab.push_back(0);
    // (1) the LDS image, per mate and bin: [0,192) keep_h - 1 of the context's row, keep_h = c0 >> 16 (a 16-bit head
    //     below keep_h is certainly "no substitution"); [192, 192 + 4W) the diagonal alias columns (reference base ==
    //     called base) in the order [col][natural base] as  col << (16 - lgW) | thr >> 16  in the low half (the draw's
    //     low half minus it is u_head - thr_head: the column bits cancel),  (lo ^ hi) << 16 | hi << 24  above, lo and hi as
    //     characters (symbol + the profile's lowest quality character)
    fast_lds_off = tab.size();
    tab.resize(fast_lds_off + (size_t)n_mates * bins * fast_stride);
    const uint32_t mq = (uint32_t)pr->min_qual;
    for (int t = 0; t < n_mates; t++)
      for (int b = 0; b < bins; b++) {
        uint32_t* blk = &tab[fast_lds_off + ((size_t)t * bins + b) * fast_stride];
        for (uint32_t sl = 0; sl < 192; sl++) blk[sl] = (uint32_t)(srows[t * sub_rows + (size_t)ctx_of(sl) * bins + b].c[0] >> 16) - 1u;
        for (uint32_t cdn = 0; cdn < 4; cdn++) {
          const uint32_t pc = prof_of(cdn);
          const sg::AliasRow& ar = arows[((size_t)pc * 4 + pc) * bins + b];
          for (uint32_t c = 0; c < W; c++)
            blk[192 + c * 4 + cdn] = (c << (16 - lgW)) | (ar.thr[c] >> 16) | (uint32_t)((ar.lo[c] + mq) ^ (ar.hi[c] + mq)) << 16 | (uint32_t)(ar.hi[c] + mq) << 24;
        }
      }
    // (2) full substitution rows for the kernel's fix-up path: [mate][bin][192] x {D0, D1, D2, j0 | n0<<2 | .. | n3<<8}
    while (tab.size() % 4) tab.push_back(0);
    fast_sub_off = tab.size();
    tab.resize(fast_sub_off + (size_t)n_mates * bins * 192 * 4);
    for (int t = 0; t < n_mates; t++)
      for (int b = 0; b < bins; b++)
        for (uint32_t sl = 0; sl < 192; sl++) {
          const sg::SubRow& sr = srows[t * sub_rows + (size_t)ctx_of(sl) * bins + b];
          uint32_t* o = &tab[fast_sub_off + (((size_t)t * bins + b) * 192 + sl) * 4];
          o[0] = sr.D[0]; o[1] = sr.D[1]; o[2] = sr.D[2];
          o[3] = sr.j0 | nat_of(sr.order[0]) << 2 | nat_of(sr.order[1]) << 4 | nat_of(sr.order[2]) << 6 | nat_of(sr.order[3]) << 8;
        }
    // (3) all alias columns in natural order: [cdn][kn][bins][W] x {thr, lo | hi << 8}
    fast_alias_off = tab.size();
    tab.resize(fast_alias_off + qrows * W * 2);
    for (uint32_t cdn = 0; cdn < 4; cdn++)
      for (uint32_t kn = 0; kn < 4; kn++)
        for (int b = 0; b < bins; b++) {
          const sg::AliasRow& ar = arows[((size_t)prof_of(cdn) * 4 + prof_of(kn)) * bins + b];
          uint32_t* o = &tab[fast_alias_off + ((((size_t)cdn * 4 + kn) * bins + b) * W) * 2];
          for (uint32_t c = 0; c < W; c++) { o[2 * c] = ar.thr[c]; o[2 * c + 1] = (uint32_t)ar.lo[c] | (uint32_t)ar.hi[c] << 8; }
        }
    while (tab.size() % 4) tab.push_back(0);
  }

  T.sub_off = sub_off; T.sub_rows = sub_rows; T.has2 = has2; T.alias_off = alias_off; T.lgW = lgW;
  T.fast_lds_off = fast_lds_off; T.fast_sub_off = fast_sub_off; T.fast_alias_off = fast_alias_off; T.fast_stride = fast_stride;
  T.ins_off = ins_off; T.ins_lg = ins_lg; T.del_off = del_off; T.del_lg = del_lg; T.isz_off = isz_off; T.isz_lg = isz_lg; T.has_isz = has_isz;
  T.inv_remap = inv_remap; T.remap = remap; T.packed = packed; T.evA = evA; T.evB = evB; T.gap_off = gap_off;
  T.kmer = pr->kmer; T.bins = bins; T.read_length = pr->read_length; T.min_qual = pr->min_qual;
  T.isize_min = pr->isize_min; T.insert_size = pr->insert_size; T.n_isize = pr->n_isize;
  return SG_OK;
}

int sg_profile_prepare(const sg_profile_cdf* pr, sg_profile_tables** out) {
  if (!out) return SG_ERR_INVALID;
  sg_profile_tables* T = new sg_profile_tables();
  *out = T;
  T->rc = build_tables(pr, *T);
  return T->rc;
}
const char* sg_profile_tables_error(const sg_profile_tables* T) { return T ? T->err.c_str() : "null tables"; }
void sg_profile_tables_free(sg_profile_tables* T) { delete T; }

int sg_load_prepared_profile(sg_ctx* ctx, const sg_profile_tables* Tp) {
  if (!ctx || !Tp) return SG_ERR_INVALID;
  const sg_profile_tables& T = *Tp;
  if (T.rc != SG_OK) return ctx->fail(T.rc, T.err);
  SG_HIP(hipSetDevice(ctx->device));
  const std::vector<uint32_t>& tab = T.tab;
  SG_ENSURE(ctx->tab, tab.size() * 4);
  SG_HIP(hipMemcpyAsync(ctx->tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));

  sg::DevProfile& P = ctx->P;
  const uint32_t* base = ctx->tab.as<uint32_t>();
  P.sub = (const uint4*)(base + T.sub_off);
  P.sub_mate_rows = T.has2 ? (uint32_t)T.sub_rows : 0u;
  P.alias = (const uint2*)(base + T.alias_off);
  P.lgW = T.lgW;
  P.fast_lds = T.kmer == 3 ? base + T.fast_lds_off : nullptr;
  P.fast_mate_words = T.has2 ? (uint32_t)T.bins * T.fast_stride : 0u;
  P.fast_stride = T.fast_stride;
  P.fast_sub = T.kmer == 3 ? (const uint4*)(base + T.fast_sub_off) : nullptr;
  P.fast_alias = T.kmer == 3 ? (const uint2*)(base + T.fast_alias_off) : nullptr;
  P.ins_row = base + T.ins_off; P.ins_lg = T.ins_lg;
  P.del_row = base + T.del_off; P.del_lg = T.del_lg;
  P.isz_row = T.has_isz ? base + T.isz_off : nullptr; P.isz_lg = T.isz_lg;
  P.inv_remap_packed = T.inv_remap;
  P.isz_min = T.isize_min;
  P.fixed_isz = T.insert_size;
  P.isz_lo = T.has_isz ? T.isize_min : T.insert_size;
  P.isz_hi = T.has_isz ? T.isize_min + T.n_isize - 1 : T.insert_size;
  P.evA = T.evA; P.evB = T.evB;
  P.gap_row = (const uint64_t*)(base + T.gap_off);
  P.L = T.read_length; P.bins = T.bins; P.kmer = T.kmer; P.min_qual = T.min_qual;
  P.remap_packed = T.remap; P.bases_packed = T.packed;
  {
    uint32_t off = 0, p = 1;
    for (int m = 0; m < 8; m++) P.kmer_off[m] = 0;
    for (int m = 1; m <= T.kmer; m++) { P.kmer_off[m] = off; p *= 4; off += p; }
  }
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

// ------------------------------------------------------------------------------------------------
// detached outputs
// ------------------------------------------------------------------------------------------------
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
  std::swap(ctx->out1, o->text[0]); std::swap(ctx->out2, o->text[1]);
  std::swap(ctx->gz1, o->gz[0]); std::swap(ctx->gz2, o->gz[1]);
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
  const uint64_t have = compressed ? o->gz_bytes[mate] : o->text_bytes[mate];
  if (offset + bytes > have) { o->err = "sg_outputs_fetch: range past the end of the data"; return SG_ERR_INVALID; }
  if (!bytes) return SG_OK;
  hipError_t e = hipSetDevice(o->device);
  const uint8_t* src = (compressed ? o->gz[mate] : o->text[mate]).as<uint8_t>() + offset;
  if (e == hipSuccess) e = hipMemcpyAsync(host_dst, src, bytes, hipMemcpyDeviceToHost, o->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(o->stream);
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

// ------------------------------------------------------------------------------------------------
// block-gzip sink (kernels: sg_deflate.hip, code construction: sg_deflate.cpp)
// ------------------------------------------------------------------------------------------------
int sg_bgzf_eof(uint8_t out[28]) {
  static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (!out) return SG_ERR_INVALID;
  memcpy(out, eof, 28);
  return SG_OK;
}

uint32_t sg_deflate_plan(const uint64_t lit_counts[286], const uint64_t dist_counts[30], uint8_t lit_lens[286], uint32_t lit_codes[286],
                         uint8_t dist_lens[30], uint32_t dist_codes[30], uint32_t len_tokens[260], uint32_t* prefix_words, uint32_t cap) {
  if (!lit_counts || !dist_counts || !lit_lens || !lit_codes || !dist_lens || !dist_codes || !len_tokens || !prefix_words) return 0;
  sg::DeflatePlan plan;
  sg::deflate_build_plan(lit_counts, dist_counts, &plan);
  if (plan.prefix.size() > cap) return 0;
  memcpy(lit_lens, plan.lit_len, sizeof plan.lit_len);
  memcpy(lit_codes, plan.lit_code, sizeof plan.lit_code);
  memcpy(dist_lens, plan.dist_len, sizeof plan.dist_len);
  memcpy(dist_codes, plan.dist_code, sizeof plan.dist_code);
  memcpy(len_tokens, plan.len_token, sizeof plan.len_token);
  memcpy(prefix_words, plan.prefix.data(), plan.prefix.size() * 4);
  return plan.prefix_bits;
}

// (declared in sg_api.h, not part of the ABI)
extern "C++" int deflate_text(sg_ctx* ctx, const uint8_t* text, uint64_t bytes, DevBuf& gz, uint64_t* gz_total, const char* who) {
  hipStream_t s = ctx->stream;
  ctx->gz_last = sg_ctx::GzLast();
  if (bytes / sg::kGzChunk >= 0xFFFFFFF0ull) return ctx->fail(SG_ERR_UNSUPPORTED, std::string(who) + ": text too large");
  const uint32_t n_chunks = (uint32_t)((bytes + sg::kGzChunk - 1) / sg::kGzChunk);
  // work buffer: hist[320] u64 | total u64 | counters | tables | msize[n] u32 | moff[n] u64 | block sums | lane bits | records
  const size_t head = 320 * 8 + 64;
  const size_t tab_words = 288 + sg::kGzLenTokens + 32 + 1024 + sg::kGzLevels * 128 + 256;  // + prefix (<= 256 words)
  const size_t off_tab = head, off_msize = off_tab + tab_words * 4;
  const size_t off_moff = (off_msize + (size_t)n_chunks * 4 + 63) & ~(size_t)63;
  const size_t off_bsum = off_moff + (size_t)n_chunks * 8;
  const size_t off_lbits = (off_bsum + ((size_t)sg::scan_blocks(n_chunks) + 8) * 8 + 63) & ~(size_t)63;
  const size_t off_rec = (off_lbits + (size_t)n_chunks * sg::kGzThreads * 4 + 63) & ~(size_t)63;
  SG_ENSURE(ctx->gz_work, off_rec + (size_t)n_chunks * sg::kGzThreads * 32);
  uint8_t* wk = ctx->gz_work.as<uint8_t>();
  sg::DevDeflate D;
  memset(&D, 0, sizeof D);
  D.text = text; D.bytes = bytes; D.n_chunks = n_chunks;
  D.min_run = sg::kGzMinRun;
  D.min_copy = sg::kGzMinGramMatch;
  if (const char* e = getenv("SG_GZ_MINCOPY")) D.min_copy = (uint32_t)std::max(8, atoi(e));   // (experiments)
  if (const char* e = getenv("SG_GZ_MINRUN")) D.min_run = (uint32_t)std::max(3, atoi(e));   // (experiments)
  D.hist = (unsigned long long*)wk;
  D.next = (uint32_t*)(wk + 320 * 8 + 16);  // inside the zeroed head of the work buffer
  D.msize = (uint32_t*)(wk + off_msize);
  D.moff = (const uint64_t*)(wk + off_moff);
  D.lbits = (uint32_t*)(wk + off_lbits);
  D.rec = (uint4*)(wk + off_rec);
  // 1. token histogram of every 16th member -> the two Huffman codes, member prefix, CRC tables (host)
  SG_HIP(hipMemsetAsync(wk, 0, head, s));
  sg::launch_gz_hist(D, n_chunks, s);
  SG_HIP(hipGetLastError());
  uint64_t hist[320];
  SG_HIP(hipMemcpyAsync(hist, wk, sizeof hist, hipMemcpyDeviceToHost, s));
  SG_HIP(hipStreamSynchronize(s));
  sg::DeflatePlan plan;
  sg::deflate_build_plan(hist, hist + 288, &plan);
  if (plan.prefix.size() > 256) return ctx->fail(SG_ERR_UNSUPPORTED, std::string(who) + ": block header longer than expected");
  if (getenv("SG_GZ_TRACE")) {   // where the sampled members' bits go: literals by character, matches by length / distance symbol
    double lit_bits[256], tot_lit = 0, tot_len = 0, tot_dist = 0, n_match = 0, n_lit = 0, match_bytes = 0;
    static const int lbase[29] = {3,4,5,6,7,8,9,10,11,13,15,17,19,23,27,31,35,43,51,59,67,83,99,115,131,163,195,227,258};
    static const int lext[29] = {0,0,0,0,0,0,0,0,1,1,1,1,2,2,2,2,3,3,3,3,4,4,4,4,5,5,5,5,0};
    for (int c = 0; c < 256; c++) { lit_bits[c] = (double)hist[c] * plan.lit_len[c]; tot_lit += lit_bits[c]; n_lit += (double)hist[c]; }
    for (int i = 0; i < 29; i++) { tot_len += (double)hist[257 + i] * (plan.lit_len[257 + i] + lext[i]); n_match += (double)hist[257 + i];
                                   match_bytes += (double)hist[257 + i] * (lbase[i] + (i + 1 < 29 ? (lbase[i + 1] - lbase[i] - 1) / 2.0 : 0)); }
    for (int i = 0; i < 30; i++) tot_dist += (double)hist[288 + i] * (plan.dist_len[i] + (i < 4 ? 0 : (i - 2) / 2));
    const double members = (double)hist[256], all = tot_lit + tot_len + tot_dist;
    fprintf(stderr, "[gz] per member: %.0f literals %.0f bits, %.0f matches (~%.0f bytes) %.0f length bits + %.0f distance bits; total %.0f bits = %.0f bytes\n",
            n_lit / members, tot_lit / members, n_match / members, match_bytes / members, tot_len / members, tot_dist / members, all / members, all / members / 8);
    fprintf(stderr, "[gz] literal bits per member by character:");
    for (int c = 0; c < 256; c++)
      if (lit_bits[c] / members >= 20) fprintf(stderr, " '%c'x%.0f(%d b)=%.0f", c >= 32 && c < 127 ? c : '?', hist[c] / members, plan.lit_len[c], lit_bits[c] / members);
    fprintf(stderr, "\n[gz] matches per member by length symbol:");
    for (int i = 0; i < 29; i++) if (hist[257 + i] / members >= 1) fprintf(stderr, " %d+:%0.f(%d b)", lbase[i], hist[257 + i] / members, plan.lit_len[257 + i] + lext[i]);
    fprintf(stderr, "\n[gz] distance symbols:");
    for (int i = 0; i < 30; i++) if (hist[288 + i] / members >= 1) fprintf(stderr, " %d:%.0f(%d b)", i, hist[288 + i] / members, plan.dist_len[i] + (i < 4 ? 0 : (i - 2) / 2));
    fprintf(stderr, "\n");
  }
  std::vector<uint32_t> tab(tab_words, 0);
  for (int i = 0; i < sg::kGzLitSyms; i++) tab[i] = plan.lit_code[i] | ((uint32_t)plan.lit_len[i] << 16);
  memcpy(&tab[288], plan.len_token, sizeof plan.len_token);
  for (int i = 0; i < sg::kGzDistSyms; i++) tab[288 + sg::kGzLenTokens + i] = plan.dist_code[i] | ((uint32_t)plan.dist_len[i] << 16);
  const size_t t_crc = 288 + sg::kGzLenTokens + 32;
  memcpy(&tab[t_crc], plan.crc_table, sizeof plan.crc_table);
  memcpy(&tab[t_crc + 1024], plan.crc_shift, sizeof plan.crc_shift);
  memcpy(&tab[t_crc + 1024 + sg::kGzLevels * 128], plan.prefix.data(), plan.prefix.size() * 4);
  SG_HIP(hipMemcpyAsync(wk + off_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, s));
  D.code = (const uint32_t*)(wk + off_tab);
  D.len_tok = D.code + 288;
  D.dist_code = D.len_tok + sg::kGzLenTokens;
  D.crc_tab = D.dist_code + 32;
  D.crc_shift = D.crc_tab + 1024;
  D.prefix = D.crc_shift + sg::kGzLevels * 128;
  D.prefix_words = (uint32_t)plan.prefix.size();
  D.prefix_bits = plan.prefix_bits;
  D.crc_init_full = plan.crc_init_full;
  const uint64_t last = bytes - (uint64_t)(n_chunks - 1) * sg::kGzChunk;
  D.crc_init_last = sg::crc_advance(plan, 0xFFFFFFFFu, last);
  // 2. tokens, member sizes -> offsets
  sg::launch_gz_match(D, n_chunks, s);
  sg::launch_scan_u32(D.msize, n_chunks, (uint64_t*)(wk + off_bsum), (uint64_t*)(wk + off_moff), (uint64_t*)(wk + 320 * 8), s);
  SG_HIP(hipGetLastError());
  uint64_t total = 0;
  SG_HIP(hipMemcpyAsync(&total, wk + 320 * 8, 8, hipMemcpyDeviceToHost, s));
  SG_HIP(hipStreamSynchronize(s));
  SG_ENSURE(gz, total + 64);
  D.out = gz.as<uint8_t>();
  // 3. encode
  sg::launch_gz_encode(D, n_chunks, plan.prefix_bits, s);
  SG_HIP(hipGetLastError());
  SG_HIP(hipStreamSynchronize(s));  // tab / plan are host-owned
  *gz_total = total;
  ctx->gz_last.text = text;
  ctx->gz_last.bytes = bytes;
  ctx->gz_last.moff = D.moff;
  return SG_OK;
}

int sg_compress(sg_ctx* ctx, uint64_t* gz_bytes_r1, uint64_t* gz_bytes_r2) {
  if (int rc = sg_pass_need(ctx, "sg_compress", sg_ctx::Pass::Settled)) return rc;
  sg_ctx::Pass& Q = ctx->pass;
  const int nm = ctx->B.paired ? 2 : 1;
  Q.have_gz = false;   // (a call that fails half-way leaves no members and no sizes)
  Q.gz_bytes[0] = Q.gz_bytes[1] = 0;
  uint64_t gz[2] = {0, 0};
  for (int m = 0; m < nm; m++) {
    const uint64_t bytes = Q.host_totals[m];
    if (!bytes) continue;
    const uint8_t* text = m == 0 ? ctx->out1.as<uint8_t>() : ctx->out2.as<uint8_t>();
    const int rc = deflate_text(ctx, text, bytes, m == 0 ? ctx->gz1 : ctx->gz2, &gz[m], "sg_compress");
    if (rc != SG_OK) return rc;
  }
  Q.have_gz = true;
  Q.gz_bytes[0] = gz[0];
  Q.gz_bytes[1] = gz[1];
  if (gz_bytes_r1) *gz_bytes_r1 = Q.gz_bytes[0];
  if (gz_bytes_r2) *gz_bytes_r2 = Q.gz_bytes[1];
  return SG_OK;
}

int sg_deflate_bgzf(sg_ctx* ctx, const void* text, uint64_t bytes, void* out, uint64_t out_cap, uint64_t* out_bytes) {
  if (!ctx || (bytes && !text) || !out_bytes) return SG_ERR_INVALID;
  *out_bytes = 0;
  if (!bytes) return SG_OK;
  SG_HIP(hipSetDevice(ctx->device));
  SG_ENSURE(ctx->defl_src, bytes + 64);
  SG_HIP(hipMemcpyAsync(ctx->defl_src.p, text, bytes, hipMemcpyHostToDevice, ctx->stream));
  uint64_t total = 0;
  const int rc = deflate_text(ctx, ctx->defl_src.as<uint8_t>(), bytes, ctx->defl_out, &total, "sg_deflate_bgzf");
  if (rc != SG_OK) return rc;
  *out_bytes = total;
  if (total > out_cap) return ctx->fail(SG_ERR_OVERFLOW, "sg_deflate_bgzf: the members do not fit out_cap");
  if (!out) return SG_ERR_INVALID;
  SG_HIP(hipMemcpy(out, ctx->defl_out.p, total, hipMemcpyDeviceToHost));
  return SG_OK;
}

int sg_fetch_compressed(sg_ctx* ctx, int mate, uint64_t offset, uint64_t bytes, void* host_dst) {
  if (!ctx || mate < 0 || mate > 1 || (bytes && !host_dst)) return SG_ERR_INVALID;
  if (!ctx->pass.have_gz) return ctx->fail(SG_ERR_INVALID, "sg_fetch_compressed: call sg_compress first");
  if (offset + bytes > ctx->pass.gz_bytes[mate]) return ctx->fail(SG_ERR_INVALID, "sg_fetch_compressed: range past the end of the compressed text");
  SG_HIP(hipSetDevice(ctx->device));
  if (bytes) {
    const uint8_t* src = (mate == 0 ? ctx->gz1.as<uint8_t>() : ctx->gz2.as<uint8_t>()) + offset;
    SG_HIP(hipMemcpyAsync(host_dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipStreamSynchronize(ctx->stream));
  }
  return SG_OK;
}

// ------------------------------------------------------------------------------------------------
// truth alignments (rule: sg_truth.h, kernels: sg_truth.hip)
// ------------------------------------------------------------------------------------------------
int sg_truth_align(const sg_truth_piece* pieces, uint64_t n_pieces, uint64_t tmpl_off, uint32_t tmpl_len, int reverse,
                   const uint32_t* events, uint32_t n_events, int32_t* contig, int64_t* pos0, uint32_t* cigar, uint32_t cap,
                   uint32_t* n_ops) {
  if (!pieces || !n_pieces || !contig || !pos0 || !n_ops || (cap && !cigar) || (n_events && !events) || n_events > SG_MAX_EVENTS ||
      tmpl_len == 0 || tmpl_len > 0xFFFFu)
    return SG_ERR_INVALID;
  std::vector<sg::TruthPiece> tp((size_t)n_pieces);
  for (uint64_t i = 0; i < n_pieces; i++) {
    const sg_truth_piece& p = pieces[i];
    if (p.len == 0 || p.contig > 0x3FFFFFFFu || (i && p.dst != pieces[i - 1].dst + pieces[i - 1].len)) return SG_ERR_INVALID;
    tp[i] = sg::TruthPiece{p.dst, p.src, p.len, sg::truth_meta(p.contig, p.kind, p.seg_first)};
  }
  if (tmpl_off < tp[0].dst || tmpl_off + tmpl_len > tp.back().dst + tp.back().len) return SG_ERR_INVALID;
  uint32_t next = 0;   // events ascend and stay apart: a deletion of [j, j + k) is followed by j + k at the earliest
  for (uint32_t e = 0; e < n_events; e++) {
    const uint32_t j = events[e] & 0xFFFFu, k = (events[e] >> 16) & 0x7FFFu, del = events[e] >> 31;
    if (k == 0 || j < next || j >= tmpl_len || (del && j + k > tmpl_len)) return SG_ERR_INVALID;
    next = del ? j + k : j + 1;
  }
  const uint64_t pi = sg::truth_find_piece(tp.data(), 0, n_pieces, tmpl_off);
  const sg::TruthAln A = sg::truth_walk(tp.data(), n_pieces, pi, tmpl_off, tmpl_len, reverse != 0, events, n_events,
                                        [&](uint32_t i, uint32_t v) { if (i < cap) cigar[i] = v; });
  *contig = A.contig;
  *pos0 = A.pos0;
  *n_ops = A.n_ops;
  return A.n_ops > cap ? SG_ERR_OVERFLOW : SG_OK;
}

int sg_truth_map(sg_ctx* ctx, const sg_hap_piece* pieces, const uint8_t* seg_first, uint64_t n_pieces, const int32_t* ref_ids,
                 uint32_t n_ref_ids) {
  if (!ctx || (n_pieces && (!pieces || !seg_first))) return SG_ERR_INVALID;
  sg_ctx::Truth& T = ctx->truth;
  if (!T.from_build || !ctx->have_haps)
    return ctx->fail(SG_ERR_INVALID, "sg_truth_map: the chains have no piece map (they were not made by sg_build_haplotypes)");
  if (n_pieces != T.n_given) return ctx->fail(SG_ERR_INVALID, "sg_truth_map: the pieces are not those of sg_build_haplotypes (another count)");
  SG_HIP(hipSetDevice(ctx->device));
  const size_t n_chains = ctx->hap.len.size();
  for (uint64_t i = 0; i < n_pieces; i++)
    if (pieces[i].chain >= n_chains) return ctx->fail(SG_ERR_INVALID, "sg_truth_map: piece " + std::to_string(i) + " names a chain that does not exist");
  std::vector<uint64_t> order((size_t)n_pieces);
  for (uint64_t i = 0; i < n_pieces; i++) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
    const sg_hap_piece &x = pieces[a], &y = pieces[b];
    return x.chain != y.chain ? x.chain < y.chain : x.dst < y.dst;
  });
  // Everything is checked and built beside the context's state, which changes only once nothing can fail any more: a
  // refused call leaves an earlier map as it was.  The pieces of a chain must tile it -- no hole, no overlap, none of
  // length 0 (the walk of sg_truth.h takes a piece's first base for granted).
  std::vector<sg_truth_piece> sorted((size_t)n_pieces);
  std::vector<uint64_t> chain_first(n_chains + 1, n_pieces);
  std::vector<sg::TruthPiece> dev((size_t)n_pieces);
  uint32_t chain = 0;
  uint64_t at = 0;   // offset in `chain` up to which it is tiled
  chain_first[0] = 0;
  auto chain_done = [&]() { return at == ctx->hap.len[chain]; };
  for (uint64_t i = 0; i < n_pieces; i++) {
    const sg_hap_piece& p = pieces[order[i]];
    while (chain < p.chain) {
      if (!chain_done()) return ctx->fail(SG_ERR_INVALID, "sg_truth_map: the pieces of chain " + std::to_string(chain) + " do not tile it");
      chain_first[++chain] = i;
      at = 0;
    }
    if (p.len == 0 || p.dst != at)
      return ctx->fail(SG_ERR_INVALID, "sg_truth_map: the pieces of chain " + std::to_string(chain) + " do not tile it (piece " + std::to_string(order[i]) + ")");
    at += p.len;
    sorted[i] = sg_truth_piece{p.dst, p.src, p.len, p.contig, p.kind ? 1u : 0u, seg_first[order[i]] ? 1u : 0u};
    int32_t ref = (int32_t)p.contig;
    if (ref_ids && !p.kind) {
      if (p.contig >= n_ref_ids) return ctx->fail(SG_ERR_INVALID, "sg_truth_map: a piece's contig has no entry in ref_ids");
      ref = ref_ids[p.contig];
    }
    if (ref < 0 || ref > 0x3FFFFFFF) return ctx->fail(SG_ERR_INVALID, "sg_truth_map: reference id out of range");
    dev[i] = sg::TruthPiece{p.dst, p.src, p.len, sg::truth_meta((uint32_t)ref, p.kind, seg_first[order[i]])};
  }
  for (;;) {
    if (n_chains && !chain_done()) return ctx->fail(SG_ERR_INVALID, "sg_truth_map: the pieces of chain " + std::to_string(chain) + " do not tile it");
    if (chain + 1 >= n_chains) break;
    chain_first[++chain] = n_pieces;
    at = 0;
  }
  // the way back for the tag kernels: refID -> the codes of the first contig row that carries it
  std::vector<sg::TagRef> refs;
  for (size_t c = ctx->ref_contigs.size(); c-- > 0;) {
    const int64_t ref = ref_ids ? (c < n_ref_ids ? ref_ids[c] : -1) : (int64_t)c;
    if (ref < 0 || ref >= (int64_t)ctx->ref_contigs.size()) continue;   // (a refID no contig row can hold: its records fail the tagged call)
    if (refs.size() <= (size_t)ref) refs.resize((size_t)ref + 1, sg::TagRef{0, 0});
    refs[(size_t)ref] = sg::TagRef{ctx->ref_contigs[c].code_off, ctx->ref_contigs[c].length};
  }
  T.mapped = false;   // (a copy that fails half-way leaves no map rather than a mixed one)
  ctx->pass.have_bam = false;   // (records of another map)
  T.n_refs = 0;
  if (!refs.empty()) {
    SG_ENSURE(T.refs, refs.size() * sizeof(sg::TagRef));
    SG_HIP(hipMemcpyAsync(T.refs.p, refs.data(), refs.size() * sizeof(sg::TagRef), hipMemcpyHostToDevice, ctx->stream));
  }
  const size_t first_b = sg::truth_map_pieces_at(n_chains);
  SG_ENSURE(T.map, first_b + dev.size() * sizeof(sg::TruthPiece) + 64);
  SG_HIP(hipMemcpyAsync(T.map.p, chain_first.data(), (n_chains + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  if (!dev.empty())
    SG_HIP(hipMemcpyAsync(T.map.as<uint8_t>() + first_b, dev.data(), dev.size() * sizeof(sg::TruthPiece), hipMemcpyHostToDevice, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));   // dev is host memory of this frame
  T.sorted.swap(sorted);
  T.chain_first.swap(chain_first);
  T.n_refs = (uint32_t)refs.size();
  T.mapped = true;
  return SG_OK;
}

int sg_truth_pieces(sg_ctx* ctx, uint32_t chain, sg_truth_piece* out, uint64_t cap, uint64_t* n) {
  if (!ctx || !n || (cap && !out)) return SG_ERR_INVALID;
  if (int rc = truth_need_map(ctx, "sg_truth_pieces")) return rc;
  const sg_ctx::Truth& T = ctx->truth;
  if ((size_t)chain + 1 >= T.chain_first.size()) return ctx->fail(SG_ERR_INVALID, "sg_truth_pieces: chain index out of range");
  const uint64_t a = T.chain_first[chain], b = T.chain_first[chain + 1];
  *n = b - a;
  if (b - a > cap) return ctx->fail(SG_ERR_OVERFLOW, "sg_truth_pieces: the pieces do not fit cap");
  std::copy(T.sorted.begin() + (long)a, T.sorted.begin() + (long)b, out);
  return SG_OK;
}

static_assert(sizeof(sg_truth_read) == sizeof(sg::TruthReadRow), "sg_truth_read is the kernel's row");

int sg_truth_reads(sg_ctx* ctx, int mate, uint32_t first_slot, uint32_t n, sg_truth_read* out) {
  if (!ctx || mate < 0 || mate > 1 || (n && !out)) return SG_ERR_INVALID;
  if (int rc = rows_need_current(ctx, "sg_truth_reads")) return rc;
  if (int rc = truth_need_map(ctx, "sg_truth_reads")) return rc;
  if (int rc = sg_pass_need(ctx, "sg_truth_reads", sg_ctx::Pass::Settled)) return rc;
  if (mate == 1 && !ctx->B.paired) return ctx->fail(SG_ERR_INVALID, "sg_truth_reads: a single-end pass has no mate 2");
  if ((uint64_t)first_slot + n > ctx->B.n_slots) return ctx->fail(SG_ERR_INVALID, "sg_truth_reads: slots past the end of the batch");
  if (!n) return SG_OK;
  SG_ENSURE(ctx->truth.rows, (size_t)n * sizeof(sg::TruthReadRow));
  sg::launch_truth_reads(ctx->P, ctx->B, (uint32_t)mate, first_slot, n, ctx->truth.rows.as<sg::TruthReadRow>(), ctx->stream);
  return sg_read_back(ctx, out, ctx->truth.rows.p, (size_t)n * sizeof(sg::TruthReadRow));
}

static_assert(SG_TAG_NM == sg::kTagNM && SG_TAG_MD == sg::kTagMD && SG_TAG_XE == sg::kTagXE, "SG_TAG_* are the kernels' bits");

int sg_truth_bam(sg_ctx* ctx, uint64_t* record_bytes, uint64_t* bgzf_bytes) { return sg_truth_bam_tags(ctx, 0, record_bytes, bgzf_bytes); }

int sg_truth_bam_tags(sg_ctx* ctx, uint32_t tags, uint64_t* record_bytes, uint64_t* bgzf_bytes) {
  return sg_pass_records(ctx, tags ? "sg_truth_bam_tags" : "sg_truth_bam", tags, false, record_bytes, bgzf_bytes);
}

// With tags == 0 exactly the kernels of the untagged stream are launched and nothing of the tags is allocated; with
// sorted == false nothing of the sort is launched or allocated.  (Declared in sg_api.h, not part of the ABI.)
extern "C++" int sg_pass_records(sg_ctx* ctx, const char* who, uint32_t tags, bool sorted, uint64_t* record_bytes, uint64_t* bgzf_bytes) {
  if (!ctx) return SG_ERR_INVALID;
  if (tags & ~(uint32_t)(SG_TAG_NM | SG_TAG_MD | SG_TAG_XE)) return ctx->fail(SG_ERR_INVALID, "sg_truth_bam_tags: tags is a mask of SG_TAG_NM, SG_TAG_MD and SG_TAG_XE");
  sg::TruthJob J;
  memset(&J, 0, sizeof J);
  if (int rc = sg_pass_prelude(ctx, who, &J.map, true)) return rc;
  sg_ctx::Truth& T = ctx->truth;
  if ((tags & (SG_TAG_NM | SG_TAG_MD)) && (!T.n_refs || !ctx->ref_codes.p))
    return ctx->fail(SG_ERR_INVALID, "sg_truth_bam_tags: NM and MD need the reference's codes (sg_reference_commit)");
  if (tags && (uint32_t)ctx->P.L > sg::kTruthTagMaxL)
    return ctx->fail(SG_ERR_UNSUPPORTED, "sg_truth_bam_tags: reads too long for the tagged record kernel (templates of more than " +
                                             std::to_string(sg::kTruthTagMaxL) + " bases)");
  sg_ctx::Pass& Q = ctx->pass;
  const sg::DevBatch& B = ctx->B;
  const uint32_t N = J.map.n_reads;
  Q.have_bam = Q.bam_sorted = false;
  Q.bam_rec_bytes = Q.bam_gz_bytes = Q.bam_records = Q.bam_unmapped = 0;
  for (uint64_t& v : Q.bam_tags) v = 0;
  hipStream_t s = ctx->stream;
  // the pack kernel's stages: one record's FASTQ text and one record's image, for reads of up to L + 512 bases
  const uint32_t np_cap = (uint32_t)ctx->P.L + 512u;
  J.text_lds = (16u + 256u + 2u * np_cap + 4u + 31u) & ~15u;
  const uint32_t tag_cap = tags ? sg::truth_tag_bytes(tags, sg::kTruthMaxMd) : 0u;
  J.image_lds = (16u + 36u + 256u + 4u * sg::kTruthMaxOps + np_cap + (np_cap + 1u) / 2u + tag_cap + 15u) & ~15u;
  if ((size_t)sg::kTruthWaveOps * 4 + 64 * 9 * 4 + J.text_lds + J.image_lds > 160u * 1024u)
    return ctx->fail(SG_ERR_UNSUPPORTED, std::string(who) + ": reads too long for the record kernel");
  // work buffer: counters (8 u64: records, unmapped, flags, -, stream bytes) | rows | rec_len | rec_off | block sums
  const size_t off_rows = 64, off_len = off_rows + (size_t)N * sizeof(sg::TruthRow);
  const size_t off_off = (off_len + (size_t)N * 4 + 63) & ~(size_t)63, off_bsum = off_off + (size_t)N * 8;
  SG_ENSURE(T.work, off_bsum + ((size_t)sg::scan_blocks(N) + 8) * 8);
  uint8_t* wk = T.work.as<uint8_t>();
  J.counters = (unsigned long long*)wk;
  J.rows = (sg::TruthRow*)(wk + off_rows);
  J.rec_len = (uint32_t*)(wk + off_len);
  J.rec_off = (const uint64_t*)(wk + off_off);
  // the tags' job: per-read rows {NM, XE, MD length} and behind them the sizing kernel's eight counters
  sg::TagJob G;
  memset(&G, 0, sizeof G);
  if (tags) {
    const size_t at = sg_counters_at((size_t)N * sizeof(sg::TagRow));
    SG_ENSURE(T.tag_rows, at + 64);
    G.tags = tags;
    G.n_refs = T.n_refs;
    G.refs = T.refs.as<sg::TagRef>();
    G.ref_codes = ctx->ref_codes.as<uint8_t>();
    G.rows = T.tag_rows.as<sg::TagRow>();
    G.counters = (unsigned long long*)(T.tag_rows.as<uint8_t>() + at);
    SG_HIP(hipMemsetAsync(G.counters, 0, 64, s));
  }
  uint64_t c[8] = {};
  int sort_rc = SG_OK;
  if (int rc = sg_run_counted(ctx, wk, 8, c, [&]() {
        if (!N) return;
        sg::launch_truth_size(ctx->P, B, J, s);
        if (tags) sg::launch_truth_tag_size(ctx->P, B, J, G, s);
        if (!sorted) sg::launch_scan_u32(J.rec_len, N, (uint64_t*)(wk + off_bsum), (uint64_t*)(wk + off_off), (uint64_t*)(wk + 32), s);
        else sort_rc = bamsort_pass_keys(ctx, J, B.paired != 0);
      }))
    return rc;
  if (sort_rc) return sort_rc;
  if (c[2] & 3) return ctx->fail(SG_ERR_OVERFLOW, std::string(who) + ": an alignment with more than " + std::to_string(sg::kTruthMaxOps) + " operations");
  uint64_t tc[8] = {};
  if (tags) {
    if (int rc = sg_read_back(ctx, tc, G.counters, 64)) return rc;
    if (tc[7] & 1) return ctx->fail(SG_ERR_INVALID, "sg_truth_bam_tags: a read whose events or operations do not end at its length");
    if (tc[7] & 2) return ctx->fail(SG_ERR_INVALID, "sg_truth_bam_tags: an alignment outside its contig of the committed reference");
    if (tc[7] & 4) return ctx->fail(SG_ERR_INVALID, "sg_truth_bam_tags: a record outside its mate's text");
  }
  if (sorted) {   // rec_off by read index from the lengths in key order
    if (int rc = bamsort_pass_order(ctx, J, (uint64_t*)(wk + off_off), &c[4])) return rc;
  }
  const uint64_t total = c[4];
  if (total) {
    SG_ENSURE(T.rec, total + 64);
    J.out = T.rec.as<uint8_t>();
    J.out_bytes = total;
    if (tags) sg::launch_truth_pack_tags(ctx->P, B, J, G, s);
    else sg::launch_truth_pack(ctx->P, B, J, s);
    uint64_t flags = 0;
    if (int rc = sg_read_back(ctx, &flags, wk + 16, 8)) return rc;
    if (flags & 4) return ctx->fail(SG_ERR_UNSUPPORTED, std::string(who) + ": a record does not fit the record kernel's stages");
    if (!sorted)
      if (int rc = deflate_text(ctx, T.rec.as<uint8_t>(), total, T.gz, &Q.bam_gz_bytes, who)) return rc;
  }
  for (int i = 0; i < 7; i++) Q.bam_tags[i] = tc[i];
  Q.bam_rec_bytes = total;
  Q.bam_records = c[0];
  Q.bam_unmapped = c[1];
  Q.have_bam = true;
  Q.bam_sorted = sorted;
  if (record_bytes) *record_bytes = Q.bam_rec_bytes;
  if (bgzf_bytes) *bgzf_bytes = Q.bam_gz_bytes;
  return SG_OK;
}

int sg_fetch_truth(sg_ctx* ctx, int compressed, uint64_t offset, uint64_t bytes, void* host_dst) {
  if (!ctx || (bytes && !host_dst)) return SG_ERR_INVALID;
  if (int rc = truth_need_map(ctx, "sg_fetch_truth")) return rc;
  if (!ctx->pass.have_bam) return ctx->fail(SG_ERR_INVALID, "sg_fetch_truth: call sg_truth_bam first");
  if (offset + bytes > (compressed ? ctx->pass.bam_gz_bytes : ctx->pass.bam_rec_bytes)) return ctx->fail(SG_ERR_INVALID, "sg_fetch_truth: range past the end of the data");
  SG_HIP(hipSetDevice(ctx->device));
  if (bytes) {
    const uint8_t* src = (compressed ? ctx->truth.gz : ctx->truth.rec).as<uint8_t>() + offset;
    SG_HIP(hipMemcpyAsync(host_dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    SG_HIP(hipStreamSynchronize(ctx->stream));
  }
  return SG_OK;
}

int sg_truth_tag_info(sg_ctx* ctx, sg_truth_tag_counts* out) {
  if (!ctx || !out) return SG_ERR_INVALID;
  if (int rc = truth_need_map(ctx, "sg_truth_tag_info")) return rc;
  if (!ctx->pass.have_bam) return ctx->fail(SG_ERR_INVALID, "sg_truth_tag_info: call sg_truth_bam first");
  const uint64_t* t = ctx->pass.bam_tags;
  *out = sg_truth_tag_counts{t[0], t[1], t[2], t[3], t[4], t[5], t[6], sg::kTruthMaxMd};
  return SG_OK;
}

int sg_truth_info(sg_ctx* ctx, uint64_t* records, uint64_t* unmapped) {
  if (!ctx) return SG_ERR_INVALID;
  if (int rc = truth_need_map(ctx, "sg_truth_info")) return rc;
  if (!ctx->pass.have_bam) return ctx->fail(SG_ERR_INVALID, "sg_truth_info: call sg_truth_bam first");
  if (records) *records = ctx->pass.bam_records;
  if (unmapped) *unmapped = ctx->pass.bam_unmapped;
  return SG_OK;
}

// ------------------------------------------------------------------------------------------------
// reference ingest + haplotype assembly on the device (kernels: sg_haplotypes.hip)
// ------------------------------------------------------------------------------------------------
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
  if (!ctx->ref_raw.p || offset + bytes > ctx->ref_raw_bytes) return ctx->fail(SG_ERR_INVALID, "sg_reference_chunk: range outside sg_reference_begin's size");
  SG_HIP(hipSetDevice(ctx->device));
  if (bytes) SG_HIP(hipMemcpyAsync((uint8_t*)ctx->ref_raw.p + offset, host, bytes, hipMemcpyHostToDevice, ctx->stream));
  return SG_OK;
}

int sg_sync(sg_ctx* ctx) {
  if (!ctx) return SG_ERR_INVALID;
  SG_HIP(hipSetDevice(ctx->device));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

int sg_reference_scan(sg_ctx* ctx, uint64_t* header_offsets, uint32_t cap, uint32_t* n_found, uint32_t* flags) {
  if (!ctx || !n_found || (cap && !header_offsets)) return SG_ERR_INVALID;
  if (!ctx->ref_raw.p) return ctx->fail(SG_ERR_INVALID, "sg_reference_scan: call sg_reference_begin first");
  SG_HIP(hipSetDevice(ctx->device));
  SG_ENSURE(ctx->hap_work, (size_t)cap * 8 + 64);
  uint32_t* counters = (uint32_t*)((uint8_t*)ctx->hap_work.p + (size_t)cap * 8);
  SG_HIP(hipMemsetAsync(counters, 0, 8, ctx->stream));
  sg::launch_ref_scan(ctx->ref_raw.as<uint8_t>(), ctx->ref_raw_bytes, ctx->hap_work.as<uint64_t>(), cap, counters, counters + 1, ctx->stream);
  SG_HIP(hipGetLastError());
  uint32_t host_c[2] = {0, 0};
  SG_HIP(hipMemcpyAsync(host_c, counters, 8, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  *n_found = host_c[0];
  if (flags) *flags = host_c[1];
  const uint32_t n = host_c[0] < cap ? host_c[0] : cap;
  if (n) SG_HIP(hipMemcpy(header_offsets, ctx->hap_work.p, (size_t)n * 8, hipMemcpyDeviceToHost));
  return SG_OK;
}

int sg_reference_commit(sg_ctx* ctx, const sg_contig* contigs, uint32_t n_contigs) {
  if (!ctx || (n_contigs && !contigs)) return SG_ERR_INVALID;
  if (!ctx->ref_raw.p) return ctx->fail(SG_ERR_INVALID, "sg_reference_commit: call sg_reference_begin first");
  SG_HIP(hipSetDevice(ctx->device));
  std::vector<sg::DevContig> tab(n_contigs);
  uint64_t code_off = 0, blocks = 0;
  for (uint32_t c = 0; c < n_contigs; c++) {
    const sg_contig& k = contigs[c];
    if (k.length && (k.line_bases == 0 || k.line_width < k.line_bases))
      return ctx->fail(SG_ERR_INVALID, "sg_reference_commit: contig " + std::to_string(c) + " has an impossible line shape");
    if (k.length > 0xFFFFFFF0ull)   // (the ingest kernel's line / column arithmetic is 32-bit; the host says the same, fasta.cpp)
      return ctx->fail(SG_ERR_UNSUPPORTED, "sg_reference_commit: contig " + std::to_string(c) + " is longer than 4 Gbp");
    const uint64_t lines = k.length ? (k.length - 1) / k.line_bases : 0;  // line breaks inside the contig
    if (k.raw_offset + k.length + lines * (k.line_width - k.line_bases) > ctx->ref_raw_bytes)
      return ctx->fail(SG_ERR_INVALID, "sg_reference_commit: contig " + std::to_string(c) + " runs past the end of the file");
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
  SG_HIP(hipGetLastError());
  uint32_t host_flags = 0;
  SG_HIP(hipMemcpyAsync(&host_flags, flags, 4, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
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
  if (ctx->ref_contigs.empty() && n_pieces) return ctx->fail(SG_ERR_INVALID, "sg_build_haplotypes: call sg_reference_commit first");
  SG_HIP(hipSetDevice(ctx->device));
  sg_ctx::ChainLayout L = chain_layout(n_chains, lens);
  // absolute offsets, long pieces split so that every workgroup moves <= 64 KB; coverage is checked
  // by summing the piece lengths per chain after a bounds check of each piece
  const uint32_t kSplit = 1u << 16;
  std::vector<sg::DevPiece> dp;
  dp.reserve((size_t)n_pieces + L.total / kSplit + 16);
  std::vector<uint64_t> covered((size_t)n_chains, 0);
  for (uint64_t i = 0; i < n_pieces; i++) {
    const sg_hap_piece& p = pieces[i];
    if ((int64_t)p.chain >= n_chains || p.dst + p.len > lens[p.chain])
      return ctx->fail(SG_ERR_INVALID, "sg_build_haplotypes: piece " + std::to_string(i) + " falls outside its chain");
    uint64_t src;
    if (p.kind == 0) {
      if (p.contig >= ctx->ref_contigs.size() || p.src + p.len > ctx->ref_contigs[p.contig].length)
        return ctx->fail(SG_ERR_INVALID, "sg_build_haplotypes: piece " + std::to_string(i) + " falls outside its contig");
      src = ctx->ref_contigs[p.contig].code_off + p.src;
    } else {
      if (p.src + p.len > n_literal_bytes)
        return ctx->fail(SG_ERR_INVALID, "sg_build_haplotypes: piece " + std::to_string(i) + " falls outside the literal bytes");
      src = p.src;
    }
    covered[p.chain] += p.len;
    for (uint32_t o = 0; o < p.len; o += kSplit)
      dp.push_back(sg::DevPiece{L.off[p.chain] + p.dst + o, src + o, std::min<uint32_t>(kSplit, p.len - o), p.kind ? 1u : 0u});
  }
  for (int c = 0; c < n_chains; c++)
    if (covered[c] != lens[c]) return ctx->fail(SG_ERR_INVALID, "sg_build_haplotypes: the pieces of chain " + std::to_string(c) + " do not add up to its length");
  std::vector<sg::DevPatch> pt((size_t)n_patches);
  for (uint64_t i = 0; i < n_patches; i++) {
    const sg_hap_patch& q = patches[i];
    if ((int64_t)q.chain >= n_chains || q.dst >= lens[q.chain])
      return ctx->fail(SG_ERR_INVALID, "sg_build_haplotypes: patch " + std::to_string(i) + " falls outside its chain");
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
  if (!ctx->have_haps) return ctx->fail(SG_ERR_INVALID, "sg_haplotype_codes: no haplotypes on the device");
  SG_HIP(hipSetDevice(ctx->device));
  if (chain >= ctx->hap.len.size()) return ctx->fail(SG_ERR_INVALID, "sg_haplotype_codes: chain index out of range");
  if (offset + n > ctx->hap.len[chain]) return ctx->fail(SG_ERR_INVALID, "sg_haplotype_codes: range past the end of the chain");
  if (n) SG_HIP(hipMemcpy(codes_out, ctx->B.chains + ctx->hap.off[chain] + offset, n, hipMemcpyDeviceToHost));
  return SG_OK;
}

// ------------------------------------------------------------------------------------------------
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

// ------------------------------------------------------------------------------------------------
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

// ------------------------------------------------------------------------------------------------
// header + emit kernels of the current batch into the context's output buffers
static int launch_text(sg_ctx* ctx, bool prof) {
  sg::DevBatch& B = ctx->B;
  hipStream_t s = ctx->stream;
  B.out[0] = ctx->out1.as<uint8_t>();
  B.out[1] = ctx->out2.as<uint8_t>();
  B.out_cap[0] = ctx->out1.cap;
  B.out_cap[1] = ctx->out2.cap;
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
  if (prof) SG_HIP(hipEventRecord(ctx->evs[5], s));  // after the (first-pass) output allocation
  sg::launch_header(ctx->P, B, s);
  ctx->pass.emit_path = sg::emit_path(ctx->P, B, false);
  sg::launch_emit(ctx->P, B, s, false, prof ? ctx->evs[7] : nullptr);
  if (prof) SG_HIP(hipEventRecord(ctx->evs[6], s));
  return SG_OK;
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
  if (!B.n_windows) SG_HIP(hipMemsetAsync(B.totals, 0, sg::kTotalsBytes, s));  // (otherwise plan_kernel clears them)
  if (prof) SG_HIP(hipEventRecord(ctx->evs[0], s));
  sg::launch_plan(ctx->P, B, s);
  if (prof) SG_HIP(hipEventRecord(ctx->evs[1], s));
  sg::launch_namebase(B, s);
  if (prof) SG_HIP(hipEventRecord(ctx->evs[2], s));
  sg::launch_indel(ctx->P, B, s);
  if (prof) SG_HIP(hipEventRecord(ctx->evs[3], s));
  sg::launch_scan(B, s);
  if (prof) SG_HIP(hipEventRecord(ctx->evs[4], s));
  SG_HIP(hipGetLastError());
  if (!ctx->out1.p && !ctx->out2.p && !ctx->gz1.p && !ctx->gz2.p && !ctx->spare.empty()) {
    // a released output set (sg_release_outputs): its buffers become this pass's
    sg_outputs* o = ctx->spare.back();
    std::swap(ctx->out1, o->text[0]); std::swap(ctx->out2, o->text[1]);
    std::swap(ctx->gz1, o->gz[0]); std::swap(ctx->gz2, o->gz[1]);
  }
  // The FASTQ size is only known now, on the device.  When the context already holds output buffers (every pass
  // but a context's first), the emit kernels are launched at once: they compare the size with the buffers' capacity
  // themselves and do nothing but raise a flag when it does not fit (settle_pass then grows the buffers and launches
  // them again).  Otherwise two u64 are read back first -- one stream sync in the middle of the pass.
  Q.speculative = ctx->out1.p != nullptr && (!B.paired || ctx->out2.p != nullptr) && getenv("SG_NO_SPECULATION") == nullptr;
  if (!Q.speculative) {
    sg::launch_mail(B.totals, ctx->mail, s);
    SG_HIP(hipStreamSynchronize(s));
    memcpy(Q.host_totals, ctx->mail, 4 * 8);
    if (Q.host_totals[3] & 1) return ctx->fail(SG_ERR_OVERFLOW, "sg_sample: a read drew more than SG_MAX_EVENTS sequencing indels");
    SG_ENSURE(ctx->out1, Q.host_totals[0] + 64);
    if (B.paired) SG_ENSURE(ctx->out2, Q.host_totals[1] + 64);
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
  if (Q.host_totals[3] & 1) {
    restart_pass(ctx);
    return ctx->fail(SG_ERR_OVERFLOW, "sg_sample: a read drew more than SG_MAX_EVENTS sequencing indels");
  }
  if (Q.speculative && (Q.host_flags[0] & 4)) {  // the buffers were too small: grow, emit again
    SG_ENSURE(ctx->out1, Q.host_totals[0] + 64);
    if (B.paired) SG_ENSURE(ctx->out2, Q.host_totals[1] + 64);
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
    for (int i = 0; i < 4; i++) SG_HIP(hipEventElapsedTime(&ctx->last_ms[i], ctx->evs[i], ctx->evs[i + 1]));
    SG_HIP(hipEventElapsedTime(&ctx->last_ms[SG_K_EMIT], ctx->evs[5], ctx->evs[7]));
    SG_HIP(hipEventElapsedTime(&ctx->last_ms[SG_K_EMIT_SLOW], ctx->evs[7], ctx->evs[6]));
  }
  Q.stage = sg_ctx::Pass::Settled;
  return SG_OK;
}

extern "C++" int sg_pass_need(sg_ctx* ctx, const char* who, sg_ctx::Pass::Stage at_least, bool settle_now) {   // (declared in sg_api.h, not part of the ABI)
  using Pass = sg_ctx::Pass;
  if (!ctx) return SG_ERR_INVALID;
  static const char* const step[] = {"", "sg_plan", "sg_sample", "sg_result"};
  const Pass::Stage need = settle_now && at_least == Pass::Settled ? Pass::Queued : at_least;   // settling asks no more
  if (ctx->pass.stage < need || (at_least == Pass::Planned && !ctx->pass.rows_current))
    return ctx->fail(SG_ERR_INVALID, std::string(who) + ": call " + step[need] + " first");
  SG_HIP(hipSetDevice(ctx->device));
  return at_least == Pass::Settled && ctx->pass.stage == Pass::Queued ? settle_pass(ctx) : SG_OK;
}

int sg_emit_variant(sg_ctx* ctx) {
  if (!ctx || !ctx->have_profile) return -1;
  return sg::emit_variant(ctx->P);
}

int sg_emit_path(const sg_ctx* ctx, sg_emit_path_info* info) {
  // (a const context: no message to leave, no device to select, so the stage is tested here and not by sg_pass_need)
  if (!ctx || !info || ctx->pass.stage != sg_ctx::Pass::Settled) return SG_ERR_INVALID;
  const sg::EmitPath& path = ctx->pass.emit_path;
  info->main_kernel = path.main_kernel;
  info->slow_rows_lds = path.slow_rows_lds;
  info->lds_bytes = path.lds_bytes;
  info->clean_cap = path.clean_cap;
  return SG_OK;
}

int sg_emit_info(sg_ctx* ctx, uint64_t* queued_items, int* requeued) {
  if (int rc = sg_pass_need(ctx, "sg_emit_info", sg_ctx::Pass::Settled)) return rc;
  if (queued_items) *queued_items = ctx->pass.slow_items;
  if (requeued) *requeued = ctx->pass.slow_overflow ? 1 : 0;
  return SG_OK;
}

int sg_sample(sg_ctx* ctx) {
  if (int rc = sg_pass_need(ctx, "sg_sample", sg_ctx::Pass::Planned)) return rc;
  return run_pass(ctx);
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
  const uint64_t* totals = ctx->pass.host_totals;
  if (host_r1 && totals[0])
    SG_HIP(hipMemcpyAsync(host_r1, ctx->out1.p, totals[0], hipMemcpyDeviceToHost, ctx->stream));
  if (host_r2 && ctx->B.paired && totals[1])
    SG_HIP(hipMemcpyAsync(host_r2, ctx->out2.p, totals[1], hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

int sg_fetch_range(sg_ctx* ctx, int mate, uint64_t offset, uint64_t bytes, char* host_dst) {
  if (!ctx || (bytes && !host_dst) || mate < 0 || mate > 1) return SG_ERR_INVALID;
  if (int rc = sg_pass_need(ctx, "sg_fetch_range", sg_ctx::Pass::Settled, true)) return rc;
  if (mate == 1 && !ctx->B.paired) return ctx->fail(SG_ERR_INVALID, "sg_fetch_range: single-end batch has no mate 2");
  if (offset + bytes > ctx->pass.host_totals[mate]) return ctx->fail(SG_ERR_INVALID, "sg_fetch_range: range past the end of the FASTQ text");
  if (!bytes) return SG_OK;
  const char* src = (const char*)(mate ? ctx->out2.p : ctx->out1.p) + offset;
  SG_HIP(hipMemcpyAsync(host_dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}

int sg_host_alloc(sg_ctx* ctx, uint64_t bytes, void** host_ptr) {
  if (!ctx || !host_ptr) return SG_ERR_INVALID;
  SG_HIP(hipSetDevice(ctx->device));
  const uint64_t want = bytes ? bytes : 1;
  if ((*host_ptr = host_cache().take(want)) != nullptr) return SG_OK;
  SG_HIP(hipHostMalloc(host_ptr, want, hipHostMallocDefault));
  host_cache().note(*host_ptr, want);
  return SG_OK;
}

void sg_release_cached_memory(void) {
  block_cache().trim();
  host_cache().trim();
}

int sg_host_free(sg_ctx* ctx, void* host_ptr) {
  if (!ctx) return SG_ERR_INVALID;
  if (!host_ptr) return SG_OK;
  // hipHostFree waits for the device; a buffer that goes to the cache instead may be handed out again at once, so copies
  // still reading or writing it (sg_reference_chunk's asynchronous uploads on an error path) must have ended
  SG_HIP(hipSetDevice(ctx->device));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  if (!host_cache().give(host_ptr)) SG_HIP(hipHostFree(host_ptr));
  return SG_OK;
}

int sg_device_output(sg_ctx* ctx, void** dev_r1, void** dev_r2) {
  // (settled here: a pass queued without its size may still move to larger buffers)
  if (int rc = sg_pass_need(ctx, "sg_device_output", sg_ctx::Pass::Settled, true)) return rc;
  if (dev_r1) *dev_r1 = ctx->out1.p;
  if (dev_r2) *dev_r2 = ctx->B.paired ? ctx->out2.p : nullptr;
  return SG_OK;
}

}  // extern "C"
