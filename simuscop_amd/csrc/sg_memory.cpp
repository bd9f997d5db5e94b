// sg_memory.cpp -- the memory that outlives a context: device blocks and pinned staging buffers stay with the process and
// serve the next request of their size.  DevBuf (sg_api.h) takes its blocks from here (ensure, release, sg_grow_keep).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <mutex>

#include "sg_api.h"

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
  // (a third of an MI355X: 96 GB -- a whole-genome run's ~60 GB of blocks fit; what other allocators and processes may need stays free)
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

// a device buffer grown with what it holds kept (the window arrays live across chunks, a stream's carried record and
// an evaluation's rows across calls); declared in sg_api.h
int sg_grow_keep(sg_ctx* ctx, DevBuf& buf, size_t keep_bytes, size_t want_bytes) {
  if (want_bytes <= buf.cap) return SG_OK;
  DevBuf bigger;
  SG_ENSURE(bigger, want_bytes + want_bytes / 2);
  if (keep_bytes) SG_HIP(hipMemcpyAsync(bigger.p, buf.p, keep_bytes, hipMemcpyDeviceToDevice, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  buf = std::move(bigger);
  return SG_OK;
}

extern "C" {

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

}  // extern "C"
