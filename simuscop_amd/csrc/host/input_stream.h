// host/input_stream.h -- how a file gets to the GPU: pinned batches cut at a boundary (BatchReader) and the loop that feeds
// one batch while a thread reads the next (stream_batches).  seqToProfile's SAM text, BAM members and VCF (host/train.cpp)
// and truthEval's two BAM files (host/eval.cpp) all come in through here.
#pragma once
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <thread>

#include "../../../include/simuscop_amd.h"
#include "common.h"
#include "reader_pool.h"

namespace simu {

constexpr uint64_t kChunk = 64ull << 20;      // bytes of text per batch
constexpr uint64_t kBamBatch = 16ull << 20;   // compressed bytes per batch of a BAM (about 3 to 4 times as many inflated)
constexpr uint64_t kVcfBatch = 8ull << 20;    // ... of a BGZF VCF (text: several times more per byte than BAM records)
constexpr uint32_t kMaxMember = 65536;        // BSIZE is 16 bits

inline int leave_open(FILE*) { return 0; }    // standard input is not closed

// Pinned batches of a file, read ahead while the device works on the batch before: a regular file by a pool of threads
// (pread of 4 MB slices: one reader took text at 10 GB/s, a fifth of what the link and the kernels take), a pipe or
// standard input by fread.  A batch is the longest prefix of (what the batch before left + what fits `cap`) that ends at
// a boundary of the reader's rule; the rest is carried to the next batch.
struct BatchReader {
  enum Cut {
    Lines,      // behind the last line break; at the end of the file everything (a batch without a line break: an error)
    Anywhere,   // wherever the buffer ends (the plain VCF: the device carries the partial line)
    Members     // behind the last whole BGZF member (SAMv1 section 4.1; a buffer holds at least one: cap > kMaxMember);
                // a member cut by the end of the file is an error
  };
  struct Pinned {
    sg_ctx* ctx;
    char* p = nullptr;
    ~Pinned() { if (p) sg_host_free(ctx, p); }
  };
  sg_ctx* ctx;
  std::string what;                                 // the file's name in messages
  const Cut cut;
  const uint64_t cap;                               // bytes a buffer is topped up to
  std::unique_ptr<FILE, int (*)(FILE*)> fp;
  int fd = -1;                                      // >= 0: a regular file, read with pread from `pos`
  uint64_t pos = 0, size = 0, file_off = 0;         // file_off: where the next batch starts
  std::unique_ptr<ReaderPool> pool;
  Pinned buf[2];
  uint64_t len[2] = {0, 0};
  std::string carry;                                // the bytes behind a batch's last boundary
  std::string last28;                               // the last 28 bytes read (the EOF member, if a BGZF file has one)
  bool eof = false, primed = false, any = false;

  static uint64_t usual(Cut c) { return c == Members ? kBamBatch + kMaxMember : kChunk; }
  // `f` is closed with `close_fp` (fclose, pclose, leave_open)
  BatchReader(sg_ctx* c, FILE* f, int (*close_fp)(FILE*), const std::string& name, int threads, Cut rule, uint64_t capacity = 0)
      : ctx(c), what(name), cut(rule), cap(capacity ? capacity : usual(rule)), fp(f, close_fp), buf{{c}, {c}} {
    struct stat sb;
    if (f != stdin && fstat(fileno(f), &sb) == 0 && S_ISREG(sb.st_mode)) {
      fd = fileno(f);
      size = (uint64_t)sb.st_size;
      pool.reset(new ReaderPool(std::min(16, std::max(1, threads))));
    }
    for (Pinned& b : buf) {
      void* p = nullptr;
      if (sg_host_alloc(ctx, cap + 16, &p) != SG_OK) throw Error(std::string("GPU engine error in sg_host_alloc: ") + sg_last_error(ctx));
      b.p = (char*)p;
    }
  }
  // a path, or `-` for standard input; `kind` names the file in the open error
  BatchReader(sg_ctx* c, const std::string& path, const char* kind, int threads, Cut rule, uint64_t capacity = 0)
      : BatchReader(c, open(path, kind), path == "-" ? leave_open : fclose, path, threads, rule, capacity) {}
  static FILE* open(const std::string& path, const char* kind) {
    if (path == "-") return stdin;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) throw Error(std::string("cannot open ") + kind + " file " + path, -1);
    return f;
  }

  bool regular() const { return fd >= 0; }
  const char* data(int i) const { return buf[i].p; }
  void rewind() { pos = 0; file_off = 0; carry.clear(); last28.clear(); eof = primed = false; }
  // the BGZF EOF member: at the end of what has been read so far, or (a regular file) at the end of the file
  bool eof_marker() const { return is_eof_member(last28.data(), last28.size()); }
  bool peek_eof_marker() const {
    char tail[28];
    return fd >= 0 && size >= 28 && pread(fd, tail, 28, (off_t)(size - 28)) == 28 && is_eof_member(tail, 28);
  }
  static bool is_eof_member(const char* p, size_t n) {
    uint8_t e[28];
    sg_bgzf_eof(e);
    return n == 28 && memcmp(p, e, 28) == 0;
  }
  // The first batch, filled on first use: a caller may look at it before stream_batches feeds it.
  bool first() {
    if (!primed) { primed = true; any = fill(0); }
    return any;
  }
  // fills buf[i] with the next batch; false when nothing is left
  bool fill(int i) {
    if (eof && carry.empty()) { len[i] = 0; return false; }
    char* const b = buf[i].p;
    uint64_t have = carry.size();
    const uint64_t carried = have;
    memcpy(b, carry.data(), have);
    if (fd >= 0) {
      const uint64_t n = std::min<uint64_t>(cap - have, size - pos);
      if (n) parallel_pread(*pool, fd, (uint8_t*)b + have, pos, n);
      have += n;
      pos += n;
      if (pos >= size) eof = true;
    } else {
      while (!eof && have < cap) {
        const size_t got = fread(b + have, 1, cap - have, fp.get());
        if (got == 0) { eof = true; break; }
        have += got;
      }
    }
    last28.append(b + have - std::min<uint64_t>(have - carried, 28), std::min<uint64_t>(have - carried, 28));
    if (last28.size() > 28) last28.erase(0, last28.size() - 28);
    uint64_t keep = have;
    if (cut == Lines && !eof) {
      while (keep > 0 && b[keep - 1] != '\n') keep--;
      if (keep == 0) throw Error("a line of the SAM text is longer than 64 MB");
    } else if (cut == Members) {
      uint64_t n_members = 0;
      if (sg_bgzf_members(b, have, nullptr, nullptr, nullptr, ~0ull, &n_members, &keep) != SG_OK)
        throw Error("Error: corrupt BGZF member at file offset " + std::to_string(file_off + keep) + " of " + what);
    }
    carry.assign(b + keep, have - keep);
    if (cut == Members && eof && !carry.empty())
      throw Error("Error: truncated BGZF member at file offset " + std::to_string(file_off + keep) + " of " + what);
    len[i] = keep;
    file_off += keep;
    return keep > 0;
  }
};

// The read-ahead loop: feed(bytes, n) for every batch in file order while a thread fills the other buffer.  The thread is
// joined before anything leaves the loop; an error that feed throws wins over the reader's.  go_on() is asked after each
// batch and ends the loop: the batch that was read meanwhile is dropped (the training cap, at which the reference leaves
// its loop and the rest of the input is not read).
template <class Feed, class GoOn>
void stream_batches(BatchReader& rd, Feed feed, GoOn go_on) {
  int cur = 0;
  bool more = rd.first();
  while (more) {
    bool next = false;
    std::string reader_error;
    std::thread reader([&]() { try { next = rd.fill(cur ^ 1); } catch (const std::exception& e) { reader_error = e.what(); } });
    struct Joined { std::thread& t; ~Joined() { t.join(); } };
    { Joined joined{reader}; feed(rd.data(cur), rd.len[cur]); }
    if (!reader_error.empty()) throw Error(reader_error);
    cur ^= 1;
    more = next && go_on();
  }
}
template <class Feed>
void stream_batches(BatchReader& rd, Feed feed) { stream_batches(rd, feed, []() { return true; }); }

}  // namespace simu
