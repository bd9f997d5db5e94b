// host/fastq_sink.h -- the FASTQ files of a stem (<output>/<stem>_1.fq + _2.fq, or <stem>.fq: Genome.cpp:857-866) and
// their asynchronous drain, one owner.  The text leaves the engine context as a detached output set and is drained by a
// worker thread (D2H on the set's own stream + the file writers) while the calling thread plans and samples the next
// piece.  One drain at a time: the pinned buffers, the files and their order belong to it.
#pragma once
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <string>
#include <thread>

#include "engine.h"
#include "simulate.h"

namespace simu {

struct PumpResult {
  int status = 0;             // of the fetch that failed (nothing is fetched or posted after it), else 0
  bool short_write = false;   // a writer's fwrite came back short
  double t_fetch = 0, t_write = 0;   // fetch time not hidden behind the writers; the slower writer's time in fwrite
};

// The chunk pump (the reference's SeqWriter::write, lib/seqwriter/SeqWriter.cpp:41-54): total[m] bytes of mate m go
// from fetch(m, offset, n, buffer) -> status to file m in chunks, double buffered per mate (buf[2 * m], buf[2 * m + 1],
// `chunk` bytes each), while one writer thread per file appends the previous chunk (an fwrite into the page cache runs at
// ~10 GB/s per thread, a fifth of the D2H rate, so the two files are written concurrently).  Mate 1 and mate 2 text are
// independent byte streams into their own files, so pair order is kept.  A null file takes nothing.
template <class Fetch>
PumpResult pump_chunks(Fetch fetch, const uint64_t total[2], int mates, FILE* f1, FILE* f2, void* const buf[4], size_t chunk) {
  using Clock = std::chrono::steady_clock;
  auto since = [](Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); };
  struct Writer {
    std::mutex mu;
    std::condition_variable cv;
    FILE* f = nullptr;
    const char* p = nullptr;
    size_t n = 0;
    bool have = false, stop = false, failed = false;
    double t_write = 0;
    std::thread th;
    void run() {
      for (;;) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&]() { return have || stop; });
        if (!have && stop) return;
        FILE* jf = f; const char* jp = p; const size_t jn = n;
        lk.unlock();
        auto tw = Clock::now();
        if (jf && jn && fwrite(jp, 1, jn, jf) != jn) failed = true;
        t_write += std::chrono::duration<double>(Clock::now() - tw).count();
        lk.lock();
        have = false;
        cv.notify_all();
      }
    }
    void wait_idle() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&]() { return !have; }); }
    void post(FILE* jf, const char* jp, size_t jn) {
      std::unique_lock<std::mutex> lk(mu);
      f = jf; p = jp; n = jn; have = true;
      cv.notify_all();
    }
    void finish() {
      { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&]() { return !have; }); stop = true; cv.notify_all(); }
      th.join();
    }
  };
  Writer w[2];
  for (int m = 0; m < mates; m++) w[m].th = std::thread([&w, m]() { w[m].run(); });
  auto t0 = Clock::now();
  PumpResult r;
  int cur[2] = {0, 0};
  for (uint64_t off = 0; (off < total[0] || (mates == 2 && off < total[1])) && r.status == 0; off += chunk) {
    for (int m = 0; m < mates && r.status == 0; m++) {
      if (off >= total[m]) continue;
      const size_t n = (size_t)std::min<uint64_t>(chunk, total[m] - off);
      void* b = buf[2 * m + cur[m]];
      // this buffer's previous chunk was posted two rounds ago; the copy overlaps both writers' fwrite
      r.status = fetch(m, off, n, b);
      w[m].wait_idle();  // the mate's other buffer is free again
      if (r.status == 0) w[m].post(m ? f2 : f1, (const char*)b, n);
      cur[m] ^= 1;
    }
  }
  for (int m = 0; m < mates; m++) { w[m].finish(); r.t_write = std::max(r.t_write, w[m].t_write); r.short_write |= w[m].failed; }
  const double wall = since(t0);
  r.t_fetch = wall > r.t_write ? wall - r.t_write : 0;
  return r;
}

class FastqSink {
 public:
  FastqSink(Engine& eng, const simu_options& opt, simu_stats& st) : eng(eng), opt(opt), st(st) {}
  ~FastqSink();   // the whole order: join the drain, release its handle, free the pinned buffers, close the files
  FastqSink(const FastqSink&) = delete;
  FastqSink& operator=(const FastqSink&) = delete;
  // a stem starts (the previous one's files close): the files under write_files only, .gz under gzip, then the shard suffix
  void open(const std::string& dir, const std::string& stem, bool paired);
  void submit(bool compressed);   // the pass just sampled (its members when compressed): waits for the drain in flight, starts this one
  void wait();                    // joins the drain in flight (if any), books its times, returns its buffers to the engine
  void close();                   // after wait(): the BGZF end-of-file blocks (unless no_eof_block), the files

 private:
  void drain(sg_outputs* h, bool compressed);
  static constexpr size_t kChunk = 64u << 20;
  Engine& eng;
  const simu_options& opt;
  simu_stats& st;
  FILE *f1 = nullptr, *f2 = nullptr;
  int mates = 1;
  void* pinned[4] = {nullptr, nullptr, nullptr, nullptr};
  struct Pending {
    sg_outputs* handle = nullptr;
    std::thread th;
    bool active = false;
    std::string err;
    double t_fetch = 0, t_write = 0;
  } pending;
};

}  // namespace simu
