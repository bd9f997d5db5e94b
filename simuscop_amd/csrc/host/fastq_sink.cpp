// host/fastq_sink.cpp -- see fastq_sink.h
#include "fastq_sink.h"

namespace simu {

FastqSink::~FastqSink() {
  if (pending.active && pending.th.joinable()) pending.th.join();
  if (pending.active && pending.handle && eng.ctx) sg_release_outputs(eng.ctx, pending.handle);
  for (void* b : pinned)
    if (b && eng.ctx) sg_host_free(eng.ctx, b);
  close();
}

void FastqSink::open(const std::string& dir, const std::string& stem, bool paired) {
  close();
  mates = paired ? 2 : 1;
  if (!opt.write_files) return;
  const std::string suffix = (opt.gzip ? ".gz" : "") + simu_shard_suffix(opt);
  if (paired) {
    std::string a = dir + "/" + stem + "_1.fq" + suffix, b = dir + "/" + stem + "_2.fq" + suffix;
    f1 = fopen(a.c_str(), "wb");
    if (!f1) throw Error("Error: can not open fastq file to save results:\n" + a, -1);
    f2 = fopen(b.c_str(), "wb");
    if (!f2) throw Error("Error: can not open fastq file to save results:\n" + b, -1);
  } else {
    std::string a = dir + "/" + stem + ".fq" + suffix;
    f1 = fopen(a.c_str(), "wb");
    if (!f1) throw Error("Error: can not open fastq file to save results:\n" + a, -1);
  }
}

void FastqSink::close() {
  if (opt.gzip && !opt.no_eof_block) {  // BGZF end-of-file marker
    uint8_t eof[28];
    sg_bgzf_eof(eof);
    if (f1) fwrite(eof, 1, 28, f1);
    if (f2) fwrite(eof, 1, 28, f2);
  }
  if (f1) fclose(f1);
  if (f2) fclose(f2);
  f1 = f2 = nullptr;
}

void FastqSink::submit(bool compressed) {
  wait();
  for (int i = 0; i < 2 * mates; i++)   // context calls stay on this thread
    if (!pinned[i]) eng.check(sg_host_alloc(eng.ctx, kChunk, &pinned[i]), "sg_host_alloc");
  sg_outputs* h = nullptr;
  eng.check(sg_detach_outputs(eng.ctx, &h), "sg_detach_outputs");
  pending.handle = h;
  pending.active = true;
  pending.err.clear();
  pending.t_fetch = pending.t_write = 0;
  pending.th = std::thread([this, h, compressed]() {
    try { drain(h, compressed); }
    catch (const std::exception& e) { pending.err = e.what(); }
  });
}

void FastqSink::wait() {
  if (!pending.active) return;
  pending.th.join();
  pending.active = false;
  st.t_fetch += pending.t_fetch;
  st.t_write += pending.t_write;
  eng.check(sg_release_outputs(eng.ctx, pending.handle), "sg_release_outputs");
  pending.handle = nullptr;
  if (!pending.err.empty()) throw Error(pending.err, -1);
}

// on the worker: D2H in pinned 64 MB chunks into the stem's files (into no file without write_files: opt.fetch)
void FastqSink::drain(sg_outputs* h, bool compressed) {
  uint64_t tb[2], gb[2];
  sg_outputs_sizes(h, tb, gb);
  const PumpResult r = pump_chunks([&](int m, uint64_t off, size_t n, void* buf) { return sg_outputs_fetch(h, m, compressed ? 1 : 0, off, n, buf); },
                                   compressed ? gb : tb, mates, f1, f2, pinned, kChunk);
  if (r.status != SG_OK) throw Error(std::string("GPU engine error in sg_outputs_fetch: ") + sg_outputs_last_error(h));
  pending.t_write = r.t_write;
  pending.t_fetch = r.t_fetch;
  if (r.short_write) throw Error("Error: short write to fastq file", -1);
}

}  // namespace simu
