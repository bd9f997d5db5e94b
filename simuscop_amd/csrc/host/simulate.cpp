// host/simulate.cpp -- the `simuReads <config>` driver (src/simuReads.cpp:24-87 +
// Genome::yieldReads, lib/genome/Genome.cpp:827-960) on top of the C ABI.
//
// Order of work per population:
//   pass 1  for every chromosome: build haplotype chains once (host), upload, GC% per window on the
//           GPU (sg_gc_percent), GC-bias weights and weighted lengths on the host in fp64 -- the read
//           apportioning truncates fp64 products, so it stays where the reference computes it;
//   counts  chromosome / segment / window read counts (Genome::setReadCounts, Segment::setReadCount);
//   pass 2  one GPU batch per chromosome: sg_plan -> sg_sample -> sg_fetch -> FASTQ files.
// The planner is read_plan.h, the FASTQ files and their drain fastq_sink.h, the truth outputs truth_outputs.h.
#include "simulate.h"

#include <sys/stat.h>

#include <chrono>
#include <thread>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>

#include "../../../include/simuscop_amd.h"
#include "fastq_sink.h"
#include "genome.h"
#include "read_plan.h"
#include "truth_outputs.h"

namespace simu {
namespace {

using Clock = std::chrono::steady_clock;
inline double since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

struct Driver {
  Config cfg;
  Genome genome{cfg};
  Profile prof;
  Engine eng;
  simu_options opt;
  simu_stats st{};
  void log(const std::string& s) { if (!opt.quiet) std::cerr << s; }
  // The contigs as the truth outputs number them (made by open(), once the inputs are loaded), and the truth outputs of
  // a stem: one lifecycle for all of them (truth_outputs.h).  Their files close with them on every path.
  ContigTable contigs;
  std::unique_ptr<TruthOutputs> truth;
  ReadPlan plan{cfg, genome, prof, eng, opt, st, contigs};
  FastqSink fastq{eng, opt, st};
  std::string out_dir;

  // the whole shard as one engine batch (step-by-step sessions: bench.py keeps it resident)
  bool prepare_batch(const std::string& popu, const std::string& chr) {
    if (!plan.build_batch(popu, chr)) return false;
    truth->begin();   // (a session has no stems: its caller adds, reads and resets the outputs itself)
    plan.plan_range(plan.cur.a0, plan.cur.a1);
    return true;
  }

  // a batch in pieces (ReadPlan::piece_end); each piece drains while the next one is sampled
  void run_batch(const std::string& popu, const std::string& chr) {
    if (!plan.build_batch(popu, chr)) return;
    for (size_t c0 = plan.cur.a0; c0 < plan.cur.a1;) {
      const size_t c1 = plan.piece_end(c0);
      run_piece(c0, c1);
      c0 = c1;
    }
  }

  void run_piece(size_t c0, size_t c1) {
    plan.plan_range(c0, c1);
    const ReadPlan::BatchPlan& cur = plan.cur;
    const bool paired = cur.paired;
    auto t0 = Clock::now();
    uint64_t n1 = 0, n2 = 0, nf = 0;
    const int reps = opt.repeat_sample > 1 ? opt.repeat_sample : 1;
    const bool trace = ReadPlan::trace_pieces();
    for (int r = 0; r < reps; r++) {
      auto ts = Clock::now();
      eng.check(sg_sample(eng.ctx), "sg_sample");
      const double d_sample = since(ts);
      eng.check(sg_result(eng.ctx, &n1, &n2, &nf), "sg_result");
      if (trace) fprintf(stderr, "[piece] %s %s segments %zu..%zu: sg_sample %.4f s, with sg_result %.4f s, %llu fragments\n", cur.popu.c_str(),
                         cur.chr.c_str(), c0, c1, d_sample, since(ts), (unsigned long long)nf);
      float ms[SG_K_COUNT];
      sg_kernel_times(eng.ctx, ms);
      for (int i = 0; i < SG_K_COUNT; i++) st.kernel_ms[i] += ms[i];
      uint64_t queued = 0;
      int requeued = 0;
      sg_emit_info(eng.ctx, &queued, &requeued);
      st.queued_items += queued;
      st.requeued_batches += (uint64_t)requeued;
      sg_emit_path_info path;
      if (sg_emit_path(eng.ctx, &path) == SG_OK) {
        st.emit_kernel = path.main_kernel;
        st.emit_slow_rows_lds = path.slow_rows_lds;
        st.emit_lds_bytes = path.lds_bytes;
        st.emit_clean_cap = path.clean_cap;
      }
    }
    st.t_sample += since(t0);
    st.fragments += nf;
    st.reads += paired ? 2 * nf : nf;
    st.fastq_bytes += n1 + n2;
    truth->piece();
    if (!(opt.write_files || opt.fetch)) return;
    bool compressed = false;
    if (opt.gzip) {
      auto tc = Clock::now();
      uint64_t g1 = 0, g2 = 0;
      eng.check(sg_compress(eng.ctx, &g1, &g2), "sg_compress");
      st.t_compress += since(tc);
      st.gz_bytes += g1 + g2;
      compressed = true;
    }
    fastq.submit(compressed);
  }

  Clock::time_point t_all;
  void open(const std::string& config_path) {
    t_all = Clock::now();
    auto t0 = Clock::now();
    const std::string refusal = simu_truth_refusal(opt, opt.shard_world > 1, true);
    if (!refusal.empty()) throw Error(refusal);
    cfg.load(config_path);
    const uint64_t seed = plan.seed = opt.has_seed ? opt.seed : (uint64_t)cfg.num["seed"];
    const int device = opt.device >= 0 ? opt.device : (int)cfg.num["device"];
    auto t1 = Clock::now();
    if (sg_create(&eng.ctx, device, seed) != SG_OK) throw Error(std::string("GPU engine error: ") + sg_last_error(nullptr));
    sg_set_profiling(eng.ctx, 1);
    st.t_engine = since(t1);
    genome.device_haps = !opt.host_haplotypes;
    genome.engine = eng.ctx;
    genome.shard_rank = opt.shard_rank;
    genome.fa.crlf_as_lf = opt.crlf_as_lf != 0;
    genome.fa.unique_contigs = opt.unique_contigs != 0;
    if (sg_set_strict_bases(eng.ctx, opt.strict_bases) != SG_OK) throw Error(std::string("GPU engine error: ") + sg_last_error(eng.ctx));
    genome.shard_world = opt.shard_world;
    genome.shard_contigs = opt.shard_contigs != 0 && opt.shard_world > 1;
    // The profile -- parsing its text (Profile::load / normParas / initCDFs), converting every CDF row into the engine's
    // integer tables (sg_profile_prepare: no device involved) -- on a worker thread while this one streams the reference
    // to the device: ~10 ms of work that every rank of a sharded run would otherwise repeat on its critical path.
    sg_profile_tables* tables = nullptr;
    std::string prof_err;
    int prof_exit = 1;
    const std::string prof_path = cfg.str["profile"];   // (the worker must not touch the config maps: operator[] inserts)
    const bool prof_paired = cfg.paired();
    const int prof_isize = (int)cfg.num["insertSize"];
    std::thread prof_thread([&]() {
      try {
        prof.train(prof_path, prof_paired, prof_isize);
        sg_profile_cdf view = prof.view();
        sg_profile_prepare(&view, &tables);
      } catch (const Error& e) { prof_err = e.what(); prof_exit = e.exit_code ? e.exit_code : 1; }
      catch (const std::exception& e) { prof_err = e.what(); }
    });
    struct Joiner { std::thread& t; sg_profile_tables*& T; ~Joiner() { if (t.joinable()) t.join(); if (T) sg_profile_tables_free(T); T = nullptr; } } joiner{prof_thread, tables};
    genome.load_data();
    st.t_reference = genome.t_reference;
    contigs.build(genome.fa);
    if (opt.truth_index)   // (before any file of a stem is opened)
      for (size_t r = 0; r < contigs.len.size(); r++)
        if (contigs.len[r] > (1ull << 29))
          throw Error("Error: --truth-index cannot index contig " + contigs.name[r] + ": it is longer than 2^29 bases, which a BAI cannot address", 1);
    truth.reset(new TruthOutputs(eng, opt, st, contigs, genome, cfg, prof));
    out_dir = (opt.output_dir && opt.output_dir[0]) ? opt.output_dir : cfg.str["output"];
    if (opt.write_files) {  // `mkdir -p` (src/simuReads.cpp:56-60)
      for (size_t i = 1; i <= out_dir.size(); i++)
        if (i == out_dir.size() || out_dir[i] == '/') mkdir(out_dir.substr(0, i).c_str(), 0755);
    }
    prof_thread.join();
    if (!prof_err.empty()) throw Error(prof_err, prof_exit);
    log("profile was loaded from file " + cfg.str["profile"] + "\n");
    eng.check(sg_load_prepared_profile(eng.ctx, tables), "sg_load_profile");
    genome.generate_segments();
    st.t_load = since(t0);
    st.planned_reads = (uint64_t)(genome.target_length() * cfg.num["coverage"] / prof.read_length);
  }

  void run(const std::string& config_path) {
    open(config_path);
    // Genome::yieldReads
    const std::vector<std::string>& popus = cfg.popu_names;
    const long reads = (long)st.planned_reads;
    if (cfg.verbose()) log("\nNumber of reads to sample: " + std::to_string(reads) + "\n");
    std::map<std::string, double> acn;  // Genome::calculateACNs, Genome.cpp:765-781
    for (auto& pp : genome.plans) {
      long sum = 0;
      for (auto& pc : pp.second)
        for (const Segment& g : pc.second.segs) sum += g.seq_size();
      acn[pp.first] = (double)sum / genome.genome_length();
    }
    log("\n*****Generating samples*****\n");
    const bool paired = cfg.paired();
    if (genome.mix_props.empty()) {
      fastq.open(out_dir, popus[0], paired);
      truth->open(out_dir, popus[0]);
      plan.set_read_counts(popus[0], reads);
      for (const std::string& chr : genome.chromosomes) run_batch(popus[0], chr);
    } else {
      for (const std::vector<float>& props : genome.mix_props) {
        double w_acn = 0;
        std::string stem;
        char buf[1000];
        for (size_t i = 0; i < popus.size(); i++) {
          w_acn += props[i] * acn[popus[i]];
          snprintf(buf, sizeof buf, i == 0 ? "%s_%.3f" : "+%s_%.3f", popus[i].c_str(), props[i]);
          stem += buf;
        }
        fastq.wait();  // the previous mixture's last batch still writes into the files about to be closed
        truth->close();
        fastq.open(out_dir, stem, paired);
        truth->open(out_dir, stem);
        for (size_t i = 0; i < popus.size(); i++) {
          const long popu_reads = (long)(reads * props[i] * acn[popus[i]] / w_acn);  // long*float is a float product (Genome.cpp:935)
          plan.set_read_counts(popus[i], popu_reads);
          for (const std::string& chr : genome.chromosomes) run_batch(popus[i], chr);
        }
      }
    }
    fastq.wait();
    truth->close();
    fastq.close();
    log("\nReads generation done!\n");
    st.t_total = since(t_all);
  }
};

}  // namespace
}  // namespace simu

extern "C" void simu_default_options(simu_options* o) {
  std::memset(o, 0, sizeof *o);
  o->device = -1;
  o->write_files = 1;
  o->shard_world = 1;
}

extern "C" void simu_assign_contigs(const uint64_t* lengths, int32_t n, int32_t world, int32_t* owner_out) {
  const std::vector<int> o = simu::Genome::assign_contigs(std::vector<uint64_t>(lengths, lengths + n), world);
  for (int32_t i = 0; i < n; i++) owner_out[i] = o[(size_t)i];
}

extern "C" int simu_run(const char* config_path, const simu_options* opt, simu_stats* stats, char* err, size_t err_len) {
  simu_options o;
  if (opt) o = *opt; else simu_default_options(&o);
  if (o.shard_world < 1) o.shard_world = 1;
  return simu::guarded(err, err_len, [&]() {
    std::unique_ptr<simu::Driver> d(new simu::Driver());
    d->opt = o;
    d->run(config_path ? config_path : "");
    if (stats) *stats = d->st;
  });
}

// ------------------------------------------------------------------------------------------------
// Session API: the same driver, opened step by step so that a caller (bench.py, a multi-GPU
// launcher) can keep the inputs resident in HBM and drive sg_sample on its own stream.
// ------------------------------------------------------------------------------------------------
struct simu_session { simu::Driver d; };

extern "C" int simu_open(const char* config_path, const simu_options* opt, simu_session** out, char* err, size_t err_len) {
  if (!out) return 1;
  *out = nullptr;
  std::unique_ptr<simu_session> s(new simu_session());
  if (opt) s->d.opt = *opt; else simu_default_options(&s->d.opt);
  if (s->d.opt.shard_world < 1) s->d.opt.shard_world = 1;
  int rc = simu::guarded(err, err_len, [&]() { s->d.open(config_path ? config_path : ""); });
  if (rc == 0) *out = s.release();
  return rc;
}
extern "C" void simu_close(simu_session* s) { delete s; }
extern "C" void* simu_engine(simu_session* s) { return s ? (void*)s->d.eng.ctx : nullptr; }
extern "C" uint64_t simu_planned_reads(simu_session* s) { return s->d.st.planned_reads; }
extern "C" int simu_chromosome_count(simu_session* s) { return (int)s->d.genome.chromosomes.size(); }
// Sum over this session's chromosomes of the GC-weighted length of population `popu`
// (Genome::setReadCounts' WL, Genome.cpp:787-797).  Runs pass 1 (haplotypes + GPU GC scan) on first use.
extern "C" int simu_weighted_length(simu_session* s, int popu, double* wl, char* err, size_t err_len) {
  return simu::guarded(err, err_len, [&]() {
    simu::Driver& d = s->d;
    const std::string& p = d.cfg.popu_names.at(popu);
    double WL = 0;
    for (const std::string& chr : d.genome.chromosomes) WL += d.plan.chromosome_weight(p, chr);
    *wl = WL;
  });
}
extern "C" int simu_set_reads(simu_session* s, int popu, int64_t reads, char* err, size_t err_len) {
  return simu::guarded(err, err_len, [&]() { s->d.plan.set_read_counts(s->d.cfg.popu_names.at(popu), (long)reads); });
}
// Upload the chromosome's haplotype chains and hand its sampling plan to the engine.  `has_work`
// is 0 when this shard has nothing to sample there.
extern "C" int simu_prepare_batch(simu_session* s, int popu, int chr, int* has_work, char* err, size_t err_len) {
  return simu::guarded(err, err_len, [&]() {
    bool w = s->d.prepare_batch(s->d.cfg.popu_names.at(popu), s->d.genome.chromosomes.at(chr));
    if (has_work) *has_work = w ? 1 : 0;
  });
}
extern "C" int simu_variant_table(simu_session* s, void* rows, uint64_t cap, uint64_t* n, char* err, size_t err_len) {
  return simu::guarded(err, err_len, [&]() {
    if (!s || !n) throw simu::Error("simu_variant_table: no session");
    if (!s->d.opt.truth_variants) throw simu::Error("simu_variant_table: the session was not opened with truth_variants");
    const std::vector<sg_variant> a = s->d.truth->variant_table().abi();
    *n = a.size();
    const uint64_t m = std::min<uint64_t>(cap, a.size());
    if (rows && m) memcpy(rows, a.data(), (size_t)m * sizeof(sg_variant));
  });
}
extern "C" void simu_get_stats(simu_session* s, simu_stats* st) { if (s && st) *st = s->d.st; }
// planned fragment slots of the batch simu_prepare_batch handed to the engine (this shard's part)
extern "C" uint64_t simu_batch_slots(simu_session* s) { return s ? s->d.plan.batch_slots() : 0; }
