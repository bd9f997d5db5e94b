// host/read_plan.cpp -- see read_plan.h
#include "read_plan.h"

#include <atomic>
#include <chrono>
#include <cstring>
#include <mutex>
#include <thread>

#include "batch_cut.h"

namespace simu {
namespace {

using Clock = std::chrono::steady_clock;
inline double since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

// (long) of a double as the reference's machine code does it (cvttsd2si: NaN or out of range -> LONG_MIN), and sums that
// wrap like its 64-bit registers: see set_read_counts
inline long to_long_x86(double v) {
  if (!(v > -9223372036854775808.0 && v < 9223372036854775808.0)) return (long)0x8000000000000000ull;
  return (long)v;
}
inline long wrap_add(long a, long b) { return (long)((unsigned long)a + (unsigned long)b); }
inline long wrap_sub(long a, long b) { return (long)((unsigned long)a - (unsigned long)b); }

// Pieces of at most kPieceSlots planned fragments (whole segments; a segment is <= 1 Mbp per copy): the
// work buffers of a pass are ~0.5 KB per fragment and its text ~0.7 KB, so a 250 Mbp chromosome at 30x
// is a handful of pieces of ~10 GB, and a 1000x run still fits the card.  Each piece drains while the
// next one is sampled.
constexpr uint64_t kPieceSlots = 12u << 20;

}  // namespace

bool ReadPlan::dev_plan() const {
  static const bool host_plan = getenv("SIMU_HOST_PLAN") != nullptr;
  return genome.targets.empty() && !host_plan;
}
bool ReadPlan::trace_pieces() { return getenv("SIMU_TRACE_PIECES") != nullptr; }

void ReadPlan::upload(const std::string& popu, const std::string& chr) {
  const std::string key = popu + "\t" + chr;
  if (resident == key) return;
  ChromPlan& plan = genome.plans[popu][chr];
  Timed acc{st.t_hap_device};
  if (genome.device_haps) {
    eng.check(sg_build_haplotypes(eng.ctx, (int32_t)plan.chain_len.size(), plan.chain_len.data(), plan.pieces.data(),
                                  plan.pieces.size(), plan.literals.data(), plan.literals.size(), plan.patches.data(),
                                  plan.patches.size()),
              "sg_build_haplotypes");
    if (opt.truth_bam || opt.truth_depth || opt.truth_variants) {  // the copy list is the reads' way back to the reference: contig rows -> refIDs of the BAM header
      eng.check(sg_truth_map(eng.ctx, plan.pieces.data(), plan.piece_seg_first.data(), plan.piece_seg_first.size(), contigs.id_of_dev.data(),
                             (uint32_t)contigs.id_of_dev.size()),
                "sg_truth_map");
    }
  } else {
    std::vector<const char*> ptr;
    std::vector<uint64_t> len;
    for (const std::string& c : plan.chains) { ptr.push_back(c.data()); len.push_back(c.size()); }
    eng.check(sg_upload_haplotypes(eng.ctx, (int32_t)ptr.size(), ptr.data(), len.data()), "sg_upload_haplotypes");
  }
  resident = key;
}

// ---- pass 1 ----
sg_gc_model ReadPlan::gc_model(const std::string& popu, const std::string& chr, int full_tile_form) {
  if (prof.gc_quantiles.empty()) prof.build_gc_quantiles();
  sg_gc_model model;
  model.means = prof.gc_means;
  model.std = prof.gc_std;
  model.quantiles = prof.gc_quantiles.data();
  model.lg_cells = 14;
  model.frag_size = Genome::kFragSize;
  model.full_tile_form = full_tile_form;
  model.ctx24 = genome.host_ctx(popu, chr);
  return model;
}

// pass 1 for one chromosome: chains, windows, GC%, weights (Segment::getWeightedLength)
void ReadPlan::weigh(const std::string& popu, const std::string& chr) {
  ChromPlan& plan = genome.plans[popu][chr];
  if (plan.weighed) return;
  auto t0 = Clock::now();
  genome.build_chains(popu, chr, seed);   // no-ops when prebuild() already did them
  if (!dev_plan()) genome.build_windows(popu, chr);
  st.t_haplotypes += since(t0);
  t0 = Clock::now();
  upload(popu, chr);
  if (dev_plan()) weigh_device(plan, popu, chr);
  else weigh_host(plan, popu, chr);
  plan.weighed = true;
  st.t_plan += since(t0);
}

// Windows, GC%, GC factors, weights and the per-segment weight sums on the device: the host never sees a window
void ReadPlan::weigh_device(ChromPlan& plan, const std::string& popu, const std::string& chr) {
  std::vector<sg_window_gen> gens;
  plan.seg_win0.assign(plan.segs.size(), 0);
  uint64_t nwin = 0;
  for (size_t k = 0; k < plan.segs.size(); k++) {
    Segment& g = plan.segs[k];
    plan.seg_win0[k] = nwin;
    g.w0 = (uint32_t)nwin;
    if (g.has_seq)
      for (size_t h = 0; h < g.hap_len.size(); h++) {  // 1 kbp tiles + a shorter tail per haplotype string (Segment.cpp:563-592)
        if (!g.hap_len[h]) continue;
        gens.push_back(sg_window_gen{g.hap_base[h], g.hap_len[h], (uint32_t)h, (uint32_t)k, 0});
        nwin += (g.hap_len[h] + Genome::kFragSize - 1) / Genome::kFragSize;
      }
    g.w1 = (uint32_t)nwin;
  }
  const sg_gc_model model = gc_model(popu, chr, 1);
  plan.store_id = model.ctx24;
  plan.seg_w.assign(plan.segs.size(), 0.0);
  uint64_t n_out = 0;
  eng.check(sg_windows_build(eng.ctx, plan.store_id, gens.data(), gens.size(), (uint32_t)plan.segs.size(), &model, plan.seg_w.data(), &n_out),
            "sg_windows_build");
  plan.dev_windows = true;
}

// GC%, GC factor and weight of every window on the device (sg_window_weights); the draws of the factor are
// addressed by (segment ordinal, window ordinal inside the segment)
void ReadPlan::weigh_host(ChromPlan& plan, const std::string& popu, const std::string& chr) {
  std::vector<sg_gc_window> gcw;
  std::vector<uint32_t> widx, seg_ord, win_ord;
  for (size_t k = 0; k < plan.segs.size(); k++) {
    const Segment& g = plan.segs[k];
    if (!g.has_seq || (!genome.targets.empty() && g.targets.empty())) continue;  // placeholder windows carry no GC draw
    for (uint32_t w = g.w0; w < g.w1; w++) {
      gcw.push_back(sg_gc_window{g.hap_base[plan.w_hap[w]] + plan.w_spos[w], plan.w_hap[w], plan.w_len[w]});
      widx.push_back(w);
      seg_ord.push_back((uint32_t)k);
      win_ord.push_back(w - g.w0);
    }
  }
  // full 1 kbp tiles: factor/fragSize; tails and targets: factor*len/(fragSize*fragSize)
  // (Segment.cpp:576,586,615 -- the two forms round differently, keep both)
  const sg_gc_model model = gc_model(popu, chr, genome.targets.empty() ? 1 : 0);
  std::vector<double> wts(gcw.size());
  eng.check(sg_window_weights(eng.ctx, gcw.data(), seg_ord.data(), win_ord.data(), gcw.size(), &model, wts.data(), nullptr),
            "sg_window_weights");
  for (size_t q = 0; q < widx.size(); q++) plan.w_weight[widx[q]] = wts[q];
}

double ReadPlan::seg_weight(const ChromPlan& plan, const Segment& g) {
  if (plan.dev_windows) return plan.seg_w[(size_t)(&g - plan.segs.data())];
  double s = 0;
  for (uint32_t w = g.w0; w < g.w1; w++) s += plan.w_weight[w];
  return s;
}

double ReadPlan::chromosome_weight(const std::string& popu, const std::string& chr) {
  weigh(popu, chr);
  ChromPlan& plan = genome.plans[popu][chr];
  double c = 0;
  for (const Segment& g : plan.segs) c += seg_weight(plan, g);
  return c;
}

// Haplotype construction of a population's chromosomes is independent work: the reference does it
// serially on the main thread, twice (Genome.cpp:793, :876-878); here once, on `threads` workers.
void ReadPlan::prebuild(const std::string& popu) {
  std::vector<std::string> todo;
  for (const std::string& chr : genome.chromosomes)
    if (genome.owns(chr) && !genome.plans[popu][chr].chains_built) todo.push_back(chr);
  const size_t nthreads = std::min<size_t>((size_t)std::max<long long>(1, cfg.num["threads"]), todo.size());
  if (nthreads <= 1) return;  // weigh() builds on demand
  auto t0 = Clock::now();
  std::atomic<size_t> next(0);
  std::mutex err_mu;
  std::string err;
  std::vector<std::thread> pool;
  for (size_t t = 0; t < nthreads; t++) {
    pool.emplace_back([&]() {
      for (;;) {
        const size_t i = next.fetch_add(1);
        if (i >= todo.size()) return;
        try {
          genome.build_chains(popu, todo[i], seed);
          if (!dev_plan()) genome.build_windows(popu, todo[i]);
        } catch (const std::exception& e) {
          std::lock_guard<std::mutex> lk(err_mu);
          if (err.empty()) err = e.what();
        }
      }
    });
  }
  for (std::thread& th : pool) th.join();
  st.t_haplotypes += since(t0);
  if (!err.empty()) throw Error(err);
}

void ReadPlan::set_read_counts(const std::string& popu, long reads) {
  prebuild(popu);
  std::vector<double>& chr_wl = chr_wl_of[popu];
  if (chr_wl.empty()) {
    for (const std::string& chr : genome.chromosomes) chr_wl.push_back(genome.owns(chr) ? chromosome_weight(popu, chr) : 0);
    if (!genome.owner_of.empty() || (opt.shard_contigs && opt.exchange)) {
      // the other ranks' chromosomes: one small exchange per population (RCCL / gloo all-reduce in the torchrun front
      // end, the parent's pipes under `simuReads --gpus N`); each entry has one owner, so the sum is exact.  (A single
      // rank that was handed an exchange runs it too -- the sum of one contribution -- so that the transport can be
      // rehearsed on one GPU: tests/test_gpu_nccl_world1.py.)
      if (!opt.exchange) throw Error("ERROR: chromosome sharding needs an exchange callback (simu_options.exchange)");
      if (opt.exchange(opt.exchange_user, chr_wl.data(), (int32_t)chr_wl.size()) != 0)
        throw Error("ERROR: the weighted-length exchange between the ranks failed");
    }
  }
  double WL = 0;
  for (double c : chr_wl) WL += c;
  auto t0 = Clock::now();
  long cur = 0;
  for (size_t i = 0; i < genome.chromosomes.size(); i++) {
    ChromPlan& plan = genome.plans[popu][genome.chromosomes[i]];
    const double cw = chr_wl[i];
    // A chromosome -- or a whole population -- without weighted length (every window holds an N, or lies outside the
    // targets) makes these divisions 0/0 in the reference too (Genome.cpp:803-817).  Its binary casts the NaN (cvttsd2si:
    // LONG_MIN), the sums wrap, the read counts come out negative and sample nothing: no reads from that chromosome,
    // the run goes on.  The same arithmetic here (the oracle restates it alike); counts <= 0 are skipped below.
    const long chr_reads = i + 1 < genome.chromosomes.size() ? to_long_x86(reads * (cw / WL)) : wrap_sub(reads, cur);
    long sum = 0;
    for (size_t j = 0; genome.owns(genome.chromosomes[i]) && j < plan.segs.size(); j++) {
      Segment& g = plan.segs[j];
      if (j + 1 < plan.segs.size()) {
        const double share = seg_weight(plan, g) / cw;
        g.read_count = to_long_x86(share * chr_reads);
        sum = wrap_add(sum, g.read_count);
      } else {
        g.read_count = wrap_sub(chr_reads, sum);
      }
    }
    cur = wrap_add(cur, chr_reads);
  }
  st.t_plan += since(t0);
}

// ---- one (population, chromosome): Genome.cpp:870-887 ----
bool ReadPlan::build_batch(const std::string& popu, const std::string& chr) {
  ChromPlan& plan = genome.plans[popu][chr];
  cur = BatchPlan();
  cur.popu = popu; cur.chr = chr;
  cur.bid = batch_id++;  // every rank numbers every batch alike: the id addresses the draws
  if (cur.bid > 0xFFFF) throw Error("ERROR: more than 65535 (population, chromosome) batches");
  if (!genome.owns(chr)) return false;
  st.batches++;
  cur.paired = cfg.paired();
  cur.prefix = "@" + popu + "#" + chr + "#";
  auto t0 = Clock::now();
  cur.dev = plan.dev_windows;
  const uint64_t nwin = cur.dev ? build_device(plan) : build_host(plan);
  st.windows += nwin;
  st.segments += cur.slots.size();
  st.t_plan += since(t0);
  if (nwin == 0) return false;
  // shard by runs of segments (multi-GPU)
  return shard_cut(cur.slots, opt.shard_contigs ? 1 : opt.shard_world, opt.shard_rank, cur.a0, cur.a1);
}

// per-window read counts, the remainder rule, planned pairs and their prefix sums on the device (sg_plan_windows);
// the host keeps what it needs to cut the batch into shards and pieces: the planned fragments per segment
uint64_t ReadPlan::build_device(ChromPlan& plan) {
  upload(cur.popu, cur.chr);
  std::vector<sg_window_gen> gens;
  std::vector<sg_active_seg> active;
  for (size_t k = 0; k < plan.segs.size(); k++) {
    const Segment& g = plan.segs[k];
    if (!g.has_seq || g.read_count <= 0) continue;   // (negative: what a weightless chromosome's NaN shares turn into)
    uint64_t w = plan.seg_win0[k];
    bool any = false;
    for (size_t h = 0; h < g.hap_len.size(); h++) {
      if (!g.hap_len[h]) continue;
      gens.push_back(sg_window_gen{g.hap_base[h], g.hap_len[h], (uint32_t)h, (uint32_t)active.size(), w});
      w += (g.hap_len[h] + Genome::kFragSize - 1) / Genome::kFragSize;
      any = true;
    }
    if (!any) throw Error("ERROR: sampling window on an absent haplotype (chromosome " + cur.chr + ")");
    active.push_back(sg_active_seg{(int64_t)g.read_count, plan.seg_w[k], g.seq_size() / (unsigned)g.cn, 0});
  }
  cur.slots.assign(active.size(), 0);
  uint64_t nwin = 0;
  if (!active.empty())
    eng.check(sg_plan_windows(eng.ctx, plan.store_id, gens.data(), gens.size(), active.data(), (uint32_t)active.size(), Genome::kFragSize,
                              cur.bid, cur.paired ? 1 : 0, cur.prefix.c_str(), cur.slots.data(), &nwin),
              "sg_plan_windows");
  return nwin;
}

uint64_t ReadPlan::build_host(ChromPlan& plan) {
  std::vector<sg_window>& wins = host.wins;
  wins.clear(); host.seg_size.clear(); host.w_first.clear();
  const bool paired = cur.paired;
  uint64_t slot = 0;
  for (size_t k = 0; k < plan.segs.size(); k++) {
    const Segment& g = plan.segs[k];
    if (!g.has_seq || g.read_count <= 0) continue;   // (negative: what a weightless chromosome's NaN shares turn into)
    const double total = seg_weight(plan, g) + 2.2204e-16;
    const uint32_t first = (uint32_t)wins.size();
    const uint64_t slot0 = slot;
    long sum = 0;
    for (uint32_t w = g.w0; w < g.w1; w++) {
      const long rc = (long)(plan.w_weight[w] * g.read_count / total);
      sum += rc;
      const uint32_t h = plan.w_hap[w];
      if (g.hap_len[h] == 0) throw Error("ERROR: sampling window on an absent haplotype (chromosome " + cur.chr + ")");
      wins.push_back(sg_window{g.hap_base[h], h, plan.w_spos[w], plan.w_len[w], (int32_t)rc, (uint32_t)cur.slots.size(), 0});
    }
    if (sum < g.read_count) wins[first].n_reads += (int32_t)(g.read_count - sum);
    for (uint32_t i = first; i < wins.size(); i++) {
      wins[i].slot_base = (uint32_t)slot;
      const int n = wins[i].n_reads;
      slot += n <= 0 ? 0 : (paired ? ((uint64_t)n + 1) / 2 : (uint64_t)n);
    }
    host.seg_size.push_back(g.seq_size() / (unsigned)g.cn);
    host.w_first.push_back(first);
    cur.slots.push_back(slot - slot0);
  }
  if (slot > 0xFFFFFFF0ull) throw Error("ERROR: more than 2^32 fragments on chromosome " + cur.chr);
  return wins.size();
}

size_t ReadPlan::piece_end(size_t c0) const {
  uint64_t piece_slots = kPieceSlots;
  if (const char* e = getenv("SIMU_PIECE_SLOTS")) piece_slots = std::max<uint64_t>(1, strtoull(e, nullptr, 10));
  return simu::piece_end(cur.slots, c0, cur.a1, piece_slots);
}

uint64_t ReadPlan::batch_slots() const {
  uint64_t n = 0;
  for (size_t i = cur.a0; i < cur.a1 && i < cur.slots.size(); i++) n += cur.slots[i];
  return n;
}

void ReadPlan::plan_range(size_t a0, size_t a1) {
  if (cur.dev) plan_range_device(a0, a1);
  else plan_range_host(a0, a1);
}

void ReadPlan::plan_range_device(size_t a0, size_t a1) {
  auto t0d = Clock::now();
  upload(cur.popu, cur.chr);
  auto t_pl = Clock::now();
  eng.check(sg_plan_range(eng.ctx, (uint32_t)a0, (uint32_t)a1), "sg_plan_range");
  st.t_plan_api += since(t_pl);
  st.t_sample += since(t0d);
  if (trace_pieces())
    fprintf(stderr, "[piece] %s %s segments %zu..%zu: upload %.4f s, sg_plan_range %.4f s\n", cur.popu.c_str(), cur.chr.c_str(), a0, a1,
            since(t0d) - since(t_pl), since(t_pl));
}

void ReadPlan::plan_range_host(size_t a0, size_t a1) {
  const std::vector<sg_window>& wins = host.wins;
  const uint32_t w_lo = host.w_first[a0];
  const uint32_t w_hi = a1 < host.w_first.size() ? host.w_first[a1] : (uint32_t)wins.size();
  const uint32_t slot_lo = wins[w_lo].slot_base;
  std::vector<sg_window> shard(wins.begin() + w_lo, wins.begin() + w_hi);
  std::vector<uint32_t> sh_first, sh_size;
  for (size_t i = a0; i < a1; i++) { sh_first.push_back(host.w_first[i] - w_lo); sh_size.push_back(host.seg_size[i]); }
  sh_first.push_back(w_hi - w_lo);
  for (sg_window& w : shard) { w.seg -= (uint32_t)a0; w.slot_base -= slot_lo; }

  auto t0 = Clock::now();
  upload(cur.popu, cur.chr);
  sg_batch b;
  std::memset(&b, 0, sizeof b);
  b.batch_id = cur.bid;
  b.paired = cur.paired ? 1 : 0;
  b.name_prefix = cur.prefix.c_str();
  b.windows = shard.data();
  b.n_windows = shard.size();
  b.seg_size = sh_size.data();
  b.seg_first_window = sh_first.data();
  b.n_segs = (uint32_t)sh_size.size();
  b.first_window = w_lo;
  b.first_slot = slot_lo;
  auto t_pl = Clock::now();
  eng.check(sg_plan(eng.ctx, &b), "sg_plan");
  st.t_plan_api += since(t_pl);
  st.t_sample += since(t0);
}

}  // namespace simu
