// host/read_plan.h -- which reads come from where: haplotype chains on the device, GC-weighted lengths (pass 1), the read
// apportioning (Genome::setReadCounts, Segment::setReadCount) and the sampling plan of one (population, chromosome) batch,
// cut into shards and pieces (batch_cut.h).  Two routes make the windows: the device planner (sg_windows_build /
// sg_plan_windows / sg_plan_range) for whole-genome runs, the host planner (sg_window_weights / sg_plan) for runs with
// BED targets and under SIMU_HOST_PLAN=1.  Each of weigh, build_batch and plan_range chooses its route in one place.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "engine.h"
#include "genome.h"
#include "simulate.h"
#include "truth_outputs.h"

namespace simu {

class ReadPlan {
 public:
  ReadPlan(Config& cfg, Genome& genome, Profile& prof, Engine& eng, const simu_options& opt, simu_stats& st, const ContigTable& contigs)
      : cfg(cfg), genome(genome), prof(prof), eng(eng), opt(opt), st(st), contigs(contigs) {}
  uint64_t seed = 0;   // of the haplotype draws; set once the config is loaded

  double chromosome_weight(const std::string& popu, const std::string& chr);   // its GC-weighted length; runs pass 1 on first use
  void set_read_counts(const std::string& popu, long reads);                   // Genome::setReadCounts, Genome.cpp:783-825
  // The sampling plan of one (population, chromosome): windows of the segments the reference would process
  // (Segment.cpp:675) with their fragRCs (Segment::setReadCount, Segment.cpp:462-476), numbered inside the
  // whole batch.  Any contiguous run of its segments can then be handed to the engine on its own
  // (plan_range): the run of a multi-GPU shard, or a memory-bounded piece of it -- the draws are addressed
  // by the batch-wide numbers, so the pieces' texts concatenate to the text of the whole.
  struct BatchPlan {
    std::string popu, chr, prefix;
    uint32_t bid = 0;
    bool paired = false;
    std::vector<uint64_t> slots;   // planned fragments of every active segment
    size_t a0 = 0, a1 = 0;         // this process's run of active segments (multi-GPU shard)
    bool dev = false;              // the window table lives on the device (sg_plan_windows)
  } cur;
  bool build_batch(const std::string& popu, const std::string& chr);   // false: nothing to sample in the batch (for this process)
  void plan_range(size_t a0, size_t a1);   // chains on the device, the plan of the active segments [a0, a1) of the current batch
  size_t piece_end(size_t c0) const;       // the piece of the shard's run that starts at c0 (SIMU_PIECE_SLOTS)
  uint64_t batch_slots() const;            // planned fragment slots of this shard's run
  static bool trace_pieces();              // SIMU_TRACE_PIECES: where a run's sampling time goes, piece by piece

 private:
  // windows made on the device (whole-genome runs; SIMU_HOST_PLAN=1 keeps the host planner for comparison runs)
  bool dev_plan() const;
  void upload(const std::string& popu, const std::string& chr);
  void prebuild(const std::string& popu);
  void weigh(const std::string& popu, const std::string& chr);
  static double seg_weight(const ChromPlan& plan, const Segment& g);
  sg_gc_model gc_model(const std::string& popu, const std::string& chr, int full_tile_form);
  void weigh_device(ChromPlan& plan, const std::string& popu, const std::string& chr);
  void weigh_host(ChromPlan& plan, const std::string& popu, const std::string& chr);
  uint64_t build_device(ChromPlan& plan);   // both: the batch's windows
  uint64_t build_host(ChromPlan& plan);
  void plan_range_device(size_t a0, size_t a1);
  void plan_range_host(size_t a0, size_t a1);

  Config& cfg;
  Genome& genome;
  Profile& prof;
  Engine& eng;
  const simu_options& opt;
  simu_stats& st;
  const ContigTable& contigs;
  uint32_t batch_id = 0;
  std::string resident;  // "popu\tchr" whose chains are on the device
  std::map<std::string, std::vector<double>> chr_wl_of;  // per population: GC-weighted length of every chromosome
  struct HostWindows {   // the host route's batch: its window table, and per active segment its size and first window
    std::vector<sg_window> wins;
    std::vector<uint32_t> seg_size, w_first;
  } host;
};

}  // namespace simu
