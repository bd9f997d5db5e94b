// host/truth_outputs.h -- the truth outputs that are summed over a stem: --truth-depth, --truth-variants, --truth-errors.
// Their lifecycle in the driver is here once (DESIGN.md "The summed truth outputs' lifecycle"); an output supplies only
// what differs (TruthOutput).  --truth-bam is a stream, not a sum, with the same three points (truth_bam.h): it is held
// here and driven first at each of them.
#pragma once
#include <cstdio>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../../include/simuscop_amd.h"
#include "engine.h"
#include "genome.h"
#include "profile.h"
#include "simulate.h"
#include "truth_variants.h"

namespace simu {

// The reference's contigs as every truth output numbers them, made once after the inputs are loaded: the FASTA's contigs
// in file order, each under the first token of its header line as the file writes it (`chr20` stays `chr20`, although
// the reads' names and the variant files say `20`), so that the outputs and the FASTA name a contig alike.  A contig
// whose key the file holds twice (the same name again, or `chr20` and `20`): no read comes from the second sequence and
// SAM wants every SN once, so only the first is listed (fasta.h; --unique-contigs refuses such a file).
struct ContigTable {
  std::vector<std::string> name;    // [refID]
  std::vector<uint64_t> len;        // [refID]
  std::vector<int32_t> id_of_row;   // FASTA row -> refID, -1: a row that is not listed
  std::vector<int32_t> id_of_dev;   // engine contig (row of the table given to sg_reference_commit) -> refID
  void build(const Fasta& fa);
};

// One contig's bedGraph rows appended to `out` (simu_depth_format, simulate.h); returns the lines, or UINT64_MAX for data
// that does not describe a contig of `ln` bases.
uint64_t depth_format(std::string& out, const std::string& name, uint64_t ln, uint64_t bin, const uint64_t* sums, const sg_depth_run* runs,
                      uint64_t n);

struct TruthOutput {  // what differs between the outputs
  const char *suffix, *open_what, *write_what;   // the file's, and the nouns of "can not open ..." and "short write to ..."
  double simu_stats::*timer;
  std::function<void()> start, add, reset;       // the device state; the add call, into the stats it feeds; zero for the next stem
  std::function<void(TruthOutput&)> render;      // the stem's text, handed to put() whole or in parts
  bool begun = false, in_stem = false;
  std::unique_ptr<FILE, int (*)(FILE*)> file{nullptr, fclose};   // closes on every path
  void put(const std::string& text);
};

class TruthBam;

// The truth BAM, then the enabled summed outputs in the order depth, variants, errors; every call goes over them once.
struct TruthOutputs {
  TruthOutputs(Engine& eng, const simu_options& opt, simu_stats& st, const ContigTable& contigs, const Genome& genome, const Config& cfg,
               const Profile& prof);
  ~TruthOutputs();
  void begin();                                               // on first use (a session has no stems: its caller adds, reads and resets itself, and makes its own sg_truth_bam calls)
  void open(const std::string& dir, const std::string& stem); // a stem starts: the file, under write_files only
  void piece();                                               // the pass just sampled
  void close();                                               // the stem ends: render, write, reset; nothing without a stem
  const VariantTable& variant_table();                        // from the variation and SNP rows of all populations, on first use

 private:
  void begin(TruthOutput& o);
  std::unique_ptr<TruthBam> bam;
  std::vector<TruthOutput> outs;
  Engine& eng;
  const simu_options& opt;
  simu_stats& st;
  const ContigTable& contigs;
  const Genome& genome;
  const Config& cfg;
  VariantTable vtable;
  bool vtable_built = false;
  sg_errtab_shape errors_shape{};
};

}  // namespace simu
