// host/truth_bam.h -- --truth-bam: <stem>.truth.bam, a stream of BGZF members (whatever the FASTQ files are) with the
// open / piece / close lifecycle of the summed truth outputs, which drive it first at each point (truth_outputs.h).
// A sharded run writes parts like the FASTQ parts: rank 0's carries the header, the last rank's the end-of-file block.
// Under --truth-sort the pieces go to the stem's spool and are merged into the file at its close (truth_sort.h).
#pragma once
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "truth_sort.h"

namespace simu {

class TruthBam {
 public:
  TruthBam(Engine& eng, const simu_options& opt, simu_stats& st, const ContigTable& contigs) : eng(eng), opt(opt), st(st), contigs(contigs) {}
  ~TruthBam() { close_file(); }   // on an error path too the file closes with its end-of-file block; the spool goes with `tsort`
  TruthBam(const TruthBam&) = delete;
  TruthBam& operator=(const TruthBam&) = delete;
  void open(const std::string& dir, const std::string& stem);   // a stem starts: file, header, spool -- under write_files only
  // the records of the pass just sampled: made, compressed, counted and (unless --no-write) appended to the file.
  // Synchronous: the members are in the context's own buffer, which the next piece reuses.
  void piece();
  void close();   // the stem ends: its sorted runs merged into the file, the end-of-file block, the file

 private:
  void write_header();
  void close_file();
  Engine& eng;
  const simu_options& opt;
  simu_stats& st;
  const ContigTable& contigs;
  FILE* file = nullptr;
  std::vector<uint8_t> host;
  std::unique_ptr<TruthSort> tsort;   // --truth-sort: the stem's spool and the index of its runs; made on first use
};

}  // namespace simu
