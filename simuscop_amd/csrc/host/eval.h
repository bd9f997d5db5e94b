// host/eval.h -- `truthEval` as a library call: an aligner's BAM scored against the truth BAM simuReads --truth-bam wrote
// (the rule: csrc/sg_eval.h).  Both files are read here, inflated and decoded on the GPU (sg_eval_*, include/simuscop_amd.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct simu_eval_options {
  const char* truth;      // --truth: any truth BAM of this project (unsorted or sorted, with or without tags, paired or single-ended)
  const char* bam;        // --bam: what an aligner, or a sort, wrote from the same FASTQ files against the same FASTA
  const char* output;     // --out ("" / NULL: standard output)
  int32_t min_overlap;    // --min-overlap: PCT of the `near` category, 1..100 (default 10)
  int32_t device;         // --device
  int32_t threads;        // reader threads
  int32_t quiet;          // no progress lines on stderr
} simu_eval_options;

typedef struct simu_eval_stats {
  uint64_t test_records, secondary, supplementary, unknown, ambiguous, repeated, truth_records, truth_duplicates;
  uint64_t scored, missing;                               // records in the table; unclaimed truth reads, all mates and classes
  uint64_t truth_bgzf_bytes, test_bgzf_bytes;             // compressed bytes fed
  uint64_t truth_bytes, test_bytes;                       // inflated
  double t_inflate, t_truth, t_sort, t_test, t_total;     // seconds: inflate and record boundaries of both files (part of the
                                                          // next two); the truth's load; its sort; the test file; everything
} simu_eval_stats;

void simu_eval_default_options(simu_eval_options* o);
// 0 on success; otherwise the exit code, its message in `err`.  Nothing is written to `output` unless the run succeeds.
int simu_eval(const simu_eval_options* opt, simu_eval_stats* stats, char* err, size_t err_len);

#ifdef __cplusplus
}
#endif
