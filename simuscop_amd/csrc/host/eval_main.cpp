// host/eval_main.cpp -- `truthEval`: how many reads an aligner placed correctly, and at which MAPQ, against the truth BAM of
// simuReads --truth-bam (host/eval.cpp; the rule: csrc/sg_eval.h).  Options, messages and exit codes in the style of seqToProfile.
//   --truth <file>       the truth BAM (unsorted or --truth-sort, with or without --truth-tags)
//   --bam <file>         the BAM file an aligner (or a sort of its output) wrote from the same FASTQ files
//   --out <file>         eval.tsv (default: standard output)
//   --min-overlap <pct>  least overlap, in percent of the shorter interval, of a `near` placement: 1..100 (default 10)
//   --device <n>         GPU to use (default 0)        --quiet   no progress lines        --stats   one JSON line of counts and times
#include <getopt.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include "eval.h"

static void usage(const char* app) {
  std::cerr << "\nUsage: " << app << " [options]\n\n"
            << "Options:\n"
            << "    -h, --help                      give this information\n"
            << "    -t, --truth <string>            truth BAM file written by simuReads --truth-bam\n"
            << "    -b, --bam <string>              BAM file of the same reads as an aligner placed them\n"
            << "    -o, --out <string>              output file [default: standard output]\n"
            << "    -m, --min-overlap <int>         least overlap in percent of the shorter interval for a near placement [default:10]\n"
            << "        --device <int>              device to use [default:0]\n"
            << "        --quiet                     no progress lines\n"
            << "        --stats                     one JSON line of counts and times on standard error\n\n"
            << "Example:\n"
            << "    " << app << " --truth sample.truth.bam --bam aligned.bam --out eval.tsv\n\n";
}

int main(int argc, char* argv[]) {
  simu_eval_options o;
  simu_eval_default_options(&o);
  std::string truth, bam, out;
  bool stats = false;
  const struct option long_options[] = {
      {"help", no_argument, 0, 'h'},          {"truth", required_argument, 0, 't'},  {"bam", required_argument, 0, 'b'},
      {"out", required_argument, 0, 'o'},     {"min-overlap", required_argument, 0, 'm'},
      {"device", required_argument, 0, 1001}, {"quiet", no_argument, 0, 1002},       {"stats", no_argument, 0, 1003},
      {0, 0, 0, 0}};
  int c;
  while ((c = getopt_long(argc, argv, "ht:b:o:m:", long_options, NULL)) != -1) {
    switch (c) {
      case 'h': usage(argv[0]); return 0;
      case 't': truth = optarg; break;
      case 'b': bam = optarg; break;
      case 'o': out = optarg; break;
      case 'm': {
        char* end = nullptr;
        const long v = strtol(optarg, &end, 10);
        o.min_overlap = (end == optarg || *end || v < 1 || v > 100) ? 0 : (int32_t)v;   // (0: refused below)
        break;
      }
      case 1001: o.device = atoi(optarg); break;
      case 1002: o.quiet = 1; break;
      case 1003: stats = true; break;
      default: usage(argv[0]); return 1;
    }
  }
  if (truth.empty()) {
    std::cerr << "Use --truth to specify the truth BAM file written by simuReads --truth-bam." << std::endl;
    usage(argv[0]);
    return 1;
  }
  if (bam.empty()) {
    std::cerr << "Use --bam to specify the BAM file to evaluate." << std::endl;
    usage(argv[0]);
    return 1;
  }
  if (o.min_overlap < 1 || o.min_overlap > 100) {
    std::cerr << "Error: parameter \"min-overlap\" should be an integer from 1 to 100!" << std::endl;
    return 1;
  }
  o.truth = truth.c_str(); o.bam = bam.c_str(); o.output = out.c_str();
  simu_eval_stats st;
  char err[4096] = "";
  const int rc = simu_eval(&o, &st, err, sizeof err);
  if (rc != 0) {
    if (err[0]) std::cerr << err << std::endl;
    return rc;
  }
  if (stats)
    fprintf(stderr, "{\"truth_records\": %llu, \"truth_duplicates\": %llu, \"test_records\": %llu, \"scored\": %llu, \"secondary\": %llu, "
                    "\"supplementary\": %llu, \"unknown\": %llu, \"ambiguous\": %llu, \"repeated\": %llu, \"missing\": %llu, "
                    "\"truth_bgzf_bytes\": %llu, \"truth_bytes\": %llu, \"test_bgzf_bytes\": %llu, \"test_bytes\": %llu, "
                    "\"t_inflate\": %.4f, \"t_truth\": %.4f, \"t_sort\": %.4f, \"t_test\": %.4f, \"t_total\": %.4f}\n",
            (unsigned long long)st.truth_records, (unsigned long long)st.truth_duplicates, (unsigned long long)st.test_records,
            (unsigned long long)st.scored, (unsigned long long)st.secondary, (unsigned long long)st.supplementary, (unsigned long long)st.unknown,
            (unsigned long long)st.ambiguous, (unsigned long long)st.repeated, (unsigned long long)st.missing,
            (unsigned long long)st.truth_bgzf_bytes, (unsigned long long)st.truth_bytes, (unsigned long long)st.test_bgzf_bytes,
            (unsigned long long)st.test_bytes, st.t_inflate, st.t_truth, st.t_sort, st.t_test, st.t_total);
  if (!o.quiet) {
    const long secs = (long)st.t_total;
    std::cerr << "\nElapsed time: " << secs / 60 << " minutes and " << secs % 60 << " seconds!\n" << std::endl;
  }
  return 0;
}
