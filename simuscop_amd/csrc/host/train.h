// host/train.h -- `seqToProfile` as a library call: the reference's profile training (src/seqToProfile.cpp:19-147,
// Genome::loadTrainData lib/genome/Genome.cpp:32-39, Profile::init / train / saveResults lib/profile/Profile.cpp:172-218,
// 1442-1484, 1240-1365) with the per-read work on the GPU (sg_train_begin / _feed / _finish, include/simuscop_amd.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct simu_train_options {
  const char* bam;        // -b: handed to `samtools view -F 0xD04 -q 20` exactly as the reference does (Profile.cpp:1448)
  const char* sam;        // --sam (additive): lines of `samtools view` text from a file, or "-" for standard input, instead
  const char* target;     // -t
  const char* vcf;        // -v
  const char* ref;        // -r
  const char* output;     // -o ("" / NULL: standard output, as in the reference)
  const char* samtools;   // -s
  int32_t kmer;           // -k (default 3)
  int32_t bins;           // -B (default 50)
  int32_t device;         // --device (additive)
  int32_t threads;        // reader threads of the reference ingest
  int32_t quiet;          // no progress lines on stderr
  const char* stamp;      // NULL: the current time as saveResults prints it; tests pass a fixed line
  uint64_t max_reads;     // --max-reads (additive): Profile::processRead's maxCount; 0 = the reference's 300,000,000 counted reads
                          // (600,000,000 with targets), behind which it stops reading (Profile.cpp:236, 497-507)
  int32_t decode_bam;     // --decode-bam (additive): `bam` is read and decoded here (BGZF inflate and the records on the GPU) instead
                          // of through samtools; the lines are the ones `samtools view -F 0xD04 -q 20` prints
  int32_t device_vcf;     // --device-vcf (additive): a plain-text `vcf` is parsed on the GPU (sg_vcf_feed) instead of by the host's
                          // fgets loop; same rows, warnings and exit codes.  A BGZF `vcf` (x.vcf.gz as bgzip writes it) always is
} simu_train_options;

typedef struct simu_train_stats {
  uint64_t lines, reads_counted, gc_rejected, gc_windows, gc_pairs, skipped_overhang, sam_bytes;
  int32_t read_length, bins, gc_fitted, capped;   // capped: the run ended at max_reads
  double t_reference, t_reads, t_total;   // seconds: reference to the device; SAM text through the kernels; everything
  double insert_rate, del_rate, std_isize, gc_std;
  uint64_t bam_bytes, bam_records;   // --decode-bam: BGZF bytes fed, records decoded (kept or not)
  double t_inflate;                  // seconds in sg_train_feed_bgzf (inflate, record boundaries, rendering)
  double t_vcf;                      // seconds reading the VCF, on either route
  uint64_t vcf_bytes, vcf_fragments, vcf_undecided;   // its text; what fgets(buf, 20000) would return; those the device handed back
  int32_t vcf_on_device;             // 1: the device route (a BGZF file, or --device-vcf)
} simu_train_stats;

void simu_train_default_options(simu_train_options* o);
// 0 on success; otherwise the exit code the reference would use, its message in `err`.
int simu_train(const simu_train_options* opt, simu_train_stats* stats, char* err, size_t err_len);

#ifdef __cplusplus
}
#endif
