// host/simulate.h -- `simuReads <config>` as a library call (used by the CLI, tests and bench.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct simu_options {
  int32_t device;          // -1: take `device` from the config (default 0)
  int32_t has_seed;        // 0: take `seed` from the config
  uint64_t seed;
  int32_t write_files;     // 1: write FASTQ like the reference (SeqWriter); 0: keep results on the device only
  int32_t fetch;           // with write_files == 0: still copy the FASTQ text to (pinned) host memory
  int32_t quiet;           // suppress the reference's stderr progress lines
  int32_t shard_rank;      // multi-GPU: this process samples batches with (batch ordinal % shard_world) == shard_rank
  int32_t shard_world;     // 1 = no sharding
  const char* output_dir;  // NULL / "": use the config's `output`
  int32_t repeat_sample;   // >1: re-run sg_sample this many times per batch (kernel timing experiments)
  int32_t host_haplotypes; // 1: parse the FASTA and edit haplotype strings on the host, upload them
                           // (sg_upload_haplotypes); 0 (default): stream the file to the device and
                           // assemble the haplotypes there (sg_reference_*, sg_build_haplotypes)
  int32_t gzip;            // 1: compress the FASTQ text on the device (sg_compress) and write <name>_1.fq.gz ...
                           // as BGZF (block gzip); what `zcat` gives back is byte for byte the plain file
  int32_t shard_contigs;   // multi-GPU, 1: rank shard_rank of shard_world OWNS whole chromosomes (longest-first assignment
                           // by length): it ingests, cuts, scans and samples only those; the per-chromosome GC-weighted
                           // lengths every rank needs for the read apportioning (Genome::setReadCounts) come through
                           // `exchange`.  0: every rank holds the whole genome and samples its run of segments of every batch.
  int32_t no_eof_block;    // gzip part files: leave the BGZF end-of-file block to whoever concatenates the parts
  // all-reduce(sum) of n doubles over the ranks, in place; every element has exactly one non-zero contributor (its
  // owner), so the sum is exact whatever the order.  Called once per population.  Returns 0 on success.
  int (*exchange)(void* user, double* values, int32_t n);
  void* exchange_user;
  // Three reference quirks are kept by default; each flag is additive and turns ONE of them off:
  int32_t crlf_as_lf;      // 1: a FASTA with CR LF line ends reads like its LF twin (default: the carriage returns stay, in the
                           //    contig names and as one unknown base per line, as fastahack keeps them: Fasta.cpp:150-199)
  int32_t strict_bases;    // 1: a literal 'X' in the genome is an unknown base (default: it walks the k-mer trie as the place
                           //    holder of the short contexts, Profile.cpp:94-101, 220-226)
  int32_t unique_contigs;  // 1: refuse a FASTA that holds a contig name twice (default: the name stands twice in the
                           //    chromosome list and both resolve to the first sequence, Fasta.cpp:67,84-97,198)
  int32_t truth_index;     // 1: with truth_bam and truth_sort, <stem>.truth.bam.bai is written beside the sorted BAM: a BAI index (SAMv1
                           //    5.2) whose rows are made on the device while each merged tile is still there (sg_bamindex_*; the
                           //    rule: DESIGN.md "Index of the sorted truth BAM").  The BAM itself is byte for byte the same.  Refused
                           //    without truth_sort, and for a contig longer than 2^29 bases
  int32_t truth_bam;       // 1: write every read's true alignment to <stem>.truth.bam beside the FASTQ files (sg_truth_bam: the
                           //    records are made and compressed on the device, piece by piece, in FASTQ order); needs the
                           //    device-assembled haplotypes (refused with host_haplotypes).  Sharded runs write parts like the
                           //    FASTQ parts: rank 0's carries the header, the last rank's the BGZF end-of-file block
  int32_t truth_tags;      // 1: with truth_bam, its records carry NM, MD and XE tags (sg_truth_bam_tags; the rule: DESIGN.md "Truth
                           //    tags"); refused without truth_bam
  int32_t truth_sort;      // 1: with truth_bam, <stem>.truth.bam is coordinate-sorted (@HD SO:coordinate; the order: DESIGN.md "Sorted
                           //    truth BAM"): every piece is sorted on the device (sg_bamsort_pass) and spooled to
                           //    <stem>.truth.bam.runs.tmp, the runs are merged on the device at the stem's close (sg_bamsort_merge),
                           //    SIMU_SORT_TILE_BYTES of records at a time.  Refused without truth_bam and in a sharded run (sorted
                           //    parts cannot be concatenated)
  int32_t truth_errors;    // 1: write per mate, cycle and reported quality how many bases were really wrong -- the read against the
                           //    haplotype bases it was cut from, so a variant allele is no error -- with a substitution matrix and
                           //    the sequencing indels to <stem>.truth.errors.tsv beside the FASTQ files (sg_errtab_*; the rule:
                           //    DESIGN.md "True error counts"), summed like truth_depth.  Needs no piece map: works with
                           //    host_haplotypes too; refused in a sharded run (partial tables would have to be summed)
  int32_t truth_variants;  // 1: write per variant of the variation and SNP files how many reads cover the site and how many
                           //    carry the allele to <stem>.truth.variants.tsv beside the FASTQ files (sg_variants_*; the
                           //    rule: DESIGN.md "True allele counts"), summed like truth_depth.  Needs the device-assembled
                           //    haplotypes; refused in a sharded run (partial counts would have to be summed)
  int32_t truth_depth;     // BIN >= 1: write the reads' true coverage to <stem>.truth.depth.bedgraph beside the FASTQ files
                           //    (sg_depth_*: every M base of every read's true alignment, summed over the pieces, chromosomes
                           //    and populations written into the stem); BIN 1: one row per run of equal depth, BIN > 1: the
                           //    mean depth of every BIN bases.  0: off.  Needs the device-assembled haplotypes like truth_bam;
                           //    refused in a sharded run (partial depths would have to be summed)
} simu_options;

typedef struct simu_stats {
  uint64_t reads;          // FASTQ records produced (both mates counted)
  uint64_t fragments;      // pairs (PE) or reads (SE)
  uint64_t fastq_bytes;
  uint64_t planned_reads;  // Genome::yieldReads `reads` (Genome.cpp:831)
  uint64_t windows, segments, batches;
  double t_load;           // config + inputs + profile
  double t_haplotypes;     // haplotype chains: edit lists or strings (host)
  double t_plan;           // GC scan (device) + weights + read counts (host)
  double t_sample;         // sg_plan + sg_sample + sg_result (GPU pass, wall)
  double t_fetch;          // D2H of FASTQ text
  double t_write;          // file output
  double t_total;
  float kernel_ms[8];      // summed per kernel (SG_K_*)
  uint64_t queued_items;   // items the fast emit kernel left to the generic item code (sg_emit_info)
  uint64_t requeued_batches;  // batches emitted again because that queue overflowed
  double t_engine;         // part of t_load: sg_create (HIP context, stream)
  double t_reference;      // part of t_load: reference FASTA to its resident form (host strings or device codes)
  double t_hap_device;     // part of t_plan/t_sample: sg_build_haplotypes / sg_upload_haplotypes calls
  double t_plan_api;       // part of t_sample: sg_plan calls (window upload, work buffers)
  double t_compress;       // sg_compress calls (gzip mode)
  uint64_t gz_bytes;       // compressed bytes produced (gzip mode)
  int32_t emit_kernel;     // the emit kernels of the last pass (sg_emit_path: SG_EMIT_*; 0: no pass ran)
  int32_t emit_slow_rows_lds;
  uint32_t emit_lds_bytes, emit_clean_cap;
  uint64_t bai_bins;       // truth_index: bins written to the .bai files (the pseudo-bins aside), ...
  uint64_t bai_chunks;     // ... the chunks in them ...
  uint64_t bai_bytes;      // ... and the files' bytes
  double t_bai;            // sg_bamindex_* calls, simu_bai_build and writing the files (part of t_truth_sort)
  uint64_t truth_records;  // truth_bam: BAM records made (one per read), of which without an alignment ...
  uint64_t truth_unmapped;
  uint64_t truth_bytes;    // ... bytes of the record stream and of its BGZF members (header and end-of-file block aside)
  uint64_t truth_bgzf_bytes;
  double t_truth;          // sg_truth_bam calls + fetching and writing their members (synchronous, per piece)
  uint64_t truth_tag_bytes;   // truth_tags: bytes of truth_bytes that are tags, ...
  uint64_t truth_md_dropped;  // ... mapped records left without MD (a text longer than the engine's cap), ...
  uint64_t truth_nm_sum;      // ... and the sums of the NM and of the XE values
  uint64_t truth_xe_sum;
  uint64_t truth_sort_runs;   // truth_sort: sorted runs spooled (one per piece with records), ...
  uint64_t truth_sort_tiles;  // ... tiles of the key space they were merged in, ...
  uint64_t truth_spool_bytes; // ... bytes the spool files held
  double t_truth_sort;        // ... and the merges at the stems' close: cutting, reading the spool, sg_bamsort_merge, writing
  uint64_t errors_bases;   // truth_errors: read bases paired with an A/C/G/T template base, ...
  uint64_t errors_subst;   // ... of which the read shows another letter
  double t_errors;         // sg_errtab_* calls, formatting and writing the table
  uint64_t variant_rows;   // truth_variants: rows of the variant table, ...
  uint64_t variant_dropped;  // ... input rows left out of it (a contig the FASTA does not hold, a position outside it, no length)
  uint64_t variant_hits;   // ... counts of `total` over all rows and stems
  double t_variants;       // building the table, sg_variants_* calls, formatting and writing the rows
  uint64_t depth_bases;    // truth_depth: M bases added to the depth, ...
  uint64_t depth_rows;     // ... bedGraph lines made (written unless write_files == 0)
  double t_depth;          // sg_depth_* calls, formatting and writing the rows
} simu_stats;

// Returns 0 on success.  On failure returns the exit code the reference would use and writes the
// message it would print to `err`.
int simu_run(const char* config_path, const simu_options* opt, simu_stats* stats, char* err, size_t err_len);

void simu_default_options(simu_options* opt);

// Chromosome ownership of the shard_contigs mode: owner_out[i] = rank of contig i (longest first onto the least
// loaded rank; ties by file order).  Exposed for the launchers and tests.
void simu_assign_contigs(const uint64_t* lengths, int32_t n, int32_t world, int32_t* owner_out);

// CPU-only self-test of the haplotype edit lists (no GPU call): every (population, chromosome) of the config is
// built twice -- as strings (Genome::segment_haplotypes, the reference's std::string editing) and as the copy list
// handed to sg_build_haplotypes (Genome::segment_pieces), materialised on the host -- and compared byte for byte.
// Returns 0 when all chains agree; otherwise 1 and a description in `err`.
int simu_selftest_haplotypes(const char* config_path, uint64_t seed, char* err, size_t err_len);

// One contig's rows of a --truth-depth bedGraph file ("name<TAB>start<TAB>end<TAB>value\n", 0-based, half open, tiling
// [0, ln)), host only.  bin == 1: `data` is n sg_depth_run rows {uint32 start, uint32 depth}, the first at 0, starts
// ascending; a row reaches to the next one's start (the last to ln), the value is the depth as a decimal integer, and
// neighbours of equal depth come out as one row.  bin > 1: `data` is n = ceil(ln / bin) uint64 sums; one row per bin,
// unmerged, the value printf("%.4f", (double)sum / (double)width) with the row's own width.  The text is written to
// out[0 .. cap) when it fits; returns its length (call again with that much room), *rows = lines.  UINT64_MAX: `data`
// does not describe a contig of ln bases.
uint64_t simu_depth_format(const char* name, uint64_t ln, uint64_t bin, const void* data, uint64_t n, char* out, uint64_t cap, uint64_t* rows);

// A --truth-variants file from raw variant rows, host only: the table is built as the driver builds it and written with
// the counts given.  Contigs are the n_contigs names / lengths in BAM refID order, populations the n_popus names in
// config order.  Input row i: kind[i] 's' (variation-file SNV), 'p' (SNP-file row), 'i', 'd'; contig[i] a contig name
// (one not listed: the row is dropped); pos[i] the file's 1-based position; popu[i] the population's index ('p' rows: any);
// text[i] the alt base, the inserted sequence or the deletion length in decimal.  Rows merge on (contig, pos - 1,
// upper-case allele) for s / p, (contig, pos - 1, length) for i (the first sequence met is written) and d; rows with
// pos - 1 outside [0, LN) or a length below 1 are dropped.  Order: refID, position, type (s / p, i, d), allele byte or
// length.  The file: the header line "#chrom\tpos\ttype\tallele\talt_reads\ttotal_reads\tpopulations", then one line per
// table row, `type` s when a variation-file row lists the allele, else p; `populations` comma-joined in config order, `.`
// for p.  counts: [rows][2] uint32 (alt, total), or NULL for zeros; n_counts must then be the table's rows (UINT64_MAX
// otherwise, and *rows still says how many there are).  table: when not NULL, room for table_cap sg_variant rows (simuscop_amd.h), filled
// with the table as sg_variants_begin takes it when it fits.  The text is written to out[0 .. cap) when it fits; returns
// its length.
uint64_t simu_variants_format(const char* const* contig_name, const uint64_t* contig_len, uint32_t n_contigs, const char* const* popu_name,
                              uint32_t n_popus, const char* kind, const char* const* contig, const int64_t* pos, const int32_t* popu,
                              const char* const* text, uint64_t n_in, const uint32_t* counts, uint64_t n_counts, void* table,
                              uint64_t table_cap, char* out, uint64_t cap, uint64_t* rows, uint64_t* dropped);

// How --truth-sort cuts the key space of a stem's sorted runs into tiles that fit the device, host only.  Run r holds
// n[r] records with ascending keys[r][i]; prefix[r] holds n[r] + 1 prefix sums of their bytes (prefix[r][0] = 0).  The
// result is `tiles` ascending splitter keys K_i: tile i holds the records with K_i <= key < K_(i+1), the last tile all
// from its K on; every tile holds a record, and together they hold every record once.  A tile takes as many bytes as fit
// under `budget`, except a tile that consists of one key value: that one may exceed it and is then marked in single[i]
// (all its keys are equal, so it needs no sort: the merged order is the runs in order).  The rule: bytes(key < K) = the
// sum over r of prefix[r][lower_bound(keys[r], K)] is monotone in K, so a binary search over K finds each splitter.
// Returns the number of tiles and writes the first min(tiles, cap) splitters and marks (either array may be NULL);
// UINT64_MAX: a NULL table.
uint64_t simu_sort_tiles(uint32_t n_runs, const uint64_t* const* keys, const uint64_t* n, const uint64_t* const* prefix, uint64_t budget,
                         uint64_t* splitters, uint8_t* single, uint64_t cap);

// The bytes of a --truth-index file (a BAI, SAMv1 5.2; the rule: csrc/sg_bamindex.h), host only.  rows: n_rows sg_bai_chunk
// rows (simuscop_amd.h) -- the rows of all sg_bamindex_add calls of a stem in call order, every open end closed.  linear
// and counts: what sg_bamindex_finish gives for the n_ref references of ref_len[] bases.  Rows are ordered by (refID,
// bin) keeping their order within a bin, neighbours of a bin with end == beg are joined, bins are written ascending, the
// pseudo-bin 37450 last for a reference with records (its end is the largest end of the reference's chunks), n_intv
// reaches to the last touched window and an untouched window takes the value of the next touched one on its right;
// n_no_coor closes the file.  The bytes are written to out[0 .. cap) when they fit; returns their number.  *bins = bins
// written, the pseudo-bins aside, *chunks = chunks in them.  UINT64_MAX: tables that do not describe an index (a NULL
// table, a row of a reference or bin that does not exist, an open end, rows and counts that disagree on whether a
// reference has records).
uint64_t simu_bai_build(uint32_t n_ref, const uint64_t* ref_len, const void* rows, uint64_t n_rows, const uint64_t* linear, const uint64_t* counts,
                        void* out, uint64_t cap, uint64_t* bins, uint64_t* chunks);

// ---- step-by-step session (bench.py / multi-GPU launcher) ----
typedef struct simu_session simu_session;
int simu_open(const char* config_path, const simu_options* opt, simu_session** out, char* err, size_t err_len);
void simu_close(simu_session* s);
void* simu_engine(simu_session* s);  // the sg_ctx* of this session
uint64_t simu_planned_reads(simu_session* s);
int simu_chromosome_count(simu_session* s);
int simu_weighted_length(simu_session* s, int popu, double* wl, char* err, size_t err_len);
int simu_set_reads(simu_session* s, int popu, int64_t reads, char* err, size_t err_len);
int simu_prepare_batch(simu_session* s, int popu, int chr, int* has_work, char* err, size_t err_len);
void simu_get_stats(simu_session* s, simu_stats* st);
// the variant table of a session opened with truth_variants (the one given to sg_variants_begin at the first
// simu_prepare_batch): *n = rows; the first min(cap, *n) are written
int simu_variant_table(simu_session* s, void* rows /* sg_variant[cap] */, uint64_t cap, uint64_t* n, char* err, size_t err_len);
uint64_t simu_batch_slots(simu_session* s);  // planned fragment slots of the prepared batch (sg_truth_reads addresses reads by slot)

#ifdef __cplusplus
}

#include <string>
// What a sharded run's rank puts behind the names of its FASTQ and truth BAM parts.
inline std::string simu_shard_suffix(const simu_options& o) { return o.shard_world > 1 ? ".part" + std::to_string(o.shard_rank) : ""; }
// The rules of the truth options, once, for whoever has to refuse a run: the text of the first one `o` breaks, or "".
// Needs device haplotypes: an output that maps reads back to the reference reads the haplotypes' copy lists.  Cannot
// be sharded: an output summed over a stem would come out as partial sums, one per rank.  `sharded`: more than one
// rank will run; `all`: the rules of a value and of the haplotypes too (the command line leaves those to the run).
inline std::string simu_truth_refusal(const simu_options& o, bool sharded, bool all) {
  struct Rule { const char* flag; int32_t on; bool is_width, needs_map; const char* partial; };
  const Rule rules[] = {{"--truth-bam", o.truth_bam, false, true, nullptr}, {"--truth-depth", o.truth_depth, true, true, "depths"},
                        {"--truth-variants", o.truth_variants, false, true, "counts"}, {"--truth-errors", o.truth_errors, false, false, "tables"}};
  if (o.truth_tags && !o.truth_bam) return "Error: --truth-tags needs --truth-bam: the tags go on the truth BAM's records";
  if (o.truth_sort && !o.truth_bam) return "Error: --truth-sort needs --truth-bam: it is the truth BAM's records that are sorted";
  if (o.truth_index && !o.truth_sort) return "Error: --truth-index needs --truth-sort: a BAI indexes a coordinate-sorted BAM";
  if (o.truth_sort && sharded)
    return "Error: --truth-sort cannot be combined with --world or --gpus above 1: the ranks' sorted parts would have to be merged, not "
           "concatenated";
  for (const Rule& r : rules) {
    if (all && r.is_width && r.on < 0) return std::string("Error: ") + r.flag + " needs a bin width of at least 1";
    if (all && r.on && r.needs_map && o.host_haplotypes)
      return std::string("Error: ") + r.flag + " needs the haplotypes assembled on the device (their copy lists map the reads back to the "
             "reference); it cannot be combined with --host-haplotypes";
    if (r.on && r.partial && sharded)
      return std::string("Error: ") + r.flag + " cannot be combined with --world or --gpus above 1: the ranks' partial " + r.partial +
             " would have to be summed, not concatenated";
  }
  return std::string();
}
#endif
