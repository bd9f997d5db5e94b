/* simuscop_amd.h -- C ABI of the MI355X read-sampling engine (libsimuscop_amd.so).
 *
 * The reference (SimuSCoP v1.0) has no FFI/plugin interface; its only seam on this path is the C
 * work item handed to the thread pool,
 *     threadPool->pool_add_work(&Segment::yieldReads, &chrSegs[k], n++)   lib/genome/Genome.cpp:881,949
 *     void* (*)(const void* arg)                                          lib/threadpool/ThreadPool.h:195
 * executed once per <=1 Mbp segment between generateSegSequences() (Genome.cpp:876-878) and
 * threadPool->wait() (:883).  This library replaces that whole per-chromosome block -- every
 * Segment::yieldReads call of one (population, chromosome), including Profile::predict,
 * Profile::yieldInsertSize, Segment::getFragSequence / Genome::produceFragment and the FASTQ
 * formatting -- by one batched GPU pass.  What crosses the boundary is exactly the state those
 * functions read: the Profile CDF tables, the haplotype strings, and the per-window sampling plan.
 * INTEGRATION.md shows the binding a SimuSCoP maintainer would add.
 *
 * Plain C, no torch / HIP types in signatures.  One sg_ctx per GPU; a ctx is thread-compatible
 * (use it from one host thread at a time).  All functions return SG_OK (0) or an error code;
 * sg_last_error() gives the message (the reference prints to cerr and exit(1)s instead,
 * e.g. lib/config/Config.cpp:67-70 -- the CLI layer maps a non-zero status to that behaviour).
 */
#ifndef SIMUSCOP_AMD_H
#define SIMUSCOP_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SG_OK 0
#define SG_ERR_INVALID 1     /* bad argument / call order            */
#define SG_ERR_HIP 2         /* HIP runtime error (no GPU, OOM, ...) */
#define SG_ERR_UNSUPPORTED 3 /* profile shape outside the kernels' range (bases != 4, kmer > 6 ...) */
#define SG_ERR_OVERFLOW 4    /* more than SG_MAX_EVENTS sequencing indels in one read             */
#define SG_ERR_FORMAT 5      /* FASTA without fixed-width lines (sg_reference_commit): use the host parser */

#define SG_MAX_EVENTS 32

typedef struct sg_ctx sg_ctx;

/* ---- lifetime ---------------------------------------------------------------------------- */
/* Replaces `threadPool = new ThreadPool(threads); pool_init()` (src/simuReads.cpp:63-64,
 * lib/threadpool/ThreadPool.cpp:8-51): one context per GPU instead of N pinned pthreads, and one
 * 64-bit seed instead of clock-seeded mt19937 pairs (ThreadPool.cpp:41-49).                      */
int sg_create(sg_ctx** ctx, int device, uint64_t seed);
void sg_destroy(sg_ctx* ctx);
/* Device blocks a destroyed context (or a grown buffer) gave up stay with the process and serve the next context's
 * requests of their size (the reference keeps its `new[]` arenas per run likewise: nothing of it outlives main());
 * this returns them to the runtime.  SG_BLOCK_CACHE_GB bounds what is kept (default 160, 0 = keep nothing).        */
void sg_release_cached_memory(void);
const char* sg_last_error(const sg_ctx* ctx); /* ctx may be NULL: error of a failed sg_create */
/* Run on a caller-owned HIP stream (hipStream_t passed as void*); NULL = the ctx's own stream. */
int sg_set_stream(sg_ctx* ctx, void* hip_stream);
int sg_set_seed(sg_ctx* ctx, uint64_t seed);
/* A literal 'X' in the genome.  The reference's k-mer trie files the short contexts of a read's first bases under the
 * character 'X' ("XXb", "Xbb": Profile::initKmers, lib/profile/Profile.cpp:94-101) and Profile::getKmerIndx (:220-226)
 * walks it with whatever the template holds, so an X of the genome acts as that place holder in the middle of a read
 * (on forward reads: Segment::getComplementSeq turns it into 'N', lib/segment/Segment.cpp:99).  Default 0: the same here.
 * 1 (`simuReads --strict-bases`): an X is an unknown base like any other non-ACGT character.                          */
int sg_set_strict_bases(sg_ctx* ctx, int on);

/* ---- profile tables ---------------------------------------------------------------------- */
/* The products of Profile::train(file) (lib/profile/Profile.cpp:1436-1440) exactly as the
 * reference holds them in memory: fp64 cumulative tables (Matrix<double>::getEntrance() rows,
 * Profile.cpp:1367-1434).  The library converts them to exact u32 thresholds of the reference's
 * 32-bit uniform (lib/threadpool/ThreadPool.cpp:203-207, lib/mydefine/MyDefine.cpp:176-184).   */
typedef struct sg_profile_cdf {
  int32_t n_bases;          /* config "bases" length, must be 4        Profile.cpp:1000 */
  char bases[8];            /* e.g. "ACTG"                                               */
  int32_t kmer;             /* Profile.cpp:1001                                           */
  int32_t bins;             /* Profile.cpp:1002 (already clipped to read_length, :185)    */
  int32_t read_length;      /* Profile.cpp:1003                                           */
  int32_t n_qual;           /* maxBaseQuality-minBaseQuality+1 = 94, Profile.cpp:208      */
  int32_t min_qual;         /* 33, Profile.cpp:173                                        */
  double insert_rate;       /* Profile::insertRate                                        */
  double del_rate;          /* Profile::delRate                                           */
  const double* ins_cdf;    /* insCdf  [n_ins]                         Profile.cpp:1375   */
  int32_t n_ins;
  const double* del_cdf;    /* delCdf  [n_del]                         Profile.cpp:1378   */
  int32_t n_del;
  const double* subs_cdf1;  /* subsCdf1[kmer_count][bins][n_bases]     Profile.cpp:1419   */
  const double* subs_cdf2;  /* subsCdf2 or NULL (SE / stdISize<=0)     Profile.cpp:1420-1430 */
  const double* qual_cdf;   /* qualityCdf[n_bases*n_bases][bins][n_qual] Profile.cpp:1398 */
  const double* isize_cdf;  /* iSizeCdf[n_isize] or NULL -> fixed insert size, Profile.cpp:1487 */
  int32_t n_isize;
  int32_t isize_min;        /* iSizeAlphabet[0] (alphabet is consecutive, Profile.cpp:919-922) */
  int32_t insert_size;      /* config insertSize (used when isize_cdf == NULL)            */
} sg_profile_cdf;
int sg_load_profile(sg_ctx* ctx, const sg_profile_cdf* prof);
/* The same in two steps, so that a host can convert the tables (milliseconds of integer arithmetic: draw counts of every
 * CDF entry, alias columns) on a worker thread while it streams the reference to the device: sg_profile_prepare touches no
 * device and no context; sg_load_prepared_profile uploads.  sg_profile_prepare always returns a tables object (free it);
 * on failure its code is also what sg_load_prepared_profile returns, with the message in sg_last_error. */
typedef struct sg_profile_tables sg_profile_tables;
int sg_profile_prepare(const sg_profile_cdf* prof, sg_profile_tables** out);
const char* sg_profile_tables_error(const sg_profile_tables* tables);
int sg_load_prepared_profile(sg_ctx* ctx, const sg_profile_tables* tables);
void sg_profile_tables_free(sg_profile_tables* tables);

/* ---- haplotypes of one (population, chromosome) ------------------------------------------- */
/* chain h = concatenation over the chromosome's segments, in order, of Segment::segSequences[h]
 * (lib/segment/Segment.cpp:448-458; NULL entries contribute nothing).  A fragment that runs past
 * its segment continues into the following segments' same-index haplotype
 * (Segment::getFragSequence :1085-1101 -> Genome::produceFragment, Genome.cpp:599-632): on a chain
 * that is a plain substring, clipped at the chain end.  Bytes are ASCII; letters of either case
 * get the codes sg_build_haplotypes gives them (the driver uploads upper case).                 */
int sg_upload_haplotypes(sg_ctx* ctx, int32_t n_chains, const char* const* chains, const uint64_t* lens);

/* ---- reference ingest and haplotype assembly on the device ------------------ */
/* Replaces the reference's per-segment FASTA reads (lib/fastahack/Fasta.cpp:304-334 through
 * Segment.cpp:137) and its std::string haplotype editing (Segment::generateSegSequences,
 * Segment.cpp:124-460) for callers that do not hold haplotype strings themselves:
 *   sg_reference_begin / _chunk   stream the FASTA file, as it is on disk, to the device;
 *   sg_reference_scan             offsets of the header lines ('>' at a line start), unordered;
 *   sg_reference_commit           contigs -> resident base codes (newlines dropped by index
 *                                 arithmetic, upper-cased as Segment.cpp:143); SG_ERR_FORMAT when a
 *                                 contig's lines are not of one width (fall back to host parsing
 *                                 and pass line_bases = line_width = length);
 *   sg_build_haplotypes           chains of one (population, chromosome) = copies of reference
 *                                 ranges and literal bases, then single-base patches; same device
 *                                 state afterwards as sg_upload_haplotypes.                        */
typedef struct sg_contig {
  uint64_t raw_offset;  /* file offset of the contig's first base                              */
  uint64_t length;      /* bases                                                               */
  uint32_t line_bases;  /* bases per line (.fai LINEBASES)                                     */
  uint32_t line_width;  /* bytes per line incl. the line break (.fai LINEWIDTH)                */
} sg_contig;
int sg_reference_begin(sg_ctx* ctx, uint64_t raw_bytes);
/* asynchronous on the ctx's stream: `host` must stay unchanged until sg_sync() returns */
int sg_reference_chunk(sg_ctx* ctx, uint64_t offset, const void* host, uint64_t bytes);
int sg_sync(sg_ctx* ctx);
/* bit 0 of *flags: the file has ';' comment lines (not handled by sg_reference_commit) */
int sg_reference_scan(sg_ctx* ctx, uint64_t* header_offsets, uint32_t cap, uint32_t* n_found, uint32_t* flags);
int sg_reference_commit(sg_ctx* ctx, const sg_contig* contigs, uint32_t n_contigs);

typedef struct sg_hap_piece {
  uint64_t dst;     /* offset in chain `chain`                                                   */
  uint64_t src;     /* kind 0: 0-based position on contig `contig`; kind 1: offset into literals */
  uint32_t len;
  uint32_t chain;
  uint32_t contig;
  uint32_t kind;
} sg_hap_piece;
typedef struct sg_hap_patch {
  uint64_t dst;     /* offset in chain `chain` */
  uint32_t chain;
  uint32_t base;    /* ASCII, any case         */
} sg_hap_patch;
/* Pieces must tile every chain exactly: ordered by dst, the pieces of chain c follow one another from 0 to lens[c]
 * without a gap and without an overlap.  They may come in any order, chains interleaved (a list already in dst order
 * chain by chain is checked in one pass, any other is sorted first); pieces of length 0 are allowed anywhere inside
 * their chain and source.  A piece outside its chain or its source, a gap and an overlap -- also an overlap that a gap
 * of the same size makes up for in the sum -- are SG_ERR_INVALID naming the piece or the chain, before anything is
 * launched; no range is too large to be told (offsets near 2^64 are refused like any other).  Patches apply afterwards;
 * two patches on one base leave either.                                                              */
int sg_build_haplotypes(sg_ctx* ctx, int32_t n_chains, const uint64_t* lens, const sg_hap_piece* pieces, uint64_t n_pieces,
                        const char* literals, uint64_t n_literal_bytes, const sg_hap_patch* patches, uint64_t n_patches);
/* Diagnostic read-back of the resident chains (either upload route): base codes A0 C1 T2 G3, 'N' = 4,
 * 'X' = 6 (letters in either case), any other character = 5.  A range that does not lie inside the
 * chain is SG_ERR_INVALID.                                                                         */
int sg_haplotype_codes(sg_ctx* ctx, uint32_t chain, uint64_t offset, uint64_t n, uint8_t* codes_out);

/* ---- sampling plan ------------------------------------------------------------------------ */
/* One entry per sampling window of every processed segment (Segment.cpp:675 skips segments with no
 * sequences or readCount == 0), i.e. Segment::fragStartPos / fragEndPos / hapIndxs / fragRCs
 * (Segment.h:45-49) flattened in segment order, window order.                                   */
typedef struct sg_window {
  uint64_t hap_base;  /* offset of this segment's haplotype string inside chain `chain`        */
  uint32_t chain;     /* hapIndxs[i]                                                            */
  uint32_t spos;      /* fragStartPos[i]                                                        */
  uint32_t len;       /* fragEndPos[i]-fragStartPos[i]+1                                        */
  int32_t n_reads;    /* fragRCs[i]  (PE: ceil(n/2) pairs are produced, Segment.cpp:848)        */
  uint32_t seg;       /* ordinal of the segment inside this batch                               */
  uint32_t slot_base; /* exclusive prefix sum of planned pairs over the batch's windows         */
} sg_window;

typedef struct sg_batch {
  uint32_t batch_id;          /* running index of (mixture, population, chromosome) batches      */
  int32_t paired;             /* Config::isPairedEnd()                                            */
  const char* name_prefix;    /* "@<popu>#<chr>#"  (Segment.cpp:780,809)                          */
  const sg_window* windows;
  uint64_t n_windows;
  const uint32_t* seg_size;   /* per segment: seqSize/CN (Segment.cpp:713-714), for pos%segsize   */
  const uint32_t* seg_first_window; /* per segment: index of its first window; [n_segs] = n_windows */
  uint32_t n_segs;
  /* Sharding: when a batch is split over several GPUs by runs of segments, each shard passes the
   * index of its first window / first fragment slot inside the WHOLE batch, so that every draw keeps
   * the address it has in the unsharded run (the shards' FASTQ concatenate to the 1-GPU output).
   * windows[].slot_base stays shard-local (starts at 0).  Both 0 for an unsharded batch.           */
  uint32_t first_window;
  uint32_t first_slot;
} sg_batch;
int sg_plan(sg_ctx* ctx, const sg_batch* batch);

/* ---- run ----------------------------------------------------------------------------------- */
/* Enqueue the whole pass (plan draws, indel pass, record offsets, base/quality sampling + FASTQ
 * formatting) for the planned batch.  Results stay in device memory.  A context that already holds
 * output buffers (any pass but its first) queues the pass without waiting for anything: what the
 * pass reports -- SG_ERR_OVERFLOW for a read with more than SG_MAX_EVENTS sequencing indels -- then
 * comes from the first of sg_result / sg_fetch / sg_fetch_range / sg_device_output instead; a pass
 * that failed so is gone (sg_sample runs the plan again).
 *
 * New chains (sg_upload_haplotypes, sg_build_haplotypes) or a new profile (sg_load_profile,
 * sg_load_prepared_profile) end the plan: sg_sample asks for sg_plan again.  A pass already sampled
 * keeps its text -- sg_result, sg_fetch, sg_fetch_range, sg_device_output, sg_compress,
 * sg_fetch_compressed, sg_detach_outputs, sg_emit_info and sg_emit_path go on working until the next
 * sg_plan / sg_sample -- but its rows are no longer those of the chains and the profile: the calls
 * that read them (sg_truth_reads, sg_truth_bam, sg_bamsort_pass, sg_depth_add, sg_variants_add,
 * sg_errtab_add) are refused with SG_ERR_INVALID.                                                 */
int sg_sample(sg_ctx* ctx);
/* Wait for the pass and report sizes: FASTQ bytes for mate 1 / mate 2 (0 for SE) and the number
 * of fragments actually produced (pairs for PE, reads for SE).                                   */
int sg_result(sg_ctx* ctx, uint64_t* bytes_r1, uint64_t* bytes_r2, uint64_t* n_fragments);
/* Copy the FASTQ text to host buffers (the bytes SeqWriter::write(char*,char*) would receive,
 * lib/seqwriter/SeqWriter.cpp:41-54).  host_r2 may be NULL for SE.  sg_fetch, sg_fetch_range and
 * sg_device_output wait for the pass as sg_result does: straight after sg_sample they give the
 * complete text.                                                                                 */
int sg_fetch(sg_ctx* ctx, char* host_r1, char* host_r2);
/* Partial copy for pipelined sinks: bytes [offset, offset+bytes) of mate 0/1's FASTQ text.  With a
 * destination from sg_host_alloc (pinned) the copy runs at PCIe speed.                            */
int sg_fetch_range(sg_ctx* ctx, int mate, uint64_t offset, uint64_t bytes, char* host_dst);
/* Page-locked host memory for sg_fetch / sg_fetch_range destinations.                             */
int sg_host_alloc(sg_ctx* ctx, uint64_t bytes, void** host_ptr);
int sg_host_free(sg_ctx* ctx, void* host_ptr);
/* Device pointers of the FASTQ text (valid until the next sg_sample / sg_plan).                  */
int sg_device_output(sg_ctx* ctx, void** dev_r1, void** dev_r2);

/* ---- GC-window scan (Segment::getWeightedLength byte scan, Segment.cpp:563-592) ------------- */
/* For every window [start, start+len) of chain `chain`: integer GC% = 100*GC/len, or -1 if the
 * window holds any 'N' (lib/mydefine/MyDefine.cpp:279-303).  Uses the uploaded haplotypes.       */
typedef struct sg_gc_window { uint64_t start; uint32_t chain; uint32_t len; } sg_gc_window;
int sg_gc_percent(sg_ctx* ctx, const sg_gc_window* windows, uint64_t n, int32_t* gc_out);

/* GC-bias weight of sampling windows, on the device: Segment::getWeightedLength's per-window loop
 * (lib/segment/Segment.cpp:550-641) -- GC% of the window (calculateGCPercent, lib/mydefine/MyDefine.cpp:279-303),
 * GC factor = Normal(means[gc], std) redrawn while negative (Profile::getGCFactor, lib/profile/Profile.cpp:1507-1517),
 * weight = factor / frag_size for a window of exactly frag_size bases when full_tile_form is set (Segment.cpp:576,586),
 * else factor * len / frag_size^2 (:615).  The normal variate is addressed (Philox kind GC: window ordinal, attempt,
 * segment ordinal, ctx24 = population << 16 | chromosome) and read off the quantile table of the model -- n_cells + 1
 * knots of the standard normal's quantile function, cell = draw >> (32 - lg_cells), linear inside the cell -- in three
 * rounded fp64 operations, so the weights are bit for bit those of the host evaluation of the same table.
 * weights_out / gc_out (either may be NULL) receive n values each. */
typedef struct sg_gc_model {
  const double* means;      /* [101] */
  double std;
  const double* quantiles;  /* [2^lg_cells + 1] */
  uint32_t lg_cells;
  uint32_t frag_size;
  int32_t full_tile_form;
  uint32_t ctx24;
} sg_gc_model;
int sg_window_weights(sg_ctx* ctx, const sg_gc_window* windows, const uint32_t* seg_ord, const uint32_t* win_ord, uint64_t n,
                      const sg_gc_model* model, double* weights_out, int32_t* gc_out);

/* ---- sampling plan made on the device (whole-genome runs without targets) ------------------- */
/* The reference tiles every haplotype string of a segment into frag_size windows (Segment::getWeightedLength,
 * Segment.cpp:566-590), weighs them (sg_window_weights), sums the weights per segment, chromosome and genome
 * (Genome::setReadCounts, Genome.cpp:783-825) and hands every window fragWeights[i] * readCount / totalWL reads,
 * the remainder going to the segment's first window (Segment::setReadCount, Segment.cpp:462-476).  Here the host
 * only keeps per-SEGMENT data; the windows exist on the device alone:
 *   sg_windows_build   tiles the generators (one per haplotype string of a segment, in the reference's window order),
 *                      computes GC%, GC factor and weight of every window and the weight sum of every segment (summed
 *                      in window order, like the reference's loop); the weights stay in the context under `store_id`;
 *   sg_plan_windows    for the segments that got reads: per-window read counts, the remainder rule, planned pairs and
 *                      their prefix sum -- the sg_window table of the batch, on the device; reports the planned
 *                      fragments of every active segment (the host cuts pieces / shards by them);
 *   sg_plan_range      makes a run [a0, a1) of those active segments the current batch (what sg_plan does for a
 *                      host-made table); first_window / first_slot keep the draws' batch-wide addresses.        */
typedef struct sg_window_gen {
  uint64_t hap_base;      /* offset of the haplotype string inside chain `chain`                               */
  uint64_t hap_len;       /* its length; windows = ceil(hap_len / frag_size), the last one shorter               */
  uint32_t chain;
  uint32_t seg;           /* sg_windows_build: segment ordinal in the chromosome; sg_plan_windows: index in `active` */
  uint64_t first_window;  /* sg_plan_windows: index of the generator's first window in the numbering of sg_windows_build */
} sg_window_gen;
int sg_windows_build(sg_ctx* ctx, uint32_t store_id, const sg_window_gen* gens, uint64_t n_gens, uint32_t n_segs,
                     const sg_gc_model* model, double* seg_weight_out, uint64_t* n_windows_out);
typedef struct sg_active_seg {
  int64_t reads;          /* Segment::readCount                                                                */
  double weight;          /* the segment's weight sum (seg_weight_out of sg_windows_build)                     */
  uint32_t seg_size;      /* seqSize / CN (Segment.cpp:713-714)                                                */
  uint32_t pad;
} sg_active_seg;
int sg_plan_windows(sg_ctx* ctx, uint32_t store_id, const sg_window_gen* gens, uint64_t n_gens, const sg_active_seg* active,
                    uint32_t n_active, uint32_t frag_size, uint32_t batch_id, int32_t paired, const char* name_prefix,
                    uint64_t* slots_out /* [n_active] */, uint64_t* n_windows_out);
int sg_plan_range(sg_ctx* ctx, uint32_t a0, uint32_t a1);
void sg_windows_drop(sg_ctx* ctx);  /* frees every window-weight store of the context */


/* ---- instrumentation ----------------------------------------------------------------------- */
#define SG_K_PLAN 0
#define SG_K_NAMEBASE 1
#define SG_K_INDEL 2
#define SG_K_SCAN 3
#define SG_K_EMIT 4       /* header + main emit kernel                                   */
#define SG_K_EMIT_SLOW 5  /* emit_slow_kernel: the items queued for the generic item code */
#define SG_K_COUNT 6
/* ---- block-gzip sink ------------------------------------------------------------ */
/* After sg_result: compress the FASTQ text of the pass on the device into BGZF blocks -- independent
 * gzip members of 32 KB of text each (RFC 1952 with the 'BC' extra field), one dynamic-Huffman DEFLATE block
 * of literals and matches (copies of earlier text of the member, runs), one pair of codes per mate and pass.  Concatenated in order (and closed with sg_bgzf_eof) they form
 * a .fq.gz file that `zcat` turns back into exactly the text sg_fetch returns.  SeqWriter::write
 * (lib/seqwriter/SeqWriter.cpp:41-54) has no such mode: additive.                                   */
int sg_compress(sg_ctx* ctx, uint64_t* gz_bytes_r1, uint64_t* gz_bytes_r2);
int sg_fetch_compressed(sg_ctx* ctx, int mate, uint64_t offset, uint64_t bytes, void* host_dst);
/* The same compressor on text in host memory, for tests and for callers that hold text of their own: `bytes` bytes of
 * `text` -> ceil(bytes / 32768) BGZF members in `out`, in order, without the EOF member of sg_bgzf_eof; *out_bytes = how
 * many bytes they take (SG_ERR_OVERFLOW when out_cap is too small: call again).  bytes = 0 gives *out_bytes = 0.  Any byte
 * value is legal in the text, 0x00 and 0xFF included; no sampling pass is needed and none is disturbed.  The text is copied
 * before the call returns.  The same text gives the same members, call after call.                   */
int sg_deflate_bgzf(sg_ctx* ctx, const void* text, uint64_t bytes, void* out, uint64_t out_cap, uint64_t* out_bytes);
/* ---- detached outputs: drain one batch while the next is sampled ------------------------------------- */
/* After sg_result (and sg_compress, if wanted) the FASTQ text -- and its BGZF form -- can be taken out of
 * the context: the handle owns the device buffers and a copy stream of its own, so sg_outputs_fetch may
 * run on another host thread while the context plans and samples the next batch into fresh buffers
 * (the reference's workers flush their 50 MB buffers through one mutex instead, Segment.cpp:834-846,
 * SeqWriter.cpp:49-54).  sg_release_outputs hands the buffers back to the context for reuse; it and
 * sg_detach_outputs are context calls (one thread at a time), sg_outputs_* are not.                  */
typedef struct sg_outputs sg_outputs;
int sg_detach_outputs(sg_ctx* ctx, sg_outputs** out);
int sg_outputs_sizes(const sg_outputs* o, uint64_t text_bytes[2], uint64_t gz_bytes[2]);
int sg_outputs_fetch(sg_outputs* o, int mate, int compressed, uint64_t offset, uint64_t bytes, void* host_dst);
const char* sg_outputs_last_error(const sg_outputs* o);
int sg_release_outputs(sg_ctx* ctx, sg_outputs* o);

/* the 28-byte empty BGZF block that ends a file */
int sg_bgzf_eof(uint8_t out[28]);
/* Host-only view of the code construction, for tests: from the histograms of the literal / length symbols
 * (286; [256] = end-of-block) and of the distance symbols (30), the code lengths and (bit-reversed) codes of both
 * alphabets, the length half of a match token per match length 3..258 (index = length) (code + extra bits in the low 24 bits, bit count
 * in the top 8) and the member prefix (gzip header with BSIZE = 0 + dynamic block header) as LSB-first 32-bit words.
 * Returns the number of prefix bits, 0 if `cap` is too small. */
uint32_t sg_deflate_plan(const uint64_t lit_counts[286], const uint64_t dist_counts[30], uint8_t lit_lens[286], uint32_t lit_codes[286],
                         uint8_t dist_lens[30], uint32_t dist_codes[30], uint32_t len_tokens[260], uint32_t* prefix_words, uint32_t cap);

/* ---- truth alignments: where every read of a pass came from, as BAM records (simuReads --truth-bam) ------------------
 * The reference has no such output (Segment::yieldReads keeps pos % segsize in the read's name and nothing else,
 * Segment.cpp:780); its trainer reads alignments (Profile::processRead, lib/profile/Profile.cpp:228-510), and these
 * records are alignments it can read.  Additive: a context that never calls sg_truth_map launches no kernel of this
 * part and holds no device memory for it.
 *
 * The rule (sg_truth_align; host only, no context): a read's template is tmpl_len bases of its chain from tmpl_off on, in
 * chain direction -- the fragment's first L bases for a forward read, its last L for a reverse read.  Walked over the
 * chain's pieces: a reference piece (kind 0) gives M, a literal piece (kind 1) I; a forward gap between consecutive
 * reference pieces of one contig gives D, or N when a segment's haplotype string began in between (seg_first); any other
 * joint (the position goes back, the contig changes) ends the alignment and the rest of the template is S.  The
 * sequencing events (ev_pack form: j | len << 16 | deletion << 31, ascending and apart, j + len <= tmpl_len for a
 * deletion) are in read direction: index j counts from the template's chain end for a reverse read.  An insertion puts
 * its bases behind template base j (I; S inside a clipped part), a deletion takes bases [j, j + len) away: D for a base
 * that was M, nothing for a literal or clipped base.  Then: equal neighbours merge; what lies in front of the first and
 * behind the last M loses its D / N and becomes one S; *pos0 is the 0-based position of the first M base.  The
 * operations (len << 4 | op, op 0 M 1 I 2 D 3 N 4 S) are in reference direction.  A read without an M base is unmapped:
 * *n_ops = 0, *contig = -1.  SG_ERR_OVERFLOW when `cap` is too small (*n_ops says how many there are).
 *   sg_truth_map     after sg_build_haplotypes, with the pieces of that call (the engine keeps no copy of them for a
 *                    caller that never asks): seg_first[i] = 1 when piece i is the first piece of a segment's haplotype
 *                    string; ref_ids[c] = BAM refID of contig c (NULL: c).  Sorts the copy list by (chain, dst) and
 *                    puts it on the device.  The pieces of a chain must tile it, none of length 0; a refused call
 *                    leaves an earlier map as it was.  The chains of sg_upload_haplotypes have no copy list:
 *                    SG_ERR_INVALID, as from every call below without a map
 *   sg_truth_pieces  the sorted pieces of one chain, as sg_truth_align takes them (contig: the one of sg_hap_piece)
 *   sg_truth_reads   after sg_result: where reads [first_slot, first_slot + n) of mate 0 / 1 came from
 *   sg_truth_bam     after sg_result, before sg_detach_outputs: the BAM records (SAMv1 section 4.2, no optional fields: see sg_truth_bam_tags) of
 *                    the pass's reads in FASTQ order -- slot by slot, mate 1 then mate 2; unused slots give nothing --
 *                    and their BGZF members (the compressor of sg_compress; no header, no EOF block).  QNAME is the FASTQ
 *                    name without '@' and "/1", SEQ / QUAL the FASTQ's, turned round for a reverse read; FLAG 0 / 16 (SE),
 *                    99 / 147 (PE), MAPQ 60; RNEXT / PNEXT the mate's place, TLEN the span of the pair's M bases (positive
 *                    for the leftmost mate).  An unmapped read: flag 0x4 without 0x10, MAPQ 0, no CIGAR, at its mate's
 *                    place (-1 / -1 without one); its mate gets 0x8 and loses 0x2, TLEN 0 for both.
 *   sg_fetch_truth   bytes [offset, offset + bytes) of the record stream (compressed = 0) or of its BGZF members (1)
 *   sg_truth_info    records and unmapped records of the last sg_truth_bam
 *
 * Tags (simuReads --truth-tags; the rule: DESIGN.md "Truth tags").  Opt-in: sg_truth_bam makes the records above and
 * launches the kernels it always has.
 *   sg_truth_bam_tags  sg_truth_bam with optional fields behind the qualities, `tags` a mask of SG_TAG_NM | SG_TAG_MD |
 *                    SG_TAG_XE (any subset; 0 is sg_truth_bam), in this order: NM:I on a mapped record (mismatching M
 *                    bases + I + D bases), XE:I on a record whose template lies in its chain, mapped or not (the read's
 *                    sequencing errors against the haplotype it was cut from: what it adds to Q.errors, I.bases and D.bases
 *                    of the true error counts), MD:Z on a mapped record unless its text is longer than max_md bytes (only a
 *                    long variant deletion inside the read makes one: the record keeps NM and XE and is counted in
 *                    md_dropped).  block_size includes the tags.  The reference letter of MD is A C G T for those codes
 *                    and N for anything else (the codes keep no IUPAC letter: the one difference from `samtools calmd`); a
 *                    SEQ letter matches iff it equals it and is one of A C G T.  Same limits as sg_truth_bam, and templates
 *                    of at most (max_md - 257) / 2 bases (SG_ERR_UNSUPPORTED); NM or MD without the codes of
 *                    sg_reference_commit: SG_ERR_INVALID.  A read whose events or operations do not end at its length, or
 *                    an alignment past its contig's end, fails the call (SG_ERR_INVALID)
 *   sg_truth_tag_info  of the last sg_truth_bam / sg_truth_bam_tags: records with each tag, the sums of NM and XE, MD texts
 *                    dropped, tag bytes, and max_md
 *   sg_truth_tags    the rule for one record (host only, no context).  NM / MD: cigar (len << 4 | op), SEQ in BAM
 *                    orientation, ref_codes = the contig's base codes (A0 C1 T2 G3, N 4, other 5, X 6) from POS on; the
 *                    first min(md_len, md_cap) bytes of the text go to md (no NUL), a text longer than md_cap is dropped
 *                    (*present lacks SG_TAG_MD).  n_ops == 0: an unmapped record, neither.  XE: tmpl_codes = the template's
 *                    chain codes in chain direction (NULL: the template does not lie in its chain, no XE), reverse, the
 *                    events (ev_pack form, read direction) and the read in FASTQ orientation.  *present = the tags the
 *                    record gets                                                                                     */
#define SG_TAG_NM 1u
#define SG_TAG_MD 2u
#define SG_TAG_XE 4u
typedef struct sg_truth_tag_counts {
  uint64_t n_nm, n_md, n_xe;   /* records with the tag                                           */
  uint64_t nm_sum, xe_sum;
  uint64_t md_dropped;         /* mapped records whose MD text was longer than max_md            */
  uint64_t tag_bytes;
  uint64_t max_md;
} sg_truth_tag_counts;
typedef struct sg_truth_piece {
  uint64_t dst;        /* offset in the chain                                                    */
  uint64_t src;        /* kind 0: 0-based position on contig `contig`                            */
  uint32_t len;
  uint32_t contig;
  uint32_t kind;       /* 0 reference, 1 literal                                                 */
  uint32_t seg_first;  /* 1: first piece of a segment's haplotype string                         */
} sg_truth_piece;
int sg_truth_align(const sg_truth_piece* pieces, uint64_t n_pieces, uint64_t tmpl_off, uint32_t tmpl_len, int reverse,
                   const uint32_t* events, uint32_t n_events, int32_t* contig, int64_t* pos0, uint32_t* cigar, uint32_t cap,
                   uint32_t* n_ops);
typedef struct sg_truth_read {
  uint32_t live;       /* 0: unused slot                                                         */
  uint32_t chain;
  uint32_t reverse;
  uint32_t read_len;   /* bases of the read (template length + inserted - deleted)               */
  uint64_t tmpl_off;   /* chain-local offset of the template's first base                        */
  uint32_t n_events;   /* from the read's row, not from the events buffer                        */
  uint32_t inside;     /* 0: the template does not lie inside its chain (the record is unmapped) */
  uint32_t events[SG_MAX_EVENTS];
} sg_truth_read;
int sg_truth_map(sg_ctx* ctx, const sg_hap_piece* pieces, const uint8_t* seg_first, uint64_t n_pieces, const int32_t* ref_ids,
                 uint32_t n_ref_ids);
int sg_truth_pieces(sg_ctx* ctx, uint32_t chain, sg_truth_piece* out, uint64_t cap, uint64_t* n);
int sg_truth_reads(sg_ctx* ctx, int mate, uint32_t first_slot, uint32_t n, sg_truth_read* out);
int sg_truth_bam(sg_ctx* ctx, uint64_t* record_bytes, uint64_t* bgzf_bytes);
int sg_fetch_truth(sg_ctx* ctx, int compressed, uint64_t offset, uint64_t bytes, void* host_dst);
int sg_truth_info(sg_ctx* ctx, uint64_t* records, uint64_t* unmapped);
int sg_truth_bam_tags(sg_ctx* ctx, uint32_t tags, uint64_t* record_bytes, uint64_t* bgzf_bytes);
int sg_truth_tag_info(sg_ctx* ctx, sg_truth_tag_counts* out);
int sg_truth_tags(const uint32_t* cigar, uint32_t n_ops, const char* seq, uint32_t seq_len, const uint8_t* ref_codes, uint64_t n_ref,
                  uint32_t md_cap, const uint8_t* tmpl_codes, uint32_t tmpl_len, int reverse, const uint32_t* events, uint32_t n_events,
                  const char* read, uint32_t read_len, uint32_t* present, uint32_t* nm, char* md, uint32_t* md_len, uint32_t* xe);

/* ---- the truth BAM in coordinate order (simuReads --truth-sort) -------------------------------------
 * The order: key of a record = (refID as u32) << 32 | (POS as u32), from the record's own fields, so an unmapped read
 * placed at its mate sorts at its mate's place and an unplaced one (-1 / -1) has the largest key and sorts last; ties
 * keep the order of the unsorted stream (a stable sort).  The records themselves are the bytes of sg_truth_bam_tags.
 * Opt-in: a context that never calls these launches no kernel of this part and holds no memory for it.
 *   sg_bamsort_pass   sg_truth_bam_tags (same preconditions, limits and failures) with the record stream in key order and
 *                     uncompressed: sizing kernels, keys of the live records, a stable radix sort on the device, offsets,
 *                     then the record kernels unchanged.  *records = records made.  sg_truth_info and sg_truth_tag_info
 *                     describe it; sg_fetch_truth reads its stream too (no members: bgzf bytes 0)
 *   sg_bamsort_merge  n_runs slices in host memory, run r holding n[r] records of lens[r][i] bytes back to back in
 *                     records[r] (record_bytes[r] in all) with keys[r][i]: uploads them in run order, sorts the
 *                     concatenation stably by key, gathers the records and compresses the stream (BGZF members as
 *                     sg_deflate_bgzf makes them, no EOF block).  Runs with ascending keys are what a merge expects, but
 *                     any keys are sorted correctly; n_runs = 0 and empty runs are legal.  Needs no pass, no profile and
 *                     no piece map, and disturbs none.  Fewer than 2^32 records; lengths that do not add up to
 *                     record_bytes[r]: SG_ERR_INVALID.  The slices are the caller's again on return
 *   sg_bamsort_index  keys and lengths, in output order, of the last sg_bamsort_pass or sg_bamsort_merge: *n = records;
 *                     with both arrays NULL only that, else SG_ERR_OVERFLOW when cap < *n
 *   sg_bamsort_fetch  bytes [offset, offset + bytes) of that call's record stream (compressed = 0) or of a merge's BGZF
 *                     members (1; a pass has none: SG_ERR_INVALID)
 * SG_BAMSORT_TILE: records one block of the sort takes (nothing a caller has to respect; the tests size their cases by it). */
#define SG_BAMSORT_TILE 1024
int sg_bamsort_pass(sg_ctx* ctx, uint32_t tags, uint64_t* record_bytes, uint64_t* records);
int sg_bamsort_merge(sg_ctx* ctx, uint32_t n_runs, const void* const* records, const uint64_t* record_bytes, const uint64_t* const* keys,
                     const uint32_t* const* lens, const uint64_t* n, uint64_t* out_bytes, uint64_t* bgzf_bytes);
int sg_bamsort_index(sg_ctx* ctx, uint64_t* keys_out, uint32_t* lens_out, uint64_t cap, uint64_t* n);
int sg_bamsort_fetch(sg_ctx* ctx, int compressed, uint64_t offset, uint64_t bytes, void* host_dst);

/* ---- the BAI index of the sorted truth BAM (simuReads --truth-index) --------------------------------
 * The index is stated once, in csrc/sg_bamindex.h.  A call indexes the records of one compressed text while the text and
 * the member offsets of its compression are still on the device; the host joins the calls' chunk rows and serialises
 * (simu_bai_build, host/simulate.h).  Opt-in: a context that never calls these launches no kernel of this part and
 * holds no memory for it.
 *   sg_bamindex_begin   a stem starts: n_ref references of ref_len[] bases; the linear index (the sum of ceil(len / 16384)
 *                       cells, all ~0) and the counts are reset.  A length above 2^29: SG_ERR_UNSUPPORTED, and the
 *                       index of an earlier sg_bamindex_begin stays as it was
 *   sg_bamindex_add     indexes the records of the context's latest compression, whose first member lies at file_offset
 *                       of the BAM file.  source SG_BAMINDEX_MERGE: the output of the last sg_bamsort_merge, whose
 *                       lengths and offsets are on the device (lens NULL, skip 0).  SG_BAMINDEX_DEFLATE: the text of the
 *                       last sg_deflate_bgzf; lens[n] are the lengths of the records that start in it, the first at
 *                       `skip` (the bytes in front belong to a record begun in an earlier text).  Only the last may run
 *                       past the text: it is kept on the device and indexed as the first record of the next call, which
 *                       must be a SG_BAMINDEX_DEFLATE one whose skip is the record's rest.  *n_chunks = chunk rows of
 *                       the call, *first_voff = the start offset of its first record (~0: it indexed none).  A source
 *                       that is not the latest compression, a record that does not parse or lies outside its reference:
 *                       SG_ERR_INVALID; after a failure of the kernels the stem's index is void (sg_bamindex_begin again)
 *   sg_bamindex_chunks  the chunk rows of the last sg_bamindex_add, grouped by key = refID << 32 | bin, keys ascending,
 *                       file order within a key; the chunk that ends the call has end = ~0 (the caller closes it with the
 *                       next call's first_voff, or with the end-of-file block's offset << 16).  rows NULL: only *n
 *   sg_bamindex_finish  the stem's linear index (`cap` cells of room; untouched windows are ~0, simu_bai_build fills
 *                       them) and counts[3 n_ref + 1]: per reference records without 0x4, records with 0x4, the
 *                       smallest start offset (~0: no record); then the records with refID -1
 *   sg_bamindex_end     gives the part's memory back                                                                  */
#define SG_BAMINDEX_MERGE 0
#define SG_BAMINDEX_DEFLATE 1
typedef struct sg_bai_chunk {
  uint64_t key, beg, end;
} sg_bai_chunk;
int sg_bamindex_begin(sg_ctx* ctx, uint32_t n_ref, const uint64_t* ref_len);
int sg_bamindex_add(sg_ctx* ctx, int source, uint64_t file_offset, uint64_t skip, const uint32_t* lens, uint64_t n, uint64_t* n_chunks,
                    uint64_t* first_voff);
int sg_bamindex_chunks(sg_ctx* ctx, sg_bai_chunk* rows, uint64_t cap, uint64_t* n);
int sg_bamindex_finish(sg_ctx* ctx, uint64_t* linear, uint64_t cap, uint64_t* counts);
int sg_bamindex_end(sg_ctx* ctx);

/* ---- true coverage: the depth the reads of all passes really laid down (simuReads --truth-depth) -------------------
 * Coverage adds up, so it needs no sort: one int32 difference array over the reference (len + 1 slots per contig, 4
 * bytes per reference base) takes +1 / -1 for every M run of every read's true alignment (the rule above), pass after
 * pass, population after population; a prefix sum at the end gives the depth.  A read counts at the reference positions
 * of its M operations only (D, N, I, S and unmapped reads add nothing; both mates count where they overlap): the
 * default of `samtools depth`.  Additive: a context that never calls sg_depth_begin launches no kernel of this part and
 * holds no device memory for it; every call below before sg_depth_begin is SG_ERR_INVALID, and so is a contig index out
 * of range.  Contigs are shorter than 2^32 - 8 bases (SG_ERR_UNSUPPORTED), depths are taken modulo 2^32.
 *   sg_depth_begin      allocates and zeroes the array for contigs of these lengths (a second call replaces the state);
 *                       SG_ERR_HIP with the size in the message when the device cannot hold it
 *   sg_depth_add        after sg_result (and sg_truth_map): adds the current pass's reads; *m_bases = M bases added.  A
 *                       run outside its contig is not written and the call fails with SG_ERR_INVALID.  Refuses a pass
 *                       that ran under SG_DIAG, like sg_truth_bam
 *   sg_depth_add_spans  adds spans [start, end) of contigs, given by the host; a span out of range or with start > end:
 *                       SG_ERR_INVALID, and nothing is added
 *   sg_depth_bins       sums[k] = 64-bit sum of the depths of bases [k * bin, min((k + 1) * bin, LN)); *n = number of bins.
 *                       cap == 0 gives the count alone; SG_ERR_OVERFLOW when 0 < cap < *n
 *   sg_depth_runs       maximal runs of equal depth as (start, depth) rows in order (a run ends where the next starts,
 *                       the last at LN); cap as above
 *   sg_depth_fetch      per-base depths of bases [first, first + n)
 *   sg_depth_reset      zeroes the array and the count, keeps the buffers
 *   sg_depth_info       contigs, M bases added since sg_depth_begin / sg_depth_reset, bases per tile of the finishing pass
 *   sg_depth_end        frees everything                                                                              */
typedef struct sg_depth_run {
  uint32_t start;
  uint32_t depth;
} sg_depth_run;
int sg_depth_begin(sg_ctx* ctx, const uint64_t* contig_len, uint32_t n_contigs);
int sg_depth_add(sg_ctx* ctx, uint64_t* m_bases);
int sg_depth_add_spans(sg_ctx* ctx, const uint32_t* contig, const uint64_t* start, const uint64_t* end, uint64_t n);
int sg_depth_bins(sg_ctx* ctx, uint32_t contig, uint64_t bin, uint64_t* sums, uint64_t cap, uint64_t* n);
int sg_depth_runs(sg_ctx* ctx, uint32_t contig, sg_depth_run* rows, uint64_t cap, uint64_t* n);
int sg_depth_fetch(sg_ctx* ctx, uint32_t contig, uint64_t first, uint64_t n, uint32_t* depth);
int sg_depth_reset(sg_ctx* ctx);
int sg_depth_info(sg_ctx* ctx, uint32_t* n_contigs, uint64_t* m_bases, uint32_t* tile);
int sg_depth_end(sg_ctx* ctx);

/* ---- true allele counts: per variant, the reads that cover the site and those that carry the allele
 * (simuReads --truth-variants) ----
 * A read counts by the haplotype bases its template was cut from (its read-length chain bases; sequencing errors,
 * strand and mate play no part), both mates of a pair as reads.  Label every template base by its piece (the map of
 * sg_truth_map): R(c, x) in a reference piece, Lit in a literal one.  A row (contig c, position p, 0-based):
 *   kind 0, SNV, allele a      every base R(c, p): total; alt when the chain's base code there is a's
 *   kind 1, insertion, len k   every base R(c, p) with a template base behind it: total when that is R(c, p + 1); total
 *                              and alt when it is the first base of a literal piece of exactly k bases that lies inside
 *                              the template and has a template base behind it
 *   kind 2, deletion, len k    (bases [p, p + k), p >= 1) every base R(c, p - 1) with a template base behind it: total
 *                              when that is R(c, p); total and alt when it is R(c, p + k)
 * Counts are per occurrence, uint32, modulo 2^32, and add up over passes.  Additive: a context that never calls
 * sg_variants_begin launches no kernel of this part and holds no device memory for it; every call below before
 * sg_variants_begin is SG_ERR_INVALID.
 *   sg_variants_begin   rows sorted by (contig, pos, kind, allele, len), no two alike; kind 0: allele an ASCII letter,
 *                       len 0; kinds 1, 2: len >= 1, allele 0; pos < 2^32; anything else: SG_ERR_INVALID.  Uploads the
 *                       table and zeroes the counters; a second call replaces the state
 *   sg_variants_add     after sg_result and sg_truth_map: counts the current pass's reads; *reads_hit = reads with at
 *                       least one count, *hits = counts of total.  Refuses a pass that ran under SG_DIAG and a context
 *                       without a piece map, like sg_depth_add
 *   sg_variants_counts  out[i] = {alt, total} of row i; *n = rows; cap == 0 gives the count alone; SG_ERR_OVERFLOW when
 *                       0 < cap < *n
 *   sg_variants_reset   zeroes the counters, keeps the buffers
 *   sg_variants_info    rows, and reads_hit / hits summed since sg_variants_begin / sg_variants_reset
 *   sg_variants_end     frees everything
 *   sg_variant_observe  host only, no context: the same rule for one template.  `pieces` are the chain's pieces in
 *                       offset order, the template tmpl_len bases from tmpl_off on, codes[i] the chain's base code
 *                       (sg_haplotype_codes form: A0 C1 T2 G3) of template base i; rows as for sg_variants_begin.  One
 *                       (hit_row, hit_alt) entry per count of total, in walk order; *n_hits = their number (all are
 *                       counted, the first cap are written)                                                          */
typedef struct sg_variant {
  uint32_t contig;   /* BAM refID */
  uint32_t kind;     /* 0 SNV, 1 insertion, 2 deletion */
  uint64_t pos;      /* 0-based */
  uint32_t len;
  uint32_t allele;
} sg_variant;
int sg_variants_begin(sg_ctx* ctx, const sg_variant* rows, uint64_t n);
int sg_variants_add(sg_ctx* ctx, uint64_t* reads_hit, uint64_t* hits);
int sg_variants_counts(sg_ctx* ctx, uint32_t* out, uint64_t cap, uint64_t* n);
int sg_variants_reset(sg_ctx* ctx);
int sg_variants_info(sg_ctx* ctx, uint64_t* n_rows, uint64_t* reads_hit, uint64_t* hits);
int sg_variants_end(sg_ctx* ctx);
int sg_variant_observe(const sg_truth_piece* pieces, uint64_t n_pieces, const uint8_t* codes, uint64_t tmpl_off, uint32_t tmpl_len,
                       const sg_variant* rows, uint64_t n_rows, uint32_t* hit_row, uint8_t* hit_alt, uint64_t cap, uint64_t* n_hits);

/* ---- true error counts: per mate, cycle and reported quality, how many bases were really wrong
 * (simuReads --truth-errors) ----
 * A read is compared with its template, the read-length haplotype bases it was cut from, not with the reference, so a
 * variant allele is no error and no piece map is needed.  In read direction the template is T'[0 .. L): the chain codes
 * (sg_haplotype_codes form: A0 C1 T2 G3, N 4, other 5, X 6) as they stand for a forward read, in reverse order and
 * complemented (code ^ 2 below 4) for a reverse one.  The read's events (ev_pack words, read direction, ascending) are
 * laid over it as Profile::predict applies them.  Walk j from 0 with read position r = 0:
 *   deletion of k at j (k clipped to L - j)   no read base; row D(mate, j): events += 1, bases += k; j += k
 *   otherwise read base r pairs with T'[j]    T'[j] in A/C/G/T: bases++ at (mate, r, quality), errors++ as well when the
 *                                             read's letter differs (an N is an error), S(mate, T'[j], letter)++;
 *                                             else other++ at (mate, r, quality); r++, j++
 *   insertion of k behind that base           the next k read bases: inserted++ at their (mate, r, quality), no verdict;
 *                                             row I(mate, j): events += 1, bases += k; r += k
 * At the end r must be the read's length.  Quality is the text byte minus 33; mate is 0 / 1 (0 for SE).  A live read
 * whose template does not lie in its chain counts nowhere (`skipped`).  The table is flat, uint64, in this order:
 *   Q [2][cycles][n_qual][4]   bases, errors, other, inserted; quality column q is quality qual_lo + q
 *   S [2][4][5]                from A C T G, to A C T G N
 *   I [2][L][2], D [2][L][2]   events, bases
 * 8 * cycles * n_qual + 40 + 8 * L cells, L the profile's read length.  Additive: a context that never calls
 * sg_errtab_begin launches no kernel of this part and holds no device memory for it; every call below before
 * sg_errtab_begin is SG_ERR_INVALID.
 *   sg_errtab_begin     after a profile is loaded; cycles in [L, 65535] (L plus what SG_MAX_EVENTS insertions can add),
 *                       n_qual in [1, 128], qual_lo + n_qual < 224; allocates and zeroes (a second call replaces the state)
 *   sg_errtab_add       after sg_result: counts the current pass's reads; *bases / *errors = what it added to those two
 *                       columns.  Refuses a pass that ran under SG_DIAG.  A read whose events do not end at its length
 *                       or lie outside its template (SG_ERR_INVALID), a read longer than `cycles` (SG_ERR_OVERFLOW) and a
 *                       quality byte outside the range (SG_ERR_INVALID; that base alone) are not counted and fail the
 *                       call.  A failed call adds nothing to the sums and returns no counts; the table may hold a part of
 *                       the pass and is undefined until sg_errtab_reset
 *   sg_errtab_counts    copies the table out; *n = cells; cap == 0 gives the size alone; SG_ERR_OVERFLOW when 0 < cap < *n
 *   sg_errtab_reset     zeroes the table and the sums, keeps the buffer
 *   sg_errtab_info      sizes, sums since sg_errtab_begin / sg_errtab_reset, and how the kernel stages the table
 *   sg_errtab_end       frees everything
 *   sg_errtab_observe   host only, no context: the same rule for one read, added into `table` (`cells` must be the
 *                       size above for tmpl_len = L).  codes[i] is the chain's code of template base i in chain
 *                       direction.  A refused read (as for sg_errtab_add; also a quality byte below 33 + qual_lo, an
 *                       event of length 0 or out of order) adds nothing                                              */
typedef struct sg_errtab_shape {
  uint32_t cycles, qual_lo, n_qual, tmpl_len;
  uint64_t cells;
  uint64_t bases, errors;   /* sums of the two columns over both mates */
  uint64_t skipped, reads;  /* live reads outside their chain; reads counted */
  uint32_t win_cycles;      /* cycles a workgroup stages in LDS, ... */
  uint32_t lds_bytes;       /* ... and the bytes that takes */
} sg_errtab_shape;
int sg_errtab_begin(sg_ctx* ctx, uint32_t cycles, uint32_t qual_lo, uint32_t n_qual);
int sg_errtab_add(sg_ctx* ctx, uint64_t* bases, uint64_t* errors);
int sg_errtab_counts(sg_ctx* ctx, uint64_t* out, uint64_t cap, uint64_t* n);
int sg_errtab_reset(sg_ctx* ctx);
int sg_errtab_info(sg_ctx* ctx, sg_errtab_shape* out);
int sg_errtab_end(sg_ctx* ctx);
int sg_errtab_observe(const uint8_t* codes, uint32_t tmpl_len, int reverse, const uint32_t* events, uint32_t n_events, const char* bases,
                      const char* quals, uint32_t read_len, uint32_t mate, uint32_t cycles, uint32_t qual_lo, uint32_t n_qual, uint64_t* table,
                      uint64_t cells);

/* When enabled, HIP events bracket every kernel of sg_sample on the ctx's stream;
 * sg_kernel_times() then returns the last pass's per-kernel milliseconds (after sg_result).     */
int sg_set_profiling(sg_ctx* ctx, int enable);
int sg_kernel_times(sg_ctx* ctx, float ms[SG_K_COUNT]);
/* Diagnostics of the last pass (after sg_result): items the straight-line emit kernel handed to the
 * generic item code (windows holding a non-ACGT base, reads with >= 2 sequencing indels), and whether
 * their queue overflowed so that the whole batch was emitted again by the generic kernel.  Results
 * are identical either way (Profile::predict, Profile.cpp:1520-1650 has one code path).          */
int sg_emit_info(sg_ctx* ctx, uint64_t* queued_items, int* requeued);
/* ---- profile training: what Profile::train gathers from the reads (lib/profile/Profile.cpp:1442-1484) ----
 * Lines of `samtools view` text (the reference reads them through popen, Profile.cpp:1448-1462) go through
 * Profile::processRead (:228-510) in file order, chunk by chunk: the filters of :262-279, Profile::countGC (:512-703: the
 * window whose reads are being counted; it turns reads away and opens windows), the CIGAR walk with its insertion /
 * deletion length counts (:290-382; events the VCF knows are not counted, only a single nM reaches the matrices),
 * subsDist1 / subsDist2 / kmersDist (:399-442), iSizeDist (:444-451), qualityDist (:453-481).  The reference bases come from
 * the contigs committed with sg_reference_commit (upper-cased, Genome.cpp:529); `contig_keys` names them in that order as the
 * FASTA index does (first token, chr / chrom prefix stripped, Fasta.cpp:58-69).
 *   sg_train_begin   tables zeroed, targets and known variants staged (refSequence / altSequence of Genome.cpp:466-475)
 *   sg_train_feed    one chunk of WHOLE lines, in file order; state is carried from chunk to chunk (once the cap of
 *                    Profile::processRead has been reached, further chunks are ignored, as the reference stops reading).
 *                    The text is copied before the call returns (the caller's buffer is free again); the chunk's kernels
 *                    are left running, so its verdict -- SG_ERR_INVALID for a line with fewer than 11 fields
 *                    (Profile.cpp:246-251), the cap -- is reported by the NEXT sg_train_feed or by sg_train_finish.
 *                    A chunk that does not end in a line break holds the file's last line, which loses its last
 *                    character as fgets + `buf[strlen(buf)-1] = '\0'` chop it (Profile.cpp:1458-1459)
 *   sg_train_finish  the count matrices; the (GC content, read count) pairs countGC pushed, in its order (gcs, readCounts)
 * Where the reference's behaviour is undefined the line is skipped and counted: reads hanging over their contig's end
 * (skipped_overhang).  Arrays are the caller's: subs1 / subs2 [kmer_count][bins][4], kmers [bins][kmer_count], quality
 * [16][bins][94], isize [n_isize], ins_len / del_len [n_indel_len].  Bases must be a permutation of ACGT, kmer 1..6.       */
typedef struct sg_train_setup {
  const char* const* contig_keys;
  uint32_t n_contigs;
  const char* bases;
  int32_t kmer, bins;
  uint32_t n_isize;        /* columns of iSizeDist kept (the reference grows its row; larger TLENs: isize_overflow) */
  uint32_t n_indel_len;    /* columns of insFreqs / delFreqs kept (longer events: indel_len_overflow) */
  int32_t count_gc;        /* 1: Profile::countGC gates and counts as the reference does; 0: every read through the filters counts */
  uint32_t window;         /* Segment::fragSize (1000) */
  uint64_t max_reads;      /* Profile::processRead's maxCount (Profile.cpp:236, 497-507): the run ends with the read that makes the
                            * count of counted reads reach it (twice it with targets); lines behind that one are never read.
                            * 0 = the reference's 300,000,000 */
  /* exome: inTargets[chr] after loadTargets + divideTargets (Genome.cpp:238-299, 684-739), in that order; the rows of contig c
   * are [target_first[c], target_first[c + 1]); spos / epos as the reference holds them.  NULL / no rows: whole genome. */
  const uint64_t* target_first;
  const int64_t* target_spos;
  const int64_t* target_epos;
  /* known variants of the sample (lib/vcfparser/vcfparser.cpp:26-106), in file order; positions as the parser stores them */
  uint64_t n_snv;  const uint32_t* snv_contig;  const int64_t* snv_pos;  const char* snv_alt;  const uint8_t* snv_homo;
  uint64_t n_ins;  const uint32_t* ins_contig;  const int64_t* ins_pos;  const int32_t* ins_len;
  uint64_t n_del;  const uint32_t* del_contig;  const int64_t* del_pos;  const int32_t* del_len;
} sg_train_setup;
typedef struct sg_train_counts {
  uint64_t *subs1, *subs2, *kmers, *quality, *isize, *ins_len, *del_len;
  uint64_t lines, reads_counted, cigar_chars, insert_events, delete_events, isize_overflow, indel_len_overflow, skipped_overhang,
      gc_rejected, gc_windows, capped;   /* capped: 1 when the run ended at max_reads */
} sg_train_counts;
int sg_train_begin(sg_ctx* ctx, const sg_train_setup* setup);
int sg_train_feed(sg_ctx* ctx, const char* sam_text, uint64_t sam_bytes);
/* 1 once the cap on counted reads is known to have been reached (the caller may stop reading its input), else 0; does not
 * wait for the chunk in flight, whose verdict arrives with the next feed / finish (a chunk fed behind the cap is ignored) */
int sg_train_capped(sg_ctx* ctx);
/* gc / rc: room for `gc_cap` pairs (NULL: none wanted); *n_gc = how many there are (SG_ERR_OVERFLOW when gc_cap is too small;
 * call again).  The session ends with a successful call or with sg_train_end. */
int sg_train_finish(sg_ctx* ctx, sg_train_counts* out, double* gc, double* rc, uint64_t gc_cap, uint64_t* n_gc);
void sg_train_end(sg_ctx* ctx);
/* One call for a text that fits memory: begin (no targets, no variants, count_gc = 0) + feed + finish. */
int sg_train_count(sg_ctx* ctx, const char* sam_text, uint64_t sam_bytes, const char* const* contig_keys, uint32_t n_contigs,
                   const char* bases, int32_t kmer, int32_t bins, uint32_t n_isize, uint32_t n_indel_len, sg_train_counts* out);

/* ---- BGZF and BAM input (SAMv1 sections 4.1-4.2): seqToProfile -b x.bam --decode-bam without samtools ----
 * A BGZF file is a run of gzip members (RFC 1952), each with the extra subfield 'BC' holding BSIZE (member bytes - 1) and at
 * most 64 KiB of input (ISIZE), closed by the 28-byte empty member of sg_bgzf_eof.  The members are inflated on the device
 * (stored, fixed- and dynamic-Huffman blocks; CRC-32 and ISIZE checked); a member that is not well formed is SG_ERR_INVALID
 * and the message names its file offset.
 *   sg_bgzf_members  host only: the member headers of `bytes` bytes -- offset, BSIZE, ISIZE of up to `cap` whole members
 *                    (any of the arrays may be NULL); *whole_bytes = the bytes they make up (a member cut by the end of the
 *                    buffer is not one of them).  SG_ERR_INVALID for a header that is not BGZF (sg_last_error(NULL) says where)
 *   sg_inflate_bgzf  whole members in host memory -> their inflated bytes in `out`; *out_bytes = how many there are
 *                    (SG_ERR_OVERFLOW when out_cap is too small: call again).  For the BAM header, and tests
 * In a training session (after sg_train_begin) the records of a BAM file take the place of the lines of text:
 *   sg_train_bam_start  the header's reference names (refID order) and where in the decompressed stream the first record
 *                    starts (behind magic, l_text, text, n_ref and the reference list); call once, before any feed
 *   sg_train_feed_bgzf  whole members in file order, from the file's first byte.  Record boundaries are found on the
 *                    device, records that straddle calls are carried over; every record `samtools view -F 0xD04 -q 20`
 *                    prints becomes the line it prints (eleven fields, QNAME and RNEXT / PNEXT included, a CIGAR of more
 *                    than 65,535 operations from its CG:B:I tag), and the lines go through the kernels of sg_train_feed.
 *                    Same contract: the members are copied before the call returns, the verdict of the lines arrives with
 *                    the next call, the cap ends the reading (sg_train_capped).  A malformed member or record is SG_ERR_INVALID
 *                    at once.  `bytes` = 0 ends the stream: SG_ERR_INVALID when a record was left unfinished
 *   sg_train_bam_info   records decoded (kept or not), bytes inflated, seconds spent in sg_train_feed_bgzf so far      */
int sg_bgzf_members(const void* buf, uint64_t bytes, uint64_t* offsets, uint32_t* bsize, uint32_t* isize, uint64_t cap, uint64_t* n_members,
                    uint64_t* whole_bytes);
int sg_inflate_bgzf(sg_ctx* ctx, const void* members, uint64_t bytes, void* out, uint64_t out_cap, uint64_t* out_bytes);
int sg_train_bam_start(sg_ctx* ctx, const char* const* ref_names, uint32_t n_ref, uint64_t first_record_skip);
int sg_train_feed_bgzf(sg_ctx* ctx, const void* members, uint64_t bytes);
int sg_train_bam_info(sg_ctx* ctx, uint64_t* records, uint64_t* inflated_bytes, double* seconds);

/* Which emit kernel the loaded profile gets (after sg_load_profile): 0 generic (tables that do not fit
 * LDS, k-mer sizes other than 3), 1 straight-line kernel (table image in LDS). */
int sg_emit_variant(sg_ctx* ctx);
/* The emit kernels the last pass launched (after sg_result), read-only.  main_kernel: SG_EMIT_STRAIGHT_LINE (k-mer 3, the
 * table image in LDS; the items it queues go to emit_slow_kernel), SG_EMIT_GENERIC_K3_LDS (generic kernel specialised for
 * k-mer 3, substitution rows staged in LDS), SG_EMIT_GENERIC_LDS (generic kernel, any k-mer, rows in LDS),
 * SG_EMIT_GENERIC_GLOBAL (generic kernel, rows read from global memory: contexts x bins x 16 bytes do not fit beside the
 * read rows).  slow_rows_lds: 1 / 0 when emit_slow_kernel stages its rows in LDS / reads them from global memory, -1
 * without the straight-line kernel.  lds_bytes: dynamic LDS of the main kernel.  clean_cap: per-wave entries of the
 * straight-line kernel's list of one-indel reads' clean items (0: those reads stay whole in the general steps).
 * A pass whose item queue overflowed (sg_emit_info) was emitted again by the generic kernel on top of this. */
#define SG_EMIT_STRAIGHT_LINE 1
#define SG_EMIT_GENERIC_K3_LDS 2
#define SG_EMIT_GENERIC_LDS 3
#define SG_EMIT_GENERIC_GLOBAL 4
typedef struct sg_emit_path_info {
  int32_t main_kernel;
  int32_t slow_rows_lds;
  uint32_t lds_bytes;
  uint32_t clean_cap;
} sg_emit_path_info;
int sg_emit_path(const sg_ctx* ctx, sg_emit_path_info* info);

/* Exact u32 form of the reference's inverse-CDF draw, exposed for tests: number of 32-bit draws
 * x for which randIndx's `r <= c` holds (r = 2.2204e-16 + (1-2.2204e-16)*x/2^32).               */
uint64_t sg_cdf_count_le(double c);

/* The per-base sampling tables, exposed for tests (host code, no GPU needed).  A CDF row partitions the 2^32 draws
 * into integer counts per outcome (sg_cdf_count_le differences); the engine samples through two rearrangements that
 * keep every count:
 *   sg_sub_row_identity_first  substitution row (Profile::getSubBaseIndx1/2, Profile.cpp:1527-1554): outcomes in the
 *                              order [cd, the other base indexes ascending], cum[i] = draws of order[0..i];
 *   sg_alias_row               quality row (Profile::getBaseQuality, Profile.cpp:1576-1580) as 2^lgW alias columns:
 *                              draw x -> column x >> (32 - lgW), symbol lo[col] if (x & (2^(32-lgW) - 1)) < thr[col] else
 *                              hi[col];  sg_row_symbols = number of symbols with a non-zero count (columns needed).   */
int sg_sub_row_identity_first(const double cdf4[4], int cd, uint64_t cum[3], uint8_t order[4]);
uint32_t sg_row_symbols(const double* cdf, int n);
int sg_alias_row(const double* cdf, int n, uint32_t lgW, uint32_t* thr, uint8_t* lo, uint8_t* hi);

/* ---- truthEval: an aligner's BAM scored against the truth BAM (the rule: csrc/sg_eval.h) ----
 * Both files are fed as whole BGZF members in file order, from the file's first byte, as sg_train_feed_bgzf takes them (the
 * same walk, inflate, record boundaries, carry of a record that straddles calls, and refusals with the file or decompressed
 * offset); `bytes` = 0 ends a stream and refuses a record left unfinished.  One session per context:
 *   sg_eval_begin        n_ref_truth references in the truth's header, whose first record starts first_record_skip bytes into
 *                        the decompressed stream.  key_bits 1..64: the bits of a read's key that are kept (64 in use; fewer
 *                        make collisions common, for tests).  min_overlap 1..100: PCT of the `near` category
 *   sg_eval_truth_bgzf   the truth's members: a row per record (key, name, refID, POS, span, strand / unmapped / class / mate),
 *                        the names in an arena on the device.  At most 2^32 - 1025 records
 *   sg_eval_truth_done   sorts the rows by key, marks every (name, mate) the truth holds more than once; *records, *duplicates
 *                        = rows, rows so marked
 *   sg_eval_test_refmap  map[i] = the truth's refID of the test file's reference i (by @SQ name), -1 for none; and where the
 *                        test file's first record starts
 *   sg_eval_test_bgzf    the test file's members: look-up, claim (the least ordinal in the file wins a truth read), score
 *   sg_eval_finish       counts the truth reads nobody claimed and returns the table, SG_EVAL_CELLS cells laid out
 *                        [mate 0..1][class: plain, edited, unmapped][MAPQ 0..255][category: exact, near, wrong_place,
 *                        wrong_strand, wrong_contig, lost, invented, both_unmapped], and the counts
 *   sg_eval_end          ends the session and frees its buffers
 *   sg_eval_classify, sg_eval_key  host only, no context: the category (0..7 in the order above) of one pair, the key of one
 *                        read -- the same code the kernels run */
#define SG_EVAL_CELLS 12288
typedef struct sg_eval_counts {
  uint64_t test_records, secondary, supplementary, unknown, ambiguous, repeated, truth_records, truth_duplicates;
  uint64_t missing[6];                 /* [mate][class] */
  uint64_t truth_bytes, test_bytes;    /* inflated */
  double t_inflate, t_truth, t_sort, t_test;   /* seconds: inflate and boundaries of both files (part of the next two); the truth's
                                                  calls; sg_eval_truth_done; the test file's calls */
} sg_eval_counts;
int sg_eval_begin(sg_ctx* ctx, uint32_t n_ref_truth, uint32_t key_bits, uint32_t min_overlap, uint64_t first_record_skip);
int sg_eval_truth_bgzf(sg_ctx* ctx, const void* members, uint64_t bytes);
int sg_eval_truth_done(sg_ctx* ctx, uint64_t* records, uint64_t* duplicates);
int sg_eval_test_refmap(sg_ctx* ctx, const int32_t* map, uint32_t n_ref_test, uint64_t first_record_skip);
int sg_eval_test_bgzf(sg_ctx* ctx, const void* members, uint64_t bytes);
int sg_eval_finish(sg_ctx* ctx, uint64_t* table, uint64_t cap, sg_eval_counts* counts);
void sg_eval_end(sg_ctx* ctx);
uint32_t sg_eval_classify(int32_t truth_ref, int64_t truth_pos, uint64_t truth_span, int truth_reverse, int truth_unmapped, int32_t test_ref,
                          int64_t test_pos, uint64_t test_span, int test_reverse, int test_unmapped, uint32_t min_overlap);
uint64_t sg_eval_key(const void* name, uint32_t len, uint32_t mate, uint32_t key_bits);

/* ---- a VCF of known variants, read on the device: the rows lib/vcfparser/vcfparser.cpp:26-106 yields ----
 * The text -- plain, or the members of a BGZF file as bgzip writes them -- is cut into the fragments the parser's
 * fgets(buf, 20000) returns, and every fragment gets the parser's verdict: skipped, an SNV, an insertion or a deletion with
 * the values the parser stores, malformed (fewer than ten fields), or UNDECIDED.  The rule and the exact set of forms
 * decided on the device are stated in csrc/sg_vcf.h; an undecided fragment (an exponent in QUAL, over-long digit strings,
 * white space in front of a number, a NUL byte) is handed back with its bytes for the caller to resolve.
 *   sg_vcf_begin      a session on `n_contigs` contig keys (each shorter than 64 bytes; row = index), one per context
 *   sg_vcf_feed       host text, cut anywhere: a line the call leaves unfinished stays on the device and leads the next one.
 *                     At most 1 GiB per call; a line longer than 64 MiB, finished or not, is SG_ERR_INVALID naming its offset
 *   sg_vcf_feed_bgzf  whole BGZF members in file order (the walk, the inflate and the refusals of sg_train_feed_bgzf: a
 *                     member that is not well formed is SG_ERR_INVALID naming its file offset).  The text goes the way of
 *                     sg_vcf_feed.  A call that fails delivers nothing: counts, rows and the carried line stay as they were
 *   sg_vcf_undecided  the undecided fragments of the LAST feed: number, offset into `bytes`, length; valid until the next
 *                     feed.  SG_ERR_OVERFLOW when `cap` rows or `bytes_cap` bytes do not hold them (*n, *n_bytes say how
 *                     many there are: call again)
 *   sg_vcf_finish     the end of the text: a last line without a line break is parsed; the counts.  Rows stay fetchable
 *   sg_vcf_rows       `n` kept rows of `kind` (SG_VCF_SNV / _INS / _DEL) from row `first` on, in file order
 *   sg_vcf_end        ends the session and frees its buffers
 *   sg_vcf_row        host only, no context: the verdict on one fragment (1..19999 bytes), the same code the kernel runs */
#define SG_VCF_SKIP 0
#define SG_VCF_SNV 1
#define SG_VCF_INS 2
#define SG_VCF_DEL 3
#define SG_VCF_MALFORMED 4
#define SG_VCF_UNDECIDED 5
#define SG_VCF_HOMO 1u    /* flags: the parser files the SNV as homozygous (everything but the genotype "1/1") */
#define SG_VCF_KNOWN 2u   /* flags: the contig is among the keys (the row is kept) */
typedef struct sg_vcf_record {
  uint64_t fragment;   /* its number, from 1: the parser's line_num */
  int64_t pos;         /* as the parser stores it: POS, POS + 1 of a deletion */
  uint32_t contig;     /* row among the contig keys */
  int32_t value;       /* SNV: the first byte of ALT (0: ALT is empty); insertion / deletion: its length */
  uint32_t kind;       /* SG_VCF_* */
  uint32_t flags;      /* SG_VCF_HOMO, SG_VCF_KNOWN */
} sg_vcf_record;
typedef struct sg_vcf_fragment {
  uint64_t number;
  uint64_t offset;     /* where its bytes start */
  uint32_t len, pad;
} sg_vcf_fragment;
typedef struct sg_vcf_counts {
  uint64_t fragments;                  /* numbered so far */
  uint64_t n_snv, n_ins, n_del;        /* as the parser counts them: rows on unknown contigs included */
  uint64_t kept_snv, kept_ins, kept_del;
  uint64_t malformed;
  uint64_t malformed_first[11];        /* the numbers of the first eleven */
  uint64_t undecided;                  /* over all feeds */
  uint64_t text_bytes;
} sg_vcf_counts;
int sg_vcf_begin(sg_ctx* ctx, const char* const* contig_keys, uint32_t n_contigs);
int sg_vcf_feed(sg_ctx* ctx, const char* text, uint64_t bytes);
int sg_vcf_feed_bgzf(sg_ctx* ctx, const void* members, uint64_t bytes);
int sg_vcf_undecided(sg_ctx* ctx, sg_vcf_fragment* rows, uint64_t cap, uint64_t* n, char* bytes, uint64_t bytes_cap, uint64_t* n_bytes);
int sg_vcf_finish(sg_ctx* ctx, sg_vcf_counts* counts);
int sg_vcf_rows(sg_ctx* ctx, uint32_t kind, uint64_t first, uint64_t n, sg_vcf_record* rows);
int sg_vcf_end(sg_ctx* ctx);
int sg_vcf_row(const char* fragment, uint32_t len, const char* const* contig_keys, uint32_t n_contigs, sg_vcf_record* row);

#ifdef __cplusplus
}
#endif
#endif
