// sg_api.h -- what the files of the C ABI share.  Internal: the ABI itself is include/simuscop_amd.h.  Who defines what:
//   sg_memory.cpp          block and pinned-memory caches: DevBuf::ensure / release, sg_grow_keep, sg_host_alloc / _free,
//                          sg_release_cached_memory
//   sg_api.cpp             the context, sg_load_profile / sg_load_prepared_profile, sg_plan and finish_plan, the sampling pass
//                          (sg_sample, sg_pass_need, retire_plan), sg_result and the fetch calls, detached outputs
//   sg_profile_tables.cpp  sg_profile_prepare and the table self-checks (host only: sg_profile_tables.h)
//   sg_api_deflate.cpp     the BGZF sink: deflate_text, sg_compress, sg_deflate_bgzf, sg_fetch_compressed, sg_bgzf_eof
//   sg_api_truth.cpp       truth alignments and the truth BAM: sg_pass_prelude, sg_truth_*, sg_pass_records, sg_fetch_truth
//   sg_api_haplotypes.cpp  reference ingest and haplotype assembly: sg_reference_*, sg_build / upload_haplotypes, sg_haplotype_codes
//   sg_api_bgzf.cpp        BGZF / BAM input: inflate_launch / _verdicts, the bam_stream_* calls, sg_bgzf_members, sg_inflate_bgzf
//                          (the member walk, bgzf_walk, is sg_bgzf.h's: host only)
//   sg_api_windows.cpp (window planner), sg_api_train.cpp (profile training: sg_train_*), sg_api_depth.cpp / _variants.cpp /
//   _errors.cpp (true coverage, allele and error counts), sg_api_bamsort.cpp / _bamindex.cpp (the sorted truth BAM, its BAI index),
//   sg_api_vcf.cpp (a VCF of known variants read on the device: sg_vcf_*), sg_api_eval.cpp (truthEval: sg_eval_*)
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "sg_bam.h"
#include "sg_device.h"
#include "sg_haplotypes.h"

// A grow-only device buffer that owns its block.  The block goes back to the process's block cache (sg_memory.cpp) when the
// buffer is destroyed, released or assigned over; the cache waits for the device first, so nothing still queued can touch
// the block once it is handed out again.  Move-only: a move hands the block over.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int dev = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)), dev(o.dev) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { release(); p = std::exchange(o.p, nullptr); cap = std::exchange(o.cap, 0); dev = o.dev; }
    return *this;
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  int ensure(size_t bytes);   // at least `bytes` (contents not kept); 0 or the hipError_t of the failed allocation
  void release();
  template <class T> T* as() const { return (T*)p; }
};

// One pass's output buffers by mate: the FASTQ text, its BGZF members (sg_compress).  Handing a set over is one std::swap.
struct OutputSet {
  DevBuf text[2], gz[2];
  bool empty() const { return !text[0].p && !text[1].p && !gz[0].p && !gz[1].p; }
};

extern thread_local std::string g_create_error;   // sg_last_error(nullptr): calls without a context

struct sg_outputs;
struct sg_train_session;
struct sg_eval_session;

struct sg_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  uint64_t seed = 0;
  std::string err;

  bool have_profile = false, have_haps = false;   // the inputs; everything about a batch and its pass is in `pass`
  sg::DevProfile P{};
  sg::DevBatch B{};
  OutputSet out;
  DevBuf tab, chains, chains2, chain_meta, windows, segmeta, prefix, pairs, win_namebase, win_slot, win_flag, win_rows, blk_win, seg_flags, events, recoff, meta, totals, bsum,
      slowq, ref_raw, ref_codes, ref_meta, hap_work, gz_work,
      infl_src, infl_meta, infl_out, infl_crc,   // sg_inflate_bgzf (infl_crc also serves the training session's BAM input)
      defl_src, defl_out;                        // sg_deflate_bgzf: the caller's text and its members
  // the haplotype chains in `chains` (sg_upload_haplotypes, sg_build_haplotypes): chain c holds len[c] bases from off[c] on;
  // chain_meta holds the same on the device for the kernels, the host checks against this copy
  struct ChainLayout {
    std::vector<uint64_t> off, len;
    size_t total = 0;   // bytes of the padded chains buffer
  } hap;
  // Each truth output's state owns its device buffers: ending one is assigning a fresh state over it.
  // truth alignments (sg_truth_*): whether the chains came from a copy list (sg_build_haplotypes; how many pieces it
  // had) and, once sg_truth_map has been given that list, its pieces sorted by (chain, dst) with the chains' first
  // indexes -- on the host for sg_truth_pieces, on the device (`map`, laid out as sg::PieceMap says) for the record
  // kernels.  Without sg_truth_map nothing is kept and nothing is allocated.  New chains forget the map and keep the
  // buffers (forget).
  struct TruthInfo {
    uint64_t n_given = 0;
    bool from_build = false, mapped = false;
    std::vector<sg_truth_piece> sorted;
    std::vector<uint64_t> chain_first;
    uint32_t n_refs = 0;   // the tag kernels' way from a refID back to its contig's codes: rows of `refs` (0: no reference codes)
  };
  struct Truth : TruthInfo {
    DevBuf map, work, rec, gz, rows, refs, tag_rows;
    void forget() { static_cast<TruthInfo&>(*this) = TruthInfo(); }
  } truth;
  // true coverage (sg_depth_*, sg_api_depth.cpp): the contigs' lengths and first slots in `diff`, the flat int32
  // difference array (`meta` holds both tables for the kernels); `work` holds one contig's tile sums, run-start
  // counts and their scans (`scanned` says whose, until the array changes), `out` a call's bins, rows or depths and
  // the spans of sg_depth_add_spans.  Without sg_depth_begin nothing is kept and nothing is allocated.
  struct Depth {
    bool on = false;
    std::vector<uint64_t> len, off;
    uint64_t slots = 0, m_bases = 0, scanned_starts = 0;
    int64_t scanned = -1;
    DevBuf diff, meta, work, out;
  } depth;
  // true allele counts (sg_variants_*, sg_api_variants.cpp): `rows` holds the sorted table as sg::VariantRow rows,
  // `counts` the [n][2] uint32 counters (total, alt) and behind them the kernel's three 64-bit counters.  Without
  // sg_variants_begin nothing is kept and nothing is allocated.
  struct Variants {
    bool on = false;
    uint64_t n = 0, reads_hit = 0, hits = 0;
    DevBuf rows, counts;
  } variants;
  // true error counts (sg_errtab_*, sg_api_errors.cpp): `table` holds the flat table of 64-bit counters (the layout:
  // sg_truth.h) and behind it the kernel's five 64-bit counters.  Without sg_errtab_begin nothing is kept and nothing
  // is allocated.
  struct Errtab {
    bool on = false;
    uint32_t cycles = 0, qual_lo = 0, n_qual = 0, L = 0, cus = 0;
    uint64_t bases = 0, errors = 0, skipped = 0, reads = 0;
    DevBuf table;
  } errtab;
  // the truth BAM in coordinate order (sg_bamsort_*, sg_api_bamsort.cpp): the keys and payloads of the sort (two of each:
  // a digit pass goes from one to the other; `cur` holds the result), the records' lengths in output order, `work` the
  // counters, histograms and offsets of a call; of a merge also its input records, output stream and members.  `n`
  // records are indexed while `have` (a merge) or the pass says bam_sorted.  Without a sg_bamsort_* call nothing is
  // kept and nothing is allocated.
  struct BamSort {
    bool have = false;
    int cur = 0;
    uint64_t n = 0, out_bytes = 0, gz_bytes = 0;
    DevBuf keys[2], vals[2], lens, work, src, out, gz;
    const uint64_t* dst_off = nullptr;   // of a merge: where its records start in `out` (in `work`, until the next sg_bamsort_* call)
  } bamsort;
  // The last compression (deflate_text): its text and the member offset table it left in gz_work -- entry i is where the
  // member of text bytes [32768 i, 32768 i + 32768) starts among the members.  Forgotten when the next one starts.
  struct GzLast {
    const uint8_t* text = nullptr;
    uint64_t bytes = 0;
    const uint64_t* moff = nullptr;
  } gz_last;
  // the BAI index of the sorted truth BAM (sg_bamindex_*, sg_api_bamindex.cpp; the index: sg_bamindex.h): of the stem the
  // references (`refs`: sg::BaiRef rows), the linear index and the counts; of a call its rows, offsets, chunk rows
  // (`work`, `chunks`) and the (key, chunk number) pairs of their sort; `carry` holds a record that a text of
  // sg_deflate_bgzf left unfinished, until the next text brings its rest.  Without sg_bamindex_begin nothing is kept and
  // nothing is allocated.
  struct BamIndex {
    bool on = false, broken = false;
    std::vector<uint64_t> ref_len;
    uint64_t n_win = 0, n_chunks = 0, carry_voff = 0;
    uint32_t carry_have = 0, carry_need = 0;   // bytes of the unfinished record in `carry`, and those still to come
    int cur = 0;
    DevBuf refs, linear, counts, work, chunks, keys[2], vals[2], carry;
  } bamindex;
  // a VCF of known variants (sg_vcf_*, sg_api_vcf.cpp; the rule: sg_vcf.h): `text[cur]` holds the line the last feed left
  // unfinished (`carry` bytes) and takes the next call's text behind it, `rows[k]` the kept rows of kind k so far, `work` a
  // call's block counts, `lines` and `frags` its line and fragment tables with their flags and scans (`scan`: the block
  // sums), `lists` its malformed numbers and undecided fragments (the latter `last_undecided`, whose bytes are in
  // text[cur ^ 1] until the next feed), `src` / `meta` the members of sg_vcf_feed_bgzf.  Without
  // sg_vcf_begin nothing is kept and nothing is allocated.
  struct Vcf {
    bool on = false, finished = false;
    uint32_t n_keys = 0;
    int cur = 0;
    uint64_t carry = 0, text_off = 0, file_off = 0;   // text_off: offset in the whole text of text[cur][0]
    uint64_t fragments = 0, n_kind[3] = {0, 0, 0}, kept[3] = {0, 0, 0}, malformed = 0, undecided = 0, text_bytes = 0;
    uint64_t malformed_first[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t last_undecided = 0;
    const sg_vcf_fragment* last_list = nullptr;   // in `lists`
    DevBuf keys, text[2], rows[3], work, lines, frags, scan, lists, info, src, meta;
  } vcf;
  std::vector<sg_outputs*> spare;  // released output sets, reused by the next pass
  // the window planner (sg_gc_percent, sg_window_weights, sg_windows_*, sg_plan_windows / sg_plan_range;
  // sg_api_windows.cpp): `stores` holds the window weights of sg_windows_build per store id, `plan` the batch table of
  // sg_plan_windows (sg_window rows) and `info` what sg_plan_range needs of it on the host.  `gc` (sg_gc_percent,
  // sg_window_weights) and `work` (sg_windows_build, sg_plan_windows) are arenas private to one call, `model` the means
  // and quantile knots of a call's sg_gc_model.  The stores and the batch table survive new chains: store ids are per
  // (population, chromosome), and the driver uploads chromosomes in turn between sg_windows_build and sg_plan_windows.
  // Only sg_windows_drop ends the stores.
  struct Windows {
    struct Store { DevBuf weights; uint64_t n = 0; };
    struct PlanInfo {
      bool valid = false;
      uint32_t n_active = 0, batch_id = 0;
      int32_t paired = 0;
      std::string prefix;
      std::vector<uint32_t> seg_first, seg_size;  // per active segment (seg_first has n_active + 1 entries)
      std::vector<uint64_t> slot_first;           // planned fragments before each active segment; [n_active] = total
    };
    std::map<uint32_t, Store> stores;
    DevBuf plan, work, gc, model;
    PlanInfo info;
  } win;
  uint64_t ref_raw_bytes = 0;
  sg_train_session* train = nullptr;   // profile training in progress (sg_train_begin .. sg_train_finish / sg_train_end)
  sg_eval_session* eval = nullptr;     // truthEval in progress (sg_eval_begin .. sg_eval_end; sg_api_eval.cpp)
  std::vector<sg::DevContig> ref_contigs;  // host copy of the committed contig table
  uint64_t* mail = nullptr;   // pinned: where a pass's totals[0..4] land (copied into `pass` when it is settled)
  // A batch and its sampling pass: the stage, and every fact whose meaning ends with the pass.  The buffers those facts
  // describe stay where they are (out.text / out.gz, truth.rec / truth.gz).  Starting over is assigning a fresh Pass.
  //
  //   None --sg_plan*--> Planned --sg_sample--> Queued --sg_pass_need(.., Settled, true)--> Settled
  //
  //   Planned  a batch is planned (finish_plan)
  //   Queued   run_pass has enqueued the kernels; sizes are not looked at yet, the text may not have fitted its buffers
  //   Settled  the stream is drained, totals / flags are the mail's, a text that did not fit and an overflowed slow queue
  //            have been emitted again, slow_items / slow_overflow and (when profiling) the kernel times are taken
  //
  //   sg_plan*, sg_sample           a fresh Pass; so does a pass that fails with SG_ERR_OVERFLOW, and sg_detach_outputs
  //                                 (both back to Planned: the plan is still good)
  //   new chains, a new profile     Planned goes back to None; a Queued or Settled pass stays for the calls that read only
  //                                 its text, with rows_current = false: its plan is gone (sg_sample: "call sg_plan
  //                                 first") and its rows no longer belong to the chains, the piece map or the profile
  //                                 (sg_pass_prelude and sg_truth_reads refuse)
  struct Pass {
    enum Stage { None, Planned, Queued, Settled } stage;
    explicit Pass(Stage s = None) : stage(s) {}
    bool rows_current = true;
    bool speculative = false;         // the emit kernels were launched before the text size was known (see run_pass)
    uint64_t host_totals[4] = {0, 0, 0, 0};
    uint64_t host_flags[2] = {0, 0};  // totals[3..4] after the emit kernels: flags, slow-queue counts
    uint64_t slow_items = 0;
    bool slow_overflow = false;
    sg::EmitPath emit_path = {0, -1, 0, 0};  // the emit kernels of the pass (sg_emit_path)
    bool have_gz = false;             // sg_compress: out.gz holds gz_bytes of members
    uint64_t gz_bytes[2] = {0, 0};
    bool have_bam = false;            // sg_truth_bam: truth.rec / truth.gz hold the pass's records
    bool bam_sorted = false;          // ... made by sg_bamsort_pass: in key order, uncompressed, indexed by ctx->bamsort
    uint64_t bam_rec_bytes = 0, bam_gz_bytes = 0, bam_records = 0, bam_unmapped = 0;
    uint64_t bam_tags[7] = {0, 0, 0, 0, 0, 0, 0};   // sg_truth_bam_tags: records with NM, MD, XE, the sums of NM and XE, MD texts dropped, tag bytes
  } pass;

  bool profiling = false;
  // the timing events of a pass, in stream order but the last: around edge_kernel, around fragment_kernel, behind
  // block_base_kernel; before header_kernel, behind the last emit kernel, and between the main emit kernel and emit_slow_kernel
  enum { EV_EDGE_BEGIN, EV_EDGE_END, EV_FRAGMENT_BEGIN, EV_FRAGMENT_END, EV_SCAN_END, EV_TEXT_BEGIN, EV_TEXT_END, EV_MAIN_EMIT_END, EV_COUNT };
  hipEvent_t evs[EV_COUNT] = {};
  bool evs_created = false;
  float last_ms[SG_K_COUNT] = {0, 0, 0, 0, 0, 0};

  ~sg_ctx();   // streams, events, pinned mail and spare output sets; the buffers go with their members
  int fail(int code, const std::string& m) { err = m; return code; }
  int hipfail(hipError_t e, const char* what) {
    err = std::string(what) + ": " + hipGetErrorString(e);
    return SG_ERR_HIP;
  }
};

#define SG_HIP(call)                                        \
  do {                                                      \
    hipError_t _e = (call);                                 \
    if (_e != hipSuccess) return ctx->hipfail(_e, #call);   \
  } while (0)
#define SG_ENSURE(buf, bytes)                                                                  \
  do {                                                                                         \
    int _e = (buf).ensure(bytes);                                                              \
    if (_e) return ctx->hipfail((hipError_t)_e, "hipMalloc(" #buf ")");                        \
  } while (0)

// ---- what the truth outputs' entry points share (sg_truth_bam, sg_depth_*, sg_variants_*, sg_errtab_*) ----
namespace sg { struct PieceMap; }
// The start of a call that reads the rows of the pass just sampled, its checks in this order: rows that still belong to
// the chains and the profile; with `map`, the chains' piece map (sg_build_haplotypes, then sg_truth_map); sg_result; with
// `map`, fewer than 2^32 reads; with `bam_names`, read names that a BAM record holds (sg_truth_bam's own check, whose
// place is in front of the next); no SG_DIAG.  The device is selected and *map filled.  Defined in sg_api_truth.cpp.
int sg_pass_prelude(sg_ctx* ctx, const char* who, sg::PieceMap* map, bool bam_names = false);
// The gate of every call that reads a pass: no context; "<who>: call sg_plan / sg_sample / sg_result first" when the
// stage is below `at_least`; then the device is selected.  Settled is asked in two ways: of a pass that sg_result has
// settled already (a Queued one is told to call sg_result), or with settle_now, which settles a Queued pass here and
// so asks no more than sg_sample of the caller.  Planned asks for a plan that new inputs have not retired.
int sg_pass_need(sg_ctx* ctx, const char* who, sg_ctx::Pass::Stage at_least, bool settle_now = false);
// Work buffers and DevBatch fields of a batch whose windows / segment arrays are in ctx->windows / ctx->segmeta: the end
// of sg_plan and sg_plan_range.  Internal like the two above, not part of the ABI.  Defined in sg_api.cpp.
int finish_plan(sg_ctx* ctx, uint64_t nw, uint32_t n_segs, uint32_t n_slots, uint32_t batch_id, uint32_t first_window,
                uint32_t first_slot, int32_t paired, const char* name_prefix);
// The chains or the profile changed: the plan is gone, and a pass's rows no longer belong to them (its text stays).
void retire_plan(sg_ctx* ctx);
// `bytes` (> 0) of text on the device -> its BGZF members in `gz`, *gz_total bytes of them.  `text` is followed by 64
// readable bytes, as the sampler's output buffers are.  What sg_compress does per mate, sg_deflate_bgzf for its caller,
// sg_truth_bam for its records and sg_bamsort_merge for its stream.  Defined in sg_api_deflate.cpp.
int deflate_text(sg_ctx* ctx, const uint8_t* text, uint64_t bytes, DevBuf& gz, uint64_t* gz_total, const char* who);
// The records of the pass just sampled into truth.rec (sg_truth_bam_tags; `sorted`: sg_bamsort_pass, whose stream is in
// key order and stays uncompressed).  Defined in sg_api_truth.cpp.
int sg_pass_records(sg_ctx* ctx, const char* who, uint32_t tags, bool sorted, uint64_t* record_bytes, uint64_t* bgzf_bytes);
// The two steps sg_pass_records takes for a sorted pass (sg_api_bamsort.cpp).  bamsort_pass_keys, behind the sizing
// kernels on the stream: the live records' keys.  bamsort_pass_order, once the stream has been waited for: sorts them and
// fills `rec_off` by read index with the scan of the lengths in key order; *total = bytes of the stream.
namespace sg { struct TruthJob; }
int bamsort_pass_keys(sg_ctx* ctx, const sg::TruthJob& J, bool paired);
int bamsort_pass_order(sg_ctx* ctx, const sg::TruthJob& J, uint64_t* rec_off, uint64_t* total);
// The stable sort of n (u64 key, u32 payload) pairs in keys[*cur] / vals[*cur] (sg_api_bamsort.cpp); the result is in
// keys[*cur] / vals[*cur] again.  A digit in which k_or and k_and agree is the same in all keys and is skipped.  hist and
// hist_off hold 256 * bamsort_blocks(n) cells, bsum what launch_scan_u32 asks for that many values, *total one cell.
struct SgSortBufs {
  DevBuf* keys;   // [2]
  DevBuf* vals;   // [2]
  int* cur;
  uint32_t* hist;
  uint64_t* hist_off;
  uint64_t* bsum;
  uint64_t* total;
};
int bamsort_sort_pairs(sg_ctx* ctx, const SgSortBufs& b, uint32_t n, uint64_t k_or, uint64_t k_and);
// BGZF input, shared by the BAM and the VCF route (sg_api_bgzf.cpp; the member walk in front of it, bgzf_walk, is in sg_bgzf.h,
// which sg_bam.h brings in).  inflate_launch: members of `src` (on the device) inflated to d_out + member.dst, the verdicts
// behind the member table in `meta`.  inflate_verdicts: those verdicts, once the stream has been waited for; the first
// member that failed names the error.
int inflate_launch(sg_ctx* ctx, const uint8_t* d_src, uint64_t src_bytes, const std::vector<sg::InflateMember>& mem, DevBuf& meta, uint8_t* d_out,
                   hipStream_t s, hipStream_t copy);
int inflate_verdicts(sg_ctx* ctx, const std::vector<sg::InflateMember>& mem, const DevBuf& meta, const char* who);
// A BAM file fed as whole BGZF members in file order (sg_api_bgzf.cpp): what sg_train_feed_bgzf and the sg_eval_*_bgzf calls
// share.  A call goes
//   bam_stream_stage    the member walk and its refusals; the members start for the device on `copy` (wait for it before the
//                       caller's buffer is let go)
//   bam_stream_records  the members inflated into stream[scur] behind the partial record the call before left (`carry` bytes),
//                       the header passed over (`skip`), record boundaries and the inflate / boundary refusals; `job` holds the
//                       stream and, queued on `s`, the start of each of its n_rec whole records
//   (the caller's own kernels over job->rec, then bam_stream_totals: job->totals on the host, a record the kernels refused
//                       turned into the call's error by bam_stream_record_error)
//   bam_stream_advance  the partial record behind the last whole one goes to the front of the other stream buffer
// and bam_stream_close, at the end of the file, refuses a record left unfinished.  bam_stream_start names the references
// (refID order; ref_names may be NULL when no kernel prints them) and where the first record starts.
struct SgBamStream {
  uint32_t n_ref = 0;
  uint64_t skip = 0;         // header bytes of the decompressed stream still to be passed over
  uint64_t carry = 0;
  uint64_t file_off = 0;     // file offset of the next member
  uint64_t stream_off = 0;   // offset in the decompressed stream of stream[scur][0]
  uint64_t records = 0, inflated = 0;
  int scur = 0;
  DevBuf names, name_off, src, meta, stream[2], seg, rec, scan, totals;
  // of the call in progress
  std::vector<sg::InflateMember> mem;
  uint64_t bytes = 0, total = 0, L = 0, tail = 0, n_rec = 0;
};
int bam_stream_start(sg_ctx* ctx, SgBamStream& B, const char* const* ref_names, uint32_t n_ref, uint64_t first_record_skip);
int bam_stream_stage(sg_ctx* ctx, SgBamStream& B, const char* who, const void* members, uint64_t bytes, hipStream_t copy);
int bam_stream_records(sg_ctx* ctx, SgBamStream& B, const char* who, hipStream_t s, hipStream_t copy, sg::BamJob* job);
int bam_stream_record_error(sg_ctx* ctx, const SgBamStream& B, const char* who, uint64_t key);
int bam_stream_advance(sg_ctx* ctx, SgBamStream& B, hipStream_t s);
int bam_stream_close(sg_ctx* ctx, const SgBamStream& B, const char* who);
// a device buffer grown with its first keep_bytes kept (sg_memory.cpp)
int sg_grow_keep(sg_ctx* ctx, DevBuf& buf, size_t keep_bytes, size_t want_bytes);
// no context, or a call in front of its output's X_begin
inline int sg_need_begun(sg_ctx* ctx, bool on, const char* who, const char* begin) {
  if (!ctx) return SG_ERR_INVALID;
  return on ? SG_OK : ctx->fail(SG_ERR_INVALID, std::string(who) + ": call " + begin + " first");
}
// Where the 64-bit counters of a counting kernel live: behind `bytes` of cells, 64-byte aligned, with 64 bytes of their own.
inline size_t sg_counters_at(size_t bytes) { return (bytes + 63) & ~(size_t)63; }
// What the kernels just launched left at `src`, on the host when this returns SG_OK (a failed launch shows here).
inline int sg_read_back(sg_ctx* ctx, void* dst, const void* src, size_t bytes) {
  SG_HIP(hipGetLastError());
  SG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  SG_HIP(hipStreamSynchronize(ctx->stream));
  return SG_OK;
}
// J.totals on the host once the caller's kernels over a stream's records have run; a record they refused is the call's error
static inline int bam_stream_totals(sg_ctx* ctx, const SgBamStream& B, const char* who, const sg::BamJob& J, uint64_t h_tot[4]) {
  if (int rc = sg_read_back(ctx, h_tot, J.totals, 32)) return rc;
  return h_tot[3] != ~0ull ? bam_stream_record_error(ctx, B, who, h_tot[3]) : SG_OK;
}
// [offset, offset + bytes) lies within `have` bytes.  (The sum is never formed: it wraps for a large offset.)
inline bool sg_range_within(uint64_t offset, uint64_t bytes, uint64_t have) { return offset <= have && bytes <= have - offset; }
// `bytes` of device memory at `src` (the caller has tested the range), on the host when this returns hipSuccess
inline hipError_t sg_fetch_bytes(int device, hipStream_t stream, void* dst, const void* src, uint64_t bytes) {
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess && bytes) e = hipStreamSynchronize(stream);
  return e;
}
// Zero n (<= 8) counters, launch, read them back.
template <class Launch>
int sg_run_counted(sg_ctx* ctx, void* counters, size_t n, uint64_t* out, Launch launch) {
  SG_HIP(hipMemsetAsync(counters, 0, n * 8, ctx->stream));
  launch();
  return sg_read_back(ctx, out, counters, n * 8);
}
// One device allocation carved into arrays, each 64-byte aligned.  `carve` takes its arrays from the arena it is given;
// it runs twice: without a base for the size, then over `buf` grown to that size for the pointers.
struct SgArena {
  uintptr_t base;
  size_t off = 0;
  template <class T> T* take(size_t count) { T* p = (T*)(base + off); off = (off + count * sizeof(T) + 63) & ~(size_t)63; return p; }
};
template <class Carve>
int sg_carve(sg_ctx* ctx, DevBuf& buf, Carve carve) {
  SgArena size{0};
  carve(size);
  if (int e = buf.ensure(size.off)) return ctx->hipfail((hipError_t)e, "hipMalloc(arena)");
  SgArena a{(uintptr_t)buf.p};
  carve(a);
  return SG_OK;
}
