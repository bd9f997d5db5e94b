"""simuscop_amd -- MI355X-native read-sampling engine behind SimuSCoP's simuReads surface.

Python is only glue here (ctypes over the C ABI in include/simuscop_amd.h and over the C++ host
library); the product is `lib/libsimuscop_amd.so` (HIP kernels, gfx950), `lib/libsimuscop_host.so`
and the `lib/simuReads` command line.  There is no Python or CPU compute path: loading fails loudly
when the native libraries are missing.
"""
from __future__ import annotations

import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(PKG_DIR, "lib")
ENGINE_SO = os.path.join(LIB_DIR, "libsimuscop_amd.so")
HOST_SO = os.path.join(LIB_DIR, "libsimuscop_host.so")
SIMUREADS = os.path.join(LIB_DIR, "simuReads")
TRUTHEVAL = os.path.join(LIB_DIR, "truthEval")

SG_K_NAMES = ["plan", "namebase", "indel", "scan", "emit", "emit_slow"]

# every symbol include/simuscop_amd.h declares
ENGINE_SYMBOLS = [
    "sg_create", "sg_destroy", "sg_last_error", "sg_set_stream", "sg_set_seed", "sg_set_strict_bases", "sg_load_profile",
    "sg_upload_haplotypes", "sg_reference_begin", "sg_reference_chunk", "sg_sync", "sg_reference_scan",
    "sg_reference_commit", "sg_build_haplotypes", "sg_haplotype_codes", "sg_compress", "sg_fetch_compressed", "sg_deflate_bgzf",
    "sg_bgzf_eof", "sg_deflate_plan", "sg_detach_outputs", "sg_outputs_sizes", "sg_outputs_fetch",
    "sg_outputs_last_error", "sg_release_outputs", "sg_plan", "sg_sample", "sg_result", "sg_fetch", "sg_device_output",
    "sg_gc_percent", "sg_set_profiling", "sg_kernel_times", "sg_emit_info", "sg_emit_variant", "sg_emit_path", "sg_cdf_count_le", "sg_fetch_range", "sg_host_alloc",
    "sg_sub_row_identity_first", "sg_row_symbols", "sg_alias_row", "sg_window_weights", "sg_windows_build", "sg_plan_windows", "sg_plan_range", "sg_windows_drop",
    "sg_host_free", "sg_profile_prepare", "sg_profile_tables_error", "sg_load_prepared_profile", "sg_profile_tables_free", "sg_train_count",
    "sg_train_begin", "sg_train_feed", "sg_train_capped", "sg_train_finish", "sg_train_end",
    "sg_bgzf_members", "sg_inflate_bgzf", "sg_train_bam_start", "sg_train_feed_bgzf", "sg_train_bam_info",
    "sg_release_cached_memory",
    "sg_truth_align", "sg_truth_map", "sg_truth_pieces", "sg_truth_reads", "sg_truth_bam", "sg_fetch_truth", "sg_truth_info",
    "sg_truth_bam_tags", "sg_truth_tag_info", "sg_truth_tags",
    "sg_bamsort_pass", "sg_bamsort_merge", "sg_bamsort_index", "sg_bamsort_fetch",
    "sg_bamindex_begin", "sg_bamindex_add", "sg_bamindex_chunks", "sg_bamindex_finish", "sg_bamindex_end",
    "sg_depth_begin", "sg_depth_add", "sg_depth_add_spans", "sg_depth_bins", "sg_depth_runs", "sg_depth_fetch", "sg_depth_reset",
    "sg_depth_info", "sg_depth_end",
    "sg_variants_begin", "sg_variants_add", "sg_variants_counts", "sg_variants_reset", "sg_variants_info", "sg_variants_end",
    "sg_variant_observe",
    "sg_errtab_begin", "sg_errtab_add", "sg_errtab_counts", "sg_errtab_reset", "sg_errtab_info", "sg_errtab_end", "sg_errtab_observe",
    "sg_eval_begin", "sg_eval_truth_bgzf", "sg_eval_truth_done", "sg_eval_test_refmap", "sg_eval_test_bgzf", "sg_eval_finish", "sg_eval_end",
    "sg_eval_classify", "sg_eval_key",
    "sg_vcf_begin", "sg_vcf_feed", "sg_vcf_feed_bgzf", "sg_vcf_undecided", "sg_vcf_finish", "sg_vcf_rows", "sg_vcf_end", "sg_vcf_row",
]


class SgTrainCounts(C.Structure):
    """sg_train_counts / orc_train_counts (same layout): caller-allocated count arrays + scalar counters."""
    _fields_ = [("subs1", C.POINTER(C.c_uint64)), ("subs2", C.POINTER(C.c_uint64)), ("kmers", C.POINTER(C.c_uint64)),
                ("quality", C.POINTER(C.c_uint64)), ("isize", C.POINTER(C.c_uint64)),
                ("ins_len", C.POINTER(C.c_uint64)), ("del_len", C.POINTER(C.c_uint64)),
                ("lines", C.c_uint64), ("reads_counted", C.c_uint64), ("cigar_chars", C.c_uint64), ("insert_events", C.c_uint64),
                ("delete_events", C.c_uint64), ("isize_overflow", C.c_uint64), ("indel_len_overflow", C.c_uint64),
                ("skipped_overhang", C.c_uint64), ("gc_rejected", C.c_uint64), ("gc_windows", C.c_uint64), ("capped", C.c_uint64)]


class SgTrainSetup(C.Structure):
    """sg_train_setup (include/simuscop_amd.h)"""
    _fields_ = [("contig_keys", C.POINTER(C.c_char_p)), ("n_contigs", C.c_uint32), ("bases", C.c_char_p), ("kmer", C.c_int32),
                ("bins", C.c_int32), ("n_isize", C.c_uint32), ("n_indel_len", C.c_uint32), ("count_gc", C.c_int32), ("window", C.c_uint32),
                ("max_reads", C.c_uint64),
                ("target_first", C.POINTER(C.c_uint64)), ("target_spos", C.POINTER(C.c_int64)), ("target_epos", C.POINTER(C.c_int64)),
                ("n_snv", C.c_uint64), ("snv_contig", C.POINTER(C.c_uint32)), ("snv_pos", C.POINTER(C.c_int64)), ("snv_alt", C.c_char_p),
                ("snv_homo", C.POINTER(C.c_uint8)),
                ("n_ins", C.c_uint64), ("ins_contig", C.POINTER(C.c_uint32)), ("ins_pos", C.POINTER(C.c_int64)), ("ins_len", C.POINTER(C.c_int32)),
                ("n_del", C.c_uint64), ("del_contig", C.POINTER(C.c_uint32)), ("del_pos", C.POINTER(C.c_int64)), ("del_len", C.POINTER(C.c_int32))]


class SgEvalCounts(C.Structure):
    """sg_eval_counts (include/simuscop_amd.h)"""
    _fields_ = [("test_records", C.c_uint64), ("secondary", C.c_uint64), ("supplementary", C.c_uint64), ("unknown", C.c_uint64),
                ("ambiguous", C.c_uint64), ("repeated", C.c_uint64), ("truth_records", C.c_uint64), ("truth_duplicates", C.c_uint64),
                ("missing", C.c_uint64 * 6), ("truth_bytes", C.c_uint64), ("test_bytes", C.c_uint64),
                ("t_inflate", C.c_double), ("t_truth", C.c_double), ("t_sort", C.c_double), ("t_test", C.c_double)]


SG_EVAL_CELLS = 12288
EVAL_CATEGORIES = ["exact", "near", "wrong_place", "wrong_strand", "wrong_contig", "lost", "invented", "both_unmapped"]
EVAL_CLASSES = ["plain", "edited", "unmapped"]


class SgProfileCdf(C.Structure):
    _fields_ = [("n_bases", C.c_int32), ("bases", C.c_char * 8), ("kmer", C.c_int32), ("bins", C.c_int32),
                ("read_length", C.c_int32), ("n_qual", C.c_int32), ("min_qual", C.c_int32),
                ("insert_rate", C.c_double), ("del_rate", C.c_double),
                ("ins_cdf", C.POINTER(C.c_double)), ("n_ins", C.c_int32),
                ("del_cdf", C.POINTER(C.c_double)), ("n_del", C.c_int32),
                ("subs_cdf1", C.POINTER(C.c_double)), ("subs_cdf2", C.POINTER(C.c_double)),
                ("qual_cdf", C.POINTER(C.c_double)), ("isize_cdf", C.POINTER(C.c_double)),
                ("n_isize", C.c_int32), ("isize_min", C.c_int32), ("insert_size", C.c_int32)]


class SgWindow(C.Structure):
    _fields_ = [("hap_base", C.c_uint64), ("chain", C.c_uint32), ("spos", C.c_uint32), ("len", C.c_uint32),
                ("n_reads", C.c_int32), ("seg", C.c_uint32), ("slot_base", C.c_uint32)]


class SgBatch(C.Structure):
    _fields_ = [("batch_id", C.c_uint32), ("paired", C.c_int32), ("name_prefix", C.c_char_p),
                ("windows", C.POINTER(SgWindow)), ("n_windows", C.c_uint64),
                ("seg_size", C.POINTER(C.c_uint32)), ("seg_first_window", C.POINTER(C.c_uint32)),
                ("n_segs", C.c_uint32), ("first_window", C.c_uint32), ("first_slot", C.c_uint32)]


class SgGcWindow(C.Structure):
    _fields_ = [("start", C.c_uint64), ("chain", C.c_uint32), ("len", C.c_uint32)]


class SgGcModel(C.Structure):
    """sg_gc_model: the GC-bias model of sg_window_weights / sg_windows_build"""
    _fields_ = [("means", C.POINTER(C.c_double)), ("std", C.c_double), ("quantiles", C.POINTER(C.c_double)), ("lg_cells", C.c_uint32),
                ("frag_size", C.c_uint32), ("full_tile_form", C.c_int32), ("ctx24", C.c_uint32)]


class SgWindowGen(C.Structure):
    _fields_ = [("hap_base", C.c_uint64), ("hap_len", C.c_uint64), ("chain", C.c_uint32), ("seg", C.c_uint32), ("first_window", C.c_uint64)]


class SgActiveSeg(C.Structure):
    _fields_ = [("reads", C.c_int64), ("weight", C.c_double), ("seg_size", C.c_uint32), ("pad", C.c_uint32)]


class SgContig(C.Structure):
    _fields_ = [("raw_offset", C.c_uint64), ("length", C.c_uint64), ("line_bases", C.c_uint32), ("line_width", C.c_uint32)]


class SgHapPiece(C.Structure):
    _fields_ = [("dst", C.c_uint64), ("src", C.c_uint64), ("len", C.c_uint32), ("chain", C.c_uint32),
                ("contig", C.c_uint32), ("kind", C.c_uint32)]


class SgTruthPiece(C.Structure):
    """sg_truth_piece: one piece of a chain's copy list, as sg_truth_align takes it"""
    _fields_ = [("dst", C.c_uint64), ("src", C.c_uint64), ("len", C.c_uint32), ("contig", C.c_uint32), ("kind", C.c_uint32),
                ("seg_first", C.c_uint32)]


class SgTruthRead(C.Structure):
    """sg_truth_read: where one read of a pass came from (sg_truth_reads)"""
    _fields_ = [("live", C.c_uint32), ("chain", C.c_uint32), ("reverse", C.c_uint32), ("read_len", C.c_uint32),
                ("tmpl_off", C.c_uint64), ("n_events", C.c_uint32), ("inside", C.c_uint32), ("events", C.c_uint32 * 32)]


class SgTruthTagCounts(C.Structure):
    """sg_truth_tag_counts: what the tags of the last truth_bam() came to (sg_truth_tag_info)"""
    _fields_ = [("n_nm", C.c_uint64), ("n_md", C.c_uint64), ("n_xe", C.c_uint64), ("nm_sum", C.c_uint64), ("xe_sum", C.c_uint64),
                ("md_dropped", C.c_uint64), ("tag_bytes", C.c_uint64), ("max_md", C.c_uint64)]


TAG_NM, TAG_MD, TAG_XE = 1, 2, 4   # SG_TAG_*
TAG_ALL = TAG_NM | TAG_MD | TAG_XE


class SgDepthRun(C.Structure):
    """sg_depth_run: a run of equal depth starts at `start` (sg_depth_runs)"""
    _fields_ = [("start", C.c_uint32), ("depth", C.c_uint32)]


class SgVariant(C.Structure):
    """sg_variant: one row of the variant table (sg_variants_begin, sg_variant_observe)"""
    _fields_ = [("contig", C.c_uint32), ("kind", C.c_uint32), ("pos", C.c_uint64), ("len", C.c_uint32), ("allele", C.c_uint32)]


class SgErrtabShape(C.Structure):
    """sg_errtab_shape: sizes, sums and staging of the true error counts (sg_errtab_info)"""
    _fields_ = [("cycles", C.c_uint32), ("qual_lo", C.c_uint32), ("n_qual", C.c_uint32), ("tmpl_len", C.c_uint32), ("cells", C.c_uint64),
                ("bases", C.c_uint64), ("errors", C.c_uint64), ("skipped", C.c_uint64), ("reads", C.c_uint64),
                ("win_cycles", C.c_uint32), ("lds_bytes", C.c_uint32)]


class SgVcfRecord(C.Structure):
    """sg_vcf_record (include/simuscop_amd.h): one fragment's verdict"""
    _fields_ = [("fragment", C.c_uint64), ("pos", C.c_int64), ("contig", C.c_uint32), ("value", C.c_int32), ("kind", C.c_uint32),
                ("flags", C.c_uint32)]


class SgVcfFragment(C.Structure):
    _fields_ = [("number", C.c_uint64), ("offset", C.c_uint64), ("len", C.c_uint32), ("pad", C.c_uint32)]


class SgVcfCounts(C.Structure):
    _fields_ = [("fragments", C.c_uint64), ("n_snv", C.c_uint64), ("n_ins", C.c_uint64), ("n_del", C.c_uint64), ("kept_snv", C.c_uint64),
                ("kept_ins", C.c_uint64), ("kept_del", C.c_uint64), ("malformed", C.c_uint64), ("malformed_first", C.c_uint64 * 11),
                ("undecided", C.c_uint64), ("text_bytes", C.c_uint64)]


class SgHapPatch(C.Structure):
    _fields_ = [("dst", C.c_uint64), ("chain", C.c_uint32), ("base", C.c_uint32)]


class SimuOptions(C.Structure):
    _fields_ = [("device", C.c_int32), ("has_seed", C.c_int32), ("seed", C.c_uint64), ("write_files", C.c_int32),
                ("fetch", C.c_int32), ("quiet", C.c_int32), ("shard_rank", C.c_int32), ("shard_world", C.c_int32),
                ("output_dir", C.c_char_p), ("repeat_sample", C.c_int32), ("host_haplotypes", C.c_int32), ("gzip", C.c_int32),
                ("shard_contigs", C.c_int32), ("no_eof_block", C.c_int32), ("exchange", C.c_void_p), ("exchange_user", C.c_void_p),
                ("crlf_as_lf", C.c_int32), ("strict_bases", C.c_int32), ("unique_contigs", C.c_int32), ("truth_index", C.c_int32), ("truth_bam", C.c_int32),
                ("truth_tags", C.c_int32), ("truth_sort", C.c_int32), ("truth_errors", C.c_int32), ("truth_variants", C.c_int32), ("truth_depth", C.c_int32)]


# simu_options.exchange: all-reduce(sum) of n doubles over the ranks, in place
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int32)


class SgEmitPathInfo(C.Structure):
    """sg_emit_path_info (include/simuscop_amd.h)"""
    _fields_ = [("main_kernel", C.c_int32), ("slow_rows_lds", C.c_int32), ("lds_bytes", C.c_uint32), ("clean_cap", C.c_uint32)]


class SimuStats(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("fragments", C.c_uint64), ("fastq_bytes", C.c_uint64),
                ("planned_reads", C.c_uint64), ("windows", C.c_uint64), ("segments", C.c_uint64),
                ("batches", C.c_uint64), ("t_load", C.c_double), ("t_haplotypes", C.c_double),
                ("t_plan", C.c_double), ("t_sample", C.c_double), ("t_fetch", C.c_double),
                ("t_write", C.c_double), ("t_total", C.c_double), ("kernel_ms", C.c_float * 8),
                ("queued_items", C.c_uint64), ("requeued_batches", C.c_uint64), ("t_engine", C.c_double),
                ("t_reference", C.c_double), ("t_hap_device", C.c_double), ("t_plan_api", C.c_double), ("t_compress", C.c_double), ("gz_bytes", C.c_uint64),
                ("emit_kernel", C.c_int32), ("emit_slow_rows_lds", C.c_int32), ("emit_lds_bytes", C.c_uint32),
                ("emit_clean_cap", C.c_uint32),
                ("bai_bins", C.c_uint64), ("bai_chunks", C.c_uint64), ("bai_bytes", C.c_uint64), ("t_bai", C.c_double),
                ("truth_records", C.c_uint64), ("truth_unmapped", C.c_uint64), ("truth_bytes", C.c_uint64),
                ("truth_bgzf_bytes", C.c_uint64), ("t_truth", C.c_double),
                ("truth_tag_bytes", C.c_uint64), ("truth_md_dropped", C.c_uint64), ("truth_nm_sum", C.c_uint64), ("truth_xe_sum", C.c_uint64),
                ("truth_sort_runs", C.c_uint64), ("truth_sort_tiles", C.c_uint64), ("truth_spool_bytes", C.c_uint64), ("t_truth_sort", C.c_double),
                ("errors_bases", C.c_uint64), ("errors_subst", C.c_uint64), ("t_errors", C.c_double),
                ("variant_rows", C.c_uint64), ("variant_dropped", C.c_uint64), ("variant_hits", C.c_uint64), ("t_variants", C.c_double),
                ("depth_bases", C.c_uint64), ("depth_rows", C.c_uint64), ("t_depth", C.c_double)]


_engine = None
_host = None


def load_engine():
    """dlopen libsimuscop_amd.so and declare the C ABI.  Raises if it has not been built."""
    global _engine
    if _engine is not None:
        return _engine
    if not os.path.exists(ENGINE_SO):
        raise RuntimeError(f"{ENGINE_SO} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(the HIP engine is the only compute path)")
    lib = C.CDLL(ENGINE_SO, mode=C.RTLD_GLOBAL)
    vp = C.c_void_p
    lib.sg_create.argtypes = [C.POINTER(vp), C.c_int, C.c_uint64]
    lib.sg_destroy.argtypes = [vp]
    lib.sg_destroy.restype = None
    lib.sg_release_cached_memory.restype = None
    lib.sg_release_cached_memory.argtypes = []
    lib.sg_last_error.argtypes = [vp]
    lib.sg_last_error.restype = C.c_char_p
    lib.sg_set_stream.argtypes = [vp, vp]
    lib.sg_set_seed.argtypes = [vp, C.c_uint64]
    lib.sg_load_profile.argtypes = [vp, C.POINTER(SgProfileCdf)]
    lib.sg_upload_haplotypes.argtypes = [vp, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64)]
    lib.sg_reference_begin.argtypes = [vp, C.c_uint64]
    lib.sg_reference_chunk.argtypes = [vp, C.c_uint64, C.c_char_p, C.c_uint64]
    lib.sg_sync.argtypes = [vp]
    lib.sg_reference_scan.argtypes = [vp, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.sg_reference_commit.argtypes = [vp, C.POINTER(SgContig), C.c_uint32]
    lib.sg_train_count.argtypes = [vp, C.c_char_p, C.c_uint64, C.POINTER(C.c_char_p), C.c_uint32, C.c_char_p, C.c_int32, C.c_int32,
                                   C.c_uint32, C.c_uint32, C.POINTER(SgTrainCounts)]
    lib.sg_train_begin.argtypes = [vp, C.POINTER(SgTrainSetup)]
    lib.sg_train_feed.argtypes = [vp, C.c_char_p, C.c_uint64]
    lib.sg_train_capped.argtypes = [vp]
    lib.sg_train_finish.argtypes = [vp, C.POINTER(SgTrainCounts), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint64, C.POINTER(C.c_uint64)]
    lib.sg_train_end.argtypes = [vp]
    lib.sg_train_end.restype = None
    lib.sg_bgzf_members.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint64,
                                    C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.sg_inflate_bgzf.argtypes = [vp, C.c_char_p, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.sg_train_bam_start.argtypes = [vp, C.POINTER(C.c_char_p), C.c_uint32, C.c_uint64]
    lib.sg_train_feed_bgzf.argtypes = [vp, C.c_char_p, C.c_uint64]
    lib.sg_train_bam_info.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    lib.sg_build_haplotypes.argtypes = [vp, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(SgHapPiece), C.c_uint64,
                                        C.c_char_p, C.c_uint64, C.POINTER(SgHapPatch), C.c_uint64]
    lib.sg_haplotype_codes.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_char_p]
    lib.sg_compress.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.sg_fetch_compressed.argtypes = [vp, C.c_int, C.c_uint64, C.c_uint64, C.c_char_p]
    lib.sg_deflate_bgzf.argtypes = [vp, C.c_char_p, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.sg_bgzf_eof.argtypes = [C.c_char_p]
    lib.sg_deflate_plan.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_char_p, C.POINTER(C.c_uint32), C.c_char_p,
                                    C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32]
    lib.sg_deflate_plan.restype = C.c_uint32
    lib.sg_detach_outputs.argtypes = [vp, C.POINTER(vp)]
    lib.sg_outputs_sizes.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.sg_outputs_fetch.argtypes = [vp, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_char_p]
    lib.sg_outputs_last_error.argtypes = [vp]
    lib.sg_outputs_last_error.restype = C.c_char_p
    lib.sg_release_outputs.argtypes = [vp, vp]
    lib.sg_plan.argtypes = [vp, C.POINTER(SgBatch)]
    lib.sg_sample.argtypes = [vp]
    lib.sg_result.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.sg_fetch.argtypes = [vp, vp, vp]
    lib.sg_fetch_range.argtypes = [vp, C.c_int, C.c_uint64, C.c_uint64, vp]
    lib.sg_host_alloc.argtypes = [vp, C.c_uint64, C.POINTER(vp)]
    lib.sg_host_free.argtypes = [vp, vp]
    lib.sg_device_output.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    lib.sg_gc_percent.argtypes = [vp, C.POINTER(SgGcWindow), C.c_uint64, C.POINTER(C.c_int32)]
    lib.sg_window_weights.argtypes = [vp, C.POINTER(SgGcWindow), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(SgGcModel),
                                      C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    lib.sg_windows_build.argtypes = [vp, C.c_uint32, C.POINTER(SgWindowGen), C.c_uint64, C.c_uint32, C.POINTER(SgGcModel), C.POINTER(C.c_double),
                                     C.POINTER(C.c_uint64)]
    lib.sg_plan_windows.argtypes = [vp, C.c_uint32, C.POINTER(SgWindowGen), C.c_uint64, C.POINTER(SgActiveSeg), C.c_uint32, C.c_uint32, C.c_uint32,
                                    C.c_int32, C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.sg_plan_range.argtypes = [vp, C.c_uint32, C.c_uint32]
    lib.sg_windows_drop.argtypes = [vp]
    lib.sg_windows_drop.restype = None
    lib.sg_set_profiling.argtypes = [vp, C.c_int]
    lib.sg_kernel_times.argtypes = [vp, C.POINTER(C.c_float)]
    lib.sg_emit_info.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    lib.sg_emit_variant.argtypes = [vp]
    lib.sg_emit_path.argtypes = [vp, C.POINTER(SgEmitPathInfo)]
    lib.sg_cdf_count_le.argtypes = [C.c_double]
    lib.sg_cdf_count_le.restype = C.c_uint64
    lib.sg_sub_row_identity_first.argtypes = [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)]
    lib.sg_row_symbols.argtypes = [C.POINTER(C.c_double), C.c_int]
    lib.sg_row_symbols.restype = C.c_uint32
    lib.sg_alias_row.argtypes = [C.POINTER(C.c_double), C.c_int, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8),
                                 C.POINTER(C.c_uint8)]
    lib.sg_truth_align.argtypes = [C.POINTER(SgTruthPiece), C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_uint32), C.c_uint32,
                                   C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]
    lib.sg_truth_map.argtypes = [vp, C.POINTER(SgHapPiece), C.c_char_p, C.c_uint64, C.POINTER(C.c_int32), C.c_uint32]
    lib.sg_truth_pieces.argtypes = [vp, C.c_uint32, C.POINTER(SgTruthPiece), C.c_uint64, C.POINTER(C.c_uint64)]
    lib.sg_truth_reads.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(SgTruthRead)]
    lib.sg_truth_bam.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.sg_fetch_truth.argtypes = [vp, C.c_int, C.c_uint64, C.c_uint64, C.c_char_p]
    lib.sg_truth_info.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.sg_truth_bam_tags.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.sg_truth_tag_info.argtypes = [vp, C.POINTER(SgTruthTagCounts)]
    lib.sg_truth_tags.argtypes = [C.POINTER(C.c_uint32), C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint64, C.c_uint32, C.c_char_p, C.c_uint32,
                                  C.c_int, C.POINTER(C.c_uint32), C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                  C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    lib.sg_bamsort_pass.argtypes = [vp, C.c_uint32, u64p, u64p]
    lib.sg_bamsort_merge.argtypes = [vp, C.c_uint32, C.POINTER(vp), u64p, C.POINTER(u64p), C.POINTER(u32p), u64p, u64p, u64p]
    lib.sg_bamsort_index.argtypes = [vp, u64p, u32p, C.c_uint64, u64p]
    lib.sg_bamsort_fetch.argtypes = [vp, C.c_int, C.c_uint64, C.c_uint64, C.c_char_p]
    lib.sg_bamindex_begin.argtypes = [vp, C.c_uint32, u64p]
    lib.sg_bamindex_add.argtypes = [vp, C.c_int, C.c_uint64, C.c_uint64, u32p, C.c_uint64, u64p, u64p]
    lib.sg_bamindex_chunks.argtypes = [vp, C.c_void_p, C.c_uint64, u64p]
    lib.sg_bamindex_finish.argtypes = [vp, u64p, C.c_uint64, u64p]
    lib.sg_bamindex_end.argtypes = [vp]
    lib.sg_depth_begin.argtypes = [vp, u64p, C.c_uint32]
    lib.sg_depth_add.argtypes = [vp, u64p]
    lib.sg_depth_add_spans.argtypes = [vp, u32p, u64p, u64p, C.c_uint64]
    lib.sg_depth_bins.argtypes = [vp, C.c_uint32, C.c_uint64, u64p, C.c_uint64, u64p]
    lib.sg_depth_runs.argtypes = [vp, C.c_uint32, C.POINTER(SgDepthRun), C.c_uint64, u64p]
    lib.sg_depth_fetch.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint64, u32p]
    lib.sg_depth_reset.argtypes = [vp]
    lib.sg_depth_info.argtypes = [vp, u32p, u64p, u32p]
    lib.sg_depth_end.argtypes = [vp]
    u8p = C.POINTER(C.c_uint8)
    lib.sg_variants_begin.argtypes = [vp, C.POINTER(SgVariant), C.c_uint64]
    lib.sg_variants_add.argtypes = [vp, u64p, u64p]
    lib.sg_variants_counts.argtypes = [vp, u32p, C.c_uint64, u64p]
    lib.sg_variants_reset.argtypes = [vp]
    lib.sg_variants_info.argtypes = [vp, u64p, u64p, u64p]
    lib.sg_variants_end.argtypes = [vp]
    lib.sg_variant_observe.argtypes = [C.POINTER(SgTruthPiece), C.c_uint64, u8p, C.c_uint64, C.c_uint32, C.POINTER(SgVariant), C.c_uint64,
                                       u32p, u8p, C.c_uint64, u64p]
    lib.sg_errtab_begin.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.sg_errtab_add.argtypes = [vp, u64p, u64p]
    lib.sg_errtab_counts.argtypes = [vp, u64p, C.c_uint64, u64p]
    lib.sg_errtab_reset.argtypes = [vp]
    lib.sg_errtab_info.argtypes = [vp, C.POINTER(SgErrtabShape)]
    lib.sg_errtab_end.argtypes = [vp]
    lib.sg_errtab_observe.argtypes = [u8p, C.c_uint32, C.c_int, u32p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.c_uint32, C.c_uint32, u64p, C.c_uint64]
    lib.sg_eval_begin.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64]
    lib.sg_eval_truth_bgzf.argtypes = [vp, C.c_char_p, C.c_uint64]
    lib.sg_eval_truth_done.argtypes = [vp, u64p, u64p]
    lib.sg_eval_test_refmap.argtypes = [vp, C.POINTER(C.c_int32), C.c_uint32, C.c_uint64]
    lib.sg_eval_test_bgzf.argtypes = [vp, C.c_char_p, C.c_uint64]
    lib.sg_eval_finish.argtypes = [vp, u64p, C.c_uint64, C.POINTER(SgEvalCounts)]
    lib.sg_eval_end.argtypes = [vp]
    lib.sg_eval_end.restype = None
    lib.sg_eval_classify.argtypes = [C.c_int32, C.c_int64, C.c_uint64, C.c_int, C.c_int, C.c_int32, C.c_int64, C.c_uint64, C.c_int, C.c_int, C.c_uint32]
    lib.sg_eval_classify.restype = C.c_uint32
    lib.sg_eval_key.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.sg_eval_key.restype = C.c_uint64
    lib.sg_vcf_begin.argtypes = [vp, C.POINTER(C.c_char_p), C.c_uint32]
    lib.sg_vcf_feed.argtypes = [vp, C.c_char_p, C.c_uint64]
    lib.sg_vcf_feed_bgzf.argtypes = [vp, C.c_char_p, C.c_uint64]
    lib.sg_vcf_undecided.argtypes = [vp, C.POINTER(SgVcfFragment), C.c_uint64, u64p, C.c_char_p, C.c_uint64, u64p]
    lib.sg_vcf_finish.argtypes = [vp, C.POINTER(SgVcfCounts)]
    lib.sg_vcf_rows.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(SgVcfRecord)]
    lib.sg_vcf_end.argtypes = [vp]
    lib.sg_vcf_row.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(SgVcfRecord)]
    _engine = lib
    return lib


def load_host():
    """dlopen libsimuscop_host.so (C++ host side: config / profile / genome / driver)."""
    global _host
    if _host is not None:
        return _host
    load_engine()
    if not os.path.exists(HOST_SO):
        raise RuntimeError(f"{HOST_SO} is missing: run __graft_entry__.build()")
    lib = C.CDLL(HOST_SO, mode=C.RTLD_GLOBAL)
    vp = C.c_void_p
    lib.simu_default_options.argtypes = [C.POINTER(SimuOptions)]
    lib.simu_default_options.restype = None
    lib.simu_assign_contigs.argtypes = [C.POINTER(C.c_uint64), C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    lib.simu_assign_contigs.restype = None
    lib.simu_run.argtypes = [C.c_char_p, C.POINTER(SimuOptions), C.POINTER(SimuStats), C.c_char_p, C.c_size_t]
    lib.simu_selftest_haplotypes.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_size_t]
    lib.simu_open.argtypes = [C.c_char_p, C.POINTER(SimuOptions), C.POINTER(vp), C.c_char_p, C.c_size_t]
    lib.simu_close.argtypes = [vp]
    lib.simu_close.restype = None
    lib.simu_engine.argtypes = [vp]
    lib.simu_engine.restype = vp
    lib.simu_planned_reads.argtypes = [vp]
    lib.simu_planned_reads.restype = C.c_uint64
    lib.simu_chromosome_count.argtypes = [vp]
    lib.simu_weighted_length.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.c_char_p, C.c_size_t]
    lib.simu_set_reads.argtypes = [vp, C.c_int, C.c_int64, C.c_char_p, C.c_size_t]
    lib.simu_prepare_batch.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    lib.simu_get_stats.argtypes = [vp, C.POINTER(SimuStats)]
    lib.simu_get_stats.restype = None
    lib.simu_batch_slots.argtypes = [vp]
    lib.simu_batch_slots.restype = C.c_uint64
    lib.simu_depth_format.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.simu_depth_format.restype = C.c_uint64
    cpp, u64p = C.POINTER(C.c_char_p), C.POINTER(C.c_uint64)
    lib.simu_variants_format.argtypes = [cpp, u64p, C.c_uint32, cpp, C.c_uint32, C.c_char_p, cpp, C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                         cpp, C.c_uint64, C.POINTER(C.c_uint32), C.c_uint64, C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64,
                                         u64p, u64p]
    lib.simu_variants_format.restype = C.c_uint64
    lib.simu_variant_table.argtypes = [vp, C.c_void_p, C.c_uint64, u64p, C.c_char_p, C.c_size_t]
    lib.simu_errors_format.argtypes = [u64p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint64, u64p]
    lib.simu_errors_format.restype = C.c_uint64
    lib.simu_sort_tiles.argtypes = [C.c_uint32, C.POINTER(u64p), u64p, C.POINTER(u64p), C.c_uint64, u64p, C.POINTER(C.c_uint8), C.c_uint64]
    lib.simu_sort_tiles.restype = C.c_uint64
    lib.simu_bai_build.argtypes = [C.c_uint32, u64p, C.c_void_p, C.c_uint64, u64p, u64p, C.c_void_p, C.c_uint64, u64p, u64p]
    lib.simu_bai_build.restype = C.c_uint64
    _host = lib
    return lib


class SimuError(RuntimeError):
    pass


def default_options(**kw) -> SimuOptions:
    o = SimuOptions()
    load_host().simu_default_options(C.byref(o))
    for k, v in kw.items():
        if k == "seed":
            o.has_seed, o.seed = 1, int(v)
        elif k == "output_dir":
            o.output_dir = v.encode() if isinstance(v, str) else v
        elif k == "exchange":
            o.exchange = C.cast(v, C.c_void_p).value   # an EXCHANGE_FN instance; the caller keeps it alive
        else:
            setattr(o, k, v)
    return o


def run_config(config_path: str, **opts) -> SimuStats:
    """`simuReads <config>` in-process (src/simuReads.cpp main)."""
    lib = load_host()
    o = default_options(**opts)
    st = SimuStats()
    err = C.create_string_buffer(4096)
    rc = lib.simu_run(config_path.encode(), C.byref(o), C.byref(st), err, len(err))
    if rc != 0:
        raise SimuError(f"simuReads failed (exit code {rc}): {err.value.decode(errors='replace')}")
    return st


class SimuTrainOptions(C.Structure):
    """simu_train_options (host/train.h): the options of the reference's seqToProfile + the additive ones"""
    _fields_ = [("bam", C.c_char_p), ("sam", C.c_char_p), ("target", C.c_char_p), ("vcf", C.c_char_p), ("ref", C.c_char_p),
                ("output", C.c_char_p), ("samtools", C.c_char_p), ("kmer", C.c_int32), ("bins", C.c_int32), ("device", C.c_int32),
                ("threads", C.c_int32), ("quiet", C.c_int32), ("stamp", C.c_char_p), ("max_reads", C.c_uint64),
                ("decode_bam", C.c_int32), ("device_vcf", C.c_int32)]


class SimuTrainStats(C.Structure):
    _fields_ = [("lines", C.c_uint64), ("reads_counted", C.c_uint64), ("gc_rejected", C.c_uint64), ("gc_windows", C.c_uint64),
                ("gc_pairs", C.c_uint64), ("skipped_overhang", C.c_uint64), ("sam_bytes", C.c_uint64), ("read_length", C.c_int32),
                ("bins", C.c_int32), ("gc_fitted", C.c_int32), ("capped", C.c_int32), ("t_reference", C.c_double), ("t_reads", C.c_double), ("t_total", C.c_double),
                ("insert_rate", C.c_double), ("del_rate", C.c_double), ("std_isize", C.c_double), ("gc_std", C.c_double),
                ("bam_bytes", C.c_uint64), ("bam_records", C.c_uint64), ("t_inflate", C.c_double),
                ("t_vcf", C.c_double), ("vcf_bytes", C.c_uint64), ("vcf_fragments", C.c_uint64), ("vcf_undecided", C.c_uint64),
                ("vcf_on_device", C.c_int32)]


def train_profile(ref: str, vcf: str, output: str, sam: str = "", bam: str = "", target: str = "", samtools: str = "", kmer: int = 3,
                  bins: int = 50, device: int = 0, quiet: int = 1, stamp: str = None, max_reads: int = 0, decode_bam: bool = False,
                  device_vcf: bool = False) -> SimuTrainStats:
    """`seqToProfile` in-process (src/seqToProfile.cpp main): reads (`sam`: a file of `samtools view` text, or `bam` through
    samtools as the reference does), the sample's VCF and the reference -> a .profile file; the per-read work runs on the GPU.
    A bgzip-compressed `vcf` is inflated and parsed on the GPU; `device_vcf` sends a plain-text one the same way."""
    lib = load_host()
    lib.simu_train_default_options.argtypes = [C.POINTER(SimuTrainOptions)]
    lib.simu_train_default_options.restype = None
    lib.simu_train.argtypes = [C.POINTER(SimuTrainOptions), C.POINTER(SimuTrainStats), C.c_char_p, C.c_size_t]
    o = SimuTrainOptions()
    lib.simu_train_default_options(C.byref(o))
    o.bam, o.sam, o.target, o.vcf, o.ref, o.output, o.samtools = (x.encode() for x in (bam, sam, target, vcf, ref, output, samtools))
    o.kmer, o.bins, o.device, o.quiet, o.max_reads = kmer, bins, device, quiet, max_reads
    o.decode_bam = 1 if decode_bam else 0
    o.device_vcf = 1 if device_vcf else 0
    if stamp is not None:
        o.stamp = stamp.encode()
    st = SimuTrainStats()
    err = C.create_string_buffer(4096)
    rc = lib.simu_train(C.byref(o), C.byref(st), err, len(err))
    if rc != 0:
        raise SimuError(f"seqToProfile failed (exit code {rc}): {err.value.decode(errors='replace')}")
    return st


class SimuEvalOptions(C.Structure):
    """simu_eval_options (host/eval.h)"""
    _fields_ = [("truth", C.c_char_p), ("bam", C.c_char_p), ("output", C.c_char_p), ("min_overlap", C.c_int32), ("device", C.c_int32),
                ("threads", C.c_int32), ("quiet", C.c_int32)]


class SimuEvalStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("test_records", "secondary", "supplementary", "unknown", "ambiguous", "repeated", "truth_records",
                                         "truth_duplicates", "scored", "missing", "truth_bgzf_bytes", "test_bgzf_bytes", "truth_bytes", "test_bytes")] + \
               [(n, C.c_double) for n in ("t_inflate", "t_truth", "t_sort", "t_test", "t_total")]


def truth_eval(truth: str, bam: str, output: str = "", min_overlap: int = 10, device: int = 0, quiet: int = 1) -> SimuEvalStats:
    """`truthEval` in-process (host/eval.h): the aligner's `bam` scored against the `truth` BAM; eval.tsv goes to `output`."""
    lib = load_host()
    lib.simu_eval_default_options.argtypes = [C.POINTER(SimuEvalOptions)]
    lib.simu_eval_default_options.restype = None
    lib.simu_eval.argtypes = [C.POINTER(SimuEvalOptions), C.POINTER(SimuEvalStats), C.c_char_p, C.c_size_t]
    o = SimuEvalOptions()
    lib.simu_eval_default_options(C.byref(o))
    o.truth, o.bam, o.output = truth.encode(), bam.encode(), output.encode()
    o.min_overlap, o.device, o.quiet = min_overlap, device, quiet
    st = SimuEvalStats()
    err = C.create_string_buffer(4096)
    rc = lib.simu_eval(C.byref(o), C.byref(st), err, len(err))
    if rc != 0:
        raise SimuError(f"truthEval failed (exit code {rc}): {err.value.decode(errors='replace')}")
    return st


def truth_align(pieces, tmpl_off: int, tmpl_len: int, reverse: bool, events=(), cap: int = 512):
    """sg_truth_align (host only, no GPU): the true alignment of a template of `tmpl_len` chain bases at `tmpl_off`.
    `pieces`: (dst, src, len, contig, kind, seg_first) of the chain in offset order; `events`: ev_pack words in read
    direction.  Returns (contig, pos0, [(len, op)]); contig -1 and no operations for an unmapped read."""
    lib = load_engine()
    arr = (SgTruthPiece * len(pieces))(*[SgTruthPiece(*p) for p in pieces])
    ev = (C.c_uint32 * max(len(events), 1))(*events)
    contig, pos0, n_ops = C.c_int32(), C.c_int64(), C.c_uint32()
    cigar = (C.c_uint32 * cap)()
    rc = lib.sg_truth_align(arr, len(pieces), tmpl_off, tmpl_len, 1 if reverse else 0, ev, len(events), C.byref(contig), C.byref(pos0),
                            cigar, cap, C.byref(n_ops))
    if rc != 0:
        raise SimuError(f"sg_truth_align failed (code {rc})")
    return contig.value, pos0.value, [(cigar[i] >> 4, cigar[i] & 15) for i in range(n_ops.value)]


def release_cached_memory() -> None:
    """Device blocks that finished contexts left with the process go back to the runtime (sg_release_cached_memory)."""
    load_engine().sg_release_cached_memory()


def depth_format(name: str, ln: int, bin_width: int, data) -> bytes:
    """simu_depth_format (host only, no GPU): one contig's rows of a --truth-depth bedGraph file.  `data`: (start, depth)
    pairs for bin_width == 1, the bins' sums otherwise."""
    lib = load_host()
    n = len(data)
    if bin_width == 1:
        arr = (SgDepthRun * max(n, 1))(*[SgDepthRun(int(a), int(b)) for a, b in data])
    else:
        arr = (C.c_uint64 * max(n, 1))(*[int(v) for v in data])
    rows = C.c_uint64()
    need = lib.simu_depth_format(name.encode(), ln, bin_width, arr, n, None, 0, C.byref(rows))
    if need == 2 ** 64 - 1:
        raise SimuError("simu_depth_format: the data does not describe a contig of that length")
    buf = C.create_string_buffer(max(int(need), 1))
    lib.simu_depth_format(name.encode(), ln, bin_width, arr, n, buf, need, C.byref(rows))
    return buf.raw[:need]


def _variant_rows(rows):
    """(contig, kind, pos, len, allele) tuples -> an SgVariant array; an allele may be a letter"""
    arr = (SgVariant * max(len(rows), 1))()
    for i, (contig, kind, pos, ln, allele) in enumerate(rows):
        arr[i] = SgVariant(int(contig), int(kind), int(pos), int(ln), ord(allele) if isinstance(allele, str) else int(allele))
    return arr


def variant_observe(pieces, codes, tmpl_off: int, tmpl_len: int, rows, cap: int = 1024):
    """sg_variant_observe (host only, no GPU): what one template counts.  `pieces`: (dst, src, len, contig, kind, seg_first)
    of the chain in offset order; `codes`: the template's tmpl_len chain base codes (A0 C1 T2 G3); `rows`: the sorted
    table as (contig, kind, pos, len, allele) tuples (pieces and rows may be ctypes arrays made before, codes a
    contiguous numpy uint8 array).  Returns [(row index, is_alt)], one entry per count of total."""
    lib = load_engine()
    arr = pieces if isinstance(pieces, C.Array) else (SgTruthPiece * len(pieces))(*[SgTruthPiece(*p) for p in pieces])
    if hasattr(codes, "ctypes"):   # a numpy uint8 array
        cod = codes.ctypes.data_as(C.POINTER(C.c_uint8))
    else:
        cod = (C.c_uint8 * max(len(codes), 1))(*[int(c) for c in codes])
    tab = rows if isinstance(rows, C.Array) else _variant_rows(rows)
    n_rows = len(rows)
    while True:
        hr, ha, n = (C.c_uint32 * cap)(), (C.c_uint8 * cap)(), C.c_uint64()
        rc = lib.sg_variant_observe(arr, len(pieces), cod, tmpl_off, tmpl_len, tab, n_rows, hr, ha, cap, C.byref(n))
        if rc != 0:
            raise SimuError(f"sg_variant_observe failed (code {rc})")
        if n.value <= cap:
            return [(hr[i], bool(ha[i])) for i in range(n.value)]
        cap = n.value


def variants_format(contigs, populations, rows, counts=None, want_table: bool = False):
    """simu_variants_format (host only, no GPU): a --truth-variants file made from raw input rows.  `contigs`: (name,
    length) in BAM refID order; `populations`: names in config order; `rows`: (kind, contig name, 1-based pos, population
    index, text) with kind 's' / 'p' / 'i' / 'd' and text the alt base, the inserted sequence or the deletion length;
    `counts`: (alt, total) per table row, or None for zeros.  Returns (text, table rows, dropped input rows), and with
    want_table the table as (contig, kind, pos, len, allele) tuples as a fourth item."""
    lib = load_host()
    n_c, n_p, n = len(contigs), len(populations), len(rows)
    cn = (C.c_char_p * max(n_c, 1))(*[c[0].encode() for c in contigs])
    cl = (C.c_uint64 * max(n_c, 1))(*[int(c[1]) for c in contigs])
    pn = (C.c_char_p * max(n_p, 1))(*[p.encode() for p in populations])
    kind = b"".join(r[0].encode() for r in rows)
    rc = (C.c_char_p * max(n, 1))(*[r[1].encode() for r in rows])
    pos = (C.c_int64 * max(n, 1))(*[int(r[2]) for r in rows])
    pop = (C.c_int32 * max(n, 1))(*[int(r[3]) for r in rows])
    txt = (C.c_char_p * max(n, 1))(*[str(r[4]).encode() for r in rows])
    n_rows, dropped = C.c_uint64(), C.c_uint64()
    cnt, n_cnt = None, 0
    if counts is not None:
        flat = [int(v) for pair in counts for v in pair]
        cnt, n_cnt = (C.c_uint32 * max(len(flat), 1))(*flat), len(counts)
    call = lambda tab, cap_t, out, cap: lib.simu_variants_format(cn, cl, n_c, pn, n_p, kind, rc, pos, pop, txt, n, cnt, n_cnt, tab, cap_t, out, cap,
                                                                 C.byref(n_rows), C.byref(dropped))
    need = call(None, 0, None, 0)
    if need == 2 ** 64 - 1:
        raise SimuError(f"simu_variants_format: the counts do not fit the table of {n_rows.value} rows")
    buf = C.create_string_buffer(max(int(need), 1))
    tab = (SgVariant * max(n_rows.value, 1))()
    call(C.cast(tab, C.c_void_p), n_rows.value, buf, need)
    res = (buf.raw[:need], n_rows.value, dropped.value)
    if want_table:
        res += ([(v.contig, v.kind, v.pos, v.len, v.allele) for v in tab[:n_rows.value]],)
    return res


def truth_tags(cigar, seq: bytes, ref_codes: bytes, md_cap: int = 2048, tmpl_codes=None, reverse: bool = False, events=(), read: bytes = b""):
    """sg_truth_tags (host only, no GPU): the tags of one truth BAM record.  `cigar`: len << 4 | op words (empty: an unmapped
    record), `seq`: SEQ in BAM orientation, `ref_codes`: the contig's base codes from POS on; `tmpl_codes`: the template's
    chain codes in chain direction (None: the template does not lie in its chain), `events`: ev_pack words in read
    direction, `read`: the read in FASTQ orientation.  Returns (present, NM, MD text or None, XE or None)."""
    lib = load_engine()
    ops = (C.c_uint32 * max(len(cigar), 1))(*[int(v) for v in cigar])
    ev = (C.c_uint32 * max(len(events), 1))(*[int(e) for e in events])
    present, nm, md_len, xe = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    md = C.create_string_buffer(max(md_cap, 1))
    rc = lib.sg_truth_tags(ops, len(cigar), bytes(seq), len(seq), bytes(ref_codes), len(ref_codes), md_cap,
                           None if tmpl_codes is None else bytes(tmpl_codes), 0 if tmpl_codes is None else len(tmpl_codes), 1 if reverse else 0,
                           ev, len(events), bytes(read), len(read), C.byref(present), C.byref(nm), md, C.byref(md_len), C.byref(xe))
    if rc != 0:
        raise SimuError(f"sg_truth_tags refused the record (code {rc})")
    p = present.value
    return p, (nm.value if p & TAG_NM else None), (md.raw[:md_len.value] if p & TAG_MD else None), (xe.value if p & TAG_XE else None)


BAMSORT_TILE = 1024   # SG_BAMSORT_TILE: records one block of the device sort takes


def _bamsort_index(eng, ctx):
    n = C.c_uint64()
    rc = eng.sg_bamsort_index(ctx, None, None, 0, C.byref(n))
    if rc != 0:
        raise SimuError(f"sg_bamsort_index: {eng.sg_last_error(ctx).decode(errors='replace')}")
    keys, lens = (C.c_uint64 * max(1, n.value))(), (C.c_uint32 * max(1, n.value))()
    rc = eng.sg_bamsort_index(ctx, keys, lens, n.value, C.byref(n))
    if rc != 0:
        raise SimuError(f"sg_bamsort_index: {eng.sg_last_error(ctx).decode(errors='replace')}")
    return list(keys[:n.value]), list(lens[:n.value])


def _bamsort_fetch(eng, ctx, compressed: bool, nbytes: int, offset: int = 0) -> bytes:
    buf = C.create_string_buffer(max(1, nbytes))
    rc = eng.sg_bamsort_fetch(ctx, 1 if compressed else 0, offset, nbytes, buf)
    if rc != 0:
        raise SimuError(f"sg_bamsort_fetch: {eng.sg_last_error(ctx).decode(errors='replace')}")
    return buf.raw[:nbytes]


def bamsort_merge(ctx, runs):
    """sg_bamsort_merge on an engine context (a c_void_p from sg_create, or Session.ctx): `runs` is a list of (records:
    bytes, keys, lens), a run's records back to back.  Returns (record stream, BGZF members, keys, lens), the stream
    sorted stably by key and the index in its order."""
    eng = load_engine()
    R = len(runs)
    recs = (C.c_void_p * max(1, R))()
    nbytes, counts = (C.c_uint64 * max(1, R))(), (C.c_uint64 * max(1, R))()
    keyp, lenp = (C.POINTER(C.c_uint64) * max(1, R))(), (C.POINTER(C.c_uint32) * max(1, R))()
    keep = []
    for r, (records, keys, lens) in enumerate(runs):
        rb = C.create_string_buffer(bytes(records), max(1, len(records)))
        ka, la = (C.c_uint64 * max(1, len(keys)))(*keys), (C.c_uint32 * max(1, len(lens)))(*lens)
        keep += [rb, ka, la]
        recs[r] = C.cast(rb, C.c_void_p)
        nbytes[r], counts[r] = len(records), len(keys)
        keyp[r], lenp[r] = C.cast(ka, C.POINTER(C.c_uint64)), C.cast(la, C.POINTER(C.c_uint32))
    ob, gb = C.c_uint64(), C.c_uint64()
    rc = eng.sg_bamsort_merge(ctx, R, recs, nbytes, keyp, lenp, counts, C.byref(ob), C.byref(gb))
    if rc != 0:
        raise SimuError(f"sg_bamsort_merge (code {rc}): {eng.sg_last_error(ctx).decode(errors='replace')}")
    keys, lens = _bamsort_index(eng, ctx)
    return _bamsort_fetch(eng, ctx, False, ob.value), _bamsort_fetch(eng, ctx, True, gb.value), keys, lens


BAMINDEX_MERGE, BAMINDEX_DEFLATE = 0, 1   # SG_BAMINDEX_*: whose records sg_bamindex_add indexes
BAI_OPEN = 2 ** 64 - 1                    # the end of the chunk that ends a call, until the caller closes it


def _bamindex_check(eng, ctx, rc, who):
    if rc != 0:
        raise SimuError(f"{who} (code {rc}): {eng.sg_last_error(ctx).decode(errors='replace')}")


def bamindex_begin(ctx, ref_len) -> None:
    """sg_bamindex_begin on an engine context: a stem of len(ref_len) references starts."""
    eng = load_engine()
    _bamindex_check(eng, ctx, eng.sg_bamindex_begin(ctx, len(ref_len), (C.c_uint64 * max(1, len(ref_len)))(*ref_len)), "sg_bamindex_begin")


def bamindex_add(ctx, source: int, file_offset: int, skip: int = 0, lens=None):
    """sg_bamindex_add: index the records of the context's latest compression (BAMINDEX_MERGE: of bamsort_merge;
    BAMINDEX_DEFLATE: of sg_deflate_bgzf, with the lengths of the records that start in its text).  Returns (chunk rows
    [(key, beg, end)] grouped by key = refID << 32 | bin, first_voff)."""
    eng = load_engine()
    nc, fv = C.c_uint64(), C.c_uint64()
    n = 0 if lens is None else len(lens)
    la = None if lens is None else (C.c_uint32 * max(1, n))(*lens)
    _bamindex_check(eng, ctx, eng.sg_bamindex_add(ctx, source, file_offset, skip, la, n, C.byref(nc), C.byref(fv)), "sg_bamindex_add")
    return bamindex_chunks(ctx), fv.value


def bamindex_chunks(ctx):
    """sg_bamindex_chunks: the chunk rows of the last bamindex_add as [(key, beg, end)]."""
    eng = load_engine()
    n = C.c_uint64()
    _bamindex_check(eng, ctx, eng.sg_bamindex_chunks(ctx, None, 0, C.byref(n)), "sg_bamindex_chunks")
    rows = (C.c_uint64 * max(1, 3 * n.value))()
    _bamindex_check(eng, ctx, eng.sg_bamindex_chunks(ctx, rows, n.value, C.byref(n)), "sg_bamindex_chunks")
    return [(rows[3 * i], rows[3 * i + 1], rows[3 * i + 2]) for i in range(n.value)]


def bamindex_finish(ctx, ref_len):
    """sg_bamindex_finish: (linear index cells of all references back to back, counts[3 n_ref + 1])."""
    eng = load_engine()
    n_win = sum((ln + 16383) >> 14 for ln in ref_len)
    lin, cnt = (C.c_uint64 * max(1, n_win))(), (C.c_uint64 * (3 * len(ref_len) + 1))()
    _bamindex_check(eng, ctx, eng.sg_bamindex_finish(ctx, lin, n_win, cnt), "sg_bamindex_finish")
    return list(lin[:n_win]), list(cnt)


def deflate_bgzf(ctx, text: bytes) -> bytes:
    """sg_deflate_bgzf on an engine context: the BGZF members of `text` (no end-of-file block)."""
    eng = load_engine()
    cap = len(text) + len(text) // 2 + 1024 * (len(text) // 32768 + 2)
    out, n = C.create_string_buffer(cap), C.c_uint64()
    _bamindex_check(eng, ctx, eng.sg_deflate_bgzf(ctx, text, len(text), out, cap, C.byref(n)), "sg_deflate_bgzf")
    return out.raw[:n.value]


VCF_KINDS = ("skip", "snv", "ins", "del", "malformed", "undecided")   # SG_VCF_*
VCF_HOMO, VCF_KNOWN = 1, 2


def _vcf_check(eng, ctx, rc, who):
    if rc != 0:
        raise SimuError(f"{who} failed ({rc}): {eng.sg_last_error(ctx).decode(errors='replace')}")


def _vcf_keys(keys):
    keys = [k if isinstance(k, bytes) else k.encode() for k in keys]
    return (C.c_char_p * max(len(keys), 1))(*keys), len(keys)


def vcf_row(fragment: bytes, keys):
    """sg_vcf_row (host only, no GPU): the verdict on one fragment of at most 19,999 bytes.  Returns (kind, pos, contig, value,
    flags) with kind one of VCF_KINDS."""
    lib = load_engine()
    arr, n = _vcf_keys(keys)
    r = SgVcfRecord()
    rc = lib.sg_vcf_row(fragment, len(fragment), arr, n, C.byref(r))
    if rc != 0:
        raise SimuError(f"sg_vcf_row failed ({rc})")
    return VCF_KINDS[r.kind], r.pos, r.contig, r.value, r.flags


def vcf_begin(ctx, keys) -> None:
    """sg_vcf_begin on a bare engine context `ctx` (sg_create)."""
    eng = load_engine()
    arr, n = _vcf_keys(keys)
    _vcf_check(eng, ctx, eng.sg_vcf_begin(ctx, arr, n), "sg_vcf_begin")


def vcf_undecided(ctx):
    """sg_vcf_undecided: [(fragment number, bytes)] of the last feed."""
    eng = load_engine()
    n, nb = C.c_uint64(), C.c_uint64()
    rc = eng.sg_vcf_undecided(ctx, None, 0, C.byref(n), None, 0, C.byref(nb))
    if rc == 0 and n.value == 0:
        return []
    rows, buf = (SgVcfFragment * n.value)(), C.create_string_buffer(max(nb.value, 1))
    _vcf_check(eng, ctx, eng.sg_vcf_undecided(ctx, rows, n.value, C.byref(n), buf, nb.value, C.byref(nb)), "sg_vcf_undecided")
    return [(r.number, buf.raw[r.offset:r.offset + r.len]) for r in rows]


def vcf_feed(ctx, text: bytes, bgzf: bool = False):
    """sg_vcf_feed / sg_vcf_feed_bgzf; returns the feed's undecided fragments (vcf_undecided)."""
    eng = load_engine()
    call, who = (eng.sg_vcf_feed_bgzf, "sg_vcf_feed_bgzf") if bgzf else (eng.sg_vcf_feed, "sg_vcf_feed")
    _vcf_check(eng, ctx, call(ctx, text, len(text)), who)
    return vcf_undecided(ctx)


def vcf_finish(ctx):
    """sg_vcf_finish -> (SgVcfCounts, the undecided fragments of the flushed last line)"""
    eng = load_engine()
    c = SgVcfCounts()
    _vcf_check(eng, ctx, eng.sg_vcf_finish(ctx, C.byref(c)), "sg_vcf_finish")
    return c, vcf_undecided(ctx)


def vcf_rows(ctx, kind: str, n: int, first: int = 0):
    """sg_vcf_rows: kept rows of `kind` ("snv", "ins", "del") as (fragment, pos, contig, value, flags) tuples"""
    eng = load_engine()
    rows = (SgVcfRecord * max(n, 1))()
    _vcf_check(eng, ctx, eng.sg_vcf_rows(ctx, VCF_KINDS.index(kind), first, n, rows), "sg_vcf_rows")
    return [(r.fragment, r.pos, r.contig, r.value, r.flags) for r in rows[:n]]


def vcf_end(ctx) -> None:
    load_engine().sg_vcf_end(ctx)


def bai_build(ref_len, rows, linear, counts):
    """simu_bai_build (host only, no GPU): the bytes of a BAI from chunk rows [(key, beg, end)] of all calls in call order
    with every open end closed, the linear cells and the counts.  Returns (bytes, bins, chunks)."""
    lib = load_host()
    R = len(ref_len)
    flat = (C.c_uint64 * max(1, 3 * len(rows)))(*[v for row in rows for v in row])
    la, ca, ra = (C.c_uint64 * max(1, len(linear)))(*linear), (C.c_uint64 * len(counts))(*counts), (C.c_uint64 * max(1, R))(*ref_len)
    bins, chunks = C.c_uint64(), C.c_uint64()
    n = lib.simu_bai_build(R, ra, flat, len(rows), la, ca, None, 0, C.byref(bins), C.byref(chunks))
    if n == 2 ** 64 - 1:
        raise SimuError("simu_bai_build refused the tables")
    out = C.create_string_buffer(max(1, n))
    lib.simu_bai_build(R, ra, flat, len(rows), la, ca, out, n, C.byref(bins), C.byref(chunks))
    return out.raw[:n], bins.value, chunks.value


def sort_tiles(runs, budget: int):
    """simu_sort_tiles (host only, no GPU): how --truth-sort cuts the key space of sorted runs into tiles.  `runs`: a list
    of (ascending keys, record lengths).  Returns [(first key, single)], ascending: tile i holds first_i <= key <
    first_(i+1), the last all from its first on; single: one key value that alone exceeds the budget."""
    lib = load_host()
    R = len(runs)
    keyp, prep = (C.POINTER(C.c_uint64) * max(1, R))(), (C.POINTER(C.c_uint64) * max(1, R))()
    counts = (C.c_uint64 * max(1, R))()
    keep = []
    for r, (keys, lens) in enumerate(runs):
        pre = [0]
        for v in lens:
            pre.append(pre[-1] + v)
        ka, pa = (C.c_uint64 * max(1, len(keys)))(*keys), (C.c_uint64 * len(pre))(*pre)
        keep += [ka, pa]
        keyp[r], prep[r], counts[r] = C.cast(ka, C.POINTER(C.c_uint64)), C.cast(pa, C.POINTER(C.c_uint64)), len(keys)
    n = lib.simu_sort_tiles(R, keyp, counts, prep, budget, None, None, 0)
    if n == 2 ** 64 - 1:
        raise SimuError("simu_sort_tiles refused the runs")
    first, single = (C.c_uint64 * max(1, n))(), (C.c_uint8 * max(1, n))()
    lib.simu_sort_tiles(R, keyp, counts, prep, budget, first, single, n)
    return [(first[i], bool(single[i])) for i in range(n)]


def errors_cells(cycles: int, n_qual: int, tmpl_len: int) -> int:
    """Cells of the true error counts' flat table (sg_errtab_counts): Q [2][cycles][n_qual][4] (bases, errors, other,
    inserted) | S [2][4][5] (from A C T G, to A C T G N) | I [2][L][2] | D [2][L][2] (events, bases)."""
    return 8 * cycles * n_qual + 40 + 8 * tmpl_len


def errors_observe(table, codes, reverse: bool, events, bases: bytes, quals: bytes, mate: int, cycles: int, qual_lo: int, n_qual: int) -> None:
    """sg_errtab_observe (host only, no GPU): add what one read counts into `table`, a contiguous numpy uint64 array of
    errors_cells(cycles, n_qual, len(codes)) cells.  `codes`: the template's chain base codes (A0 C1 T2 G3, N 4 ...) in chain
    direction, a numpy uint8 array or a sequence; `events`: ev_pack words in read direction; `mate` 0 / 1.  A refused read
    raises SimuError and adds nothing."""
    lib = load_engine()
    if hasattr(codes, "ctypes"):
        cod = codes.ctypes.data_as(C.POINTER(C.c_uint8))
    else:
        cod = (C.c_uint8 * max(len(codes), 1))(*[int(c) for c in codes])
    ev = (C.c_uint32 * max(len(events), 1))(*[int(e) for e in events])
    if len(bases) != len(quals):
        raise ValueError("errors_observe: bases and qualities differ in length")
    rc = lib.sg_errtab_observe(cod, len(codes), 1 if reverse else 0, ev, len(events), bytes(bases), bytes(quals), len(bases), mate, cycles, qual_lo,
                               n_qual, table.ctypes.data_as(C.POINTER(C.c_uint64)), table.size)
    if rc != 0:
        raise SimuError(f"sg_errtab_observe refused the read (code {rc})")


def errors_format(table, cycles: int, qual_lo: int, n_qual: int, tmpl_len: int, mates: int):
    """simu_errors_format (host only, no GPU): the text of a --truth-errors file made of a table in sg_errtab_counts'
    layout (a contiguous numpy uint64 array).  Returns (text, data lines)."""
    lib = load_host()
    rows = C.c_uint64()
    ptr = table.ctypes.data_as(C.POINTER(C.c_uint64))
    need = lib.simu_errors_format(ptr, table.size, cycles, qual_lo, n_qual, tmpl_len, mates, None, 0, C.byref(rows))
    if need == 2 ** 64 - 1:
        raise SimuError("simu_errors_format: the table does not have the size these dimensions give, or mates is not 1 or 2")
    buf = C.create_string_buffer(max(int(need), 1))
    lib.simu_errors_format(ptr, table.size, cycles, qual_lo, n_qual, tmpl_len, mates, buf, need, C.byref(rows))
    return buf.raw[:need], rows.value


class Session:
    """Step-by-step driver: inputs stay resident in HBM, the caller launches the sampling pass."""

    def __init__(self, config_path: str, **opts):
        self.lib = load_host()
        self.eng = load_engine()
        self._opts = default_options(**opts)
        self._h = C.c_void_p()
        self._err = C.create_string_buffer(4096)
        rc = self.lib.simu_open(config_path.encode(), C.byref(self._opts), C.byref(self._h), self._err, len(self._err))
        if rc != 0:
            raise SimuError(self._err.value.decode(errors="replace"))
        self.ctx = C.c_void_p(self.lib.simu_engine(self._h))

    def _check(self, rc):
        if rc != 0:
            raise SimuError(self._err.value.decode(errors="replace"))

    def _sg(self, rc, what):
        if rc != 0:
            raise SimuError(f"{what}: {self.eng.sg_last_error(self.ctx).decode(errors='replace')}")

    @property
    def planned_reads(self) -> int:
        return int(self.lib.simu_planned_reads(self._h))

    @property
    def n_chromosomes(self) -> int:
        return int(self.lib.simu_chromosome_count(self._h))

    def weighted_length(self, popu: int = 0) -> float:
        wl = C.c_double()
        self._check(self.lib.simu_weighted_length(self._h, popu, C.byref(wl), self._err, len(self._err)))
        return wl.value

    def set_reads(self, reads: int, popu: int = 0) -> None:
        self._check(self.lib.simu_set_reads(self._h, popu, int(reads), self._err, len(self._err)))

    def prepare_batch(self, chrom: int = 0, popu: int = 0) -> bool:
        hw = C.c_int()
        self._check(self.lib.simu_prepare_batch(self._h, popu, chrom, C.byref(hw), self._err, len(self._err)))
        return bool(hw.value)

    @property
    def batch_slots(self) -> int:
        """Planned fragment slots of the prepared batch: truth_reads addresses the reads by slot."""
        return int(self.lib.simu_batch_slots(self._h))

    def set_stream(self, stream_handle: int) -> None:
        self._sg(self.eng.sg_set_stream(self.ctx, C.c_void_p(stream_handle)), "sg_set_stream")

    def set_seed(self, seed: int) -> None:
        self._sg(self.eng.sg_set_seed(self.ctx, int(seed)), "sg_set_seed")

    def sample(self) -> None:
        self._sg(self.eng.sg_sample(self.ctx), "sg_sample")

    def result(self):
        b1, b2, nf = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._sg(self.eng.sg_result(self.ctx, C.byref(b1), C.byref(b2), C.byref(nf)), "sg_result")
        return b1.value, b2.value, nf.value

    def kernel_times(self):
        ms = (C.c_float * 8)()
        self._sg(self.eng.sg_kernel_times(self.ctx, ms), "sg_kernel_times")
        return {n: float(ms[i]) for i, n in enumerate(SG_K_NAMES)}

    def compress(self):
        """BGZF-compress the FASTQ text of the last pass on the device; returns the compressed sizes."""
        g1, g2 = C.c_uint64(), C.c_uint64()
        self._sg(self.eng.sg_compress(self.ctx, C.byref(g1), C.byref(g2)), "sg_compress")
        return g1.value, g2.value

    def fetch_compressed(self, mate: int, nbytes: int, offset: int = 0) -> bytes:
        buf = C.create_string_buffer(max(nbytes, 1))
        self._sg(self.eng.sg_fetch_compressed(self.ctx, mate, offset, nbytes, buf), "sg_fetch_compressed")
        return buf.raw[:nbytes]

    # ---- truth alignments (sessions opened with truth_bam=1: the driver hands the piece map to the engine) ----
    def truth_pieces(self, chain: int):
        """The chain's copy list sorted by offset: (dst, src, len, contig, kind, seg_first) rows for truth_align."""
        n = C.c_uint64()
        self.eng.sg_truth_pieces(self.ctx, chain, None, 0, C.byref(n))
        arr = (SgTruthPiece * max(n.value, 1))()
        self._sg(self.eng.sg_truth_pieces(self.ctx, chain, arr, n.value, C.byref(n)), "sg_truth_pieces")
        return [(p.dst, p.src, p.len, p.contig, p.kind, p.seg_first) for p in arr[:n.value]]

    def truth_reads(self, mate: int, first_slot: int, n: int):
        """Where reads [first_slot, first_slot + n) of mate 0 / 1 of the last pass came from: SgTruthRead rows."""
        arr = (SgTruthRead * max(n, 1))()
        self._sg(self.eng.sg_truth_reads(self.ctx, mate, first_slot, n, arr), "sg_truth_reads")
        return arr

    def truth_bam(self, tags: int = 0):
        """Build the pass's BAM records and their BGZF members on the device; returns (record bytes, BGZF bytes).  `tags`: a
        mask of TAG_NM | TAG_MD | TAG_XE, the optional fields the records carry (0: none, the records of sg_truth_bam)."""
        a, b = C.c_uint64(), C.c_uint64()
        self._sg(self.eng.sg_truth_bam_tags(self.ctx, int(tags), C.byref(a), C.byref(b)), "sg_truth_bam_tags")
        return a.value, b.value

    def truth_tag_info(self):
        """sg_truth_tag_counts of the last truth_bam(): records with each tag, the sums of NM and XE, MD texts dropped, tag
        bytes, and the longest MD text a record carries."""
        out = SgTruthTagCounts()
        self._sg(self.eng.sg_truth_tag_info(self.ctx, C.byref(out)), "sg_truth_tag_info")
        return out

    def fetch_truth(self, compressed: bool, nbytes: int, offset: int = 0) -> bytes:
        buf = C.create_string_buffer(max(nbytes, 1))
        self._sg(self.eng.sg_fetch_truth(self.ctx, 1 if compressed else 0, offset, nbytes, buf), "sg_fetch_truth")
        return buf.raw[:nbytes]

    def truth_info(self):
        """(records, unmapped records) of the last truth_bam()."""
        a, b = C.c_uint64(), C.c_uint64()
        self._sg(self.eng.sg_truth_info(self.ctx, C.byref(a), C.byref(b)), "sg_truth_info")
        return a.value, b.value

    # ---- the truth BAM in coordinate order (sg_bamsort_*) ----
    def bamsort_pass(self, tags: int = 0):
        """sg_bamsort_pass: truth_bam(tags) with the record stream in key order, uncompressed.  Returns (record bytes, records)."""
        a, b = C.c_uint64(), C.c_uint64()
        self._sg(self.eng.sg_bamsort_pass(self.ctx, int(tags), C.byref(a), C.byref(b)), "sg_bamsort_pass")
        return a.value, b.value

    def bamsort_index(self):
        """(keys, lengths) in output order of the last bamsort_pass() or bamsort_merge()."""
        return _bamsort_index(self.eng, self.ctx)

    def bamsort_fetch(self, compressed: bool, nbytes: int, offset: int = 0) -> bytes:
        return _bamsort_fetch(self.eng, self.ctx, compressed, nbytes, offset)

    # ---- true coverage (sessions opened with truth_depth=BIN: the driver hands over the piece map and begins the depth
    # with the reference's contigs at the first prepare_batch; depth_begin starts one over contigs of the caller's) ----
    def depth_begin(self, contig_len) -> None:
        arr = (C.c_uint64 * max(len(contig_len), 1))(*[int(v) for v in contig_len])
        self._sg(self.eng.sg_depth_begin(self.ctx, arr, len(contig_len)), "sg_depth_begin")

    def depth_add(self) -> int:
        """Add the reads of the last pass (after result()); returns the M bases added."""
        mb = C.c_uint64()
        self._sg(self.eng.sg_depth_add(self.ctx, C.byref(mb)), "sg_depth_add")
        return mb.value

    def depth_add_spans(self, contig, start, end) -> None:
        """Add spans [start, end) of contigs (numpy arrays or sequences of equal length)."""
        import numpy as np
        c = np.ascontiguousarray(contig, dtype=np.uint32)
        a = np.ascontiguousarray(start, dtype=np.uint64)
        b = np.ascontiguousarray(end, dtype=np.uint64)
        if not (len(c) == len(a) == len(b)):
            raise ValueError("depth_add_spans: contig, start and end differ in length")
        self._sg(self.eng.sg_depth_add_spans(self.ctx, c.ctypes.data_as(C.POINTER(C.c_uint32)), a.ctypes.data_as(C.POINTER(C.c_uint64)),
                                             b.ctypes.data_as(C.POINTER(C.c_uint64)), len(c)), "sg_depth_add_spans")

    def depth_bins(self, contig: int, bin_width: int):
        """64-bit sums of the per-base depths of the contig's bins of bin_width bases (numpy uint64)."""
        import numpy as np
        n = C.c_uint64()
        self._sg(self.eng.sg_depth_bins(self.ctx, contig, bin_width, None, 0, C.byref(n)), "sg_depth_bins")
        out = np.zeros(n.value, dtype=np.uint64)
        if n.value:
            self._sg(self.eng.sg_depth_bins(self.ctx, contig, bin_width, out.ctypes.data_as(C.POINTER(C.c_uint64)), n.value, C.byref(n)), "sg_depth_bins")
        return out

    def depth_runs(self, contig: int):
        """The contig's runs of equal depth: numpy uint32 [n, 2] of (start, depth)."""
        import numpy as np
        n = C.c_uint64()
        self._sg(self.eng.sg_depth_runs(self.ctx, contig, None, 0, C.byref(n)), "sg_depth_runs")
        out = np.zeros((n.value, 2), dtype=np.uint32)
        if n.value:
            self._sg(self.eng.sg_depth_runs(self.ctx, contig, C.cast(out.ctypes.data, C.POINTER(SgDepthRun)), n.value, C.byref(n)), "sg_depth_runs")
        return out

    def depth_fetch(self, contig: int, first: int, n: int):
        """Per-base depths of bases [first, first + n) (numpy uint32)."""
        import numpy as np
        out = np.zeros(n, dtype=np.uint32)
        self._sg(self.eng.sg_depth_fetch(self.ctx, contig, first, n, out.ctypes.data_as(C.POINTER(C.c_uint32))), "sg_depth_fetch")
        return out

    def depth_reset(self) -> None:
        self._sg(self.eng.sg_depth_reset(self.ctx), "sg_depth_reset")

    def depth_info(self):
        """(contigs, M bases added, bases per tile of the finishing pass)."""
        nc, mb, tile = C.c_uint32(), C.c_uint64(), C.c_uint32()
        self._sg(self.eng.sg_depth_info(self.ctx, C.byref(nc), C.byref(mb), C.byref(tile)), "sg_depth_info")
        return nc.value, mb.value, tile.value

    def depth_end(self) -> None:
        self._sg(self.eng.sg_depth_end(self.ctx), "sg_depth_end")

    # ---- true allele counts (sessions opened with truth_variants=1: the driver hands over the piece map and begins the
    # counts with its own table at the first prepare_batch; variants_begin starts over with a table of the caller's) ----
    def haplotype_codes(self, chain: int, offset: int, n: int):
        """Base codes (A0 C1 T2 G3, N 4) of chain bases [offset, offset + n) on the device (numpy uint8)."""
        import numpy as np
        out = np.zeros(max(n, 1), dtype=np.uint8)
        self._sg(self.eng.sg_haplotype_codes(self.ctx, chain, offset, n, out.ctypes.data_as(C.c_char_p)), "sg_haplotype_codes")
        return out[:n]

    def variant_table(self):
        """The driver's variant table for the open config: (contig, kind, pos, len, allele) tuples, allele an ASCII code."""
        n = C.c_uint64()
        self._check(self.lib.simu_variant_table(self._h, None, 0, C.byref(n), self._err, len(self._err)))
        arr = (SgVariant * max(n.value, 1))()
        self._check(self.lib.simu_variant_table(self._h, C.cast(arr, C.c_void_p), n.value, C.byref(n), self._err, len(self._err)))
        return [(v.contig, v.kind, v.pos, v.len, v.allele) for v in arr[:n.value]]

    def variants_begin(self, rows) -> None:
        self._sg(self.eng.sg_variants_begin(self.ctx, _variant_rows(rows), len(rows)), "sg_variants_begin")

    def variants_add(self):
        """Count the reads of the last pass (after result()); returns (reads with a hit, hits)."""
        a, b = C.c_uint64(), C.c_uint64()
        self._sg(self.eng.sg_variants_add(self.ctx, C.byref(a), C.byref(b)), "sg_variants_add")
        return a.value, b.value

    def variants_counts(self):
        """numpy uint32 [rows, 2] of (alt, total)."""
        import numpy as np
        n = C.c_uint64()
        self._sg(self.eng.sg_variants_counts(self.ctx, None, 0, C.byref(n)), "sg_variants_counts")
        out = np.zeros((n.value, 2), dtype=np.uint32)
        if n.value:
            self._sg(self.eng.sg_variants_counts(self.ctx, out.ctypes.data_as(C.POINTER(C.c_uint32)), n.value, C.byref(n)), "sg_variants_counts")
        return out

    def variants_reset(self) -> None:
        self._sg(self.eng.sg_variants_reset(self.ctx), "sg_variants_reset")

    def variants_info(self):
        """(rows, reads with a hit, hits) since variants_begin / variants_reset."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._sg(self.eng.sg_variants_info(self.ctx, C.byref(a), C.byref(b), C.byref(c)), "sg_variants_info")
        return a.value, b.value, c.value

    def variants_end(self) -> None:
        self._sg(self.eng.sg_variants_end(self.ctx), "sg_variants_end")

    # ---- true error counts (sessions opened with truth_errors=1: the driver begins the table with the profile's cycle
    # capacity and quality range at the first prepare_batch; errors_begin starts over with the caller's) ----
    def errors_begin(self, cycles: int, qual_lo: int, n_qual: int) -> None:
        self._sg(self.eng.sg_errtab_begin(self.ctx, cycles, qual_lo, n_qual), "sg_errtab_begin")

    def errors_add(self):
        """Count the reads of the last pass (after result()); returns (bases, errors) added to those two columns."""
        a, b = C.c_uint64(), C.c_uint64()
        self._sg(self.eng.sg_errtab_add(self.ctx, C.byref(a), C.byref(b)), "sg_errtab_add")
        return a.value, b.value

    def errors_counts(self):
        """The flat table (numpy uint64, errors_cells(...) cells)."""
        import numpy as np
        n = C.c_uint64()
        self._sg(self.eng.sg_errtab_counts(self.ctx, None, 0, C.byref(n)), "sg_errtab_counts")
        out = np.zeros(n.value, dtype=np.uint64)
        self._sg(self.eng.sg_errtab_counts(self.ctx, out.ctypes.data_as(C.POINTER(C.c_uint64)), n.value, C.byref(n)), "sg_errtab_counts")
        return out

    def errors_reset(self) -> None:
        self._sg(self.eng.sg_errtab_reset(self.ctx), "sg_errtab_reset")

    def errors_info(self) -> SgErrtabShape:
        """sg_errtab_shape: cycles, qual_lo, n_qual, tmpl_len, cells, sums since errors_begin / errors_reset, staging."""
        out = SgErrtabShape()
        self._sg(self.eng.sg_errtab_info(self.ctx, C.byref(out)), "sg_errtab_info")
        return out

    def errors_end(self) -> None:
        self._sg(self.eng.sg_errtab_end(self.ctx), "sg_errtab_end")

    def emit_info(self):
        """(items handed to the generic item code, whether the batch was re-emitted) of the last pass."""
        q, r = C.c_uint64(), C.c_int()
        self._sg(self.eng.sg_emit_info(self.ctx, C.byref(q), C.byref(r)), "sg_emit_info")
        return q.value, bool(r.value)

    def fetch(self, n1: int, n2: int):
        b1 = C.create_string_buffer(max(n1, 1))
        b2 = C.create_string_buffer(max(n2, 1))
        self._sg(self.eng.sg_fetch(self.ctx, b1, b2 if n2 else None), "sg_fetch")
        return b1.raw[:n1], b2.raw[:n2]

    def output_md5(self, chunk: int = 1 << 27):
        """md5 of each mate's whole FASTQ text of the last pass, fetched from the device in chunks."""
        import hashlib
        b1, b2, _ = self.result()
        out = []
        buf = C.create_string_buffer(chunk)
        for mate, total in ((0, b1), (1, b2)):
            if mate == 1 and not total:
                break
            h = hashlib.md5()
            for off in range(0, total, chunk):
                n = min(chunk, total - off)
                self._sg(self.eng.sg_fetch_range(self.ctx, mate, off, n, buf), "sg_fetch_range")
                h.update(memoryview(buf)[:n])
            out.append(h.hexdigest())
        return out

    # ---- detached output sets: the text of a pass drains to pinned host memory while the next pass is sampled ----
    def host_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._sg(self.eng.sg_host_alloc(self.ctx, nbytes, C.byref(p)), "sg_host_alloc")
        return p.value

    def host_free(self, ptr: int) -> None:
        self._sg(self.eng.sg_host_free(self.ctx, C.c_void_p(ptr)), "sg_host_free")

    def detach_outputs(self):
        h = C.c_void_p()
        self._sg(self.eng.sg_detach_outputs(self.ctx, C.byref(h)), "sg_detach_outputs")
        return h

    def outputs_sizes(self, h):
        tb, gb = (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
        self.eng.sg_outputs_sizes(h, tb, gb)
        return (tb[0], tb[1]), (gb[0], gb[1])

    def outputs_fetch_into(self, h, mate: int, compressed: bool, offset: int, nbytes: int, host_ptr: int) -> None:
        rc = self.eng.sg_outputs_fetch(h, mate, 1 if compressed else 0, offset, nbytes, C.cast(C.c_void_p(host_ptr), C.c_char_p))
        if rc != 0:
            raise SimuError("sg_outputs_fetch: " + self.eng.sg_outputs_last_error(h).decode(errors="replace"))

    def release_outputs(self, h) -> None:
        self._sg(self.eng.sg_release_outputs(self.ctx, h), "sg_release_outputs")

    def stats(self) -> SimuStats:
        st = SimuStats()
        self.lib.simu_get_stats(self._h, C.byref(st))
        return st

    def close(self):
        if self._h:
            self.lib.simu_close(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
