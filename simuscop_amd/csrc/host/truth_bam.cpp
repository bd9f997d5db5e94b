// host/truth_bam.cpp -- see truth_bam.h
#include "truth_bam.h"

namespace simu {

void TruthBam::open(const std::string& dir, const std::string& stem) {
  if (!opt.write_files) return;
  const std::string a = dir + "/" + stem + ".truth.bam" + simu_shard_suffix(opt);
  file = fopen(a.c_str(), "wb");
  if (!file) throw Error("Error: can not open BAM file to save the true alignments:\n" + a, -1);
  if (opt.shard_world <= 1 || opt.shard_rank == 0) write_header();
  if (opt.truth_sort) {
    if (!tsort) {
      tsort.reset(new TruthSort(eng, st));
      if (opt.truth_index) tsort->index_with(contigs.len);
    }
    tsort->open(a);
  }
}

// magic, header text, reference list (SAMv1 section 4.2) as BGZF members of their own, made by the device compressor
void TruthBam::write_header() {
  std::string text = opt.truth_sort ? "@HD\tVN:1.6\tSO:coordinate\n" : "@HD\tVN:1.6\tSO:unsorted\tGO:query\n";
  for (size_t r = 0; r < contigs.name.size(); r++) text += "@SQ\tSN:" + contigs.name[r] + "\tLN:" + std::to_string(contigs.len[r]) + "\n";
  text += "@PG\tID:simuReads\n";
  std::string h("BAM\1", 4);
  auto put32 = [&](uint32_t v) { for (int i = 0; i < 4; i++) h.push_back((char)(v >> (8 * i))); };
  put32((uint32_t)text.size());
  h += text;
  put32((uint32_t)contigs.name.size());
  for (size_t r = 0; r < contigs.name.size(); r++) {
    put32((uint32_t)contigs.name[r].size() + 1);
    h += contigs.name[r];
    h.push_back('\0');
    put32((uint32_t)contigs.len[r]);
  }
  std::vector<uint8_t> gz(h.size() + h.size() / 2 + 1024 * (h.size() / 32768 + 2));
  uint64_t n = 0;
  eng.check(sg_deflate_bgzf(eng.ctx, h.data(), h.size(), gz.data(), gz.size(), &n), "sg_deflate_bgzf");
  if (fwrite(gz.data(), 1, n, file) != n) throw Error("Error: short write to the truth BAM file", -1);
}

void TruthBam::piece() {
  Timed timed{st.t_truth};
  uint64_t rb = 0, gb = 0, nrec = 0, nun = 0;
  const uint32_t tags = opt.truth_tags ? SG_TAG_NM | SG_TAG_MD | SG_TAG_XE : 0u;
  if (opt.truth_sort) eng.check(sg_bamsort_pass(eng.ctx, tags, &rb, nullptr), "sg_bamsort_pass");   // (uncompressed: gb stays 0 until the merge)
  else if (opt.truth_tags) eng.check(sg_truth_bam_tags(eng.ctx, tags, &rb, &gb), "sg_truth_bam_tags");
  else eng.check(sg_truth_bam(eng.ctx, &rb, &gb), "sg_truth_bam");
  if (opt.truth_tags) {
    sg_truth_tag_counts tc;
    eng.check(sg_truth_tag_info(eng.ctx, &tc), "sg_truth_tag_info");
    st.truth_tag_bytes += tc.tag_bytes;
    st.truth_md_dropped += tc.md_dropped;
    st.truth_nm_sum += tc.nm_sum;
    st.truth_xe_sum += tc.xe_sum;
  }
  eng.check(sg_truth_info(eng.ctx, &nrec, &nun), "sg_truth_info");
  st.truth_records += nrec;
  st.truth_unmapped += nun;
  st.truth_bytes += rb;
  st.truth_bgzf_bytes += gb;
  if (opt.truth_sort) {
    if (file && rb && tsort && tsort->active()) tsort->add_run(rb);
  } else if (file && gb) {
    if (host.size() < gb) host.resize(gb);
    eng.check(sg_fetch_truth(eng.ctx, 1, 0, gb, host.data()), "sg_fetch_truth");
    if (fwrite(host.data(), 1, gb, file) != gb) throw Error("Error: short write to the truth BAM file", -1);
  }
}

void TruthBam::close() {
  if (tsort && tsort->active() && file) tsort->finish(file);   // in front of the end-of-file block (nothing without a spool)
  close_file();
}

void TruthBam::close_file() {
  if (!file) return;
  if (!opt.no_eof_block && (opt.shard_world <= 1 || opt.shard_rank == opt.shard_world - 1)) {
    uint8_t eof[28];
    sg_bgzf_eof(eof);
    fwrite(eof, 1, 28, file);
  }
  fclose(file);
  file = nullptr;
}

}  // namespace simu
