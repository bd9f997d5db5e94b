// host/truth_outputs.cpp -- see truth_outputs.h
#include "truth_outputs.h"

#include <algorithm>
#include <cstring>

#include "truth_bam.h"
#include "truth_errors.h"

namespace simu {

void ContigTable::build(const Fasta& fa) {
  std::vector<std::string> row_name(fa.contigs.size());
  for (const auto& kv : fa.contig_of) {
    auto w = fa.written.find(kv.first);
    row_name[kv.second] = w == fa.written.end() || w->second.empty() ? kv.first : w->second;
  }
  id_of_row.assign(row_name.size(), -1);
  for (size_t r = 0; r < row_name.size(); r++) {
    if (!row_name[r].empty()) {
      id_of_row[r] = (int32_t)name.size();
      name.push_back(row_name[r]);
      len.push_back(fa.contigs[r].length);
    }
    const int32_t dev = fa.dev_row.empty() ? (int32_t)r : fa.dev_row[r];
    if (dev < 0) continue;
    if ((size_t)dev >= id_of_dev.size()) id_of_dev.resize((size_t)dev + 1, 0);
    id_of_dev[(size_t)dev] = std::max(id_of_row[r], 0);   // (an unlisted row has no reads; its entry only has to be valid)
  }
}

uint64_t depth_format(std::string& out, const std::string& name, uint64_t ln, uint64_t bin, const uint64_t* sums, const sg_depth_run* runs,
                      uint64_t n) {
  char buf[96];
  uint64_t rows = 0;
  if (bin == 1) {
    if ((ln == 0) != (n == 0) || (n && runs[0].start != 0)) return UINT64_MAX;
    for (uint64_t i = 0; i < n;) {
      uint64_t j = i + 1;
      while (j < n && runs[j].depth == runs[i].depth) j++;   // (the device's runs differ from their neighbours already)
      for (uint64_t k = i + 1; k <= j && k < n; k++)
        if (runs[k].start <= runs[k - 1].start || runs[k].start >= ln) return UINT64_MAX;
      const uint64_t end = j < n ? runs[j].start : ln;
      const int m = snprintf(buf, sizeof buf, "\t%llu\t%llu\t%llu\n", (unsigned long long)runs[i].start, (unsigned long long)end,
                             (unsigned long long)runs[i].depth);
      out += name;
      out.append(buf, (size_t)m);
      rows++;
      i = j;
    }
    return rows;
  }
  if (bin < 1 || n != (ln + bin - 1) / bin) return UINT64_MAX;
  for (uint64_t k = 0; k < n; k++) {
    const uint64_t a = k * bin, b = std::min(ln, a + bin);
    const int m = snprintf(buf, sizeof buf, "\t%llu\t%llu\t%.4f\n", (unsigned long long)a, (unsigned long long)b,
                           (double)sums[k] / (double)(b - a));
    out += name;
    out.append(buf, (size_t)m);
    rows++;
  }
  return rows;
}

const VariantTable& TruthOutputs::variant_table() {
  if (vtable_built) return vtable;
  vtable_built = true;
  auto ref_id = [&](const std::string& chr) {   // by the variant files' name; -1: a contig the reference does not hold
    const auto it = genome.fa.contig_of.find(chr);
    return it == genome.fa.contig_of.end() ? -1 : contigs.id_of_row[it->second];
  };
  std::vector<VariantIn> in;
  for (size_t q = 0; q < cfg.popu_names.size(); q++) {
    const std::string& popu = cfg.popu_names[q];
    auto each = [&](const auto& by_popu, auto make) {
      const auto it = by_popu.find(popu);
      if (it == by_popu.end()) return;
      for (const auto& kv : it->second) {
        const int32_t id = ref_id(kv.first);
        for (const auto& v : kv.second) in.push_back(make(v, id));
      }
    };
    each(genome.snvs, [&](const SNV& v, int32_t id) { return VariantIn{'s', id, (int64_t)v.pos, (int32_t)q, std::string(1, v.alt), 0}; });
    each(genome.inserts, [&](const Insertion& v, int32_t id) { return VariantIn{'i', id, (int64_t)v.pos, (int32_t)q, v.seq, 0}; });
    each(genome.dels, [&](const Deletion& v, int32_t id) { return VariantIn{'d', id, (int64_t)v.pos, (int32_t)q, std::string(), (int64_t)v.length}; });
  }
  for (const auto& kv : genome.snps) {
    const int32_t id = ref_id(kv.first);
    for (const SNP& v : kv.second) in.push_back(VariantIn{'p', id, (int64_t)v.pos, -1, std::string(1, v.nucleotide), 0});
  }
  vtable.build(in, contigs.len, cfg.popu_names.size());
  st.variant_rows = vtable.rows.size();
  st.variant_dropped = vtable.dropped;
  return vtable;
}

// ---- the lifecycle ----
void TruthOutputs::begin(TruthOutput& o) {
  if (o.begun) return;
  Timed timed{st.*o.timer};
  o.start();
  o.begun = true;
}
void TruthOutputs::begin() { for (TruthOutput& o : outs) begin(o); }

void TruthOutputs::open(const std::string& dir, const std::string& stem) {
  if (bam) bam->open(dir, stem);
  for (TruthOutput& o : outs) {
    begin(o);
    Timed timed{st.*o.timer};
    o.in_stem = true;
    if (!opt.write_files) continue;
    const std::string a = dir + "/" + stem + o.suffix;
    o.file.reset(fopen(a.c_str(), "wb"));
    if (!o.file) throw Error(std::string("Error: can not open ") + o.open_what + ":\n" + a, -1);
  }
}

void TruthOutputs::piece() {
  if (bam) bam->piece();
  for (TruthOutput& o : outs) {
    Timed timed{st.*o.timer};
    o.add();
  }
}

void TruthOutputs::close() {
  if (bam) bam->close();
  for (TruthOutput& o : outs) {
    if (!o.in_stem) continue;
    Timed timed{st.*o.timer};
    o.in_stem = false;
    struct Closer { TruthOutput& o; ~Closer() { o.file.reset(); } } closer{o};
    o.render(o);
    o.reset();
  }
}

void TruthOutput::put(const std::string& text) {
  if (file && !text.empty() && fwrite(text.data(), 1, text.size(), file.get()) != text.size())
    throw Error(std::string("Error: short write to ") + write_what, -1);
}

// ---- the three outputs ----
TruthOutputs::~TruthOutputs() = default;
TruthOutputs::TruthOutputs(Engine& eng_, const simu_options& opt_, simu_stats& st_, const ContigTable& contigs_, const Genome& genome_,
                           const Config& cfg_, const Profile& prof)
    : eng(eng_), opt(opt_), st(st_), contigs(contigs_), genome(genome_), cfg(cfg_) {
  if (opt.truth_bam) bam.reset(new TruthBam(eng, opt, st, contigs));
  if (opt.truth_depth) {
    // the device's runs or bin sums, contig by contig in header order, put into text here
    outs.push_back(TruthOutput{".truth.depth.bedgraph", "bedGraph file to save the true depth", "the true depth's bedGraph file", &simu_stats::t_depth});
    TruthOutput& o = outs.back();
    o.start = [this] { eng.check(sg_depth_begin(eng.ctx, contigs.len.data(), (uint32_t)contigs.len.size()), "sg_depth_begin"); };
    o.add = [this] {
      uint64_t mb = 0;
      eng.check(sg_depth_add(eng.ctx, &mb), "sg_depth_add");
      st.depth_bases += mb;
    };
    o.render = [this](TruthOutput& o) {   // without a file too: the rows are counted
      const uint64_t bin = (uint64_t)opt.truth_depth;
      std::vector<uint64_t> sums;
      std::vector<sg_depth_run> runs;
      std::string text;
      for (size_t c = 0; c < contigs.name.size(); c++) {
        uint64_t n = 0;
        text.clear();
        if (bin == 1) {
          eng.check(sg_depth_runs(eng.ctx, (uint32_t)c, nullptr, 0, &n), "sg_depth_runs");
          if (runs.size() < n) runs.resize(n);
          if (n) eng.check(sg_depth_runs(eng.ctx, (uint32_t)c, runs.data(), n, &n), "sg_depth_runs");
          st.depth_rows += depth_format(text, contigs.name[c], contigs.len[c], 1, nullptr, runs.data(), n);
        } else {
          eng.check(sg_depth_bins(eng.ctx, (uint32_t)c, bin, nullptr, 0, &n), "sg_depth_bins");
          if (sums.size() < n) sums.resize(n);
          if (n) eng.check(sg_depth_bins(eng.ctx, (uint32_t)c, bin, sums.data(), n, &n), "sg_depth_bins");
          st.depth_rows += depth_format(text, contigs.name[c], contigs.len[c], bin, sums.data(), nullptr, n);
        }
        o.put(text);
      }
    };
    o.reset = [this] { eng.check(sg_depth_reset(eng.ctx), "sg_depth_reset"); };
  }
  if (opt.truth_variants) {
    // the table with the device's two counters per row
    outs.push_back(TruthOutput{".truth.variants.tsv", "file to save the true allele counts", "the true allele counts' file", &simu_stats::t_variants});
    TruthOutput& o = outs.back();
    o.start = [this] {
      const std::vector<sg_variant> rows = variant_table().abi();
      eng.check(sg_variants_begin(eng.ctx, rows.data(), rows.size()), "sg_variants_begin");
    };
    o.add = [this] {
      uint64_t rh = 0, h = 0;
      eng.check(sg_variants_add(eng.ctx, &rh, &h), "sg_variants_add");
      st.variant_hits += h;
    };
    o.render = [this](TruthOutput& o) {
      if (!o.file) return;
      std::vector<uint32_t> counts(vtable.rows.size() * 2 + 2);
      uint64_t n = 0;
      eng.check(sg_variants_counts(eng.ctx, counts.data(), vtable.rows.size(), &n), "sg_variants_counts");
      o.put(vtable.format(contigs.name, cfg.popu_names, counts.data()));
    };
    o.reset = [this] { eng.check(sg_variants_reset(eng.ctx), "sg_variants_reset"); };
  }
  if (opt.truth_errors) {
    // the device's table (errors_format, truth_errors.h); the reads are compared with their haplotype templates, so no
    // piece map is involved
    outs.push_back(TruthOutput{".truth.errors.tsv", "file to save the true error counts", "the true error counts' file", &simu_stats::t_errors});
    TruthOutput& o = outs.back();
    o.start = [this, &prof] {
      // cycles: the template plus what SG_MAX_EVENTS insertions of the longest kind can add; qualities: the profile's
      // alphabet, at least the 21 an N draws from (Profile::predict)
      const uint32_t L = (uint32_t)prof.read_length, max_ins = prof.ins_cdf.empty() ? 0u : (uint32_t)prof.ins_cdf.size() - 1u;
      const uint32_t cycles = (uint32_t)std::min<uint64_t>(0xFFFFu, (uint64_t)L + (uint64_t)SG_MAX_EVENTS * max_ins);
      const uint32_t qual_lo = (uint32_t)std::max(0, prof.min_qual - 33), n_qual = (uint32_t)std::max(prof.n_qual, 21);
      eng.check(sg_errtab_begin(eng.ctx, cycles, qual_lo, n_qual), "sg_errtab_begin");
      eng.check(sg_errtab_info(eng.ctx, &errors_shape), "sg_errtab_info");
    };
    o.add = [this] {
      uint64_t b = 0, e = 0;
      eng.check(sg_errtab_add(eng.ctx, &b, &e), "sg_errtab_add");
      st.errors_bases += b;
      st.errors_subst += e;
    };
    o.render = [this](TruthOutput& o) {
      if (!o.file) return;
      const sg_errtab_shape& s = errors_shape;
      std::vector<uint64_t> table(s.cells);
      uint64_t n = 0;
      eng.check(sg_errtab_counts(eng.ctx, table.data(), table.size(), &n), "sg_errtab_counts");
      o.put(errors_format(table.data(), s.cycles, s.qual_lo, s.n_qual, s.tmpl_len, cfg.paired() ? 2u : 1u, nullptr));
    };
    o.reset = [this] { eng.check(sg_errtab_reset(eng.ctx), "sg_errtab_reset"); };
  }
}

}  // namespace simu

extern "C" uint64_t simu_depth_format(const char* name, uint64_t ln, uint64_t bin, const void* data, uint64_t n, char* out, uint64_t cap,
                                      uint64_t* rows) {
  if (!name || (n && !data) || bin < 1) return UINT64_MAX;
  std::string text;
  const uint64_t r = simu::depth_format(text, name, ln, bin, bin == 1 ? nullptr : (const uint64_t*)data,
                                        bin == 1 ? (const sg_depth_run*)data : nullptr, n);
  if (r == UINT64_MAX) return UINT64_MAX;
  if (rows) *rows = r;
  if (out && text.size() <= cap) memcpy(out, text.data(), text.size());
  return text.size();
}
