// host/truth_variants.cpp -- see truth_variants.h
#include "truth_variants.h"

#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <tuple>

#include "simulate.h"

namespace simu {

void VariantTable::build(const std::vector<VariantIn>& in, const std::vector<uint64_t>& contig_len, size_t n_popus) {
  rows.clear();
  dropped = 0;
  struct Keyed { uint32_t contig, rank, a; uint64_t p; size_t src; };
  std::vector<Keyed> keyed;
  keyed.reserve(in.size());
  for (size_t i = 0; i < in.size(); i++) {
    const VariantIn& v = in[i];
    const int64_t p = v.pos - 1;
    if (v.contig < 0 || (size_t)v.contig >= contig_len.size() || p < 0 || (uint64_t)p >= contig_len[(size_t)v.contig] || p > 0xFFFFFFFFll) { dropped++; continue; }
    Keyed k{(uint32_t)v.contig, 0, 0, (uint64_t)p, i};
    if (v.kind == 's' || v.kind == 'p') {
      if (v.text.empty()) { dropped++; continue; }
      k.a = (uint32_t)(unsigned char)toupper((unsigned char)v.text[0]);
    } else if (v.kind == 'i') {
      if (v.text.empty() || v.text.size() > 0xFFFFFFFFull) { dropped++; continue; }
      k.rank = 1;
      k.a = (uint32_t)v.text.size();
    } else if (v.kind == 'd') {
      if (v.len < 1 || v.len > 0xFFFFFFFFll) { dropped++; continue; }
      k.rank = 2;
      k.a = (uint32_t)v.len;
    } else { dropped++; continue; }
    keyed.push_back(k);
  }
  auto key = [](const Keyed& k) { return std::make_tuple(k.contig, k.p, k.rank, k.a); };
  std::stable_sort(keyed.begin(), keyed.end(), [&](const Keyed& x, const Keyed& y) { return key(x) < key(y); });   // equal keys stay in input order
  for (size_t i = 0; i < keyed.size(); i++) {
    const Keyed& k = keyed[i];
    const VariantIn& v = in[k.src];
    if (i == 0 || key(keyed[i - 1]) != key(k)) {
      Row r;
      r.contig = k.contig;
      r.kind = k.rank;
      r.p = k.p;
      r.len = k.rank ? k.a : 0u;
      r.allele = k.rank ? '\0' : (char)k.a;
      r.listed = false;
      if (k.rank == 1) r.seq = v.text;
      r.popus.assign(n_popus, 0);
      rows.push_back(std::move(r));
    }
    Row& r = rows.back();
    if (v.kind != 'p') {
      r.listed = true;
      if (v.popu >= 0 && (size_t)v.popu < n_popus) r.popus[(size_t)v.popu] = 1;
    }
  }
}

std::vector<sg_variant> VariantTable::abi() const {
  std::vector<sg_variant> out(rows.size());
  for (size_t i = 0; i < rows.size(); i++) {
    const Row& r = rows[i];
    out[i] = sg_variant{r.contig, r.kind, r.p, r.len, r.kind ? 0u : (uint32_t)(unsigned char)r.allele};
  }
  return out;
}

std::string VariantTable::format(const std::vector<std::string>& contig_name, const std::vector<std::string>& popu_name, const uint32_t* counts) const {
  std::string out = "#chrom\tpos\ttype\tallele\talt_reads\ttotal_reads\tpopulations\n";
  char buf[96];
  for (size_t i = 0; i < rows.size(); i++) {
    const Row& r = rows[i];
    out += r.contig < contig_name.size() ? contig_name[r.contig] : std::string("?");
    int m = snprintf(buf, sizeof buf, "\t%llu\t%c\t", (unsigned long long)(r.p + 1), r.kind == 0 ? (r.listed ? 's' : 'p') : r.kind == 1 ? 'i' : 'd');
    out.append(buf, (size_t)m);
    if (r.kind == 0) out.push_back(r.allele);
    else if (r.kind == 1) out += r.seq;
    else out += std::to_string(r.len);
    m = snprintf(buf, sizeof buf, "\t%u\t%u\t", counts ? counts[2 * i] : 0u, counts ? counts[2 * i + 1] : 0u);
    out.append(buf, (size_t)m);
    bool any = false;
    if (r.kind != 0 || r.listed)
      for (size_t q = 0; q < r.popus.size() && q < popu_name.size(); q++)
        if (r.popus[q]) {
          if (any) out.push_back(',');
          out += popu_name[q];
          any = true;
        }
    if (!any) out.push_back('.');
    out.push_back('\n');
  }
  return out;
}

}  // namespace simu

extern "C" uint64_t simu_variants_format(const char* const* contig_name, const uint64_t* contig_len, uint32_t n_contigs, const char* const* popu_name,
                                         uint32_t n_popus, const char* kind, const char* const* contig, const int64_t* pos, const int32_t* popu,
                                         const char* const* text, uint64_t n_in, const uint32_t* counts, uint64_t n_counts, void* table,
                                         uint64_t table_cap, char* out, uint64_t cap, uint64_t* rows, uint64_t* dropped) {
  if ((n_contigs && (!contig_name || !contig_len)) || (n_popus && !popu_name) || (n_in && (!kind || !contig || !pos || !popu || !text)))
    return UINT64_MAX;
  std::vector<std::string> cn(contig_name, contig_name + n_contigs), pn(popu_name, popu_name + n_popus);
  std::vector<uint64_t> cl(contig_len, contig_len + n_contigs);
  std::vector<simu::VariantIn> in((size_t)n_in);
  for (uint64_t i = 0; i < n_in; i++) {
    simu::VariantIn& v = in[(size_t)i];
    v.kind = kind[i];
    v.contig = -1;
    for (uint32_t c = 0; c < n_contigs && contig[i]; c++)
      if (cn[c] == contig[i]) { v.contig = (int32_t)c; break; }
    v.pos = pos[i];
    v.popu = popu[i];
    v.text = text[i] ? text[i] : "";
    v.len = v.kind == 'd' ? atoll(v.text.c_str()) : 0;
  }
  simu::VariantTable T;
  T.build(in, cl, n_popus);
  if (rows) *rows = T.rows.size();
  if (dropped) *dropped = T.dropped;
  if (counts && n_counts != T.rows.size()) return UINT64_MAX;
  if (table && T.rows.size() <= table_cap) {
    const std::vector<sg_variant> a = T.abi();
    if (!a.empty()) memcpy(table, a.data(), a.size() * sizeof(sg_variant));
  }
  const std::string s = T.format(cn, pn, counts);
  if (out && s.size() <= cap) memcpy(out, s.data(), s.size());
  return s.size();
}
