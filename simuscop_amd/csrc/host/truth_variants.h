// host/truth_variants.h -- the variant table of simuReads --truth-variants: built once from the rows of the variation and
// SNP files, given to the engine (sg_variants_begin), and written with the device's counts as <stem>.truth.variants.tsv.
// The counting rule is the engine's (DESIGN.md "True allele counts"); this file knows rows, keys, order and text.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/simuscop_amd.h"

namespace simu {

struct VariantIn {
  char kind;         // 's' variation-file SNV, 'p' SNP-file row, 'i' insertion, 'd' deletion
  int32_t contig;    // BAM refID, or -1: a contig the reference does not hold
  int64_t pos;       // 1-based, as the file wrote it
  int32_t popu;      // index in config order ('p': unused)
  std::string text;  // s / p: the allele; i: the inserted sequence; d: unused
  int64_t len;       // d: the length
};

struct VariantTable {
  struct Row {
    uint32_t contig, kind;   // kind as sg_variant: 0 SNV / SNP, 1 insertion, 2 deletion
    uint64_t p;              // 0-based
    uint32_t len;
    char allele;             // kind 0: upper case
    bool listed;             // kind 0: a variation-file row lists it (type s), otherwise p
    std::string seq;         // kind 1: the first sequence met
    std::vector<uint8_t> popus;   // [n_popus] 1: that population lists the row
  };
  std::vector<Row> rows;
  uint64_t dropped = 0;

  // Merges on (contig, p, allele) / (contig, p, length), orders by refID, p, type (s / p, i, d), allele byte or length;
  // rows on no contig, with p outside [0, LN) or with a length below 1 are counted in `dropped`.
  void build(const std::vector<VariantIn>& in, const std::vector<uint64_t>& contig_len, size_t n_popus);
  std::vector<sg_variant> abi() const;
  // the whole file; counts: [rows][2] (alt, total) or nullptr for zeros
  std::string format(const std::vector<std::string>& contig_name, const std::vector<std::string>& popu_name, const uint32_t* counts) const;
};

}  // namespace simu
