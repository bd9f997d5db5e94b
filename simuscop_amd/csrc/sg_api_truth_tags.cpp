// sg_api_truth_tags.cpp -- sg_truth_tags: the rule of the truth BAM's NM, MD and XE tags for one record, on the host and
// without a context (the rule itself: truth_tags_walk and truth_xe, sg_truth.h; the kernels that state it for a pass:
// sg_truth_tags.hip, sg_truth.hip).  A file of its own so that tools/tags_sanitized.sh can build it under the sanitizers.
#include "simuscop_amd.h"
#include "sg_truth.h"

extern "C" {

int sg_truth_tags(const uint32_t* cigar, uint32_t n_ops, const char* seq, uint32_t seq_len, const uint8_t* ref_codes, uint64_t n_ref,
                  uint32_t md_cap, const uint8_t* tmpl_codes, uint32_t tmpl_len, int reverse, const uint32_t* events, uint32_t n_events,
                  const char* read, uint32_t read_len, uint32_t* present, uint32_t* nm, char* md, uint32_t* md_len, uint32_t* xe) {
  if (!present || !nm || !md_len || !xe || (n_ops && (!cigar || !seq)) || (md_cap && !md) || (n_events && !events) || n_events > SG_MAX_EVENTS)
    return SG_ERR_INVALID;
  *present = *nm = *md_len = *xe = 0;
  if (n_ops) {   // a mapped record: NM, and MD unless its text is longer than md_cap
    uint64_t q = 0, r = 0;
    for (uint32_t k = 0; k < n_ops; k++) {
      const uint32_t len = cigar[k] >> 4, op = cigar[k] & 15u;
      if (op > sg::kOpS) return SG_ERR_INVALID;
      if (op == sg::kOpM || op == sg::kOpI || op == sg::kOpS) q += len;
      if (op == sg::kOpM || op == sg::kOpD || op == sg::kOpN) r += len;
    }
    if (q != seq_len || r > n_ref || (n_ref && !ref_codes)) return SG_ERR_INVALID;
    const sg::TagWalk W = sg::truth_tags_walk(cigar, n_ops, [&](uint32_t i) { return (uint32_t)(uint8_t)seq[i]; },
                                              [&](uint64_t x) { return (uint32_t)ref_codes[x]; }, [&](uint32_t o, uint32_t ch) { if (o < md_cap) md[o] = (char)ch; });
    *nm = W.nm;
    *present |= SG_TAG_NM;
    if (W.md_len <= md_cap) { *md_len = W.md_len; *present |= SG_TAG_MD; }
  }
  if (tmpl_codes) {   // a read whose template lies in its chain: XE
    if (!read || !tmpl_len) return SG_ERR_INVALID;
    const uint32_t v = sg::truth_xe(events, n_events, tmpl_len, read_len,
                                    [&](uint32_t j) { return sg::errtab_tmpl_code(tmpl_codes[reverse ? tmpl_len - 1u - j : j], reverse != 0); },
                                    [&](uint32_t i) { return (uint32_t)(uint8_t)read[i]; });
    if (v == sg::kErrWalkBad) return SG_ERR_INVALID;
    *xe = v;
    *present |= SG_TAG_XE;
  }
  return SG_OK;
}

}  // extern "C"
