// host/truth_errors.h -- the text of a --truth-errors file (<stem>.truth.errors.tsv), host only.
#pragma once
#include <stdint.h>

#ifdef __cplusplus
#include <string>

namespace simu {
// The file made of a table in sg_errtab_counts' layout (include/simuscop_amd.h): four blocks, each behind its own header
// line, tab separated, mates 1 .. `mates`:
//   #Q  mate  cycle  qual  bases  errors  other  inserted    cycle 1-based, qual = qual_lo + column; rows whose four
//                                                            counts are all 0 are left out; by mate, cycle, quality
//   #S  mate  from  to  count                                from A C G T, to A C G T N: all 20 rows of every mate
//   #I  mate  index  events  bases                           index = j + 1; rows with events only
//   #D  mate  index  events  bases
// *rows = data lines.
std::string errors_format(const uint64_t* table, uint32_t cycles, uint32_t qual_lo, uint32_t n_qual, uint32_t tmpl_len, uint32_t mates,
                          uint64_t* rows);
}  // namespace simu

extern "C" {
#endif

// errors_format for callers outside: `cells` must be 8 * cycles * n_qual + 40 + 8 * tmpl_len and mates 1 or 2 (UINT64_MAX
// otherwise).  The text is written to out[0 .. cap) when it fits; returns its length (call again with that much room).
uint64_t simu_errors_format(const uint64_t* table, uint64_t cells, uint32_t cycles, uint32_t qual_lo, uint32_t n_qual, uint32_t tmpl_len,
                            uint32_t mates, char* out, uint64_t cap, uint64_t* rows);

#ifdef __cplusplus
}
#endif
