// sg_bgzf.h -- the member headers of a BGZF buffer (SAMv1 section 4.1) and the row the walk fills per member.  Host only and
// without HIP: the engine (sg_api_bgzf.cpp, sg_api_vcf.cpp) and the CPU check of the input readers (tools/input_stream_check.cpp)
// run the same walk.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/simuscop_amd.h"

namespace sg {

constexpr uint32_t kBgzfMaxIsize = 65536;    // BGZF: at most 64 KiB of input per member (SAMv1 section 4.1)
constexpr uint32_t kBgzfMinMember = 28;      // 18-byte header with the BC subfield, an empty final block, CRC32, ISIZE

// one whole member of a batch: `src` .. `src + bytes` in the compressed batch, `isize` inflated bytes at `dst`
struct InflateMember {
  uint64_t src, dst;
  uint32_t bytes, isize;
  uint64_t file_off;   // where the member starts in the file (error messages)
};

}  // namespace sg

// The member headers of a buffer: up to `cap` whole members; *whole = bytes they make up.  A member cut by the end of the
// buffer ends the walk; a header that is not BGZF is an error (message in *err).  The one file that defines
// SG_BGZF_IMPLEMENTATION in front of its includes holds the definition: sg_api_bgzf.cpp in the engine.
int bgzf_walk(const uint8_t* b, uint64_t bytes, uint64_t file_off, uint64_t cap, std::vector<sg::InflateMember>* out, uint64_t* n_out,
              uint64_t* whole, std::string* err, uint64_t* offs = nullptr, uint32_t* bsizes = nullptr, uint32_t* isizes = nullptr);

#ifdef SG_BGZF_IMPLEMENTATION
int bgzf_walk(const uint8_t* b, uint64_t bytes, uint64_t file_off, uint64_t cap, std::vector<sg::InflateMember>* out, uint64_t* n_out,
              uint64_t* whole, std::string* err, uint64_t* offs, uint32_t* bsizes, uint32_t* isizes) {
  uint64_t p = 0, n = 0, dst = 0;
  auto bad = [&](const char* what) {
    *err = "BGZF member at file offset " + std::to_string(file_off + p) + ": " + what;
    *n_out = n;
    *whole = p;
    return SG_ERR_INVALID;
  };
  while (p < bytes && n < cap) {
    if (bytes - p < 12) break;
    if (b[p] != 31 || b[p + 1] != 139 || b[p + 2] != 8 || !(b[p + 3] & 4)) return bad("not a gzip member with an extra field");
    // BGZF fixes FLG = 4 (SAMv1 section 4.1); FNAME, FCOMMENT or FHCRC would also move the DEFLATE data from 12 + XLEN
    if (b[p + 3] != 4) return bad("gzip flags other than FEXTRA");
    const uint32_t xlen = b[p + 10] | ((uint32_t)b[p + 11] << 8);
    if (p + 12 + xlen > bytes) break;
    int64_t bsize = -1;
    for (uint64_t q = p + 12; q + 4 <= p + 12 + xlen;) {
      const uint32_t slen = b[q + 2] | ((uint32_t)b[q + 3] << 8);
      if (b[q] == 'B' && b[q + 1] == 'C' && slen == 2 && q + 6 <= p + 12 + xlen) { bsize = b[q + 4] | ((uint32_t)b[q + 5] << 8); break; }
      q += 4 + slen;
    }
    if (bsize < 0) return bad("no BC subfield");
    const uint64_t size = (uint64_t)bsize + 1;
    if (size < 12 + xlen + 8 || size < sg::kBgzfMinMember - 2) return bad("BSIZE smaller than its own header and trailer");
    if (p + size > bytes) break;
    const uint32_t isize = b[p + size - 4] | ((uint32_t)b[p + size - 3] << 8) | ((uint32_t)b[p + size - 2] << 16) | ((uint32_t)b[p + size - 1] << 24);
    if (isize > sg::kBgzfMaxIsize) return bad("ISIZE above 64 KiB");
    if (out) out->push_back(sg::InflateMember{p, dst, (uint32_t)size, isize, file_off + p});
    if (offs) offs[n] = p;
    if (bsizes) bsizes[n] = (uint32_t)bsize;
    if (isizes) isizes[n] = isize;
    dst += isize;
    n++;
    p += size;
  }
  *n_out = n;
  *whole = p;
  return SG_OK;
}
#endif
