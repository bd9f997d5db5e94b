// host/bam_reader.h -- the header of a BAM file, read through a BatchReader of whole BGZF members (host/input_stream.h): what
// seqToProfile --decode-bam (host/train.cpp) and truthEval (host/eval.cpp) share.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/simuscop_amd.h"
#include "common.h"
#include "input_stream.h"

namespace simu {

inline uint32_t le32(const uint8_t* p) { return p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// The header (magic, l_text, text, n_ref, the reference list) and, with `probe`, the first record for which it returns
// non-zero, searched over the whole stream (*found: what it returned; seqToProfile's read length).  Without `probe` the
// reading stops behind the header.  Inflated with the device inflater; the batches a pipe gave are kept for the caller's
// pass, a file is read again.
struct BamHeader {
  std::vector<std::string> names;
  uint64_t bytes = 0;   // where the first record starts in the decompressed stream
};
inline void bam_prepare(sg_ctx* ctx, BatchReader& rd,BamHeader& H, std::vector<std::string>& replay, int (*probe)(const uint8_t*, uint32_t) = nullptr,
                        int* found = nullptr) {
  int none = 0;
  int& read_length = found ? *found : none;
  std::string dec;        // inflated bytes not yet looked at
  uint64_t dec_off = 0;   // their offset in the stream
  bool have_header = false, more = true;
  std::vector<char> out(kBamBatch * 8);
  while (more && !(probe ? read_length != 0 : have_header)) {
    more = rd.fill(0);
    if (!more) break;
    if (!rd.regular()) replay.emplace_back(rd.data(0), rd.len[0]);
    uint64_t n = 0;
    int rc = sg_inflate_bgzf(ctx, rd.data(0), rd.len[0], out.data(), out.size(), &n);
    if (rc == SG_ERR_OVERFLOW) { out.resize(n); rc = sg_inflate_bgzf(ctx, rd.data(0), rd.len[0], out.data(), out.size(), &n); }
    if (rc != SG_OK) throw Error(std::string("GPU engine error in sg_inflate_bgzf: ") + sg_last_error(ctx) + " (" + rd.what + ")");
    dec.append(out.data(), n);
    size_t p = 0;
    if (!have_header) {
      const uint8_t* d = (const uint8_t*)dec.data();
      if (dec.size() < 12) continue;
      if (memcmp(d, "BAM\1", 4) != 0) throw Error("Error: " + rd.what + " is not a BAM file (bad magic)");
      const uint64_t l_text = le32(d + 4);
      if (l_text > (1ull << 31) || dec.size() < 12 + l_text) continue;
      const uint32_t n_ref = le32(d + 8 + l_text);
      uint64_t q = 12 + l_text;
      std::vector<std::string> names;
      bool whole = true;
      for (uint32_t i = 0; i < n_ref; i++) {
        if (q + 4 > dec.size()) { whole = false; break; }
        const uint32_t l_name = le32(d + q);
        if (l_name < 1 || l_name > (1u << 20)) throw Error("Error: malformed BAM header in " + rd.what);
        if (q + 4 + l_name + 4 > dec.size()) { whole = false; break; }
        names.emplace_back((const char*)d + q + 4, strnlen((const char*)d + q + 4, l_name));
        q += 4 + l_name + 4;
      }
      if (!whole) continue;
      H.names = names;
      H.bytes = q;
      have_header = true;
      p = q;
    }
    while (probe && !read_length && dec.size() - p >= 4) {
      const uint32_t bs = le32((const uint8_t*)dec.data() + p);
      if (bs < 32) throw Error("Error: malformed BAM record at decompressed offset " + std::to_string(dec_off + p) + " of " + rd.what);
      if (dec.size() - p < 4ull + bs) break;
      read_length = probe((const uint8_t*)dec.data() + p, bs);
      p += 4ull + bs;
    }
    dec.erase(0, p);
    dec_off += p;
  }
  if (!have_header) throw Error("Error: truncated BAM header in " + rd.what);
}

}  // namespace simu
