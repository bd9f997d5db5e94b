// host/bam_reader.h -- a BGZF file read in batches of whole members, and the header of a BAM file: what seqToProfile
// --decode-bam (host/train.cpp), its BGZF VCF and truthEval (host/eval.cpp) share.
#pragma once
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../../include/simuscop_amd.h"
#include "common.h"
#include "reader_pool.h"

namespace simu {

// ---- --decode-bam: the BAM file itself, read in batches of whole BGZF members (SAMv1 section 4.1) ----
constexpr uint64_t kBamBatch = 16ull << 20;   // compressed bytes per batch (about 3 to 4 times as many inflated)
constexpr uint32_t kMaxMember = 65536;        // BSIZE is 16 bits

inline uint32_t le32(const uint8_t* p) { return p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// Pinned batches cut at a member boundary, read ahead while the device works on the batch before: a regular file by the pread
// pool, standard input by fread.  A member cut by the end of the file is an error.  Any BGZF file: the BAM of --decode-bam,
// a bgzip-compressed VCF (`kind` names it in the open error, `batch` is the compressed bytes of a batch).
struct BamReader {
  sg_ctx* ctx;
  std::string what;
  uint64_t batch = kBamBatch;
  FILE* fp = nullptr;
  int fd = -1;
  uint64_t pos = 0, size = 0, file_off = 0;   // file_off: where the next batch starts
  std::unique_ptr<ReaderPool> pool;
  char* buf[2] = {nullptr, nullptr};
  uint64_t len[2] = {0, 0};
  std::string pending;   // bytes behind the last whole member of a batch
  std::string last28;    // the last 28 bytes read (the EOF member, if the file has one)
  bool eof = false;
  BamReader(sg_ctx* c, const std::string& path, int threads, const char* kind = "BAM", uint64_t batch_bytes = kBamBatch)
      : ctx(c), what(path), batch(batch_bytes) {
    if (path == "-") fp = stdin;
    else if (!(fp = fopen(path.c_str(), "rb"))) throw Error(std::string("cannot open ") + kind + " file " + path, -1);
    struct stat sb;
    if (fp != stdin && fstat(fileno(fp), &sb) == 0 && S_ISREG(sb.st_mode)) {
      fd = fileno(fp);
      size = (uint64_t)sb.st_size;
      pool.reset(new ReaderPool(std::min(16, std::max(1, threads))));
    }
    for (int i = 0; i < 2; i++) {
      void* p = nullptr;
      if (sg_host_alloc(ctx, batch + kMaxMember, &p) != SG_OK) throw Error(std::string("GPU engine error in sg_host_alloc: ") + sg_last_error(ctx));
      buf[i] = (char*)p;
    }
  }
  ~BamReader() {
    for (char* b : buf) if (b) sg_host_free(ctx, b);
    if (fp && fp != stdin) fclose(fp);
  }
  void rewind() { pos = 0; file_off = 0; pending.clear(); last28.clear(); eof = false; }
  bool eof_marker() const {
    uint8_t e[28];
    sg_bgzf_eof(e);
    return last28.size() == 28 && memcmp(last28.data(), e, 28) == 0;
  }
  // fills buf[i] with whole members; false when nothing is left
  bool fill(int i) {
    if (eof && pending.empty()) { len[i] = 0; return false; }
    uint64_t have = pending.size();
    const uint64_t p0 = have;
    memcpy(buf[i], pending.data(), have);
    pending.clear();
    if (fd >= 0) {
      const uint64_t n = std::min<uint64_t>(batch + kMaxMember - have, size - pos);
      if (n) parallel_pread(*pool, fd, (uint8_t*)buf[i] + have, pos, n);
      have += n;
      pos += n;
      if (pos >= size) eof = true;
    } else {
      while (!eof && have < batch + kMaxMember) {
        const size_t got = fread(buf[i] + have, 1, batch + kMaxMember - have, fp);
        if (got == 0) { eof = true; break; }
        have += got;
      }
    }
    {
      const uint64_t fresh = have - p0, k = std::min<uint64_t>(fresh, 28);
      const std::string t = last28 + std::string(buf[i] + have - k, k);
      last28 = t.substr(t.size() > 28 ? t.size() - 28 : 0);
    }
    uint64_t n_members = 0, whole = 0;
    if (sg_bgzf_members(buf[i], have, nullptr, nullptr, nullptr, ~0ull, &n_members, &whole) != SG_OK)
      throw Error("Error: corrupt BGZF member at file offset " + std::to_string(file_off + whole) + " of " + what);
    pending.assign(buf[i] + whole, have - whole);
    if (eof && !pending.empty())
      throw Error("Error: truncated BGZF member at file offset " + std::to_string(file_off + whole) + " of " + what);
    len[i] = whole;
    file_off += whole;
    return whole > 0;
  }
};

// The header (magic, l_text, text, n_ref, the reference list) and, with `probe`, the first record for which it returns
// non-zero, searched over the whole stream (*found: what it returned; seqToProfile's read length).  Without `probe` the
// reading stops behind the header.  Inflated with the device inflater; the batches a pipe gave are kept for the caller's
// pass, a file is read again.
struct BamHeader {
  std::vector<std::string> names;
  uint64_t bytes = 0;   // where the first record starts in the decompressed stream
};
inline void bam_prepare(sg_ctx* ctx, BamReader& rd, BamHeader& H, std::vector<std::string>& replay, int (*probe)(const uint8_t*, uint32_t) = nullptr,
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
    if (rd.fd < 0) replay.emplace_back(rd.buf[0], rd.len[0]);
    uint64_t n = 0;
    int rc = sg_inflate_bgzf(ctx, rd.buf[0], rd.len[0], out.data(), out.size(), &n);
    if (rc == SG_ERR_OVERFLOW) { out.resize(n); rc = sg_inflate_bgzf(ctx, rd.buf[0], rd.len[0], out.data(), out.size(), &n); }
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
