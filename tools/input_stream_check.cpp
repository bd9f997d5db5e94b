// tools/input_stream_check.cpp -- BatchReader and stream_batches (host/input_stream.h: how seqToProfile and truthEval get a
// file to the GPU) on the CPU, for the sanitizer builds of tools/input_stream_sanitized.sh.  The product's batches are 8 to
// 64 MB, so no quick test carries a partial line, a partial BGZF member or the 28 EOF bytes from one batch to the next;
// here the capacities are 64 bytes of lines and 256 bytes of members (of at most 64 bytes each), and every case is compared
// with a plain model that cuts the whole file image at boundaries.  The few engine calls the reader links against are
// defined here -- pinned memory over malloc, sg_bgzf_members over the engine's own walk (sg_bgzf.h) -- so no GPU is touched.
// BGZF members are made by hand as stored blocks: the walk reads the header, BSIZE and ISIZE only.
// usage: input_stream_check [workdir] [lines] [members] [loop]   (no group named: all three)
#define SG_BGZF_IMPLEMENTATION
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../simuscop_amd/csrc/host/input_stream.h"
#include "../simuscop_amd/csrc/sg_bgzf.h"

// ---- the engine calls of host/input_stream.h ----
static std::string g_error;
static long g_pinned = 0;   // buffers handed out and not yet given back
extern "C" {
int sg_host_alloc(sg_ctx*, uint64_t bytes, void** p) { *p = malloc(bytes ? bytes : 1); g_pinned++; return *p ? SG_OK : SG_ERR_HIP; }
int sg_host_free(sg_ctx*, void* p) { free(p); g_pinned--; return SG_OK; }
const char* sg_last_error(const sg_ctx*) { return g_error.c_str(); }
int sg_bgzf_eof(uint8_t out[28]) {
  static const uint8_t e[28] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  memcpy(out, e, 28);
  return SG_OK;
}
int sg_bgzf_members(const void* buf, uint64_t bytes, uint64_t* offsets, uint32_t* bsize, uint32_t* isize, uint64_t cap, uint64_t* n_members,
                    uint64_t* whole_bytes) {
  return bgzf_walk((const uint8_t*)buf, bytes, 0, cap, nullptr, n_members, whole_bytes, &g_error, offsets, bsize, isize);
}
}

namespace {

using simu::BatchReader;
constexpr uint64_t kLineCap = 64, kMemberCap = 256;   // (kMemberCap: 192 bytes of batch + 64 of the largest member)

std::string g_dir;
int g_checks = 0;
void fail(const std::string& what) { fprintf(stderr, "input_stream_check: %s\n", what.c_str()); exit(1); }
void expect(bool ok, const std::string& what) { g_checks++; if (!ok) fail(what); }

std::string write_file(const std::string& name, const std::string& image) {
  const std::string path = g_dir + "/" + name;
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(image.data(), 1, image.size(), f) != image.size()) fail("cannot write " + path);
  fclose(f);
  return path;
}

struct Batches {
  std::vector<std::string> got;
  std::string error;   // what ended the reading, if anything did
  bool operator==(const Batches& o) const { return got == o.got && error == o.error; }
};
std::string show(const Batches& b) {
  std::string s = "[";
  for (const std::string& g : b.got) s += std::to_string(g.size()) + " ";
  return s + "] " + b.error;
}
// every batch of a reader, through fill() on alternating buffers as stream_batches calls it
Batches drain(BatchReader& rd) {
  Batches out;
  try {
    for (int cur = 0; rd.fill(cur); cur ^= 1) out.got.emplace_back(rd.data(cur), rd.len[cur]);
  } catch (const std::exception& e) { out.error = e.what(); }
  return out;
}

// ---- the model: the longest prefix of (what is left of the image, up to `cap` bytes) that ends at a boundary ----
// Lines.  A regular file knows its end when the last byte is read; a pipe when a read comes back short, so a file whose
// last bytes fill a buffer exactly is cut once more there (as it always was: the two routes differ in this alone).
Batches model_lines(const std::string& img, uint64_t cap, bool whole_lines, bool pipe) {
  Batches out;
  uint64_t pos = 0;
  bool eof = false;
  while (!(eof && pos == img.size())) {
    const uint64_t end = std::min<uint64_t>(img.size(), pos + cap);
    eof = pipe ? end - pos < cap : end == img.size();
    uint64_t cut = end;
    if (whole_lines && !eof) {
      while (cut > pos && img[cut - 1] != '\n') cut--;
      if (cut == pos) { out.error = "a line of the SAM text is longer than 64 MB"; return out; }
    }
    if (cut == pos) break;
    out.got.push_back(img.substr(pos, cut - pos));
    pos = cut;
  }
  return out;
}
// Members of the sizes their headers claim, the one at index `damaged` with a header that is not BGZF.
Batches model_members(const std::string& img, const std::vector<uint64_t>& sizes, int damaged, uint64_t cap, const std::string& path) {
  Batches out;
  uint64_t pos = 0;
  size_t k = 0;
  for (;;) {
    const uint64_t end = std::min<uint64_t>(img.size(), pos + cap);
    uint64_t cut = pos;
    while (k < sizes.size() && end - cut >= 12) {
      if ((int)k == damaged) { out.error = "Error: corrupt BGZF member at file offset " + std::to_string(cut) + " of " + path; return out; }
      if (cut + sizes[k] > end) break;
      cut += sizes[k++];
    }
    if (end == img.size() && cut < end) { out.error = "Error: truncated BGZF member at file offset " + std::to_string(cut) + " of " + path; return out; }
    if (cut == pos) break;
    out.got.push_back(img.substr(pos, cut - pos));
    pos = cut;
  }
  return out;
}

std::string member(uint32_t payload, char fill) {   // 31 + payload bytes: header, one stored block, CRC-32 (not looked at), ISIZE
  const uint32_t bsize = 31 + payload - 1;
  std::string m = {31, (char)139, 8, 4, 0, 0, 0, 0, 0, (char)255, 6, 0, 'B', 'C', 2, 0, (char)(bsize & 255), (char)(bsize >> 8)};
  m += {1, (char)payload, 0, (char)~payload, (char)255};
  m += std::string(payload, fill);
  m += std::string(4, 'c');
  m += {(char)payload, 0, 0, 0};
  return m;
}
std::string eof_member() { uint8_t e[28]; sg_bgzf_eof(e); return std::string((const char*)e, 28); }

// ---- lines, and cuts anywhere ----
void lines_case(const char* name, const std::string& img, bool routes_differ = false) {
  const std::string path = write_file(name, img);
  for (int anywhere = 0; anywhere < 2; anywhere++) {
    const BatchReader::Cut cut = anywhere ? BatchReader::Anywhere : BatchReader::Lines;
    BatchReader file(nullptr, path, "SAM", 2, cut, kLineCap);
    expect(file.regular(), std::string(name) + ": a regular file");
    const Batches got = drain(file), want = model_lines(img, kLineCap, !anywhere, false);
    expect(got == want, std::string(name) + (anywhere ? " (anywhere)" : " (lines)") + ": file " + show(got) + " model " + show(want));
    FILE* p = popen(("cat '" + path + "'").c_str(), "r");
    if (!p) fail("popen");
    BatchReader pipe(nullptr, p, pclose, path, 2, cut, kLineCap);
    expect(!pipe.regular(), std::string(name) + ": a pipe");
    const Batches piped = drain(pipe), want_piped = model_lines(img, kLineCap, !anywhere, true);
    expect(piped == want_piped, std::string(name) + (anywhere ? " (anywhere)" : " (lines)") + ": pipe " + show(piped) + " model " + show(want_piped));
    expect((piped == got) == (anywhere || !routes_differ), std::string(name) + ": the pipe gives the batches of the file");
    if (got.error.empty()) {
      std::string all;
      for (size_t i = 0; i < got.got.size(); i++) {
        all += got.got[i];
        if (anywhere) expect(got.got[i].size() == kLineCap || i + 1 == got.got.size(), std::string(name) + ": a cut anywhere is at the capacity");
        else expect(got.got[i].back() == '\n' || i + 1 == got.got.size(), std::string(name) + ": every batch but the last ends in a line break");
      }
      expect(all == img, std::string(name) + ": the batches concatenate to the file");
    }
  }
}
std::string text_lines(std::initializer_list<int> lengths, bool last_break = true) {   // lines of these lengths, line break included
  std::string t;
  char c = 'a';
  for (int n : lengths) { t += std::string((size_t)n - 1, c); t += '\n'; c = c == 'z' ? 'a' : c + 1; }
  if (!last_break) t.pop_back();
  return t;
}
void check_lines() {
  lines_case("empty.sam", "");
  lines_case("one_open.sam", "one line without a final line break");
  lines_case("exact.sam", text_lines({64}));
  lines_case("exact_then_more.sam", text_lines({64, 10, 64, 3}));
  lines_case("too_long.sam", text_lines({65}));                          // capacity + 1: the error text
  lines_case("too_long_later.sam", text_lines({20, 30, 65, 5}));
  lines_case("multiple.sam", text_lines({30, 34, 16, 48, 60, 4}));       // 192 bytes: three buffers, each ends on a line break
  lines_case("cut_on_break.sam", text_lines({40, 24, 50, 7}));           // the first buffer's last byte is a line break
  lines_case("carried.sam", text_lines({50, 50, 50, 50, 13, 1, 1, 60}));
  lines_case("open_end.sam", text_lines({50, 50, 41}, false));
  // the routes' one difference: the last buffer is full and the text ends without a line break
  lines_case("open_end_full.sam", text_lines({50, 50, 30, 35}, false), true);   // the pipe cuts once more, at the last line break
  lines_case("open_end_full_line.sam", text_lines({50, 50, 65}, false), true);  // ... and finds none: the error, where the file gives the line
  {
    const std::string path = write_file("too_long.sam", text_lines({65}));
    BatchReader rd(nullptr, path, "SAM", 2, BatchReader::Lines, kLineCap);
    expect(drain(rd).error == "a line of the SAM text is longer than 64 MB", "the text of a line longer than a batch");
  }
  try {
    BatchReader rd(nullptr, g_dir + "/no_such_file", "VCF", 2, BatchReader::Lines, kLineCap);
    fail("a file that does not exist was opened");
  } catch (const simu::Error& e) {
    expect(std::string(e.what()) == "cannot open VCF file " + g_dir + "/no_such_file" && e.exit_code == -1, "the open error");
  }
}

// ---- whole BGZF members ----
struct MemberFile {
  std::string img;
  std::vector<uint64_t> sizes;
  void add(const std::string& m) { img += m; sizes.push_back(m.size()); }
};
Batches members_case(const std::string& name, const MemberFile& f, int damaged = -1, uint64_t cap = kMemberCap) {
  const std::string path = write_file(name, f.img);
  BatchReader rd(nullptr, path, "BAM", 2, BatchReader::Members, cap);
  const Batches got = drain(rd), want = model_members(f.img, f.sizes, damaged, cap, path);
  expect(got == want, name + ": file " + show(got) + " model " + show(want));
  uint64_t sum = 0;
  for (const std::string& g : got.got) sum += g.size();
  expect(rd.file_off == sum, name + ": file_off is where the next batch starts");
  if (got.error.empty()) {
    rd.rewind();
    expect(rd.file_off == 0 && drain(rd) == want, name + ": the same batches again after rewind()");
  }
  return got;
}
void check_members() {
  MemberFile none;
  expect(members_case("none.bam", none).got.empty(), "zero members: no batch");
  MemberFile only_eof;
  only_eof.add(eof_member());
  expect(members_case("only_eof.bam", only_eof).got.size() == 1, "only the EOF member: one batch");
  MemberFile straddle;   // 5 x 60 bytes: the fifth straddles 256
  for (int i = 0; i < 5; i++) straddle.add(member(29, (char)('A' + i)));
  straddle.add(eof_member());
  const Batches s = members_case("straddle.bam", straddle);
  expect(s.got.size() == 2 && s.got[0].size() == 240 && s.got[1].size() == 88, "a member that straddles the capacity is carried whole");
  MemberFile exact;      // 4 x 64 bytes fill a batch exactly, twice
  for (int i = 0; i < 8; i++) exact.add(member(33, (char)('a' + i)));
  exact.add(eof_member());
  const Batches e = members_case("exact.bam", exact);
  expect(e.got.size() == 3 && e.got[0].size() == 256 && e.got[1].size() == 256 && e.got[2].size() == 28, "members that fill a batch exactly");
  MemberFile mixed;
  for (int i = 0; i < 23; i++) mixed.add(member((uint32_t)(i * 7 % 34), (char)('0' + i % 10)));
  mixed.add(eof_member());
  members_case("mixed.bam", mixed);
  // a last member cut at every byte of its length: the "truncated" text with the member's file offset
  for (uint64_t keep = 1; keep < 60; keep++) {
    MemberFile cut = straddle;
    cut.img.resize(240 + keep);
    cut.sizes.resize(5);
    const Batches t = members_case("truncated.bam", cut);
    // (up to byte 256 the first fill sees the end of the file and refuses: the four whole members are not handed over)
    expect(t.error == "Error: truncated BGZF member at file offset 240 of " + g_dir + "/truncated.bam" && t.got.size() == (keep <= 16 ? 0u : 1u),
           "truncated after " + std::to_string(keep) + " bytes: " + show(t));
  }
  // a damaged header in member k, wherever k lies in its batch
  for (int k = 0; k < (int)mixed.sizes.size(); k++) {
    MemberFile bad = mixed;
    uint64_t at = 0;
    for (int i = 0; i < k; i++) at += bad.sizes[i];
    bad.img[at + 1] = 0;   // (not the gzip magic)
    const Batches c = members_case("corrupt.bam", bad, k);
    expect(c.error == "Error: corrupt BGZF member at file offset " + std::to_string(at) + " of " + g_dir + "/corrupt.bam", "damaged member " + std::to_string(k) + ": " + show(c));
  }
  // the EOF marker: looked up at the end of a regular file, and met while streaming with its 28 bytes split over two fills
  for (int with_marker = 0; with_marker < 2; with_marker++) {
    MemberFile f;
    for (int i = 0; i < 3; i++) f.add(member(9, 'x'));   // 120 bytes
    f.add(eof_member());
    if (!with_marker) f.img[f.img.size() - 6] ^= 1;      // (a CRC byte: still a member, no longer the marker)
    const std::string path = write_file("marker.bam", f.img);
    for (uint64_t split = 0; split <= 28; split++) {
      BatchReader rd(nullptr, path, "BAM", 2, BatchReader::Members, 120 + split);
      expect(rd.peek_eof_marker() == (with_marker == 1), "peek_eof_marker()");
      expect(!rd.eof_marker(), "eof_marker() in front of the first fill");
      const Batches got = drain(rd);
      expect(got.error.empty() && got.got.size() == (split == 28 ? 1u : 2u), "the marker split at " + std::to_string(split) + ": " + show(got));
      expect(rd.eof_marker() == (with_marker == 1), "eof_marker() with the 28 bytes split at " + std::to_string(split));
    }
  }
  {
    const std::string path = write_file("short.bam", "short");
    BatchReader rd(nullptr, path, "BAM", 2, BatchReader::Members, kMemberCap);
    expect(!rd.peek_eof_marker(), "peek_eof_marker() of a file shorter than 28 bytes");
  }
}

// ---- the read-ahead loop ----
void check_loop() {
  MemberFile f;
  for (int i = 0; i < 23; i++) f.add(member((uint32_t)(i * 5 % 34), (char)('a' + i)));
  f.add(eof_member());
  const std::string path = write_file("loop.bam", f.img);
  const Batches want = model_members(f.img, f.sizes, -1, kMemberCap, path);
  expect(want.got.size() >= 4, "the loop's file has at least four batches");
  {
    BatchReader rd(nullptr, path, "BAM", 2, BatchReader::Members, kMemberCap);
    Batches got;
    simu::stream_batches(rd, [&](const char* p, uint64_t n) { got.got.emplace_back(p, n); });
    expect(got == want, "stream_batches feeds the batches in file order");
    expect(rd.eof_marker(), "eof_marker() after the loop");
  }
  {  // the first batch may be looked at before the loop feeds it
    BatchReader rd(nullptr, path, "BAM", 2, BatchReader::Members, kMemberCap);
    expect(rd.first() && std::string(rd.data(0), rd.len[0]) == want.got[0] && rd.first(), "first()");
    Batches got;
    simu::stream_batches(rd, [&](const char* p, uint64_t n) { got.got.emplace_back(p, n); });
    expect(got == want, "stream_batches starts from the batch first() filled");
  }
  for (size_t k = 0; k < want.got.size(); k++) {   // feed throws in batch k: its error arrives, the reader thread joined
    size_t fed = 0;
    std::string said;
    {
      BatchReader rd(nullptr, path, "BAM", 2, BatchReader::Members, kMemberCap);
      try {
        simu::stream_batches(rd, [&](const char*, uint64_t) { if (fed++ == k) throw simu::Error("feed refused batch " + std::to_string(k), 7); });
      } catch (const simu::Error& e) { said = e.what(); expect(e.exit_code == 7, "feed's own exit code"); }
    }   // (the reader is gone here: a thread still filling it would be the sanitizers' to find)
    expect(said == "feed refused batch " + std::to_string(k) && fed == k + 1, "an error of feed in batch " + std::to_string(k));
  }
  for (size_t k = 0; k < want.got.size(); k++) {   // go_on says no after batch k: nothing more is fed
    size_t fed = 0;
    BatchReader rd(nullptr, path, "BAM", 2, BatchReader::Members, kMemberCap);
    simu::stream_batches(rd, [&](const char*, uint64_t) { fed++; }, [&]() { return fed <= k; });
    expect(fed == k + 1, "go_on false after batch " + std::to_string(k));
  }
  {  // the reader fails on the second batch: on the first member that no byte of the first buffer shows
    MemberFile bad = f;
    uint64_t at = 0;
    for (size_t i = 0; at < kMemberCap; i++) at += bad.sizes[i];
    bad.img[at] = 0;
    const std::string bad_path = write_file("loop_bad.bam", bad.img);
    size_t fed = 0;
    std::string said;
    {
      BatchReader rd(nullptr, bad_path, "BAM", 2, BatchReader::Members, kMemberCap);
      try { simu::stream_batches(rd, [&](const char*, uint64_t) { fed++; }); } catch (const simu::Error& e) { said = e.what(); }
    }
    expect(fed == 1 && said == "Error: corrupt BGZF member at file offset " + std::to_string(at) + " of " + bad_path, "a reader error after a clean feed: " + said);
    {
      BatchReader rd(nullptr, bad_path, "BAM", 2, BatchReader::Members, kMemberCap);
      try { simu::stream_batches(rd, [&](const char*, uint64_t) { throw simu::Error("feed first"); }); } catch (const simu::Error& e) { said = e.what(); }
    }
    expect(said == "feed first", "feed's error wins over the reader's");
  }
}

}  // namespace

int main(int argc, char** argv) {
  g_dir = argc > 1 ? argv[1] : "/tmp";
  bool lines = argc <= 2, members = argc <= 2, loop = argc <= 2;
  for (int i = 2; i < argc; i++) {
    lines |= !strcmp(argv[i], "lines");
    members |= !strcmp(argv[i], "members");
    loop |= !strcmp(argv[i], "loop");
  }
  if (lines) check_lines();
  if (members) check_members();
  if (loop) check_loop();
  if (g_pinned) fail(std::to_string(g_pinned) + " pinned buffers were not given back");
  printf("input_stream_check: %d checks, all as the model has them\n", g_checks);
  return 0;
}
