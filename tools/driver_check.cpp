// tools/driver_check.cpp -- the parts of the simuReads driver that need no GPU, for the sanitizer builds of
// tools/driver_sanitized.sh: the chunk pump of the FASTQ sink (pump_chunks, host/fastq_sink.h) and the two cuts of a batch
// (shard_cut and piece_end, host/batch_cut.h).  The product's chunks are 64 MB, so no quick test reaches a chunk boundary,
// and the pump is the only part of the program with two levels of threads; here a chunk is 64 bytes, the four buffers are
// mallocs of exactly that, the fetch is a memcpy from a source string that can fail at its k-th call, and every file is
// compared with its source.  The cuts are compared with a brute-force restatement over hand-made and seeded random vectors.
// usage: driver_check [workdir]
#include <csignal>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../simuscop_amd/csrc/host/batch_cut.h"
#include "../simuscop_amd/csrc/host/fastq_sink.h"

namespace {

constexpr size_t kChunk = 64;
std::string g_dir;
int g_checks = 0;
void fail(const std::string& what) { fprintf(stderr, "driver_check: %s\n", what.c_str()); exit(1); }
void expect(bool ok, const std::string& what) { g_checks++; if (!ok) fail(what); }

std::string slurp(const std::string& path) {
  std::string s;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) fail("cannot read back " + path);
  char buf[4096];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) s.append(buf, n);
  fclose(f);
  return s;
}
std::string source(int m, uint64_t n) {
  std::string s((size_t)n, '\0');
  for (uint64_t i = 0; i < n; i++) s[(size_t)i] = (char)('!' + (i * 131 + i / kChunk * 7 + (uint64_t)m * 29) % 90);
  return s;
}

// ---- the chunk pump ----
struct Pumped { simu::PumpResult r; std::string file[2]; int calls = 0, ok_calls[2] = {0, 0}; };
// one run: `fail_at` >= 1 makes that fetch call (1-based) return status 7; `full`: the files refuse every write
Pumped pump(uint64_t n1, uint64_t n2, int mates, int fail_at = 0, bool full = false) {
  const std::string src[2] = {source(0, n1), source(1, n2)};
  const uint64_t total[2] = {n1, n2};
  const std::string path[2] = {g_dir + "/driver_check_1.fq", g_dir + "/driver_check_2.fq"};
  FILE* f[2] = {nullptr, nullptr};
  for (int m = 0; m < mates; m++) {
    f[m] = fopen(full ? "/dev/full" : path[m].c_str(), "wb");
    if (!f[m]) fail("cannot open an output file");
    if (full) setvbuf(f[m], nullptr, _IONBF, 0);
  }
  void* buf[4];
  for (void*& b : buf) b = malloc(kChunk);
  Pumped p;
  int last[2] = {-1, -1};
  p.r = simu::pump_chunks(
      [&](int m, uint64_t off, size_t n, void* dst) {
        p.calls++;
        expect(m >= 0 && m < mates && off % kChunk == 0 && n >= 1 && n <= kChunk && off + n <= total[m], "a fetch inside its mate's text");
        const int which = dst == buf[2 * m] ? 0 : dst == buf[2 * m + 1] ? 1 : -1;
        expect(which >= 0 && which != last[m], "the mate's two buffers take turns");
        last[m] = which;
        if (p.calls == fail_at) return 7;
        memcpy(dst, src[m].data() + off, n);
        p.ok_calls[m]++;
        return 0;
      },
      total, mates, f[0], f[1], buf, kChunk);
  for (void* b : buf) free(b);
  for (int m = 0; m < mates; m++) {
    fclose(f[m]);
    if (!full) p.file[m] = slurp(path[m]);
  }
  if (!fail_at && !full)
    for (int m = 0; m < mates; m++) expect(p.file[m] == src[m], "file " + std::to_string(m + 1) + " of (" + std::to_string(n1) + ", " + std::to_string(n2) + ") equals its source");
  if (fail_at)
    for (int m = 0; m < mates; m++) {
      const uint64_t want = std::min<uint64_t>(total[m], (uint64_t)p.ok_calls[m] * kChunk);
      expect(p.file[m] == src[m].substr(0, (size_t)want), "after a failed fetch file " + std::to_string(m + 1) + " holds its whole chunks and no more");
    }
  return p;
}

void check_pump() {
  const uint64_t pairs[][2] = {{0, 0}, {1, 0}, {64, 64}, {65, 64}, {64, 129}, {1000, 37}, {4096 + 1, 4096 - 1}};
  for (const auto& c : pairs) {
    const Pumped p = pump(c[0], c[1], 2);
    expect(p.r.status == 0 && !p.r.short_write, "a clean paired run");
    expect((uint64_t)p.calls == (c[0] + kChunk - 1) / kChunk + (c[1] + kChunk - 1) / kChunk, "one fetch per chunk");
    expect(p.r.t_fetch >= 0 && p.r.t_write >= 0, "times");
  }
  for (uint64_t n : {0, 63, 64, 65, 1000}) {
    const Pumped p = pump(n, 12345, 1);   // (a single-end run never looks at the second total)
    expect(p.r.status == 0 && !p.r.short_write && (uint64_t)p.calls == (n + kChunk - 1) / kChunk, "a clean single-end run");
  }
  // a fetch that fails at its k-th call, every k: that status comes back, no fetch follows it, nothing is posted after it
  for (const auto& c : {pairs[5], pairs[4]}) {
    const int calls = (int)((c[0] + kChunk - 1) / kChunk + (c[1] + kChunk - 1) / kChunk);
    for (int k = 1; k <= calls; k++) {
      const Pumped p = pump(c[0], c[1], 2, k);
      expect(p.r.status == 7 && p.calls == k && p.ok_calls[0] + p.ok_calls[1] == k - 1, "the pump ends at the failed fetch " + std::to_string(k));
    }
  }
  // files that refuse every write: the flag comes back and the pump still ends
  {
    const Pumped p = pump(300, 200, 2, 0, true);
    expect(p.r.status == 0 && p.r.short_write && p.calls == 9, "short writes to both files are reported");
    const Pumped q = pump(65, 0, 1, 0, true);
    expect(q.r.status == 0 && q.r.short_write, "a short write to the only file is reported");
  }
}

// ---- the two cuts ----
using Slots = std::vector<uint64_t>;
uint64_t sum(const Slots& s, size_t a, size_t b) { uint64_t t = 0; for (size_t i = a; i < b; i++) t += s[i]; return t; }

void check_cuts_of(const Slots& s) {
  const uint64_t total = sum(s, 0, s.size());
  uint64_t smallest = s.empty() ? 0 : s[0];
  for (uint64_t v : s) smallest = std::min(smallest, v);
  for (int world : {1, 2, 3, 8, (int)s.size() + 3}) {
    // brute force: every segment's owner from the fragments planned in front of it
    std::vector<int> owner(s.size(), 0);
    const uint64_t per = (total + (uint64_t)world - 1) / (uint64_t)world;
    for (size_t i = 0; i < s.size(); i++) {
      const uint64_t before = sum(s, 0, i);
      owner[i] = world == 1 || per == 0 ? 0 : (int)(before / per < (uint64_t)world - 1 ? before / per : (uint64_t)world - 1);
    }
    size_t covered = 0;
    for (int rank = 0; rank < world; rank++) {
      size_t a0 = 99, a1 = 99;
      const bool any = simu::shard_cut(s, world, rank, a0, a1);
      size_t n_own = 0;
      for (size_t i = 0; i < s.size(); i++) n_own += owner[i] == rank;
      if (world == 1) expect(any && a0 == 0 && a1 == s.size(), "one rank has every segment");
      expect(any == (n_own > 0), "a rank without segments reports nothing");
      if (!any) continue;
      expect(a0 == covered && a1 == a0 + n_own && a1 <= s.size(), "the ranks' runs are contiguous, disjoint and in rank order");
      for (size_t i = a0; i < a1; i++) expect(owner[i] == rank, "a run holds its rank's segments");
      covered = a1;
      // the pieces of this rank's run
      for (uint64_t piece_slots : {(uint64_t)1, smallest, total, total + 1}) {
        for (size_t c0 = a0; c0 < a1;) {
          const size_t c1 = simu::piece_end(s, c0, a1, piece_slots);
          size_t want = c0 + 1;   // brute force: the longest run of whole segments that fits, at least one
          for (size_t e = c0 + 2; e <= a1; e++)
            if (sum(s, c0, e) <= piece_slots) want = e;
          expect(c1 == want, "a piece ends where the brute-force cut ends");
          expect(c1 > c0 && c1 <= a1 && (c1 == c0 + 1 || sum(s, c0, c1) <= piece_slots), "a piece holds a segment, and no more than fits unless it is one segment");
          c0 = c1;   // (so the pieces concatenate to the run: the walk ends at a1 exactly, checked by c1 <= a1)
        }
      }
    }
    expect(covered == s.size(), "together the runs hold every segment once");
  }
}

void check_cuts() {
  check_cuts_of(Slots(10, 5));
  check_cuts_of(Slots(1, 7));
  check_cuts_of(Slots{1, 1, 1000000, 1, 1});
  check_cuts_of(Slots{0, 0, 3, 4, 0, 5, 0, 0});
  check_cuts_of(Slots{0, 0, 0});
  uint64_t x = 0x9E3779B97F4A7C15ull;   // xorshift64, seeded
  auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  for (int v = 0; v < 200; v++) {
    Slots s(1 + next() % 40);
    const int kind = (int)(next() % 3);
    for (uint64_t& e : s) e = next() % 4 == 0 ? 0 : kind == 0 ? next() % 10 : kind == 1 ? next() % 1000000 : 1 + next() % 3;
    check_cuts_of(s);
  }
}

}  // namespace

int main(int argc, char** argv) {
  g_dir = argc > 1 ? argv[1] : "/tmp";
  signal(SIGPIPE, SIG_IGN);
  check_pump();
  check_cuts();
  printf("driver_check: %d checks, all as the model has them\n", g_checks);
  return 0;
}
