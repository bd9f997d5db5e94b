// host/eval.cpp -- see eval.h.  The host keeps what happens once per file -- options, the header, the @SQ names and the
// map between the two files' refIDs, the text of eval.tsv -- and streams both files through the GPU in batches of whole BGZF
// members while a reader thread fills the next batch (BatchReader and stream_batches, host/input_stream.h).
#include "eval.h"

#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../../include/simuscop_amd.h"
#include "bam_reader.h"
#include "common.h"
#include "engine.h"
#include "input_stream.h"

namespace simu {
namespace {

using Clock = std::chrono::steady_clock;
double since(Clock::time_point t) { return std::chrono::duration<double>(Clock::now() - t).count(); }

constexpr uint32_t kCategories = 8, kClasses = 3, kMapqs = 256;
const char* const kClassName[kClasses] = {"plain", "edited", "unmapped"};

// Refused before a device is touched: a file that cannot be opened, or whose first bytes are no BGZF member.
void need_bgzf(const std::string& path) {
  FILE* fp = fopen(path.c_str(), "rb");
  if (!fp) throw Error("cannot open BAM file " + path, -1);
  std::vector<uint8_t> head(kMaxMember);
  const size_t got = fread(head.data(), 1, head.size(), fp);
  fclose(fp);
  uint64_t n = 0, whole = 0;
  const bool magic = got >= 18 && head[0] == 31 && head[1] == 139 && head[2] == 8 && head[3] == 4;
  if (!magic || sg_bgzf_members(head.data(), got, nullptr, nullptr, nullptr, 1, &n, &whole) != SG_OK)
    throw Error("Error: " + path + " is not a BGZF file: a BAM file as samtools or simuReads --truth-bam writes it is expected", 1);
}

// One file through `feed` (sg_eval_truth_bgzf / sg_eval_test_bgzf), `start` called with its header in front of the first batch.
template <class Start, class Feed>
uint64_t stream_file(const Engine& eng, const std::string& path, int threads, Start start, Feed feed) {
  BatchReader rd(eng.ctx, path, "BAM", threads, BatchReader::Members);
  if (!rd.regular()) throw Error("Error: " + path + " is not a regular file (the header is read first, then the file from its start)", 1);
  if (!rd.peek_eof_marker()) std::cerr << "[W::bam_hdr_read] EOF marker is absent. The input is probably truncated" << std::endl;
  BamHeader H;
  std::vector<std::string> replay;
  bam_prepare(eng.ctx, rd, H, replay);
  rd.rewind();
  start(H);
  auto said = [&](int rc) {
    if (rc != SG_OK) throw Error(std::string("Error: ") + sg_last_error(eng.ctx) + " (" + path + ")", 1);
  };
  uint64_t fed = 0;
  stream_batches(rd, [&](const char* p, uint64_t n) { said(feed(p, n)); fed += n; });
  said(feed(nullptr, 0));
  return fed;
}

void put(std::string& out, uint64_t v) { out += std::to_string(v); }

std::string render(const std::vector<uint64_t>& table, const sg_eval_counts& C, int pct, simu_eval_stats& st) {
  std::string out;
  auto scalar = [&](const char* name, uint64_t v) { out += "#T\t"; out += name; out += '\t'; put(out, v); out += '\n'; };
  scalar("min_overlap", (uint64_t)pct);
  scalar("truth_records", C.truth_records);
  scalar("truth_duplicates", C.truth_duplicates);
  scalar("test_records", C.test_records);
  scalar("secondary", C.secondary);
  scalar("supplementary", C.supplementary);
  scalar("unknown", C.unknown);
  scalar("ambiguous", C.ambiguous);
  scalar("repeated", C.repeated);
  std::vector<uint64_t> mapped(kMapqs, 0), correct(kMapqs, 0);
  for (uint32_t mate = 0; mate < 2; mate++)
    for (uint32_t cls = 0; cls < kClasses; cls++)
      for (uint32_t q = 0; q < kMapqs; q++) {
        const uint64_t* row = &table[(((size_t)mate * kClasses + cls) * kMapqs + q) * kCategories];
        uint64_t any = 0;
        for (uint32_t c = 0; c < kCategories; c++) any += row[c];
        if (!any) continue;
        st.scored += any;
        out += "#M\t"; put(out, mate); out += '\t'; out += kClassName[cls]; out += '\t'; put(out, q);
        for (uint32_t c = 0; c < kCategories; c++) { out += '\t'; put(out, row[c]); }
        out += '\n';
        mapped[q] += any - row[5] - row[7];   // every category but lost and both_unmapped
        correct[q] += row[0] + row[1];        // exact + near
      }
  for (uint32_t mate = 0; mate < 2; mate++)
    for (uint32_t cls = 0; cls < kClasses; cls++) {
      out += "#X\t"; put(out, mate); out += '\t'; out += kClassName[cls]; out += '\t'; put(out, C.missing[mate * kClasses + cls]); out += '\n';
      st.missing += C.missing[mate * kClasses + cls];
    }
  uint64_t cum_mapped = 0, cum_correct = 0;
  for (int q = (int)kMapqs - 1; q >= 0; q--) {
    if (!mapped[q]) continue;
    cum_mapped += mapped[q];
    cum_correct += correct[q];
    out += "#R\t"; put(out, (uint64_t)q); out += '\t'; put(out, mapped[q]); out += '\t'; put(out, correct[q]); out += '\t'; put(out, cum_mapped);
    out += '\t'; put(out, cum_correct); out += '\n';
  }
  return out;
}

void run(const simu_eval_options& o, simu_eval_stats& st) {
  const auto t0 = Clock::now();
  const std::string truth = o.truth ? o.truth : "", bam = o.bam ? o.bam : "", output = o.output ? o.output : "";
  if (truth.empty()) throw Error("Error: no truth BAM file: use --truth to specify it.", 1);
  if (bam.empty()) throw Error("Error: no BAM file to evaluate: use --bam to specify it.", 1);
  if (o.min_overlap < 1 || o.min_overlap > 100) throw Error("Error: parameter \"min-overlap\" should be an integer from 1 to 100!", 1);
  need_bgzf(truth);
  need_bgzf(bam);
  Engine eng;
  if (sg_create(&eng.ctx, o.device, 0) != SG_OK) throw Error(std::string("GPU engine error: ") + sg_last_error(nullptr));
  const int threads = std::max(1, o.threads);
  std::vector<std::string> truth_names;
  st.truth_bgzf_bytes = stream_file(
      eng, truth, threads,
      [&](const BamHeader& H) {
        truth_names = H.names;
        eng.check(sg_eval_begin(eng.ctx, (uint32_t)H.names.size(), 64, (uint32_t)o.min_overlap, H.bytes), "sg_eval_begin");
      },
      [&](const void* p, uint64_t n) { return sg_eval_truth_bgzf(eng.ctx, p, n); });
  uint64_t n_truth = 0, n_dup = 0;
  eng.check(sg_eval_truth_done(eng.ctx, &n_truth, &n_dup), "sg_eval_truth_done");
  if (!o.quiet) std::cerr << "\nTruth: " << n_truth << " records from " << truth << (n_dup ? " (" + std::to_string(n_dup) + " with a name the file holds twice)" : "") << std::endl;
  std::map<std::string, int32_t> truth_id;
  for (size_t i = 0; i < truth_names.size(); i++) truth_id.emplace(truth_names[i], (int32_t)i);
  st.test_bgzf_bytes = stream_file(
      eng, bam, threads,
      [&](const BamHeader& H) {
        std::vector<int32_t> map(H.names.size() + 1, -1);
        for (size_t i = 0; i < H.names.size(); i++) {
          const auto it = truth_id.find(H.names[i]);
          if (it != truth_id.end()) map[i] = it->second;
        }
        eng.check(sg_eval_test_refmap(eng.ctx, map.data(), (uint32_t)H.names.size(), H.bytes), "sg_eval_test_refmap");
      },
      [&](const void* p, uint64_t n) { return sg_eval_test_bgzf(eng.ctx, p, n); });
  std::vector<uint64_t> table(SG_EVAL_CELLS);
  sg_eval_counts C;
  eng.check(sg_eval_finish(eng.ctx, table.data(), table.size(), &C), "sg_eval_finish");
  st.test_records = C.test_records; st.secondary = C.secondary; st.supplementary = C.supplementary; st.unknown = C.unknown;
  st.ambiguous = C.ambiguous; st.repeated = C.repeated; st.truth_records = C.truth_records; st.truth_duplicates = C.truth_duplicates;
  st.truth_bytes = C.truth_bytes; st.test_bytes = C.test_bytes;
  st.t_inflate = C.t_inflate; st.t_truth = C.t_truth; st.t_sort = C.t_sort; st.t_test = C.t_test;
  const std::string text = render(table, C, o.min_overlap, st);
  if (!output.empty()) {
    std::ofstream ofs(output.c_str(), std::ios::binary);
    if (!ofs.is_open()) throw Error("Error: cannot open file to save the evaluation:\n" + output, -1);
    ofs << text;
  } else {
    std::cout << text;
    std::cout.flush();
  }
  if (!o.quiet) std::cerr << "Evaluated: " << C.test_records << " records from " << bam << std::endl;
  st.t_total = since(t0);
}

}  // namespace
}  // namespace simu

extern "C" void simu_eval_default_options(simu_eval_options* o) {
  std::memset(o, 0, sizeof *o);
  o->min_overlap = 10;
  o->threads = 8;
}

extern "C" int simu_eval(const simu_eval_options* opt, simu_eval_stats* stats, char* err, size_t err_len) {
  return simu::guarded(err, err_len, [&]() {
    if (!opt) throw simu::Error("no options");
    simu_eval_stats st;
    std::memset(&st, 0, sizeof st);
    simu::run(*opt, st);
    if (stats) *stats = st;
  });
}
