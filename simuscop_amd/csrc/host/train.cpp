// host/train.cpp -- see train.h.  The host keeps what the reference's seqToProfile does once per run -- options, the VCF,
// the BED file, the arithmetic on the finished count matrices (a few hundred thousand numbers) and the file format -- and
// streams the reads through the GPU: the reference to HBM (Fasta::open_on_device), the SAM text in pinned chunks of whole
// lines while a reader thread fills the next one (sg_train_feed; BatchReader and stream_batches, host/input_stream.h).
#include "train.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/simuscop_amd.h"
#include "common.h"
#include "bam_reader.h"
#include "engine.h"
#include "fasta.h"
#include "input_stream.h"

namespace simu {
namespace {

using Clock = std::chrono::steady_clock;
double since(Clock::time_point t) { return std::chrono::duration<double>(Clock::now() - t).count(); }

constexpr double kZeroFinal = 2.2204e-16;   // lib/mydefine/MyDefine.cpp:20
constexpr uint32_t kWindow = 1000;          // Segment::fragSize
constexpr uint32_t kIsizeCols = 1u << 20, kIndelCols = 1u << 16;

// ---- lib/vcfparser/vcfparser.cpp:26-106 ----
struct KnownVariants {
  std::vector<uint32_t> snv_contig, ins_contig, del_contig;
  std::vector<int64_t> snv_pos, ins_pos, del_pos;
  std::string snv_alt;
  std::vector<uint8_t> snv_homo;
  std::vector<int32_t> ins_len, del_len;
  uint64_t n_snv = 0, n_ins = 0, n_del = 0;   // as the reference counts them (rows on contigs the FASTA lacks included)
};
// What the parser's loop does with one fragment -- what one fgets(buf, 20000) returned, NUL terminated; the fields are cut in
// place.  False: malformed (fewer than ten fields).  Both VCF routes run this: the host route on every fragment, the device
// route on those the device hands back undecided (csrc/sg_vcf.h).
bool vcf_fragment(char* buf, const std::map<std::string, uint32_t>& row_of, KnownVariants& kv) {
  if (buf[0] == '#') return true;
  // ten fields, the rest of the line stays with the tenth
  char* f[10];
  int nf = 0;
  char* p = buf;
  f[nf++] = p;
  while (*p && nf < 10) {
    if (*p == '\t') { *p = '\0'; f[nf++] = p + 1; }
    p++;
  }
  if (nf < 10) return false;
  const std::string info = f[7];
  const size_t dp = info.find("DP=");
  if (dp != std::string::npos) {
    const size_t semi = info.find(";", dp);
    if (atoi(info.substr(dp + 3, semi - dp - 3).c_str()) < 10) return true;   // depth_th
  }
  if ((float)atof(f[5]) < 20.0f) return true;                                  // quality_th
  const std::string chr = abbr_of_chr(f[0]);
  const long pos = atol(f[1]);
  std::string gt = f[9];
  gt = gt.substr(0, gt.find(':'));
  // (the parser files 1/1 as het and everything else as homo, :81-86: kept as it is -- including what fgets leaves behind:
  // a sample column that holds the genotype alone ends in the line break, and "1/1\n" is not "1/1")
  const bool homo = gt != "1/1";
  const auto it = row_of.find(chr);
  const size_t ref_len = strlen(f[3]), alt_len = strlen(f[4]);
  if (ref_len > 1) {
    kv.n_del++;
    if (it != row_of.end()) { kv.del_contig.push_back(it->second); kv.del_pos.push_back(pos + 1); kv.del_len.push_back((int32_t)ref_len - 1); }
  } else if (alt_len > 1) {
    kv.n_ins++;
    if (it != row_of.end()) { kv.ins_contig.push_back(it->second); kv.ins_pos.push_back(pos); kv.ins_len.push_back((int32_t)alt_len - 1); }
  } else {
    kv.n_snv++;
    if (it != row_of.end()) { kv.snv_contig.push_back(it->second); kv.snv_pos.push_back(pos); kv.snv_alt.push_back(f[4][0]); kv.snv_homo.push_back(homo ? 1 : 0); }
  }
  return true;
}
void vcf_malformed_warning(const std::string& path, uint64_t line_num) {
  std::cerr << "Warning: malformed VCF file " << path << ", there should be at least 10 fields @line " << line_num << std::endl;
}
void vcf_total_line(const std::string& path, const KnownVariants& kv) {
  std::cerr << "total " << kv.n_snv << " SNPs, " << kv.n_ins << " inserts and " << kv.n_del << " deletions were loaded from file " << path << std::endl;
}
void parse_vcf(const std::string& path, const std::map<std::string, uint32_t>& row_of, KnownVariants& kv, bool quiet, simu_train_stats& st) {
  if (path.empty()) { std::cerr << "Error: VCF file was not specified" << std::endl; return; }
  FILE* fp = fopen(path.c_str(), "r");
  if (!fp) throw Error("Error: cannot open VCF file " + path, -1);
  std::vector<char> buf(20000);
  long line_num = 0;
  int wrong = 0;
  while (fgets(buf.data(), (int)buf.size(), fp)) {
    line_num++;
    if (!vcf_fragment(buf.data(), row_of, kv)) {
      vcf_malformed_warning(path, (uint64_t)line_num);
      if (++wrong > 10) { fclose(fp); throw Error("", 1); }
    }
  }
  const long at = ftell(fp);
  st.vcf_bytes = at > 0 ? (uint64_t)at : 0;
  st.vcf_fragments = (uint64_t)line_num;
  fclose(fp);
  if (!quiet) vcf_total_line(path, kv);
}

// ---- the VCF through the device (sg_vcf_*, csrc/sg_vcf.h): the same rows, warnings and counts ----
enum class VcfForm { Plain, Bgzf, Gzip };
// What the file's first bytes say: gzip magic with a well-formed BGZF member header (SAMv1 section 4.1), gzip without, or
// anything else.  A file that cannot be opened is Plain: parse_vcf reports it where it always did.
VcfForm vcf_form(const std::string& path) {
  FILE* fp = path.empty() ? nullptr : fopen(path.c_str(), "rb");
  if (!fp) return VcfForm::Plain;
  std::vector<uint8_t> head(65536 + 64);
  const size_t n = fread(head.data(), 1, head.size(), fp);
  fclose(fp);
  if (n < 2 || head[0] != 31 || head[1] != 139) return VcfForm::Plain;
  uint64_t n_members = 0, whole = 0;
  return sg_bgzf_members(head.data(), n, nullptr, nullptr, nullptr, 1, &n_members, &whole) == SG_OK ? VcfForm::Bgzf : VcfForm::Gzip;
}

// ---- Genome::loadTargets (Genome.cpp:238-299) + divideTargets (:684-739) into inTargets ----
struct Piece { long spos, epos; };
std::map<std::string, std::vector<Piece>> load_targets(const std::string& path, const Fasta& fa, bool quiet) {
  std::map<std::string, std::vector<Piece>> raw, out;
  if (path.empty()) return out;
  std::ifstream ifs(path.c_str());
  if (!ifs.is_open()) throw Error("can not open target file " + path, -1);
  std::string line;
  int line_num = 0, n = 0;
  while (std::getline(ifs, line)) {
    line_num++;
    const std::vector<std::string> f = split(line, '\t');
    if (f.size() < 3) throw Error("ERROR: line " + std::to_string(line_num) + " should have at least 3 fields in file " + path + "\n" + line);
    const std::string chr = abbr_of_chr(f[0]);
    const long len = fa.length(chr);
    if (len <= 0) continue;
    const long e = atol(f[2].c_str());
    Piece t;
    t.spos = std::max(1L, atol(f[1].c_str()) - 50 + 1);
    t.epos = std::min(len, (e <= 0 ? len - (-e) % len : e) + 50);
    raw[chr].push_back(t);
    n++;
  }
  if (!quiet) std::cerr << "\ntotal " << n << " targets were loaded from file " << path << std::endl;
  for (const auto& kv : raw)
    for (const Piece& t : kv.second) {
      long spos = t.spos;
      const int k = (int)((t.epos - t.spos + 1) / (long)kWindow);
      for (int i = 0; i < k; i++) {
        const Piece p{spos, i == k - 1 ? t.epos : spos + (long)kWindow - 1};
        spos = p.epos + 1;
        out[kv.first].push_back(p);
      }
      if (spos <= t.epos) out[kv.first].push_back(Piece{spos, t.epos});
    }
  return out;
}

// ---- where the lines come from: a file, standard input, or `samtools view` as the reference runs it ----
std::unique_ptr<BatchReader> open_lines(sg_ctx* ctx, const simu_train_options& o) {
  const std::string sam = o.sam ? o.sam : "";
  if (!sam.empty()) return std::unique_ptr<BatchReader>(new BatchReader(ctx, sam, "SAM", o.threads, BatchReader::Lines));
  std::string samtools = o.samtools ? o.samtools : "";
  if (samtools.empty()) samtools = "samtools";
  const std::string bam = o.bam ? o.bam : "";
  const std::string cmd = samtools + " view -F 0xD04 -q 20 " + bam;   // Profile.cpp:1448
  FILE* fp = popen(cmd.c_str(), "r");
  if (!fp) throw Error("cannot open BAM file " + bam, -1);
  return std::unique_ptr<BatchReader>(new BatchReader(ctx, fp, pclose, bam, o.threads, BatchReader::Lines));
}

// CIGAR of a line when it is a single nM (Profile::setReadLength, Profile.cpp:155-163), else 0
int single_match_length(const char* p, const char* le) {
  int tabs = 0;
  while (p < le && tabs < 5) { if (*p == '\t') tabs++; p++; }
  if (tabs < 5) return 0;
  const char* e = p;
  while (e < le && *e != '\t') e++;
  const int n = (int)(e - p);
  int i = 0;
  for (; i < n - 1; i++) if (!(p[i] >= '0' && p[i] <= '9')) break;
  if (n >= 1 && i == n - 1 && p[i] == 'M') return atoi(std::string(p, e).c_str());
  return 0;
}

int bam_record_single_match(const uint8_t* r, uint32_t bs) {
  const int32_t ref = (int32_t)le32(r + 4), pos = (int32_t)le32(r + 8), lseq = (int32_t)le32(r + 20);
  const uint32_t lname = r[12], mapq = r[13], ncig = r[16] | ((uint32_t)r[17] << 8), flag = r[18] | ((uint32_t)r[19] << 8);
  if ((flag & 0xD04u) || mapq < 20 || lseq < 0) return 0;
  const uint64_t cig = 36 + lname, aux = cig + 4ull * ncig + ((uint64_t)lseq + 1) / 2 + (uint64_t)lseq, end = 4ull + bs;
  if (aux > end) return 0;
  const uint8_t* ops = r + cig;
  uint32_t nops = ncig;
  if (ncig > 0 && ref >= 0 && pos >= 0 && (ops[0] & 15u) == 4 && (le32(ops) >> 4) == (uint32_t)lseq) {   // htslib's bam_tag2cigar
    uint64_t p = aux;
    auto size_of = [](uint8_t t) -> uint32_t { return strchr("AcC", t) ? 1 : strchr("sS", t) ? 2 : strchr("iIf", t) ? 4 : t == 'd' ? 8 : 0; };
    while (p + 3 <= end) {
      const uint8_t t0 = r[p], t1 = r[p + 1], ty = r[p + 2];
      p += 3;
      if (ty == 'Z' || ty == 'H') { while (p < end && r[p]) p++; p++; continue; }
      if (ty == 'B') {
        if (p + 5 > end || !ty) break;
        const uint8_t sub = r[p];
        const uint32_t n = le32(r + p + 1), es = sub ? size_of(sub) : 0;
        if (!es) break;
        if (t0 == 'C' && t1 == 'G' && (sub == 'I' || sub == 'i')) {
          if (n >= ncig && n < (1u << 29) && p + 5 + 4ull * n <= end) { ops = r + p + 5; nops = n; }
          break;
        }
        p += 5 + (uint64_t)n * es;
        continue;
      }
      const uint32_t es = ty ? size_of(ty) : 0;
      if (!es) break;
      p += es;
    }
  }
  if (nops == 1 && (ops[0] & 15u) == 0) return (int)(le32(ops) >> 4);
  return 0;
}

// The device route of the VCF: the file's text (plain: pinned chunks cut anywhere; BGZF: batches of whole members) goes
// through sg_vcf_feed / sg_vcf_feed_bgzf while a reader thread fills the next chunk (stream_batches).  The fragments the device leaves
// undecided go through vcf_fragment here and are merged back by fragment number, so every list keeps the file's order.
void load_vcf_device(sg_ctx* ctx, const std::string& path, bool bgzf, const std::map<std::string, uint32_t>& row_of, KnownVariants& kv, bool quiet, int threads, simu_train_stats& st) {
  auto said = [&](int rc, const char* where) {
    if (rc == SG_OK) return;
    const std::string m = sg_last_error(ctx);
    if (rc == SG_ERR_INVALID) throw Error("Error: " + m + " (" + path + ")", 1);
    throw Error(std::string("GPU engine error in ") + where + ": " + m);
  };
  std::vector<const char*> keys;      // the map's keys, and the row each one stands for
  std::vector<uint32_t> row_of_key;
  for (const auto& kr : row_of) { keys.push_back(kr.first.c_str()); row_of_key.push_back(kr.second); }
  said(sg_vcf_begin(ctx, keys.data(), (uint32_t)keys.size()), "sg_vcf_begin");
  struct Session { sg_ctx* c; ~Session() { sg_vcf_end(c); } } session{ctx};
  KnownVariants hv;                                    // what the host resolved, and the fragment numbers of its kept rows
  std::vector<uint64_t> h_num[3], h_malformed;
  std::vector<char> buf(20000);
  auto resolve = [&]() {
    uint64_t n = 0, nb = 0;
    const int rc = sg_vcf_undecided(ctx, nullptr, 0, &n, nullptr, 0, &nb);
    if (rc == SG_OK && !n) return;
    if (rc != SG_ERR_OVERFLOW) said(rc, "sg_vcf_undecided");
    std::vector<sg_vcf_fragment> fr(n);
    std::vector<char> bytes(nb + 1);
    said(sg_vcf_undecided(ctx, fr.data(), n, &n, bytes.data(), nb, &nb), "sg_vcf_undecided");
    for (const sg_vcf_fragment& f : fr) {
      memcpy(buf.data(), bytes.data() + f.offset, f.len);
      buf[f.len] = '\0';
      const size_t before[3] = {hv.snv_pos.size(), hv.ins_pos.size(), hv.del_pos.size()};
      if (!vcf_fragment(buf.data(), row_of, hv)) h_malformed.push_back(f.number);
      if (hv.snv_pos.size() > before[0]) h_num[0].push_back(f.number);
      if (hv.ins_pos.size() > before[1]) h_num[1].push_back(f.number);
      if (hv.del_pos.size() > before[2]) h_num[2].push_back(f.number);
    }
  };
  {
    FILE* fp = fopen(path.c_str(), "rb");   // (the two forms have always worded this differently)
    if (!fp) throw Error((bgzf ? "cannot open VCF file " : "Error: cannot open VCF file ") + path, -1);
    BatchReader rd(ctx, fp, fclose, path, threads, bgzf ? BatchReader::Members : BatchReader::Anywhere, bgzf ? kVcfBatch + kMaxMember : kChunk);
    if (bgzf && rd.regular() && !rd.peek_eof_marker())
      std::cerr << "Warning: no BGZF EOF marker at the end of " << path << ". The input is probably truncated" << std::endl;
    stream_batches(rd, [&](const char* p, uint64_t n) {
      if (bgzf) said(sg_vcf_feed_bgzf(ctx, p, n), "sg_vcf_feed_bgzf");
      else said(sg_vcf_feed(ctx, p, n), "sg_vcf_feed");
      resolve();
    });
  }
  sg_vcf_counts C;
  said(sg_vcf_finish(ctx, &C), "sg_vcf_finish");
  resolve();   // (a last line without a line break)
  // ---- the warnings of malformed fragments, in file order; more than ten end the run (vcfparser.cpp:44-51) ----
  std::vector<uint64_t> bad(C.malformed_first, C.malformed_first + std::min<uint64_t>(C.malformed, 11));
  bad.insert(bad.end(), h_malformed.begin(), h_malformed.end());
  std::sort(bad.begin(), bad.end());
  const uint64_t n_bad = C.malformed + h_malformed.size();
  for (size_t i = 0; i < bad.size() && i < 11; i++) vcf_malformed_warning(path, bad[i]);
  if (n_bad > 10) throw Error("", 1);
  // ---- the rows: the device's and the host's, by fragment number ----
  const uint64_t n_dev[3] = {C.kept_snv, C.kept_ins, C.kept_del};
  for (int k = 0; k < 3; k++) {
    std::vector<sg_vcf_record> rows(n_dev[k]);
    said(sg_vcf_rows(ctx, (uint32_t)(SG_VCF_SNV + k), 0, n_dev[k], rows.data()), "sg_vcf_rows");
    size_t d = 0, h = 0;
    while (d < rows.size() || h < h_num[k].size()) {
      const bool from_host = d == rows.size() || (h < h_num[k].size() && h_num[k][h] < rows[d].fragment);
      if (k == 0) {
        if (from_host) { kv.snv_contig.push_back(hv.snv_contig[h]); kv.snv_pos.push_back(hv.snv_pos[h]); kv.snv_alt.push_back(hv.snv_alt[h]); kv.snv_homo.push_back(hv.snv_homo[h]); }
        else { kv.snv_contig.push_back(row_of_key[rows[d].contig]); kv.snv_pos.push_back(rows[d].pos); kv.snv_alt.push_back((char)rows[d].value); kv.snv_homo.push_back((rows[d].flags & SG_VCF_HOMO) ? 1 : 0); }
      } else {
        std::vector<uint32_t>& contig = k == 1 ? kv.ins_contig : kv.del_contig;
        std::vector<int64_t>& pos = k == 1 ? kv.ins_pos : kv.del_pos;
        std::vector<int32_t>& len = k == 1 ? kv.ins_len : kv.del_len;
        if (from_host) { contig.push_back((k == 1 ? hv.ins_contig : hv.del_contig)[h]); pos.push_back((k == 1 ? hv.ins_pos : hv.del_pos)[h]); len.push_back((k == 1 ? hv.ins_len : hv.del_len)[h]); }
        else { contig.push_back(row_of_key[rows[d].contig]); pos.push_back(rows[d].pos); len.push_back(rows[d].value); }
      }
      if (from_host) h++; else d++;
    }
  }
  kv.n_snv = C.n_snv + hv.n_snv; kv.n_ins = C.n_ins + hv.n_ins; kv.n_del = C.n_del + hv.n_del;
  st.vcf_bytes = C.text_bytes; st.vcf_fragments = C.fragments; st.vcf_undecided = C.undecided; st.vcf_on_device = 1;
  if (!quiet) vcf_total_line(path, kv);
}

// ---- the arithmetic of Profile::train behind the counting (Profile.cpp:1471-1483) ----
struct Model {
  std::string bases;
  int kmer = 3, bins = 50, kmer_count = 0, read_length = 0;
  std::vector<double> subs1, subs2, kmers, quality, isize, ins, del;   // the count matrices, then their normalised forms
  double insert_rate = 0, del_rate = 0, base_count = 0, std_isize = 0;
  std::vector<double> gcs, rcs;
  double gc_means[101];
  double gc_std = 0;
  bool gc_fitted = false;
};

double clamp0(double x) { return std::fabs(x) < kZeroFinal ? 0.0 : x; }   // Matrix::operator*, lib/matrix/Matrix.h:683-697

double median_of(std::vector<double> v) {   // lib/mydefine/MyDefine.h:72-104; no windows at all: 0
  if (v.empty()) return 0;
  std::sort(v.begin(), v.end());
  const size_t n = v.size();
  return (n & 1) ? v[n / 2] : (v[n / 2] + v[n / 2 - 1]) / 2;
}

// Profile::estimateGCParas (Profile.cpp:713-834): thin the windows to ~150,000, normalise the read counts by their median,
// fit a locally weighted line at every GC percent.  Four places where the reference reads memory it does not own are
// given a meaning here: the thinning counters start where the reference's do in practice -- its
// `new int[bins]` (:735) gets the block of the per-bin counts freed at :728, so bin b starts at per_bin[b], except for
// bins 0-3, whose first 16 bytes hold the allocator's free-list link and cleared key (zero here) -- a window of G/C only
// has a cell of its own, fewer than 50 windows thin nothing, and without any fitted percent no tail is extrapolated.
void fit_gc_model(Model& M, const std::string& gc_file) {
  const int B = 50;
  std::vector<int> per_bin(B + 1, 0), step(B + 1, 1);
  for (double g : M.gcs) per_bin[(int)(g * B)]++;
  std::vector<int> seen(per_bin);
  for (int b = 0; b < 4; b++) seen[b] = 0;
  const int expect = std::min(150000, (int)M.gcs.size()) / B;
  if (expect > 0)
    for (int b = 0; b <= B; b++) step[b] = std::max(1, per_bin[b] / expect);
  std::ofstream ofs(gc_file.c_str());
  std::vector<int> kept;
  const double med = median_of(M.rcs);
  for (size_t i = 0; i < M.rcs.size(); i++) {
    const int b = (int)(M.gcs[i] * B);
    if (seen[b] % step[b] == 0) {
      M.rcs[i] = M.rcs[i] / (med + kZeroFinal);
      if (M.rcs[i] < 3) {
        ofs << M.rcs[i] << '\t' << M.gcs[i] << std::endl;
        kept.push_back((int)i);
      }
    }
    seen[b]++;
  }
  ofs.close();
  const double tau = 5, half = 0.03 / 2;
  int lo = -1, hi = -1;
  std::vector<double> g, r, w;
  for (int k = 0; k <= 100; k++) {
    const double at = k / 100.0;
    g.clear(); r.clear();
    for (int j : kept)
      if (std::fabs(at - M.gcs[j]) <= half) { g.push_back(M.gcs[j]); r.push_back(M.rcs[j]); }
    if (g.size() <= 20) { M.gc_means[k] = 0; continue; }
    if (lo < 0) lo = k;
    hi = k;
    // beta = (B'WB)^-1 B'W y, B = [1 g], W = diag(w): the reference forms every product as a dense Matrix product -- running
    // sums from zero in index order, each result clamped to 0 below 2.2204e-16 -- and the sums over the diagonal W have one
    // term that is not zero.  Same operations, same order, without the n x n matrix.
    const size_t n = g.size();
    w.resize(n);
    double a00 = 0, a01 = 0, a10 = 0, a11 = 0;
    for (size_t i = 0; i < n; i++) {
      w[i] = std::exp(-std::pow(g[i] - at, 2) / (2 * tau));
      const double u0 = clamp0(0.0 + 1.0 * w[i]), u1 = clamp0(0.0 + g[i] * w[i]);   // (B'W)[.][i]
      a00 += u0 * 1.0; a01 += u0 * g[i]; a10 += u1 * 1.0; a11 += u1 * g[i];
    }
    a00 = clamp0(a00); a01 = clamp0(a01); a10 = clamp0(a10); a11 = clamp0(a11);
    // determinant by elimination (Matrix.h:223-268), then the cofactor inverse (:184-220)
    double c00 = a00, c01 = a01, c10 = a10, c11 = a11;
    bool swapped = false, stuck = false;
    if (c00 == 0) {
      if (c10 == 0) stuck = true;
      else { std::swap(c00, c10); std::swap(c01, c11); swapped = true; }
    }
    if (!stuck && c10 != 0) {
      const double q = c10 / c00;
      c10 -= q * c00;
      c11 -= q * c01;
    }
    double det = 1.0;
    det *= c00;
    det *= c11;
    if (swapped) det = -det;
    const double i00 = clamp0(a11 / det), i01 = clamp0(-a01 / det), i10 = clamp0(-a10 / det), i11 = clamp0(a00 / det);
    double b0 = 0, b1 = 0;
    for (size_t i = 0; i < n; i++) {
      double p0 = 0, p1 = 0;
      p0 += i00 * 1.0; p0 += i01 * g[i];
      p1 += i10 * 1.0; p1 += i11 * g[i];
      b0 += clamp0(0.0 + clamp0(p0) * w[i]) * r[i];
      b1 += clamp0(0.0 + clamp0(p1) * w[i]) * r[i];
    }
    b0 = clamp0(b0); b1 = clamp0(b1);
    double y = 0;
    y += 1.0 * b0;
    y += at * b1;
    M.gc_means[k] = std::max(0.0, clamp0(y));
  }
  if (lo >= 0) {   // (no percent with more than 20 windows -- an exome with few targets: every mean stays 0)
    for (int k = 0; k < lo; k++) M.gc_means[k] = M.gc_means[lo] * k / lo;
    for (int k = hi + 1; k <= 100; k++) M.gc_means[k] = M.gc_means[hi] - M.gc_means[hi] * (k - hi) / (100 - hi);
  }
  double ss = 0;
  for (int j : kept) ss += std::pow(M.rcs[j] - M.gc_means[(int)(M.gcs[j] * 100)], 2);
  M.gc_std = std::sqrt(ss / kept.size());
}

// Matrix::normalize(0) (Matrix.h:483-503) on `rows` rows of `cols` numbers
void normalise_rows(double* m, size_t rows, size_t cols) {
  for (size_t i = 0; i < rows; i++) {
    double s = 0;
    for (size_t j = 0; j < cols; j++) s += m[i * cols + j];
    for (size_t j = 0; j < cols; j++) m[i * cols + j] /= (kZeroFinal + s);
  }
}

// the k-mer of context index i (Profile::initKmers, Profile.cpp:70-124): contexts of one real base first, X-padded
std::string kmer_text(const Model& M, int i) {
  int m = 1, first = 0, block = 4;
  while (i >= first + block) { first += block; block *= 4; m++; }
  int v = i - first;
  std::string s((size_t)M.kmer, 'X');
  for (int t = M.kmer - 1; t >= M.kmer - m; t--) { s[(size_t)t] = M.bases[(size_t)(v & 3)]; v >>= 2; }
  return s;
}

// Profile::normParas(false), Profile.cpp:836-900
void normalise(Model& M) {
  const int N = 4, bins = M.bins;
  normalise_rows(M.kmers.data(), (size_t)bins, (size_t)M.kmer_count);
  for (int i = 0; i < M.kmer_count; i++) {
    const std::string km = kmer_text(M, i);
    const int last = (int)M.bases.find(km[(size_t)M.kmer - 1]);
    for (std::vector<double>* sd : {&M.subs1, &M.subs2}) {
      double* blk = sd->data() + (size_t)i * bins * N;
      normalise_rows(blk, (size_t)bins, N);
      for (int j = 0; j < bins; j++) {   // an empty row becomes "no substitution" (:847-861)
        double s = 0;
        for (int k = 0; k < N; k++) s += blk[j * N + k];
        if (s < kZeroFinal) blk[j * N + last] = 1;
      }
    }
  }
  for (int i = 0; i < N * N; i++) normalise_rows(M.quality.data() + (size_t)i * bins * 94, (size_t)bins, 94);
  // insert sizes: the mode, everything from five times the mode on dropped, standard deviation of what is left (:869-891)
  int best = 0, mode = 0;
  for (size_t i = 0; i < M.isize.size(); i++)
    if (M.isize[i] > best) { best = (int)M.isize[i]; mode = (int)i; }
  for (size_t i = (size_t)mode * 5; i < M.isize.size(); i++) M.isize[i] = 0;
  normalise_rows(M.isize.data(), 1, M.isize.size());
  auto col = [&](int i) { return (size_t)i < M.isize.size() ? M.isize[(size_t)i] : 0.0; };   // (past the row: 0)
  double mean = 0;
  for (int i = 0; i < mode * 5; i++) mean += col(i) * i;
  double var = 0;
  for (int i = 0; i < mode * 5; i++) var += col(i) * std::pow(i - mean, 2);
  M.std_isize = std::sqrt(var);
  normalise_rows(M.ins.data(), 1, M.ins.size());
  normalise_rows(M.del.data(), 1, M.del.size());
  M.insert_rate /= M.base_count;
  M.del_rate /= M.base_count;
}

// Profile::saveResults, Profile.cpp:1240-1365
void write_profile(const Model& M, std::ostream& os, const std::string& reads_label, const std::string& stamp) {
  const int N = 4;
  os << "#model created at " << stamp;
  os << "#reads: " << reads_label << std::endl << std::endl;
  os << "bases: " << M.bases << std::endl;
  os << "readLength: " << M.read_length << std::endl;
  os << "binCount: " << M.bins << std::endl;
  os << "kmer: " << M.kmer << std::endl << std::endl;
  auto row = [&](const std::vector<double>& v) {
    for (size_t i = 0; i + 1 < v.size(); i++) os << v[i] << '\t';
    os << v.back() << std::endl;
  };
  os << "\n[Insert Rate]" << std::endl << M.insert_rate << std::endl << "[Insert Frequency]" << std::endl;
  row(M.ins);
  os << "\n[Deletion Rate]" << std::endl << M.del_rate << std::endl << "[Deletion Frequency]" << std::endl;
  row(M.del);
  os << "\n[Substitution Probs]" << std::endl;
  for (int i = 0; i < M.kmer_count; i++) {
    os << "kmer: " << kmer_text(M, i) << std::endl;
    for (const std::vector<double>* sd : {&M.subs1, &M.subs2}) {
      const double* p = sd->data() + (size_t)i * M.bins * N;
      for (int j = 0; j < M.bins; j++)
        for (int k = 0; k < N; k++) os << p[j * N + k] << (k < N - 1 ? '\t' : '\n');
    }
  }
  os << "\n[Base Quality Distribution]" << std::endl;
  for (int i = 0; i < N * N; i++) {
    os << "basePairIndx: " << i << std::endl;
    const double* p = M.quality.data() + (size_t)i * M.bins * 94;
    for (int j = 0; j < M.bins; j++)
      for (int k = 0; k < 94; k++) os << p[j * 94 + k] << (k < 93 ? '\t' : '\n');
  }
  os << "\n[Insert Size Standard Deviation]" << std::endl << M.std_isize << std::endl;
  os << "\n[Log Ratio Mean Value]" << std::endl;
  for (int i = 0; i < 101; i++) os << i << '\t' << M.gc_means[i] << std::endl;
  os << "\n[Log Ratio Standard Deviation]" << std::endl << M.gc_std << std::endl;
}

void run(const simu_train_options& o, simu_train_stats& st) {
  const auto t0 = Clock::now();
  const bool quiet = o.quiet != 0;
  const std::string ref = o.ref ? o.ref : "", vcf = o.vcf ? o.vcf : "", target = o.target ? o.target : "", output = o.output ? o.output : "";
  // a compressed VCF: BGZF goes through the device, any other gzip file is refused before anything is touched
  const VcfForm form = vcf_form(vcf);
  if (form == VcfForm::Gzip)
    throw Error("Error: VCF file " + vcf + " is gzip-compressed but not BGZF: decompress it, or recompress it with bgzip", 1);
  Engine eng;
  if (sg_create(&eng.ctx, o.device, 0) != SG_OK) throw Error(std::string("GPU engine error: ") + sg_last_error(nullptr));
  // ---- Genome::loadTrainData: VCF, reference, targets (Genome.cpp:32-39; the VCF needs the contig rows, so the reference
  // goes first here) ----
  auto t1 = Clock::now();
  Fasta fa;
  fa.open_on_device(ref, eng.ctx, std::max(1, o.threads));
  if (fa.names.empty()) throw Error("ERROR: reference sequence cannot be empty!");
  if (!quiet) std::cerr << "\nReference sequence was loaded from file " << ref << std::endl;
  st.t_reference = since(t1);
  std::vector<std::string> key_of_row(fa.contigs.size());
  for (const auto& kv : fa.contig_of) key_of_row[kv.second] = kv.first;
  KnownVariants kv;
  t1 = Clock::now();
  if (form == VcfForm::Bgzf || (o.device_vcf && !vcf.empty()))
    load_vcf_device(eng.ctx, vcf, form == VcfForm::Bgzf, fa.contig_of, kv, quiet, std::max(1, o.threads), st);
  else
    parse_vcf(vcf, fa.contig_of, kv, quiet, st);
  st.t_vcf = since(t1);
  const std::map<std::string, std::vector<Piece>> targets = load_targets(target, fa, quiet);
  std::vector<uint64_t> tfirst(key_of_row.size() + 1, 0);
  std::vector<int64_t> tspos, tepos;
  for (size_t r = 0; r < key_of_row.size(); r++) {
    tfirst[r] = tspos.size();
    const auto it = targets.find(key_of_row[r]);
    if (it != targets.end())
      for (const Piece& p : it->second) { tspos.push_back(p.spos); tepos.push_back(p.epos); }
  }
  tfirst[key_of_row.size()] = tspos.size();
  // ---- Profile::init (Profile.cpp:172-218): the read length is the first single-nM CIGAR of the text ----
  const bool decode_bam = o.decode_bam != 0;
  std::unique_ptr<BatchReader> rd;   // the BAM's members (--decode-bam), else lines of SAM text
  BamHeader bam_header;
  std::vector<std::string> replay;   // (standard input: the batches the header and the read length took)
  int read_length = 0;
  if (decode_bam) {
    rd.reset(new BatchReader(eng.ctx, o.bam ? o.bam : "", "BAM", o.threads, BatchReader::Members));
    if (rd->regular() && !rd->peek_eof_marker())   // a file shows its end now; a pipe once it is read
      std::cerr << "[W::bam_hdr_read] EOF marker is absent. The input is probably truncated" << std::endl;
    bam_prepare(eng.ctx, *rd, bam_header, replay, bam_record_single_match, &read_length);
    if (rd->regular()) rd->rewind();
  } else {
    rd = open_lines(eng.ctx, o);
    const char* p = rd->data(0);
    const char* end = p + (rd->first() ? rd->len[0] : 0);
    while (p < end && !read_length) {
      const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
      const char* le = nl ? nl : end;
      read_length = single_match_length(p, le);
      p = nl ? nl + 1 : end;
    }
  }
  const std::string reads_label = rd->what;
  if (read_length <= 0) throw Error("Error: no read with a single match in its CIGAR among the first lines of " + reads_label);
  Model M;
  M.bases = "ACTG";   // (Config.cpp: the default of "bases"; seqToProfile has no option for it)
  M.kmer = o.kmer; M.bins = std::min(o.bins, read_length); M.read_length = read_length;
  for (int m = 1, p4 = 4; m <= M.kmer; m++, p4 *= 4) M.kmer_count += p4;
  // ---- Profile::train, the counting (Profile.cpp:1442-1469) ----
  t1 = Clock::now();
  std::vector<const char*> keys;
  for (const std::string& k : key_of_row) keys.push_back(k.c_str());
  sg_train_setup S;
  memset(&S, 0, sizeof S);
  S.contig_keys = keys.data(); S.n_contigs = (uint32_t)keys.size();
  S.bases = M.bases.c_str(); S.kmer = M.kmer; S.bins = M.bins;
  S.n_isize = kIsizeCols; S.n_indel_len = kIndelCols; S.count_gc = 1; S.window = kWindow; S.max_reads = o.max_reads;
  if (!tspos.empty()) { S.target_first = tfirst.data(); S.target_spos = tspos.data(); S.target_epos = tepos.data(); }
  S.n_snv = kv.snv_pos.size(); S.snv_contig = kv.snv_contig.data(); S.snv_pos = kv.snv_pos.data(); S.snv_alt = kv.snv_alt.data(); S.snv_homo = kv.snv_homo.data();
  S.n_ins = kv.ins_pos.size(); S.ins_contig = kv.ins_contig.data(); S.ins_pos = kv.ins_pos.data(); S.ins_len = kv.ins_len.data();
  S.n_del = kv.del_pos.size(); S.del_contig = kv.del_contig.data(); S.del_pos = kv.del_pos.data(); S.del_len = kv.del_len.data();
  eng.check(sg_train_begin(eng.ctx, &S), "sg_train_begin");
  // (a chunk's verdict -- a malformed line, the cap -- is known when the next chunk is fed or at sg_train_finish)
  auto engine_said = [&](int rc, const char* where) {
    if (rc == SG_OK) return;
    const std::string m = sg_last_error(eng.ctx);
    if (rc == SG_ERR_INVALID && m.find("malformed read") != std::string::npos) throw Error(m, 1);
    throw Error(std::string("GPU engine error in ") + where + ": " + m);
  };
  auto not_capped = [&]() { return !sg_train_capped(eng.ctx); };   // (at the cap the reference leaves its loop: the rest of the input is not read)
  if (decode_bam) {
    std::vector<const char*> names;
    for (const std::string& n : bam_header.names) names.push_back(n.c_str());
    eng.check(sg_train_bam_start(eng.ctx, names.data(), (uint32_t)names.size(), bam_header.bytes), "sg_train_bam_start");
    for (const std::string& b : replay) {
      if (sg_train_capped(eng.ctx)) break;
      engine_said(sg_train_feed_bgzf(eng.ctx, b.data(), b.size()), "sg_train_feed_bgzf");
      st.bam_bytes += b.size();
    }
    replay.clear();
    if (not_capped())
      stream_batches(*rd, [&](const char* p, uint64_t n) { engine_said(sg_train_feed_bgzf(eng.ctx, p, n), "sg_train_feed_bgzf"); st.bam_bytes += n; }, not_capped);
    if (not_capped()) engine_said(sg_train_feed_bgzf(eng.ctx, nullptr, 0), "sg_train_feed_bgzf");
    if (!rd->regular() && !rd->eof_marker() && not_capped())
      std::cerr << "[W::bam_hdr_read] EOF marker is absent. The input is probably truncated" << std::endl;
    eng.check(sg_train_bam_info(eng.ctx, &st.bam_records, nullptr, &st.t_inflate), "sg_train_bam_info");
  } else {
    stream_batches(*rd, [&](const char* p, uint64_t n) { engine_said(sg_train_feed(eng.ctx, p, n), "sg_train_feed"); st.sam_bytes += n; }, not_capped);
  }
  const size_t subs_n = (size_t)M.kmer_count * M.bins * 4, kmers_n = (size_t)M.bins * M.kmer_count, qual_n = (size_t)16 * M.bins * 94;
  std::vector<uint64_t> c_subs1(subs_n), c_subs2(subs_n), c_kmers(kmers_n), c_qual(qual_n), c_isize(kIsizeCols), c_ins(kIndelCols), c_del(kIndelCols);
  sg_train_counts C;
  memset(&C, 0, sizeof C);
  C.subs1 = c_subs1.data(); C.subs2 = c_subs2.data(); C.kmers = c_kmers.data(); C.quality = c_qual.data();
  C.isize = c_isize.data(); C.ins_len = c_ins.data(); C.del_len = c_del.data();
  uint64_t n_gc = 0;
  {
    std::vector<double> gc(1), rc(1);
    int rcode = sg_train_finish(eng.ctx, &C, gc.data(), rc.data(), 0, &n_gc);
    (void)rcode;   // (gc_cap 0: the pairs are counted, the session stays open when there are any)
    if (rcode == SG_ERR_OVERFLOW) {
      M.gcs.resize(n_gc); M.rcs.resize(n_gc);
      engine_said(sg_train_finish(eng.ctx, &C, M.gcs.data(), M.rcs.data(), n_gc, &n_gc), "sg_train_finish");
    } else {
      engine_said(rcode, "sg_train_finish");
    }
  }
  st.t_reads = since(t1);
  rd.reset();
  if (C.isize_overflow || C.indel_len_overflow)
    throw Error("Error: insert sizes beyond " + std::to_string(kIsizeCols) + " or CIGAR insertions / deletions beyond " + std::to_string(kIndelCols) +
                " bases in the reads (" + std::to_string(C.isize_overflow) + " / " + std::to_string(C.indel_len_overflow) + " of them): not representable");
  auto as_double = [](const std::vector<uint64_t>& v, size_t n) { std::vector<double> d(n); for (size_t i = 0; i < n; i++) d[i] = (double)v[i]; return d; };
  auto grown = [](const std::vector<uint64_t>& v, size_t least) {   // the row as the reference grew it: up to the largest length met
    size_t n = least;
    for (size_t i = v.size(); i-- > least;) if (v[i]) { n = i + 1; break; }
    return n;
  };
  M.subs1 = as_double(c_subs1, subs_n); M.subs2 = as_double(c_subs2, subs_n); M.kmers = as_double(c_kmers, kmers_n); M.quality = as_double(c_qual, qual_n);
  M.isize = as_double(c_isize, grown(c_isize, 10)); M.ins = as_double(c_ins, grown(c_ins, 1)); M.del = as_double(c_del, grown(c_del, 1));
  M.insert_rate = (double)C.insert_events; M.del_rate = (double)C.delete_events; M.base_count = (double)C.cigar_chars;
  // ---- the GC model (Profile.cpp:1471-1481) ----
  const double med = median_of(M.rcs);
  if (med < 5) {
    if (!quiet) std::cerr << "\nWarning: no enough reads to evaluate GC-content effects!" << std::endl;
    for (double& m : M.gc_means) m = 1;   // Profile::initGCParas, :705-711
    M.gc_std = 1.0e-5;
  } else {
    fit_gc_model(M, output + ".gc");
    M.gc_fitted = true;
    if (!quiet) std::cerr << "\nread counts std: " << M.gc_std << std::endl;
  }
  normalise(M);
  if (!quiet) std::cerr << "insert rate: " << M.insert_rate << ", deletion rate: " << M.del_rate << std::endl;
  std::string stamp;
  if (o.stamp) stamp = o.stamp;
  else { time_t now; time(&now); stamp = asctime(gmtime(&now)); }
  if (!output.empty()) {
    std::ofstream ofs(output.c_str());
    if (!ofs.is_open()) throw Error("Error: cannot open file to save model training results:\n" + output, -1);
    write_profile(M, ofs, reads_label, stamp);
  } else {
    write_profile(M, std::cout, reads_label, stamp);
  }
  st.lines = C.lines; st.reads_counted = C.reads_counted; st.gc_rejected = C.gc_rejected; st.gc_windows = C.gc_windows;
  st.gc_pairs = n_gc; st.skipped_overhang = C.skipped_overhang; st.read_length = read_length; st.bins = M.bins;
  st.capped = (int32_t)C.capped;
  st.gc_fitted = M.gc_fitted ? 1 : 0; st.insert_rate = M.insert_rate; st.del_rate = M.del_rate; st.std_isize = M.std_isize; st.gc_std = M.gc_std;
  st.t_total = since(t0);
}

}  // namespace
}  // namespace simu

extern "C" void simu_train_default_options(simu_train_options* o) {
  std::memset(o, 0, sizeof *o);
  o->kmer = 3;
  o->bins = 50;
  o->threads = 8;
}

extern "C" int simu_train(const simu_train_options* opt, simu_train_stats* stats, char* err, size_t err_len) {
  return simu::guarded(err, err_len, [&]() {
    if (!opt) throw simu::Error("no options");
    simu_train_stats st;
    std::memset(&st, 0, sizeof st);
    simu::run(*opt, st);
    if (stats) *stats = st;
  });
}
