// sg_truth.h -- truth alignments of the sampled reads (simuReads --truth-bam): the alignment rule, once, for the host
// function sg_truth_align and for the record kernels of sg_truth.hip, and what those kernels share with the host API.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sg_emit.h"

namespace sg {

// CIGAR operation codes of SAMv1 section 4.2
enum : uint32_t { kOpM = 0, kOpI = 1, kOpD = 2, kOpN = 3, kOpS = 4 };

// One entry of the piece map (sg_build_haplotypes' copy list, sorted by chain and offset): 24 bytes.
struct TruthPiece {
  uint64_t dst;    // offset in its chain
  uint64_t src;    // kind 0: 0-based position on the contig
  uint32_t len;
  uint32_t meta;   // contig (BAM refID) | kind << 30 | seg_first << 31
};
__host__ __device__ inline uint32_t truth_meta(uint32_t contig, uint32_t kind, uint32_t seg_first) {
  return (contig & 0x3FFFFFFFu) | ((kind ? 1u : 0u) << 30) | ((seg_first ? 1u : 0u) << 31);
}

// What the walk found: the alignment's contig, the position of its first and behind its last M base, its operations.
struct TruthAln {
  int32_t contig;
  int64_t pos0, end;
  uint32_t n_ops;
};

// The alignment rule (DESIGN.md "Truth alignments").  The template is `L` chain bases from `tmpl_off` on; `pieces` are
// its chain's pieces in offset order, `pi` the index of the one that holds tmpl_off.  Events are in read direction
// (ev_pack form): for a reverse read index j counts from the template's chain end.  The walk goes base by base in chain
// direction and hands runs of operations to `put(index, len << 4 | op)`; what it hands over is already normalised:
//   * before the first M base nothing is put: query bases met there (literal bases, inserted bases) are summed up and
//     become one S in front of that M, gaps are dropped (the position is the first M base's);
//   * operations behind an M run are put as they close; at the end everything behind the last M run is withdrawn
//     (n_ops steps back: `put` may have been called for indexes that do not count) and its query bases become one S.
// A read without an M base is unmapped: n_ops = 0, contig = -1.
template <class Put>
__host__ __device__ inline TruthAln truth_walk(const TruthPiece* pieces, uint64_t n_pieces, uint64_t pi, uint64_t tmpl_off, uint32_t L,
                                               bool reverse, const uint32_t* events, uint32_t n_events, Put put) {
  TruthAln A;
  A.contig = -1; A.pos0 = -1; A.end = -1; A.n_ops = 0;
  uint32_t n = 0, cur_op = kOpM, cur_len = 0, m_end = 0, lead_q = 0, q_since = 0;
  bool seen_m = false;
  auto unit = [&](uint32_t op, uint32_t len, int64_t refpos) {
    if (!len) return;
    if (!seen_m) {
      if (op == kOpM) {
        seen_m = true;
        if (lead_q) put(n++, (lead_q << 4) | kOpS);
        cur_op = kOpM; cur_len = len;
        A.pos0 = refpos; A.end = refpos + len;
      } else if (op == kOpI || op == kOpS) {
        lead_q += len;
      }
      return;
    }
    if (op == cur_op) {
      cur_len += len;
    } else {
      put(n++, (cur_len << 4) | cur_op);
      if (cur_op == kOpM) m_end = n;
      cur_op = op; cur_len = len;
    }
    if (op == kOpM) { q_since = 0; A.end = refpos + len; }
    else if (op == kOpI || op == kOpS) q_since += len;
  };

  // the last reference piece walked through: where it ends on its contig; whether a segment began since
  bool have_ref = false, broken = false, seg_began = false;
  uint32_t ref_contig = 0;
  uint64_t ref_next = 0;
  int e = reverse ? (int)n_events - 1 : 0;   // next event in chain direction
  uint32_t del_until = 0;
  bool fresh = true;                          // the current piece has not been looked at yet
  for (uint32_t c = 0; c < L; c++) {
    const uint64_t at = tmpl_off + c;
    while (pi + 1 < n_pieces && at >= pieces[pi].dst + pieces[pi].len) { pi++; fresh = true; }
    const TruthPiece& p = pieces[pi];
    const bool literal = (p.meta >> 30) & 1u;
    if (fresh) {
      fresh = false;
      if (c > 0 && (p.meta >> 31)) seg_began = true;
      if (!literal) {
        const uint32_t contig = p.meta & 0x3FFFFFFFu;
        const uint64_t here = p.src + (at - p.dst);
        if (have_ref && !broken) {
          if (contig != ref_contig || here < ref_next) broken = true;
          else if (here > ref_next) unit(seg_began ? kOpN : kOpD, (uint32_t)(here - ref_next), 0);
        }
        have_ref = true;
        ref_contig = contig;
        ref_next = p.src + p.len;
        seg_began = false;
        if (!seen_m && !broken) A.contig = (int32_t)contig;
      }
    }
    const uint32_t cls = broken ? kOpS : literal ? kOpI : kOpM;
    const int64_t refpos = (int64_t)(p.src + (at - p.dst));
    uint32_t ins_behind = 0;
    if (!reverse) {
      if (e < (int)n_events && (events[e] & 0xFFFFu) == c) {
        const uint32_t k = (events[e] >> 16) & 0x7FFFu;
        if (events[e] >> 31) del_until = c + k; else ins_behind = k;
        e++;
      }
    } else if (e >= 0) {
      const uint32_t j = events[e] & 0xFFFFu, k = (events[e] >> 16) & 0x7FFFu;
      if (events[e] >> 31) {
        if (L - j - k == c) { del_until = c + k; e--; }
      } else if (L - 1u - j == c) {
        unit(cls == kOpS ? kOpS : kOpI, k, 0);   // read direction: behind base j = in front of it on the chain
        e--;
      }
    }
    if (c < del_until) {
      if (cls == kOpM) unit(kOpD, 1, refpos);
    } else {
      unit(cls, 1, refpos);
    }
    if (ins_behind) unit(cls == kOpS ? kOpS : kOpI, ins_behind, 0);
  }
  if (!seen_m) { A.contig = -1; A.pos0 = -1; A.end = -1; return A; }
  if (cur_op == kOpM) {
    put(n++, (cur_len << 4) | kOpM);
  } else {
    n = m_end;
    if (q_since) put(n++, (q_since << 4) | kOpS);
  }
  A.n_ops = n;
  return A;
}

// index of the piece of [first, last) that holds chain offset `off` (the pieces tile the chain)
__host__ __device__ inline uint64_t truth_find_piece(const TruthPiece* pieces, uint64_t first, uint64_t last, uint64_t off) {
  uint64_t lo = first, hi = last;   // the last piece with dst <= off
  while (lo + 1 < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (pieces[mid].dst <= off) lo = mid; else hi = mid;
  }
  return lo;
}

// reg2bin of SAMv1 section 5.3 for [beg, end)
__host__ __device__ inline uint32_t truth_reg2bin(int64_t beg, int64_t end) {
  --end;
  if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
  return 0;
}

// What the pass left of read (t, m): the meta row of fragment_kernel and the fragment's window
struct ReadGeom {
  bool live, inside;      // inside: the template lies in its chain
  uint32_t chain, reverse, np, nev, hdr;
  uint64_t tmpl_off;      // chain-local
  const uint32_t* events;
};
__device__ __forceinline__ ReadGeom read_geom(const DevProfile& P, const DevBatch& B, uint32_t t, uint32_t m) {
  ReadGeom g = {};
  const size_t idx = (size_t)m * B.n_slots + t;
  ReadRow rd;   // (sg_emit.h)
  rd.m1 = B.meta[idx * 3 + 1];
  const uint32_t flen = rd.flen();
  g.live = flen != 0u;
  if (!g.live) return g;
  rd.m0 = B.meta[idx * 3];
  const uint64_t foff = rd.frag_off();
  const uint32_t L = (uint32_t)P.L;
  g.reverse = rd.rev() ? 1u : 0u;
  g.np = rd.np();
  g.nev = rd.nev();   // the row's count: fragment_kernel drops the events of a read that would get shorter than 50
  g.hdr = rd.hdr_len();
  g.chain = B.windows[slot_window(B, t)].chain;
  const uint64_t c0 = B.chain_off[g.chain], tmpl = g.reverse ? foff + flen - L : foff;
  g.inside = flen >= L && tmpl >= c0 && tmpl - c0 + L <= B.chain_len[g.chain];
  g.tmpl_off = tmpl - c0;
  g.events = B.events + idx * SG_MAX_EVENTS;
  return g;
}

// where read t's FASTQ record starts in its mate's text
__device__ __forceinline__ uint64_t text_offset(const DevBatch& B, uint32_t m, uint32_t t) { return rec_offset(B, m, t); }

constexpr uint32_t kTruthMaxOps = 256;     // CIGAR operations of one record (more: SG_ERR_OVERFLOW)
constexpr uint32_t kTruthWaveOps = 2048;   // ... and of the 64 records one wave packs

// Per read, in record order (index = slot * mates + mate): what the sizing kernel found.
struct TruthRow {
  int32_t contig;   // -1: unmapped
  int32_t pos, end;
  uint32_t n_ops;
};

// The piece map as a pass's kernels read it, and the reads they run over: the first member of every job that maps reads
// back to the reference.  On the device the map is one buffer (sg_truth_map writes it, the pass prelude of sg_api.h
// reads it): chain_first, then from truth_map_pieces_at() on the pieces.
struct PieceMap {
  const TruthPiece* pieces;
  const uint64_t* chain_first;   // [n_chains + 1] first piece of every chain
  uint32_t n_chains;
  uint32_t n_reads;              // n_slots * mates
};
inline size_t truth_map_pieces_at(size_t n_chains) { return ((n_chains + 1) * 8 + 63) & ~(size_t)63; }

// Read `idx` of a pass in record order (index = slot * mates + mate): whether there is one, its slot and its mate.  The
// kernels then take its geometry behind `in_range` (an index behind the last read keeps the empty one: not live) and
// test its chain against the piece map's.  (Those stay the caller's own lines: with the geometry fetched or tested
// through a wrapper too, the kernels come out with other register counts than they had.)
struct PassRead {
  bool in_range;
  uint32_t t, m;
};
__device__ __forceinline__ PassRead pass_read(const DevBatch& B, uint32_t idx, uint32_t n_reads) {
  const uint32_t nm = B.paired ? 2u : 1u;
  const bool in_range = idx < n_reads;
  return PassRead{in_range, in_range ? idx / nm : 0u, in_range ? idx % nm : 0u};
}

struct TruthJob {
  PieceMap map;
  TruthRow* rows;                // [n_reads]
  uint32_t* rec_len;             // [n_reads] bytes of the record with its block_size word (0: unused slot)
  const uint64_t* rec_off;       // [n_reads] exclusive scan of rec_len
  unsigned long long* counters;  // [0] records, [1] unmapped, [2] flags: 1 a record with more than kTruthMaxOps operations, 2 a wave's records with more than kTruthWaveOps, 4 a record that does not fit the pack kernel's LDS
  uint8_t* out;                  // the record stream
  uint64_t out_bytes;
  uint32_t text_lds;             // bytes of the pack kernel's text stage, image stage (multiples of 16)
  uint32_t image_lds;
};
void launch_truth_size(const DevProfile& P, const DevBatch& B, const TruthJob& J, hipStream_t s);
void launch_truth_pack(const DevProfile& P, const DevBatch& B, const TruthJob& J, hipStream_t s);
// sg_truth_reads: the layout of sg_truth_read (simuscop_amd.h)
struct TruthReadRow {
  uint32_t live, chain, reverse, read_len;
  uint64_t tmpl_off;
  uint32_t n_events, inside;
  uint32_t events[SG_MAX_EVENTS];
};
void launch_truth_reads(const DevProfile& P, const DevBatch& B, uint32_t mate, uint32_t first_slot, uint32_t n, TruthReadRow* out, hipStream_t s);

// ---- true coverage (simuReads --truth-depth; kernels: sg_depth.hip) ----
// One flat int32 difference array: contig c owns slots [off[c], off[c] + len[c] + 1), off[c] a multiple of 4 (16-byte
// loads).  A run [a, b) of M bases adds +1 at a and -1 at b; the depth of base i is the sum of slots 0..i, taken modulo
// 2^32 (so a depth of up to 2^32 - 1 comes out right).
constexpr uint32_t kDepthStageRuns = 8; // M runs of a read depth_add_kernel stages in LDS (a read with more walks twice)
constexpr uint32_t kDepthTile = 4096;   // bases one wave of the finishing pass rebuilds (16 steps of 64 lanes x 4 bases)
struct DepthJob {
  PieceMap map;
  int32_t* diff;
  const uint64_t* contig_off;    // [n_contigs] first slot of each contig
  const uint64_t* contig_len;    // [n_contigs]
  uint32_t n_contigs;
  uint32_t stage_runs;           // <= kDepthStageRuns
  unsigned long long* counters;  // [0] M bases, [1] flags: 1 a run outside its contig (not written), 2 a walk whose runs do not end at its `end`
};
struct DepthRun { uint32_t start, depth; };   // sg_depth_run
// one contig's slots for the finishing pass
struct DepthView {
  const int32_t* diff;   // 16-byte aligned
  uint32_t len, n_tiles;
};
void launch_depth_add(const DevProfile& P, const DevBatch& B, const DepthJob& J, hipStream_t s);
void launch_depth_spans(const DepthJob& J, const uint32_t* contig, const uint64_t* start, const uint64_t* end, uint64_t n, hipStream_t s);
// per tile: the sum of its differences and the number of its run starts (base 0, and every base whose difference is not 0)
void launch_depth_tiles(const DepthView& V, uint32_t* tile_sum, uint32_t* tile_starts, hipStream_t s);
// tile_base: the exclusive scan of tile_sum (its low 32 bits are the depth in front of the tile)
void launch_depth_bins(const DepthView& V, const uint64_t* tile_base, uint32_t bin, unsigned long long* sums, hipStream_t s);
void launch_depth_runs(const DepthView& V, const uint64_t* tile_base, const uint64_t* start_base, DepthRun* rows, uint64_t cap, hipStream_t s);
void launch_depth_fetch(const DepthView& V, const uint64_t* tile_base, uint32_t first, uint32_t n, uint32_t* out, hipStream_t s);

// ---- true allele counts per variant (simuReads --truth-variants; kernel: sg_variants.hip) ----
// One row of the variant table as the scan reads it: 16 bytes, sorted by key.  kind 0 SNV (len unused), 1 insertion of
// `len` bases behind base p, 2 deletion of bases [p, p + len).
struct VariantRow {
  uint64_t key;        // BAM refID << 32 | p (0-based on the contig)
  uint32_t len;
  uint32_t kind_code;  // kind | the allele's base code << 8 (SNV rows)
};
__host__ __device__ inline uint64_t variant_key(uint32_t contig, uint64_t p) { return ((uint64_t)contig << 32) | (p & 0xFFFFFFFFull); }
// the chains' base codes (encode_base, sg_haplotypes.hip) for an allele given as a letter
__host__ __device__ inline uint32_t variant_base_code(uint32_t b) {
  switch (b & 0xDFu) {
    case 'A': return 0u;
    case 'C': return 1u;
    case 'T': return 2u;
    case 'G': return 3u;
    case 'N': return 4u;
    case 'X': return 6u;
    default: return 5u;
  }
}
// first row of [0, n) whose key is not below `key`
__host__ __device__ inline uint64_t variant_lower_bound(const VariantRow* table, uint64_t n, uint64_t key) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (table[mid].key < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The counting rule (DESIGN.md "True allele counts").  The template is `L` chain bases from `tmpl_off` on, `pieces` its
// chain's pieces in offset order ([0, n_pieces) may hold further chains behind it: the walk stops at the template's
// end), `pi` the index of the piece that holds tmpl_off.  `codes[o - codes_off]` is the chain's base code at chain
// offset o; it is read for SNV rows only.  The walk goes piece by piece: every reference piece is clipped to the
// template, the table is searched once for the clipped span [a, b) of its contig, and the rows with p in [a, b] are
// visited -- a base at x can touch the SNV and insertion rows at x and the deletion rows at x + 1 (a deletion is
// anchored on the base in front of it).  Pairs of neighbours inside a piece are reference neighbours; the pair across
// the clipped piece's end is resolved against the next piece that holds a base.  `hit(row, is_alt)` is called once
// per count of `total`.
template <class Hit>
__host__ __device__ inline void truth_variant_scan(const TruthPiece* pieces, uint64_t n_pieces, uint64_t pi, uint64_t tmpl_off, uint32_t L,
                                                   const uint8_t* codes, uint64_t codes_off, const VariantRow* table, uint64_t n_rows,
                                                   Hit hit) {
  if (!n_rows || !L) return;
  const uint64_t t_end = tmpl_off + L;
  for (uint64_t j = pi; j < n_pieces && pieces[j].dst < t_end; j++) {
    const TruthPiece& p = pieces[j];
    if ((p.meta >> 30) & 1u) continue;   // no clause is anchored on a literal base
    const uint64_t ca = p.dst > tmpl_off ? p.dst : tmpl_off, pe = p.dst + p.len, cb = pe < t_end ? pe : t_end;
    if (ca >= cb) continue;
    const uint32_t contig = p.meta & 0x3FFFFFFFu;
    const uint64_t a = p.src + (ca - p.dst), b = a + (cb - ca);
    uint64_t r = variant_lower_bound(table, n_rows, variant_key(contig, a));
    const uint64_t key_end = variant_key(contig, b);
    if (r >= n_rows || table[r].key > key_end) continue;
    // what follows the clipped piece's last base: nothing (the template ends there), a reference base, or a literal
    // piece -- of `nx_len` bases, `nx_whole` when it lies inside the template with one more template base behind it
    bool nx_any = false, nx_lit = false, nx_whole = false;
    uint32_t nx_contig = 0, nx_len = 0;
    uint64_t nx_pos = 0;
    if (cb < t_end) {
      uint64_t q = j + 1;
      while (q < n_pieces && pieces[q].len == 0u) q++;
      if (q < n_pieces && pieces[q].dst == cb) {
        const TruthPiece& nx = pieces[q];
        nx_any = true;
        nx_lit = (nx.meta >> 30) & 1u;
        nx_contig = nx.meta & 0x3FFFFFFFu;
        nx_pos = nx.src;
        nx_len = nx.len;
        nx_whole = nx.dst + nx.len < t_end;
      }
    }
    for (; r < n_rows && table[r].key <= key_end; r++) {
      const VariantRow row = table[r];
      const uint64_t pos = row.key & 0xFFFFFFFFull;
      const uint32_t kind = row.kind_code & 0xFFu;
      if (kind == 0u) {
        if (pos < b) hit(r, (uint32_t)codes[ca + (pos - a) - codes_off] == (row.kind_code >> 8));
      } else if (kind == 1u) {
        if (pos >= b) continue;
        if (pos + 1 < b) hit(r, false);
        else if (nx_any) {
          if (!nx_lit) { if (nx_contig == contig && nx_pos == pos + 1) hit(r, false); }
          else if (nx_whole && nx_len == row.len) hit(r, true);
        }
      } else {
        if (pos <= a) continue;          // anchored on base pos - 1 (a row with p = 0 has none)
        if (pos < b) hit(r, false);
        else if (nx_any && !nx_lit && nx_contig == contig) {
          if (nx_pos == pos) hit(r, false);
          else if (nx_pos == pos + row.len) hit(r, true);
        }
      }
    }
  }
}

struct VariantJob {
  PieceMap map;
  const VariantRow* table;
  uint64_t n_rows;
  uint32_t* counts;              // [n_rows][2]: total, alt
  unsigned long long* counters;  // [0] reads with a hit, [1] hits, [2] flags: 1 a template whose first piece was not found
};
void launch_variants_add(const DevProfile& P, const DevBatch& B, const VariantJob& J, hipStream_t s);


// ---- true error counts per cycle and quality (simuReads --truth-errors; kernel: sg_errors.hip) ----
// One flat table of 64-bit counters (the layout of sg_errtab_counts, simuscop_amd.h), mate 0 / 1:
//   Q [2][cycles][n_qual][4]  bases, errors, other, inserted of read position `cycle` reported with quality qual_lo + q
//   S [2][4][5]               template base (A C T G) -> read letter (A C T G N) of the paired bases
//   I [2][L][2], D [2][L][2]  events, bases of the sequencing insertions behind / deletions at template base j
struct ErrtabDims { uint32_t cycles, qual_lo, n_qual, L; };
enum : uint32_t { kErrBases = 0, kErrErrors = 1, kErrOther = 2, kErrInserted = 3 };
__host__ __device__ inline uint64_t errtab_q(const ErrtabDims& d, uint32_t mate, uint32_t cycle, uint32_t q) {
  return (((uint64_t)mate * d.cycles + cycle) * d.n_qual + q) * 4u;
}
__host__ __device__ inline uint64_t errtab_s(const ErrtabDims& d, uint32_t mate, uint32_t from, uint32_t to) {
  return 8ull * d.cycles * d.n_qual + mate * 20u + from * 5u + to;
}
__host__ __device__ inline uint64_t errtab_indel(const ErrtabDims& d, uint32_t del, uint32_t mate, uint32_t j) {
  return 8ull * d.cycles * d.n_qual + 40u + (uint64_t)del * 4u * d.L + ((uint64_t)mate * d.L + j) * 2u;
}
__host__ __device__ inline uint64_t errtab_cells(const ErrtabDims& d) { return 8ull * d.cycles * d.n_qual + 40u + 8ull * d.L; }

// a chain's base code as the read sees it: complemented for a reverse read (codes of 4 and above are no A/C/G/T)
__host__ __device__ inline uint32_t errtab_tmpl_code(uint32_t code, bool reverse) { return reverse && code < 4u ? code ^ 2u : code; }
// the read's letter as a column of S: A0 C1 T2 G3, anything else (N) 4
__host__ __device__ inline uint32_t errtab_read_code(uint32_t ch) { return ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'T' ? 2u : ch == 'G' ? 3u : 4u; }

// The counting rule (DESIGN.md "True error counts"): how a read's positions lie over its template T'[0 .. L) in read
// direction, given its events (ev_pack form, read direction, ascending).  The walk hands over runs, in read order:
//   seg(0, j, r, n)   read bases r .. r + n - 1 pair with T'[j .. j + n - 1]           (n may be 0)
//   seg(1, j, r, n)   read bases r .. r + n - 1 were inserted behind the base paired with T'[j]
//   seg(2, j, r, n)   T'[j .. j + n - 1] was deleted in front of read base r (n already clipped to L - j)
// and returns the read's length, or kErrWalkBad for events no pass makes: more than SG_MAX_EVENTS, one of length 0, one
// outside the template or in front of where the event before it ends.
constexpr uint32_t kErrWalkBad = 0xFFFFFFFFu;
template <class Seg>
__host__ __device__ inline uint32_t errtab_walk(const uint32_t* events, uint32_t n_events, uint32_t L, Seg seg) {
  if (n_events > SG_MAX_EVENTS) return kErrWalkBad;
  uint32_t j = 0, r = 0;
  for (uint32_t e = 0; e < n_events; e++) {
    const uint32_t w = events[e], je = w & 0xFFFFu, k = (w >> 16) & 0x7FFFu;
    if (je < j || je >= L || k == 0u) return kErrWalkBad;
    if (w >> 31) {
      const uint32_t kc = k < L - je ? k : L - je;
      seg(0u, j, r, je - j);
      r += je - j;
      seg(2u, je, r, kc);
      j = je + kc;
    } else {
      seg(0u, j, r, je - j + 1u);
      r += je - j + 1u;
      seg(1u, je, r, k);
      r += k;
      j = je + 1u;
    }
  }
  seg(0u, j, r, L - j);
  return r + (L - j);
}

struct ErrtabJob {
  ErrtabDims d;
  uint32_t win_cycles;           // cycles one workgroup stages in LDS (a multiple of 64)
  unsigned long long* table;     // [errtab_cells]
  unsigned long long* counters;  // [0] paired A/C/G/T bases, [1] errors among them, [2] reads skipped (live, not inside), [3] reads counted,
                                 // [4] flags: 2 a walk that does not end at the read's length, 4 a read longer than `cycles`,
                                 //            8 a quality outside the range, 16 a record outside its mate's text
};
constexpr uint32_t kErrLdsBudget = 72u * 1024u;   // two workgroups a CU
uint32_t errtab_win_cycles(const ErrtabDims& d);
void launch_errtab_add(const DevProfile& P, const DevBatch& B, const ErrtabJob& J, uint32_t n_cus, hipStream_t s);

// ---- NM, MD and XE tags of the truth BAM records (simuReads --truth-tags; kernels: sg_truth_tags.hip, sg_truth.hip) ----
// The rule (DESIGN.md "Truth tags").  NM and MD are a function of the record's own fields and the reference: POS, the
// operations, SEQ in BAM orientation and the contig's base codes.  XE is the read in FASTQ orientation against its
// template, laid out by errtab_walk.
enum : uint32_t { kTagNM = 1u, kTagMD = 2u, kTagXE = 4u };   // SG_TAG_*
// The longest MD text a record carries.  Without a variant deletion a text has at most 2 * L + 2 * (D runs) + 1 bytes
// (DESIGN.md derives it), and an alignment has at most kTruthMaxOps / 2 D runs: templates of up to kTruthTagMaxL bases
// never reach the cap, and the tagged call refuses longer ones.
constexpr uint32_t kTruthMaxMd = 2048;
constexpr uint32_t kTruthTagMaxL = (kTruthMaxMd - kTruthMaxOps - 1u) / 2u;
constexpr uint32_t kMdDropped = 0xFFFFFFFFu;
// the reference letter of a base code: the codes keep no IUPAC letter, so all but A C T G come out as N
__host__ __device__ inline uint32_t truth_ref_letter(uint32_t code) { return code == 0u ? 'A' : code == 1u ? 'C' : code == 2u ? 'T' : code == 3u ? 'G' : 'N'; }
// a SEQ letter matches iff it is the reference letter and one of A, C, G, T (an N never matches: calmd's rule)
__host__ __device__ inline bool truth_base_matches(uint32_t seq_letter, uint32_t code) { return code < 4u && seq_letter == truth_ref_letter(code); }
// a FASTQ letter as SEQ shows it in a record that is turned round
__host__ __device__ inline uint32_t truth_complement(uint32_t ch) { return ch == 'A' ? 'T' : ch == 'T' ? 'A' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch; }
__host__ __device__ inline uint32_t truth_digits(uint32_t v) {
  uint32_t n = 1;
  while (v >= 10u) { v /= 10u; n++; }
  return n;
}
// digit `i` (0: the leading one) of v, which has n digits
__host__ __device__ inline uint32_t truth_digit(uint32_t v, uint32_t n, uint32_t i) {
  for (uint32_t k = i + 1u; k < n; k++) v /= 10u;
  return '0' + v % 10u;
}
// bytes of a record's tags: `present` says which it gets, md_len is its MD text's length
__host__ __device__ inline uint32_t truth_tag_bytes(uint32_t present, uint32_t md_len) {
  return ((present & kTagNM) ? 7u : 0u) + ((present & kTagXE) ? 7u : 0u) + ((present & kTagMD) ? 3u + md_len + 1u : 0u);
}

struct TagWalk {
  uint32_t nm, md_len;   // md_len counts every byte of the text, written or not
  uint32_t q_end;        // SEQ letters the operations cover
  uint64_t r_end;        // reference bases from POS on they cover
};
// NM and MD of one record, base by base.  `ops` are its operations (len << 4 | op), seq(i) is SEQ letter i in BAM
// orientation, ref(x) the base code x bases behind POS; put(o, ch) gets byte o of the MD text.
template <class Seq, class Ref, class Put>
__host__ __device__ inline TagWalk truth_tags_walk(const uint32_t* ops, uint32_t n_ops, Seq seq, Ref ref, Put put) {
  TagWalk W = {0u, 0u, 0u, 0u};
  uint32_t m = 0;
  auto number = [&]() {
    const uint32_t n = truth_digits(m);
    for (uint32_t i = 0; i < n; i++) put(W.md_len++, truth_digit(m, n, i));
    m = 0;
  };
  for (uint32_t k = 0; k < n_ops; k++) {
    const uint32_t len = ops[k] >> 4, op = ops[k] & 15u;
    if (op == kOpM) {
      for (uint32_t i = 0; i < len; i++) {
        const uint32_t code = ref(W.r_end + i);
        if (truth_base_matches(seq(W.q_end + i), code)) { m++; continue; }
        number();
        put(W.md_len++, truth_ref_letter(code));
        W.nm++;
      }
      W.q_end += len;
      W.r_end += len;
    } else if (op == kOpD) {
      number();
      put(W.md_len++, (uint32_t)'^');
      for (uint32_t i = 0; i < len; i++) put(W.md_len++, truth_ref_letter(ref(W.r_end + i)));
      W.nm += len;
      W.r_end += len;
    } else if (op == kOpN) {
      W.r_end += len;
    } else {   // I, S
      if (op == kOpI) W.nm += len;
      W.q_end += len;
    }
  }
  number();
  return W;
}
// XE of one read: tmpl(j) is the chain's base code of T'[j] as the read sees it (errtab_tmpl_code), read(r) letter r of
// the read in FASTQ orientation.  kErrWalkBad: the events do not end at `np`.
template <class Tmpl, class Read>
__host__ __device__ inline uint32_t truth_xe(const uint32_t* events, uint32_t n_events, uint32_t L, uint32_t np, Tmpl tmpl, Read read) {
  if (errtab_walk(events, n_events, L, [](uint32_t, uint32_t, uint32_t, uint32_t) {}) != np) return kErrWalkBad;
  uint32_t xe = 0;
  errtab_walk(events, n_events, L, [&](uint32_t kind, uint32_t j, uint32_t r, uint32_t n) {
    if (kind != 0u) { xe += n; return; }
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t tc = tmpl(j + i);
      if (tc < 4u && errtab_read_code(read(r + i)) != tc) xe++;
    }
  });
  return xe;
}

// Per read, in record order: what truth_tag_size_kernel found (md_len = kMdDropped: the text is longer than kTruthMaxMd)
struct TagRow { uint32_t nm, xe, md_len; };
// refID -> its contig's codes (the first row of the committed reference with that refID)
struct TagRef { uint64_t code_off, length; };
struct TagJob {
  uint32_t tags;                 // kTag*
  uint32_t n_refs;
  const TagRef* refs;            // [n_refs]
  const uint8_t* ref_codes;
  TagRow* rows;                  // [n_reads]
  unsigned long long* counters;  // [0..2] records with NM, MD, XE, [3] sum of NM, [4] of XE, [5] MD texts dropped, [6] tag bytes,
                                 // [7] flags: 1 a walk that does not end at the read's length, 2 a reference span past its contig's end,
                                 //            4 a record outside its mate's text
};
void launch_truth_tag_size(const DevProfile& P, const DevBatch& B, const TruthJob& J, const TagJob& T, hipStream_t s);
void launch_truth_pack_tags(const DevProfile& P, const DevBatch& B, const TruthJob& J, const TagJob& T, hipStream_t s);

}  // namespace sg
