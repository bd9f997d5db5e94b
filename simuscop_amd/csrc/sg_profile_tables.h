// sg_profile_tables.h -- the tables of a profile as the engine wants them: one array of 32-bit words and the layout that
// says where each table lies in it.  Made on the host by sg_profile_prepare (sg_profile_tables.cpp: no device, any
// thread, no HIP header -- it compiles with a plain C++ compiler next to sg_tables.cpp), uploaded and mapped onto
// sg::DevProfile by sg_load_prepared_profile (sg_api.cpp).  tools/profile_tables_check.cpp prints the words' hash and
// every field below for a list of profiles; tests/test_profile_tables_cpu.py pins its output.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/simuscop_amd.h"

// Offsets are in 32-bit words into the table, every one a multiple of 4 (the kernels read uint2 / uint4 / uint64).
struct SgTableLayout {
  uint64_t sub_off = 0, sub_rows = 0;   // substitution rows [mate][context][bin] x uint4; sub_rows = rows of one mate
  uint64_t alias_off = 0;               // quality rows as alias columns [16][bins][W] x uint2, W = 1 << lgW
  uint64_t ins_off = 0, del_off = 0, isz_off = 0;   // threshold rows [k0, T..] of 1 + (1 << *_lg) words (sg_tables.h)
  uint64_t gap_off = 0;                 // read_length + 1 x uint64: P(no indel candidate in k positions)
  uint64_t fast_lds_off = 0, fast_sub_off = 0, fast_alias_off = 0;   // the straight-line kernel's tables (kmer 3 only, else 0)
  uint32_t lgW = 0, ins_lg = 0, del_lg = 0, isz_lg = 0;
  uint32_t fast_stride = 0;             // words per (mate, bin) of the LDS image: 192 + 4 W
  uint32_t remap = 0, inv_remap = 0;    // natural base code (A0 C1 T2 G3) -> profile code and back, 2 bits each
  uint32_t packed = 0;                  // the profile's four base characters, one byte each
  uint32_t kmer_off[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // first context id of the contexts with m real bases
  uint64_t evA = 0, evB = 0;            // indel candidates per 2^64 positions: insertions, all
  bool has2 = false, has_isz = false;   // a second mate's substitution rows; an insert-size row
  int32_t kmer = 0, bins = 0, read_length = 0, min_qual = 0, isize_min = 0, insert_size = 0, n_isize = 0;   // the profile's own
};

struct sg_profile_tables {
  SgTableLayout L;
  std::vector<uint32_t> tab;
  int rc = SG_OK;
  std::string err;
  int fail(int code, const std::string& msg) { rc = code; err = msg; return code; }
};
