// sg_windows.h -- what the window planner's kernels (sg_windows.hip) share with their host API (sg_api_windows.cpp): the
// device arrays of each entry point as one typed view, filled where the entry point carves its work buffer, and the
// launchers that take them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simuscop_amd.h"

namespace sg {

// n windows: geometry, the address of their GC draw (segment ordinal, ordinal inside the segment), GC%
struct WindowList { sg_gc_window* win; uint32_t* seg_ord; uint32_t* win_ord; int32_t* gc; };
// the generators of a call and the first window of each (prefix[n_gens] = all windows)
struct GenList { sg_window_gen* gens; uint64_t* prefix; uint32_t n_gens; };
// sg_windows_build: seg_first[n_segs + 1] first window of every segment, seg_sum[n_segs] the segments' weights
struct BuildWork { GenList g; uint64_t* seg_first; WindowList w; double* seg_sum; };
// sg_plan_windows: act[n_act], seg_first[n_act + 1], seg_sum[n_act] reads handed out per segment, planned[n] fragments
// per window and off[n] their exclusive scan (bsum, total: the scan's), seg_slots[n_act + 1] fragments before each segment
struct PlanWork {
  GenList g;
  sg_active_seg* act;
  uint32_t *seg_first, *planned;
  unsigned long long* seg_sum;
  uint64_t *off, *bsum, *total, *seg_slots;
};

void launch_gc(const uint8_t* chains, const uint64_t* chain_off, const sg_gc_window* wins, uint64_t n, int32_t* out, hipStream_t s);
// GC% into w.gc, then the weights; `m`: the model with means / quantiles on the device
void launch_weights(const uint8_t* chains, const uint64_t* chain_off, const WindowList& w, uint64_t n, const sg_gc_model& m, uint64_t seed,
                    double* out, hipStream_t s);
void launch_tile(const BuildWork& b, uint64_t n, uint32_t frag, hipStream_t s);
void launch_seg_sum(const double* wt, const uint64_t* seg_first, uint32_t n_segs, double* out, hipStream_t s);
// the batch table from the stored weights `wt`: reads per window, the remainder rule, planned fragments, their scan, slot
// bases into the rows and p.seg_slots
void launch_plan_rows(const PlanWork& p, uint64_t n, uint32_t frag, const double* wt, uint32_t n_act, sg_window* rows, int32_t paired,
                      hipStream_t s);
void launch_slice(const sg_window* all, uint64_t w_lo, uint64_t n, uint32_t a0, uint32_t slot_lo, sg_window* out, hipStream_t s);

}  // namespace sg
