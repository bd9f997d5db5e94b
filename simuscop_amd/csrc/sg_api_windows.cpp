// sg_api_windows.cpp -- the window planner of the C ABI (include/simuscop_amd.h: sg_gc_percent, sg_window_weights,
// sg_windows_build / sg_windows_drop, sg_plan_windows / sg_plan_range) on the kernels of sg_windows.hip.  Its state is
// sg_ctx::Windows (sg_api.h).
#include <cstring>

#include "sg_api.h"
#include "sg_scan.h"
#include "sg_windows.h"

namespace {

int bad(sg_ctx* ctx, const char* who, const std::string& what) { return ctx->fail(SG_ERR_INVALID, std::string(who) + ": " + what); }

int check_model(sg_ctx* ctx, const sg_gc_model* m, const char* who) { return m->lg_cells < 1 || m->lg_cells > 20 || !m->frag_size ? bad(ctx, who, "bad model") : SG_OK; }
// means[101] and the quantile knots behind them into Windows::model; *dev: the model with both pointers on the device
int upload_model(sg_ctx* ctx, const sg_gc_model* m, sg_gc_model* dev) {
  const size_t cells = (size_t)1 << m->lg_cells;
  SG_ENSURE(ctx->win.model, (101 + cells + 1) * 8);
  double* d = ctx->win.model.as<double>();
  SG_HIP(hipMemcpyAsync(d, m->means, 101 * 8, hipMemcpyHostToDevice, ctx->stream));
  SG_HIP(hipMemcpyAsync(d + 101, m->quantiles, (cells + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  *dev = {d, m->std, d + 101, m->lg_cells, m->frag_size, m->full_tile_form, m->ctx24};
  return SG_OK;
}
int check_windows(sg_ctx* ctx, const sg_gc_window* windows, uint64_t n, const char* who) {
  for (uint64_t w = 0; w < n; w++) {
    if (windows[w].chain >= ctx->hap.len.size()) return bad(ctx, who, "chain out of range");
    if (windows[w].start + windows[w].len > ctx->hap.len[windows[w].chain]) return bad(ctx, who, "window runs past its chain");
  }
  return SG_OK;
}
// prefix[g]: first window of generator g, [n_gens] all windows
int check_gens(sg_ctx* ctx, const sg_window_gen* gens, uint64_t n_gens, uint32_t n_segs, uint32_t frag, std::vector<uint64_t>& prefix,
               const char* who) {
  prefix.assign(n_gens + 1, 0);
  for (uint64_t g = 0; g < n_gens; g++) {
    const sg_window_gen& G = gens[g];
    if (G.chain >= ctx->hap.len.size() || G.hap_len == 0 || G.hap_base + G.hap_len > ctx->hap.len[G.chain])
      return bad(ctx, who, "generator " + std::to_string(g) + " does not lie inside its chain");
    if (G.seg >= n_segs || (g && G.seg < gens[g - 1].seg)) return bad(ctx, who, "generators must be ordered by segment");
    prefix[g + 1] = prefix[g] + (G.hap_len + frag - 1) / frag;
  }
  return SG_OK;
}
// first window of every segment, [n_segs] all windows (u64 for tile_kernel / seg_sum_kernel, u32 for the plan's kernels)
template <class T>
std::vector<T> seg_first_of(const sg_window_gen* gens, uint64_t n_gens, uint32_t n_segs, const std::vector<uint64_t>& prefix) {
  std::vector<T> first((size_t)n_segs + 1, (T)prefix[n_gens]);
  uint32_t k = 0;
  for (uint64_t g = 0; g < n_gens; g++)
    for (; k <= gens[g].seg; k++) first[k] = (T)prefix[g];
  return first;
}
sg::GenList take_gens(SgArena& a, uint64_t n_gens) { return {a.take<sg_window_gen>(n_gens), a.take<uint64_t>(n_gens + 1), (uint32_t)n_gens}; }
int upload_gens(sg_ctx* ctx, const sg::GenList& g, const sg_window_gen* gens, const std::vector<uint64_t>& prefix) {
  SG_HIP(hipMemcpyAsync(g.gens, gens, g.n_gens * sizeof(sg_window_gen), hipMemcpyHostToDevice, ctx->stream));
  SG_HIP(hipMemcpyAsync(g.prefix, prefix.data(), ((size_t)g.n_gens + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  return SG_OK;
}
sg::WindowList take_windows(SgArena& a, uint64_t n) {   // (a braced list is evaluated left to right)
  return {a.take<sg_gc_window>(n), a.take<uint32_t>(n), a.take<uint32_t>(n), a.take<int32_t>(n)};
}

}  // namespace

extern "C" {

int sg_gc_percent(sg_ctx* ctx, const sg_gc_window* windows, uint64_t n, int32_t* gc_out) {
  if (!ctx || (n && (!windows || !gc_out))) return SG_ERR_INVALID;
  if (!ctx->have_haps) return ctx->fail(SG_ERR_INVALID, "sg_gc_percent: call sg_upload_haplotypes first");
  if (!n) return SG_OK;
  SG_HIP(hipSetDevice(ctx->device));
  if (int rc = check_windows(ctx, windows, n, "sg_gc_percent")) return rc;
  sg::WindowList w{};
  if (int rc = sg_carve(ctx, ctx->win.gc, [&](SgArena& a) { w.win = a.take<sg_gc_window>(n); w.gc = a.take<int32_t>(n); })) return rc;
  SG_HIP(hipMemcpyAsync(w.win, windows, n * sizeof(sg_gc_window), hipMemcpyHostToDevice, ctx->stream));
  sg::launch_gc(ctx->B.chains, ctx->B.chain_off, w.win, n, w.gc, ctx->stream);
  return sg_read_back(ctx, gc_out, w.gc, n * 4);
}

int sg_window_weights(sg_ctx* ctx, const sg_gc_window* windows, const uint32_t* seg_ord, const uint32_t* win_ord, uint64_t n,
                      const sg_gc_model* model, double* weights_out, int32_t* gc_out) {
  if (!ctx || !model || !model->means || !model->quantiles || (n && (!windows || !seg_ord || !win_ord))) return SG_ERR_INVALID;
  if (int rc = check_model(ctx, model, "sg_window_weights")) return rc;
  if (!ctx->have_haps) return ctx->fail(SG_ERR_INVALID, "sg_window_weights: call sg_upload_haplotypes first");
  if (!n) return SG_OK;
  SG_HIP(hipSetDevice(ctx->device));
  if (int rc = check_windows(ctx, windows, n, "sg_window_weights")) return rc;
  sg::WindowList w{};
  double* wt = nullptr;
  if (int rc = sg_carve(ctx, ctx->win.gc, [&](SgArena& a) { w = take_windows(a, n); wt = a.take<double>(n); })) return rc;
  hipStream_t s = ctx->stream;
  SG_HIP(hipMemcpyAsync(w.win, windows, n * sizeof(sg_gc_window), hipMemcpyHostToDevice, s));
  SG_HIP(hipMemcpyAsync(w.seg_ord, seg_ord, n * 4, hipMemcpyHostToDevice, s));
  SG_HIP(hipMemcpyAsync(w.win_ord, win_ord, n * 4, hipMemcpyHostToDevice, s));
  sg_gc_model dm;
  if (int rc = upload_model(ctx, model, &dm)) return rc;
  sg::launch_weights(ctx->B.chains, ctx->B.chain_off, w, n, dm, ctx->seed, wt, s);
  SG_HIP(hipGetLastError());
  if (weights_out) SG_HIP(hipMemcpyAsync(weights_out, wt, n * 8, hipMemcpyDeviceToHost, s));
  if (gc_out) SG_HIP(hipMemcpyAsync(gc_out, w.gc, n * 4, hipMemcpyDeviceToHost, s));
  SG_HIP(hipStreamSynchronize(s));
  return SG_OK;
}

// ------------------------------------------------------------------------------------------------
// sampling plan made on the device
// ------------------------------------------------------------------------------------------------
int sg_windows_build(sg_ctx* ctx, uint32_t store_id, const sg_window_gen* gens, uint64_t n_gens, uint32_t n_segs, const sg_gc_model* model,
                     double* seg_weight_out, uint64_t* n_windows_out) {
  if (!ctx || !model || !model->means || !model->quantiles || (n_gens && !gens) || (n_segs && !seg_weight_out)) return SG_ERR_INVALID;
  if (int rc = check_model(ctx, model, "sg_windows_build")) return rc;
  if (!ctx->have_haps) return ctx->fail(SG_ERR_INVALID, "sg_windows_build: call sg_upload_haplotypes / sg_build_haplotypes first");
  SG_HIP(hipSetDevice(ctx->device));
  std::vector<uint64_t> prefix;
  if (int rc = check_gens(ctx, gens, n_gens, n_segs, model->frag_size, prefix, "sg_windows_build")) return rc;
  const uint64_t n = prefix[n_gens];
  const std::vector<uint64_t> seg_first = seg_first_of<uint64_t>(gens, n_gens, n_segs, prefix);
  if (n_windows_out) *n_windows_out = n;
  for (uint32_t k = 0; k < n_segs; k++) seg_weight_out[k] = 0.0;
  sg_ctx::Windows::Store& store = ctx->win.stores[store_id];
  store.n = n;
  if (!n) return SG_OK;
  SG_ENSURE(store.weights, n * 8);
  sg::BuildWork b{};
  auto carve = [&](SgArena& a) { b = {take_gens(a, n_gens), a.take<uint64_t>((size_t)n_segs + 1), take_windows(a, n), a.take<double>(n_segs)}; };
  if (int rc = sg_carve(ctx, ctx->win.work, carve)) return rc;
  if (int rc = upload_gens(ctx, b.g, gens, prefix)) return rc;
  SG_HIP(hipMemcpyAsync(b.seg_first, seg_first.data(), ((size_t)n_segs + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  sg_gc_model dm;
  if (int rc = upload_model(ctx, model, &dm)) return rc;
  sg::launch_tile(b, n, model->frag_size, ctx->stream);
  sg::launch_weights(ctx->B.chains, ctx->B.chain_off, b.w, n, dm, ctx->seed, store.weights.as<double>(), ctx->stream);
  sg::launch_seg_sum(store.weights.as<double>(), b.seg_first, n_segs, b.seg_sum, ctx->stream);
  return sg_read_back(ctx, seg_weight_out, b.seg_sum, (size_t)n_segs * 8);
}

void sg_windows_drop(sg_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  ctx->win.stores.clear();
}

int sg_plan_windows(sg_ctx* ctx, uint32_t store_id, const sg_window_gen* gens, uint64_t n_gens, const sg_active_seg* active, uint32_t n_active,
                    uint32_t frag_size, uint32_t batch_id, int32_t paired, const char* name_prefix, uint64_t* slots_out,
                    uint64_t* n_windows_out) {
  if (!ctx || (n_gens && !gens) || (n_active && (!active || !slots_out)) || frag_size == 0) return SG_ERR_INVALID;
  const char* who = "sg_plan_windows";
  if (!ctx->have_profile) return bad(ctx, who, "call sg_load_profile first");
  if (!ctx->have_haps) return bad(ctx, who, "no haplotypes on the device");
  if (batch_id > 0xFFFF) return bad(ctx, who, "batch_id must fit 16 bits");
  const size_t plen = name_prefix ? strlen(name_prefix) : 0;
  if (plen == 0 || plen > 990) return bad(ctx, who, "bad name_prefix (1..990 bytes)");
  auto it = ctx->win.stores.find(store_id);
  if (it == ctx->win.stores.end()) return bad(ctx, who, "no window weights under this store id (sg_windows_build)");
  SG_HIP(hipSetDevice(ctx->device));
  std::vector<uint64_t> prefix;
  if (int rc = check_gens(ctx, gens, n_gens, n_active, frag_size, prefix, who)) return rc;
  const uint64_t n = prefix[n_gens];
  if (n > 0xFFFFFFF0ull) return bad(ctx, who, "more than 2^32 windows in one batch");
  for (uint64_t g = 0; g < n_gens; g++)
    if (gens[g].first_window + (prefix[g + 1] - prefix[g]) > it->second.n)
      return bad(ctx, who, "generator " + std::to_string(g) + " points past the stored weights");
  sg_ctx::Windows::PlanInfo& pi = ctx->win.info;
  pi = sg_ctx::Windows::PlanInfo();
  pi.seg_first = seg_first_of<uint32_t>(gens, n_gens, n_active, prefix);
  for (uint32_t a = 0; a < n_active; a++) {
    if (active[a].seg_size == 0) return bad(ctx, who, "seg_size 0");
    if (pi.seg_first[a] == pi.seg_first[a + 1]) return bad(ctx, who, "active segment without windows");
    pi.seg_size.push_back(active[a].seg_size);
  }
  if (n_windows_out) *n_windows_out = n;
  pi.n_active = n_active; pi.batch_id = batch_id; pi.paired = paired ? 1 : 0; pi.prefix = name_prefix;
  pi.slot_first.assign((size_t)n_active + 1, 0);
  if (n) {
    sg::PlanWork p{};
    auto carve = [&](SgArena& a) {
      p.g = take_gens(a, n_gens), p.act = a.take<sg_active_seg>(n_active), p.seg_first = a.take<uint32_t>((size_t)n_active + 1);
      p.seg_sum = a.take<unsigned long long>(n_active), p.planned = a.take<uint32_t>(n), p.off = a.take<uint64_t>(n);
      p.bsum = a.take<uint64_t>((size_t)sg::scan_blocks((uint32_t)n) + 8), p.total = a.take<uint64_t>(1), p.seg_slots = a.take<uint64_t>((size_t)n_active + 1);
    };
    if (int rc = sg_carve(ctx, ctx->win.work, carve)) return rc;
    SG_ENSURE(ctx->win.plan, n * sizeof(sg_window));
      if (int rc = upload_gens(ctx, p.g, gens, prefix)) return rc;
    SG_HIP(hipMemcpyAsync(p.act, active, (size_t)n_active * sizeof(sg_active_seg), hipMemcpyHostToDevice, ctx->stream));
    SG_HIP(hipMemcpyAsync(p.seg_first, pi.seg_first.data(), ((size_t)n_active + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    SG_HIP(hipMemsetAsync(p.seg_sum, 0, (size_t)n_active * 8, ctx->stream));
    sg::launch_plan_rows(p, n, frag_size, it->second.weights.as<double>(), n_active, ctx->win.plan.as<sg_window>(), paired, ctx->stream);
    if (int rc = sg_read_back(ctx, pi.slot_first.data(), p.seg_slots, ((size_t)n_active + 1) * 8)) return rc;
    if (pi.slot_first[n_active] > 0xFFFFFFF0ull) return bad(ctx, who, "more than 2^32 fragments in one batch");
  }
  for (uint32_t a = 0; a < n_active; a++) slots_out[a] = pi.slot_first[a + 1] - pi.slot_first[a];
  pi.valid = true;
  // a batch planned from the table this one replaces is not sampled any more; a pass already sampled keeps its rows
  // (ctx->windows is untouched until sg_plan_range)
  if (ctx->pass.stage == sg_ctx::Pass::Planned) ctx->pass = sg_ctx::Pass();
  return SG_OK;
}

int sg_plan_range(sg_ctx* ctx, uint32_t a0, uint32_t a1) {
  if (!ctx) return SG_ERR_INVALID;
  const sg_ctx::Windows::PlanInfo& pi = ctx->win.info;
  if (!pi.valid) return ctx->fail(SG_ERR_INVALID, "sg_plan_range: call sg_plan_windows first");
  if (a0 >= a1 || a1 > pi.n_active) return ctx->fail(SG_ERR_INVALID, "sg_plan_range: empty or out-of-range run of segments");
  SG_HIP(hipSetDevice(ctx->device));
  const uint32_t w_lo = pi.seg_first[a0], w_hi = pi.seg_first[a1], n_segs = a1 - a0;
  const uint64_t nw = (uint64_t)w_hi - w_lo;
  const uint64_t slot_lo = pi.slot_first[a0], slots = pi.slot_first[a1] - slot_lo;
  SG_ENSURE(ctx->windows, (nw + 1) * sizeof(sg_window));
  SG_ENSURE(ctx->segmeta, ((size_t)n_segs * 2 + 2) * 4);
  std::vector<uint32_t> segmeta;
  for (uint32_t a = a0; a < a1; a++) segmeta.push_back(pi.seg_size[a]);
  for (uint32_t a = a0; a <= a1; a++) segmeta.push_back(pi.seg_first[a] - w_lo);
  SG_HIP(hipMemcpyAsync(ctx->segmeta.p, segmeta.data(), segmeta.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  sg::launch_slice(ctx->win.plan.as<sg_window>(), w_lo, nw, a0, (uint32_t)slot_lo, ctx->windows.as<sg_window>(), ctx->stream);
  SG_HIP(hipGetLastError());
  return finish_plan(ctx, nw, n_segs, (uint32_t)slots, pi.batch_id, w_lo, (uint32_t)slot_lo, pi.paired, pi.prefix.c_str());
}

}  // extern "C"
