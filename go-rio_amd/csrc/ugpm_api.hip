// ugpm_api.hip -- host side of the UGPM C ABI (include/gorio_ugpm.h): the per-thread device context, the workspace, and the kernel
// sequencing of ugpm_kernels.hip as a sequence of named steps.  The window bookkeeping (state time line, sample slicing:
// preint.h:766-811) is ugpm_windows.h.  No numerics happen on the host and there is no CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <atomic>
#include <vector>

#include "../../include/gorio_ugpm.h"
#include "dev_buffer.h"
#include "ugpm_kernels.hip"
#include "ugpm_lpm_out.hip"
#include "ugpm_chunks.h"
#include "ugpm_windows.h"

using namespace gorio;
using namespace gorio::windows;

namespace {

#ifndef GORIO_EVAL_SPLIT
#define GORIO_EVAL_SPLIT 12  // measured in round 3 (6 / 12 / 24): LM fits of a C4 batch alone 3.10 / 2.98 / 3.00 ms
#endif
constexpr int kEvalSplit = GORIO_EVAL_SPLIT;  // workgroups per window in the residual / Jacobian evaluators

thread_local std::string g_err;
thread_local double g_stage_s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
thread_local int g_stage_n[8] = {0, 0, 0, 0, 0, 0, 0, 0};
std::atomic<int> g_speculative_rot{1};  // gorio_ugpm_debug_set_schedule
std::atomic<int> g_debug_path{0};       // gorio_ugpm_debug_set_path

int ufail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define UHIP(expr)                                                                                              \
  do {                                                                                                          \
    hipError_t e_ = (expr);                                                                                     \
    if (e_ != hipSuccess) return ufail(GORIO_UGPM_ERR_NO_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

struct StreamPair {  // a main stream, the stream of the state-correlation chain beside it, and the two events that order them
  hipStream_t s = nullptr, s2 = nullptr;
  hipEvent_t ev_jac = nullptr, ev_corr = nullptr;
};

// highest priority when the device has a range: these are many small latency-bound launches that should not queue behind the scan matcher's large grids
int make_stream_pair(StreamPair& p) {
  int lo = 0, hi = 0;
  if (!(hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hipStreamCreateWithPriority(&p.s, hipStreamNonBlocking, hi) == hipSuccess))
    UHIP(hipStreamCreateWithFlags(&p.s, hipStreamNonBlocking));
  UHIP(hipStreamCreateWithFlags(&p.s2, hipStreamNonBlocking));
  UHIP(hipEventCreateWithFlags(&p.ev_jac, hipEventDisableTiming));
  UHIP(hipEventCreateWithFlags(&p.ev_corr, hipEventDisableTiming));
  return 0;
}

void destroy_stream_pair(StreamPair& p) {
  if (p.s) hipStreamDestroy(p.s);
  if (p.s2) hipStreamDestroy(p.s2);
  if (p.ev_jac) hipEventDestroy(p.ev_jac);
  if (p.ev_corr) hipEventDestroy(p.ev_corr);
  p = StreamPair();
}

struct Ctx {  // per-thread, per-device cached streams and buffers; every buffer frees itself (dev_buffer.h)
  int device = -1;
  StreamPair main;  // s2: the state-correlation chain runs here, beside the two GP fits (a helper thread in the reference, preint.h:939-1064)
  hipEvent_t ev_up = nullptr;
  struct Group : StreamPair { hipEvent_t ev_done = nullptr, ev_tab = nullptr; };
  std::vector<Group> groups;  // group 0 borrows the main pair
  DevBuf<double> ws;
  DevBuf<UgpmWin> d_wins;  // d_wins, d_ints (kWinInts per window: lmi[16], status) and d_diag (4 per window): one group of capacity wins_cap
  DevBuf<int> d_ints;
  DevBuf<double> d_diag;
  size_t wins_cap = 0;
  int lm_budget[2] = {0, 0};  // iterations the two fits of the PREVIOUS batch needed: that many are enqueued, without a look at the done flags (run_fit)
  PinnedBuf pin_in;  // pinned staging of the batch's input arrays (the H2D copy is then a DMA the call does not wait for)
  PinnedBuf pin_out;  // where the results land: records, diagnostics, control words (a download into pageable memory is staged by the runtime)
  DevBuf<double> lpm_ws;  // opt.type = LPM windows (ugpm_lpm_out.hip)
  DevBuf<int> lpm_ints;
  DevBuf<ug::LpmOutWin> d_lpm_wins;
  struct StageEvents { hipEvent_t a, b; int stage; };
  std::vector<StageEvents> ev;  // of the batch in flight (Stage); drop_stage_events ends them

  void drop_stage_events() {
    for (auto& e : ev) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
    ev.clear();
  }
  // back to the empty state, on the context's own device (a half-made context has none yet); results ignored: a thread_local context
  // may die while the HIP runtime is already shutting down
  void reset() {
    if (device >= 0) hipSetDevice(device);
    for (size_t g = 1; g < groups.size(); ++g) destroy_stream_pair(groups[g]);
    for (Group& g : groups) { hipEventDestroy(g.ev_done); hipEventDestroy(g.ev_tab); }
    groups.clear();
    destroy_stream_pair(main);
    if (ev_up) hipEventDestroy(ev_up);
    ev_up = nullptr;
    drop_stage_events();
    ws.reset(); d_wins.reset(); d_ints.reset(); d_diag.reset(); pin_in.reset(); pin_out.reset(); lpm_ws.reset(); lpm_ints.reset(); d_lpm_wins.reset();
    wins_cap = 0;
    lm_budget[0] = lm_budget[1] = 0;
    device = -1;
  }
  ~Ctx() { reset(); }
};
thread_local Ctx g_ctx;

struct Stage {  // HIP events around a group of launches on `stream` (default: the context's main stream); may nest
  Ctx& c;
  hipStream_t stream;
  size_t slot = 0;
  bool on = false;
  Stage(Ctx& c_, int s, hipStream_t st = nullptr) : c(c_), stream(st ? st : c_.main.s) {
    hipEvent_t a = nullptr, b = nullptr;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
    slot = c.ev.size();
    c.ev.push_back({a, b, s});
    hipEventRecord(a, stream);
    on = true;
  }
  ~Stage() {
    if (on) hipEventRecord(c.ev[slot].b, stream);
  }
};
struct StageEventsGuard {  // of one batch: however the call returns, no stage event stays behind for the next call to count
  Ctx& c;
  ~StageEventsGuard() { c.drop_stage_events(); }
};

struct Run : Ctx::Group {  // the windows [g0, g0 + nw) of the batch on one group's streams
  int g0 = 0, nw = 0;
  const UgpmWin* wins = nullptr;  // d_wins + g0
  bool active = true;
};

struct Batch {  // what the steps of one preint_batch_flat call share; the host vectors outlive every asynchronous copy out of them
  const gorio_ugpm_window* windows;
  int nw;
  std::vector<HostWin> hw;
  std::vector<UgpmWin> dw;
  std::vector<int> ints, flags, lpm_ints_h;
  std::vector<double> lpm_in;
  std::vector<ug::LpmOutWin> lw;
  std::vector<size_t> out_offs;
  std::vector<Run> runs;
  size_t total_doubles = 0, total_in = 0, total_out = 0;
  double* out_region = nullptr;  // the input region is the start of the workspace, the output region follows it
  int max_S = 0, max_G = 2, max_V = 2, max_infer = 0, n_lpm = 0;
  bool rerun = false;             // this batch is the unfinished windows of another one
  bool looks = false;             // every fit looks at the done flags (a re-run, or gorio_ugpm_debug_set_path bit 1)
  bool enqueued_blind[2] = {false, false};  // fit p got the budgeted iterations and no look: collect() sorts out who finished
  std::vector<int> final_status;  // per window, once collect() and the re-run are through
  int first_error = 0;
  std::string first_error_msg;
  void note_error(int i, int code, const std::string& m) {
    if (first_error) return;
    first_error = code;
    first_error_msg = "window " + std::to_string(i) + ": " + m;
  }
};

// the thread's context, made this device's: a context of another device is reset first, and it becomes this device's only once it is complete
int ensure_context(Ctx& c, int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ufail(GORIO_UGPM_ERR_NO_DEVICE, "no usable HIP device (no CPU fallback exists)");
  if (device < 0 || device >= ndev) return ufail(GORIO_UGPM_ERR_INVALID, "bad device ordinal");
  if (c.device != device) c.reset();
  UHIP(hipSetDevice(device));
  if (c.device == device) return 0;
  if (int rc = make_stream_pair(c.main)) return rc;
  // ata_kernel stages J through up to ~128 KB of dynamic LDS (the default limit is 64 KB)
  UHIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ug::corr_diag_kernel<kSolveKmaxSmall>), hipFuncAttributeMaxDynamicSharedMemorySize, 140 * 1024));
  UHIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ug::corr_diag_kernel<kSolveKmaxFull>), hipFuncAttributeMaxDynamicSharedMemorySize, 140 * 1024));
  UHIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ug::infer_kernel<kSolveKmaxSmall>), hipFuncAttributeMaxDynamicSharedMemorySize, 17 * (6 * 160 + 16) * 8));
  UHIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ug::infer_kernel<kSolveKmaxFull>), hipFuncAttributeMaxDynamicSharedMemorySize, 17 * (6 * 160 + 16) * 8) /* S = 160: with the 31 KB of static LDS this is just inside the 160 KB of a CU */);
  const void* fns[] = {reinterpret_cast<const void*>(&ug::ata_kernel<4, 16, kAtaTilesCorr>), reinterpret_cast<const void*>(&ug::ata_kernel<8, 16, kAtaTilesCorr>),
                       reinterpret_cast<const void*>(&ug::ata_kernel<16, 8, kAtaTilesCorr>), reinterpret_cast<const void*>(&ug::ata_kernel<4, 16, kAtaTilesLm>),
                       reinterpret_cast<const void*>(&ug::ata_kernel<8, 16, kAtaTilesLm>)};
  for (const void* f : fns) UHIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024));
  c.device = device;
  return 0;
}

// ---- host bookkeeping per window (ugpm_windows.h) and the sizes of the batch
void plan_windows(Batch& b) {
  b.hw.resize(b.nw);
  int total_infer = 0;
  for (int i = 0; i < b.nw; ++i) {
    const gorio_ugpm_window& w = b.windows[i];
    HostWin& h = b.hw[i];
    total_infer += std::max(0, w.n_infer);
    b.max_infer = std::max(b.max_infer, w.n_infer);
    std::string err;
    if (plan_window(w, h, err) != 0) {
      b.note_error(i, h.status, err);
    } else if (h.is_lpm) {
      b.n_lpm++;
    } else {
      b.max_S = std::max(b.max_S, h.S);
      b.total_in += input_slot(w, h);
      b.total_doubles += h.ws_doubles;
    }
  }
  for (const HostWin& h : b.hw) {  // refused windows included, as their slices stand
    b.max_G = std::max(b.max_G, h.is_lpm ? 2 : h.G);
    b.max_V = std::max(b.max_V, h.is_lpm ? 2 : h.V);
  }
  b.total_out = (size_t)total_infer * 83;
  b.total_doubles += b.total_in + b.total_out + 64;
}

int reserve_workspace(Ctx& c, const Batch& b) {
  const size_t nw = b.nw;
  UHIP(c.ws.reserve(b.total_doubles));
  UHIP(reserve_group(c.wins_cap, nw, nw, c.d_wins, nw, c.d_ints, kWinInts * nw, c.d_diag, 4 * nw));
  UHIP(c.pin_in.reserve(sizeof(double) * b.total_in, sizeof(double) * (b.total_in + b.total_in / 4 + 64)));
  const size_t down = sizeof(double) * (b.total_out + 4 * nw) + sizeof(int) * kWinInts * nw;
  UHIP(c.pin_out.reserve(down, down + down / 4 + 64));
  return 0;
}

// ---- carve the workspace, stage the inputs, and enqueue the three uploads
int stage_and_upload(Ctx& c, Batch& b) {
  b.dw.resize(b.nw);
  b.ints.assign(kWinInts * (size_t)b.nw, 0);
  b.out_offs.assign(b.nw, 0);
  double* const in_region = c.ws.get();
  b.out_region = in_region + b.total_in;
  double* base = b.out_region + (b.total_out + 31) / 32 * 32;
  double* const stage_in = static_cast<double*>(c.pin_in.get());  // every use of it ends before this call returns (the call ends with a stream synchronisation)
  size_t in_off = 0, out_off = 0;
  for (int i = 0; i < b.nw; ++i) {
    const gorio_ugpm_window& w = b.windows[i];
    const HostWin& h = b.hw[i];
    UgpmWin& u = b.dw[i];
    std::memset(&u, 0, sizeof(u));
    u.lmi = c.d_ints + kWinInts * (size_t)i;
    u.status = c.d_ints + kWinInts * (size_t)i + 16;
    b.ints[kWinInts * (size_t)i + 16] = h.status;
    u.n_infer = std::max(0, w.n_infer);
    b.out_offs[i] = out_off;
    u.out = b.out_region + out_off;
    out_off += (size_t)u.n_infer * 83;
    if (h.status != 0) continue;
    if (h.is_lpm) {
      b.ints[kWinInts * (size_t)i + 16] = 1;  // every UGPM kernel skips this window; its own status word is slot 17
      u.n_infer = 0;                          // and infer_kernel writes nothing for it
      continue;
    }
    carve(w, h, u, base, in_region + in_off, u.out);
    u.G = h.G; u.V = h.V; u.S = h.S;
    u.correlate = w.correlate ? 1 : 0; u.overlap = w.overlap;
    u.state_freq = h.state_freq;
    copy_noise_and_priors(w, u);
    base += h.ws_doubles;
    double* s = stage_in + in_off;
    const size_t padded = input_slot(w, h);
    for (size_t k = padded - 4; k < padded; ++k) s[k] = 0.0;  // the padding of this window's slot (filled below up to input_doubles)
    s = stage_samples(s, w, h.g0, h.G, h.v0, h.V);
    std::copy(h.state_t.begin(), h.state_t.end(), s);
    in_off += padded;
  }
  // no synchronisation behind these: the staging vectors outlive every use of them (they belong to the Batch of this call, which ends with a
  // stream synchronisation), and the kernels are ordered behind the copies on the same stream
  if (b.total_in) UHIP(hipMemcpyAsync(in_region, stage_in, sizeof(double) * b.total_in, hipMemcpyHostToDevice, c.main.s));
  UHIP(hipMemcpyAsync(c.d_wins, b.dw.data(), sizeof(UgpmWin) * b.nw, hipMemcpyHostToDevice, c.main.s));
  UHIP(hipMemcpyAsync(c.d_ints, b.ints.data(), sizeof(int) * b.ints.size(), hipMemcpyHostToDevice, c.main.s));
  UHIP(hipMemsetAsync(c.d_diag, 0, sizeof(double) * 4 * b.nw, c.main.s));  // windows no solver touches report zero iterations
  return 0;
}

// ---- opt.type = LPM windows: their own workspace and three launches (ugpm_lpm_out.hip)
int run_lpm_windows(Ctx& c, Batch& b) {
  if (b.n_lpm == 0) return 0;
  std::vector<LpmHost> lh(b.n_lpm);
  std::vector<int> widx;
  size_t dbl = 0, in_dbl = 0, nint = 0;
  int max_T = 2;
  for (int i = 0; i < b.nw; ++i) {
    if (!b.hw[i].is_lpm || b.hw[i].status != 0) continue;
    LpmHost& L = lh[widx.size()];
    build_lpm_timeline(b.windows[i], L);
    widx.push_back(i);
    max_T = std::max(max_T, (int)L.tl.size());
    ug::LpmOutWin dummy;
    const LpmSize sz = carve_lpm(b.windows[i], L.tl.size(), dummy, nullptr, nullptr, nullptr);
    in_dbl += sz.in;
    dbl += sz.scratch + 8;
    nint += sz.ints;
  }
  UHIP(c.lpm_ws.reserve(in_dbl + dbl));
  UHIP(c.lpm_ints.reserve(nint));
  UHIP(c.d_lpm_wins.reserve(b.n_lpm));
  b.lw.resize(widx.size());
  b.lpm_in.assign(in_dbl, 0.0);
  b.lpm_ints_h.assign(nint, 0);
  LpmSize at;  // inputs of all LPM windows at the start of lpm_ws (one upload), their scratch behind them
  for (size_t k = 0; k < widx.size(); ++k) {
    const int i = widx[k];
    const gorio_ugpm_window& w = b.windows[i];
    const LpmHost& L = lh[k];
    ug::LpmOutWin& u = b.lw[k];
    std::memset(&u, 0, sizeof(u));
    const LpmSize sz = carve_lpm(w, L.tl.size(), u, c.lpm_ws.get() + at.in, c.lpm_ws.get() + in_dbl + at.scratch, c.lpm_ints.get() + at.ints);
    std::copy(L.tl.begin(), L.tl.end(), stage_samples(b.lpm_in.data() + at.in, w, 0, w.n_gyr, 0, w.n_vel));
    stage_lpm_tables(b.lpm_ints_h.data() + at.ints, L);
    at.in += sz.in; at.scratch += sz.scratch; at.ints += sz.ints;
    u.G = w.n_gyr; u.V = w.n_vel; u.T = (int)L.tl.size(); u.n_infer = w.n_infer;
    u.start_index = L.start_index; u.dt_index = L.dt_index;
    copy_noise_and_priors(w, u);
    u.out = b.dw[i].out;
    u.status = c.d_ints + kWinInts * (size_t)i + 17;
  }
  UHIP(hipMemcpyAsync(c.lpm_ws, b.lpm_in.data(), sizeof(double) * in_dbl, hipMemcpyHostToDevice, c.main.s));
  UHIP(hipMemcpyAsync(c.lpm_ints, b.lpm_ints_h.data(), sizeof(int) * nint, hipMemcpyHostToDevice, c.main.s));
  UHIP(hipMemcpyAsync(c.d_lpm_wins, b.lw.data(), sizeof(ug::LpmOutWin) * b.lw.size(), hipMemcpyHostToDevice, c.main.s));
  const int nl = (int)b.lw.size();
  if (nl > 0) {
    Stage st(c, 0);
    ug::lpm_out_steps_kernel<<<dim3((max_T + 255) / 256, 5, nl), 256, 0, c.main.s>>>(c.d_lpm_wins);
    ug::lpm_out_scan_kernel<<<dim3(5, nl), 64, 0, c.main.s>>>(c.d_lpm_wins);
    ug::lpm_out_finish_kernel<<<nl, 256, 0, c.main.s>>>(c.d_lpm_wins);
    UHIP(hipGetLastError());
  }
  return 0;
}

// The windows are independent and nearly every kernel below is a chain of short, latency-bound launches with one (or a few)
// workgroups per window, so the batch CAN be cut into groups that advance on their own pairs of streams (main + correlation
// chain).  Measured on the C4 batch (64 windows, profiles/r02/ugpm_groups.txt): 1 group 5.54 ms, 2 groups 5.70 ms, 4 groups
// 7.36 ms alone, and 10.5 / 10.8 / 11.2 ms per overlapped step -- twice the launches cost more host and queue time than the
// concurrency returns, so the default stays ONE group; GORIO_UGPM_GROUPS overrides it for experiments.  The arithmetic of a
// window does not depend on the grouping.
int open_groups(Ctx& c, Batch& b) {
  int n_groups = 1;
  if (const char* e = std::getenv("GORIO_UGPM_GROUPS")) n_groups = std::atoi(e);
  n_groups = std::max(1, std::min(std::min(n_groups, 8), b.nw));
  while ((int)c.groups.size() < n_groups) {
    Ctx::Group g;
    if (c.groups.empty()) static_cast<StreamPair&>(g) = c.main;
    else if (int rc = make_stream_pair(g)) return rc;
    UHIP(hipEventCreateWithFlags(&g.ev_done, hipEventDisableTiming));
    UHIP(hipEventCreateWithFlags(&g.ev_tab, hipEventDisableTiming));
    c.groups.push_back(g);
  }
  if (!c.ev_up) UHIP(hipEventCreateWithFlags(&c.ev_up, hipEventDisableTiming));
  UHIP(hipEventRecord(c.ev_up, c.main.s));  // inputs, window descriptors and control words are on the device once this fires
  b.runs.resize(n_groups);
  for (int g = 0; g < n_groups; ++g) {
    Run& r = b.runs[g];
    static_cast<Ctx::Group&>(r) = c.groups[g];
    r.g0 = (int)((long)b.nw * g / n_groups);
    r.nw = (int)((long)b.nw * (g + 1) / n_groups) - r.g0;
    r.wins = c.d_wins + r.g0;
    if (g > 0) UHIP(hipStreamWaitEvent(r.s, c.ev_up, 0));
  }
  return 0;
}

// J^T J launches: one workgroup per (row slice, tile group, window), see ata_kernel
void launch_ata(Ctx& c, int max_S, const Run& r, int which, int decide = 0) {
  hipStream_t sq = which == 2 ? r.s2 : r.s;
  Stage st_ata(c, which == 2 ? 6 : 5, sq);
  const int n = (which == 2 ? 6 : 3) * max_S;
  const int tpg = which == 2 ? kAtaTilesCorr : kAtaTilesLm;
  const int dense = (g_debug_path.load() & 1) ? 1 : 0;
  const int ng = ata_cut(n, which == 2 && !dense ? 3 * max_S : n, tpg).groups();  // of the largest window: no window has more (both kinds of group grow with S)
  const int npad = ((n + 15) / 32) * 32 + 16;
  const int grid = ((r.nw + 7) / 8) * ng * 8;  // 8 windows (one per XCD) x ng tile groups per slice of the grid
  // LDS as small as the staging needs (53 KB at n = 198): the scan matcher's kernels share the CUs with these workgroups
  auto lds = [&](int kc) { return sizeof(double) * 2 * kc * (npad + 1); };
  if (which == 2) {
    if (npad <= 256) ug::ata_kernel<4, 16, kAtaTilesCorr><<<grid, 512, lds(16), sq>>>(r.wins, which, r.nw, ng, decide, dense);
    else if (npad <= 512) ug::ata_kernel<8, 16, kAtaTilesCorr><<<grid, 512, lds(16), sq>>>(r.wins, which, r.nw, ng, decide, dense);
    else ug::ata_kernel<16, 8, kAtaTilesCorr><<<grid, 512, lds(8), sq>>>(r.wins, which, r.nw, ng, decide, dense);
  } else {
    if (npad <= 256) ug::ata_kernel<4, 16, kAtaTilesLm><<<grid, 512, lds(16), sq>>>(r.wins, which, r.nw, ng, decide, dense);
    else ug::ata_kernel<8, 16, kAtaTilesLm><<<grid, 512, lds(16), sq>>>(r.wins, which, r.nw, ng, decide, dense);  // n = 3S <= 480
  }
}

// The solver kernels in the instantiation solver_sizes (ugpm_windows.h) picks for the largest window of the batch.  Each switch names every
// value solver_sizes can return for that kernel; a smaller instantiation runs the same instructions on the same data as the full one
// (the conditions are written down with solver_sizes), so which one runs never shows in the results.
SolverSizes batch_sizes(const Batch& b) { return solver_sizes(b.max_S, (g_debug_path.load() & 4) != 0); }

void launch_gram(const Run& r, const SolverSizes& z) {
  const dim3 grid(6, r.nw);
  if (z.gram_rows == kGramRowsSmall) ug::gram_kernel<kGramRowsSmall, kGramKmax><<<grid, 256, 0, r.s>>>(r.wins);
  else if (z.gram_rows == kGramRows) ug::gram_kernel<kGramRows, kGramKmax><<<grid, 256, 0, r.s>>>(r.wins);
  else ug::gram_kernel<kCholRowsFull, kSolveKmaxFull><<<grid, 256, 0, r.s>>>(r.wins);
}

void launch_lm_step(const Run& r, const SolverSizes& z, int problem) {
  const dim3 grid(r.nw, problem == 1 ? kVelBlocks : 1);
  if (z.lm_rows == kLmRowsSmall) ug::lm_step_kernel<kLmRowsSmall><<<grid, 512, 0, r.s>>>(r.wins);
  else ug::lm_step_kernel<kCholRowsFull><<<grid, 512, 0, r.s>>>(r.wins);
}

void launch_corr_diag(const Run& r, const SolverSizes& z, int max_S) {
  const dim3 grid((6 * max_S + 15) / 16, r.nw);
  const size_t lds = sizeof(double) * 17 * (6 * max_S + 16);
  if (z.solve_kmax == kSolveKmaxSmall) ug::corr_diag_kernel<kSolveKmaxSmall><<<grid, 256, lds, r.s2>>>(r.wins);
  else ug::corr_diag_kernel<kSolveKmaxFull><<<grid, 256, lds, r.s2>>>(r.wins);
}

void launch_infer(const Run& r, const SolverSizes& z, int max_S, int max_infer) {
  const dim3 grid(std::max(1, max_infer), r.nw);
  const size_t lds = sizeof(double) * 17 * (6 * max_S + 16);
  if (z.solve_kmax == kSolveKmaxSmall) ug::infer_kernel<kSolveKmaxSmall><<<grid, 256, lds, r.s>>>(r.wins);
  else ug::infer_kernel<kSolveKmaxFull><<<grid, 256, lds, r.s>>>(r.wins);
}

int enqueue_tables_and_correlation(Ctx& c, Batch& b) {
  const int max_S = b.max_S;
  const SolverSizes sizes = batch_sizes(b);
  for (const Run& r : b.runs) {
    {
      Stage st(c, 0, r.s);
      ug::lpm_rot_kernel<<<dim3(r.nw, 5), 320, 0, r.s>>>(r.wins);
      ug::lpm_init_kernel<<<r.nw, 320, 0, r.s>>>(r.wins);
    }
    {
      Stage st(c, 1, r.s);
      launch_gram(r, sizes);
      ug::cross_kernel<<<dim3(12, r.nw, (std::max(b.max_G, b.max_V) + ug::kCrossRows - 1) / ug::kCrossRows), 256, sizeof(double) * ug::kCrossRows * (((max_S + 31) / 32) * 32 + 4), r.s>>>(r.wins);
    }
    // State correlation at the LPM-initialised state.  The reference assembles the Jacobian synchronously (preint.h:887-937) and
    // hands J^T J, its factorisation and the inverse diagonal to a helper thread that runs beside the two ceres::Solve calls and is
    // joined before the first get() (preint.h:939, 1062-1065).  Here the whole chain, Jacobian included, runs on a second stream
    // as soon as the kernel tables exist; the Jacobian reads the LPM-initialised states, so the main stream waits for it (ev_jac)
    // before the first fit writes its solution back (lm_end_kernel), and the inference waits for the end of the chain (ev_corr).
    UHIP(hipEventRecord(r.ev_tab, r.s));
    UHIP(hipStreamWaitEvent(r.s2, r.ev_tab, 0));
    {
      Stage st(c, 2, r.s2);
      ug::corr_jac_kernel<<<dim3(ug::kCorrJacParts, r.nw), 256, 0, r.s2>>>(r.wins);
      UHIP(hipEventRecord(r.ev_jac, r.s2));
      launch_ata(c, max_S, r, 2);
      ug::corr_factor_kernel<<<r.nw, 512, 0, r.s2>>>(r.wins);
      launch_corr_diag(r, sizes, max_S);
    }
    UHIP(hipEventRecord(r.ev_corr, r.s2));
  }
  return 0;
}

// ceres::Solve #1 (problem 0, rotation) or #2 (problem 1, velocity), preint.h:943-967
int run_fit(Ctx& c, Batch& b, int problem) {
  const int max_S = b.max_S;
  const SolverSizes sizes = batch_sizes(b);
  std::vector<int>& flags = b.flags;
  const bool lmtrace = std::getenv("GORIO_UGPM_LMTRACE") != nullptr;
  const bool speculative = g_speculative_rot.load() != 0;
  std::vector<std::unique_ptr<Stage>> st_lm;
  for (Run& r : b.runs) {
    st_lm.emplace_back(new Stage(c, 3, r.s));  // the fit was started by lpm_init_kernel (rotation) / lm_turn_kernel (velocity)
    if (problem == 0) ug::rot_eval_kernel<<<dim3(r.nw, kEvalSplit), 256, 0, r.s>>>(r.wins, 2);
    else ug::vel_eval_kernel<<<dim3(r.nw, kEvalSplit), 256, 0, r.s>>>(r.wins, 2);
    launch_ata(c, max_S, r, problem);
    r.active = true;
  }
  for (int it = 0; it <= 51; ++it) {
    bool any = false;
    for (Run& r : b.runs) {
      if (!r.active) continue;
      any = true;
      launch_lm_step(r, sizes, problem);
      if (problem == 0 && speculative) {
        // three launches per iteration: the candidate residual AND the Jacobian at the candidate in one evaluation, the
        // acceptance test inside the J^T J launch (rot_eval_kernel mode 3, ata_kernel decide)
        ug::rot_eval_kernel<<<dim3(r.nw, kEvalSplit), 256, 0, r.s>>>(r.wins, 3);
        launch_ata(c, max_S, r, problem, 1);
        continue;
      }
      if (problem == 0) ug::rot_eval_kernel<<<dim3(r.nw, kEvalSplit), 256, 0, r.s>>>(r.wins, 0);
      else ug::vel_eval_kernel<<<dim3(r.nw, kEvalSplit), 256, 0, r.s>>>(r.wins, 0);
      if (problem == 0) {
        ug::rot_eval_kernel<<<dim3(r.nw, kEvalSplit), 256, 0, r.s>>>(r.wins, 1);
        launch_ata(c, max_S, r, problem);
      } else {
        ug::lm_relinearize_linear_kernel<<<dim3(r.nw, (3 * max_S + 63) / 64), 256, 0, r.s>>>(r.wins);  // linear problem: J and J^T J stay exact
      }
    }
    if (!any) break;
    if (lmtrace) {  // GORIO_UGPM_LMTRACE: the solver's control words of window 0 after every iteration (a debugging aid: drains the stream)
      double lc[16];
      int li[16];
      UHIP(hipStreamSynchronize(b.runs[0].s));
      UHIP(hipMemcpy(lc, b.dw[0].lmc, sizeof(lc), hipMemcpyDeviceToHost));
      UHIP(hipMemcpy(li, b.dw[0].lmi, sizeof(li), hipMemcpyDeviceToHost));
      std::fprintf(stderr, "[ugpm lm] problem %d it %d: iter %d done %d term %d succ %d cost %.17g cost_new %.17g radius %.6g mcc %.17g step_norm2 %.6g x_norm %.17g initial %.17g\n", problem, it,
                   li[0], li[1], li[5], li[6], lc[0], lc[1], lc[2], lc[8], lc[11], lc[4], lc[7]);
    }
    // When to look at the done flags (a look drains the stream: copy, synchronise, ~30 us of idle GPU, and far more while the queue
    // runs empty behind the scan matcher's launches).  A finished window's kernels return at once, so iterations enqueued beyond the
    // need cost three empty launches each, far less than a look.  The first batch of a context looks every other iteration from the
    // fourth on (no window of the C2 shape finishes in fewer than four).  Later batches enqueue as many iterations as the previous
    // batch needed and go straight on, without a look: the kernel that ends the fit (lm_end_block) marks a window that is not done,
    // nothing touches it after that, and collect() runs the marked windows again -- with looks, which then start at the budget.
    const int budget = c.lm_budget[problem];
    if (budget > 0 && !b.looks) {
      b.enqueued_blind[problem] = true;
      if (it + 1 >= budget) break;
      continue;
    }
    const bool look = budget > 0 ? (it + 1 >= budget && ((it + 1 - budget) & 1) == 0) : (it >= 3 && (it & 1) == 1);
    if (look) {
      for (Run& r : b.runs)
        if (r.active) UHIP(hipMemcpyAsync(flags.data() + kWinInts * (size_t)r.g0, c.d_ints + kWinInts * (size_t)r.g0, sizeof(int) * kWinInts * (size_t)r.nw, hipMemcpyDeviceToHost, r.s));
      for (Run& r : b.runs) {
        if (!r.active) continue;
        UHIP(hipStreamSynchronize(r.s));
        bool all = true;
        for (int i = r.g0; i < r.g0 + r.nw; ++i) all = all && (flags[kWinInts * (size_t)i + 1] || flags[kWinInts * (size_t)i + 16] != 0);
        if (all) r.active = false;
      }
      bool every = true;
      for (Run& r : b.runs) every = every && !r.active;
      if (every) {  // iterations the slowest window really needed: its step count, plus the step kernel that noticed a termination of its own (gradient, iteration cap, radius)
        int need = 1;
        for (int i = 0; i < b.nw; ++i) {
          const int* f = flags.data() + kWinInts * (size_t)i;
          if (f[16] != 0) continue;
          need = std::max(need, f[0] + (f[5] >= 3 ? 1 : 0));
        }
        need = std::min(need, it + 1);
        c.lm_budget[problem] = b.rerun ? std::max(c.lm_budget[problem], need) : need;  // a re-run is the rest of its batch: the slowest window of both counts
      }
    }
  }
  for (size_t g = 0; g < b.runs.size(); ++g) {
    const Run& r = b.runs[g];
    if (problem == 0) {  // the rotation fit ends and the velocity fit starts in one launch; the velocity fit ends inside finish_kernel
      UHIP(hipStreamWaitEvent(r.s, r.ev_jac, 0));  // corr_jac_kernel has read the initial states
      ug::lm_turn_kernel<<<r.nw, 256, 0, r.s>>>(r.wins, c.d_diag + 4 * (size_t)r.g0);
    }
    st_lm[g].reset();  // stage stop event behind the group's last launch of this problem
  }
  return 0;
}

int enqueue_finish_and_infer(Ctx& c, Batch& b) {
  const SolverSizes sizes = batch_sizes(b);
  for (const Run& r : b.runs) {
    UHIP(hipStreamWaitEvent(r.s, r.ev_corr, 0));  // join of the correlation chain (preint.h:1062-1065)
    {
      Stage st(c, 4, r.s);
      ug::finish_kernel<<<r.nw, 256, 0, r.s>>>(r.wins, c.d_diag + 4 * (size_t)r.g0);
      launch_infer(r, sizes, b.max_S, b.max_infer);
    }
    UHIP(hipEventRecord(r.ev_done, r.s));
  }
  for (size_t g = 1; g < b.runs.size(); ++g) UHIP(hipStreamWaitEvent(c.main.s, b.runs[g].ev_done, 0));  // the downloads follow every group
  UHIP(hipGetLastError());
  return 0;
}

// ---- results: the downloads, the stage times, and per window its status and diagnostics; returns the windows whose fits were not done
int collect(Ctx& c, Batch& b, gorio_ugpm_meas* out, gorio_ugpm_diag* diag, std::vector<int>& unfinished) {
  double* const rec = static_cast<double*>(c.pin_out.get());  // [total_out] records, [4 nw] diagnostics, then the control words
  double* const dg = rec + b.total_out;
  int* const fin = reinterpret_cast<int*>(dg + 4 * (size_t)b.nw);
  UHIP(hipMemcpyAsync(fin, c.d_ints, sizeof(int) * kWinInts * (size_t)b.nw, hipMemcpyDeviceToHost, c.main.s));
  UHIP(hipMemcpyAsync(dg, c.d_diag, sizeof(double) * 4 * (size_t)b.nw, hipMemcpyDeviceToHost, c.main.s));
  if (b.total_out) UHIP(hipMemcpyAsync(rec, b.out_region, sizeof(double) * b.total_out, hipMemcpyDeviceToHost, c.main.s));
  UHIP(hipStreamSynchronize(c.main.s));
  if (b.total_out) std::memcpy(out, rec, sizeof(double) * b.total_out);
  for (const Ctx::StageEvents& e : c.ev) {
    float ms = 0.f;
    if (hipEventSynchronize(e.b) == hipSuccess && hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
      g_stage_s[e.stage] += ms * 1e-3;
      g_stage_n[e.stage] += 1;
    }
  }
  c.drop_stage_events();
  if (b.enqueued_blind[0] || b.enqueued_blind[1]) {
    // the budget of the next batch: what the slowest window of this one needed.  A fit that looked has set it already (run_fit);
    // the re-run of the unfinished windows raises it to what they need.
    FitOutcome o = fit_outcome(fin, b.hw);
    for (int p = 0; p < 2; ++p)
      if (b.enqueued_blind[p] && o.need[p] > 0) c.lm_budget[p] = o.need[p];
    unfinished.swap(o.rerun);
  }
  b.final_status.assign(b.nw, 0);
  for (int i = 0; i < b.nw; ++i) {
    const HostWin& h = b.hw[i];
    const int st = h.status != 0 ? h.status : fin[kWinInts * (size_t)i + (h.is_lpm ? 17 : 16)];
    b.final_status[i] = st;
    if (diag) {
      gorio_ugpm_diag& d = diag[i];
      d.nb_state = h.S; d.nb_gyr = h.G; d.nb_vel = h.V;
      d.iters_rot = (int)dg[4 * (size_t)i + 0]; d.cost_rot = dg[4 * (size_t)i + 1];
      d.iters_vel = (int)dg[4 * (size_t)i + 2]; d.cost_vel = dg[4 * (size_t)i + 3];
      d.status = st; d.state_freq = h.state_freq;
    }
  }
  return 0;
}

int preint_batch_flat(const gorio_ugpm_window* windows, int n_windows, gorio_ugpm_meas* out, gorio_ugpm_diag* diag, int device, bool rerun);

// The windows a fit left unfinished (it had the budget of the previous batch and no look), as a batch of their own that looks: a
// window's result does not depend on the batch it is in.  Their records, diagnostics and statuses replace the placeholders.
int rerun_unfinished(Batch& b, const std::vector<int>& unfinished, gorio_ugpm_meas* out, gorio_ugpm_diag* diag, int device) {
  std::vector<gorio_ugpm_window> sub;
  size_t n_out = 0;
  for (int i : unfinished) {
    sub.push_back(b.windows[i]);
    n_out += (size_t)b.windows[i].n_infer;
  }
  std::vector<gorio_ugpm_meas> sub_out(n_out);
  std::vector<gorio_ugpm_diag> sub_diag(sub.size());
  const int rc = preint_batch_flat(sub.data(), (int)sub.size(), sub_out.data(), sub_diag.data(), device, true);
  bool per_window = false;  // as in gorio_ugpm_preint_batch: a per-window failure is reported through the diagnostics, anything else fails the call
  for (const gorio_ugpm_diag& d : sub_diag) per_window = per_window || d.status != 0;
  if (rc != 0 && !per_window) return rc;
  size_t at = 0;
  for (size_t k = 0; k < unfinished.size(); ++k) {
    const int i = unfinished[k];
    const size_t cnt = (size_t)b.windows[i].n_infer;
    std::memcpy(reinterpret_cast<double*>(out) + b.out_offs[i], sub_out.data() + at, sizeof(gorio_ugpm_meas) * cnt);
    at += cnt;
    b.final_status[i] = sub_diag[k].status;
    if (diag) diag[i] = sub_diag[k];
  }
  return 0;
}

// per window: NaN records where it failed, and the first failure as the error of the call
void report(Batch& b, gorio_ugpm_meas* out) {
  for (int i = 0; i < b.nw; ++i) {
    const HostWin& h = b.hw[i];
    const int st = b.final_status[i];
    // rejected on the host: its records were never written; the LPM kernels stop mid-way on a data-domain error: no partial records
    if (h.status != 0 || (h.is_lpm && st != 0)) {
      double* o = reinterpret_cast<double*>(out) + b.out_offs[i];
      std::fill(o, o + (size_t)std::max(0, b.windows[i].n_infer) * 83, std::numeric_limits<double>::quiet_NaN());
    }
    if (st != 0 && h.status == 0)
      b.note_error(i, st, st == GORIO_UGPM_ERR_NUMERIC ? "Cholesky factorisation met a non-positive pivot" : "LPM Partial: the start_time is not in the data domain");
  }
}

// every window non-chunked (quantum < 0): the device path
int preint_batch_flat(const gorio_ugpm_window* windows, int n_windows, gorio_ugpm_meas* out, gorio_ugpm_diag* diag, int device, bool rerun) {
  if (!windows || n_windows <= 0 || !out) return ufail(GORIO_UGPM_ERR_INVALID, "gorio_ugpm_preint_batch: bad arguments");
  Ctx& c = g_ctx;
  if (int rc = ensure_context(c, device)) return rc;
  if (!rerun)
    for (int i = 0; i < 8; ++i) { g_stage_s[i] = 0; g_stage_n[i] = 0; }  // a re-run adds to the stage times of its batch
  std::vector<int> unfinished;
  Batch b{windows, n_windows};
  b.rerun = rerun;
  b.looks = rerun || (g_debug_path.load() & 2) != 0;
  {
    StageEventsGuard guard{c};
    auto tnow = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double tt0 = tnow();
    plan_windows(b);
    if (int rc = reserve_workspace(c, b)) return rc;
    if (int rc = stage_and_upload(c, b)) return rc;
    const double tt1 = tnow();
    if (int rc = run_lpm_windows(c, b)) return rc;
    if (b.max_S > 0) {
      b.flags.resize(kWinInts * (size_t)b.nw);
      if (int rc = open_groups(c, b)) return rc;
      if (int rc = enqueue_tables_and_correlation(c, b)) return rc;
      for (int problem = 0; problem < 2; ++problem)
        if (int rc = run_fit(c, b, problem)) return rc;
      if (int rc = enqueue_finish_and_infer(c, b)) return rc;
    }
    const double tt3 = tnow();
    if (int rc = collect(c, b, out, diag, unfinished)) return rc;
    if (std::getenv("GORIO_UGPM_TRACE")) std::fprintf(stderr, "[ugpm trace] prep %.3f ms, kernels+polls %.3f ms, results %.3f ms, unfinished %d\n", (tt1 - tt0) * 1e3, (tt3 - tt1) * 1e3, (tnow() - tt3) * 1e3, (int)unfinished.size());
  }
  if (!unfinished.empty())  // the device buffers of the context are free again: every download above is complete
    if (int rc = rerun_unfinished(b, unfinished, out, diag, device)) return rc;
  report(b, out);
  if (b.first_error) return ufail(b.first_error, b.first_error_msg);
  return GORIO_UGPM_OK;
}

}  // namespace

extern "C" {

void gorio_ugpm_default_window(gorio_ugpm_window* w) {
  if (!w) return;
  std::memset(w, 0, sizeof(*w));
  w->type = GORIO_UGPM_TYPE_UGPM;  // types.h:288
  w->min_freq = 500;                // types.h:287
  w->quantum = -1;                  // types.h:289
  w->state_freq = 50.0;             // types.h:290
  w->correlate = 1;                 // types.h:291
  w->overlap = 8;                   // preint.h:19
  w->vel_bias_std = 0.3;            // preint.h:55
  w->gyr_bias_std = 0.03;
}

const char* gorio_ugpm_last_error(void) { return g_err.c_str(); }

void gorio_ugpm_debug_set_schedule(int speculative_rot) { g_speculative_rot.store(speculative_rot ? 1 : 0); }

void gorio_ugpm_debug_set_path(int flags) { g_debug_path.store(flags); }

int gorio_ugpm_get_stage_times(double seconds[8], int counts[8]) {
  for (int i = 0; i < 8; ++i) {
    if (seconds) seconds[i] = g_stage_s[i];
    if (counts) counts[i] = g_stage_n[i];
  }
  return 0;
}

// Requests with opt.quantum >= 0 (preint.h:1584-1702) are cut into chunk windows (ugpm_chunks.h); the chunk windows of ALL such
// requests join the other windows of the call in one device batch, and their records are chained on the host afterwards.
int gorio_ugpm_preint_batch(const gorio_ugpm_window* windows, int n_windows, gorio_ugpm_meas* out, gorio_ugpm_diag* diag, int device) {
  if (!windows || n_windows <= 0 || !out) return ufail(GORIO_UGPM_ERR_INVALID, "gorio_ugpm_preint_batch: bad arguments");
  bool any_chunked = false;
  for (int i = 0; i < n_windows; ++i) any_chunked = any_chunked || windows[i].quantum >= 0;
  if (!any_chunked) return preint_batch_flat(windows, n_windows, out, diag, device, false);
  struct Req { int first = 0, count = 0, status = 0; chunks::Plan plan; size_t out0 = 0; };  // first/count: its windows in the expanded batch
  std::vector<Req> reqs(n_windows);
  std::vector<gorio_ugpm_window> flat;
  std::vector<size_t> flat_out0;
  int first_error = 0;
  std::string first_error_msg;
  size_t n_flat_out = 0, out_off = 0;
  for (int i = 0; i < n_windows; ++i) {
    const gorio_ugpm_window& w = windows[i];
    Req& r = reqs[i];
    r.out0 = out_off;
    out_off += (size_t)std::max(0, w.n_infer);
    r.first = (int)flat.size();
    if (w.quantum < 0) {
      r.count = 1;
      flat.push_back(w);
      flat_out0.push_back(n_flat_out);
      n_flat_out += (size_t)std::max(0, w.n_infer);
      continue;
    }
    std::string err;
    if (!w.gyr_t || !w.gyr || !w.vel_t || !w.vel || !w.infer_t || w.n_infer <= 0) {
      r.status = GORIO_UGPM_ERR_INVALID;
      err = "null pointers or no inference time";
    } else {
      r.status = chunks::plan_chunks(w, r.plan, err);
    }
    if (r.status != 0) {
      if (!first_error) {
        first_error = r.status;
        first_error_msg = "window " + std::to_string(i) + ": " + err;
      }
      continue;
    }
    for (chunks::Chunk& c : r.plan.chunks) {  // one ordinary window per chunk: VelPreintegration(data of the chunk, chunk start, stamps, quantum = -1), get(.., 0, 0)
      gorio_ugpm_window cw = w;
      cw.gyr_t = w.gyr_t + c.g0; cw.gyr = w.gyr + 3 * (size_t)c.g0; cw.n_gyr = c.ng;
      cw.vel_t = w.vel_t + c.v0; cw.vel = w.vel + 3 * (size_t)c.v0; cw.n_vel = c.nv;
      cw.start_t = c.start_t;
      cw.infer_t = c.infer_t.data(); cw.n_infer = (int)c.infer_t.size();
      cw.group_sizes = c.group_sizes.data(); cw.n_groups = (int)c.group_sizes.size();
      cw.quantum = -1;
      cw.vel_bias_std = 0.0; cw.gyr_bias_std = 0.0;
      flat.push_back(cw);
      flat_out0.push_back(n_flat_out);
      n_flat_out += c.infer_t.size();
    }
    r.count = (int)r.plan.chunks.size();
  }
  const gorio_ugpm_meas nan_meas = [] {
    gorio_ugpm_meas m;
    double* p = reinterpret_cast<double*>(&m);
    for (size_t k = 0; k < sizeof(m) / sizeof(double); ++k) p[k] = std::numeric_limits<double>::quiet_NaN();
    return m;
  }();
  std::vector<gorio_ugpm_meas> flat_out(std::max<size_t>(1, n_flat_out), nan_meas);
  std::vector<gorio_ugpm_diag> flat_diag(std::max<size_t>(1, flat.size()));
  int rc = 0;
  if (!flat.empty()) {
    rc = preint_batch_flat(flat.data(), (int)flat.size(), flat_out.data(), flat_diag.data(), device, false);
    bool per_window = false;  // a per-window failure leaves the other windows valid and is reported through the diagnostics; anything else fails the call
    for (const gorio_ugpm_diag& d : flat_diag) per_window = per_window || d.status != 0;
    if (rc != 0 && !per_window) return rc;
  }
  const std::string flat_msg = rc != 0 ? g_err : std::string();
  for (int i = 0; i < n_windows; ++i) {
    const gorio_ugpm_window& w = windows[i];
    Req& r = reqs[i];
    gorio_ugpm_meas* o = out + r.out0;
    gorio_ugpm_diag d{};
    if (r.status == 0 && w.quantum < 0) {
      for (int k = 0; k < w.n_infer; ++k) o[k] = flat_out[flat_out0[r.first] + k];
      d = flat_diag[r.first];
      r.status = d.status;
    } else if (r.status == 0) {
      std::vector<const gorio_ugpm_meas*> recs;
      for (int q = 0; q < r.count; ++q) {
        const gorio_ugpm_diag& cd = flat_diag[r.first + q];
        if (cd.status != 0 && r.status == 0) r.status = cd.status;
        recs.push_back(flat_out.data() + flat_out0[r.first + q]);
        // diagnostics of a chunked request: sizes and state frequency of its LAST chunk, iterations and costs summed over the chunks
        d.nb_state = cd.nb_state; d.nb_gyr = cd.nb_gyr; d.nb_vel = cd.nb_vel; d.state_freq = cd.state_freq;
        d.iters_rot += cd.iters_rot; d.iters_vel += cd.iters_vel; d.cost_rot += cd.cost_rot; d.cost_vel += cd.cost_vel;
      }
      if (r.status == 0) chunks::chain_chunks(r.plan, recs, w.vel_bias_std, w.gyr_bias_std, o);
    }
    if (r.status != 0) {
      for (int k = 0; k < std::max(0, w.n_infer); ++k) o[k] = nan_meas;
      if (!first_error) {
        first_error = r.status;
        first_error_msg = "window " + std::to_string(i) + (flat_msg.empty() ? std::string(": failed") : ": (expanded batch) " + flat_msg);
      }
    }
    d.status = r.status;
    if (diag) diag[i] = d;
  }
  if (first_error) return ufail(first_error, first_error_msg);
  return 0;
}

/* combinePreints (math_utils.h:689-726) */
int gorio_ugpm_combine_preints(const gorio_ugpm_meas* prev, const gorio_ugpm_meas* cur, gorio_ugpm_meas* out) {
  if (!prev || !cur || !out) return ufail(GORIO_UGPM_ERR_INVALID, "gorio_ugpm_combine_preints: null pointer");
  *out = chunks::combine_preints(*prev, *cur);
  return 0;
}

}  // extern "C"
