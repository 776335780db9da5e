// ugpm_windows.h -- host bookkeeping of one pre-integration window, before anything touches the device: the checks of a request, its
// state time line and sample slices (preint.h:766-811, 1532-1556), the layout of its workspace slab and input slot, the SoA staging of
// its samples, and for opt.type = LPM the merged time line of one IterativeIntegrator with the layout of its scratch.  Host code without
// HIP: ugpm_api.hip drives the device with it, host/test/ugpm_window_plan.cpp runs it alone.  No numerics beyond the state time line.
#pragma once

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/gorio_ugpm.h"
#include "ugpm_device.h"

namespace gorio {
namespace windows {

constexpr int kMaxStates = 160;  // plan_window refuses larger windows; the solver kernels' capacities (solver_sizes below) are sized for it

struct HostWin {
  int g0 = 0, G = 0, v0 = 0, V = 0, S = 0;
  double state_freq = 0;
  std::vector<double> state_t;
  int status = 0;
  size_t ws_doubles = 0;
  bool is_lpm = false;  // opt.type = LPM: handled by ugpm_lpm_out.hip, skipped by every UGPM kernel
};

// GyroVelData::get(from, to): samples with from < t < to, scanning until the first t >= to (types.h:187-223)
inline void slice(const double* t, int n, double from, double to, int& i0, int& cnt) {
  i0 = 0;
  cnt = 0;
  if (from >= to || n <= 0) return;
  for (int i = 0; i < n; ++i) {
    if (!(t[i] > from)) continue;
    if (!(t[i] < to)) break;
    if (cnt++ == 0) i0 = i;
  }
}

inline size_t input_doubles(const gorio_ugpm_window& w, const HostWin& h) { return (size_t)h.G * 4 + (size_t)h.V * 4 + (size_t)w.n_infer + (size_t)h.S; }
// the window's slot in the batch-wide input region: input_doubles padded to 4 doubles (zeros)
inline size_t input_slot(const gorio_ugpm_window& w, const HostWin& h) { return (input_doubles(w, h) + 3) / 4 * 4; }

// `cnt` elements at offset `off` of `base`, then off += cnt; a null base (the sizing pass) stays null
template <typename T>
T* take_at(T* base, size_t& off, size_t cnt) {
  T* r = base ? base + off : nullptr;
  off += cnt;
  return r;
}

// carve one window's slab; returns the number of doubles used (called once with null pointers for sizing).
// `in` = this window's slice of the batch-wide contiguous input region (one upload for the whole batch), `outp` = its slice of
// the batch-wide output region (one download)
inline size_t carve(const gorio_ugpm_window& w, const HostWin& h, UgpmWin& u, double* base, double* in, double* outp) {
  size_t used = 0, used_in = 0;
  auto take = [&](size_t cnt) { return take_at(base, used, cnt); };
  auto take_in = [&](size_t cnt) { return take_at(in, used_in, cnt); };
  const size_t S = h.S, G = h.G, V = h.V, n = 3 * S, mrot = 3 * S + 3 * G, mvel = 3 * V + 3 * S, mc = 3 * G + 3 * V, nc = 6 * S;
  u.gyr_t = take_in(G); u.gyr = take_in(3 * G); u.vel_t = take_in(V); u.vel = take_in(3 * V); u.infer_t = take_in(w.n_infer); u.state_t = take_in(S);
  u.Rq = take(5 * 2 * S * 9); u.Rstart = take(5 * 9); u.velr = take(3 * V); u.dp = take(2 * S * 3); u.r0 = take(5 * S * 3); u.r1 = take(5 * S * 3);
  u.s_dr = take(3 * S); u.s_vel = take(3 * S); u.hyper = take(24);
  u.d_r_dt_local = take(S * 3); u.d_r_dt_local_shift = take(S * 3); u.delta_r_time = take(S * 3); u.delta_r_bw = take(3 * S * 3); u.d_r_bw_local_shift = take(3 * S * 3);
  u.Kinv = take(6 * S * S); u.KKinv = take(6 * S * S); u.KintKinv = take(3 * S * S); u.var = take(6 * S); u.wgp = take(6 * S); u.sstd = take(6 * S);
  u.KsKinv = take(3 * G * S); u.KsIntKinv = take(3 * G * S); u.KgyrIntKinv = take(3 * V * S); u.KvelKinv = take(3 * V * S);
  u.Jrot = take(mrot * n); u.Jvel = take(mvel * n); u.res = take(std::max(mrot, mvel)); u.res_new = take(std::max(mrot, mvel));
  u.JtJ = take(n * n); u.lhs = take(n * n); u.lmv = take(8 * n); u.sample_tmp = take(std::max(G, V) * 24); u.sample_tmp_c = take(std::max(G, V) * 24);
  if (w.correlate) { u.Jc = take(mc * nc); u.Ac = take(nc * nc); }
  u.dsc = take(nc);
  u.alpha = take(6 * S); u.state_r = take(3 * S); u.d_state_bw = take(3 * S * 3); u.d_d_r_dt = take(3 * S); u.d_vel_bv = take(3 * S * 3); u.d_vel_bw = take(3 * S * 3);
  u.d_vel_dt = take(3 * S); u.out = outp; u.lmc = take(16);
  return (used + 31) / 32 * 32;
}

// The checks and the plan of one request (preint.h:1532-1556, 766-811), in the reference's order: fills `h`, returns its status and,
// for a refusal, the text in `err`.  An LPM request is only checked here (is_lpm, G, V = all samples); its plan is build_lpm_timeline.
inline int plan_window(const gorio_ugpm_window& w, HostWin& h, std::string& err) {
  auto fail = [&](int code, const char* m) {
    err = m;
    return h.status = code;
  };
  if (!w.gyr_t || !w.gyr || !w.vel_t || !w.vel || !w.infer_t || w.n_infer <= 0) return fail(GORIO_UGPM_ERR_INVALID, "null pointers or no inference time");
  if (w.quantum >= 0) return fail(GORIO_UGPM_ERR_INVALID, "a chunked request reached the device path");  // gorio_ugpm_preint_batch expands them
  if (w.type != GORIO_UGPM_TYPE_UGPM && w.type != GORIO_UGPM_TYPE_LPM) return fail(GORIO_UGPM_ERR_INVALID, "unknown pre-integration type");
  if (w.n_gyr < 2 || w.n_vel < 2) return fail(GORIO_UGPM_ERR_RANGE, "InterpolateLinear: this function need at least 2 data points to interpolate");
  if (w.group_sizes && w.n_groups > 0) {
    long tot = 0;
    for (int g = 0; g < w.n_groups; ++g) tot += w.group_sizes[g] < 0 ? -(1L << 40) : w.group_sizes[g];
    if (tot != w.n_infer) return fail(GORIO_UGPM_ERR_INVALID, "group_sizes do not add up to n_infer");
  }
  if (w.type == GORIO_UGPM_TYPE_LPM) {  // preint.h:1567-1580: IterativeIntegrator over the WHOLE data set, no state window
    if (!(w.min_freq > 0.0)) return fail(GORIO_UGPM_ERR_INVALID, "min_freq must be positive");
    bool any = false;
    for (int j = 0; j < w.n_infer; ++j) any = any || (w.infer_t[j] >= w.start_t);
    if (!any) return fail(GORIO_UGPM_ERR_RANGE, "FullLPM: the start_time is not in the query domain");  // preint.h:559
    h.is_lpm = true;
    h.G = w.n_gyr;
    h.V = w.n_vel;
    return 0;
  }
  const double vel_freq = (w.n_vel - 1) / (w.vel_t[w.n_vel - 1] - w.vel_t[0]);
  const double gyr_freq = (w.n_gyr - 1) / (w.gyr_t[w.n_gyr - 1] - w.gyr_t[0]);
  const double duration = *std::max_element(w.infer_t, w.infer_t + w.n_infer) - w.start_t;  // preint.h:1544-1552
  if (!(duration > 0.0) || !std::isfinite(duration)) return fail(GORIO_UGPM_ERR_ARGUMENT, "inference time is not after start_t");
  double sf = std::max(w.state_freq, 5.0 / duration);  // preint.h:770-771
  sf = std::min(sf, std::min(vel_freq, gyr_freq));
  h.state_freq = sf;
  h.S = (int)(std::ceil(duration * sf) + (2 * w.overlap));  // preint.h:775
  if (h.S < 2 * w.overlap + 1 || h.S > kMaxStates) return fail(GORIO_UGPM_ERR_UNSUPPORTED, "number of GP states outside [2 overlap + 1, 160]");
  h.state_t.resize(h.S);
  const double t0 = w.start_t - (((double)w.overlap) / sf);
  for (int k = 0; k < h.S; ++k) h.state_t[k] = t0 + ((double)k) / sf;  // preint.h:777-783
  if (!(h.state_t[0] <= h.state_t.back())) return fail(GORIO_UGPM_ERR_ARGUMENT, "The argument of GyroVelData::Get are not consistent");
  slice(w.gyr_t, w.n_gyr, h.state_t[0], h.state_t.back(), h.g0, h.G);  // preint.h:789
  slice(w.vel_t, w.n_vel, h.state_t[0], h.state_t.back(), h.v0, h.V);
  if (h.G < 2 || h.V < 2) return fail(GORIO_UGPM_ERR_RANGE, "fewer than 2 gyro / velocity samples inside the state window");
  UgpmWin dummy;
  h.ws_doubles = carve(w, h, dummy, nullptr, nullptr, nullptr);
  return 0;
}

// the input arrays of a window in their SoA order -- gyr_t[G], gyr[3][G], vel_t[V], vel[3][V], infer_t[n_infer] -- from G gyro samples at
// g0 and V velocity samples at v0; returns the end of what it wrote (UGPM windows append state_t and the padding, LPM windows their time line)
inline double* stage_samples(double* dst, const gorio_ugpm_window& w, int g0, size_t G, int v0, size_t V) {
  for (size_t k = 0; k < G; ++k) dst[k] = w.gyr_t[g0 + k];
  dst += G;
  for (int a = 0; a < 3; ++a)
    for (size_t k = 0; k < G; ++k) dst[a * G + k] = w.gyr[3 * (size_t)(g0 + k) + a];
  dst += 3 * G;
  for (size_t k = 0; k < V; ++k) dst[k] = w.vel_t[v0 + k];
  dst += V;
  for (int a = 0; a < 3; ++a)
    for (size_t k = 0; k < V; ++k) dst[a * V + k] = w.vel[3 * (size_t)(v0 + k) + a];
  dst += 3 * V;
  for (int k = 0; k < w.n_infer; ++k) dst[k] = w.infer_t[k];
  return dst + w.n_infer;
}

// what both kinds of device window (UgpmWin, ug::LpmOutWin) take over from the request as it is
template <typename Win>
void copy_noise_and_priors(const gorio_ugpm_window& w, Win& u) {
  u.start_t = w.start_t; u.gyr_var = w.gyr_var; u.vel_var = w.vel_var;
  for (int a = 0; a < 3; ++a) { u.gyr_bias[a] = w.gyr_bias[a]; u.vel_bias[a] = w.vel_bias[a]; }
  u.vel_bias_std = w.vel_bias_std; u.gyr_bias_std = w.gyr_bias_std;
}

// ---- the fits of a batch that was enqueued without a look at the done flags (ugpm_api.hip run_fit): each fit got as many iterations
// as the previous batch needed.  `ints` are the control words of the batch as they come back with the results, kWinInts per window:
// the status word [16] is kStatusUnfinished where a fit was not done after those iterations (the kernels left that window alone from
// there on), and [kLmiNeed + p] is the number of iterations fit p needed where it was done.
struct FitOutcome {
  std::vector<int> rerun;  // windows to run again, with looks, in the order of the batch
  int need[2] = {0, 0};    // most iterations a finished window needed per fit; 0: no UGPM window finished that fit
};

inline FitOutcome fit_outcome(const int* ints, const std::vector<HostWin>& hw) {
  FitOutcome o;
  for (size_t i = 0; i < hw.size(); ++i) {
    if (hw[i].status != 0 || hw[i].is_lpm) continue;  // refused on the host, or not a UGPM window: no fit ran
    const int* f = ints + kWinInts * i;
    if (f[16] == kStatusUnfinished) o.rerun.push_back((int)i);
    if (f[16] != 0) continue;  // unfinished, or failed on the device
    for (int p = 0; p < 2; ++p) o.need[p] = std::max(o.need[p], f[kLmiNeed + p]);
  }
  return o;
}

// ---- which instantiations of the solver kernels a batch runs (ugpm_kernels.hip: CholLds<ROWS>, block_cholesky, blocked_lower_solve16<KMAX>).
// ROWS is the number of 16-column panel rows block_cholesky keeps in LDS, KMAX the number of 16 x 16 blocks of one block row a wave of
// blocked_lower_solve16 prefetches into registers.  The kernels were built for the largest system of the library (ROWS = 384, KMAX = 16);
// a window of S <= 160 states needs far less, and registers and LDS that hold nothing cost scratch traffic, waves per SIMD and room on the
// CU the scan matcher's kernels share (profiles/r21/gp_footprint.md).  A smaller instantiation runs the SAME instructions on the same data as the full one, under these conditions:
//   block_cholesky of an n x n system (+ 1 row where a right-hand side rides along): ROWS decides the look-ahead (`la`), which threads own
//   a panel row (`own`), the number of panel passes and the element-wise fall-back.  With me0 = n - min(16, n) + rhs, the rows of the first
//   (longest) panel, every one of them comes out as with 384 exactly when me0 <= ROWS (chol_same_path).  What is stored: the panel rows up
//   to the end of the last 16-row tile, the right-hand-side row behind the matrix rows (chol_rows_needed), and n <= ROWS + 16 inverse pivots;
//   blocked_lower_solve16 of n rows from block row jb: wave v multiplies blocks k = jb + v + 4 t < i <= ceil(n / 16) - 1, so every t >=
//   ceil((ceil(n / 16) - 1) / 4) fails the k < i test for every wave and block row (solve16_blocks_needed): those iterations load
//   predicated zeros and multiply nothing.
// The largest window of a batch decides for all of its windows: the needs grow with S, so a smaller window fits what the largest one fits.
constexpr int kSolveKmaxFull = 16;  // with kCholRowsFull (ugpm_device.h) the capacities every kernel had before they were sized; gorio_ugpm_debug_set_path bit 2 brings them back
constexpr int kGramRowsSmall = 96, kGramRows = 160;  // gram_kernel: n = S, and ceil16(S) rows of the solve's X in the same buffer
constexpr int kGramKmax = 3;                         // gram_kernel's solve: n = S <= 160, 10 block rows
constexpr int kLmRowsSmall = 192;                    // lm_step_kernel: n <= 3 S with the right-hand side, block_backward's 34 staging rows
constexpr int kSolveKmaxSmall = 8;                   // corr_diag_kernel, infer_kernel: n = 6 S

constexpr int ceil16(int v) { return (v + 15) / 16 * 16; }
// rows of the first panel of block_cholesky: what `la`, `own`, the pass count and the fall-back compare with ROWS
constexpr int chol_first_panel(int n, bool rhs) { return n - (n < 16 ? n : 16) + (rhs ? 1 : 0); }
constexpr bool chol_same_path(int rows, int n, bool rhs) { return chol_first_panel(n, rhs) <= rows; }
// panel rows written in one pass: the matrix rows padded to whole 16-row tiles, and with a right-hand side its row behind the m matrix rows
constexpr int chol_rows_needed(int n, bool rhs) {
  const int m = n - (n < 16 ? n : 16);
  return rhs ? (ceil16(m) > m + 1 ? ceil16(m) : m + 1) : ceil16(m);
}
constexpr int solve16_blocks_needed(int n) { return (ceil16(n) / 16 - 1 + 3) / 4; }
constexpr int gram_rows_needed(int S) { return chol_rows_needed(S, false) > ceil16(S) ? chol_rows_needed(S, false) : ceil16(S); }
constexpr int lm_rows_needed(int S) { return chol_rows_needed(3 * S, true) > 34 ? chol_rows_needed(3 * S, true) : 34; }
constexpr bool gram_fits(int rows, int S) { return gram_rows_needed(S) <= rows && chol_same_path(rows, S, false); }
// a fit's step factors 3 S unknowns (rotation) or S (one velocity channel); the right-hand side rides along below 384 unknowns
constexpr bool lm_fits(int rows, int S) { return 3 * S < kCholRowsFull && lm_rows_needed(S) <= rows && 3 * S <= rows + 16 && chol_same_path(rows, 3 * S, true) && chol_same_path(rows, S, true); }

struct SolverSizes {
  int gram_rows, gram_kmax;  // gram_kernel<ROWS, KMAX>
  int lm_rows;               // lm_step_kernel<ROWS>
  int solve_kmax;            // corr_diag_kernel<KMAX>, infer_kernel<KMAX>
};

// the instantiations for a batch whose largest window has max_S states; `full`: the capacities from before the sizing, for comparisons.
// Every branch ends in an instantiation that holds max_S <= kMaxStates (the static_asserts below); nothing is left to check at run time.
constexpr SolverSizes solver_sizes(int max_S, bool full) {
  if (full) return SolverSizes{kCholRowsFull, kSolveKmaxFull, kCholRowsFull, kSolveKmaxFull};
  return SolverSizes{gram_fits(kGramRowsSmall, max_S) ? kGramRowsSmall : kGramRows, kGramKmax, lm_fits(kLmRowsSmall, max_S) ? kLmRowsSmall : kCholRowsFull,
                     solve16_blocks_needed(6 * max_S) <= kSolveKmaxSmall ? kSolveKmaxSmall : kSolveKmaxFull};
}
static_assert(gram_fits(kGramRows, kMaxStates) && solve16_blocks_needed(kMaxStates) <= kGramKmax, "gram_kernel's capacities hold the largest window");
static_assert(solve16_blocks_needed(6 * kMaxStates) <= kSolveKmaxFull, "the full solve holds the largest correlation system");
static_assert(solver_sizes(66, false).gram_rows == kGramRowsSmall && solver_sizes(66, false).lm_rows == kLmRowsSmall && solver_sizes(66, false).solve_kmax == kSolveKmaxSmall,
              "the 66-state window of the scan-to-scan step runs the small instantiations");

// ---- opt.type = LPM (preint.h:1567-1580): host bookkeeping of one IterativeIntegrator = the merged, sorted time line
// (SortIndexTracker2, types.h:332-458) and the filler stamps of preint.h:228-237.  No numerics.
struct LpmHost {
  std::vector<double> tl;
  std::vector<int> kind, kidx, qpos, qorder, qrot;
  int start_index = 0, dt_index = 0;
};

inline void build_lpm_timeline(const gorio_ugpm_window& w, LpmHost& L) {
  struct Stamp { double t; int kind, idx; };
  std::vector<Stamp> st;
  st.reserve((size_t)w.n_infer + 2 + w.n_vel);
  for (int j = 0; j < w.n_infer; ++j) st.push_back({w.infer_t[j], 0, j});
  st.push_back({w.start_t, 1, 0});
  st.push_back({w.start_t + 0.01, 1, 1});  // kNumDtJacobianDelta, preint.h:216-219
  for (int i = 0; i < w.n_vel; ++i) st.push_back({w.vel_t[i], 2, i});
  auto by_time = [](const Stamp& a, const Stamp& b) { return a.t < b.t; };
  std::stable_sort(st.begin(), st.end(), by_time);
  // getSmallestGap() returns the LAST gap of the sorted line (types.h:442-450), preint.h:228
  if (st.size() >= 2 && (st.back().t - st[st.size() - 2].t) > (1.0 / w.min_freq)) {
    const double first = st.front().t, last = st.back().t;
    const int nb = (int)std::floor((last - first) * w.min_freq);
    if (nb > 0) {
      const double quantum = (last - first) / ((double)nb);
      for (int i = 0; i < nb; ++i) st.push_back({first + (i * quantum), 3, i});
      std::stable_sort(st.begin(), st.end(), by_time);
    }
  }
  const size_t T = st.size();
  L.tl.resize(T); L.kind.resize(T); L.kidx.resize(T);
  L.qpos.assign(w.n_infer, 0);
  L.qorder.clear();
  for (size_t r = 0; r < T; ++r) {
    L.tl[r] = st[r].t; L.kind[r] = st[r].kind; L.kidx[r] = st[r].idx;
    if (st[r].kind == 0) { L.qpos[st[r].idx] = (int)r; L.qorder.push_back(st[r].idx); }
    if (st[r].kind == 1 && st[r].idx == 0) L.start_index = (int)r;
    if (st[r].kind == 1 && st[r].idx == 1) L.dt_index = (int)r;
  }
  // preint_[g] = t.getVector(preint, g) (preint.h:259, types.h:378-387): the rotation part of record k of inner vector g is that of the
  // vector's k-th stamp IN SORTED ORDER; the position part is written by original index later (preint.h:640-664)
  L.qrot.assign(w.n_infer, 0);
  std::vector<int> group_of(w.n_infer, 0), first_of_group(1, 0);
  if (w.group_sizes && w.n_groups > 0) {
    int o = 0;
    first_of_group.clear();
    for (int g = 0; g < w.n_groups; ++g) {
      first_of_group.push_back(o);
      for (int k = 0; k < w.group_sizes[g] && o < w.n_infer; ++k) group_of[o++] = g;
    }
  }
  std::vector<int> filled(first_of_group.size(), 0);
  for (size_t r = 0; r < T; ++r)
    if (st[r].kind == 0) {
      const int g = group_of[st[r].idx];
      L.qrot[first_of_group[g] + filled[g]++] = (int)r;
    }
}

struct LpmSize {  // of one LPM window: doubles of input (samples, queries, time line), doubles of scratch, ints (time-line tables)
  size_t in = 0, scratch = 0, ints = 0;
};

// carve one LPM window (LpmWin = ug::LpmOutWin) with a time line of T stamps out of the three regions of the LPM workspace; returns what
// it used of each (called with null pointers for sizing)
template <typename LpmWin>
LpmSize carve_lpm(const gorio_ugpm_window& w, size_t T, LpmWin& u, const double* in, double* scratch, const int* ints) {
  LpmSize used;
  auto take_in = [&](size_t cnt) { return take_at(in, used.in, cnt); };
  auto take = [&](size_t cnt) { return take_at(scratch, used.scratch, cnt); };
  auto take_int = [&](size_t cnt) { return take_at(ints, used.ints, cnt); };
  const size_t G = w.n_gyr, V = w.n_vel, Q = w.n_infer;
  u.gyr_t = take_in(G); u.gyr = take_in(3 * G); u.vel_t = take_in(V); u.vel = take_in(3 * V); u.infer_t = take_in(Q); u.tl = take_in(T);
  u.kind = take_int(T); u.kidx = take_int(T); u.qpos = take_int(Q); u.qorder = take_int(Q); u.qrot = take_int(Q);
  u.E = take(45 * T); u.B = take(9 * T); u.cov3 = take(9 * T); u.dRdt = take(3 * T); u.dRdbw = take(9 * T);
  u.velr = take(3 * V); u.d_bw = take(18 * V); u.d_dt = take(3 * V); u.dp_shift = take(3 * Q);
  return used;
}

// the time-line tables of an LPM window in the order carve_lpm lays them out: kind[T], kidx[T], qpos[Q], qorder[Q], qrot[Q]
inline void stage_lpm_tables(int* dst, const LpmHost& L) {
  for (const std::vector<int>* v : {&L.kind, &L.kidx, &L.qpos, &L.qorder, &L.qrot}) dst = std::copy(v->begin(), v->end(), dst);
}

}  // namespace windows
}  // namespace gorio
