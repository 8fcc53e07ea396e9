// chemverse_optimal.hip — the device part of ChemVerse's ground-truth cost oracle (the reference's ChemistryEnvironment.
// compute_optimal_cost, xenoverse/chemverse/environment/api.py:1777-2266): for N candidates at once — a candidate is one
// synthesis route of one world, or one (one-pot charge, temperature) — the bisection on the scale of the layer-1 charge that
// _compute_chain_cost (:1903-1942, 30 iterations on [0.1, 1000]) and _compute_one_pot_cost (:2182-2217, 12 on [0.5, 200])
// run serially.  Host restatement, which is the specification, and everything that is rounded or priced:
// xenoverse_amd/chemverse/optimal_host.py.
//
// One launch is ONE pass: every candidate runs _simulate_chain (:1944-2109) once at its own scale — one experiment of the
// shared simulator (chemverse.hip chem_lane_run) per reaction of its route, products carried forward through a virtual pool —
// and then takes its own bisection decision.  lo, hi, best and the decision bits stay in device memory between passes; the
// C entry issues the passes back to back on the engine's stream with no host round trip: the bisection passes, the pass at
// scale_hi for candidates no scale has served yet, and the pass at best_scale that writes the per-step rows.  A launch is
// therefore bounded by one pass of the longest route, and every loop inside it by a launch-time bound: steps of a route <=
// l_stride <= XV_CHEM_CHAIN_MAX, charge entries <= k_stride, and the simulator's own bounds.
//
// Mapping: as chem_simulate_kernel — one lane per candidate, the 64 lanes of a workgroup of ONE world (cand_world < 0 pads).
// Lanes of a wave run different routes and diverge; no lane waits for another, the only atomic is the error word.  LDS is
// the simulator's c_stride * 640 bytes.  The virtual pool is in the handle's workspace [workgroup][chemical][lane], touched
// once per reaction of the route, the per-step rows go straight to the caller's arrays in the last pass.
//
// No decimal rounding happens here.  The reference compares round(yield, 6) >= min_yield_g; the caller passes the smallest
// double whose rounding passes (optimal_host.yield_threshold) and the kernel compares the unrounded yield with it.  The
// midpoint (lo + hi) / 2.0 is the same fp64 operation as the reference's, so equal decisions give a bit-equal best_scale.
#define XV_KERNELS_ONLY
#include "chemverse.hip"
#undef XV_KERNELS_ONLY

#define CHEM_PASS_PROBE XV_CHEM_BISECT_MAX            // the pass at scale_hi (:1930-1935)
#define CHEM_PASS_FINAL (XV_CHEM_BISECT_MAX + 1)      // the pass at best_scale (:1937)
#define CHEM_BIT_PROBE 31

struct ChemCand {
  const int32_t* cand_world;      // [n]; < 0: a padding lane
  const int32_t *n_step, *equipment, *target, *mode, *n_iter;      // [n]
  const double *threshold, *lo0, *hi0;                             // [n]
  const double *step_T, *step_dur;      // [n][ls]
  const int32_t* n_charge;              // [n][ls]
  const int32_t* charge;                // [n][ls][ks]: chemical | kind << 8
  double step_seconds;
  int n_cand, ls, ks;
};

struct ChemCandOut {
  double* best_scale;
  uint8_t* found;
  uint32_t* bits;
  double *yield, *charged, *consumed, *produced, *byproduct, *final_pool;
  uint8_t* failure;
};

struct ChemCandState {      // the handle's, per candidate slot
  double *vpool, *lo, *hi, *best;
  uint32_t* bits;      // [slot][2]: decision bits, found
};

__global__ __launch_bounds__(CHEM_LANES) void chem_optimal_pass_kernel(ChemWorlds W, ChemCand K, ChemCandOut O, ChemCandState S,
                                                                       int pass, double* __restrict__ ws_acc,
                                                                       int32_t* __restrict__ ws_fired, uint32_t* err_word) {
  extern __shared__ double chem_smem[];
  const int lane = threadIdx.x;
  const int cs = W.c_stride, rs = W.r_stride, ls = K.ls, ks = K.ks;
  double* s_pool = chem_smem;
  double* s_chem = chem_smem + (size_t)cs * CHEM_LANES;
  uint8_t* s_order = reinterpret_cast<uint8_t*>(s_chem + CHEM_F * cs);
  const int e0 = blockIdx.x * CHEM_LANES;
  const int e = e0 + lane;
  uint32_t err = 0u;

  int wb = K.cand_world[e0];
  if ((unsigned)wb >= (unsigned)W.n_world) { wb = 0; if (lane == 0) err |= XV_DEVERR_ACTION_RANGE; }
  const ChemWorldAt A = chem_stage_world(W, wb, lane, s_chem, &err);
  const int C = A.C;

  bool active = e < K.n_cand;
  if (active) {
    const int w = K.cand_world[e];
    if (w < 0) active = false;
    else if (w != wb) { active = false; err |= XV_DEVERR_ACTION_RANGE; }
  }
  if (!active) {
    if (err) atomicOr(err_word, err);
    return;      // no barrier follows
  }

  // the candidate's bisection state and this pass's scale
  int n_iter = K.n_iter[e];
  if (n_iter < 0 || n_iter > XV_CHEM_BISECT_MAX) { err |= XV_DEVERR_ACTION_RANGE; n_iter = n_iter < 0 ? 0 : XV_CHEM_BISECT_MAX; }
  double lo, hi, best;
  uint32_t bits, found;
  if (pass == 0) {
    lo = K.lo0[e]; hi = K.hi0[e]; best = 0.0; bits = 0u; found = 0u;
    if (!(isfinite(lo) && isfinite(hi))) { err |= XV_DEVERR_NONFINITE; lo = hi = 0.0; }
  } else {
    lo = S.lo[e]; hi = S.hi[e]; best = S.best[e]; bits = S.bits[2 * e]; found = S.bits[2 * e + 1];
  }
  const double threshold = K.threshold[e];
  if (threshold != threshold) err |= XV_DEVERR_NONFINITE;
  const bool final_pass = pass == CHEM_PASS_FINAL;
  bool run_it;
  double scale;
  if (pass < XV_CHEM_BISECT_MAX) { run_it = pass < n_iter; scale = (lo + hi) / 2.0; }
  else if (pass == CHEM_PASS_PROBE) { run_it = !found; scale = hi; }
  else { run_it = found != 0u; scale = best; }

  double yield = 0.0;
  if (run_it) {
    ChemLane L;
    L.pool = s_pool + lane;
    L.order = s_order + lane;
    L.chem = s_chem;
    L.cs = cs;
    L.C = C;
    double* acc = ws_acc + (size_t)blockIdx.x * CHEM_ACC * cs * CHEM_LANES + lane;
    int32_t* fired = ws_fired + (size_t)blockIdx.x * rs * CHEM_LANES + lane;
    double* vp = S.vpool + (size_t)blockIdx.x * cs * CHEM_LANES + lane;      // chemical c: vp[c * 64]
    for (int c = 0; c < C; ++c) vp[c * CHEM_LANES] = 0.0;
    int n_step = K.n_step[e];
    if (n_step < 0 || n_step > ls) { err |= XV_DEVERR_ACTION_RANGE; n_step = n_step < 0 ? 0 : ls; }
    int target = K.target[e];
    if ((unsigned)target >= (unsigned)C) { err |= XV_DEVERR_ACTION_RANGE; target = 0; }
    const int mode = K.mode[e];
    const ChemOut none = ChemOut();      // no history, no log
    int last_failure = 0;

    for (int s = 0; s < n_step; ++s) {      // _simulate_chain :1967-2095, one reaction of the route
      const size_t es = (size_t)e * ls + s;
      uint64_t member;
      chem_lane_clear(L, &member, acc, fired, A.R);
      int n_ch = K.n_charge[es];
      if (n_ch < 0 || n_ch > ks) { err |= XV_DEVERR_ACTION_RANGE; n_ch = n_ch < 0 ? 0 : ks; }
      for (int k = 0; k < n_ch; ++k) {      // :1968-1990: reactants, then catalysts; a chemical named twice is summed
        const int ent = K.charge[es * ks + k];
        const int c = ent & 0xff, kind = (ent >> 8) & 3;
        if ((unsigned)ent > 0x3ffu || c >= C) { err |= XV_DEVERR_ACTION_RANGE; continue; }
        const double g = kind == 0 ? scale : (kind == 1 ? scale * 0.1 : (kind == 2 ? scale * 5.0 : fmax(vp[c * CHEM_LANES], 0.01)));
        if (final_pass && O.charged) O.charged[es * ks + k] = g;
        if (!isfinite(g)) { err |= XV_DEVERR_NONFINITE; continue; }
        if ((member >> c) & 1ull) CHEM_POOL(L, c) += g;
        else chem_lane_charge(L, &member, c, g);
      }
      ChemRun run;
      run.T = K.step_T[es]; run.P = 1.0; run.duration = K.step_dur[es]; run.rate = 0.0; run.volume = 1.0;
      run.eq = K.equipment[e];
      chem_lane_run(W, A, L, member, acc, fired, K.step_seconds, run, none, e, &err);
      const int failure = run.failure;
      last_failure = failure;
      for (int c = 0; c < C; ++c) {      // the result dict's totals (simulator.py:780-806, :863-865), then :2067-2074
        const double consumed = (failure == 1 || failure == 2) ? 0.0 : CHEM_ACCUM(3, c);
        const double produced = failure ? 0.0 : CHEM_ACCUM(4, c);
        const double byproduct = failure ? 0.0 : CHEM_ACCUM(5, c);
        if (final_pass) {
          if (O.consumed) O.consumed[es * cs + c] = consumed;
          if (O.produced) O.produced[es * cs + c] = produced;
          if (O.byproduct) O.byproduct[es * cs + c] = byproduct;
        }
        double v = vp[c * CHEM_LANES];
        if (consumed > 1e-9) v = fmax(0.0, v - consumed);
        if (produced >= 0.001) v += produced;
        if (byproduct >= 0.001) v += byproduct;
        vp[c * CHEM_LANES] = v;
      }
      if (final_pass && O.failure) O.failure[es] = (uint8_t)failure;
    }
    if (mode == 0) {
      yield = vp[target * CHEM_LANES];      // :2097
    } else {      // the one-pot search reads the last experiment's pool (:2196)
      const double g = CHEM_POOL(L, target);
      yield = (n_step > 0 && last_failure == 0 && g > 1e-9) ? g : 0.0;
      if (final_pass && O.final_pool)
        for (int c = 0; c < C; ++c) {
          const double p = CHEM_POOL(L, c);
          O.final_pool[(size_t)e * cs + c] = (n_step > 0 && last_failure == 0 && p > 1e-9) ? p : 0.0;
        }
    }
    const bool ok = yield >= threshold;
    if (pass < XV_CHEM_BISECT_MAX) {      // :1921-1928
      if (ok) { best = scale; hi = scale; found = 1u; bits |= 1u << pass; }
      else lo = scale;
    } else if (pass == CHEM_PASS_PROBE && ok) {
      best = scale; found = 1u; bits |= 1u << CHEM_BIT_PROBE;
    }
  }
  if (final_pass) {
    if (O.best_scale) O.best_scale[e] = found ? best : 0.0;
    if (O.found) O.found[e] = (uint8_t)found;
    if (O.bits) O.bits[e] = bits;
    if (O.yield) O.yield[e] = yield;
  } else {
    S.lo[e] = lo; S.hi[e] = hi; S.best[e] = best; S.bits[2 * e] = bits; S.bits[2 * e + 1] = found;
  }
  if (err) atomicOr(err_word, err);
}

extern "C" int xv_chem_optimal(xv_chem* h, int n_cand, int l_stride, int k_stride, int n_pass, const int32_t* cand_world,
                               const int32_t* n_step, const int32_t* equipment, const int32_t* target, const int32_t* mode,
                               const int32_t* n_iter, const double* threshold, const double* scale_lo, const double* scale_hi,
                               const double* step_T, const double* step_duration, const int32_t* n_charge,
                               const int32_t* charge, double step_seconds, const xv_chem_opt_out* out, float* launch_ms) {
  XV_CHECK_ARG(h != nullptr && n_cand >= 1 && out != nullptr && l_stride >= 1 && k_stride >= 1);
  XV_CHECK_ARG(cand_world && n_step && equipment && target && mode && n_iter && threshold && scale_lo && scale_hi && step_T &&
               step_duration && n_charge && charge);
  XV_CHECK_ARG(step_seconds > 0.0 && step_seconds <= 1.7e308);
  XV_CHECK_ARG(n_pass >= 1 && n_pass <= XV_CHEM_BISECT_MAX);
  if (l_stride > XV_CHEM_CHAIN_MAX) {
    xv_set_error("xv_chem_optimal: l_stride = %d reactions per route is beyond the supported XV_CHEM_CHAIN_MAX = %d", l_stride,
                 XV_CHEM_CHAIN_MAX);
    return XV_ERR_UNSUPPORTED;
  }
  if (!h->worlds_set) {
    xv_set_error("xv_chem_optimal: no worlds set (xv_chem_set_worlds)");
    return XV_ERR_INVALID;
  }
  const int blocks = xv_div_up(n_cand, CHEM_LANES);
  if (blocks > h->blocks) {
    xv_set_error("xv_chem_optimal: n_cand = %d needs %d workgroups, the handle (capacity %d, %d worlds) serves %d", n_cand,
                 blocks, h->capacity, h->w.n_world, h->blocks);
    return XV_ERR_INVALID;
  }
  xv_engine* e = h->eng;
  XV_HIP(hipSetDevice(e->device));
  const size_t slots = (size_t)h->blocks * CHEM_LANES;
  if (!h->ws_opt) {      // freed with the rest of the workspace (set_worlds, destroy); both arrays or neither
    double* ws = nullptr;
    uint32_t* bits = nullptr;
    XV_HIP(hipMalloc(&ws, ((size_t)h->blocks * h->w.c_stride * CHEM_LANES + 3 * slots) * sizeof(double)));
    const hipError_t got = hipMalloc(&bits, 2 * slots * sizeof(uint32_t));
    if (got != hipSuccess) {
      (void)hipFree(ws);
      xv_set_error("xv_chem_optimal: hipMalloc of the decision bits failed: %s", hipGetErrorString(got));
      return XV_ERR_HIP;
    }
    h->ws_opt = ws;
    h->ws_opt_bits = bits;
  }
  ChemCandState s;
  s.vpool = h->ws_opt;
  s.lo = h->ws_opt + (size_t)h->blocks * h->w.c_stride * CHEM_LANES;
  s.hi = s.lo + slots;
  s.best = s.hi + slots;
  s.bits = h->ws_opt_bits;
  ChemCand k;
  k.cand_world = cand_world; k.n_step = n_step; k.equipment = equipment; k.target = target; k.mode = mode; k.n_iter = n_iter;
  k.threshold = threshold; k.lo0 = scale_lo; k.hi0 = scale_hi; k.step_T = step_T; k.step_dur = step_duration;
  k.n_charge = n_charge; k.charge = charge; k.step_seconds = step_seconds; k.n_cand = n_cand; k.ls = l_stride; k.ks = k_stride;
  ChemCandOut o;
  o.best_scale = out->best_scale; o.found = out->found; o.bits = out->bits; o.yield = out->yield; o.charged = out->charged;
  o.consumed = out->consumed; o.produced = out->produced; o.byproduct = out->byproduct; o.final_pool = out->final_pool;
  o.failure = out->failure;
  const size_t lds = (size_t)h->w.c_stride * (CHEM_LANES * sizeof(double) + CHEM_F * sizeof(double) + CHEM_LANES);
  const int n_launch = n_pass + 2;
  hipEvent_t ev[XV_CHEM_BISECT_MAX + 3];
  int n_ev = 0;      // timing (scripts/bench_chemverse_optimal.py): one event between launches, read after the last
  auto issue = [&]() -> int {
    if (launch_ms) {
      for (; n_ev <= n_launch; ++n_ev) XV_HIP(hipEventCreate(&ev[n_ev]));
      XV_HIP(hipEventRecord(ev[0], e->stream));
    }
    for (int i = 0; i < n_launch; ++i) {
      const int pass = i < n_pass ? i : (i == n_pass ? CHEM_PASS_PROBE : CHEM_PASS_FINAL);      // pass 0 starts the state
      hipLaunchKernelGGL(chem_optimal_pass_kernel, dim3((unsigned)blocks), dim3(CHEM_LANES), lds, e->stream, h->w, k, o, s,
                         pass, h->ws_acc, h->ws_fired, e->d_err);
      XV_LAUNCH_CHECK();
      if (launch_ms) XV_HIP(hipEventRecord(ev[i + 1], e->stream));
    }
    if (launch_ms) {
      XV_HIP(hipEventSynchronize(ev[n_launch]));
      for (int i = 0; i < n_launch; ++i) XV_HIP(hipEventElapsedTime(&launch_ms[i], ev[i], ev[i + 1]));
    }
    return XV_OK;
  };
  const int rc = issue();
  for (int i = 0; i < n_ev; ++i) (void)hipEventDestroy(ev[i]);      // also after a failure part of the way
  return rc;
}
