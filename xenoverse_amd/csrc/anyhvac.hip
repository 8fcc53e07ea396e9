// anyhvac.hip — AnyHVAC (include/xeno.h: xv_anyhvac_*): batched data-centre thermal rooms, one workgroup per room.
//
// Reference: anyhvac_env.py HVACEnv (control_type 'Temperature', no_switch_action=True, box actions); the bit-exact host
// restatement the tests compare with is xenoverse_amd/anyhvac/host.py.  One step is `iters` inner iterations of
//   A  per cooler (one lane each, strided past the block): bilinear read of the grid, push / pop of its delay ring, low-pass
//      filter, proportional controller, EER, float32 energy accumulator -> -eer, power_cool, power_vent in LDS
//   B  scatter: net_heat[cell] = static_heat[cell] + sum_c ((-eer_c) D_c[cell]) power_cool_c   (one lane per cell)
//               net_chtc[wall] = chtc[wall] + sum_c (V_c[wall] power_vent_c) eff_vent_c        (lanes strided over walls)
//      with the coolers in index order, which is the host's order of addition
//   C  5-point stencil into the other grid buffer
// with a workgroup barrier after each, the grid double-buffered in LDS, and the step's epilogue (time rounding,
// observation, reward, counters, flags, same-step autoreset) in the same launch.  Every product and sum is written in the
// host's order (the build has -ffp-contract=off), so device and host differ only by the last bits of exp, sin and cos and
// by the order of the float32 means of the reward.  Sums over lanes are fixed-shape trees in LDS: an env's result does not
// depend on the batch it runs in.
//
// The PID teacher (anyhvac_solver.py HVACSolverGTPID / LOCPID .policy; host restatement xenoverse_amd/anyhvac/pid.py) is
// hv_pid: lanes strided over the sensors form the float32 diff, advance the fp64 acc_diff and leave d_e in LDS; after one
// barrier lanes strided over the coolers sum d_e[s] corr[s][c] over the task's sensors in index order (a row of the
// row-major weights is read coalesced across c), clip, round to float32 and write 1 - value.  It is called by a kernel of
// its own (xv_anyhvac_pid_action) and, as the PID instantiation of the step kernel, in front of every step of a rollout.
//
// The RL action spaces (anyhvac_env.py HVACEnvDiscreteAction / HVACEnvDiffAction; host restatement
// xenoverse_amd/anyhvac/actions.py) are the step kernel's action mode AM: in the two mapped modes the lane that owns a
// cooler turns the raw input — a float32, or an int32 bin under the difference mode — into this step's value from the
// value the env applied at the step before, in the host's operations and order; the action cost keeps each cooler's last
// ten bins in one 64-bit word; the eight stat() counts are taken on the float32 readings of the observation.  All of it sits
// outside the iteration loop and uses the LDS the box kernel has (s_ne before the loop, s_red after it).
//
// The episode protocol of the reference's RL trainer (anyhvac_env.py reset :296-371, the cooler state history :256-294,
// reward :519-524, step :648-649; host restatement in host.py) is hv_reset: under an env's random-start flag one lane
// picks the start time — a uniform step, 100 steps before the env's last failure with the rest index of 100 history
// entries ago, or the reference's mixed draw (inverse CDF, or an upper-bound search of numpy's choice table) — and hands
// it to the workgroup through LDS.  The step's epilogue appends the rest index of every step that does not fail to a
// ring of XV_ANYHVAC_HISTORY int16 per env, remembers the time of every failing one, and under the no-terminate flag
// reports such a step as not terminated.  The flags are runtime data: the instantiations stay <INJECT, PID, AM>.
#include <cmath>
#include <new>

#include "philox.h"
#include "xv_common.h"

#define HV_BLOCK 256
#define HV_MAX_GRID 16
#define HV_MAX_C 320
#define HV_MAX_SH 640
#define HV_MAX_K 16
#define HV_MAX_WALL (17 * 17 * 2)
#define HV_DRAW_GRID 7u      // Philox purpose of the reset grid (sub-index: the cell)
#define HV_DRAW_START 8u     // ... of the episode start: (u0, u1) from one block of its own, so the grid does not move
#define HV_STEPS_BACK 100    // reset: restart this many steps before the last failure, from the rest index of then
#define HV_HIST_MASK (XV_ANYHVAC_HISTORY - 1)
#define HV_HIST_WRAP (1024 + XV_ANYHVAC_HISTORY)      // the count goes back by one ring here: it saturates, its slot does not move
#define HV_REST_SECONDS 3600.0
#define HV_MAX_HEAT 20000.0
#define HV_WINDOW_MASK ((1ull << 40) - 1)      // ten 4-bit entries: bin + 1, 0 = empty; the newest in the low bits

struct HvArgs {
  int NW, NL, C, S, H, KS, KH;      // padded sizes of the tables
  const double* tables;
  const int32_t* env_task;
  int n_task, n_env, iters, reward_mode;
  double dt, lb, ub, max_t;
  // state
  double *grid, *t, *last_call;
  int32_t *episode_step, *warning_count, *rest_idx;
  double* rest_start;
  float* value;
  double *filter, *ring_t, *ring_v;
  int32_t *head, *tail;
  uint32_t* err;
  uint64_t seed, gid_base, tick;
  const uint64_t* tick_dev;
  // the episode start (xv_anyhvac_set_start_mode / _set_start_draws): flags per env, the choice table, injected draws;
  // the time of the last failure and the rest indices of the last steps that did not fail
  const uint8_t* start_flags;
  const double *cdf, *start_u;
  long long n_cdf, max_steps;
  double* last_fail;
  int16_t* hist;
  int32_t* hist_n;
};

struct HvAct {      // the mapped action modes' arguments (xv_anyhvac_set_action_mode, xv_anyhvac_act_io)
  const int32_t* index;            // [T][n_env][C] bins, or null: io.action's floats are mapped
  float* applied;                  // [T][n_env][C] or null
  double *delta, *cost;            // [T][n_env][C], [T][n_env] or null
  int32_t* counts;                 // [T][n_env][XV_ANYHVAC_STAT_COUNTS] or null
  unsigned long long* window;      // [n_env][C]
  const double* table;             // [XV_ANYHVAC_ACT_BINS] the cost's non-zero-step term per bin
  int flags;
};

struct xv_anyhvac {
  xv_engine* eng;
  HvArgs a;
  int act_mode, act_flags;
  unsigned long long* act_window;
  double* act_table;
  // the PID teacher's arguments (xv_anyhvac_set_pid): weights, gains, arithmetic flag; the state it owns
  const double *pid_weights, *pid_gains;
  int pid_f64;
  double* pid_acc;
  float* pid_last_obs;
  int32_t* pid_fresh;
  uint8_t* start_flags;      // what a.start_flags, a.cdf point to (owned)
  double* cdf;
};

struct HvTask {      // one task's table, taken apart (layout: include/xeno.h)
  const double *sc, *base, *chtc, *hc, *sens, *heat, *hd, *cool, *cd, *cv;
  int nw, nl, nC, nS, nH, NL, NC, NWALL, KS, KH, srow, hrow, task;
};

__device__ __forceinline__ HvTask hv_task(const HvArgs& P, int env) {
  HvTask K;
  const int NC = P.NW * P.NL, NWALL = XV_ANYHVAC_NWALL(P.NW, P.NL);
  const size_t stride = (size_t)XV_ANYHVAC_TASK_DOUBLES(P.NW, P.NL, P.C, P.S, P.H, P.KS, P.KH);
  int task = P.env_task[env];
  task = task < 0 ? 0 : (task >= P.n_task ? P.n_task - 1 : task);
  const double* p = P.tables + (size_t)task * stride;
  K.task = task;
  K.NL = P.NL; K.NC = NC; K.NWALL = NWALL; K.KS = P.KS; K.KH = P.KH;
  K.srow = 8 + 3 * P.KS; K.hrow = 4 + 3 * P.KH;
  K.sc = p; p += 16;
  K.base = p; p += 3 * P.KH;
  K.chtc = p; p += NWALL;
  K.hc = p; p += NC;
  K.sens = p; p += (size_t)P.S * K.srow;
  K.heat = p; p += (size_t)P.H * K.hrow;
  K.hd = p; p += (size_t)P.H * NC;
  K.cool = p; p += (size_t)P.C * 24;
  K.cd = p; p += (size_t)P.C * NC;
  K.cv = p;
  // counts are clamped to the padded sizes: a table that lies cannot send an index out of its arrays
  K.nw = min(max((int)K.sc[0], 1), P.NW); K.nl = min(max((int)K.sc[1], 1), P.NL);
  K.nC = min(max((int)K.sc[2], 1), P.C); K.nS = min(max((int)K.sc[3], 1), P.S); K.nH = min(max((int)K.sc[4], 1), P.H);
  return K;
}

__device__ __forceinline__ int hv_cell(const HvTask& K, double a, double b) {      // a clipped cell of a table row -> LDS index
  const int i = min(max((int)a, 0), K.nw - 1), j = min(max((int)b, 0), K.nl - 1);
  return i * K.NL + j;
}

// RandomFourier.__call__: y = 0; y += a sin(order x) + b cos(order x), term after term
__device__ __forceinline__ double hv_series(const double* order, int K, int n, double x) {
  const double *a = order + K, *b = order + 2 * K;
  double y = 0.0;
  n = min(n, K);
  for (int j = 0; j < n; ++j) y = y + (a[j] * sin(order[j] * x) + b[j] * cos(order[j] * x));
  return y;
}

__device__ __forceinline__ double hv_curve(double heat_base, double period, int n, const double* order, int K, double t) {
  const double y = hv_series(order, K, n, t / period);
  return fmin(heat_base + fmax(y, 0.0), HV_MAX_HEAT);
}

__device__ __forceinline__ double hv_heater(const HvTask& K, int h, double t) {
  const double* r = K.heat + (size_t)h * K.hrow;
  const double base = hv_curve(K.sc[11], K.sc[12], (int)K.sc[13], K.base, K.KH, t);
  const double own = hv_curve(r[1], r[2], (int)r[3], r + 4, K.KH, t);
  return r[0] * base + (1.0 - r[0]) * own;
}

// the bilinear read both node kinds make: r = {s0, s1, d0, d1, k0, k1, ...}
__device__ __forceinline__ double hv_read(const HvTask& K, const double* g, const double* r) {
  const int ss = hv_cell(K, r[0], r[1]), ds = hv_cell(K, r[2], r[1]), sd = hv_cell(K, r[0], r[3]), dd = hv_cell(K, r[2], r[3]);
  const double k0 = r[4], k1 = r[5];
  return g[ss] * (1.0 - k0) * (1.0 - k1) + g[ds] * k0 * (1.0 - k1) + g[sd] * (1.0 - k0) * k1 + g[dd] * k0 * k1;
}

// sum over the block, a fixed tree: the same value in every lane, the same bits in every batch
__device__ __forceinline__ double hv_block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int o = HV_BLOCK / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] = red[tid] + red[tid + o];
    __syncthreads();
  }
  const double s = red[0];
  __syncthreads();
  return s;
}

struct HvObsOut {
  float *sensor, *heat, *atemp;
  int32_t* timestep;
};

__device__ __forceinline__ HvObsOut hv_obs_rows(float* sensor, float* heat, float* atemp, int32_t* timestep, size_t row,
                                                const HvArgs& P) {
  HvObsOut o;
  o.sensor = sensor ? sensor + row * P.S : nullptr;
  o.heat = heat ? heat + row * P.H : nullptr;
  o.atemp = atemp ? atemp + row * P.C : nullptr;
  o.timestep = timestep ? timestep + row : nullptr;
  return o;
}

// _get_obs: sensor readings, heater powers, set temperatures and the step index at time t; padded columns are zero.
// cnt (nullable): eight counters this lane's readings are added to, stat()'s thresholds.
// loss / hot (nullable): this lane's share of sum max(sqrt(d), d), d = clip(reading - target, 0, 8) in float32, and of the
// count of readings above the failure bound; keep (nullable): the readings once more, [P.S] in LDS, entry s by lane s % HV_BLOCK
__device__ __forceinline__ void hv_obs(const HvArgs& P, const HvTask& K, const double* g, double t, int rest, const float* value,
                                       const HvObsOut& o, double* loss, double* hot, float* keep = nullptr,
                                       int* cnt = nullptr) {
  const int tid = threadIdx.x;
  const float target = (float)K.sc[9];
  const double fub = K.sc[15];
  double ls = 0.0, ht = 0.0;
  for (int s = tid; s < P.S; s += HV_BLOCK) {
    float v = 0.0f;
    if (s < K.nS) {
      const double* r = K.sens + (size_t)s * K.srow;
      v = (float)(hv_read(K, g, r) + hv_series(r + 8, K.KS, (int)r[7], t / r[6]));
      const float d = fminf(fmaxf(v - target, 0.0f), 8.0f);
      ls += (double)fmaxf(sqrtf(d), d);
      ht += ((double)v > fub) ? 1.0 : 0.0;
      if (cnt) {      // stat(): reading - target in float32 against 0, +-2, +-4, +-6 (this lane's share)
        const float e = v - target;
        cnt[0] += e > 0.0f; cnt[1] += e > 2.0f; cnt[2] += e > 4.0f; cnt[3] += e > 6.0f;
        cnt[4] += e < 0.0f; cnt[5] += e < -2.0f; cnt[6] += e < -4.0f; cnt[7] += e < -6.0f;
      }
    }
    if (o.sensor) o.sensor[s] = v;
    if (keep) keep[s] = v;
  }
  if (loss) *loss = ls;
  if (hot) *hot = ht;
  if (o.heat)
    for (int h = tid; h < P.H; h += HV_BLOCK) o.heat[h] = h < K.nH ? (float)hv_heater(K, h, t) : 0.0f;
  if (o.atemp)
    for (int c = tid; c < P.C; c += HV_BLOCK) {
      float a = 0.0f;
      if (c < K.nC) a = c == rest ? -1.0f : value[c] * (float)(P.ub - P.lb) + (float)P.lb;
      o.atemp[c] = a;
    }
  if (o.timestep && tid == 0) *o.timestep = (int32_t)(t / ((double)P.iters * P.dt));
}

struct HvEnv {      // what every lane carries of its env (uniform) and of its coolers (c = tid, tid + HV_BLOCK)
  double t, last_call, rest_since;
  int episode_step, warning_count, rest, tail;
  double filt[2];
  int head[2];
};

// the time of the env's last failure and the count of its history, in LDS: lane 0 keeps them (the step's epilogue, the
// reset), every lane reads last_fail at a reset; they stay out of the registers the iteration loop carries
struct HvHist {
  double last_fail;
  int n;
};

// reset :301-323 under random_start_t, by ONE lane: the start time and the resting cooler of env; E holds the time and hs
// the last failure and the history count from before the reset.
//   generate_record             t = randint(0, max_steps) (iter_per_step sec_per_iter)
//   last_fail > 0, t < max_t    t = max(0, last_fail - 100 steps), the rest index of 100 steps ago (the oldest, if fewer)
//   otherwise                   u0 < 0.5: t = int((1 - sqrt(1 - u1)) max_t); else numpy's choice over p ~ 1 / (s + 1)^2:
//                               the count of cdf entries <= u1 (searchsorted, side='right')
template <bool INJECT>
__device__ __forceinline__ void hv_start(const HvArgs& P, const HvTask& K, int env, uint64_t tick, unsigned flags, bool back,
                                         const HvHist& hs, double* out) {
  double t, rest = 0.0;
  if (back) {
    t = fmax(0.0, hs.last_fail - (double)(HV_STEPS_BACK * P.iters) * P.dt);
    if (hs.n > 0) {
      const int at = hs.n >= HV_STEPS_BACK ? hs.n - HV_STEPS_BACK : 0;
      rest = (double)min(max((int)P.hist[(size_t)env * XV_ANYHVAC_HISTORY + (at & HV_HIST_MASK)], 0), K.nC - 1);
    }
  } else {
    double u0, u1;
    if (INJECT && P.start_u) {
      u0 = P.start_u[(size_t)env * 2];
      u1 = P.start_u[(size_t)env * 2 + 1];
    } else {
      const xv_u32x4 w = xv_env_draw_sub(P.seed, P.gid_base + (uint64_t)env, tick, HV_DRAW_START, 0u);
      u0 = xv_u53(w.x, w.y);
      u1 = xv_u53(w.z, w.w);
    }
    u1 = fmin(fmax(u1, 0.0), 0x1.fffffffffffffp-1);      // (an injected draw outside [0, 1), a NaN: into it)
    if (flags & XV_ANYHVAC_START_RECORD) {
      const long long k = min((long long)(u1 * (double)P.max_steps), P.max_steps - 1);
      t = (double)(k * (long long)P.iters) * P.dt;
    } else if (u0 < 0.5 || !P.cdf) {
      t = (double)(long long)((1.0 - __dsqrt_rn(1.0 - u1)) * P.max_t);
    } else {
      long long lo = 0, hi = P.n_cdf;      // upper bound: the first entry above u1
      while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (P.cdf[mid] <= u1) lo = mid + 1;
        else hi = mid;
      }
      t = (double)min(lo, P.n_cdf - 1);
    }
  }
  out[0] = t;
  out[1] = rest;
}

// HVACEnv.reset + Cooler.reset: grid into g (LDS), the rest into E and the env's global rows.  E.t comes in as the env's
// time before the reset, hs (LDS, settled by a barrier) as its last failure and history count: the restart-before-failure
// branch reads them.
template <bool INJECT>
__device__ __forceinline__ void hv_reset(const HvArgs& P, const HvTask& K, int env, uint64_t tick, const double* grid_in,
                                         double* g, HvEnv& E, HvHist& hs) {
  __shared__ double s_start[2];
  const int tid = threadIdx.x;
  if (tid < K.NC) {
    double v;
    if (INJECT) {
      v = grid_in[(size_t)env * K.NC + tid];
    } else {
      const xv_u32x4 w = xv_env_draw_sub(P.seed, P.gid_base + (uint64_t)env, tick, HV_DRAW_GRID, (uint32_t)tid);
      v = K.sc[8] + 2.0 * (double)xv_normal1(w.x, w.y);
    }
    g[tid] = v;
  }
  const unsigned flags = P.start_flags[env];
  const bool random = (flags & XV_ANYHVAC_START_RANDOM) != 0;      // uniform over the workgroup, as is all of E read here
  const bool back = random && !(flags & XV_ANYHVAC_START_RECORD) && hs.last_fail > 0.0 && E.t < P.max_t;
  if (random && tid == 0) {
    hv_start<INJECT>(P, K, env, tick, flags, back, hs, s_start);
    if (!back) hs.n = 0;      // (no other lane reads the count)
  }
  __syncthreads();
  double t0 = 0.0;
  int rest = 0;
  if (random) {
    t0 = s_start[0];
    rest = (int)s_start[1];
  }
  E.t = t0; E.last_call = NAN; E.rest_since = t0;
  E.episode_step = 0; E.warning_count = 0; E.rest = rest; E.tail = 0;
  const float dflt = (float)K.sc[14];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int c = tid + q * HV_BLOCK;
    E.filt[q] = 0.0; E.head[q] = 0;
    if (c < P.C) {
      P.value[(size_t)env * P.C + c] = dflt;
      P.rest_start[(size_t)env * P.C + c] = c == rest ? t0 : 0.0;
    }
  }
}

__device__ __forceinline__ void hv_load(const HvArgs& P, int env, double* g, HvEnv& E, HvHist& hs) {
  const int tid = threadIdx.x, NC = P.NW * P.NL;
  if (tid == 0) { hs.last_fail = P.last_fail[env]; hs.n = P.hist_n[env]; }
  if (tid < NC) g[tid] = P.grid[(size_t)env * NC + tid];
  E.t = P.t[env]; E.last_call = P.last_call[env];
  E.episode_step = P.episode_step[env]; E.warning_count = P.warning_count[env];
  E.rest = min(max(P.rest_idx[env], 0), P.C - 1); E.tail = P.tail[env];
  E.rest_since = P.rest_start[(size_t)env * P.C + E.rest];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int c = tid + q * HV_BLOCK;
    E.filt[q] = c < P.C ? P.filter[(size_t)env * P.C + c] : 0.0;
    E.head[q] = c < P.C ? P.head[(size_t)env * P.C + c] : 0;
  }
  __syncthreads();
}

__device__ __forceinline__ void hv_store(const HvArgs& P, int env, const double* g, const HvEnv& E, const HvHist& hs) {
  const int tid = threadIdx.x, NC = P.NW * P.NL;
  if (tid < NC) P.grid[(size_t)env * NC + tid] = g[tid];
  if (tid == 0) {
    P.t[env] = E.t; P.last_call[env] = E.last_call;
    P.episode_step[env] = E.episode_step; P.warning_count[env] = E.warning_count;
    P.rest_idx[env] = E.rest; P.tail[env] = E.tail;
    P.rest_start[(size_t)env * P.C + E.rest] = E.rest_since;
    P.last_fail[env] = hs.last_fail; P.hist_n[env] = hs.n;
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int c = tid + q * HV_BLOCK;
    if (c < P.C) {
      P.filter[(size_t)env * P.C + c] = E.filt[q];
      P.head[(size_t)env * P.C + c] = E.head[q];
    }
  }
}

__global__ __launch_bounds__(HV_BLOCK) void xv_anyhvac_act_reset_kernel(unsigned long long* window, int C, const uint8_t* mask) {
  const int env = blockIdx.x;
  if (mask && !mask[env]) return;
  for (int c = threadIdx.x; c < C; c += HV_BLOCK) window[(size_t)env * C + c] = 0ull;
}

template <bool INJECT>
__global__ __launch_bounds__(HV_BLOCK) void xv_anyhvac_reset_kernel(HvArgs P, const uint8_t* mask, const double* grid_in,
                                                                    xv_anyhvac_io io) {
  __shared__ double s_grid[HV_MAX_GRID * HV_MAX_GRID];
  const int env = blockIdx.x;
  if (mask && !mask[env]) return;
  const HvTask K = hv_task(P, env);
  __shared__ HvHist s_hist;
  HvEnv E;
  E.t = P.t[env];
  if (threadIdx.x == 0) { s_hist.last_fail = P.last_fail[env]; s_hist.n = P.hist_n[env]; }
  __syncthreads();
  hv_reset<INJECT>(P, K, env, xv_launch_tick(P.tick, P.tick_dev), grid_in, s_grid, E, s_hist);
  hv_obs(P, K, s_grid, E.t, E.rest, P.value + (size_t)env * P.C,
         hv_obs_rows(io.sensor_readings, io.heat_readings, io.action_temp, io.timestep, (size_t)env, P), nullptr, nullptr);
  hv_store(P, env, s_grid, E, s_hist);
}


// ---- the PID teacher ---------------------------------------------------------------------------------------------------
struct HvPid {
  const double* weights;      // [n_task][S][C] corr_sensor_cooler, padded rows and columns zero
  const double* gains;        // [n_env][3]: kp, ki, kd
  double* acc;                // [n_env][S] acc_diff
  float* last_obs;            // [n_env][S] last_observation
  int32_t* fresh;             // [n_env]: 1 from a reset to the first controller call
  int f64;                    // the gains are numpy.float64 scalars (all three products in fp64), not Python floats
  float* action_out;          // [T][n_env][C]
  float* flat_out;            // [n_env][2 C] or null (xv_anyhvac_pid_action)
  double* stats;              // [n_env][XV_ANYHVAC_PID_STATS] or null (xv_anyhvac_rollout_pid)
};

// One controller call of env.  obs[P.S]: the readings (entry s is read by lane s % HV_BLOCK only); act[P.C]: the env's
// action 1 - value, padded columns 0; flat (nullable): the reference's [switch[P.C], value[P.C]].  acc_diff and
// last_obs advance.  Every lane of the block calls it: there is one barrier inside.
//   diff = target - obs, last_diff = target - last_obs, dd = diff - last_diff              float32
//   d_e = -(kp diff - kd dd / delta_t + ki acc_diff): the first two products float32 under Python-float gains (numpy
//   rounds the gain and delta_t to float32), fp64 under numpy.float64 gains; ki acc_diff fp64 always
__device__ __forceinline__ void hv_pid(const HvArgs& P, const HvTask& K, const HvPid& D, int env, const float* obs, double* s_de,
                                       float* act, float* flat) {
  const int tid = threadIdx.x;
  const double* gn = D.gains + (size_t)env * 3;
  const double kp = gn[0], ki = gn[1], kd = gn[2];
  const double delta_t = (double)P.iters * P.dt / 60.0;
  const float target = (float)K.sc[9];
  double* acc = D.acc + (size_t)env * P.S;
  float* last = D.last_obs + (size_t)env * P.S;
  for (int s = tid; s < P.S; s += HV_BLOCK) {
    double de = 0.0;
    if (s < K.nS) {
      const float o = obs[s];
      const float diff = target - o, last_diff = target - last[s];
      const double a = acc[s] + (double)diff;
      acc[s] = a;
      last[s] = o;
      const float dd = diff - last_diff;
      double pd;
      if (D.f64) pd = kp * (double)diff - kd * (double)dd / delta_t;
      else pd = (double)((float)kp * diff - (float)kd * dd / (float)delta_t);
      de = -(pd + ki * a);
    }
    s_de[s] = de;
  }
  if (tid == 0) D.fresh[env] = 0;
  __syncthreads();
  const double* W = D.weights + (size_t)K.task * P.S * P.C;
  for (int c = tid; c < P.C; c += HV_BLOCK) {
    float a = 0.0f, sw = 0.0f, v = 0.0f;
    if (c < K.nC) {
      double x = 0.0;
      for (int s = 0; s < K.nS; ++s) x += s_de[s] * W[(size_t)s * P.C + c];
      sw = x > -0.05 ? 1.0f : 0.0f;
      v = x == x ? (float)fmin(fmax(x, 0.0), 1.0) : (float)x;
      a = 1.0f - v;
    }
    act[c] = a;
    if (flat) { flat[c] = sw; flat[P.C + c] = v; }
  }
}

__device__ __forceinline__ void hv_pid_clear(const HvArgs& P, const HvPid& D, int env) {
  for (int s = threadIdx.x; s < P.S; s += HV_BLOCK) {
    D.acc[(size_t)env * P.S + s] = 0.0;
    D.last_obs[(size_t)env * P.S + s] = 0.0f;
  }
  if (threadIdx.x == 0) D.fresh[env] = 1;
}

__device__ __forceinline__ double hv_block_max(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int o = HV_BLOCK / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] = fmax(red[tid], red[tid + o]);
    __syncthreads();
  }
  const double s = red[0];
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(HV_BLOCK) void xv_anyhvac_pid_reset_kernel(HvArgs P, HvPid D, const uint8_t* mask) {
  const int env = blockIdx.x;
  if (mask && !mask[env]) return;
  hv_pid_clear(P, D, env);
}

// one controller call per env without a step: the readings given, or the env's current observation (hv_obs of its grid
// and t: the function and inputs of the step's epilogue, so the same bits)
__global__ __launch_bounds__(HV_BLOCK) void xv_anyhvac_pid_kernel(HvArgs P, HvPid D, const float* readings) {
  __shared__ double s_grid[HV_MAX_GRID * HV_MAX_GRID];
  __shared__ double s_de[HV_MAX_SH];
  __shared__ float s_obs[HV_MAX_SH];
  const int env = blockIdx.x, tid = threadIdx.x;
  const HvTask K = hv_task(P, env);
  if (readings) {
    for (int s = tid; s < P.S; s += HV_BLOCK) s_obs[s] = readings[(size_t)env * P.S + s];
  } else {
    if (tid < K.NC) s_grid[tid] = P.grid[(size_t)env * K.NC + tid];
    __syncthreads();
    hv_obs(P, K, s_grid, P.t[env], 0, nullptr, hv_obs_rows(nullptr, nullptr, nullptr, nullptr, 0, P), nullptr, nullptr, s_obs);
  }
  hv_pid(P, K, D, env, s_obs, s_de, D.action_out + (size_t)env * P.C, D.flat_out ? D.flat_out + (size_t)env * 2 * P.C : nullptr);
}

// one mapped action of cooler c: the raw input and the value applied at the step before -> this step's value before the
// base step's clip (fp64), the bin taken (idx; 6 = no change) and whether the input was in range.  The host's operations
// in the host's order (actions.py): float32 v (ub - lb) + lb; under DIFF an fp64 add of the bin's step, the target - 3
// floor, / 0.1 in fp64; under DISCRETE / 0.1 in float32; round half to even, * 0.1 in fp64, back to a value.
template <int AM>
__device__ __forceinline__ double hv_map_action(const HvArgs& P, const HvTask& K, const HvAct& A, size_t at, const float* act_in,
                                                float last, int& idx, bool& ok) {
  const float span = (float)(P.ub - P.lb), lo = (float)P.lb;
  double temp;
  idx = (XV_ANYHVAC_ACT_BINS - 1) / 2;
  if (AM == XV_ANYHVAC_ACT_DIFF) {
    if (A.index) {
      const int i = A.index[at];
      ok = i >= 0 && i < XV_ANYHVAC_ACT_BINS;
      if (ok) idx = i;
    } else {
      const float raw = act_in[at];
      ok = raw == raw;
      if (ok) idx = (int)fminf(fmaxf(rintf(raw * (float)(XV_ANYHVAC_ACT_BINS - 1)), 0.0f), (float)(XV_ANYHVAC_ACT_BINS - 1));
    }
    temp = (double)(last * span + lo) + (-3.0 + 0.5 * (double)idx);
    const double floor_temp = K.sc[9] - 3.0;
    if ((A.flags & XV_ANYHVAC_ACT_TOO_COLD_LIMIT) && temp < floor_temp) temp = floor_temp;
    temp = rint(temp / 0.1) * 0.1;
  } else {
    const float raw = act_in[at];
    ok = raw == raw;
    temp = (double)rintf((raw * span + lo) / 0.1f) * 0.1;
  }
  return (temp - P.lb) / (P.ub - P.lb);
}

// adjacent nonzero sign reversals among a window's entries (bin + 1 per 4 bits; 7 is the zero step)
__device__ __forceinline__ int hv_reversals(unsigned long long w) {
  int n = 0;
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    const int a = (int)((w >> (4 * j)) & 15u), b = (int)((w >> (4 * j + 4)) & 15u);
    n += (a != 0 && b != 0 && ((a > 7 && b < 7) || (a < 7 && b > 7))) ? 1 : 0;
  }
  return n;
}

// PID: the teacher's controller call in front of every step (the action is D.action_out's row, not io.action's)
// AM: XV_ANYHVAC_ACT_BOX (the action row is the value), _DISCRETE, _DIFF (the row is mapped, hv_map_action)
template <bool INJECT, bool PID, int AM>
__global__ __launch_bounds__(HV_BLOCK) void xv_anyhvac_step_kernel(HvArgs P, xv_anyhvac_io io, const double* reset_grid,
                                                                   int mode, int T, HvPid D, HvAct A) {
  __shared__ double s_grid[2][HV_MAX_GRID * HV_MAX_GRID];
  __shared__ double s_static[HV_MAX_GRID * HV_MAX_GRID];
  __shared__ double s_chtc[HV_MAX_WALL];
  __shared__ double s_ne[HV_MAX_C], s_pc[HV_MAX_C], s_pv[HV_MAX_C], s_ev[HV_MAX_C];
  __shared__ float s_energy[HV_MAX_C];
  __shared__ double s_heat[HV_MAX_SH];
  __shared__ double s_red[HV_BLOCK];
  __shared__ int s_bad;
  __shared__ HvHist s_hist;
  __shared__ double s_de[PID ? HV_MAX_SH : 1];
  __shared__ float s_obs[PID ? HV_MAX_SH : 1];      // the readings the next controller call takes
  const int env = blockIdx.x, tid = threadIdx.x;
  const HvTask K = hv_task(P, env);
  const int NL = K.NL, NC = K.NC;
  const int ci = tid / NL, cj = tid - ci * NL;
  const bool cell_on = tid < NC && ci < K.nw && cj < K.nl;
  const double amb = K.sc[8], csa = K.sc[5] * K.sc[6], fcc_area = K.sc[7] * (K.sc[5] * K.sc[5]);
  const double hc = cell_on ? K.hc[tid] : 1.0;
  const size_t N = (size_t)P.n_env;
  float* value = P.value + (size_t)env * P.C;
  double* ring_t = P.ring_t + (size_t)env * XV_ANYHVAC_RING;
  double* ring_v = P.ring_v + (size_t)env * XV_ANYHVAC_RING * P.C;
  HvEnv E;
  int cur = 0;
  hv_load(P, env, s_grid[0], E, s_hist);
  const float* act_in = PID ? D.action_out : io.action;
  double st_abs = 0.0, st_max = 0.0, st_sq = 0.0, st_c1 = 0.0, st_c2 = 0.0, st_over = 0.0, st_rew = 0.0, st_n = 0.0;
  if (PID)
    hv_obs(P, K, s_grid[0], E.t, E.rest, value, hv_obs_rows(nullptr, nullptr, nullptr, nullptr, 0, P), nullptr, nullptr, s_obs);

  for (int ts = 0; ts < T; ++ts) {
    const size_t row = (size_t)ts * N + env;
    const HvEnv E0 = E;      // what a NaN puts back, with the grid as the env's global row has it
    if (tid == 0) s_bad = 0;
    if (ts > 0 && tid < NC) P.grid[(size_t)env * NC + tid] = s_grid[cur][tid];
    // -- _update_swith_action: the resting cooler hands over after MORE than an hour
    if (E.t - E.rest_since > HV_REST_SECONDS) {
      E.rest = E.rest + 1 > K.nC - 1 ? 0 : E.rest + 1;
      E.rest_since = E.t;
      if (tid == 0) P.rest_start[(size_t)env * P.C + E.rest] = E.t;
    }
    E.episode_step += 1;
    // -- heater powers at the step's starting t, held for all iterations
    for (int h = tid; h < P.H; h += HV_BLOCK) {
      const double p = h < K.nH ? hv_heater(K, h, E.t) : 0.0;
      s_heat[h] = p;
      if (io.heat_power) io.heat_power[row * P.H + h] = p;
    }
    // -- the teacher: readings -> PID -> this step's action row (column c is written by the lane that reads it below)
    if (PID) hv_pid(P, K, D, env, s_obs, s_de, D.action_out + row * P.C, nullptr);
    // -- this step's action: clipped float32, the resting cooler's replaced by the default value
    const bool cost_on = AM == XV_ANYHVAC_ACT_DIFF && (A.flags & XV_ANYHVAC_ACT_COST) != 0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int c = tid + q * HV_BLOCK;
      if (c < P.C) {
        float v;
        if (AM == XV_ANYHVAC_ACT_BOX) {
          v = act_in[row * P.C + c];
          v = fminf(fmaxf(v, 0.0f), 1.0f);
          if (!(v == v)) v = 0.0f;
        } else {      // padded columns keep their value and put out zeros
          v = value[c];
          double dl = 0.0;
          if (c < K.nC) {
            int idx;
            bool ok;
            const double x = hv_map_action<AM>(P, K, A, row * P.C + c, act_in, v, idx, ok);
            if (ok) v = (float)fmin(fmax(x, 0.0), 1.0);      // (out of range: the value keeps its bits, the bin is 6)
            else atomicOr(P.err, XV_DEVERR_ACTION_RANGE);
            if (AM == XV_ANYHVAC_ACT_DIFF) dl = -3.0 + 0.5 * (double)idx;
            if (cost_on) {
              unsigned long long* wp = A.window + (size_t)env * P.C + c;
              const unsigned long long w = ((*wp << 4) | (unsigned long long)(idx + 1)) & HV_WINDOW_MASK;
              *wp = w;
              s_ne[c] = 0.5 * A.table[idx] + 0.5 * ((double)hv_reversals(w) * 0.6);
            }
          }
          if (A.delta) A.delta[row * P.C + c] = dl;
        }
        if (c == E.rest) v = (float)K.sc[14];
        if (AM != XV_ANYHVAC_ACT_BOX && A.applied) A.applied[row * P.C + c] = c < K.nC ? v : 0.0f;
        value[c] = v;
        s_energy[c] = 0.0f;
        s_ev[c] = c < K.nC ? K.cool[(size_t)c * 24 + 8] : 0.0;
      }
    }
    __syncthreads();
    double act_cost = 0.0;      // -mean over the coolers in index order, by every lane (s_ne is free until the loop)
    if (cost_on) {
      double cs = 0.0;
      for (int c = 0; c < K.nC; ++c) cs += s_ne[c];
      act_cost = -(cs / (double)K.nC);
    }
    double heat_sum = 0.0;
    for (int h = tid; h < K.nH; h += HV_BLOCK) heat_sum += s_heat[h];
    heat_sum = hv_block_sum(heat_sum, s_red);      // current_heat_power (numpy sums pairwise: last bits may differ)
    if (cell_on) {
      double acc = 0.0;
      for (int h = 0; h < K.nH; ++h) acc += K.hd[(size_t)h * NC + tid] * s_heat[h];
      s_static[tid] = acc;
    }
    bool bad = false;

    for (int it = 0; it < P.iters; ++it) {
      const double* g = s_grid[cur];
      const double call_dt = E.last_call == E.last_call ? E.t - E.last_call : 0.0;
      // -- A: the coolers
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int c = tid + q * HV_BLOCK;
        if (c < K.nC) {
          const double* r = K.cool + (size_t)c * 24;
          const double cur_in = hv_read(K, g, r) + r[19];
          const int slot = E.tail & (XV_ANYHVAC_RING - 1);
          ring_v[(size_t)slot * P.C + c] = cur_in;
          if (c == 0) ring_t[slot] = E.t;
          const double delay = r[20], cutoff = E.t - delay;
          int head = E.head[q];
          if (E.tail - head >= XV_ANYHVAC_RING) head = E.tail - (XV_ANYHVAC_RING - 1);      // (a ring the caller sized wrongly)
          while (head < E.tail && ring_t[head & (XV_ANYHVAC_RING - 1)] < cutoff) ++head;
          E.head[q] = head;
          const double delayed = head < E.tail ? ring_v[(size_t)(head & (XV_ANYHVAC_RING - 1)) * P.C + c] : cur_in;
          const double alpha = call_dt > 0.0 ? exp(-call_dt / (delay / 3.0)) : 1.0;
          const double env_temp = alpha * E.filt[q] + (1.0 - alpha) * delayed;
          E.filt[q] = env_temp;
          double power_cool = 0.0, power_vent = 0.0;
          bool plain = true;      // the reference's power is a Python float here: resting, or the ratio clamped
          if (c != E.rest) {
            const double set_temp = (double)(value[c] * (float)(P.ub - P.lb) + (float)P.lb);
            const double temp_diff = env_temp - set_temp, ub = r[13], lb = r[14];
            double power_all;
            if (temp_diff > ub) power_all = (r[15] - r[16]) * 1.0 + r[16];
            else if (temp_diff < lb) power_all = (r[15] - r[16]) * 0.0 + r[16];
            else { power_all = (r[15] - r[16]) * ((temp_diff - lb) / (ub - lb)) + r[16]; plain = false; }
            const double pr = r[18] * power_all;
            const double m = r[17] > pr ? r[17] : pr;            // max(ratio * all, vent_min)
            power_vent = power_all < m ? power_all : m;          // min(., all)
            power_cool = power_all - power_vent;
          }
          const double diff_amb = amb - g[hv_cell(K, r[6], r[7])];
          double eer;
          if (diff_amb < 0.0) eer = r[12];
          else if (diff_amb < r[10]) eer = r[9];
          else if (diff_amb < r[11]) eer = r[9] * ((r[11] - diff_amb) / (r[11] - r[10]));
          else eer = 0.0;
          s_ne[c] = -eer; s_pc[c] = power_cool; s_pv[c] = power_vent;
          // float32 array += power * dt under numpy's promotion: a Python-float product is rounded to float32 and added
          // in float32, a numpy.float64 one is added in fp64 and the sum rounded (host.py)
          const double step_energy = (power_cool + power_vent) * P.dt;
          s_energy[c] = plain ? s_energy[c] + (float)step_energy : (float)((double)s_energy[c] + step_energy);
        }
      }
      E.last_call = E.t;
      E.tail += 1;
      __syncthreads();
      // -- B: scatter, coolers in index order
      double nh = 0.0;
      if (cell_on) {
        nh = s_static[tid];
        for (int c = 0; c < K.nC; ++c) nh += (s_ne[c] * K.cd[(size_t)c * NC + tid]) * s_pc[c];
      }
      for (int w = tid; w < K.NWALL; w += HV_BLOCK) {
        double a = K.chtc[w];
        for (int c = 0; c < K.nC; ++c) a += (K.cv[(size_t)c * K.NWALL + w] * s_pv[c]) * s_ev[c];
        s_chtc[w] = a;
      }
      __syncthreads();
      // -- C: the stencil, into the other buffer
      if (cell_on) {
        const double S = g[tid];
        const double up = ci > 0 ? g[tid - NL] : amb, down = ci < K.nw - 1 ? g[tid + NL] : amb;
        const double left = cj > 0 ? g[tid - 1] : amb, right = cj < K.nl - 1 ? g[tid + 1] : amb;
        const int w = (ci * (NL + 1) + cj) * 2;
        const double h0 = (-(S - up)) * s_chtc[w] * csa, h1 = (-(down - S)) * s_chtc[w + 2 * (NL + 1)] * csa;
        const double v0 = (-(S - left)) * s_chtc[w + 1] * csa, v1 = (-(right - S)) * s_chtc[w + 3] * csa;
        const double net_in = ((h0 - h1) + (v0 - v1)) + fcc_area * (amb - S);
        bad = bad || nh != nh || net_in != net_in;
        s_grid[cur ^ 1][tid] = S + (nh + net_in) / hc * P.dt;
      }
      cur ^= 1;
      E.t += P.dt;
      __syncthreads();
    }
    E.t = E.t >= 0.0 ? (double)(long long)(E.t + 0.5) : (double)(long long)(E.t - 0.5);
    if (bad) atomicOr(&s_bad, 1);
    __syncthreads();
    const bool nonfinite = s_bad != 0;
    if (nonfinite) {      // the reference raises: the grid, time and counters go back to the step's start
      if (tid < NC) s_grid[cur][tid] = P.grid[(size_t)env * NC + tid];
      E = E0;
      if (tid == 0) atomicOr(P.err, XV_DEVERR_NONFINITE);
      __syncthreads();
    }
    // -- observation, reward, flags
    double loss, hot;
    int cnt[XV_ANYHVAC_STAT_COUNTS] = {0, 0, 0, 0, 0, 0, 0, 0};
    hv_obs(P, K, s_grid[cur], E.t, E.rest, value,
           hv_obs_rows(io.sensor_readings, io.heat_readings, io.action_temp, io.timestep, row, P), &loss, &hot,
           PID ? s_obs : nullptr, AM != XV_ANYHVAC_ACT_BOX ? cnt : nullptr);
    if (AM != XV_ANYHVAC_ACT_BOX && A.counts) {      // four counts (<= 640 each) per fp64 sum, 12 bits apart: exact
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int* n = cnt + 4 * half;
        const double packed = (double)((long long)n[0] | ((long long)n[1] << 12) | ((long long)n[2] << 24) | ((long long)n[3] << 36));
        const long long tot = (long long)hv_block_sum(packed, s_red);
        if (tid == 0)
          for (int i = 0; i < 4; ++i) A.counts[row * XV_ANYHVAC_STAT_COUNTS + 4 * half + i] = (int32_t)((tot >> (12 * i)) & 4095);
      }
    }
    if (PID && D.stats) {      // e = reading - target in float32, over the real sensors (this lane's entries of s_obs)
      const float target = (float)K.sc[9], over = (float)(K.sc[9] + 2.0);
      for (int s = tid; s < K.nS; s += HV_BLOCK) {
        const double ae = (double)fabsf(s_obs[s] - target);
        st_abs += ae; st_max = fmax(st_max, ae); st_sq += ae * ae;
        st_c1 += ae <= 1.0 ? 1.0 : 0.0; st_c2 += ae <= 2.0 ? 1.0 : 0.0;
        st_over += s_obs[s] > over ? 1.0 : 0.0; st_n += 1.0;
      }
    }
    loss = hv_block_sum(loss, s_red);
    hot = hv_block_sum(hot, s_red);
    double psum = 0.0;
    const float span = (float)(P.dt * (double)P.iters);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int c = tid + q * HV_BLOCK;
      if (c < P.C) {
        const float p = c < K.nC ? s_energy[c] / span : 0.0f;
        if (io.cool_power) io.cool_power[row * P.C + c] = p;
        psum += (double)p;
      }
    }
    psum = hv_block_sum(psum, s_red);
    float target_cost = -0.5f * (float)(loss / (double)K.nS);
    const float power = (float)(psum / (double)K.nC);
    double energy_cost = -3.0 * (K.sc[10] / heat_sum) * (double)(power / 10000.0f);
    if (P.reward_mode == 1) { energy_cost = energy_cost * 1.25; target_cost = target_cost * 0.75f; }
    else if (P.reward_mode == 2) { energy_cost = energy_cost * 1.5; target_cost = target_cost * 0.5f; }
    int overheat = 0, over_tol = 0;
    double reward;
    if (hot > 0.0 && E.episode_step > 5) {
      overheat = 1;
      E.warning_count = min(5 + 1, E.warning_count + 1);
    } else {
      E.warning_count = max(E.warning_count - 1, 0);
    }
    int term = 0;
    if (E.warning_count > 5) {      // reward :519-522: the failure is remembered; step :648: a flagged env goes on
      over_tol = 1; reward = -30.0;
      term = (P.start_flags[env] & XV_ANYHVAC_START_NO_TERMINATE) ? 0 : 1;
      if (!nonfinite && tid == 0) s_hist.last_fail = E.t;
    } else {
      reward = (double)(1.0f + target_cost) + 0.0 + energy_cost + 0.0 + (overheat ? -10.0 : 0.0);
      if (!nonfinite && tid == 0) {      // _save_cooler_state_history: a step that did not fail leaves its rest index
        const int n = s_hist.n;
        P.hist[(size_t)env * XV_ANYHVAC_HISTORY + (n & HV_HIST_MASK)] = (int16_t)E.rest;
        s_hist.n = n + 1 >= HV_HIST_WRAP ? n + 1 - XV_ANYHVAC_HISTORY : n + 1;
      }
    }
    if (cost_on) reward = reward + act_cost;      // (the failure reward too, as the reference)
    int trunc = E.t >= P.max_t ? 1 : 0;
    if (nonfinite) { reward = NAN; term = 0; trunc = 0; E.warning_count = E0.warning_count; }
    if (PID) st_rew += reward;
    if (tid == 0) {
      io.reward[row] = reward;
      io.terminated[row] = (uint8_t)term;
      io.truncated[row] = (uint8_t)trunc;
      if (AM != XV_ANYHVAC_ACT_BOX && A.cost) A.cost[row] = act_cost;
      if (io.misc) {
        double* m = io.misc + row * 8;
        m[0] = overheat; m[1] = over_tol; m[2] = energy_cost; m[3] = (double)target_cost; m[4] = E.t; m[5] = E.rest;
        m[6] = E.warning_count; m[7] = E.episode_step;
      }
    }
    const bool redo = (term || trunc) && mode == XV_AUTORESET_SAME_STEP;
    const HvObsOut fin = hv_obs_rows(io.final_sensor_readings, io.final_heat_readings, io.final_action_temp, io.final_timestep,
                                     row, P);
    if (redo) {
      hv_obs(P, K, s_grid[cur], E.t, E.rest, value, fin, nullptr, nullptr);
      __syncthreads();
      hv_reset<INJECT>(P, K, env, xv_launch_tick(P.tick, P.tick_dev) + (uint64_t)ts, reset_grid, s_grid[cur], E, s_hist);
      hv_obs(P, K, s_grid[cur], E.t, E.rest, value,
             hv_obs_rows(io.sensor_readings, io.heat_readings, io.action_temp, io.timestep, row, P), nullptr, nullptr,
             PID ? s_obs : nullptr);
      if (PID) hv_pid_clear(P, D, env);      // the new episode starts with a fresh controller
      if (AM != XV_ANYHVAC_ACT_BOX)          // ... and an empty window (each lane its own coolers' words)
        for (int c = tid; c < P.C; c += HV_BLOCK) A.window[(size_t)env * P.C + c] = 0ull;
    } else {
      if (fin.sensor) for (int s = tid; s < P.S; s += HV_BLOCK) fin.sensor[s] = 0.0f;
      if (fin.heat) for (int h = tid; h < P.H; h += HV_BLOCK) fin.heat[h] = 0.0f;
      if (fin.atemp) for (int c = tid; c < P.C; c += HV_BLOCK) fin.atemp[c] = 0.0f;
      if (fin.timestep && tid == 0) *fin.timestep = 0;
    }
    __syncthreads();
  }
  hv_store(P, env, s_grid[cur], E, s_hist);
  if (PID && D.stats) {      // lane partials over the T steps, then one fixed tree each: the same bits in any batch
    double* st = D.stats + (size_t)env * XV_ANYHVAC_PID_STATS;
    const double sums[6] = {st_abs, st_sq, st_c1, st_c2, st_over, st_n};
    double red[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) red[i] = hv_block_sum(sums[i], s_red);
    const double mx = hv_block_max(st_max, s_red);
    if (tid == 0) {
      st[0] += red[0]; st[1] = fmax(st[1], mx); st[2] += red[1]; st[3] += red[2]; st[4] += red[3]; st[5] += red[4];
      st[6] += st_rew; st[7] += red[5];
    }
  }
}

#ifndef XV_KERNELS_ONLY
// ---- host side of the C-ABI ---------------------------------------------------------------------------------------
#include <cstddef>
#include <initializer_list>

static void hv_bind_rng(xv_anyhvac* h, uint64_t ticks) {
  h->a.seed = h->eng->seed;
  h->a.gid_base = h->eng->env_id_base;
  const XvTickBind b = xv_engine_bind_tick(h->eng, ticks);
  h->a.tick = b.tick;
  h->a.tick_dev = b.tick_dev;
}

__global__ void xv_anyhvac_fill_kernel(double* p, size_t n, double v) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

static hipError_t hv_fill(double* p, size_t n, double v, hipStream_t stream) {
  hipLaunchKernelGGL(xv_anyhvac_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p, n, v);
  return hipGetLastError();
}

// ---- the handle's device buffers ---------------------------------------------------------------------------------------
// Every buffer the handle owns, once: create, the lazy allocations of set_action_mode and set_pid, destroy and the four
// get/set copies all walk this table.  A buffer with `state` is one of its group's get/set pointers, in the table's order
// (the env group: xv_anyhvac_state's fields; the others: the positional arguments of xv_anyhvac_<group>_get_state).
enum { HV_ENV, HV_START, HV_ACT, HV_PID };
struct HvBuf {
  size_t slot;                         // where the handle keeps the pointer
  size_t (*bytes)(const HvArgs& a);    // of the whole buffer, from the handle's dims
  int fill;                            // the byte a new buffer is filled with; -1: who allocates it writes every entry
  int group;
  bool state;
};
#define HV_SLOT(member) offsetof(xv_anyhvac, member)
#define HV_PER_ENV(x) [](const HvArgs& a) -> size_t { return (size_t)a.n_env * (size_t)(x); }
#define HV_SHARED(x) [](const HvArgs& a) -> size_t { return (size_t)(x); }
static const HvBuf HV_BUFS[] = {
    {HV_SLOT(a.grid), HV_PER_ENV(a.NW * a.NL * 8), 0, HV_ENV, true},
    {HV_SLOT(a.t), HV_PER_ENV(8), 0, HV_ENV, true},
    {HV_SLOT(a.last_call), HV_PER_ENV(8), 0xFF, HV_ENV, true},      // (0xFF bytes: a NaN, "no last call")
    {HV_SLOT(a.episode_step), HV_PER_ENV(4), 0, HV_ENV, true},
    {HV_SLOT(a.warning_count), HV_PER_ENV(4), 0, HV_ENV, true},
    {HV_SLOT(a.rest_idx), HV_PER_ENV(4), 0, HV_ENV, true},
    {HV_SLOT(a.rest_start), HV_PER_ENV(a.C * 8), 0, HV_ENV, true},
    {HV_SLOT(a.value), HV_PER_ENV(a.C * 4), 0, HV_ENV, true},
    {HV_SLOT(a.filter), HV_PER_ENV(a.C * 8), 0, HV_ENV, true},
    {HV_SLOT(a.ring_t), HV_PER_ENV(XV_ANYHVAC_RING * 8), 0, HV_ENV, true},
    {HV_SLOT(a.ring_v), HV_PER_ENV(XV_ANYHVAC_RING * a.C * 8), 0, HV_ENV, true},
    {HV_SLOT(a.head), HV_PER_ENV(a.C * 4), 0, HV_ENV, true},
    {HV_SLOT(a.tail), HV_PER_ENV(4), 0, HV_ENV, true},
    {HV_SLOT(a.last_fail), HV_PER_ENV(8), 0, HV_START, true},       // (create goes on to fill it with -1.0)
    {HV_SLOT(a.hist), HV_PER_ENV(XV_ANYHVAC_HISTORY * 2), 0, HV_START, true},
    {HV_SLOT(a.hist_n), HV_PER_ENV(4), 0, HV_START, true},
    {HV_SLOT(start_flags), HV_PER_ENV(1), 0, HV_START, false},
    {HV_SLOT(cdf), HV_SHARED(a.n_cdf * 8), -1, HV_START, false},    // (no bytes until xv_anyhvac_set_start_mode brings a table)
    {HV_SLOT(act_window), HV_PER_ENV(a.C * 8), 0, HV_ACT, true},
    {HV_SLOT(act_table), HV_SHARED(XV_ANYHVAC_ACT_BINS * 8), -1, HV_ACT, false},      // (set_action_mode writes it)
    {HV_SLOT(pid_acc), HV_PER_ENV(a.S * 8), -1, HV_PID, true},      // (xv_anyhvac_pid_reset writes the three)
    {HV_SLOT(pid_last_obs), HV_PER_ENV(a.S * 4), -1, HV_PID, true},
    {HV_SLOT(pid_fresh), HV_PER_ENV(4), -1, HV_PID, true},
};
#undef HV_SLOT
#undef HV_PER_ENV
#undef HV_SHARED
static const int HV_N_BUFS = (int)(sizeof(HV_BUFS) / sizeof(HV_BUFS[0]));
static_assert(sizeof(HV_BUFS) / sizeof(HV_BUFS[0]) <= 32, "hv_free and hv_alloc keep a bit per buffer in 32");

static void** hv_slot(xv_anyhvac* h, const HvBuf& b) { return (void**)((char*)h + b.slot); }

static void hv_free(xv_anyhvac* h, uint32_t which) {      // which: a bit per entry of HV_BUFS
  for (int i = 0; i < HV_N_BUFS; ++i) {
    void** p = hv_slot(h, HV_BUFS[i]);
    if ((which >> i & 1u) && *p) { (void)hipFree(*p); *p = nullptr; }
  }
}

// Allocate what `group` still lacks and fill what is new, with `clear` every buffer of the group that has a fill byte.
// A failure frees what this call allocated: the group is then as it was.
static hipError_t hv_alloc(xv_anyhvac* h, int group, bool clear) {
  uint32_t made = 0;
  hipError_t r = hipSuccess;
  for (int i = 0; i < HV_N_BUFS && r == hipSuccess; ++i) {
    const HvBuf& b = HV_BUFS[i];
    const size_t bytes = b.bytes(h->a);
    void** p = hv_slot(h, b);
    if (b.group != group || bytes == 0) continue;
    bool fill = clear;
    if (!*p) {
      r = hipMalloc(p, bytes);
      if (r != hipSuccess) { *p = nullptr; break; }
      made |= 1u << i;
      fill = true;
    }
    if (fill && b.fill >= 0) r = hipMemsetAsync(*p, b.fill, bytes, h->eng->stream);
  }
  if (r != hipSuccess) hv_free(h, made);
  return r;
}

// get (set false) or set a group's state: user[i] goes with the group's i-th state buffer, a null pointer is skipped
static int hv_copy(xv_anyhvac* h, int group, std::initializer_list<const void*> user, bool set) {
  XV_CHECK_ARG(h);
  const void* const* u = user.begin();
  for (const HvBuf& b : HV_BUFS) {
    if (b.group != group || !b.state) continue;
    void* own = *hv_slot(h, b);
    void* usr = const_cast<void*>(*u++);
    XV_CHECK_ARG(own != nullptr);      // (the act and pid groups exist from xv_anyhvac_set_action_mode / _set_pid on)
    if (usr) XV_HIP(hipMemcpyAsync(set ? own : usr, set ? usr : own, b.bytes(h->a), hipMemcpyDeviceToDevice, h->eng->stream));
  }
  return XV_OK;
}

extern "C" int xv_anyhvac_destroy(xv_anyhvac* h) {
  if (!h) return XV_OK;
  (void)hipSetDevice(h->eng->device);
  (void)hipStreamSynchronize(h->eng->stream);
  hv_free(h, ~0u);
  delete h;
  return XV_OK;
}

extern "C" int xv_anyhvac_create(xv_engine* e, int n_env, int NW, int NL, int C, int S, int H, int KS, int KH,
                                 int iter_per_step, double sec_per_iter, double set_lower_bound, double set_upper_bound,
                                 double max_t, int reward_mode, xv_anyhvac** out) {
  XV_CHECK_ARG(out != nullptr);
  *out = nullptr;
  XV_CHECK_ARG(e && n_env > 0 && NW > 0 && NL > 0 && C > 0 && S > 0 && H > 0 && KS > 0 && KH > 0 && iter_per_step > 0);
  XV_CHECK_ARG(sec_per_iter > 0.0 && set_upper_bound > set_lower_bound && reward_mode >= 0 && reward_mode <= 2);
  if (NW > HV_MAX_GRID || NL > HV_MAX_GRID || C > HV_MAX_C || S > HV_MAX_SH || H > HV_MAX_SH || KS > HV_MAX_K || KH > HV_MAX_K) {
    xv_set_error("xv_anyhvac_create: NW, NL <= %d, C <= %d, S, H <= %d, KS, KH <= %d (got %d x %d, C %d, S %d, H %d, KS %d, KH %d)",
                 HV_MAX_GRID, HV_MAX_C, HV_MAX_SH, HV_MAX_K, NW, NL, C, S, H, KS, KH);
    return XV_ERR_UNSUPPORTED;
  }
  XV_HIP(hipSetDevice(e->device));
  xv_anyhvac* h = new (std::nothrow) xv_anyhvac();
  if (!h) {
    xv_set_error("xv_anyhvac_create: out of host memory");
    return XV_ERR_NOMEM;
  }
  h->eng = e;
  HvArgs& a = h->a;      // value-initialised: every pointer is null until it is set here
  a.NW = NW; a.NL = NL; a.C = C; a.S = S; a.H = H; a.KS = KS; a.KH = KH;
  a.n_env = n_env; a.iters = iter_per_step; a.reward_mode = reward_mode;
  a.dt = sec_per_iter; a.lb = set_lower_bound; a.ub = set_upper_bound; a.max_t = max_t;
  a.err = e->d_err;
  hipError_t r = hv_alloc(h, HV_ENV, false);
  if (r == hipSuccess) r = hv_alloc(h, HV_START, false);
  if (r == hipSuccess) r = hv_fill(a.last_fail, (size_t)n_env, -1.0, e->stream);      // last_fail_timestemp = -1: no failure yet
  if (r != hipSuccess) {
    xv_set_error("xv_anyhvac_create: device allocation failed: %s", hipGetErrorString(r));
    (void)xv_anyhvac_destroy(h);
    return XV_ERR_HIP;
  }
  a.start_flags = h->start_flags;
  a.max_steps = 1;
  *out = h;
  return XV_OK;
}

extern "C" int xv_anyhvac_set_task(xv_anyhvac* h, int n_task, const double* tables, const int32_t* env_task) {
  XV_CHECK_ARG(h && n_task > 0 && tables && env_task);
  h->a.n_task = n_task;
  h->a.tables = tables;
  h->a.env_task = env_task;
  return XV_OK;
}

// ---- the episode start -------------------------------------------------------------------------------------------------
extern "C" int xv_anyhvac_set_start_mode(xv_anyhvac* h, const uint8_t* flags, int64_t max_steps, const double* choice_cdf,
                                         int64_t n_cdf) {
  XV_CHECK_ARG(h && flags && max_steps > 0 && (!choice_cdf || n_cdf > 0));
  const uint8_t all = XV_ANYHVAC_START_RANDOM | XV_ANYHVAC_START_RECORD | XV_ANYHVAC_START_NO_TERMINATE;
  bool choice = false;
  for (int i = 0; i < h->a.n_env; ++i) {
    XV_CHECK_ARG((flags[i] & ~all) == 0);
    choice = choice || (flags[i] & (XV_ANYHVAC_START_RANDOM | XV_ANYHVAC_START_RECORD)) == XV_ANYHVAC_START_RANDOM;
  }
  XV_CHECK_ARG(!choice || choice_cdf || h->cdf);      // (an env that may take the choice branch needs its table)
  XV_HIP(hipSetDevice(h->eng->device));
  XV_HIP(hipStreamSynchronize(h->eng->stream));       // launches in flight keep the flags and the table they were given
  if (choice_cdf) {
    if (h->cdf && h->a.n_cdf != n_cdf) {
      XV_HIP(hipFree(h->cdf));
      h->cdf = nullptr; h->a.cdf = nullptr; h->a.n_cdf = 0;
    }
    if (!h->cdf) XV_HIP(hipMalloc((void**)&h->cdf, (size_t)n_cdf * sizeof(double)));
    XV_HIP(hipMemcpy(h->cdf, choice_cdf, (size_t)n_cdf * sizeof(double), hipMemcpyHostToDevice));
    h->a.cdf = h->cdf;
    h->a.n_cdf = n_cdf;
  }
  XV_HIP(hipMemcpy(h->start_flags, flags, (size_t)h->a.n_env, hipMemcpyHostToDevice));
  h->a.max_steps = max_steps;
  return XV_OK;
}

extern "C" int xv_anyhvac_set_start_draws(xv_anyhvac* h, const double* u) {
  XV_CHECK_ARG(h);
  h->a.start_u = u;
  return XV_OK;
}

extern "C" int xv_anyhvac_start_get_state(xv_anyhvac* h, double* last_fail, int16_t* ring, int32_t* count) {
  return hv_copy(h, HV_START, {last_fail, ring, count}, false);
}
extern "C" int xv_anyhvac_start_set_state(xv_anyhvac* h, const double* last_fail, const int16_t* ring, const int32_t* count) {
  return hv_copy(h, HV_START, {last_fail, ring, count}, true);
}

template <bool INJECT>
static int hv_reset_call(xv_anyhvac* h, const uint8_t* mask, const double* grid, const xv_anyhvac_io* io) {
  XV_CHECK_ARG(h && h->a.tables && (grid || !INJECT));
  xv_anyhvac_io o = {};
  if (io) o = *io;
  hv_bind_rng(h, INJECT ? 0 : 1);
  hipLaunchKernelGGL((xv_anyhvac_reset_kernel<INJECT>), dim3(h->a.n_env), dim3(HV_BLOCK), 0, h->eng->stream, h->a, mask, grid,
                     o);
  XV_LAUNCH_CHECK();
  if (h->act_window) {      // a reset env starts with an empty action window
    hipLaunchKernelGGL(xv_anyhvac_act_reset_kernel, dim3(h->a.n_env), dim3(HV_BLOCK), 0, h->eng->stream, h->act_window, h->a.C,
                       mask);
    XV_LAUNCH_CHECK();
  }
  return XV_OK;
}

extern "C" int xv_anyhvac_reset(xv_anyhvac* h, const uint8_t* mask, const xv_anyhvac_io* io) {
  return hv_reset_call<false>(h, mask, nullptr, io);
}

extern "C" int xv_anyhvac_reset_injected(xv_anyhvac* h, const uint8_t* mask, const double* grid, const xv_anyhvac_io* io) {
  return hv_reset_call<true>(h, mask, grid, io);
}

// ---- the mapped action modes -------------------------------------------------------------------------------------------
extern "C" int xv_anyhvac_set_action_mode(xv_anyhvac* h, int mode, int flags, const double* cost_table) {
  XV_CHECK_ARG(h && mode >= XV_ANYHVAC_ACT_BOX && mode <= XV_ANYHVAC_ACT_DIFF);
  XV_CHECK_ARG((flags & ~(XV_ANYHVAC_ACT_COST | XV_ANYHVAC_ACT_TOO_COLD_LIMIT)) == 0);
  XV_CHECK_ARG(mode == XV_ANYHVAC_ACT_DIFF || flags == 0);
  XV_CHECK_ARG(cost_table || !(flags & XV_ANYHVAC_ACT_COST));
  XV_HIP(hipSetDevice(h->eng->device));
  if (mode != XV_ANYHVAC_ACT_BOX) {
    XV_HIP(hv_alloc(h, HV_ACT, mode != h->act_mode));      // (new windows are empty; a change of flags alone keeps them)
    XV_HIP(hipStreamSynchronize(h->eng->stream));
    if (cost_table) XV_HIP(hipMemcpy(h->act_table, cost_table, XV_ANYHVAC_ACT_BINS * sizeof(double), hipMemcpyHostToDevice));
    else XV_HIP(hipMemset(h->act_table, 0, XV_ANYHVAC_ACT_BINS * sizeof(double)));
  }
  h->act_mode = mode;
  h->act_flags = flags;
  return XV_OK;
}

extern "C" int xv_anyhvac_act_get_state(xv_anyhvac* h, uint64_t* window) {
  XV_CHECK_ARG(window);
  return hv_copy(h, HV_ACT, {window}, false);
}
extern "C" int xv_anyhvac_act_set_state(xv_anyhvac* h, const uint64_t* window) {
  XV_CHECK_ARG(window);
  return hv_copy(h, HV_ACT, {window}, true);
}

// ---- the env's state ---------------------------------------------------------------------------------------------------
static int hv_env_copy(xv_anyhvac* h, const xv_anyhvac_state* s, bool set) {
  XV_CHECK_ARG(s);
  return hv_copy(h, HV_ENV, {s->grid, s->t, s->last_call, s->episode_step, s->warning_count, s->rest_idx, s->rest_start, s->value,
                             s->filter, s->ring_t, s->ring_v, s->head, s->tail}, set);
}

extern "C" int xv_anyhvac_get_state(xv_anyhvac* h, const xv_anyhvac_state* out) { return hv_env_copy(h, out, false); }
extern "C" int xv_anyhvac_set_state(xv_anyhvac* h, const xv_anyhvac_state* in) { return hv_env_copy(h, in, true); }

// ---- the PID teacher ---------------------------------------------------------------------------------------------------
static HvPid hv_pid_args(const xv_anyhvac* h, float* action_out, float* flat_out, double* stats) {
  HvPid D = {};
  D.weights = h->pid_weights; D.gains = h->pid_gains; D.f64 = h->pid_f64;
  D.acc = h->pid_acc; D.last_obs = h->pid_last_obs; D.fresh = h->pid_fresh;
  D.action_out = action_out; D.flat_out = flat_out; D.stats = stats;
  return D;
}

extern "C" int xv_anyhvac_pid_reset(xv_anyhvac* h, const uint8_t* mask) {
  XV_CHECK_ARG(h && h->pid_acc);
  hipLaunchKernelGGL(xv_anyhvac_pid_reset_kernel, dim3(h->a.n_env), dim3(HV_BLOCK), 0, h->eng->stream, h->a,
                     hv_pid_args(h, nullptr, nullptr, nullptr), mask);
  XV_LAUNCH_CHECK();
  return XV_OK;
}

extern "C" int xv_anyhvac_set_pid(xv_anyhvac* h, const double* weights, const double* gains, int kind_flags) {
  XV_CHECK_ARG(h && h->a.tables && weights && gains && (kind_flags & ~XV_ANYHVAC_PID_FLOAT64) == 0);
  XV_HIP(hipSetDevice(h->eng->device));
  const hipError_t r = hv_alloc(h, HV_PID, false);      // (all three or, after a failure, none)
  if (r != hipSuccess) {
    xv_set_error("xv_anyhvac_set_pid: device allocation failed: %s", hipGetErrorString(r));
    return XV_ERR_HIP;
  }
  h->pid_weights = weights;
  h->pid_gains = gains;
  h->pid_f64 = (kind_flags & XV_ANYHVAC_PID_FLOAT64) ? 1 : 0;
  return xv_anyhvac_pid_reset(h, nullptr);
}

extern "C" int xv_anyhvac_pid_action(xv_anyhvac* h, const float* readings, float* action_out, float* flat_out) {
  XV_CHECK_ARG(h && h->a.tables && h->pid_acc && action_out);
  hipLaunchKernelGGL(xv_anyhvac_pid_kernel, dim3(h->a.n_env), dim3(HV_BLOCK), 0, h->eng->stream, h->a,
                     hv_pid_args(h, action_out, flat_out, nullptr), readings);
  XV_LAUNCH_CHECK();
  return XV_OK;
}

extern "C" int xv_anyhvac_pid_get_state(xv_anyhvac* h, double* acc_diff, float* last_obs, int32_t* fresh) {
  return hv_copy(h, HV_PID, {acc_diff, last_obs, fresh}, false);
}
extern "C" int xv_anyhvac_pid_set_state(xv_anyhvac* h, const double* acc_diff, const float* last_obs, const int32_t* fresh) {
  return hv_copy(h, HV_PID, {acc_diff, last_obs, fresh}, true);
}

// ---- the step family ---------------------------------------------------------------------------------------------------
// What the seven entry points below ask of the one launch.  mapped: the call is one of a mapped action mode's (act: its
// arguments); pid: the teacher acts in front of every step (action_out, stats: its outputs).
struct HvRun {
  int T, mode;
  bool inject = false;
  const double* reset_grid = nullptr;
  bool mapped = false;
  const xv_anyhvac_act_io* act = nullptr;
  bool pid = false;
  float* action_out = nullptr;
  double* stats = nullptr;
};

typedef void (*HvStepKernel)(HvArgs, xv_anyhvac_io, const double*, int, int, HvPid, HvAct);

static int hv_run(xv_anyhvac* h, const xv_anyhvac_io* io, const HvRun& r) {
  XV_CHECK_ARG(h && h->a.tables && io && io->reward && io->terminated && io->truncated && r.T > 0);
  XV_CHECK_ARG(r.reset_grid || !r.inject);
  // a handle in a mapped mode steps through the _mapped entry points, a box handle through the others (the teachers put
  // out box actions)
  XV_CHECK_ARG((h->act_mode != XV_ANYHVAC_ACT_BOX) == r.mapped);
  HvAct A = {};
  if (r.mapped) {
    const xv_anyhvac_act_io* act = r.act;
    XV_CHECK_ARG(act && h->act_window && h->act_table);
    XV_CHECK_ARG(io->action || (act->action_index && h->act_mode == XV_ANYHVAC_ACT_DIFF));
    XV_CHECK_ARG(!act->action_index || h->act_mode == XV_ANYHVAC_ACT_DIFF);
    A.index = act->action_index; A.applied = act->applied_value; A.delta = act->delta; A.cost = act->action_cost;
    A.counts = act->stat_counts; A.window = h->act_window; A.table = h->act_table; A.flags = h->act_flags;
  } else if (r.pid) {
    XV_CHECK_ARG(h->pid_acc && r.action_out);
  } else {
    XV_CHECK_ARG(io->action);
  }
  if (r.mode != XV_AUTORESET_DISABLED && r.mode != XV_AUTORESET_SAME_STEP) {
    xv_set_error("xv_anyhvac: autoreset mode %d is not built (disabled and same_step are)", r.mode);
    return XV_ERR_UNSUPPORTED;
  }
  const HvPid D = r.pid ? hv_pid_args(h, r.action_out, nullptr, r.stats) : HvPid{};
  hv_bind_rng(h, r.inject ? 0 : (uint64_t)r.T);
  static const HvStepKernel plain[3][2] = {      // [the handle's action mode][inject]
      {xv_anyhvac_step_kernel<false, false, XV_ANYHVAC_ACT_BOX>, xv_anyhvac_step_kernel<true, false, XV_ANYHVAC_ACT_BOX>},
      {xv_anyhvac_step_kernel<false, false, XV_ANYHVAC_ACT_DISCRETE>, xv_anyhvac_step_kernel<true, false, XV_ANYHVAC_ACT_DISCRETE>},
      {xv_anyhvac_step_kernel<false, false, XV_ANYHVAC_ACT_DIFF>, xv_anyhvac_step_kernel<true, false, XV_ANYHVAC_ACT_DIFF>}};
  const HvStepKernel kernel = r.pid ? xv_anyhvac_step_kernel<false, true, XV_ANYHVAC_ACT_BOX> : plain[h->act_mode][r.inject ? 1 : 0];
  hipLaunchKernelGGL(kernel, dim3(h->a.n_env), dim3(HV_BLOCK), 0, h->eng->stream, h->a, *io, r.reset_grid, r.mode, r.T, D, A);
  XV_LAUNCH_CHECK();
  return XV_OK;
}

extern "C" int xv_anyhvac_step(xv_anyhvac* h, const xv_anyhvac_io* io, int autoreset_mode) {
  return hv_run(h, io, {1, autoreset_mode});
}
extern "C" int xv_anyhvac_step_injected(xv_anyhvac* h, const xv_anyhvac_io* io, const double* reset_grid, int autoreset_mode) {
  return hv_run(h, io, {1, autoreset_mode, true, reset_grid});
}
extern "C" int xv_anyhvac_rollout(xv_anyhvac* h, int T, const xv_anyhvac_io* io, int autoreset_mode) {
  return hv_run(h, io, {T, autoreset_mode});
}
extern "C" int xv_anyhvac_step_mapped(xv_anyhvac* h, const xv_anyhvac_io* io, const xv_anyhvac_act_io* act, int autoreset_mode) {
  return hv_run(h, io, {1, autoreset_mode, false, nullptr, true, act});
}
extern "C" int xv_anyhvac_step_mapped_injected(xv_anyhvac* h, const xv_anyhvac_io* io, const xv_anyhvac_act_io* act,
                                               const double* reset_grid, int autoreset_mode) {
  return hv_run(h, io, {1, autoreset_mode, true, reset_grid, true, act});
}
extern "C" int xv_anyhvac_rollout_mapped(xv_anyhvac* h, int T, const xv_anyhvac_io* io, const xv_anyhvac_act_io* act,
                                         int autoreset_mode) {
  return hv_run(h, io, {T, autoreset_mode, false, nullptr, true, act});
}
extern "C" int xv_anyhvac_rollout_pid(xv_anyhvac* h, int T, const xv_anyhvac_io* io, float* action_out, double* stats,
                                      int autoreset_mode) {
  return hv_run(h, io, {T, autoreset_mode, false, nullptr, false, nullptr, true, action_out, stats});
}
#endif  // XV_KERNELS_ONLY
