// anymdp_sampler.hip — AnyMDP task sampler on the device: generate, repair and accept thousands of candidate tasks per
// launch, one workgroup per candidate, and write the accepted ones straight into the step engine's row records.
//
// Reference: xenoverse/anymdp/task_sampler.py:15-65 (AnyMDPTaskSampler), task_sampler_utils.py:11-256 (generative
// model: start / terminal states, banded transition kernel split over the actions, potential + position + state-action
// rewards, terminal rewards repaired against the value function) and solver.py:57-148 (acceptance: value gap between
// the optimal and the uniform policy, long-run occupancy of the greedy policy).  There the work is a Python triple loop
// (518 s per 64x8 task without numba).
//
// ONE MODEL: xs_candidate<Rows> states every stage once — head scalars, terminal redraws, bands, the split of a row over
// the actions, rewards, the repair loop, the acceptance test and every output:
//   * every random quantity is a counter-based draw, Philox4x32-10(counter = {candidate, index, purpose}, key = seed):
//     a pure function of its coordinates, so the threads of a state simply recompute what they share (band, weights)
//     instead of exchanging it, and a candidate is reproducible whatever the launch geometry.  Same distributions as the
//     reference, not NumPy's sequential stream (the seed-compatible sampler is host code: anymdp/task_sampler.py);
//   * value iteration is the synchronous sweep Q <- ER + gamma T V(Q) to rms update <= 1e-4 (the reference's stopping
//     rule; same fixed point as its damped Gauss-Seidel): V through LDS broadcast reads, two barriers per sweep;
//   * accepted candidates are emitted in the layout xv_anymdp_create reads (blocks of 7 {cdf, reward, noise}).
// TWO STORAGES for the rows T[s, a, :] of the candidate's transition tensor, the `Rows` of the model:
//   * RegRows<SP> (S <= 64, S * A <= 512): thread (s, a) owns its row in registers for the whole life of the candidate:
//     generation, 5 + 2 value iterations and the emission never move the transition tensor through memory.  Every loop
//     over a row is unrolled over SP = 16 / 32 / 64; a state's action centres are shared through LDS;
//   * BigRows<R> (the rest up to S <= 256, S * A <= 4096: the reference's GarnetTaskSampler defaults to 128 states and its
//     MultiTokensAnyPOMDPTaskSampler to 256, task_sampler.py:90-126): S * A rows of S doubles are 2.6 MB at 256 x 5, so
//     they live in a per-candidate global scratch, TRANSPOSED in blocks of 64 rows — Tt[(row >> 6) * S + j][row & 63] — so
//     that the 64 lanes of a wave, which own 64 consecutive rows, read element j of their rows as one coalesced 512-byte
//     access.  Thread tid owns rows tid, tid + blockDim, ... (R <= 4 of them); the value iteration and the expected
//     reward sweep the union of a wave's bands only; each thread recomputes its state's action centres.
// A zero outside a row's band adds nothing to an fma over j ascending, so both storages give the same bits, and the file
// is built with -ffp-contract=off: an expression evaluated as written is the same bits wherever it is instantiated.  The
// Philox index strides (64 words per 256 states) were laid out for 256 states, so the coordinates are one set too.
// oracle/xeno_oracle_sampler.c (part 2) restates the model draw for draw; tests/test_gpu_sampler.py diffs them.
#include "philox.h"
#include "xv_common.h"
#include "xv_draws.h"

namespace {

enum : uint32_t { XS_HEAD = 0, XS_PERM, XS_S0, XS_PIT, XS_PITS, XS_BAND, XS_BANDW, XS_ACT, XS_ACTW, XS_POT, XS_POS,
                  XS_POSN, XS_POSU, XS_SA, XS_SAM, XS_STEP, XS_REPAIR };
constexpr int XS_MAX_SWEEPS = 20000;
constexpr double XS_EPS = 1e-10;
constexpr double XS_TWO_PI = 6.283185307179586476925286766559;

struct SamplerArgs {
  uint64_t seed;
  int64_t cand_base;
  int n_cand, S, A, s0_max, row_lines;
  // table outputs, slot = candidate index within the launch (written for accepted candidates only)
  double* rows;          // [n_cand][S][A][row_lines][16]
  int32_t* state_map;    // [n_cand][S]
  uint64_t* term_mask;   // [n_cand][ceil(S / 64)]
  double* s0_cdf;        // [n_cand][s0_max]
  int32_t* s0_ids;       // [n_cand][s0_max]
  int32_t* max_steps;    // [n_cand]
  // optional dense outputs (written for every candidate that was generated, accepted or not)
  double *transition, *reward, *noise;   // [n_cand][S][A][S]
  xv_anymdp_cand_info* info;             // [n_cand]
  int32_t* status;                       // [n_cand]
};

// the 32-bit-word draws of this file (xv_draws.h builds its uniforms and normals from 53-bit pairs instead)
__device__ __forceinline__ double xs_u32(uint32_t w) { return (double)w * (1.0 / 4294967296.0); }
__device__ __forceinline__ void xs_normal2(uint32_t wa, uint32_t wb, double& z0, double& z1) {
  const double u1 = ((double)wa + 1.0) * (1.0 / 4294967296.0), u2 = xs_u32(wb);
  const double r = sqrt(-2.0 * log(u1));
  z0 = r * cos(XS_TWO_PI * u2);
  z1 = r * sin(XS_TWO_PI * u2);
}
__device__ __forceinline__ uint32_t xs_word(const xv_u32x4& w, int k) {
  return k == 0 ? w.x : (k == 1 ? w.y : (k == 2 ? w.z : w.w));
}
// element k (0..3) of the four normals of one Philox call
__device__ __forceinline__ double xs_normal_of(const xv_u32x4& w, int k) {
  double z0, z1;
  if (k < 2) xs_normal2(w.x, w.y, z0, z1); else xs_normal2(w.z, w.w, z0, z1);
  return (k & 1) ? z1 : z0;
}
__device__ __forceinline__ double xs_clip(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }
__device__ __forceinline__ double xs_row_max(const double* row, int A) {
  double v = row[0];
  for (int a = 1; a < A; ++a) v = row[a] > v ? row[a] : v;
  return v;
}

// One candidate as its workgroup sees it: its draws and its per-state arrays.  Each kernel carves the arrays its own way;
// all are LDS, except that Pm / Pm2 are global scratch under BigRows.
struct Cand {
  const SamplerArgs& P;
  uint64_t cand;
  int S, A, SA;
  double *Qs;                                  // [rows]  Q of every row (also: action centres, the state permutation)
  double *Vs, *part;                           // [S] V of a sweep (first: band totals), [waves] update-norm partials
  double *pot, *rpos, *npos, *bonus, *vstate;  // [S] reward pieces; V(s) = max_a Q after a value iteration
  int *pitm, *bandlo, *bandhi;                 // [S] terminal flag, band [lo, hi)
  double *Pm, *Pm2;                            // [S*S] band weights during generation, occupancy matrices at acceptance

  __device__ __forceinline__ xv_u32x4 draw(uint32_t purpose, uint32_t idx) const {
    return xv_philox4x32_10((uint32_t)cand, (uint32_t)(cand >> 32), idx, purpose, (uint32_t)P.seed, (uint32_t)(P.seed >> 32));
  }
  // centre of action b of live state s, uniform over the state's band
  __device__ __forceinline__ double centre(int s, int b) const {
    const int first = bandlo[s], last = bandhi[s];
    const xv_u32x4 q4 = draw(XS_ACT, (uint32_t)s * 16u + (uint32_t)(b >> 2));
    return (double)(first - 1) + xs_u32(xs_word(q4, b & 3)) * (double)(last - (first - 1));
  }
};

// ---- row storage.  A storage names the rows of this thread (slot k < R is row `row(k)`; slots without storage are
// skipped), visits their elements in ascending j — each(k, lo, hi, f) calls f(j, T[row][j]) for lo <= j < hi — and
// chooses the inner range of the fma chains (each_inner) and how a thread gets the action centres of a row's state.

template <int SP>
struct RegRows {
  static constexpr int R = 1;
  double T[SP] = {};
  __device__ __forceinline__ int row(int) const { return threadIdx.x; }
  __device__ __forceinline__ bool stored(int) const { return true; }
  template <class F>
  __device__ __forceinline__ void each(int, int lo, int hi, F f) {
#pragma unroll
    for (int j = 0; j < SP; ++j)
      if (j >= lo && j < hi) f(j, T[j]);
  }
  // all of the row, unrolled.  SP / 2 <= S (xv_anymdp_sample_tasks chooses the smallest SP that holds S), so the first half
  // needs no test: each test is a wave-uniform branch per sweep and a mask held in scalar registers for the whole kernel
  template <class F>
  __device__ __forceinline__ void each_inner(int, int S, F f) {
#pragma unroll
    for (int j = 0; j < SP; ++j)
      if (j < SP / 2 || j < S) f(j, T[j]);
  }
  __device__ __forceinline__ void set_inner(int, bool, int, int, int) {}
  // the state's A centres are shared through LDS: every live row's thread draws its own
  __device__ __forceinline__ void share_centres(const Cand& C) {
    const int tid = threadIdx.x;
    if (tid < C.SA) {
      const int s = tid / C.A;
      if (!C.pitm[s]) C.Qs[tid] = C.centre(s, tid - s * C.A);
    }
    __syncthreads();
  }
  __device__ __forceinline__ const double* centres(const Cand& C, int s, double (&)[64]) { return C.Qs + s * C.A; }
};

template <int R_>
struct BigRows {
  static constexpr int R = R_;
  double* Tt;        // this candidate's [n_rb * S * 64]
  int S, SAp;        // SAp = n_rb * 64 rows have storage
  int wf[R_], wl[R_];
  __device__ __forceinline__ int row(int k) const { return k * (int)blockDim.x + (int)threadIdx.x; }
  __device__ __forceinline__ bool stored(int k) const { return row(k) < SAp; }
  template <class F>
  __device__ __forceinline__ void each(int k, int lo, int hi, F f) {
    const int r = row(k);
    double* col = Tt + ((size_t)(r >> 6) * S) * 64 + (r & 63);
    for (int j = lo; j < hi; ++j) f(j, col[(size_t)j * 64]);
  }
  template <class F>
  __device__ __forceinline__ void each_inner(int k, int, F f) { each(k, wf[k], wl[k], f); }
  // the wave-uniform union of the bands of slot k's 64 rows (empty where none of them is live: nothing is read)
  __device__ __forceinline__ void set_inner(int k, bool live, int first, int last, int S_) {
    int lo = live ? first : S_, hi = live ? last : 0;
    for (int o = 32; o > 0; o >>= 1) {
      const int l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
      lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi;
    }
    wf[k] = lo < hi ? lo : 0; wl[k] = lo < hi ? hi : 0;
  }
  __device__ __forceinline__ void share_centres(const Cand&) {}
  // (the buffer is the caller's: a dynamically indexed member would keep the whole storage out of registers)
  __device__ __forceinline__ const double* centres(const Cand& C, int s, double (&cen)[64]) {
    for (int b = 0; b < C.A; ++b) cen[b] = C.centre(s, b);
    return cen;
  }
};

// Q of this thread's rows -> LDS
template <class Rows>
__device__ __forceinline__ void xs_publish(const Cand& C, const Rows& T, const double (&q)[Rows::R]) {
#pragma unroll
  for (int k = 0; k < Rows::R; ++k) {
    const int r = T.row(k);
    if (r < C.SA) C.Qs[r] = q[k];
  }
}

// Synchronous value iteration on the candidate's rows.  q: Q of this thread's rows, in/out.  Returns the sweep count
// (uniform).  Each sweep: Q -> LDS | barrier | V = max / mean per state, and the previous sweep's update norm is
// inspected (uniform decision) | barrier | broadcast reads of V over the storage's inner range, one fma each.
template <class Rows>
__device__ __forceinline__ int xs_value_iteration(const Cand& C, Rows& T, double gamma, bool greedy,
                                                  const double (&er)[Rows::R], double (&q)[Rows::R]) {
  const int tid = threadIdx.x, S = C.S, A = C.A, n_waves = (int)(blockDim.x >> 6);
  double d2 = 0.0;
  int it = 0;
  for (;;) {
    xs_publish(C, T, q);
    {
      double x = d2;
      for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
      if ((tid & 63) == 0) C.part[tid >> 6] = x;
    }
    __syncthreads();
    if (it > 0) {
      double tot = 0.0;
      for (int w = 0; w < n_waves; ++w) tot += C.part[w];
      if (sqrt(tot / (double)C.SA) <= 1.0e-4 || it >= XS_MAX_SWEEPS) break;
    }
    if (tid < S) {
      const double* row = C.Qs + tid * A;
      double v;
      if (greedy) {
        v = xs_row_max(row, A);
      } else {
        v = 0.0;
        for (int a = 0; a < A; ++a) v += row[a];
        v /= (double)A;
      }
      C.Vs[tid] = v;
    }
    __syncthreads();
    d2 = 0.0;
#pragma unroll
    for (int k = 0; k < Rows::R; ++k) {
      double acc = 0.0;
      T.each_inner(k, S, [&](int j, double& t) { acc = fma(t, C.Vs[j], acc); });
      const double qn = fma(gamma, acc, er[k]);
      if (T.row(k) < C.SA) d2 += (qn - q[k]) * (qn - q[k]);
      q[k] = qn;
    }
    ++it;
  }
  __syncthreads();
  return it;
}

// The model: one candidate, by the whole workgroup.
template <class Rows>
__device__ __forceinline__ void xs_candidate(const Cand& C, Rows& T) {
  constexpr int R = Rows::R;
  const SamplerArgs& P = C.P;
  const int S = C.S, A = C.A, SA = C.SA, tid = threadIdx.x, BD = blockDim.x, ci = blockIdx.x;
  double *Qs = C.Qs, *Vs = C.Vs, *pot = C.pot, *rpos = C.rpos, *npos = C.npos, *bonus = C.bonus, *vstate = C.vstate;
  int *pitm = C.pitm, *bandlo = C.bandlo, *bandhi = C.bandhi;
  double* Pm = C.Pm;

  // ---- uniform scalars: every thread derives them from the same draws ----
  xv_u32x4 w = C.draw(XS_HEAD, 0);
  const double lower = 4.0 * S > 100 ? 4.0 * S : 100;
  double upper = 8.0 * S < 500 ? 8.0 * S : 500;
  if (upper < lower + 1) upper = lower + 1;
  const double max_steps = lower + xv_u53(w.x, w.y) * (upper - lower);
  // start states (task_sampler_utils.py:70-79)
  double w0[3] = {1.0, 0.0, 0.0};
  for (uint32_t r = 0; r < 16; ++r) {
    const xv_u32x4 q4 = C.draw(XS_S0, r);
    double z0, z1, z2, z3;
    xs_normal2(q4.x, q4.y, z0, z1);
    xs_normal2(q4.z, q4.w, z2, z3);
    const double c0 = z0 > 0.0 ? z0 : 0.0, c1 = z1 > 0.0 ? z1 : 0.0, c2 = z2 > 0.0 ? z2 : 0.0;
    if ((c0 + c1) + c2 >= XS_EPS) { w0[0] = c0; w0[1] = c1; w0[2] = c2; break; }
  }
  // the (at most three) start states, compacted.  Indexed through selects, never dynamically: a stack array indexed by a
  // variable may be left in scratch memory
  int s0_id[3] = {0, 0, 0}, n_s0 = 0;
  double s0_p[3] = {0.0, 0.0, 0.0}, s0sum = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (w0[k] > XS_EPS) {
#pragma unroll
      for (int i = 0; i <= k; ++i) if (i == n_s0) { s0_id[i] = k; s0_p[i] = w0[k]; }
      s0sum += w0[k]; ++n_s0;
    }
#pragma unroll
  for (int k = 0; k < 3; ++k) if (k < n_s0) s0_p[k] /= s0sum;
  auto s0i = [&](int k) { return k == 0 ? s0_id[0] : (k == 1 ? s0_id[1] : s0_id[2]); };
  auto s0p = [&](int k) { return k == 0 ? s0_p[0] : (k == 1 ? s0_p[1] : s0_p[2]); };
  // terminal states (:81-93)
  w = C.draw(XS_PIT, 0);
  double p_pit = -0.20 + 0.60 * xv_u53(w.x, w.y);
  if (p_pit < 0.0) p_pit = 0.0;
  const int goal = xs_u32(w.z) < 0.3 ? 1 : 0;
  {
    int mine = 0;
    for (uint32_t r = 0; r < 64; ++r) {
      mine = 0;
      if (tid < S) {
        const xv_u32x4 q4 = C.draw(XS_PITS, r * 64u + (uint32_t)(tid >> 2));
        mine = xs_u32(xs_word(q4, tid & 3)) < p_pit ? 1 : 0;
      }
      const int cnt = __syncthreads_count(mine);
      if ((double)cnt < (double)S * p_pit + 1.0) break;
    }
    if (tid < S) {
      for (int k = 0; k < n_s0; ++k) if (tid == s0i(k)) mine = 0;
      if (tid == S - 1) mine = goal;
      pitm[tid] = mine;
    }
  }
  __syncthreads();
  int n_se = 0;
  for (int j = 0; j < S; ++j) n_se += pitm[j];

  // ---- band of every live state (:95-124), by the state's own thread ----
  if (tid < S) {
    int first = 0, last = 0;
    if (!pitm[tid]) {
      const int st = tid;
      const int fwd_max = S / 4 + 1 > 2 ? S / 4 + 1 : 2, back_max = S / 2 + 1 > 2 ? S / 2 + 1 : 2;
      const int a_lo = st - back_max > 0 ? st - back_max : 0;
      int a_hi = st - 1 > 0 ? st - 1 : 0;
      if (a_hi < a_lo + 1) a_hi = a_lo + 1;
      const int b_hi = S < st + fwd_max ? S : st + fwd_max;
      int b_lo = S - 1 < st + 1 ? S - 1 : st + 1;
      if (b_lo > b_hi - 1) b_lo = b_hi - 1;
      w = C.draw(XS_BAND, (uint32_t)st);
      first = a_lo + (int)(w.x % (uint32_t)(a_hi - a_lo));
      last = b_lo + (int)(w.y % (uint32_t)(b_hi - b_lo));
      while (last < S) {          // widen until two live states lie ahead inside the band
        int ahead = 0;
        for (int j = st + 1; j < last; ++j) ahead += !pitm[j];
        if (ahead > 1) break;
        ++last;
      }
    }
    bandlo[tid] = first; bandhi[tid] = last;
  }
  __syncthreads();
  // band weights clip(N(0,1), 0.1, 1) (:126-133), element (state, next state) by element over the whole workgroup,
  // staged in the (still unused) occupancy buffer
  for (int el = tid; el < S * S; el += BD) {
    const int st = el / S, j = el - st * S;
    double v = 0.0;
    if (j >= bandlo[st] && j < bandhi[st]) {
      const xv_u32x4 q4 = C.draw(XS_BANDW, ((uint32_t)st * 8u) * 64u + (uint32_t)(j >> 2));
      v = xs_clip(xs_normal_of(q4, j & 3), 0.10, 1.0);
    }
    Pm[el] = v;
  }
  __syncthreads();
  if (tid < S && !pitm[tid]) {     // damp the self loop (none at the last state), then the row total
    Pm[tid * S + tid] = (tid == S - 1) ? 0.0 : Pm[tid * S + tid] / 2.0;
    double tot = 0.0;
    for (int j = bandlo[tid]; j < bandhi[tid]; ++j) tot += Pm[tid * S + j];
    Vs[tid] = tot;
  }
  __syncthreads();

  // ---- the rows of the transition tensor (:154-175): the band weights of the state, split over its actions ----
  T.share_centres(C);
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int r = T.row(k);
    const bool in = r < SA;
    const int s = in ? r / A : 0, a = in ? r - s * A : 0;
    const bool live = in && !pitm[s];
    const int first = live ? bandlo[s] : 0, last = live ? bandhi[s] : 0;
    T.set_inner(k, live, first, last, S);
    if (!T.stored(k)) continue;
    if (!live) {
      T.each(k, 0, S, [](int, double& t) { t = 0.0; });
      continue;
    }
    const double tot = Vs[s];
    double cen_own[64];      // only a storage that recomputes the centres uses it
    const double* cen = T.centres(C, s, cen_own);
    w = C.draw(XS_ACTW, (uint32_t)s);
    const double width = xs_clip(xv_expo(xv_u53(w.x, w.y)), 0.20, 1.6);
    const double inv_w2 = 1.0 / (width * width);
    double rs = 0.0;
    T.each(k, 0, S, [&](int j, double& t) {
      double v = 0.0;
      if (j >= first && j < last) {
        double col = 0.0, dmin = 0.0, e_me = 0.0;
        int amin = 0;
        for (int b = 0; b < A; ++b) {
          const double d = cen[b] - (double)j, d2 = d * d;
          const double e = exp(-d2 * inv_w2);
          col += e;
          if (b == a) e_me = e;
          if (b == 0 || d2 < dmin) { dmin = d2; amin = b; }
        }
        if (col < XS_EPS) {      // no action reaches this next state: it goes to the nearest one
          col = 0.0;
          for (int b = 0; b < A; ++b) {
            const double d = cen[b] - (double)j;
            col += (b == amin) ? 1.0 : exp(-(d * d) * inv_w2);
          }
          if (a == amin) e_me = 1.0;
        }
        v = (e_me / col) * (Pm[s * S + j] / tot);
        rs += v;
      }
      t = v;
    });
    T.each(k, first, last, [&](int, double& t) { t /= rs; });
  }
  __syncthreads();

  // ---- rewards (:11-63, :193-207): per-state pieces in LDS, the state-action pieces in registers ----
  double pbase, ub;
  {
    w = C.draw(XS_POS, 0);
    pbase = 0.2 * xv_expo(xv_u53(w.x, w.y));
    ub = xv_u53(w.z, w.w);
  }
  if (tid < S) {
    const int j = tid;
    // potential: a few Fourier terms over the state index (RandomFourier, utils/random_nn.py:346-368)
    xv_u32x4 q4 = C.draw(XS_POT, 0);
    const double base = xv_u53(q4.x, q4.y) < 0.5 ? 0.0 : xs_clip(xv_expo(xv_u53(q4.z, q4.w)), 0.20, 5.0);
    q4 = C.draw(XS_POT, 1);
    double box = -base + 2.0 * base * xv_u53(q4.x, q4.y);
    if (box < 0.0) box = 0.0;
    const int n_items = 1 + (int)(q4.z % 3u);
    const double scale = box / sqrt((double)n_items);
    const double x = (double)j / (double)(2 * S);
    double pj = 0.0;
    for (int k = 0; k <= n_items; ++k) {
      double za, zb, order = 0.0;
      q4 = C.draw(XS_POT, 2u + (uint32_t)k);
      xs_normal2(q4.x, q4.y, za, zb);
      const double ca = za * (xv_expo(xs_u32(q4.z)) * scale), cb = zb * (xv_expo(xs_u32(q4.w)) * scale);
      if (k > 0) {
        double zo, zd;
        q4 = C.draw(XS_POT, 8u + (uint32_t)k);
        xs_normal2(q4.y, q4.z, zo, zd);
        order = (double)(1 + (int)(q4.x % 5u)) + zo;
      }
      pj += ca * sin(order * x) + cb * cos(order * x);
    }
    pot[j] = pj;
    q4 = C.draw(XS_POSN, (uint32_t)(j >> 2));
    double pdf = xs_normal_of(q4, j & 3);
    pdf = pdf > 0.0 ? pdf : 0.0;
    if (j == S - 1) pdf += 0.20;
    rpos[j] = pdf * pbase;
    q4 = C.draw(XS_POSU, (uint32_t)(j >> 2));
    const double u = -0.30 + 0.60 * xs_u32(xs_word(q4, j & 3));
    npos[j] = pitm[j] ? 0.0 : (u > 0.0 ? u : 0.0) * pbase;
    bonus[j] = (j == S - 1) ? 1.0 : 0.0;
  }
  __syncthreads();
  double cdf_j = 0.0, c_all = 0.0;
  for (int i = 0; i < S; ++i) {         // cumulative sums in index order, as numpy.cumsum forms them
    c_all += rpos[i];
    if (i == tid) cdf_j = c_all;
  }
  __syncthreads();
  if (tid < S) {
    const double baseline = 0.1 * c_all + ub * (0.9 * c_all - 0.1 * c_all);
    rpos[tid] = pitm[tid] ? 0.0 : cdf_j - baseline;
  }
  w = C.draw(XS_SA, 0);
  const double sbase = xs_clip(0.05 * xv_expo(xv_u53(w.x, w.y)), 0.0, 0.10);
  auto sa_pieces = [&](int r, double& rsa_r, double& nsa_r) {
    double zr, zn;
    const xv_u32x4 q4 = C.draw(XS_SAM, (uint32_t)r);
    const double on = xs_u32(q4.x) > 0.7 ? 1.0 : 0.0;
    xs_normal2(q4.y, q4.z, zr, zn);
    rsa_r = sbase * zr * on;
    nsa_r = 0.30 * sbase * (zn > 0.0 ? zn : 0.0) * on;
  };
  double r_step = 0.0, rsa[R], pot_s[R];
  {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int r = T.row(k);
      double nsa;
      rsa[k] = 0.0; pot_s[k] = 0.0;
      if (r < SA) {
        sa_pieces(r, rsa[k], nsa);
        pot_s[k] = pot[r / A];
      }
    }
    double zs, zd;
    w = C.draw(XS_STEP, 0);
    xs_normal2(w.x, w.y, zs, zd);
    if (goal) r_step = (zs < 0.0 ? zs : 0.0) * 0.01;
    else if (n_se > 0) r_step = (zs > 0.0 ? zs : 0.0) * 0.01;
  }
  __syncthreads();

  // reward of slot k's row -> next state j under the current terminal bonus, and a row's expectation of it: one fma per
  // element of the storage's inner range, j ascending
  auto reward = [&](int k, int j) {
    const double r = (((pot_s[k] - pot[j]) + rpos[j]) + rsa[k]) + r_step;
    return r + bonus[j];
  };
  auto expected = [&](double (&er)[R]) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      double e = 0.0;
      if (T.row(k) < SA) T.each_inner(k, S, [&](int j, double& t) { e = fma(t, reward(k, j), e); });
      er[k] = e;
    }
  };
  // V(s) = max_a Q(s, a) of this thread's q -> vstate, through Qs
  auto state_values = [&](const double (&q)[R]) {
    xs_publish(C, T, q);
    __syncthreads();
    if (tid < S) vstate[tid] = xs_row_max(Qs + tid * A, A);
    __syncthreads();
  };

  // ---- terminal rewards repaired against the value function (:209-256) ----
  const int last_live = goal ? S - 2 : S - 1;
  int status = 1, repair_rounds = 0;
  int sweeps[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double q[R], er[R];
#pragma unroll
  for (int k = 0; k < R; ++k) q[k] = 0.0;
  for (int tries = 0; tries < 5; ++tries) {
    expected(er);
    const int sw = xs_value_iteration(C, T, 0.99, true, er, q);
    sweeps[tries] = sw;
    repair_rounds = tries + 1;
    if (sw >= XS_MAX_SWEEPS) { status = 4; break; }
    state_values(q);
    double vmin_live = 0.0, vmax_s0 = 0.0, bmin = bonus[0];
    bool first_live = true;
    for (int j = 0; j < S; ++j) {
      const double v = vstate[j];
      if (!pitm[j] && (first_live || v < vmin_live)) { vmin_live = v; first_live = false; }
      if (bonus[j] < bmin) bmin = bonus[j];
    }
    for (int k = 0; k < n_s0; ++k) {
      const double v = vstate[s0i(k)];
      if (k == 0 || v > vmax_s0) vmax_s0 = v;
    }
    w = C.draw(XS_REPAIR, (uint32_t)tries);
    const double pit_gap = bmin - vmin_live + 1.0;
    const double goal_gap = vmax_s0 - vstate[last_live] + (2.0 + 3.0 * xv_u53(w.x, w.y));
    if (pit_gap <= 0.0 && goal_gap <= 0.0) { status = 0; break; }
    __syncthreads();       // everyone has read bonus / vstate
    if (tid < S) {
      double bj = bonus[tid];
      if (pit_gap > 0.0 && pitm[tid] && !(goal && tid == S - 1)) bj -= pit_gap + (1.0 + 9.0 * xs_u32(w.z));
      if (goal_gap > 0.0 && tid == S - 1) {
        const double extra = 1.0 + 9.0 * xs_u32(w.w);
        const double lift = 2.0 * goal_gap > extra ? 2.0 * goal_gap : extra;
        bj += goal ? lift : (1.0 - 0.99) * lift;
      }
      bonus[tid] = bj;
    }
    __syncthreads();
  }

  // ---- acceptance (solver.py:105-148) ----
  double gini = 0.0, ent = 0.0, gap_min = 0.0;
  if (status == 0) {
    const double g2 = exp2(-1.0 / (double)S);
    expected(er);
    double qo[R], qr[R];
#pragma unroll
    for (int k = 0; k < R; ++k) { qo[k] = 0.0; qr[k] = 0.0; }
    sweeps[5] = xs_value_iteration(C, T, g2, true, er, qo);
    state_values(qo);
    // occupancy matrix: row s = the greedy action's row of T (first maximum), by the thread that owns it, or the start
    // distribution for terminal states
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int r = T.row(k);
      if (r < SA) {
        const int s = r / A, a = r - s * A;
        int g_s = 0;
        double v = Qs[s * A];
        for (int b = 1; b < A; ++b) if (Qs[s * A + b] > v) { v = Qs[s * A + b]; g_s = b; }
        if (a == g_s)
          T.each(k, 0, S, [&](int j, double& t) {
            double pj = t;
            if (pitm[s]) {
              pj = 0.0;
              for (int kk = 0; kk < n_s0; ++kk) if (j == s0i(kk)) pj = s0p(kk);
            }
            Pm[s * S + j] = pj;
          });
      }
    }
    __syncthreads();
    sweeps[6] = xs_value_iteration(C, T, g2, false, er, qr);
    if (sweeps[5] >= XS_MAX_SWEEPS || sweeps[6] >= XS_MAX_SWEEPS) status = 4;
    xs_publish(C, T, qr);
    __syncthreads();
    const double scale = (1.0 - g2) * max_steps;
    for (int k = 0; k < n_s0; ++k) {
      const double vr = xs_row_max(Qs + s0i(k) * A, A);
      const double gap = vstate[s0i(k)] * scale - vr * scale;
      if (k == 0 || gap < gap_min) gap_min = gap;
    }
    if (status == 0 && gap_min < 2.0) status = 2;
    if (status == 0) {      // uniform
      const int K = (int)log2(max_steps) + 1;
      double* Pa = Pm;
      double* Pb = C.Pm2;
      for (int rep = 0; rep < K; ++rep) {
        __syncthreads();
        for (int e = tid; e < S * S; e += BD) {
          const int i = e / S, j = e - i * S;
          double acc = 0.0;
          for (int k = 0; k < S; ++k) acc = fma(Pa[i * S + k], Pa[k * S + j], acc);
          Pb[e] = acc;
        }
        double* t = Pa; Pa = Pb; Pb = t;
      }
      __syncthreads();
      for (int k = 0; k < n_s0; ++k) {
        const double* row = Pa + s0i(k) * S;
        double s2 = 0.0, h = 0.0;
        for (int j = 0; j < S; ++j) {
          const double p = row[j] + 1.0e-12;
          s2 += p * p;
          h += p * log(p);
        }
        const double gk = 1.0 - s2, ek = -h / log((double)S);
        if (k == 0 || gk < gini) gini = gk;
        if (k == 0 || ek < ent) ent = ek;
      }
      if (!(gini > 0.70 && ent > 0.35)) status = 3;
    }
  }

  // ---- outputs ----
  double nsa[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    double again;
    nsa[k] = 0.0;
    if (T.row(k) < SA && (P.noise || (status == 0 && P.rows))) sa_pieces(T.row(k), again, nsa[k]);
  }
  if (tid == 0) {
    P.status[ci] = status;
    if (P.info) {
      xv_anymdp_cand_info& o = P.info[ci];
      o.status = status; o.goal = goal; o.n_s0 = n_s0; o.repair_rounds = repair_rounds;
      for (int k = 0; k < 4; ++k) { o.s0[k] = k < n_s0 ? s0i(k) : 0; o.s0_prob[k] = k < n_s0 ? s0p(k) : 0.0; }
      for (int k = 0; k < 8; ++k) o.sweeps[k] = sweeps[k];
      o.max_steps = max_steps; o.gini = gini; o.ent = ent; o.gap_min = gap_min;
    }
  }
  if (P.info && tid < S) {
    P.info[ci].band_lo[tid] = bandlo[tid];
    P.info[ci].band_hi[tid] = bandhi[tid];
    P.info[ci].s_e[tid] = (uint8_t)pitm[tid];
  }
  if (P.transition || P.reward || P.noise) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int r = T.row(k);
      if (r < SA) {
        const size_t o = ((size_t)ci * SA + r) * S;
        T.each(k, 0, S, [&](int j, double& t) {
          if (P.transition) P.transition[o + j] = t;
          if (P.reward) P.reward[o + j] = reward(k, j);
          if (P.noise) P.noise[o + j] = npos[j] + nsa[k];
        });
      }
    }
  }
  // state_mapping: a Fisher-Yates permutation of the state ids (task_sampler.py:44), sequential by nature
  if (tid == 0 && (P.state_map || P.info)) {
    int* sm = reinterpret_cast<int*>(Qs);
    for (int i = 0; i < S; ++i) sm[i] = i;
    for (int i = S - 1; i >= 1; --i) {
      const xv_u32x4 q4 = C.draw(XS_PERM, (uint32_t)(i >> 2));
      const int j = (int)(xs_word(q4, i & 3) % (uint32_t)(i + 1));
      const int t = sm[i]; sm[i] = sm[j]; sm[j] = t;
    }
    for (int i = 0; i < S; ++i) {
      if (P.info) P.info[ci].state_map[i] = sm[i];
      if (P.state_map && status == 0) P.state_map[(size_t)ci * S + i] = sm[i];
    }
  }
  if (status != 0 || P.rows == nullptr) return;
  // accepted: the step engine's tables.  Row record of (s, a): line 0 (fence) left zero — xv_anymdp_create completes
  // it — then blocks of 7 entries {cdf fp64, reward fp32, noise fp32}; cdf = cumsum(row) / cumsum(row)[-1] as
  // numpy.random.choice forms it, 1.0 for the all-zero rows of terminal states, 2.0 past the last state.
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int r = T.row(k);
    if (r >= SA) continue;
    double* rec = P.rows + ((size_t)ci * SA + r) * (size_t)P.row_lines * 16;
    for (int e = 0; e < P.row_lines * 16; ++e) rec[e] = 0.0;
    double tot = 0.0;
    T.each(k, 0, S, [&](int, double& t) { tot += t; });
    const bool zero_row = tot == 0.0;
    double c = 0.0;
    T.each(k, 0, S, [&](int j, double& t) {
      c += t;
      const float rf = (float)reward(k, j), nf = (float)(npos[j] + nsa[k]);
      double* ent2 = rec + 16 * (1 + j / 7) + 2 * (j % 7);
      ent2[0] = zero_row ? 1.0 : c / tot;
      ent2[1] = __hiloint2double((int)__float_as_uint(nf), (int)__float_as_uint(rf));
    });
    const int n_ent = (P.row_lines - 1) * 7;
    for (int j = S; j < n_ent; ++j) rec[16 * (1 + j / 7) + 2 * (j % 7)] = 2.0;
  }
  if (tid < (S + 63) / 64) {      // one mask word per 64 states
    uint64_t m = 0;
    for (int j = 0; j < 64 && 64 * tid + j < S; ++j) if (pitm[64 * tid + j]) m |= 1ull << j;
    P.term_mask[(size_t)ci * ((S + 63) / 64) + tid] = m;
  }
  if (tid == 0) {
    double c = 0.0, ctot = 0.0;
    for (int k = 0; k < n_s0; ++k) ctot += s0p(k);
    for (int k = 0; k < P.s0_max; ++k) {
      if (k < n_s0) {      // cumsum(p) / cumsum(p)[-1], as numpy.random.choice forms it (anymdp_env.py:89)
        c += s0p(k);
        P.s0_cdf[(size_t)ci * P.s0_max + k] = c / ctot;
        P.s0_ids[(size_t)ci * P.s0_max + k] = s0i(k);
      } else {
        P.s0_cdf[(size_t)ci * P.s0_max + k] = 1.0;
        P.s0_ids[(size_t)ci * P.s0_max + k] = s0i(n_s0 - 1);
      }
    }
    P.max_steps[ci] = (int32_t)ceil(max_steps);
  }
}

// ---- the two kernels: carve the candidate's arrays, name the storage, run the model ----

template <int SP>
__global__ __launch_bounds__(512) void anymdp_sampler_kernel(SamplerArgs P) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  Cand C{P, (uint64_t)(P.cand_base + blockIdx.x), P.S, P.A, P.S * P.A};
  C.Qs = lds;                          // [SA]
  C.Vs = C.Qs + C.SA;                  // [SP]
  C.part = C.Vs + SP;                  // [8]
  C.pot = C.part + 8;                  // [SP] each
  C.rpos = C.pot + SP;
  C.npos = C.rpos + SP;
  C.bonus = C.npos + SP;
  C.vstate = C.bonus + SP;
  C.pitm = reinterpret_cast<int*>(C.vstate + SP);
  C.Pm = reinterpret_cast<double*>(C.pitm + SP);     // [2][SP*SP]
  C.Pm2 = C.Pm + SP * SP;
  C.bandlo = reinterpret_cast<int*>(C.Pm + 2 * SP * SP);
  C.bandhi = C.bandlo + SP;
  RegRows<SP> T;
  xs_candidate(C, T);
}

struct BigScratch {
  double* Tt;        // [n_cand][n_rb * S * 64]
  double* Pm;        // [n_cand][2 * S * S]
  int n_rb;
};

template <int R>
__global__ __launch_bounds__(1024) void anymdp_sampler_big_kernel(SamplerArgs P, BigScratch X) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int S = P.S, SAp = X.n_rb * 64;
  Cand C{P, (uint64_t)(P.cand_base + blockIdx.x), S, P.A, S * P.A};
  C.Qs = lds;                          // [SAp]
  C.Vs = C.Qs + SAp;                   // [S]
  C.part = C.Vs + S;                   // [16]
  C.pot = C.part + 16;                 // [S] each
  C.rpos = C.pot + S;
  C.npos = C.rpos + S;
  C.bonus = C.npos + S;
  C.vstate = C.bonus + S;
  C.pitm = reinterpret_cast<int*>(C.vstate + S);
  C.bandlo = C.pitm + S;
  C.bandhi = C.bandlo + S;
  C.Pm = X.Pm + (size_t)blockIdx.x * 2 * S * S;
  C.Pm2 = C.Pm + (size_t)S * S;
  BigRows<R> T;
  T.Tt = X.Tt + (size_t)blockIdx.x * SAp * S;
  T.S = S; T.SAp = SAp;
  xs_candidate(C, T);
}

}  // namespace

extern "C" int xv_anymdp_sample_tasks(xv_engine* e, uint64_t seed, int64_t cand_base, int n_cand, int S, int A, int s0_max,
                                      void* rows, int32_t* state_map, uint64_t* term_mask, double* s0_cdf,
                                      int32_t* s0_ids, int32_t* max_steps, double* transition, double* reward,
                                      double* reward_noise, xv_anymdp_cand_info* info, int32_t* status) {
  XV_CHECK_ARG(e != nullptr && status != nullptr);
  XV_CHECK_ARG(n_cand > 0 && cand_base >= 0);
  const bool small = S >= 8 && S <= 64 && A >= 2 && A <= 64 && S * A <= 512;
  const bool big = !small && S > 16 && S <= 256 && A >= 2 && A <= 64 && S * A <= 4096;
  if (!small && !big) {
    xv_set_error("xv_anymdp_sample_tasks: the device sampler covers 8 <= S <= 64 with S * A <= 512 and S <= 256 with S * A <= 4096 "
                 "(got S = %d, A = %d); larger tasks: the seeded host sampler", S, A);
    return XV_ERR_UNSUPPORTED;
  }
  XV_CHECK_ARG(s0_max >= 3 && s0_max <= 256);
  if (rows != nullptr) XV_CHECK_ARG(state_map && term_mask && s0_cdf && s0_ids && max_steps);
  XV_HIP(hipSetDevice(e->device));
  SamplerArgs P;
  P.seed = seed; P.cand_base = cand_base; P.n_cand = n_cand; P.S = S; P.A = A; P.s0_max = s0_max;
  P.row_lines = XV_ANYMDP_ROW_LINES(S);
  P.rows = static_cast<double*>(rows); P.state_map = state_map; P.term_mask = term_mask; P.s0_cdf = s0_cdf;
  P.s0_ids = s0_ids; P.max_steps = max_steps; P.transition = transition; P.reward = reward; P.noise = reward_noise;
  P.info = info; P.status = status;
  if (big) {
    // rows in a transposed global scratch (stream-ordered allocation: no synchronisation), R rows per thread
    const int SA = S * A, n_rb = (SA + 63) / 64, R = (SA + 1023) / 1024;
    const int threads = 64 * ((n_rb + R - 1) / R);
    BigScratch X;
    X.n_rb = n_rb; X.Tt = nullptr; X.Pm = nullptr;
    const size_t tt_bytes = sizeof(double) * (size_t)n_cand * n_rb * 64 * S, pm_bytes = sizeof(double) * (size_t)n_cand * 2 * S * S;
    hipError_t r = hipMallocAsync((void**)&X.Tt, tt_bytes, e->stream);
    if (r == hipSuccess) r = hipMallocAsync((void**)&X.Pm, pm_bytes, e->stream);
    if (r != hipSuccess) {
      (void)hipGetLastError();
      if (X.Tt) (void)hipFreeAsync(X.Tt, e->stream);
      xv_set_error("xv_anymdp_sample_tasks: cannot allocate %.1f GiB of candidate scratch (lower n_cand)",
                   (double)(tt_bytes + pm_bytes) / (double)(1ull << 30));
      return XV_ERR_NOMEM;
    }
    const size_t lds = sizeof(double) * ((size_t)n_rb * 64 + 6 * (size_t)S + 16) + sizeof(int) * 3 * (size_t)S;
    hipError_t attr = hipSuccess;      // a failed attribute call must not leave with the scratch allocated
#define XSB_LAUNCH(R_)                                                                                              \
  do {                                                                                                              \
    if (lds > 48 * 1024)                                                                                            \
      attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&anymdp_sampler_big_kernel<R_>),                     \
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                            \
    if (attr == hipSuccess)                                                                                         \
      hipLaunchKernelGGL(anymdp_sampler_big_kernel<R_>, dim3(n_cand), dim3(threads), lds, e->stream, P, X);         \
  } while (0)
    if (R == 1) XSB_LAUNCH(1);
    else if (R == 2) XSB_LAUNCH(2);
    else if (R == 3) XSB_LAUNCH(3);
    else XSB_LAUNCH(4);
#undef XSB_LAUNCH
    const hipError_t le = attr != hipSuccess ? attr : hipGetLastError();
    (void)hipFreeAsync(X.Tt, e->stream);
    (void)hipFreeAsync(X.Pm, e->stream);
    if (le != hipSuccess) {
      xv_set_error("xv_anymdp_sample_tasks: kernel launch failed: %s", hipGetErrorString(le));
      return XV_ERR_HIP;
    }
    return XV_OK;
  }
  const int threads = (S * A + 63) / 64 * 64;
  const int SP = S <= 16 ? 16 : (S <= 32 ? 32 : 64);      // the smallest that holds S, and S >= 8: SP / 2 <= S (RegRows::each_inner)
  const size_t lds = sizeof(double) * ((size_t)S * A + 6 * SP + 8 + 2 * (size_t)SP * SP) + sizeof(int) * 3 * SP;
#define XS_LAUNCH(SP_)                                                                                            \
  do {                                                                                                            \
    if (lds > 48 * 1024)                                                                                          \
      XV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&anymdp_sampler_kernel<SP_>),                     \
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                         \
    hipLaunchKernelGGL(anymdp_sampler_kernel<SP_>, dim3(n_cand), dim3(threads), lds, e->stream, P);               \
  } while (0)
  if (SP == 16) XS_LAUNCH(16);
  else if (SP == 32) XS_LAUNCH(32);
  else XS_LAUNCH(64);
#undef XS_LAUNCH
  XV_LAUNCH_CHECK();
  return XV_OK;
}

// ------------------------------------------------------------------------------------------------
// Observation models of AnyPOMDPTaskSampler / MultiTokensAnyPOMDPTaskSampler (task_sampler.py:78-87, :103-117) for whole
// task batches: per (task, observation token) a matrix obs[S][n_obs] = scipy.sparse.random(S, n_obs, density) — exactly
// k = round(density * S * n_obs) cells, uniformly chosen without replacement over the WHOLE matrix, values U[0, 1) —
// where a row left empty gets a 1 in a random column, every row normalised; density = min(density,
// maximum_distribution / n_obs).  Emitted as the step engine's table: the inclusive row CDF cumsum(row) / cumsum(row)[-1]
// (what numpy.random.choice forms, anymdp_env.py:150-157), obs_cdf[task][token][s][:].
// Same distribution and rules as the reference, its own stream: every cell c of matrix m draws Philox(counter = {c, m,
// purpose}, key = seed); the k chosen cells are the k smallest 64-bit keys {random high bits | cell index}, found by a
// 64-step bisection of the key threshold (no sort, no storage: keys are recomputed).  One workgroup per matrix.
// Oracle: xo_anymdp_sample_observation_model (same draws, bit-identical tables).
// ------------------------------------------------------------------------------------------------
#define XS_OBS_KEY 0x40u
#define XS_OBS_FIX 0x41u
__device__ __forceinline__ uint64_t xs_obs_key(uint64_t seed, uint64_t mat, uint32_t cell, uint64_t idx_mask, double* val) {
  const xv_u32x4 w = xv_philox4x32_10(cell, (uint32_t)mat, (uint32_t)(mat >> 32), XS_OBS_KEY, (uint32_t)seed, (uint32_t)(seed >> 32));
  if (val) *val = xv_u53(w.z, w.w);
  return ((((uint64_t)w.x << 32) | (uint64_t)w.y) & ~idx_mask) | (uint64_t)cell;
}

__global__ __launch_bounds__(256) void anymdp_obs_model_kernel(uint64_t seed, uint64_t mat_base, int S, int n_obs, long long k_cells,
                                                               double* obs_cdf) {
  __shared__ unsigned long long s_cnt;
  __shared__ unsigned long long s_thr;
  const uint64_t mat = mat_base + blockIdx.x;
  const int M = S * n_obs, tid = threadIdx.x;
  uint64_t idx_mask = 1;
  while (idx_mask < (uint64_t)M) idx_mask <<= 1;
  idx_mask -= 1;
  // smallest threshold T with #{key <= T} >= k  (keys are distinct: their low bits are the cell index)
  uint64_t lo = 0, hi = ~0ull;
  if (k_cells > 0) {
    for (int it = 0; it < 64; ++it) {
      const uint64_t mid = lo + ((hi - lo) >> 1);
      if (tid == 0) s_cnt = 0ull;
      __syncthreads();
      unsigned long long c = 0;
      for (int cell = tid; cell < M; cell += blockDim.x) c += xs_obs_key(seed, mat, (uint32_t)cell, idx_mask, nullptr) <= mid ? 1ull : 0ull;
      atomicAdd(&s_cnt, c);
      __syncthreads();
      const bool enough = s_cnt >= (unsigned long long)k_cells;
      __syncthreads();
      if (enough) hi = mid; else lo = mid + 1;
      if (lo >= hi) break;
    }
  }
  if (tid == 0) s_thr = hi;
  __syncthreads();
  const uint64_t thr = s_thr;
  double* out = obs_cdf + (size_t)blockIdx.x * (size_t)M;
  for (int row = tid; row < S; row += blockDim.x) {   // one thread per row: values, empty-row fix, cumsum, normalisation
    double* o = out + (size_t)row * n_obs;
    double acc = 0.0;
    for (int j = 0; j < n_obs; ++j) {
      double v;
      const uint64_t key = xs_obs_key(seed, mat, (uint32_t)(row * n_obs + j), idx_mask, &v);
      acc += (k_cells > 0 && key <= thr) ? v : 0.0;
      o[j] = acc;
    }
    if (acc == 0.0) {   // obs_mat[i][random.randint(observation_space)] = 1
      const xv_u32x4 w = xv_philox4x32_10((uint32_t)row, (uint32_t)mat, (uint32_t)(mat >> 32), XS_OBS_FIX, (uint32_t)seed,
                                          (uint32_t)(seed >> 32));
      const int col = (int)(((uint64_t)w.x * (uint64_t)(uint32_t)n_obs) >> 32);
      for (int j = 0; j < n_obs; ++j) o[j] = j >= col ? 1.0 : 0.0;
      acc = 1.0;
    }
    for (int j = 0; j < n_obs; ++j) o[j] = o[j] / acc;
  }
}

extern "C" int xv_anymdp_sample_observation_model(xv_engine* e, uint64_t seed, int64_t task_base, int n_task, int S, int n_obs,
                                                  int d_obs, double density, double maximum_distribution, double* obs_cdf) {
  XV_CHECK_ARG(e != nullptr && obs_cdf != nullptr);
  XV_CHECK_ARG(n_task > 0 && task_base >= 0 && S >= 1 && S <= 512 && n_obs >= 1 && n_obs <= 65536 && d_obs >= 1 && d_obs <= 64);
  XV_CHECK_ARG(density >= 0.0 && density <= 1.0 && maximum_distribution > 0.0);
  XV_CHECK_ARG((long long)S * n_obs < (1ll << 31));
  XV_HIP(hipSetDevice(e->device));
  const double d = density < maximum_distribution / (double)n_obs ? density : maximum_distribution / (double)n_obs;
  const long long k = (long long)rint(d * (double)S * (double)n_obs);     // scipy.sparse.random: int(round(density * m * n))
  const size_t n_mat = (size_t)n_task * d_obs;
  const size_t chunk = 1u << 20;
  for (size_t m0 = 0; m0 < n_mat; m0 += chunk) {
    const size_t nm = n_mat - m0 < chunk ? n_mat - m0 : chunk;
    hipLaunchKernelGGL(anymdp_obs_model_kernel, dim3((unsigned)nm), dim3(256), 0, e->stream, seed,
                       (uint64_t)task_base * (uint64_t)d_obs + m0, S, n_obs, k, obs_cdf + m0 * (size_t)S * n_obs);
  }
  XV_LAUNCH_CHECK();
  return XV_OK;
}
