// anymdp_qlearn.hip — Q-learning agents on the device: the reference's AnyMDPSolverQ (xenoverse/anymdp/anymdp_solver_q.py)
// for every env of an xv_anymdp handle, one agent per env, driven by the reference's training loop (anymdp/test_utils.py:
// epoch_run :42-60: policy -> step -> learner, reset on done) with SAME_STEP auto-reset.  Host restatement and the full
// statement of the semantics: xenoverse_amd/anymdp/qlearner.py.  Per agent, in fp64 (states are observations):
//   learner :30-49  lr = sqrt(max((M + 1) / (M + sa[s, a]), 1e-3)); terminated: Q[ns, :] = 0, target = r, else
//                   target = r + gamma max(Q[ns]); Q[s, a] += alpha lr (target - Q[s, a]); sa[s, a] += 1; sv[s] += 1
//   policy  :51-59  greedy: first argmax Q[o];  else v = Q[o] - max, k = min((M + sv[o]) / (M + 1), 10),
//                   v = v / max(std(v), 1e-2) k, p = exp(v) / sum(exp(v)), a = #{cumsum(p) / cumsum(p)[-1] <= u}
// Sums and the population std use numpy's pairwise order of a length-A row (xv_np_sum; anymdp_vi_host.hip: np_sum).  The
// learner update uses + - * / sqrt max only, and the build keeps -ffp-contract=off, so it is bit-for-bit the host's; exp is
// the device's, so a probability may differ from numpy's in its last bit (an action only where u lies within ~1e-15 of a
// cut).  The learner learns from the step's fp32 reward widened to fp64: the reference's reward is fp64 and the engine's
// rewards already differ from it by up to ~1e-5 relative.
//
// Layout: agent state in HBM, one lane per env — Q fp64 [N][S][A] (a row contiguous for its lane), sa_visits u32 [N][S][A],
// s_visits u32 [N][S], and the observation the env's last action was chosen from, int32 [N].  A rollout issues from C, per
// step, the existing step launch (xv_anymdp_step_info; xv_anymdp_step_injected with injected draws) and then ONE learner
// launch that learns from that step's (s, a, ns = done ? final_obs : obs, r, terminated) and picks the next action from
// obs: T + 1 learner launches for T steps (the first only picks, the last only learns).  The policy draw is Philox keyed by
// (engine seed, global env id, the launch tick of the step that takes the action, XV_DRAW_QPOLICY), so results do not depend
// on how T is split across calls or how envs are sharded.
#define XV_KERNELS_ONLY
#include "anymdp.hip"
#undef XV_KERNELS_ONLY
#include "anymdp_learner.h"

#define XV_DRAW_QPOLICY 4u   // words 0,1 -> the uniform numpy.random.choice searches in the Q-learner's policy

struct xv_anymdp_qlearn {
  xv_anymdp* h;        // borrowed: must outlive the learner
  int device;
  double gamma, alpha;
  int max_steps;
  int n_env, S, A;
  double* q;           // [n_env][S][A]
  uint32_t* sa;        // [n_env][S][A]
  uint32_t* sv;        // [n_env][S]
  int32_t* cur_obs;    // [n_env]
  int u_per_env() const { return 1; }   // the policy's uniforms per env and step (random.choice draws one)
};

struct QLArgs {
  double* q;
  uint32_t* sa;
  uint32_t* sv;
  int32_t* cur_obs;
  double gamma, alpha, M;
  XvLearnerBind B;
};

// numpy's sum of the n <= AM values f(0..n-1): add.reduce of a contiguous row (pairwise_sum: a plain loop below 8, eight
// partial sums from 8 up), onto the identity 0.  Every k is a compile-time index (the loops unroll over AM, n is checked), so
// f can read a register array.
template <int AM, class F>
__device__ __forceinline__ double xv_np_sum(const F& f, int n) {
  static_assert(AM >= 8 && AM <= 128, "xv_np_sum: 8 <= AM <= 128");
  if (n < 8) {
    double res = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < n) res += f(k);
    return 0.0 + res;
  }
  double r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = f(j);
  const int body = n - (n % 8);
#pragma unroll
  for (int k = 8; k < AM; ++k)
    if (k < body) r[k & 7] += f(k);
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
  for (int k = 8; k < AM; ++k)
    if (k >= body && k < n) res += f(k);
  return 0.0 + res;
}

// policy() :51-59 on one row (A <= AM doubles); u: the uniform random.choice consumes.  The row, then exp(v), then the
// cumulative sum live in one register array: one exp per action.
template <int AM>
__device__ __forceinline__ int qlearn_choice(const double* row, int A, uint32_t s_visits, double M, double u) {
  double v[AM];
#pragma unroll
  for (int k = 0; k < AM; ++k) v[k] = k < A ? row[k] : 0.0;
  double m = v[0];
#pragma unroll
  for (int k = 1; k < AM; ++k)
    if (k < A) m = v[k] > m ? v[k] : m;
#pragma unroll
  for (int k = 0; k < AM; ++k) v[k] = v[k] - m;                       // value = Q[state] - max
  const double stiff = fmin((M + (double)s_visits) / (M + 1.0), 10.0);
  const double mean = xv_np_sum<AM>([&](int k) { return v[k]; }, A) / (double)A;
  const double var = xv_np_sum<AM>([&](int k) { const double d = v[k] - mean; return d * d; }, A) / (double)A;
  const double den = fmax(sqrt(var), 1.0e-2);
#pragma unroll
  for (int k = 0; k < AM; ++k) v[k] = k < A ? exp(v[k] / den * stiff) : 0.0;
  const double z = xv_np_sum<AM>([&](int k) { return v[k]; }, A);
  double c = 0.0;
#pragma unroll
  for (int k = 0; k < AM; ++k)
    if (k < A) { c += v[k] / z; v[k] = c; }                             // cumsum(p)
  int a = 0;
#pragma unroll
  for (int k = 0; k < AM; ++k)                                          // searchsorted(cumsum / cumsum[-1], u, 'right')
    if (k < A) a += (v[k] / c <= u) ? 1 : 0;
  return a < A ? a : A - 1;
}

template <bool LEARN, bool ACT, bool INJECT, int AM>
__global__ __launch_bounds__(256) void anymdp_qlearn_kernel(AnyMDPArgs P, QLArgs L, XvLearnStepIO io) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L.B.n_env) return;
  const int S = L.B.S, A = L.B.A;
  double* Qe = L.q + (size_t)i * S * A;
  uint32_t* SAe = L.sa + (size_t)i * S * A;
  uint32_t* SVe = L.sv + (size_t)i * S;
  if (LEARN) {   // learner(s, a, ns, r, terminated, truncated) :30-49; truncation bootstraps like any other step
    const int s = L.cur_obs[i], a = io.act_prev[i];
    const bool term = io.terminated[i] != 0;
    const int ns = term || io.truncated[i] != 0 ? io.final_obs[i] : io.obs[i];
    if ((unsigned)s < (unsigned)S && (unsigned)a < (unsigned)A && (unsigned)ns < (unsigned)S) {
      const double r = (double)io.reward[i];
      double* qs = Qe + (size_t)s * A;
      double* qn = Qe + (size_t)ns * A;
      const uint32_t n_sa = SAe[(size_t)s * A + a];
      const double lr = sqrt(fmax((L.M + 1.0) / (L.M + (double)n_sa), 1.0e-3));
      double target;
      if (term) {
        for (int k = 0; k < A; ++k) qn[k] = 0.0;
        target = r;
      } else {
        double m = qn[0];
        for (int k = 1; k < A; ++k) m = qn[k] > m ? qn[k] : m;
        target = r + L.gamma * m;
      }
      const double q_sa = qs[a];
      qs[a] = q_sa + L.alpha * lr * (target - q_sa);
      SAe[(size_t)s * A + a] = n_sa + 1u;
      SVe[s] += 1u;
    }
  }
  if (ACT) {
    const int o = xv_learner_act_obs(P, io.obs, i);
    L.cur_obs[i] = o;
    int a = 0;
    if ((unsigned)o < (unsigned)S) {
      const double* row = Qe + (size_t)o * A;
      if (io.greedy) {    // numpy.argmax: the first maximum
        double m = row[0];
        for (int k = 1; k < A; ++k)
          if (row[k] > m) { m = row[k]; a = k; }
      } else {
        double u;
        if (INJECT) {
          u = io.u_policy[i];
        } else {
          const xv_u32x4 w = xv_env_draw(L.B.seed, L.B.gid_base + (uint64_t)i, xv_launch_tick(L.B.tick, L.B.tick_dev), XV_DRAW_QPOLICY);
          u = xv_u53(w.x, w.y);
        }
        a = qlearn_choice<AM>(row, A, SVe[o], L.M, u);
      }
    }
    io.action_out[i] = a;
  }
}

// __init__ :8-27 for the masked agents (nullptr: all)
static __global__ __launch_bounds__(256) void anymdp_qlearn_reset_kernel(QLArgs L, const uint8_t* mask) {
  const size_t per = (size_t)L.B.S * L.B.A, total = (size_t)L.B.n_env * per;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t i = idx / per;
    if (mask && !mask[i]) continue;
    L.q[idx] = 1.0 / (1.0 - L.gamma);
    L.sa[idx] = 1u;
    const size_t j = idx - i * per;
    if (j < (size_t)L.B.S) L.sv[i * L.B.S + j] = 1u;
  }
}

static QLArgs qlearn_args(xv_anymdp_qlearn* ql) {
  QLArgs L;
  L.q = ql->q; L.sa = ql->sa; L.sv = ql->sv; L.cur_obs = ql->cur_obs;
  L.gamma = ql->gamma; L.alpha = ql->alpha; L.M = (double)ql->max_steps;
  L.B = xv_learner_bind(ql->h);
  return L;
}

static void qlearn_free(xv_anymdp_qlearn* ql) {
  if (ql->q) (void)hipFree(ql->q);
  if (ql->sa) (void)hipFree(ql->sa);
  if (ql->sv) (void)hipFree(ql->sv);
  if (ql->cur_obs) (void)hipFree(ql->cur_obs);
  delete ql;
}

extern "C" int xv_anymdp_qlearn_reset(xv_anymdp_qlearn* ql, const uint8_t* mask) {
  XV_CHECK_ARG(ql != nullptr);
  hipLaunchKernelGGL(anymdp_qlearn_reset_kernel, dim3(xv_learner_blocks((size_t)ql->n_env * ql->S * ql->A)), dim3(256), 0,
                     ql->h->eng->stream, qlearn_args(ql), mask);
  XV_LAUNCH_CHECK();
  return XV_OK;
}

extern "C" int xv_anymdp_qlearn_create(xv_anymdp* h, double gamma, double alpha, int max_steps, xv_anymdp_qlearn** out) {
  XV_CHECK_ARG(out != nullptr);
  *out = nullptr;
  XV_CHECK_ARG(h != nullptr && gamma >= 0.0 && gamma < 1.0 && alpha == alpha && max_steps >= 0);
  // anymdp_solver_q.py:17: assert env.task_type == "MDP"; Q rows are indexed by observation id: every id must be a row
  int rc = xv_anymdp_learner_check(h, __func__,
                                   "the Q-learner takes MDP tasks only (the reference asserts task_type == \"MDP\")", "Q");
  if (rc != XV_OK) return rc;
  xv_engine* e = h->eng;
  xv_anymdp_qlearn* ql = new (std::nothrow) xv_anymdp_qlearn();
  if (!ql) {
    xv_set_error("xv_anymdp_qlearn_create: out of host memory");
    return XV_ERR_NOMEM;
  }
  ql->h = h; ql->device = e->device; ql->gamma = gamma; ql->alpha = alpha; ql->max_steps = max_steps;
  ql->n_env = h->a.n_env; ql->S = h->a.S; ql->A = h->a.A;
  const size_t nsa = (size_t)ql->n_env * ql->S * ql->A, ns = (size_t)ql->n_env * ql->S;
  hipError_t r = hipMalloc(&ql->q, sizeof(double) * nsa);
  if (r == hipSuccess) r = hipMalloc(&ql->sa, sizeof(uint32_t) * nsa);
  if (r == hipSuccess) r = hipMalloc(&ql->sv, sizeof(uint32_t) * ns);
  if (r == hipSuccess) r = hipMalloc(&ql->cur_obs, sizeof(int32_t) * (size_t)ql->n_env);
  if (r != hipSuccess) {
    (void)hipGetLastError();
    xv_set_error("xv_anymdp_qlearn_create: %zu bytes of agent tables do not fit: %s",
                 nsa * (sizeof(double) + sizeof(uint32_t)) + ns * sizeof(uint32_t), hipGetErrorString(r));
    qlearn_free(ql);
    return r == hipErrorOutOfMemory ? XV_ERR_NOMEM : XV_ERR_HIP;
  }
  r = hipMemsetAsync(ql->cur_obs, 0, sizeof(int32_t) * (size_t)ql->n_env, e->stream);
  if (r != hipSuccess) {
    xv_set_error("xv_anymdp_qlearn_create: %s", hipGetErrorString(r));
    qlearn_free(ql);
    return XV_ERR_HIP;
  }
  rc = xv_anymdp_qlearn_reset(ql, nullptr);
  if (rc != XV_OK) {
    qlearn_free(ql);
    return rc;
  }
  *out = ql;
  return XV_OK;
}

extern "C" int xv_anymdp_qlearn_destroy(xv_anymdp_qlearn* ql) { return xv_learner_destroy(ql, qlearn_free); }

static int qlearn_copy(xv_anymdp_qlearn* ql, bool to_learner, const void* q, const void* sa_visits, const void* s_visits) {
  const size_t nsa = (size_t)ql->n_env * ql->S * ql->A, ns = (size_t)ql->n_env * ql->S;
  void* const dev[3] = {ql->q, ql->sa, ql->sv};
  const size_t bytes[3] = {sizeof(double) * nsa, sizeof(uint32_t) * nsa, sizeof(uint32_t) * ns};
  const void* const user[3] = {q, sa_visits, s_visits};
  return xv_learner_copy(ql->h, to_learner, 3, dev, bytes, user);
}

extern "C" int xv_anymdp_qlearn_get_state(xv_anymdp_qlearn* ql, double* q, uint32_t* sa_visits, uint32_t* s_visits) {
  XV_CHECK_ARG(ql != nullptr);
  return qlearn_copy(ql, false, q, sa_visits, s_visits);
}

extern "C" int xv_anymdp_qlearn_set_state(xv_anymdp_qlearn* ql, const double* q, const uint32_t* sa_visits,
                                          const uint32_t* s_visits) {
  XV_CHECK_ARG(ql != nullptr);
  return qlearn_copy(ql, true, q, sa_visits, s_visits);
}

template <bool LEARN, bool ACT, bool INJECT, int AM>
static void qlearn_launch_am(xv_anymdp_qlearn* ql, const QLArgs& L, const XvLearnStepIO& io) {
  hipLaunchKernelGGL((anymdp_qlearn_kernel<LEARN, ACT, INJECT, AM>), dim3(xv_div_up(ql->n_env, 256)), dim3(256), 0,
                     ql->h->eng->stream, ql->h->a, L, io);
}

// the policy's register row: the smallest of 8, 16, 32, 64 doubles that holds A (a launch that only learns needs none)
template <bool LEARN, bool ACT, bool INJECT>
static void qlearn_launch_inj(xv_anymdp_qlearn* ql, const QLArgs& L, const XvLearnStepIO& io) {
  if constexpr (!ACT) qlearn_launch_am<LEARN, ACT, INJECT, 8>(ql, L, io);
  else if (ql->A <= 8) qlearn_launch_am<LEARN, ACT, INJECT, 8>(ql, L, io);
  else if (ql->A <= 16) qlearn_launch_am<LEARN, ACT, INJECT, 16>(ql, L, io);
  else if (ql->A <= 32) qlearn_launch_am<LEARN, ACT, INJECT, 32>(ql, L, io);
  else qlearn_launch_am<LEARN, ACT, INJECT, 64>(ql, L, io);
}

template <bool LEARN, bool ACT>
static int qlearn_launch(xv_anymdp_qlearn* ql, const XvLearnStepIO& io) {
  const QLArgs L = qlearn_args(ql);
  if (io.u_policy) qlearn_launch_inj<LEARN, ACT, true>(ql, L, io);
  else qlearn_launch_inj<LEARN, ACT, false>(ql, L, io);
  XV_LAUNCH_CHECK();
  return XV_OK;
}

static int qlearn_first(xv_anymdp_qlearn* ql, const XvLearnStepIO& io) { return qlearn_launch<false, true>(ql, io); }
static int qlearn_after(xv_anymdp_qlearn* ql, const XvLearnStepIO& io, bool act) {
  return act ? qlearn_launch<true, true>(ql, io) : qlearn_launch<true, false>(ql, io);
}

extern "C" int xv_anymdp_rollout_qlearn(xv_anymdp* h, xv_anymdp_qlearn* ql, int T, int greedy, const double* u_policy,
                                        const double* u, const float* z, const double* u_reset, int32_t* action_out,
                                        int32_t* obs, float* reward, float* reward_gt, uint8_t* terminated,
                                        uint8_t* truncated, int32_t* final_obs) {
  return xv_learner_rollout(__func__, qlearn_first, qlearn_after, h, ql, T, greedy, u_policy, u, z, u_reset, action_out, obs,
                            reward, reward_gt, terminated, truncated, final_obs);
}
