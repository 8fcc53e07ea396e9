// xv_control.h — what the one-lane-per-env fp64 control families (cartpole.hip, acrobot.hip) share: the argument structs,
// the step body with its auto-reset state machine and the fused roll-out loop, the reset kernel, the Philox binding and
// the host side of the C-ABI (create / destroy / launches / get_state / set_state).  A family supplies its handle
//   struct xv_<name> { xv_engine* eng; ControlArgs a; };
// and a trait F with
//   Handle, NAME ("<name>"), N_PARAM (doubles per task row), N_OBS (even), N_ACTION (actions are 0 .. N_ACTION - 1, clamped),
//   BLOCK (workgroup size), F32_RESET (the reset state is a float32 array whose observation is float32 math: `fresh`),
//   Task + load_task(prm)                     the task row and its derived constants, loaded once per launch
//   frames(K, frameskip, action, s, reward, term, err)   the `frameskip` loop of one step on the state s[4]
//   draw_reset(P, i, tick, u)                 the four reset uniforms of env i off its Philox stream
//   reset_state(P, u, s)                      the reset state from four uniforms
//   obs(s, f32, o)                            the observation of a state
// and its extern "C" entry points as one-line calls of the templates below.
#pragma once
#include "philox.h"
#include "xv_common.h"
#include "xv_hand.h"

struct ControlArgs {
  const double* params;      // [n_task][F::N_PARAM]
  double reset_scale[4];
  const int32_t* env_task;
  double* state;             // [4][n_env]
  int32_t* steps;
  uint8_t* need_reset;
  uint32_t* err;
  int n_env, n_task, frameskip, max_steps;
  uint64_t seed, gid_base, tick;
  const uint64_t* tick_dev;   // device tick mode of the engine: the launch tick is *tick_dev + tick (xv_launch_tick)
  uint32_t* hand;             // [waves] HAND kernels only (mixed.hip): hand-off words of the waves' envs, xv_hand.h
  uint8_t* fresh;             // F32_RESET families only: state still holds the float32 reset values
  int scale_is_vector;        // F32_RESET families only: reset_bounds_scale was given as a vector (float64 reset math)
};

struct ControlIO {
  const int32_t* action;
  const double* u_reset;     // [4][n_env] (INJECT)
  float* obs;                // [n_env][F::N_OBS]
  float* reward;
  uint8_t* terminated;
  uint8_t* truncated;
  float* final_obs;          // nullable
  uint8_t* done_out;         // nullable: terminated | truncated of the same step (xv_*_step_info)
};

template <int W>
__device__ __forceinline__ void xv_control_store_obs(float* dst, const float (&o)[W]) {
  static_assert(W % 2 == 0, "observation rows are stored as float4 / float2");
  if constexpr (W % 4 == 0) {
#pragma unroll
    for (int k = 0; k < W / 4; ++k)
      reinterpret_cast<float4*>(dst)[k] = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
  } else {
#pragma unroll
    for (int k = 0; k < W / 2; ++k) reinterpret_cast<float2*>(dst)[k] = make_float2(o[2 * k], o[2 * k + 1]);
  }
}

template <class F, bool INJECT>
__device__ __forceinline__ void xv_control_reset_state(const ControlArgs& P, const double* u_in, int i, uint64_t tick,
                                                       double (&s)[4]) {
  double u[4];
  if (INJECT) {
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = u_in[(size_t)k * P.n_env + i];
  } else {
    F::draw_reset(P, i, tick, u);
  }
  F::reset_state(P, u, s);
}

template <class F, bool INJECT, bool HAND = false>
__device__ __forceinline__ void xv_control_step_body(const ControlArgs& P, const ControlIO& io, int mode, int T, int bid) {
  // T steps per launch (xv_*_rollout; T = 1 for xv_*_step): the state stays in registers, step ts reads action[ts][i],
  // writes row ts of the outputs and draws with tick + ts — the same values as T launches of one step
  // (`bid`: the workgroup's index within this family's part of the launch, see mixed.hip)
  static_assert(!(HAND && F::F32_RESET), "the hand-off carries no `fresh` byte");
  const int i = bid * blockDim.x + threadIdx.x;
  if (i >= P.n_env) return;
  const size_t N = (size_t)P.n_env;
  double s[4];
  int steps, nr, fresh = 0;
  uint32_t err = 0;
  const double* prm = P.params + (size_t)P.env_task[i] * F::N_PARAM;
  // HAND (overlapped step_many of the mixed batch, mixed.hip; T = 1): the wave waits for its word P.hand[wave] to carry this
  // step's tick — written by the same wave of the step before, after its state stores completed — and hands on likewise
  // (xv_hand.h).  The env's word in P.steps carries need_reset in bit 31 between HAND launches (mixed.hip packs / unpacks).
  if (HAND) {
    if (!xv_hand_wait(P.hand + (i >> 6), (uint32_t)xv_launch_tick(P.tick, P.tick_dev), P.err)) err |= XV_DEVERR_HANDOFF;
    asm volatile("" ::: "memory");
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = xv_agent_load_f64(P.state + k * N + i);
    const uint32_t w = xv_agent_load32(P.steps + i);
    steps = (int)(w & 0x7FFFFFFFu); nr = (int)(w >> 31);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = P.state[k * N + i];
    steps = P.steps[i];
    nr = P.need_reset[i];
    if (F::F32_RESET) fresh = P.fresh[i];
  }
  const typename F::Task K = F::load_task(prm);
  for (int ts = 0; ts < T; ++ts) {
    const size_t o = (size_t)ts * N + i;
    int action = io.action[o];
    float reward = 0.0f;
    int term = 0, trunc = 0;
    float fobs[F::N_OBS] = {};
    bool do_reset = false;
    if (mode == XV_AUTORESET_NEXT_STEP && nr) {
      do_reset = true;
    } else {
      if (action < 0 || action >= F::N_ACTION) {
        err |= XV_DEVERR_ACTION_RANGE;
        action = action < 0 ? 0 : F::N_ACTION - 1;
      }
      F::frames(K, P.frameskip, action, s, reward, term, err);
      fresh = 0;
      steps += 1;
      trunc = (P.max_steps > 0 && steps >= P.max_steps) ? 1 : 0;
      if (term || trunc) {
        if (mode == XV_AUTORESET_SAME_STEP) {
          F::obs(s, false, fobs);
          do_reset = true;
        } else if (mode == XV_AUTORESET_NEXT_STEP) {
          nr = 1;
        }
      }
    }
    if (do_reset) {
      xv_control_reset_state<F, INJECT>(P, io.u_reset, i, xv_launch_tick(P.tick, P.tick_dev) + (uint64_t)ts, s);
      fresh = 1;
      steps = 0;
      nr = 0;
    }
    float ob[F::N_OBS];
    F::obs(s, F::F32_RESET && fresh && !P.scale_is_vector, ob);
    xv_control_store_obs(io.obs + o * F::N_OBS, ob);
    io.reward[o] = reward;
    io.terminated[o] = (uint8_t)term;
    io.truncated[o] = (uint8_t)trunc;
    if (io.done_out) io.done_out[o] = (uint8_t)((term || trunc) ? 1 : 0);
    if (io.final_obs) xv_control_store_obs(io.final_obs + o * F::N_OBS, fobs);
  }
  if (HAND) {
#pragma unroll
    for (int k = 0; k < 4; ++k) xv_agent_store_f64(P.state + k * N + i, s[k]);
    xv_agent_store32(P.steps + i, (uint32_t)steps | ((uint32_t)nr << 31));
    xv_hand_publish(P.hand + (i >> 6), (uint32_t)xv_launch_tick(P.tick, P.tick_dev) + 1u);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) P.state[k * N + i] = s[k];
    P.steps[i] = steps;
    P.need_reset[i] = (uint8_t)nr;
    if (F::F32_RESET) P.fresh[i] = (uint8_t)fresh;
  }
  if (err) atomicOr(P.err, err);
}

template <class F, bool INJECT>
__global__ __launch_bounds__(F::BLOCK) void xv_control_step_kernel(ControlArgs P, ControlIO io, int mode, int T) {
  xv_control_step_body<F, INJECT>(P, io, mode, T, (int)blockIdx.x);
}

template <class F, bool INJECT>
__global__ __launch_bounds__(F::BLOCK) void xv_control_reset_kernel(ControlArgs P, const uint8_t* mask, const double* u,
                                                                    float* obs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P.n_env) return;
  if (mask && !mask[i]) return;
  const size_t N = (size_t)P.n_env;
  double s[4];
  xv_control_reset_state<F, INJECT>(P, u, i, xv_launch_tick(P.tick, P.tick_dev), s);
#pragma unroll
  for (int k = 0; k < 4; ++k) P.state[k * N + i] = s[k];
  P.steps[i] = 0;
  P.need_reset[i] = 0;
  if (F::F32_RESET) P.fresh[i] = 1;
  if (obs) {
    float ob[F::N_OBS];
    F::obs(s, F::F32_RESET && !P.scale_is_vector, ob);
    xv_control_store_obs(obs + (size_t)i * F::N_OBS, ob);
  }
}

template <class H>
static inline void xv_control_bind_rng(H* h, uint64_t ticks, bool advance = true) {
  h->a.seed = h->eng->seed;
  h->a.gid_base = h->eng->env_id_base;
  const XvTickBind b = xv_engine_bind_tick(h->eng, ticks, advance);
  h->a.tick = b.tick;
  h->a.tick_dev = b.tick_dev;
}

// ---- host side of the C-ABI ----
template <class H>
static int xv_control_destroy(H* h) {
  if (!h) return XV_OK;
  (void)hipSetDevice(h->eng->device);
  (void)hipStreamSynchronize(h->eng->stream);
  void* ps[] = {h->a.state, h->a.steps, h->a.need_reset, h->a.fresh};
  for (void* q : ps) if (q) (void)hipFree(q);
  delete h;
  return XV_OK;
}

template <class F>
static int xv_control_create(xv_engine* e, int n_env, int n_task, int frameskip, int max_steps, const double* params,
                             const double* reset_scale, int scale_is_vector, const int32_t* env_task,
                             typename F::Handle** out) {
  XV_CHECK_ARG(out != nullptr);
  *out = nullptr;
  XV_CHECK_ARG(e && params && reset_scale && env_task && n_env > 0 && n_task > 0 && frameskip >= 1);
  XV_HIP(hipSetDevice(e->device));
  typename F::Handle* h = new (std::nothrow) typename F::Handle();
  if (!h) {
    xv_set_error("xv_%s_create: out of host memory", F::NAME);
    return XV_ERR_NOMEM;
  }
  h->eng = e;
  ControlArgs& a = h->a;      // value-initialised: every pointer is null until it is set here
  a.params = params; a.env_task = env_task;
  a.n_env = n_env; a.n_task = n_task; a.frameskip = frameskip; a.max_steps = max_steps;
  a.scale_is_vector = scale_is_vector ? 1 : 0;
  a.err = e->d_err;
  a.seed = e->seed; a.gid_base = e->env_id_base;
  const size_t n = (size_t)n_env;
  hipError_t r = hipMemcpyAsync(a.reset_scale, reset_scale, sizeof(a.reset_scale), hipMemcpyDeviceToHost, e->stream);
  if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
  const char* what = r == hipSuccess ? "device allocation" : "reading reset_scale";
  if (r == hipSuccess) r = hipMalloc(&a.state, sizeof(double) * 4 * n);
  if (r == hipSuccess) r = hipMalloc(&a.steps, sizeof(int32_t) * n);
  if (r == hipSuccess) r = hipMalloc(&a.need_reset, n);
  if (r == hipSuccess && F::F32_RESET) r = hipMalloc(&a.fresh, n);
  if (r == hipSuccess) r = hipMemsetAsync(a.state, 0, sizeof(double) * 4 * n, e->stream);
  if (r == hipSuccess) r = hipMemsetAsync(a.steps, 0, sizeof(int32_t) * n, e->stream);
  if (r == hipSuccess) r = hipMemsetAsync(a.need_reset, 1, n, e->stream);
  if (r == hipSuccess && F::F32_RESET) r = hipMemsetAsync(a.fresh, 0, n, e->stream);
  if (r != hipSuccess) {      // whatever was made so far is freed, the handle included
    xv_set_error("xv_%s_create: %s failed: %s", F::NAME, what, hipGetErrorString(r));
    (void)xv_control_destroy(h);
    return XV_ERR_HIP;
  }
  *out = h;
  return XV_OK;
}

template <class F, bool INJECT>
static int xv_control_reset(typename F::Handle* h, const uint8_t* mask, const double* u, float* obs) {
  XV_CHECK_ARG(h != nullptr && (u != nullptr || !INJECT));
  xv_control_bind_rng(h, INJECT ? 0 : 1);
  hipLaunchKernelGGL((xv_control_reset_kernel<F, INJECT>), dim3(xv_div_up(h->a.n_env, F::BLOCK)), dim3(F::BLOCK), 0,
                     h->eng->stream, h->a, mask, u, obs);
  XV_LAUNCH_CHECK();
  return XV_OK;
}

// step (T = 1), step_info (io.done_out), rollout (T steps) and step_injected (INJECT: io.u_reset, no tick is consumed)
template <class F, bool INJECT>
static int xv_control_step(typename F::Handle* h, const ControlIO& io, int autoreset_mode, int T) {
  XV_CHECK_ARG(h && io.action && (io.u_reset || !INJECT) && io.obs && io.reward && io.terminated && io.truncated && T > 0);
  XV_CHECK_ARG(autoreset_mode >= 0 && autoreset_mode <= 2);
  xv_control_bind_rng(h, INJECT ? 0 : (uint64_t)T);
  hipLaunchKernelGGL((xv_control_step_kernel<F, INJECT>), dim3(xv_div_up(h->a.n_env, F::BLOCK)), dim3(F::BLOCK), 0,
                     h->eng->stream, h->a, io, autoreset_mode, T);
  XV_LAUNCH_CHECK();
  return XV_OK;
}

template <class H>
static int xv_control_get_state(H* h, double* state, int32_t* steps, uint8_t* need_reset) {
  XV_CHECK_ARG(h != nullptr);
  const size_t n = (size_t)h->a.n_env;
  if (state) XV_HIP(hipMemcpyAsync(state, h->a.state, n * 32, hipMemcpyDeviceToDevice, h->eng->stream));
  if (steps) XV_HIP(hipMemcpyAsync(steps, h->a.steps, n * 4, hipMemcpyDeviceToDevice, h->eng->stream));
  if (need_reset) XV_HIP(hipMemcpyAsync(need_reset, h->a.need_reset, n, hipMemcpyDeviceToDevice, h->eng->stream));
  return XV_OK;
}

template <class H>
static int xv_control_set_state(H* h, const double* state, const int32_t* steps, const uint8_t* need_reset) {
  XV_CHECK_ARG(h != nullptr);
  const size_t n = (size_t)h->a.n_env;
  if (state) {
    XV_HIP(hipMemcpyAsync(h->a.state, state, n * 32, hipMemcpyDeviceToDevice, h->eng->stream));
    if (h->a.fresh) XV_HIP(hipMemsetAsync(h->a.fresh, 0, n, h->eng->stream));   // a caller-supplied state is a float64 array
  }
  if (steps) XV_HIP(hipMemcpyAsync(h->a.steps, steps, n * 4, hipMemcpyDeviceToDevice, h->eng->stream));
  if (need_reset) XV_HIP(hipMemcpyAsync(h->a.need_reset, need_reset, n, hipMemcpyDeviceToDevice, h->eng->stream));
  return XV_OK;
}
