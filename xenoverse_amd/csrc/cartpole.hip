// cartpole.hip — domain-randomised CartPole batched step / reset for gfx950 and its C-ABI.
//
// Reproduces xenoverse/metacontrol/random_cartpole.py (set_task :46-50, step :52-61 = `frameskip` repeats of
// gymnasium's CartPoleEnv.step, reset :63-75).  The physics equations are gymnasium's (third-party, not
// vendored, not installed here: restated from the public 1.x source — parity unpinned).
// One lane per env, 4 fp64 state words in component-major arrays (coalesced), 32 B of task parameters: gymnasium keeps
// `self.state` and the whole Euler update in float64 and casts only the returned observation to float32 — so does
// this kernel (an fp32 state would drift from the reference within tens of steps and move the step at which the
// |x| > 2.4 / |theta| > 12 deg termination fires).
// Same operation order as oracle/xeno_oracle.c: cartpole_step_one.
#include "xv_control.h"

using CartPoleArgs = ControlArgs;   // the names mixed.hip uses
using CartPoleIO = ControlIO;

struct xv_cartpole {
  xv_engine* eng;
  ControlArgs a;
};

struct CartPole {
  using Handle = xv_cartpole;
  static constexpr const char* NAME = "cartpole";
  static constexpr int N_PARAM = 4, N_OBS = 4, N_ACTION = 2, BLOCK = 256;   // params: gravity, masscart, masspole, length
  static constexpr bool F32_RESET = false;
  struct Task { double gravity, masspole, length, polemass_length, total_mass; };

  static __device__ __forceinline__ Task load_task(const double* prm) {
    const double gravity = prm[0], masscart = prm[1], masspole = prm[2], length = prm[3];
    return Task{gravity, masspole, length, masspole * length /* :49 */, masspole + masscart /* :50 */};
  }

  static __device__ __forceinline__ void frames(const Task& K, int frameskip, int action, double (&s)[4], float& reward,
                                                int& term, uint32_t& err) {
    double x = s[0], xd = s[1], th = s[2], thd = s[3];
    const double force = action == 1 ? 10.0 : -10.0;
    const double theta_threshold = 12 * 2 * 3.141592653589793 / 360, x_threshold = 2.4, tau = 0.02;
    for (int f = 0; f < frameskip; ++f) {            // :56-60
      double sn, cs;
      sincos(th, &sn, &cs);
      const double temp = (force + K.polemass_length * (thd * thd) * sn) / K.total_mass;
      const double thacc = (K.gravity * sn - cs * temp) / (K.length * (4.0 / 3.0 - K.masspole * (cs * cs) / K.total_mass));
      const double xacc = temp - K.polemass_length * thacc * cs / K.total_mass;
      x = x + tau * xd;
      xd = xd + tau * xacc;
      th = th + tau * thd;
      thd = thd + tau * thacc;
      term = ((x < -x_threshold) || (x > x_threshold) || (th < -theta_threshold) || (th > theta_threshold)) ? 1 : 0;
      reward += 1.0f;
      if (term) break;
    }
    if (!(fabs(x) <= 1.0e300) || !(fabs(thd) <= 1.0e300)) err |= XV_DEVERR_NONFINITE;
    s[0] = x; s[1] = xd; s[2] = th; s[3] = thd;
  }

  static __device__ __forceinline__ void draw_reset(const ControlArgs& P, int i, uint64_t tick, double (&u)[4]) {
    const xv_u32x4 w = xv_env_draw(P.seed, P.gid_base + (uint64_t)i, tick, XV_DRAW_RESET);
    u[0] = (double)w.x * (1.0 / 4294967296.0); u[1] = (double)w.y * (1.0 / 4294967296.0);
    u[2] = (double)w.z * (1.0 / 4294967296.0); u[3] = (double)w.w * (1.0 / 4294967296.0);
  }

  // state = uniform(-1, 1, 4) * reset_bounds_scale   (random_cartpole.py:70)
  static __device__ __forceinline__ void reset_state(const ControlArgs& P, const double (&u)[4], double (&s)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = fma(2.0, u[k], -1.0) * P.reset_scale[k];
  }

  // the float32 cast of :75
  static __device__ __forceinline__ void obs(const double (&s)[4], bool, float (&o)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (float)s[k];
  }
};

// the step of the mixed batch (mixed.hip) calls the body from its own kernels
template <bool INJECT, bool HAND = false>
__device__ __forceinline__ void cartpole_step_body(const CartPoleArgs& P, const CartPoleIO& io, int mode, int T, int bid) {
  xv_control_step_body<CartPole, INJECT, HAND>(P, io, mode, T, bid);
}

#ifndef XV_KERNELS_ONLY   // mixed.hip includes this file for its kernels and handle types only
extern "C" int xv_cartpole_create(xv_engine* e, int n_env, int n_task, int frameskip, int max_steps,
                                  const double* params, const double* reset_scale, const int32_t* env_task,
                                  xv_cartpole** out) {
  return xv_control_create<CartPole>(e, n_env, n_task, frameskip, max_steps, params, reset_scale, 0, env_task, out);
}

extern "C" int xv_cartpole_destroy(xv_cartpole* h) { return xv_control_destroy(h); }

extern "C" int xv_cartpole_reset(xv_cartpole* h, const uint8_t* mask, float* obs) {
  return xv_control_reset<CartPole, false>(h, mask, nullptr, obs);
}

extern "C" int xv_cartpole_reset_injected(xv_cartpole* h, const uint8_t* mask, const double* u, float* obs) {
  return xv_control_reset<CartPole, true>(h, mask, u, obs);
}

extern "C" int xv_cartpole_step(xv_cartpole* h, const int32_t* action, float* obs, float* reward,
                                uint8_t* terminated, uint8_t* truncated, float* final_obs, int autoreset_mode) {
  return xv_control_step<CartPole, false>(h, {action, nullptr, obs, reward, terminated, truncated, final_obs, nullptr},
                                          autoreset_mode, 1);
}

// xv_cartpole_step that also writes the terminated | truncated mask from the same launch (done uint8[n_env], nullable)
extern "C" int xv_cartpole_step_info(xv_cartpole* h, const int32_t* action, float* obs, float* reward, uint8_t* terminated,
                                     uint8_t* truncated, float* final_obs, uint8_t* done, int autoreset_mode) {
  return xv_control_step<CartPole, false>(h, {action, nullptr, obs, reward, terminated, truncated, final_obs, done},
                                          autoreset_mode, 1);
}

extern "C" int xv_cartpole_rollout(xv_cartpole* h, int T, const int32_t* action, float* obs, float* reward,
                                   uint8_t* terminated, uint8_t* truncated, float* final_obs, int autoreset_mode) {
  return xv_control_step<CartPole, false>(h, {action, nullptr, obs, reward, terminated, truncated, final_obs, nullptr},
                                          autoreset_mode, T);
}

extern "C" int xv_cartpole_step_injected(xv_cartpole* h, const int32_t* action, const double* u_reset, float* obs,
                                         float* reward, uint8_t* terminated, uint8_t* truncated,
                                         float* final_obs, int autoreset_mode) {
  return xv_control_step<CartPole, true>(h, {action, u_reset, obs, reward, terminated, truncated, final_obs, nullptr},
                                         autoreset_mode, 1);
}

extern "C" int xv_cartpole_get_state(xv_cartpole* h, double* state, int32_t* steps, uint8_t* need_reset) {
  return xv_control_get_state(h, state, steps, need_reset);
}

extern "C" int xv_cartpole_set_state(xv_cartpole* h, const double* state, const int32_t* steps,
                                     const uint8_t* need_reset) {
  return xv_control_set_state(h, state, steps, need_reset);
}
#endif   // XV_KERNELS_ONLY
