// acrobot.hip — domain-randomised Acrobot batched step / reset for gfx950 and its C-ABI.
//
// Reproduces xenoverse/metacontrol/random_acrobot.py: _dsdt :58-96 (book dynamics), _terminal :98-101,
// set_task :103-106, step :108-117 (= `frameskip` repeats of gymnasium's AcrobotEnv.step), reset :119-130.
// The integrator around _dsdt (rk4 over [0, 0.2], wrap to [-pi, pi], velocity bounds 4pi / 9pi, torques
// {-1, 0, +1}) is gymnasium's (third-party, not vendored, not installed here: restated from the public 1.x
// source — that part of the parity is unpinned); _dsdt and _terminal are pinned to the reference's own code
// through oracle/xeno_oracle.c (tests/golden/acrobot_dsdt.npz).
// One lane per env, fp64 state (the reference integrates in float64) in component-major arrays, 56 B of task
// parameters.  Same operation order as oracle/xeno_oracle.c: acrobot_substep.
#include "acrobot_wrap.h"
#include "xv_control.h"

#define AC_PI 3.141592653589793

struct xv_acrobot {
  xv_engine* eng;
  ControlArgs a;
};

struct AcrobotTask {
  double l1, m1, m2, lc1, lc2, g, I1, I2;
};

// sin and cos of an angle of this system in ~45 fp64 instructions (ocml's sincos is ~200 with its large-argument path,
// and a step evaluates 16 of them: they were four fifths of the kernel).  The classic two-step Cody-Waite reduction by
// pi/2 (x - n pio2_1 is exact: 33-bit constant, |n| < 2^20) followed by the degree-13 / degree-14 minimax kernels with the
// reduction's tail — the construction of fdlibm / msun (k_sin.c, k_cos.c, e_rem_pio2.c: public constants), restated.
// Within 1 ulp of glibc's sin / cos (96.8 % of 8e6 arguments in +-1000 identical, the rest 1 ulp off; the oracle calls
// glibc).  Domain: |x| < ~1e6 — the state is wrapped to [-pi, pi] and the velocities are bounded by 9 pi.
__device__ __forceinline__ void ac_sincos(double x, double* sn, double* cs) {
  const double fn = rint(x * 6.36619772367581382433e-01);
  double r = x - fn * 1.57079632673412561417e+00;
  const double t = r;
  double w = fn * 6.07710050630396597660e-11;
  r = t - w;
  w = fn * 2.02226624879595063154e-21 - ((t - r) - w);
  const double y0 = r - w, y1 = (r - y0) - w;
  const double z = y0 * y0, v = z * y0;
  const double rs = 8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 +
                    z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)));
  const double s = y0 - ((z * (0.5 * y1 - v * rs) - y1) - v * -1.66666666666666324348e-01);
  const double rc = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 +
                    z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
  const double hz = 0.5 * z, wv = 1.0 - hz;
  const double c = wv + (((1.0 - wv) - hz) + (z * rc - y0 * y1));
  const int n = (int)fn & 3;
  const double a = (n & 1) ? c : s, b = (n & 1) ? s : c;
  *sn = (n & 2) ? -a : a;
  *cs = ((n + 1) & 2) ? -b : b;
}
__device__ __forceinline__ double ac_cos(double x) { double sn, cs; ac_sincos(x, &sn, &cs); return cs; }

// random_acrobot.py:58-96; y = (theta1, theta2, dtheta1, dtheta2), a = torque
__device__ __forceinline__ void acrobot_dsdt(const AcrobotTask& K, const double (&y)[4], double a, double (&out)[4]) {
  const double theta1 = y[0], theta2 = y[1], dtheta1 = y[2], dtheta2 = y[3];
  double s2, c2;
  ac_sincos(theta2, &s2, &c2);
  const double d1 = K.m1 * (K.lc1 * K.lc1) + K.m2 * (K.l1 * K.l1 + K.lc2 * K.lc2 + 2 * K.l1 * K.lc2 * c2) + K.I1 + K.I2;
  const double d2 = K.m2 * (K.lc2 * K.lc2 + K.l1 * K.lc2 * c2) + K.I2;
  const double phi2 = K.m2 * K.lc2 * K.g * ac_cos(theta1 + theta2 - AC_PI / 2.0);
  const double phi1 = -K.m2 * K.l1 * K.lc2 * (dtheta2 * dtheta2) * s2 - 2 * K.m2 * K.l1 * K.lc2 * dtheta2 * dtheta1 * s2 +
                      (K.m1 * K.lc1 + K.m2 * K.l1) * K.g * ac_cos(theta1 - AC_PI / 2) + phi2;
  const double ddtheta2 = (a + d2 / d1 * phi1 - K.m2 * K.l1 * K.lc2 * (dtheta1 * dtheta1) * s2 - phi2) /
                          (K.m2 * (K.lc2 * K.lc2) + K.I2 - d2 * d2 / d1);
  const double ddtheta1 = -(d2 * ddtheta2 + phi1) / d1;
  out[0] = dtheta1; out[1] = dtheta2; out[2] = ddtheta1; out[3] = ddtheta2;
}

__device__ __forceinline__ double acrobot_bound(double x, double m, double M) {
  const double t = (m > x) ? m : x;
  return (M < t) ? M : t;
}

struct Acrobot {
  using Handle = xv_acrobot;
  using Task = AcrobotTask;
  static constexpr const char* NAME = "acrobot";
  static constexpr int N_PARAM = 7, N_OBS = 6, N_ACTION = 3, BLOCK = 64;   // params: l1, l2, m1, m2, lc1, lc2, g
  static constexpr bool F32_RESET = true;

  static __device__ __forceinline__ Task load_task(const double* prm) {
    Task K;
    K.l1 = prm[0]; K.m1 = prm[2]; K.m2 = prm[3]; K.lc1 = prm[4]; K.lc2 = prm[5]; K.g = prm[6];
    const double l2 = prm[1];
    K.I1 = K.m1 * (K.lc1 * K.lc1 + (K.l1 - K.lc1) * (K.l1 - K.lc1)) / 6.0;
    K.I2 = K.m2 * (K.lc2 * K.lc2 + (l2 - K.lc2) * (l2 - K.lc2)) / 6.0;
    return K;
  }

  static __device__ __forceinline__ void frames(const Task& K, int frameskip, int action, double (&s)[4], float& reward,
                                                int& term, uint32_t& err) {
    const double torque = (double)(action - 1);   // AVAIL_TORQUE = [-1.0, 0.0, +1]
    const double dt = 0.2, dt2 = dt / 2.0;
    double total = 0.0;
    for (int f = 0; f < frameskip; ++f) {         // :112-116
      double k1[4], k2[4], k3[4], k4[4], y[4];
      acrobot_dsdt(K, s, torque, k1);
#pragma unroll
      for (int q = 0; q < 4; ++q) y[q] = s[q] + dt2 * k1[q];
      acrobot_dsdt(K, y, torque, k2);
#pragma unroll
      for (int q = 0; q < 4; ++q) y[q] = s[q] + dt2 * k2[q];
      acrobot_dsdt(K, y, torque, k3);
#pragma unroll
      for (int q = 0; q < 4; ++q) y[q] = s[q] + dt * k3[q];
      acrobot_dsdt(K, y, torque, k4);
#pragma unroll
      for (int q = 0; q < 4; ++q) y[q] = s[q] + dt / 6.0 * (k1[q] + 2 * k2[q] + 2 * k3[q] + k4[q]);
      int stuck = 0;                              // wrap(x, -pi, pi): the reference's loop, evaluated exactly
      s[0] = xv_acrobot_wrap(y[0], &stuck);       // in O(log x) steps (acrobot_wrap.h)
      s[1] = xv_acrobot_wrap(y[1], &stuck);
      if (stuck) err |= XV_DEVERR_NONFINITE;      // the reference would loop forever here
      s[2] = acrobot_bound(y[2], -4 * AC_PI, 4 * AC_PI);
      s[3] = acrobot_bound(y[3], -9 * AC_PI, 9 * AC_PI);
      term = (-ac_cos(s[0]) - ac_cos(s[1] + s[0]) > K.l1) ? 1 : 0;   // _terminal :98-101
      total += term ? 0.0 : -1.0;
      if (term) break;
    }
    reward = (float)total;
    if (!(fabs(s[2]) <= 1.0e300) || !(fabs(s[0]) <= 1.0e300)) err |= XV_DEVERR_NONFINITE;
  }

  static __device__ __forceinline__ void draw_reset(const ControlArgs& P, int i, uint64_t tick, double (&u)[4]) {
    const xv_u32x4 w = xv_env_draw(P.seed, P.gid_base + (uint64_t)i, tick, XV_DRAW_RESET);
    const xv_u32x4 v = xv_env_draw(P.seed, P.gid_base + (uint64_t)i, tick, 3u);
    u[0] = xv_u53(w.x, w.y); u[1] = xv_u53(w.z, w.w); u[2] = xv_u53(v.x, v.y); u[3] = xv_u53(v.z, v.w);
  }

  // state = uniform(-1, 1, 4).astype(float32) * reset_bounds_scale   (:123-125)
  static __device__ __forceinline__ void reset_state(const ControlArgs& P, const double (&u)[4], double (&s)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float f = (float)(-1.0 + 2.0 * u[k]);
      s[k] = P.scale_is_vector ? (double)f * P.reset_scale[k] : (double)(f * (float)P.reset_scale[k]);
    }
  }

  // observation of a state: float32 math while the state is the float32 reset array, float64 afterwards
  static __device__ __forceinline__ void obs(const double (&s)[4], bool f32, float (&o)[6]) {
    if (f32) {
      float sn, cs;
      sincosf((float)s[0], &sn, &cs); o[0] = cs; o[1] = sn;
      sincosf((float)s[1], &sn, &cs); o[2] = cs; o[3] = sn;
    } else {
      double sn, cs;
      ac_sincos(s[0], &sn, &cs); o[0] = (float)cs; o[1] = (float)sn;
      ac_sincos(s[1], &sn, &cs); o[2] = (float)cs; o[3] = (float)sn;
    }
    o[4] = (float)s[2]; o[5] = (float)s[3];
  }
};

extern "C" int xv_acrobot_create(xv_engine* e, int n_env, int n_task, int frameskip, int max_steps, const double* params,
                                 const double* reset_scale, int scale_is_vector, const int32_t* env_task,
                                 xv_acrobot** out) {
  return xv_control_create<Acrobot>(e, n_env, n_task, frameskip, max_steps, params, reset_scale, scale_is_vector, env_task,
                                    out);
}

extern "C" int xv_acrobot_destroy(xv_acrobot* h) { return xv_control_destroy(h); }

extern "C" int xv_acrobot_reset(xv_acrobot* h, const uint8_t* mask, float* obs) {
  return xv_control_reset<Acrobot, false>(h, mask, nullptr, obs);
}

extern "C" int xv_acrobot_reset_injected(xv_acrobot* h, const uint8_t* mask, const double* u, float* obs) {
  return xv_control_reset<Acrobot, true>(h, mask, u, obs);
}

extern "C" int xv_acrobot_step(xv_acrobot* h, const int32_t* action, float* obs, float* reward, uint8_t* terminated,
                               uint8_t* truncated, float* final_obs, int autoreset_mode) {
  return xv_control_step<Acrobot, false>(h, {action, nullptr, obs, reward, terminated, truncated, final_obs, nullptr},
                                         autoreset_mode, 1);
}

// xv_acrobot_step that also writes the terminated | truncated mask from the same launch (done uint8[n_env], nullable)
extern "C" int xv_acrobot_step_info(xv_acrobot* h, const int32_t* action, float* obs, float* reward, uint8_t* terminated,
                                    uint8_t* truncated, float* final_obs, uint8_t* done, int autoreset_mode) {
  return xv_control_step<Acrobot, false>(h, {action, nullptr, obs, reward, terminated, truncated, final_obs, done},
                                         autoreset_mode, 1);
}

extern "C" int xv_acrobot_rollout(xv_acrobot* h, int T, const int32_t* action, float* obs, float* reward,
                                  uint8_t* terminated, uint8_t* truncated, float* final_obs, int autoreset_mode) {
  return xv_control_step<Acrobot, false>(h, {action, nullptr, obs, reward, terminated, truncated, final_obs, nullptr},
                                         autoreset_mode, T);
}

extern "C" int xv_acrobot_step_injected(xv_acrobot* h, const int32_t* action, const double* u_reset, float* obs,
                                        float* reward, uint8_t* terminated, uint8_t* truncated, float* final_obs,
                                        int autoreset_mode) {
  return xv_control_step<Acrobot, true>(h, {action, u_reset, obs, reward, terminated, truncated, final_obs, nullptr},
                                        autoreset_mode, 1);
}

extern "C" int xv_acrobot_get_state(xv_acrobot* h, double* state, int32_t* steps, uint8_t* need_reset) {
  return xv_control_get_state(h, state, steps, need_reset);
}

extern "C" int xv_acrobot_set_state(xv_acrobot* h, const double* state, const int32_t* steps, const uint8_t* need_reset) {
  return xv_control_set_state(h, state, steps, need_reset);
}
