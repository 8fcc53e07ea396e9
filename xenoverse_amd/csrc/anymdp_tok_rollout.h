// anymdp_tok_rollout.h — fused rollouts of the POMDP / multi-token POMDP tasks: T token steps of every env in ONE launch, with
// the actions given (xv_anymdp_rollout_tokens) or chosen on the device by the ground-truth teacher, argmax_a Q[inner state]
// (xv_anymdp_rollout_tokens_teacher; anymdp_solver_opt.py:38-51, one action token per step).  anymdp.hip includes this file
// inside its `#ifndef XV_KERNELS_ONLY` block, behind the token step kernels and their host code.
//
// A step here IS the token step under XV_AUTORESET_SAME_STEP (anymdp_tok_step_kernel / anymdp_tok_step_coop_body): the same
// draws at the same (tick, purpose, words), the same arithmetic in the same order, so a rollout equals T calls of
// xv_anymdp_step_tokens bit for bit and splitting T over calls changes nothing.  The draws of step ts use tick tick0 + ts:
//   transition token k    purpose 32 + k      uniform from words (x, y), reward normal from (z, w)
//   observation token k   purpose 64 + k      (x, y) after the step, (z, w) after a restart
//   restart state         XV_DRAW_RESET       (x, y)
//   teacher's epsilon     purpose 2           x: 24-bit compare with epsilon, y % A: the random action (as the MDP teacher)
// What a step launch reads and writes per step and a rollout does not: the env record (inner state, step counter) and the
// env's constants (task, max_steps, terminal mask word / reset record) stay in registers for the whole call; P.sr[i] is read
// once and written once.
#pragma once

struct AnyMDPTokRollIO {
  const int32_t* actions;      // [T][n_env][d_act]   (given actions; nullptr for the teacher)
  const uint8_t* greedy;       // [n_task][S]         (teacher)
  float epsilon;
  int32_t* actions_out;        // [T][n_env]          (teacher: the actions taken)
  int32_t* obs;                // [T][n_env][d_obs]
  float* reward;               // [T][n_env] each
  float* reward_gt;
  uint8_t* terminated;
  uint8_t* truncated;
  int32_t* final_obs;          // [T][n_env][d_obs], nullable; -1 where the step ends no episode
};

// the teacher's action from inner state s (anymdp_step_body's teacher, same draw and arithmetic)
__device__ __forceinline__ int anymdp_tok_teacher_action(const AnyMDPArgs& P, const AnyMDPTokRollIO& io, int t, int s, uint64_t gid,
                                                         uint64_t tick) {
  int a = io.greedy[(size_t)t * P.S + s];
  if (io.epsilon > 0.0f) {
    const xv_u32x4 e = xv_env_draw(P.seed, gid, tick, 2u);
    if ((float)(e.x >> 8) * (1.0f / 16777216.0f) < io.epsilon) a = (int)(e.y % (uint32_t)P.A);
  }
  return a;
}

__device__ __forceinline__ void anymdp_pin_draw(xv_u32x4& w) {   // keeps a Philox call where it is written (hipcc sinks it to its use)
  asm volatile("" : "+v"(w.x), "+v"(w.y), "+v"(w.z), "+v"(w.w));
}

// ---- per-lane body: one lane per env, binary searches of the rows (binary and fence handles; bucket handles whose
//      observation lines are not built).  A token is a chain of dependent fp64 row reads; what is put under them: the Philox
//      call of the NEXT draw (made in front of every search), the next action (requested in front of the search it follows),
//      and the step's output stores. ----
template <bool TEACHER>
__global__ __launch_bounds__(256) void anymdp_tok_rollout_kernel(AnyMDPArgs P, AnyMDPTokArgs K, AnyMDPTokRollIO io, int T) {
  const uint64_t tick0 = xv_launch_tick(P.tick, P.tick_dev);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P.n_env) return;
  const int S = P.S, A = P.A, DO = K.d_obs, DA = K.d_act;
  const size_t N = (size_t)P.n_env;
  const int t = P.env_task[i];
  const uint64_t gid = P.gid_base + (uint64_t)i;
  const uint64_t tm0 = P.term_mask[(size_t)t * P.words];
  const int max_steps = P.max_steps[t];
  const uint2 sr0 = P.sr[i];
  int s = (int)(sr0.x & 0xFFFFu), steps = (int)sr0.y, nr = (sr0.x & XV_ANYMDP_SR_NR) ? 1 : 0;
  uint32_t err = 0;
  int a_first = TEACHER ? 0 : io.actions[(size_t)i * DA];
  xv_u32x4 w = xv_env_draw(P.seed, gid, tick0, 32u);
  for (int ts = 0; ts < T; ++ts) {
    const uint64_t tick = tick0 + (uint64_t)ts;
    const size_t o = (size_t)ts * N + (size_t)i;
    steps += 1;                       // anymdp_env.py:113, once per step
    const int trunc = steps >= max_steps;
    int term = 0;
    float rsum = 0.0f, rgsum = 0.0f;
    int a_cur = a_first;
    if (TEACHER) {
      a_cur = anymdp_tok_teacher_action(P, io, t, s, gid, tick);
      io.actions_out[o] = a_cur;
    } else if (ts + 1 < T) {
      a_first = io.actions[(o + N) * DA];      // the next step's first token, behind this step's searches
    }
    // ---- transition tokens (:120-126) ----
    for (int k = 0; k < DA; ++k) {
      int a = a_cur;
      if (a < 0 || a >= A) { err |= XV_DEVERR_ACTION_RANGE; a = a < 0 ? 0 : A - 1; }
      const uint32_t rowidx = ((uint32_t)t * S + s) * A + a;
      const double u = xv_u53(w.x, w.y);
      const float z = xv_normal1(w.z, w.w);
      const bool more = k + 1 < DA;
      if (more) a_cur = io.actions[o * DA + k + 1];
      xv_u32x4 wn = xv_env_draw(P.seed, gid, tick, more ? 32u + (uint32_t)(k + 1) : 64u);   // the next draw, under this search
      anymdp_pin_draw(wn);
      int lo = 0, m = S;
      while (m > 0) {
        const int half = m >> 1;
        if (anymdp_cdf(P, rowidx, lo + half) <= u) { lo += half + 1; m -= half + 1; }
        else m = half;
      }
      const int s2 = lo < S - 1 ? lo : S - 1;
      const float2 rsv = anymdp_rs(P, rowidx, s2);
      rsum = rsum + fmaf(rsv.y, z, rsv.x);
      rgsum = rgsum + rsv.x;
      s = s2;
      w = wn;
      if (anymdp_is_term(P, t, tm0, s2)) {
        term = 1;
        if (more) w = xv_env_draw(P.seed, gid, tick, 64u);      // the remaining tokens are not taken: observe next
        break;
      }
    }
    const bool done = term || trunc;
    // ---- observation tokens (:148-157) of the state the step ended in ----
    for (int k = 0; k < DO; ++k) {
      const double u = xv_u53(w.x, w.y);
      if (k + 1 < DO) { w = xv_env_draw(P.seed, gid, tick, 64u + (uint32_t)(k + 1)); anymdp_pin_draw(w); }
      const double* row = K.obs_cdf + ((((size_t)t * DO + k) * S) + s) * (size_t)K.n_obs;
      const int ob = xv_upper_bound_f64(row, K.n_obs, u);
      io.obs[o * DO + k] = ob;
      if (io.final_obs) io.final_obs[o * DO + k] = done ? ob : -1;
    }
    if (done) {                        // SAME_STEP: restart now, report the restart state's observation
      const xv_u32x4 v = xv_env_draw(P.seed, gid, tick, XV_DRAW_RESET);
      s = anymdp_draw_s0(P, t, xv_u53(v.x, v.y));
      steps = 0;
      nr = 0;
      for (int k = 0; k < DO; ++k) {
        const xv_u32x4 q = xv_env_draw(P.seed, gid, tick, 64u + (uint32_t)k);
        const double* row = K.obs_cdf + ((((size_t)t * DO + k) * S) + s) * (size_t)K.n_obs;
        io.obs[o * DO + k] = xv_upper_bound_f64(row, K.n_obs, xv_u53(q.z, q.w));
      }
    }
    io.reward[o] = rsum; io.reward_gt[o] = rgsum;
    io.terminated[o] = (uint8_t)term; io.truncated[o] = (uint8_t)trunc;
    w = xv_env_draw(P.seed, gid, tick + 1u, 32u);      // the next step's first transition draw
  }
  P.sr[i] = anymdp_sr_pack(s, steps, nr, anymdp_is_term(P, t, tm0, s) ? 1 : 0);
  if (err) atomicOr(P.err, err);
}

// ---- cooperative body (bucket search with observation bucket lines built): the line reader, its decode and the order of
//      requests of anymdp_tok_step_coop_body<.., HAND = false> under SAME_STEP — one transition bucket line per token, the
//      observation lines of two tokens in flight together, a restart state's lines requested with them, a draw a line cannot
//      answer searched per lane — with the T loop around it and no hand-off: the env's record never leaves its lane. ----
template <int FMT, bool PAIR, bool TEACHER>
__global__ __launch_bounds__(256) void anymdp_tok_rollout_coop_kernel(AnyMDPArgs P, AnyMDPTokArgs K, AnyMDPTokRollIO io, int T) {
  const uint64_t tick0 = xv_launch_tick(P.tick, P.tick_dev);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < P.n_env;
  const int ic = valid ? i : P.n_env - 1;
  const int lane = threadIdx.x & 63;
  const int S = P.S, A = P.A, DO = K.d_obs, DA = K.d_act, NBK = P.NBK;
  const size_t N = (size_t)P.n_env;
  const uint2 sr0 = P.sr[ic];
  const uint4 rcu = P.rs_c[ic];
  const double2 rc01 = P.rs_a[ic];
  const uint4 rb = P.rs_b[ic];
  const int t = (int)rcu.w, max_steps = (int)(rcu.z & 0x7FFFFFFu);
  const uint64_t gid = P.gid_base + (uint64_t)ic;
  uint32_t err = 0;
  int s = (int)(sr0.x & 0xFFFFu), steps = (int)sr0.y, nr = (sr0.x & XV_ANYMDP_SR_NR) ? 1 : 0;
  int cterm = (sr0.x & XV_ANYMDP_SR_TERM) ? 1 : 0;
  int a_first = TEACHER ? 0 : io.actions[(size_t)ic * DA];

  auto pin2 = [](double& x, double& y) {
    int a0 = __double2loint(x), a1 = __double2hiint(x), b0 = __double2loint(y), b1 = __double2hiint(y);
    asm volatile("" : "+v"(a0), "+v"(a1), "+v"(b0), "+v"(b1));
    x = __hiloint2double(a1, a0);
    y = __hiloint2double(b1, b0);
  };
  const int kR1 = PAIR && DO > 1 ? 1 : 0;

  for (int ts = 0; ts < T; ++ts) {
    const uint64_t tick_now = tick0 + (uint64_t)ts;
    const size_t o = (size_t)ts * N + (size_t)ic;
    auto act_draw = [&](int k, double& u, xv_u32x4& w) {
      w = xv_env_draw(P.seed, gid, tick_now, 32u + (uint32_t)k);
      u = xv_u53(w.x, w.y);
    };
    auto obs_draw = [&](int k, double& us, double& ur_) {      // both uniforms of observation token k from ONE call
      const xv_u32x4 w = xv_env_draw(P.seed, gid, tick_now, 64u + (uint32_t)k);
      us = xv_u53(w.x, w.y);
      ur_ = xv_u53(w.z, w.w);
    };
    auto obs_line = [&](int k, int state, double u) -> uint32_t {
      return ((((uint32_t)t * DO + k) * S + state) * (uint32_t)NBK) + (uint32_t)(int)(u * (double)NBK);
    };
    auto obs_pick = [&](int k, int state, double u, int id, bool beyond, bool want) -> int {
      int ob = id;
      if (want && beyond) {   // the line cannot answer this draw: search the row
        const double* row = K.obs_cdf + ((((size_t)t * DO + k) * S) + state) * (size_t)K.n_obs;
        ob = xv_upper_bound_f64(row, K.n_obs, u);
      }
      return ob;
    };
    // under the latency of the step's FIRST transition line: the uniforms of the first two observation tokens and the
    // restart state (it depends on the env's reset record and one uniform only)
    int k0r = 0, s_new = 0;
    double uS0 = 0.0, uS1 = 0.0, uR0 = 0.0, uR1 = 0.0;
    auto early_work = [&]() {
      obs_draw(0, uS0, uR0);
      if (PAIR) obs_draw(kR1, uS1, uR1);
      pin2(uS0, uS1);
      const xv_u32x4 v = xv_env_draw(P.seed, gid, tick_now, XV_DRAW_RESET);
      const double ur = xv_u53(v.x, v.y);
      k0r = (int)(rc01.x <= ur) + (int)(rc01.y <= ur) + (int)(xv_u2d(rb.x, rb.y) <= ur);
      s_new = (int)(((k0r < 2 ? rb.z : rb.w) >> (16 * (k0r & 1))) & 0xFFFFu);
      pin2(uR0, uR1);
      asm volatile("" : "+v"(k0r), "+v"(s_new));
    };

    int a_cur = a_first;
    if (TEACHER) {
      a_cur = anymdp_tok_teacher_action(P, io, t, s, gid, tick_now);
      if (valid) io.actions_out[o] = a_cur;
    }
    // ---- transition tokens (:120-126): one bucket line each ----
    float rsum = 0.0f, rgsum = 0.0f;
    int term = 0;
    steps += 1;                                                            // :113-114, once per step
    const int trunc = steps >= max_steps;
    bool alive = true;
    double u_cur;
    xv_u32x4 w_cur{0u, 0u, 0u, 0u};
    act_draw(0, u_cur, w_cur);
    for (int k = 0; k < DA; ++k) {                                         // wave-uniform trip count
      int a = a_cur;
      if (a < 0 || a >= A) { if (alive && valid) err |= XV_DEVERR_ACTION_RANGE; a = a < 0 ? 0 : A - 1; }
      const uint32_t rowidx = ((uint32_t)t * S + s) * A + a;
      AnyMDPTokLine L;
      L.issue_if(P.bucket, rowidx * (uint32_t)NBK + (uint32_t)(int)(u_cur * (double)NBK), alive, lane);
      L.send(u_cur, lane);
      __builtin_amdgcn_sched_barrier(0);
      float z = xv_normal1(w_cur.z, w_cur.w);
      double u_next = 0.0;
      xv_u32x4 w_next{0u, 0u, 0u, 0u};
      if (k + 1 < DA) {
        act_draw(k + 1, u_next, w_next);
        a_cur = io.actions[o * DA + k + 1];
      }
      if (k == 0) {
        early_work();
        if (!TEACHER && ts + 1 < T) a_first = io.actions[(o + N) * DA];   // the next step's first token, behind the line
      }
      {
        int ulo = __double2loint(u_next), uhi = __double2hiint(u_next);
        asm volatile("" : "+v"(z), "+v"(ulo), "+v"(uhi), "+v"(w_next.z), "+v"(w_next.w));
        u_next = __hiloint2double(uhi, ulo);
      }
      __builtin_amdgcn_sched_barrier(0);
      bool beyond;
      float rx, ry;
      uint32_t meta;
      L.template resolve_entry<FMT>(u_cur, lane, beyond, rx, ry, meta);
      int s2 = (int)((meta >> 16) & 0x1FFu);
      bool term2 = (meta >> 25) & 1u;
      float2 rsv = make_float2(rx, ry);
      if (alive && beyond) {   // the line cannot answer this draw: search the row
        int lo = 0, m = S;
        while (m > 0) {
          const int half = m >> 1;
          if (anymdp_cdf(P, rowidx, lo + half) <= u_cur) { lo += half + 1; m -= half + 1; }
          else m = half;
        }
        s2 = lo < S - 1 ? lo : S - 1;
        rsv = anymdp_rs(P, rowidx, s2);
        term2 = (P.term_mask[(size_t)t * P.words + (s2 >> 6)] >> (s2 & 63)) & 1ull;
      }
      if (alive) {
        rsum = rsum + fmaf(rsv.y, z, rsv.x);
        rgsum = rgsum + rsv.x;
        s = s2;
        cterm = term2 ? 1 : 0;
        if (term2) { term = 1; alive = false; }
      }
      u_cur = u_next;
      w_cur = w_next;
    }
    const bool done = term || trunc;      // SAME_STEP: the env restarts in this step

    // ---- observation tokens (:148-157), two lines in flight; a restarting env reports its restart state's observation
    //      and the step's as final_obs ----
    for (int kp = 0; kp < DO; kp += 2) {
      const int k1 = PAIR && kp + 1 < DO ? kp + 1 : kp;
      double u0 = uS0, u1 = uS1, v0 = uR0, v1 = uR1;
      if (kp > 0) {
        obs_draw(kp, u0, v0);
        obs_draw(k1, u1, v1);
      }
      AnyMDPTokLine S0, S1, Q0, Q1;
      S0.issue_if(K.obs_bucket, obs_line(kp, s, u0), true, lane);
      if (PAIR) S1.issue_if(K.obs_bucket, obs_line(k1, s, u1), k1 != kp, lane);
      Q0.issue_if(K.obs_bucket, obs_line(kp, s_new, v0), done, lane);
      if (PAIR) Q1.issue_if(K.obs_bucket, obs_line(k1, s_new, v1), done && k1 != kp, lane);
      S0.send(u0, lane);
      if (PAIR) S1.send(u1, lane);
      Q0.send(v0, lane);
      if (PAIR) Q1.send(v1, lane);
      __builtin_amdgcn_sched_barrier(0);
      int c0, c1 = 0, cr0, cr1 = 0;
      bool f0, f1 = false, fr0, fr1 = false;
      S0.resolve_obs(u0, lane, f0, c0);
      if (PAIR) S1.resolve_obs(u1, lane, f1, c1);
      const int ob0 = obs_pick(kp, s, u0, c0, f0, true), ob1 = PAIR ? obs_pick(k1, s, u1, c1, f1, k1 != kp) : 0;
      Q0.resolve_obs(v0, lane, fr0, cr0);
      if (PAIR) Q1.resolve_obs(v1, lane, fr1, cr1);
      const int rb0 = obs_pick(kp, s_new, v0, cr0, fr0, done);
      const int rb1 = PAIR ? obs_pick(k1, s_new, v1, cr1, fr1, done && k1 != kp) : 0;
      if (valid) {
        io.obs[o * DO + kp] = done ? rb0 : ob0;
        if (k1 != kp) io.obs[o * DO + k1] = done ? rb1 : ob1;
        if (io.final_obs) {
          io.final_obs[o * DO + kp] = done ? ob0 : -1;
          if (k1 != kp) io.final_obs[o * DO + k1] = done ? ob1 : -1;
        }
      }
    }
    if (done) {
      s = s_new;
      cterm = (int)((rcu.z >> (27 + k0r)) & 1u);
      steps = 0;
      nr = 0;
    }
    if (valid) {
      io.reward[o] = rsum; io.reward_gt[o] = rgsum;
      io.terminated[o] = (uint8_t)term; io.truncated[o] = (uint8_t)trunc;
    }
  }
  if (valid) {
    P.sr[i] = anymdp_sr_pack(s, steps, nr, cterm);
    if (err) atomicOr(P.err, err);
  }
}

// ---- host ----
static int anymdp_tok_launch_rollout(xv_anymdp* h, const AnyMDPTokRollIO& io, int T, bool teacher) {
  AnyMDPTokArgs K{h->obs_cdf, h->n_obs, h->d_obs, h->d_act, h->obs_bucket};
  const dim3 grid(xv_div_up(h->a.n_env, 256)), block(256);
  if (anymdp_tok_coop(h)) {
    anymdp_select_tok_variant(h, [&](auto v) {
      using V = decltype(v);
      if (teacher) hipLaunchKernelGGL((anymdp_tok_rollout_coop_kernel<V::fmt, V::pair, true>), grid, block, 0, h->eng->stream, h->a, K, io, T);
      else hipLaunchKernelGGL((anymdp_tok_rollout_coop_kernel<V::fmt, V::pair, false>), grid, block, 0, h->eng->stream, h->a, K, io, T);
    });
  } else if (teacher) {
    hipLaunchKernelGGL(anymdp_tok_rollout_kernel<true>, grid, block, 0, h->eng->stream, h->a, K, io, T);
  } else {
    hipLaunchKernelGGL(anymdp_tok_rollout_kernel<false>, grid, block, 0, h->eng->stream, h->a, K, io, T);
  }
  XV_LAUNCH_CHECK();
  return XV_OK;
}

extern "C" int xv_anymdp_rollout_tokens(xv_anymdp* h, int T, const int32_t* actions, int32_t* obs, float* reward, float* reward_gt,
                                        uint8_t* terminated, uint8_t* truncated, int32_t* final_obs) {
  XV_CHECK_ARG(h && h->obs_cdf && T > 0 && actions && obs && reward && reward_gt && terminated && truncated);
  anymdp_bind_rng(h, (uint64_t)T);
  AnyMDPTokRollIO io{};
  io.actions = actions; io.obs = obs; io.reward = reward; io.reward_gt = reward_gt;
  io.terminated = terminated; io.truncated = truncated; io.final_obs = final_obs;
  return anymdp_tok_launch_rollout(h, io, T, false);
}

extern "C" int xv_anymdp_rollout_tokens_teacher(xv_anymdp* h, int T, const uint8_t* greedy, float epsilon, int32_t* actions_out,
                                                int32_t* obs, float* reward, float* reward_gt, uint8_t* terminated,
                                                uint8_t* truncated, int32_t* final_obs) {
  XV_CHECK_ARG(h && h->obs_cdf && T > 0 && greedy && actions_out && obs && reward && reward_gt && terminated && truncated);
  XV_CHECK_ARG(epsilon >= 0.0f && epsilon <= 1.0f);
  if (h->d_act > 1) {
    xv_set_error("xv_anymdp_rollout_tokens_teacher: the teacher emits one action token per step (AnyMDPSolverOpt.policy returns "
                 "a scalar; its multi-token branch tests for the type name 'MTMDP', which no sampler produces); this handle "
                 "takes d_act = %d", h->d_act);
    return XV_ERR_UNSUPPORTED;
  }
  anymdp_bind_rng(h, (uint64_t)T);
  AnyMDPTokRollIO io{};
  io.greedy = greedy; io.epsilon = epsilon; io.actions_out = actions_out; io.obs = obs; io.reward = reward;
  io.reward_gt = reward_gt; io.terminated = terminated; io.truncated = truncated; io.final_obs = final_obs;
  return anymdp_tok_launch_rollout(h, io, T, true);
}
