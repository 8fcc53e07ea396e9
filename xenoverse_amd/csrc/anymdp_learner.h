// anymdp_learner.h — what the on-device AnyMDP learners (anymdp_qlearn.hip, anymdp_mbrl.hip) share: everything that is not
// a learning rule.  Include it after anymdp.hip (under XV_KERNELS_ONLY): it uses xv_anymdp, AnyMDPArgs and
// anymdp_max_obs_kernel.  A learner `Lr` is a struct with `xv_anymdp* h` (borrowed: the handle outlives its learners) and
// `int device`; it supplies its tables, its kernels, the two launches of xv_learner_rollout and `u_per_env()`.
#pragma once

// one step of a rollout as a learner launch sees it
struct XvLearnStepIO {
  // the step just made (learning launches)
  const int32_t* act_prev;
  const int32_t* obs;        // also where the next action is chosen from; nullptr: the env's current state (first launch)
  const int32_t* final_obs;
  const float* reward;
  const uint8_t* terminated;
  const uint8_t* truncated;
  // the next action
  const double* u_policy;    // injected uniforms [n_env][u_per_env] or nullptr (Philox)
  int32_t* action_out;
  int greedy;
};

// what every learner launch takes from the handle: sizes and the key of its policy draws.  A learner's args struct ends
// with it, after its own tables and constants (where the kernels of both learners have always read these words).
struct XvLearnerBind {
  int n_env, S, A;
  uint64_t seed, gid_base, tick;
  const uint64_t* tick_dev;
};

static XvLearnerBind xv_learner_bind(xv_anymdp* h) {
  XvLearnerBind B;
  B.n_env = h->a.n_env; B.S = h->a.S; B.A = h->a.A;
  xv_engine* e = h->eng;
  B.seed = e->seed; B.gid_base = e->env_id_base;
  // the tick the NEXT step launch will draw with (no advance: that launch advances it)
  const XvTickBind b = xv_engine_bind_tick(e, 0);
  B.tick = b.tick; B.tick_dev = b.tick_dev;
  return B;
}

// the observation env i acts from (the learner notes it in its cur_obs[i]).  obs = io.obs: what the step returned (the next
// episode's first observation when it ended), or nullptr before any step: the env's current state
__device__ __forceinline__ int xv_learner_act_obs(const AnyMDPArgs& P, const int32_t* obs, int i) {
  int o;
  if (obs) {
    o = obs[i];
  } else {
    const int t = P.env_task[i], st = (int)(P.sr[i].x & 0xFFFFu);
    o = P.state_map[(size_t)t * P.S + st];
  }
  return o;
}

// what a create checks before it allocates: MDP tasks, the whole handle, and every observation id a row of the tables.
// fn: the entry point's name; mdp_only, rows_of: that learner's words in the messages.  Leaves the handle's device current.
static int xv_anymdp_learner_check(xv_anymdp* h, const char* fn, const char* mdp_only, const char* rows_of) {
  if (h->obs_cdf != nullptr) {
    xv_set_error("%s: %s", fn, mdp_only);
    return XV_ERR_UNSUPPORTED;
  }
  if (h->parent != nullptr) {
    xv_set_error("%s: a view (xv_anymdp_view) cannot carry learners; create them on the whole handle", fn);
    return XV_ERR_UNSUPPORTED;
  }
  xv_engine* e = h->eng;
  const size_t n_map = (size_t)h->a.n_task * h->a.S;
  int* d_max = nullptr;
  int h_max = 0;
  hipError_t r = hipSetDevice(e->device);
  if (r == hipSuccess) r = hipMalloc(&d_max, sizeof(int));
  if (r == hipSuccess) r = hipMemsetAsync(d_max, 0, sizeof(int), e->stream);
  if (r == hipSuccess) {
    hipLaunchKernelGGL(anymdp_max_obs_kernel, dim3((unsigned)((n_map + 255) / 256)), dim3(256), 0, e->stream,
                       h->a.state_map, n_map, d_max);
    r = hipMemcpyAsync(&h_max, d_max, sizeof(int), hipMemcpyDeviceToHost, e->stream);
  }
  if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
  (void)hipFree(d_max);
  if (r != hipSuccess) {
    xv_set_error("%s: %s", fn, hipGetErrorString(r));
    return XV_ERR_HIP;
  }
  if (h_max >= h->a.S) {
    xv_set_error("%s: observation id %d does not index the S = %d rows of %s", fn, h_max, h->a.S, rows_of);
    return XV_ERR_UNSUPPORTED;
  }
  return XV_OK;
}

// blocks of a 256-thread grid-stride launch over n elements (n may exceed what one grid dimension holds)
static inline unsigned xv_learner_blocks(size_t n) {
  const size_t blocks = (n + 255) / 256;
  return (unsigned)(blocks < (1u << 20) ? blocks : (1u << 20));
}

// get_state / set_state: k device-to-device copies on the engine's stream between the learner's tables dev[j] (bytes[j]
// each) and the caller's arrays user[j]; a nullptr array is skipped
static int xv_learner_copy(xv_anymdp* h, bool to_learner, int k, void* const* dev, const size_t* bytes,
                           const void* const* user) {
  for (int j = 0; j < k; ++j) {
    if (!user[j]) continue;
    if (to_learner) XV_HIP(hipMemcpyAsync(dev[j], user[j], bytes[j], hipMemcpyDeviceToDevice, h->eng->stream));
    else XV_HIP(hipMemcpyAsync((void*)user[j], dev[j], bytes[j], hipMemcpyDeviceToDevice, h->eng->stream));
  }
  return XV_OK;
}

template <class Lr>
static int xv_learner_destroy(Lr* lr, void (*free_tables)(Lr*)) {
  if (!lr) return XV_OK;
  (void)hipSetDevice(lr->device);
  (void)hipStreamSynchronize(lr->h->eng->stream);   // the handle outlives its learners (xeno.h)
  free_tables(lr);
  return XV_OK;
}

#define XV_ROLLOUT_ARG(cond) \
  do { if (!(cond)) { xv_set_error("%s: invalid argument: %s", fn, #cond); return XV_ERR_INVALID; } } while (0)

// T steps of [policy -> step (SAME_STEP auto-reset) -> learner] for fn, the C-ABI entry point whose arguments these are:
// T + 1 learner launches for T steps.  first: the policy from every env's current observation; after(act): learn from the
// step just made and, when act, pick the next action (the last step only learns).  u_policy is [T][n_env][lr->u_per_env()];
// a launch whose io.u_policy is set takes injected uniforms.
template <class Lr>
static int xv_learner_rollout(const char* fn, int (*first)(Lr*, const XvLearnStepIO&),
                              int (*after)(Lr*, const XvLearnStepIO&, bool act), xv_anymdp* h, Lr* lr, int T, int greedy,
                              const double* u_policy, const double* u, const float* z, const double* u_reset,
                              int32_t* action_out, int32_t* obs, float* reward, float* reward_gt, uint8_t* terminated,
                              uint8_t* truncated, int32_t* final_obs) {
  XV_ROLLOUT_ARG(h != nullptr && lr != nullptr && lr->h == h && T > 0);
  XV_ROLLOUT_ARG(action_out && obs && reward && reward_gt && terminated && truncated && final_obs);
  const bool inject = u != nullptr;
  XV_ROLLOUT_ARG((z != nullptr) == inject && (u_reset != nullptr) == inject);
  XV_ROLLOUT_ARG(greedy || (u_policy != nullptr) == inject);
  const size_t n = (size_t)h->a.n_env, u_stride = n * (size_t)lr->u_per_env();
  const double* up = greedy ? nullptr : u_policy;
  int rc = first(lr, XvLearnStepIO{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, up, action_out, greedy});
  for (int t = 0; t < T && rc == XV_OK; ++t) {
    const size_t o = (size_t)t * n;
    if (inject)
      rc = xv_anymdp_step_injected(h, action_out + o, u + o, z + o, u_reset + o, obs + o, reward + o, reward_gt + o,
                                   terminated + o, truncated + o, final_obs + o, XV_AUTORESET_SAME_STEP);
    else
      rc = xv_anymdp_step_info(h, action_out + o, obs + o, reward + o, reward_gt + o, terminated + o, truncated + o,
                               final_obs + o, nullptr, nullptr, XV_AUTORESET_SAME_STEP);
    if (rc != XV_OK) break;
    const bool act = t + 1 < T;
    rc = after(lr, XvLearnStepIO{action_out + o, obs + o, final_obs + o, reward + o, terminated + o, truncated + o,
                                 (up && act) ? up + (size_t)(t + 1) * u_stride : nullptr,
                                 act ? action_out + o + n : nullptr, greedy}, act);
  }
  return rc;
}
#undef XV_ROLLOUT_ARG
