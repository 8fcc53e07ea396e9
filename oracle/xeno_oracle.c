/* xeno_oracle.c — CPU restatement of the Xenoverse env-step hot path.  TEST INFRASTRUCTURE.
 *
 * See xeno_oracle.h for who may use this.  Written from the semantics of the reference (cited per
 * function as file:line under /root/reference/xenoverse), not from its text: the reference is one Python
 * object per env with numpy's global RNG; this is a scalar loop over a struct-of-arrays batch with the
 * random inputs passed in (or drawn from Philox with the device's counter convention).
 *
 * Build: oracle/Makefile  (-O2 -ffp-contract=off: no fused multiply-add is formed unless written as
 * fma()/fmaf(), so float results are reproducible and match the device code, which spells out its FMAs).
 */
#include "xeno_oracle.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

/* ------------------------------------------------------------------------------------------------
 * Philox4x32-10 and the draw conventions shared with the device (xenoverse_amd/csrc/philox.h)
 * ---------------------------------------------------------------------------------------------- */
void xo_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
  uint32_t k0 = key[0], k1 = key[1];
  for (int r = 0; r < 10; ++r) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    uint32_t n1 = (uint32_t)p1;
    uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    uint32_t n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

void xo_env_draw(uint64_t seed, uint64_t gid, uint64_t tick, uint32_t purpose, uint32_t out[4]) {
  uint32_t ctr[4] = {(uint32_t)gid, (uint32_t)(gid >> 32), (uint32_t)tick,
                     (purpose & 0xFFu) | ((uint32_t)(tick >> 32) << 8)};
  uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  xo_philox4x32_10(ctr, key, out);
}

/* draw family with a wide sub-index: the sub-index enters the key (xv_env_draw_sub of csrc/philox.h) */
void xo_env_draw_sub(uint64_t seed, uint64_t gid, uint64_t tick, uint32_t purpose, uint32_t sub, uint32_t out[4]) {
  uint32_t ctr[4] = {(uint32_t)gid, (uint32_t)(gid >> 32), (uint32_t)tick,
                     (purpose & 0xFFu) | ((uint32_t)(tick >> 32) << 8)};
  uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32) ^ (0x80000000u | sub)};
  xo_philox4x32_10(ctr, key, out);
}

/* numpy legacy random_sample: (a>>5, b>>6) -> 53-bit double */
double xo_u53(uint32_t a, uint32_t b) {
  return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) / 9007199254740992.0;
}

void xo_box_muller(uint32_t a, uint32_t b, float* z0, float* z1) {
  double u1 = ((double)(a >> 8) + 1.0) * (1.0 / 16777216.0); /* (0,1] */
  double u2 = (double)(b >> 8) * (1.0 / 16777216.0);         /* [0,1) */
  double r = sqrt(-2.0 * log(u1));
  double ang = 6.283185307179586476925286766559 * u2;
  if (z0) *z0 = (float)(r * cos(ang));
  if (z1) *z1 = (float)(r * sin(ang));
}

/* eight normals from one Philox call (csrc/philox.h: xv_box_muller16): word p -> pair p, radius from the high 16 bits,
 * angle from the low 16 */
void xo_box_muller16(uint32_t w, float* z0, float* z1) {
  double u1 = ((double)(w >> 16) + 1.0) * (1.0 / 65536.0); /* (0,1] */
  double u2 = (double)(w & 0xFFFFu) * (1.0 / 65536.0);     /* [0,1) */
  double r = sqrt(-2.0 * log(u1));
  double ang = 6.283185307179586476925286766559 * u2;
  if (z0) *z0 = (float)(r * cos(ang));
  if (z1) *z1 = (float)(r * sin(ang));
}

int xo_max_threads(void) {
#ifdef _OPENMP
  return omp_get_max_threads();
#else
  return 1;
#endif
}

/* ------------------------------------------------------------------------------------------------
 * AnyMDP — reference: anymdp/anymdp_env.py
 * ---------------------------------------------------------------------------------------------- */

/* numpy.random.choice(n, p=row) == searchsorted(cdf, u, side='right') on cdf = cumsum(row)/cumsum(row)[-1]
 * (anymdp_env.py:89,100; pinned by probe).  Clamp mirrors the device, which cannot
 * index past the row; with a valid CDF (last entry 1.0 > u) the clamp is never taken. */
int xo_upper_bound(const double* cdf, int n, double u) {
  int j = 0;
  while (j < n && cdf[j] <= u) ++j;
  return j < n ? j : n - 1;
}

static inline int is_terminal(const xo_anymdp* h, int t, int s) {
  int words = (h->S + 63) / 64;
  return (int)((h->term_mask[(size_t)t * words + (s >> 6)] >> (s & 63)) & 1u);
}

/* reset: anymdp_env.py:81-90.  steps = 0; _state = choice(s_0, p=s_0_prob); returns observation */
static inline void anymdp_reset_one(xo_anymdp* h, int i, double u, int32_t* obs) {
  int t = h->env_task[i];
  int k = xo_upper_bound(h->s0_cdf + (size_t)t * h->s0_max, h->s0_max, u);
  int s = h->s0_ids[(size_t)t * h->s0_max + k];
  h->state[i] = s;
  h->steps[i] = 0;
  h->need_reset[i] = 0;
  if (obs) obs[i] = h->state_map[(size_t)t * h->S + s]; /* get_observation, MDP: :146-148 */
}

void xo_anymdp_reset_injected(xo_anymdp* h, const uint8_t* mask, const double* u, int32_t* obs) {
  for (int i = 0; i < h->n_env; ++i)
    if (!mask || mask[i]) anymdp_reset_one(h, i, u[i], obs);
}

/* step: anymdp_env.py:112-132 with single_step :92-110 inlined. */
static inline void anymdp_step_one(xo_anymdp* h, int i, int a_in, double u, float z, double u_reset,
                                   int32_t* obs, float* reward, float* reward_gt, uint8_t* terminated,
                                   uint8_t* truncated, int32_t* final_obs, int mode, uint32_t* err) {
  const int S = h->S, A = h->A;
  const int t = h->env_task[i];
  int s = h->state[i];
  if (final_obs) final_obs[i] = -1;
  if (mode == 1 /* NEXT_STEP */ && h->need_reset[i]) {
    /* the call after a done ignores the action and returns the reset observation (gymnasium 1.x) */
    anymdp_reset_one(h, i, u_reset, obs);
    reward[i] = 0.0f; reward_gt[i] = 0.0f; terminated[i] = 0; truncated[i] = 0;
    return;
  }
  int a = a_in;
  if (a < 0 || a >= A) { /* reference: assert action < self.na (:97) */
    *err |= 1u;
    a = a < 0 ? 0 : A - 1;
  }
  if (mode == 0 /* DISABLED */ && is_terminal(h, t, s)) {
    /* reference raises "given an terminated state" (:95-96): the env is left untouched */
    *err |= 2u;
    obs[i] = h->state_map[(size_t)t * S + s];
    reward[i] = 0.0f; reward_gt[i] = 0.0f; terminated[i] = 1;
    truncated[i] = (uint8_t)(h->steps[i] >= h->max_steps[t]);
    return;
  }
  int steps = h->steps[i] + 1;                              /* :113 */
  int trunc = steps >= h->max_steps[t];                     /* :114, max_steps = ceil(task max_steps) */
  size_t row = (((size_t)t * S + s) * A + a) * (size_t)S;
  int s2 = xo_upper_bound(h->cdf + row, S, u);              /* :99-100 */
  float r_gt = h->rs[(row + s2) * 2 + 0];                   /* :103 */
  float sg = h->rs[(row + s2) * 2 + 1];                     /* :104 */
  float r = fmaf(sg, z, r_gt);                              /* :105 normal(mu, sigma) = mu + sigma*z */
  int term = is_terminal(h, t, s2);                         /* :107-108 */
  h->state[i] = s2;
  h->steps[i] = steps;
  reward[i] = r; reward_gt[i] = r_gt;
  terminated[i] = (uint8_t)term; truncated[i] = (uint8_t)trunc;
  int o = h->state_map[(size_t)t * S + s2];                 /* :146-148 */
  obs[i] = o;
  if (term || trunc) {
    if (mode == 2 /* SAME_STEP */) {
      if (final_obs) final_obs[i] = o;
      anymdp_reset_one(h, i, u_reset, obs);
    } else if (mode == 1) {
      h->need_reset[i] = 1;
    }
  }
}

void xo_anymdp_step_injected(xo_anymdp* h, const int32_t* action, const double* u, const float* z,
                             const double* u_reset, int32_t* obs, float* reward, float* reward_gt,
                             uint8_t* terminated, uint8_t* truncated, int32_t* final_obs, int mode) {
  for (int i = 0; i < h->n_env; ++i)
    anymdp_step_one(h, i, action[i], u[i], z[i], u_reset[i], obs, reward, reward_gt, terminated,
                    truncated, final_obs, mode, &h->err_flags);
}

static inline uint64_t anymdp_gid(const xo_anymdp* h, uint64_t gid_base, int i) {
  return gid_base + (uint64_t)i * (uint64_t)(h->gid_stride ? h->gid_stride : 1u);
}

void xo_anymdp_reset(xo_anymdp* h, uint64_t seed, uint64_t gid_base, uint64_t tick, const uint8_t* mask,
                     int32_t* obs) {
  for (int i = 0; i < h->n_env; ++i) {
    if (mask && !mask[i]) continue;
    uint32_t w[4];
    xo_env_draw(seed, anymdp_gid(h, gid_base, i), tick, 1, w);
    anymdp_reset_one(h, i, xo_u53(w[0], w[1]), obs);
  }
}

static inline void anymdp_step_free_one(xo_anymdp* h, int i, uint64_t seed, uint64_t gid_base,
                                        uint64_t tick, const int32_t* action, int32_t* obs,
                                        float* reward, float* reward_gt, uint8_t* terminated,
                                        uint8_t* truncated, int32_t* final_obs, int mode, uint32_t* err) {
  uint32_t w[4], v[4];
  xo_env_draw(seed, anymdp_gid(h, gid_base, i), tick, 0, w);
  xo_env_draw(seed, anymdp_gid(h, gid_base, i), tick, 1, v);
  float z;
  xo_box_muller(w[2], w[3], &z, 0);
  anymdp_step_one(h, i, action[i], xo_u53(w[0], w[1]), z, xo_u53(v[0], v[1]), obs, reward, reward_gt,
                  terminated, truncated, final_obs, mode, err);
}

void xo_anymdp_step(xo_anymdp* h, uint64_t seed, uint64_t gid_base, uint64_t tick, const int32_t* action,
                    int32_t* obs, float* reward, float* reward_gt, uint8_t* terminated,
                    uint8_t* truncated, int32_t* final_obs, int mode) {
  for (int i = 0; i < h->n_env; ++i)
    anymdp_step_free_one(h, i, seed, gid_base, tick, action, obs, reward, reward_gt, terminated,
                         truncated, final_obs, mode, &h->err_flags);
}

void xo_anymdp_step_mt(xo_anymdp* h, uint64_t seed, uint64_t gid_base, uint64_t tick,
                       const int32_t* action, int32_t* obs, float* reward, float* reward_gt,
                       uint8_t* terminated, uint8_t* truncated, int32_t* final_obs, int mode,
                       int n_threads) {
  uint32_t err_all = 0;
  (void)n_threads;
#ifdef _OPENMP
#pragma omp parallel for num_threads(n_threads) schedule(static) reduction(| : err_all)
#endif
  for (int i = 0; i < h->n_env; ++i) {
    uint32_t err = 0;
    anymdp_step_free_one(h, i, seed, gid_base, tick, action, obs, reward, reward_gt, terminated,
                         truncated, final_obs, mode, &err);
    err_all |= err;
  }
  h->err_flags |= err_all;
}

/* info["transition_gt"] = transition_obs[self.state, action] (anymdp_env.py:130; transition_obs built by
 * map_transition_reward :12-20): the pmf row of the CURRENT inner state scattered to observation ids. */
void xo_anymdp_transition_gt(const xo_anymdp* h, const int32_t* action, double* out) {
  const int S = h->S, A = h->A;
  for (int i = 0; i < h->n_env; ++i) {
    int t = h->env_task[i], s = h->state[i], a = action[i];
    if (a < 0) a = 0;
    if (a >= A) a = A - 1;
    const double* c = h->cdf + (((size_t)t * S + s) * A + a) * (size_t)S;
    double* o = out + (size_t)i * S;
    for (int j = 0; j < S; ++j) o[j] = 0.0;
    if (is_terminal(h, t, s)) continue; /* all-zero row in the reference */
    for (int j = 0; j < S; ++j)
      o[h->state_map[(size_t)t * S + j]] = c[j] - (j ? c[j - 1] : 0.0);
  }
}

/* ------------------------------------------------------------------------------------------------
 * Synthetic AnyMDP tasks (bench configs 2a/2b).  Integer-only construction so that the
 * device generator (anymdp_synth.hip) is bit-identical: every weight is an integer, every partial sum is
 * exact in uint32, and each CDF entry is one IEEE division.
 * Shape follows the reference sampler's banded transition rows (anymdp/task_sampler_utils.py:65-175):
 * support of row (s,a) is a band [lo,hi) around s; ~15 % of states terminal; s_0 = {0,1,2}.
 * ---------------------------------------------------------------------------------------------- */
static inline void synth_draw(uint64_t seed, uint64_t task, uint32_t c2, uint32_t c3, uint32_t out[4]) {
  uint32_t ctr[4] = {(uint32_t)task, (uint32_t)(task >> 32), c2, c3};
  uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  xo_philox4x32_10(ctr, key, out);
}

void xo_anymdp_synth(uint64_t seed, int64_t task_index_base, int n_task, int S, int A, int s0_max,
                     double* cdf, float* rs, int32_t* state_map, uint64_t* term_mask, double* s0_cdf,
                     int32_t* s0_ids, int32_t* max_steps) {
  xo_anymdp_synth_strided(seed, task_index_base, 1, n_task, S, A, s0_max, cdf, rs, state_map, term_mask, s0_cdf, s0_ids,
                          max_steps);
}

void xo_anymdp_synth_strided(uint64_t seed, int64_t task_index_base, int64_t task_stride, int n_task, int S, int A,
                             int s0_max, double* cdf, float* rs, int32_t* state_map, uint64_t* term_mask, double* s0_cdf,
                             int32_t* s0_ids, int32_t* max_steps) {
  const int words = (S + 63) / 64;
  /* tasks are independent (every draw is keyed by the task index): large batches are built by all host threads */
#pragma omp parallel for schedule(static) if (n_task >= 256)
  for (int tl = 0; tl < n_task; ++tl) {
    const uint64_t task = (uint64_t)(task_index_base + (int64_t)tl * task_stride);
    uint32_t w[4];
    /* header */
    synth_draw(seed, task, 0xFFFFFFFFu, 0, w);
    max_steps[tl] = 256 + (int32_t)(w[0] % 245u);
    int s0_len = 3;
    if (s0_len > s0_max) s0_len = s0_max;
    if (s0_len > S) s0_len = S;
    uint32_t cum = 0, tot = 0;
    for (int k = 0; k < s0_len; ++k) tot += 1u + (w[1 + k] >> 8);
    for (int k = 0; k < s0_max; ++k) {
      if (k < s0_len) {
        cum += 1u + (w[1 + k] >> 8);
        s0_cdf[(size_t)tl * s0_max + k] = (double)cum / (double)tot;
        s0_ids[(size_t)tl * s0_max + k] = k;
      } else {
        s0_cdf[(size_t)tl * s0_max + k] = 1.0;
        s0_ids[(size_t)tl * s0_max + k] = s0_len - 1;
      }
    }
    /* state_map: Fisher-Yates permutation */
    int32_t* sm = state_map + (size_t)tl * S;
    for (int i = 0; i < S; ++i) sm[i] = i;
    for (int i = S - 1; i >= 1; --i) {
      synth_draw(seed, task, 0xFFFFFFFFu, 0x100u + (uint32_t)(i >> 2), w);
      int j = (int)(w[i & 3] % (uint32_t)(i + 1));
      int32_t tmp = sm[i]; sm[i] = sm[j]; sm[j] = tmp;
    }
    /* terminal states: floor(0.15 S) of the states 3..S-1 */
    uint64_t* tm = term_mask + (size_t)tl * words;
    for (int k = 0; k < words; ++k) tm[k] = 0;
    int n_c = S - 3, n_term = (15 * S) / 100;
    if (n_c < 0) n_c = 0;
    if (n_term > n_c) n_term = n_c;
    int cand[512];
    for (int k = 0; k < n_c; ++k) cand[k] = 3 + k;
    for (int k = 0; k < n_term; ++k) {
      synth_draw(seed, task, 0xFFFFFFFFu, 0x200u + (uint32_t)(k >> 2), w);
      int j = k + (int)(w[k & 3] % (uint32_t)(n_c - k));
      int tmp = cand[k]; cand[k] = cand[j]; cand[j] = tmp;
      tm[cand[k] >> 6] |= (uint64_t)1 << (cand[k] & 63);
    }
    /* rows */
    for (int s = 0; s < S; ++s) {
      int term = (int)((tm[s >> 6] >> (s & 63)) & 1u);
      for (int a = 0; a < A; ++a) {
        const uint32_t rowid = (uint32_t)(s * A + a);
        size_t row = (((size_t)tl * S + s) * A + a) * (size_t)S;
        synth_draw(seed, task, rowid, 0x1000u, w);
        int lo_min = s - 33 > 0 ? s - 33 : 0;
        int lo = lo_min + (int)(w[0] % (uint32_t)(s - lo_min + 1));
        int hi_min = s + 2 < S ? s + 2 : S;
        int hi_max = s + 17 < S ? s + 17 : S;
        int hi = hi_min + (int)(w[1] % (uint32_t)(hi_max - hi_min + 1));
        uint32_t wt[512];
        uint32_t total = 0;
        for (int j = 0; j < S; ++j) {
          if ((j & 3) == 0) synth_draw(seed, task, rowid, (uint32_t)(j >> 2), w);
          wt[j] = (j >= lo && j < hi) ? 104858u + (w[j & 3] >> 12) % 943718u : 0u;
          total += wt[j];
        }
        uint32_t c = 0;
        for (int j = 0; j < S; ++j) {
          c += wt[j];
          cdf[row + j] = term ? 1.0 : (double)c / (double)total;
        }
        for (int j = 0; j < S; ++j) {
          if ((j & 1) == 0) synth_draw(seed, task, rowid, 0x100u + (uint32_t)(j >> 1), w);
          uint32_t wa = w[(j & 1) * 2], wb = w[(j & 1) * 2 + 1];
          rs[(row + j) * 2 + 0] = (float)((int32_t)(wa >> 8) - 8388608) * (1.0f / 4194304.0f);
          rs[(row + j) * 2 + 1] = (wb & 1u) ? (float)(wb >> 8) * (1.0f / 67108864.0f) : 0.0f;
        }
      }
    }
  }
}

/* ------------------------------------------------------------------------------------------------
 * LinDS — reference: linds/linds_env.py (dynamics :78-80, get_observation :83-91, get_inner_cmd :93-98,
 * reset :108-131, step :133-169) and utils/random_nn.py:346-368 (RandomFourier.__call__).
 *
 * The reference computes in fp64; the device computes in fp32 (north_star: float dynamics within 1e-5 rel)
 * with every product-sum spelled as an fmaf chain in a FIXED order, restated here operation for operation so
 * that device-vs-oracle is bit-exact on the state/observation path:
 *   x'_j = fmaf chain over k in xo_linds_yorder() of Phi[j][k]*x[k], continued over k = 0..NA-1 of Gamma[j][k]*act[k],
 *          then + Xt[j], then fmaf(noise_scale, z_j, .)
 *   y_j  = fmaf chain over k in xo_linds_yorder() of C[j][k]*x'[k], then + Y[j]
 * (both products visit the state components in the order in which the device's matrix instructions find them in its
 *  accumulator registers, so that a state never has to be re-arranged between steps: see xo_linds_yorder)
 * ---------------------------------------------------------------------------------------------- */
int xo_linds_yorder(int NS, int* ord) {
  /* the device forms y = C x' with 16x16x4 matrix instructions fed straight from the accumulators of x': M-tile m,
   * register r of lane group g holds row 16 m + 4 g + r, and slab s = 4 m + r adds its four k's in g order */
  int n = 0;
  for (int s = 0; s < 8; ++s)
    for (int g = 0; g < 4; ++g) {
      int k = 16 * (s >> 2) + 4 * g + (s & 3);
      if (k < NS) ord[n++] = k;
    }
  return n;
}

static inline const float* L_scal(const xo_linds* h, int t) { return h->scal + (size_t)t * 8; }
static inline const int32_t* L_ints(const xo_linds* h, int t) { return h->ints + (size_t)t * 4; }

void xo_linds_cmd(const xo_linds* h, int t, int tt, float* out) {
  const int NO = h->NO;
  const int nf = L_ints(h, t)[3];
  const float* valid = h->valid + (size_t)t * NO;
  if (nf == 0) { /* static target: command * target_valid (:95-96) */
    for (int j = 0; j < NO; ++j) out[j] = h->cmd0[(size_t)t * NO + j] * valid[j];
    return;
  }
  for (int j = 0; j < NO; ++j) out[j] = 0.0f;
  for (int k = 0; k < nf; ++k) { /* random_nn.py:362-368: x = t/max_steps; y += c0*sin(order*x) + c1*cos(order*x) */
    double ang = h->four_omega[(size_t)t * XO_LINDS_KMAX + k] * ((double)tt / h->four_period[t]);
    ang -= 6.283185307179586476925286766559 * rint(ang * 0.15915494309189533576888376337251);
    float sn = (float)sin(ang), cs = (float)cos(ang);
    const float* c = h->four_coef + (((size_t)t * XO_LINDS_KMAX + k) * NO) * 2;
    for (int j = 0; j < NO; ++j) {
      out[j] = fmaf(c[2 * j], sn, out[j]);
      out[j] = fmaf(c[2 * j + 1], cs, out[j]);
    }
  }
  for (int j = 0; j < NO; ++j) out[j] *= valid[j]; /* :98 */
}

static inline void linds_observe(const xo_linds* h, int t, const float* xs, float* y) {
  int ord[32];
  const int n = xo_linds_yorder(h->NS, ord);
  for (int j = 0; j < h->NO; ++j) {
    float acc = 0.0f;
    for (int p = 0; p < n; ++p)
      acc = fmaf(h->cT[((size_t)t * h->NS + ord[p]) * h->NO + j], xs[ord[p]], acc);
    y[j] = acc + h->y0[(size_t)t * h->NO + j]; /* :85 */
  }
}

/* The sums over the observation rows run as four fmaf chains — chain g over the rows j = 16 mo + 4 g + r (mo, r
 * ascending), the rows one lane group of the device's matrix kernel holds — combined as (p0 + p1) + (p2 + p3)
 * (csrc/linds.hip: linds_err / linds_sumsq / linds_quad_sum). */
static inline float linds_err(const xo_linds* h, int t, const float* y, const float* cmd) {
  /* error = || (obs[:no] - cmd) * target_valid ||  (:127, :153) */
  float p[4];
  for (int g = 0; g < 4; ++g) {
    float acc = 0.0f;
    for (int mo = 0; mo < h->NO / 16; ++mo)
      for (int r = 0; r < 4; ++r) {
        const int j = 16 * mo + 4 * g + r;
        float d = (y[j] - cmd[j]) * h->valid[(size_t)t * h->NO + j];
        acc = fmaf(d, d, acc);
      }
    p[g] = acc;
  }
  return sqrtf((p[0] + p[1]) + (p[2] + p[3]));
}
static inline float linds_sumsq(const xo_linds* h, const float* y) {
  float p[4];
  for (int g = 0; g < 4; ++g) {
    float acc = 0.0f;
    for (int mo = 0; mo < h->NO / 16; ++mo)
      for (int r = 0; r < 4; ++r) acc = fmaf(y[16 * mo + 4 * g + r], y[16 * mo + 4 * g + r], acc);
    p[g] = acc;
  }
  return (p[0] + p[1]) + (p[2] + p[3]);
}

static void linds_reset_one(xo_linds* h, int i, int idx, float* obs, float* cmd, float* error) {
  const int t = h->env_task[i], NS = h->NS, NO = h->NO;
  const int n_init = L_ints(h, t)[2];
  if (idx < 0) idx = 0;
  if (idx >= n_init) idx = n_init - 1;
  float xs[32];
  for (int k = 0; k < NS; ++k) { /* :117 */
    xs[k] = h->init[((size_t)t * h->NI + idx) * NS + k];
    h->x[(size_t)k * h->n_env + i] = xs[k];
  }
  h->steps[i] = 0;
  h->need_reset[i] = 0;
  float y[32], c[32];
  linds_observe(h, t, xs, y);
  xo_linds_cmd(h, t, 0, c); /* :120-126: the last pre-filled command is cmd(0) */
  if (obs) for (int j = 0; j < NO; ++j) obs[(size_t)i * NO + j] = y[j];
  if (cmd) for (int j = 0; j < NO; ++j) cmd[(size_t)i * NO + j] = c[j];
  if (error) error[i] = linds_err(h, t, y, c);
}

void xo_linds_reset_injected(xo_linds* h, const uint8_t* mask, const int32_t* init_index, float* obs,
                             float* cmd, float* error) {
  for (int i = 0; i < h->n_env; ++i)
    if (!mask || mask[i]) linds_reset_one(h, i, init_index[i], obs, cmd, error);
}

static void linds_step_one(xo_linds* h, int i, const float* a_raw, const float* z /*[NS] for this env*/,
                           int init_idx, float* obs, float* reward, uint8_t* terminated,
                           uint8_t* truncated, float* cmd, float* error, float* final_obs, int mode) {
  const int t = h->env_task[i], NS = h->NS, NA = h->NA, NO = h->NO, N = h->n_env;
  const float* sc = L_scal(h, t);
  const int32_t* in = L_ints(h, t);
  /* final_obs: rows of envs that finish in this call only (the device leaves the other rows untouched) */
  if (mode == 1 && h->need_reset[i]) { /* NEXT_STEP: the call after a done returns the reset observation */
    linds_reset_one(h, i, init_idx, obs, cmd, error);
    reward[i] = 0.0f; terminated[i] = 0; truncated[i] = 0;
    return;
  }
  float xs[32], xn[32], act[32], y[32], ctrack[32], crep[32];
  for (int k = 0; k < NS; ++k) xs[k] = h->x[(size_t)k * N + i];
  float sa; /* :164 cost on the RAW padded action, summed like the row sums: chain g over k = g, 4 + g, .. */
  {
    float p[4];
    for (int g = 0; g < 4; ++g) {
      float acc = 0.0f;
      for (int kk = 0; kk < NA / 4; ++kk) acc = fmaf(a_raw[4 * kk + g], a_raw[4 * kk + g], acc);
      p[g] = acc;
    }
    sa = (p[0] + p[1]) + (p[2] + p[3]);
  }
  for (int k = 0; k < NA; ++k) { /* :138 clip */
    float a = a_raw[k];
    act[k] = a < -1.0f ? -1.0f : (a > 1.0f ? 1.0f : a);
  }
  int kord[32];
  const int n_ord = xo_linds_yorder(NS, kord);
  for (int j = 0; j < NS; ++j) { /* :78-80 */
    float acc = 0.0f;
    for (int p = 0; p < n_ord; ++p) acc = fmaf(h->phiT[((size_t)t * NS + kord[p]) * NS + j], xs[kord[p]], acc);
    for (int k = 0; k < NA; ++k) acc = fmaf(h->gamT[((size_t)t * NA + k) * NS + j], act[k], acc);
    acc = acc + h->xt[(size_t)t * NS + j];
    xn[j] = fmaf(sc[4], z[j], acc);
  }
  linds_observe(h, t, xn, y); /* :145 */
  const int steps = h->steps[i] + 1; /* :147 */
  xo_linds_cmd(h, t, steps - 1 - in[1], ctrack); /* :150-151: tracked command is cmd(steps-1-delay) */
  xo_linds_cmd(h, t, steps, crep);               /* :168: reported command is cmd(steps) */
  const float err = linds_err(h, t, y, ctrack);  /* :153 */
  const float obs_scale = sqrtf(linds_sumsq(h, y)); /* :154 */
  const int term = (err > 10.0f) || (obs_scale > 20.0f); /* :156 */
  float r = term ? -sc[2] : 0.0f; /* :158-161 */
  float tmp = fmaf(-sc[3], err, sc[1]);
  tmp = fmaf(-sc[0], sa, tmp);
  r = fmaf(tmp, sc[5], r); /* :163-164 */
  const int trunc = steps >= in[0] - 1; /* :165 */
  for (int k = 0; k < NS; ++k) h->x[(size_t)k * N + i] = xn[k];
  h->steps[i] = steps;
  for (int j = 0; j < NO; ++j) { obs[(size_t)i * NO + j] = y[j]; cmd[(size_t)i * NO + j] = crep[j]; }
  reward[i] = r; error[i] = err; terminated[i] = (uint8_t)term; truncated[i] = (uint8_t)trunc;
  int bad = 0;
  for (int k = 0; k < NS; ++k) if (!isfinite(xn[k])) bad = 1;
  if (bad) h->err_flags |= 4u;
  if (term || trunc) {
    if (mode == 2) {
      if (final_obs) for (int j = 0; j < NO; ++j) final_obs[(size_t)i * NO + j] = y[j];
      linds_reset_one(h, i, init_idx, obs, cmd, error);
    } else if (mode == 1) {
      h->need_reset[i] = 1;
    }
  }
}

void xo_linds_step_injected(xo_linds* h, const float* action, const float* z, const int32_t* init_index,
                            float* obs, float* reward, uint8_t* terminated, uint8_t* truncated, float* cmd,
                            float* error, float* final_obs, int mode) {
  float zz[32];
  for (int i = 0; i < h->n_env; ++i) {
    for (int k = 0; k < h->NS; ++k) zz[k] = z[(size_t)k * h->n_env + i];
    linds_step_one(h, i, action + (size_t)i * h->NA, zz, init_index[i], obs, reward, terminated, truncated,
                   cmd, error, final_obs, mode);
  }
}

/* free-running draws (csrc/linds.hip: linds_init_from_word, linds_noise_group): reset index = floor(w0 * n_init / 2^32)
 * with w0 the first word of purpose 1; the normal of state component j is normal i = 4 (j >> 4) + (j & 3) of Philox
 * purpose 16 + ((j >> 2) & 3), whose word p yields normals 2p (cos) and 2p + 1 (sin) */
static inline int linds_draw_init(const xo_linds* h, int i, uint64_t seed, uint64_t gid, uint64_t tick) {
  uint32_t w[4];
  xo_env_draw(seed, gid, tick, 1, w);
  int n = L_ints(h, h->env_task[i])[2];
  int idx = (int)(((uint64_t)w[0] * (uint64_t)(uint32_t)n) >> 32);
  return idx < n ? idx : n - 1;
}
/* the initial state of an env that finishes inside a STEP call comes from that step's restart word: the xor of the four
 * words of its noise call of lane group 0 (csrc/linds.hip: linds_noise_group) — no Philox call of its own */
static inline int linds_step_restart_index(const xo_linds* h, int i, uint64_t seed, uint64_t gid, uint64_t tick) {
  uint32_t w[4];
  xo_env_draw(seed, gid, tick, 16u, w);
  int n = L_ints(h, h->env_task[i])[2];
  int idx = (int)(((uint64_t)((w[0] ^ w[1]) ^ (w[2] ^ w[3])) * (uint64_t)(uint32_t)n) >> 32);
  return idx < n ? idx : n - 1;
}
static inline void linds_draw_noise(int NS, uint64_t seed, uint64_t gid, uint64_t tick, float* z) {
  for (int g = 0; g < 4; ++g) {
    uint32_t w[4];
    float v[8];
    xo_env_draw(seed, gid, tick, 16u + (uint32_t)g, w);
    for (int p = 0; p < 4; ++p) xo_box_muller16(w[p], &v[2 * p], &v[2 * p + 1]);
    for (int i = 0; i < 8; ++i) {
      const int j = 16 * (i >> 2) + 4 * g + (i & 3);
      if (j < NS) z[j] = v[i];
    }
  }
}

void xo_linds_reset(xo_linds* h, uint64_t seed, uint64_t gid_base, uint64_t tick, const uint8_t* mask,
                    float* obs, float* cmd, float* error) {
  for (int i = 0; i < h->n_env; ++i) {
    if (mask && !mask[i]) continue;
    linds_reset_one(h, i, linds_draw_init(h, i, seed, gid_base + (uint64_t)i, tick), obs, cmd, error);
  }
}

void xo_linds_step(xo_linds* h, uint64_t seed, uint64_t gid_base, uint64_t tick, const float* action,
                   float* obs, float* reward, uint8_t* terminated, uint8_t* truncated, float* cmd,
                   float* error, float* final_obs, int mode, int n_threads) {
  (void)n_threads;
#ifdef _OPENMP
#pragma omp parallel for num_threads(n_threads > 0 ? n_threads : 1) schedule(static)
#endif
  for (int i = 0; i < h->n_env; ++i) {
    float zz[32];
    const uint64_t gid = gid_base + (uint64_t)i;
    linds_draw_noise(h->NS, seed, gid, tick, zz);
    const int idx = linds_step_restart_index(h, i, seed, gid, tick);
    linds_step_one(h, i, action + (size_t)i * h->NA, zz, idx, obs, reward, terminated, truncated, cmd,
                   error, final_obs, mode);
  }
}

/* ------------------------------------------------------------------------------------------------
 * CartPole — metacontrol/random_cartpole.py :46-75 over gymnasium CartPoleEnv.step (Euler integrator,
 * force_mag 10, tau 0.02, x_threshold 2.4, theta_threshold 12 deg).  PARITY UNPINNED (gymnasium absent).
 * ---------------------------------------------------------------------------------------------- */
static void cartpole_reset_one(xo_cartpole* h, int i, const double u[4], float* obs) {
  /* state = uniform(-1, 1, 4) * reset_bounds_scale (random_cartpole.py:70): a float64 array; the observation is its
   * float32 cast (:75) */
  for (int k = 0; k < 4; ++k) {
    double v = fma(2.0, u[k], -1.0) * h->reset_scale[k];
    h->state[(size_t)k * h->n_env + i] = v;
    if (obs) obs[(size_t)i * 4 + k] = (float)v;
  }
  h->steps[i] = 0;
  h->need_reset[i] = 0;
}

/* gymnasium CartPoleEnv.step keeps `self.state` and all of its arithmetic in float64 (Python floats / numpy float64)
 * and casts only the returned observation to float32; so does this restatement. */
static void cartpole_step_one(xo_cartpole* h, int i, int action, const double u_reset[4], float* obs,
                              float* reward, uint8_t* terminated, uint8_t* truncated, float* final_obs, int mode) {
  const int N = h->n_env, t = h->env_task[i];
  if (final_obs) for (int k = 0; k < 4; ++k) final_obs[(size_t)i * 4 + k] = 0.0f;
  if (mode == 1 && h->need_reset[i]) {
    cartpole_reset_one(h, i, u_reset, obs);
    reward[i] = 0.0f; terminated[i] = 0; truncated[i] = 0;
    return;
  }
  if (action != 0 && action != 1) { h->err_flags |= 1u; action = action > 0 ? 1 : 0; }
  const double gravity = h->params[t * 4 + 0], masscart = h->params[t * 4 + 1], masspole = h->params[t * 4 + 2],
               length = h->params[t * 4 + 3];
  const double polemass_length = masspole * length;  /* :49 */
  const double total_mass = masspole + masscart;     /* :50 */
  double x = h->state[i], xd = h->state[(size_t)N + i], th = h->state[(size_t)2 * N + i], thd = h->state[(size_t)3 * N + i];
  const double force = action == 1 ? 10.0 : -10.0;
  const double theta_threshold = 12 * 2 * 3.141592653589793 / 360, x_threshold = 2.4, tau = 0.02;
  float total_reward = 0.0f;
  int term = 0;
  for (int f = 0; f < h->frameskip; ++f) { /* :56-60 */
    const double cs = cos(th), sn = sin(th);
    const double temp = (force + polemass_length * (thd * thd) * sn) / total_mass;
    const double thacc = (gravity * sn - cs * temp) / (length * (4.0 / 3.0 - masspole * (cs * cs) / total_mass));
    const double xacc = temp - polemass_length * thacc * cs / total_mass;
    x = x + tau * xd;
    xd = xd + tau * xacc;
    th = th + tau * thd;
    thd = thd + tau * thacc;
    term = (x < -x_threshold) || (x > x_threshold) || (th < -theta_threshold) || (th > theta_threshold);
    total_reward += 1.0f;
    if (term) break;
  }
  const int steps = h->steps[i] + 1;
  const int trunc = h->max_steps > 0 && steps >= h->max_steps;
  h->state[i] = x; h->state[(size_t)N + i] = xd; h->state[(size_t)2 * N + i] = th; h->state[(size_t)3 * N + i] = thd;
  h->steps[i] = steps;
  obs[(size_t)i * 4 + 0] = (float)x; obs[(size_t)i * 4 + 1] = (float)xd; obs[(size_t)i * 4 + 2] = (float)th;
  obs[(size_t)i * 4 + 3] = (float)thd;
  reward[i] = total_reward; terminated[i] = (uint8_t)term; truncated[i] = (uint8_t)trunc;
  if (term || trunc) {
    if (mode == 2) {
      if (final_obs) for (int k = 0; k < 4; ++k) final_obs[(size_t)i * 4 + k] = obs[(size_t)i * 4 + k];
      cartpole_reset_one(h, i, u_reset, obs);
    } else if (mode == 1) {
      h->need_reset[i] = 1;
    }
  }
}

void xo_cartpole_reset_injected(xo_cartpole* h, const uint8_t* mask, const double* u, float* obs) {
  for (int i = 0; i < h->n_env; ++i) {
    if (mask && !mask[i]) continue;
    double uu[4];
    for (int k = 0; k < 4; ++k) uu[k] = u[(size_t)k * h->n_env + i];
    cartpole_reset_one(h, i, uu, obs);
  }
}

void xo_cartpole_step_injected(xo_cartpole* h, const int32_t* action, const double* u_reset, float* obs,
                               float* reward, uint8_t* terminated, uint8_t* truncated, float* final_obs, int mode) {
  for (int i = 0; i < h->n_env; ++i) {
    double uu[4];
    for (int k = 0; k < 4; ++k) uu[k] = u_reset[(size_t)k * h->n_env + i];
    cartpole_step_one(h, i, action[i], uu, obs, reward, terminated, truncated, final_obs, mode);
  }
}

static inline void cartpole_draw(uint64_t seed, uint64_t gid, uint64_t tick, double u[4]) {
  uint32_t w[4];
  xo_env_draw(seed, gid, tick, 1, w);
  for (int k = 0; k < 4; ++k) u[k] = (double)w[k] * (1.0 / 4294967296.0);
}

void xo_cartpole_reset(xo_cartpole* h, uint64_t seed, uint64_t gid_base, uint64_t tick, const uint8_t* mask, float* obs) {
  for (int i = 0; i < h->n_env; ++i) {
    if (mask && !mask[i]) continue;
    double u[4];
    cartpole_draw(seed, gid_base + (uint64_t)i, tick, u);
    cartpole_reset_one(h, i, u, obs);
  }
}

void xo_cartpole_step(xo_cartpole* h, uint64_t seed, uint64_t gid_base, uint64_t tick, const int32_t* action,
                      float* obs, float* reward, uint8_t* terminated, uint8_t* truncated, float* final_obs, int mode) {
  for (int i = 0; i < h->n_env; ++i) {
    double u[4];
    cartpole_draw(seed, gid_base + (uint64_t)i, tick, u);
    cartpole_step_one(h, i, action[i], u, obs, reward, terminated, truncated, final_obs, mode);
  }
}

/* ------------------------------------------------------------------------------------------------
 * Acrobot — metacontrol/random_acrobot.py over gymnasium AcrobotEnv (dt 0.2, torques {-1,0,+1}, MAX_VEL 4pi/9pi,
 * book dynamics, no torque noise).  Every expression keeps the reference's Python evaluation order.
 * ---------------------------------------------------------------------------------------------- */
#define AC_PI 3.141592653589793 /* numpy.pi */

/* random_acrobot.py:58-96 (book_or_nips == "book", the gymnasium default) */
void xo_acrobot_dsdt(const double prm[7], const double y[5], double out[5]) {
  const double l1 = prm[0], l2 = prm[1], m1 = prm[2], m2 = prm[3], lc1 = prm[4], lc2 = prm[5], g = prm[6];
  const double I1 = m1 * (lc1 * lc1 + (l1 - lc1) * (l1 - lc1)) / 6.0;
  const double I2 = m2 * (lc2 * lc2 + (l2 - lc2) * (l2 - lc2)) / 6.0;
  const double a = y[4], theta1 = y[0], theta2 = y[1], dtheta1 = y[2], dtheta2 = y[3];
  const double c2 = cos(theta2), s2 = sin(theta2);
  const double d1 = m1 * (lc1 * lc1) + m2 * (l1 * l1 + lc2 * lc2 + 2 * l1 * lc2 * c2) + I1 + I2;
  const double d2 = m2 * (lc2 * lc2 + l1 * lc2 * c2) + I2;
  const double phi2 = m2 * lc2 * g * cos(theta1 + theta2 - AC_PI / 2.0);
  const double phi1 = -m2 * l1 * lc2 * (dtheta2 * dtheta2) * s2 - 2 * m2 * l1 * lc2 * dtheta2 * dtheta1 * s2 +
                      (m1 * lc1 + m2 * l1) * g * cos(theta1 - AC_PI / 2) + phi2;
  const double ddtheta2 = (a + d2 / d1 * phi1 - m2 * l1 * lc2 * (dtheta1 * dtheta1) * s2 - phi2) /
                          (m2 * (lc2 * lc2) + I2 - d2 * d2 / d1);
  const double ddtheta1 = -(d2 * ddtheta2 + phi1) / d1;
  out[0] = dtheta1; out[1] = dtheta2; out[2] = ddtheta1; out[3] = ddtheta2; out[4] = 0.0;
}

/* random_acrobot.py:98-101 */
int xo_acrobot_terminal(const double prm[7], const double s[4]) { return -cos(s[0]) - cos(s[1] + s[0]) > prm[0]; }

static double ac_wrap(double x, double m, double M) { /* gymnasium acrobot.wrap */
  const double diff = M - m;
  while (x > M) x = x - diff;
  while (x < m) x = x + diff;
  return x;
}
static double ac_bound(double x, double m, double M) { /* min(max(x, m), M) with Python's comparison semantics */
  const double t = (m > x) ? m : x; /* max(x, m): returns x unless m > x */
  return (M < t) ? M : t;           /* min(t, M): returns t unless M < t */
}

/* one AcrobotEnv.step: rk4 over [0, dt], wrap, bound, terminal */
static int acrobot_substep(const double prm[7], double s[4], double torque) {
  const double dt = 0.2, dt2 = dt / 2.0;
  double y0[5] = {s[0], s[1], s[2], s[3], torque}, k1[5], k2[5], k3[5], k4[5], y[5];
  xo_acrobot_dsdt(prm, y0, k1);
  for (int i = 0; i < 5; ++i) y[i] = y0[i] + dt2 * k1[i];
  xo_acrobot_dsdt(prm, y, k2);
  for (int i = 0; i < 5; ++i) y[i] = y0[i] + dt2 * k2[i];
  xo_acrobot_dsdt(prm, y, k3);
  for (int i = 0; i < 5; ++i) y[i] = y0[i] + dt * k3[i];
  xo_acrobot_dsdt(prm, y, k4);
  double ns[4];
  for (int i = 0; i < 4; ++i) ns[i] = y0[i] + dt / 6.0 * (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]);
  s[0] = ac_wrap(ns[0], -AC_PI, AC_PI);
  s[1] = ac_wrap(ns[1], -AC_PI, AC_PI);
  s[2] = ac_bound(ns[2], -4 * AC_PI, 4 * AC_PI);
  s[3] = ac_bound(ns[3], -9 * AC_PI, 9 * AC_PI);
  return xo_acrobot_terminal(prm, s);
}

static void acrobot_obs(const xo_acrobot* h, int i, float* o) { /* AcrobotEnv._get_ob -> float32[6] */
  const size_t N = (size_t)h->n_env;
  const double s0 = h->state[i], s1 = h->state[N + i], s2 = h->state[2 * N + i], s3 = h->state[3 * N + i];
  if (h->fresh[i] && !h->scale_is_vector) { /* the state is a float32 array: numpy's cos/sin stay in float32 */
    o[0] = cosf((float)s0); o[1] = sinf((float)s0); o[2] = cosf((float)s1); o[3] = sinf((float)s1);
  } else {
    o[0] = (float)cos(s0); o[1] = (float)sin(s0); o[2] = (float)cos(s1); o[3] = (float)sin(s1);
  }
  o[4] = (float)s2; o[5] = (float)s3;
}

static void acrobot_reset_one(xo_acrobot* h, int i, const double u[4], float* obs) {
  /* state = uniform(-1, 1, 4).astype(float32) * reset_bounds_scale   (random_acrobot.py:123-125) */
  const size_t N = (size_t)h->n_env;
  for (int k = 0; k < 4; ++k) {
    const float f = (float)(-1.0 + 2.0 * u[k]);
    h->state[k * N + i] = h->scale_is_vector ? (double)f * h->reset_scale[k] : (double)(f * (float)h->reset_scale[k]);
  }
  h->fresh[i] = 1;
  h->steps[i] = 0;
  h->need_reset[i] = 0;
  if (obs) acrobot_obs(h, i, obs + (size_t)i * 6);
}

static void acrobot_step_one(xo_acrobot* h, int i, int action, const double u_reset[4], float* obs, float* reward,
                             uint8_t* terminated, uint8_t* truncated, float* final_obs, int mode) {
  const size_t N = (size_t)h->n_env;
  const double* prm = h->params + (size_t)h->env_task[i] * 7;
  if (final_obs) for (int k = 0; k < 6; ++k) final_obs[(size_t)i * 6 + k] = 0.0f;
  if (mode == 1 && h->need_reset[i]) {
    acrobot_reset_one(h, i, u_reset, obs);
    reward[i] = 0.0f; terminated[i] = 0; truncated[i] = 0;
    return;
  }
  if (action < 0 || action > 2) { h->err_flags |= 1u; action = action < 0 ? 0 : 2; }
  const double torque = (double)(action - 1); /* AVAIL_TORQUE = [-1.0, 0.0, +1] */
  double s[4] = {h->state[i], h->state[N + i], h->state[2 * N + i], h->state[3 * N + i]};
  double total_reward = 0.0;
  int term = 0;
  for (int f = 0; f < h->frameskip; ++f) { /* :112-116 */
    term = acrobot_substep(prm, s, torque);
    total_reward += term ? 0.0 : -1.0;
    if (term) break;
  }
  for (int k = 0; k < 4; ++k) h->state[k * N + i] = s[k];
  h->fresh[i] = 0;
  const int steps = h->steps[i] + 1;
  const int trunc = h->max_steps > 0 && steps >= h->max_steps;
  h->steps[i] = steps;
  acrobot_obs(h, i, obs + (size_t)i * 6);
  reward[i] = (float)total_reward; terminated[i] = (uint8_t)term; truncated[i] = (uint8_t)trunc;
  if (term || trunc) {
    if (mode == 2) {
      if (final_obs) for (int k = 0; k < 6; ++k) final_obs[(size_t)i * 6 + k] = obs[(size_t)i * 6 + k];
      acrobot_reset_one(h, i, u_reset, obs);
    } else if (mode == 1) {
      h->need_reset[i] = 1;
    }
  }
}

void xo_acrobot_reset_injected(xo_acrobot* h, const uint8_t* mask, const double* u, float* obs) {
  for (int i = 0; i < h->n_env; ++i) {
    if (mask && !mask[i]) continue;
    double uu[4];
    for (int k = 0; k < 4; ++k) uu[k] = u[(size_t)k * h->n_env + i];
    acrobot_reset_one(h, i, uu, obs);
  }
}

void xo_acrobot_step_injected(xo_acrobot* h, const int32_t* action, const double* u_reset, float* obs, float* reward,
                              uint8_t* terminated, uint8_t* truncated, float* final_obs, int mode) {
  for (int i = 0; i < h->n_env; ++i) {
    double uu[4];
    for (int k = 0; k < 4; ++k) uu[k] = u_reset[(size_t)k * h->n_env + i];
    acrobot_step_one(h, i, action[i], uu, obs, reward, terminated, truncated, final_obs, mode);
  }
}

/* reset draws: two Philox calls (purposes 1 and 3), a 53-bit uniform from each word pair */
static inline void acrobot_draw(uint64_t seed, uint64_t gid, uint64_t tick, double u[4]) {
  uint32_t w[4], v[4];
  xo_env_draw(seed, gid, tick, 1, w);
  xo_env_draw(seed, gid, tick, 3, v);
  u[0] = xo_u53(w[0], w[1]); u[1] = xo_u53(w[2], w[3]); u[2] = xo_u53(v[0], v[1]); u[3] = xo_u53(v[2], v[3]);
}

void xo_acrobot_reset(xo_acrobot* h, uint64_t seed, uint64_t gid_base, uint64_t tick, const uint8_t* mask, float* obs) {
  for (int i = 0; i < h->n_env; ++i) {
    if (mask && !mask[i]) continue;
    double u[4];
    acrobot_draw(seed, gid_base + (uint64_t)i, tick, u);
    acrobot_reset_one(h, i, u, obs);
  }
}

void xo_acrobot_step(xo_acrobot* h, uint64_t seed, uint64_t gid_base, uint64_t tick, const int32_t* action, float* obs,
                     float* reward, uint8_t* terminated, uint8_t* truncated, float* final_obs, int mode) {
  for (int i = 0; i < h->n_env; ++i) {
    double u[4];
    acrobot_draw(seed, gid_base + (uint64_t)i, tick, u);
    acrobot_step_one(h, i, action[i], u, obs, reward, terminated, truncated, final_obs, mode);
  }
}

/* ------------------------------------------------------------------------------------------------
 * MazeWorld
 * ---------------------------------------------------------------------------------------------- */
#define MZ_PI 3.1415926      /* dynamics.py:7-8: the reference's own truncated constants */
#define MZ_TPI 6.2831852

static double mz_angle_norm(double t) { /* dynamics.py:48-54 */
  while (t > MZ_PI) t -= MZ_TPI;
  while (t < -MZ_PI) t += MZ_TPI;
  return t;
}

/* dynamics.py:56-69: distance to / nearest point on the segment l1-l2 */
static double mz_nearest_point(const double p[2], const double l1[2], const double l2[2], double np_[2]) {
  double u0 = l2[0] - l1[0], u1 = l2[1] - l1[1];
  const double edge = sqrt(u0 * u0 + u1 * u1);
  const double m = edge > 1.0e-6 ? edge : 1.0e-6;
  u0 /= m; u1 /= m;
  const double d1 = (p[0] - l1[0]) * u0 + (p[1] - l1[1]) * u1;
  if (d1 > edge) { np_[0] = l2[0]; np_[1] = l2[1]; }
  else if (d1 < 0) { np_[0] = l1[0]; np_[1] = l1[1]; }
  else { np_[0] = l1[0] + d1 * u0; np_[1] = l1[1] + d1 * u1; }
  const double a = p[0] - np_[0], b = p[1] - np_[1];
  return sqrt(a * a + b * b);
}

/* dynamics.py:71-96: soft push-out force from the wall cell whose centre is at -dv (cell units) */
static void mz_collision_force(const double dv[2], double cell_size, double col_dist, double f[2]) {
  static const double O10[2] = {0.5, 0.5}, O01[2] = {-0.5, 0.5}, Om0[2] = {-0.5, -0.5}, O0m[2] = {0.5, -0.5};
  const double dist = sqrt(dv[0] * dv[0] + dv[1] * dv[1]);
  const double eff = col_dist / cell_size;
  f[0] = f[1] = 0.0;
  if (dist > 0.708 + eff) return;
  if (fabs(dv[0]) < 0.5 && fabs(dv[1]) < 0.5) { /* centre inside the wall cell: :77-78 */
    const double s = 0.50 / (dist > 1.0e-6 ? dist : 1.0e-6) * (0.708 + eff - dist) * cell_size;
    f[0] = s * dv[0]; f[1] = s * dv[1];
    return;
  }
  const int x_pos = dv[0] + dv[1] > 0, y_pos = dv[1] - dv[0] > 0;
  double np_[2], d;
  if (x_pos && y_pos) d = mz_nearest_point(dv, O10, O01, np_);
  else if (!x_pos && y_pos) d = mz_nearest_point(dv, O01, Om0, np_);
  else if (!x_pos && !y_pos) d = mz_nearest_point(dv, Om0, O0m, np_);
  else d = mz_nearest_point(dv, O0m, O10, np_);
  if (eff < d) return;
  double o0 = dv[0] - np_[0], o1 = dv[1] - np_[1];
  const double on = sqrt(o0 * o0 + o1 * o1);
  const double inv = 1.0 / (on > 1.0e-6 ? on : 1.0e-6);
  o0 *= inv; o1 *= inv;
  const double s = 0.50 * (eff - d) * cell_size;
  f[0] = s * o0; f[1] = s * o1;
}

/* dynamics.py:158-187 with vector_move_no_collision :98-123 inlined: delta_t = 1.0 in 100 sub-steps of 0.01 */
void xo_maze_move(double* ori_io, double pos[2], double turn_rate, double walk_speed, const int8_t* walls, int n,
                  int NG, double cell_size, double col_dist, double* collision) {
  double ori = *ori_io, p0 = pos[0], p1 = pos[1], coll = 0.0;
  const double t_prec = 0.01, delta_t = 1.0;
  const int iteration = (int)(delta_t / t_prec);
  for (int it = 0; it < iteration + 1; ++it) {
    const double rem = delta_t - it * t_prec;
    const double dt = rem < t_prec ? rem : t_prec;
    if (dt < 1.0e-8) continue;
    const double d_theta = turn_rate * dt, arc = walk_speed * dt;
    const double c_t = cos(ori), s_t = sin(ori), c_dt = cos(0.5 * d_theta), s_dt = sin(0.5 * d_theta);
    const double n_ori = mz_angle_norm(ori + d_theta);
    double dx, dy;
    if (fabs(d_theta) < 1.0e-8) { dx = c_t * arc; dy = s_t * arc; }
    else {
      const double rad = walk_speed / turn_rate, off = 2.0 * s_dt * rad;
      const double c_n = c_t * c_dt - s_t * s_dt, s_n = c_t * s_dt + s_t * c_dt;
      dx = c_n * off; dy = s_n * off;
    }
    ori = n_ori;
    const double e0 = p0 + dx, e1 = p1 + dy;
    const double c0 = e0 / cell_size, c1 = e1 / cell_size;
    double f0 = 0.0, f1 = 0.0;
    for (int i = -1; i < 2; ++i)
      for (int j = -1; j < 2; ++j) {
        const int wi = i + (int)c0, wj = j + (int)c1;
        if (wi > -1 && wi < n && wj > -1 && wj < n && walls[wi * NG + wj] > 0) {
          const double dv[2] = {c0 - floor(c0) - (double)(float)(i + 0.5), c1 - floor(c1) - (double)(float)(j + 0.5)};
          double f[2];
          mz_collision_force(dv, cell_size, col_dist, f);
          f0 += f[0]; f1 += f[1];
        }
      }
    p0 = f0 + e0; p1 = f1 + e1;
    coll += sqrt(f0 * f0 + f1 * f1);
  }
  *ori_io = ori; pos[0] = p0; pos[1] = p1;
  if (collision) *collision = coll;
}

void xo_maze_reset(xo_maze* h, const uint8_t* mask) { /* maze_base.py:83-105 */
  for (int e = 0; e < h->n_env; ++e) {
    if (mask && !mask[e]) continue;
    const int t = h->env_task[e];
    const int32_t* in = h->ints + (size_t)t * 8;
    const double cs = h->dbl[(size_t)t * 8];
    h->grid[e] = in[1]; h->grid[(size_t)h->n_env + e] = in[2];
    h->pos[e] = in[1] * cs + 0.5 * cs;                       /* get_cell_center :215-218 */
    h->pos[(size_t)h->n_env + e] = in[2] * cs + 0.5 * cs;
    h->ori[e] = 0.0;
    h->cmd_idx[e] = 0; h->cmd_age[e] = 0; h->steps[e] = 0; h->need_reset[e] = 0;
    h->collision[e] = 0.0;
  }
}

void xo_maze_step(xo_maze* h, const double* action, float* reward, uint8_t* terminated, uint8_t* truncated,
                  int mode) {
  const int N = h->n_env;
  for (int e = 0; e < N; ++e) {
    const int t = h->env_task[e];
    const int32_t* in = h->ints + (size_t)t * 8;
    const double* db = h->dbl + (size_t)t * 8;
    if (mode == 1 && h->need_reset[e]) {
      uint8_t m = 1;
      xo_maze tmp = *h; (void)tmp;
      /* reset this env only */
      const double cs = db[0];
      h->grid[e] = in[1]; h->grid[(size_t)N + e] = in[2];
      h->pos[e] = in[1] * cs + 0.5 * cs; h->pos[(size_t)N + e] = in[2] * cs + 0.5 * cs;
      h->ori[e] = 0.0; h->cmd_idx[e] = 0; h->cmd_age[e] = 0; h->steps[e] = 0; h->need_reset[e] = 0;
      (void)m;
      reward[e] = 0.0f; terminated[e] = 0; truncated[e] = 0;
      continue;
    }
    /* do_action: maze_continuous_3d.py:49-62 */
    double tr = action[2 * e], ws = action[2 * e + 1];
    tr = (tr < -1.0 ? -1.0 : (tr > 1.0 ? 1.0 : tr)) * MZ_PI;
    ws = ws < -1.0 ? -1.0 : (ws > 1.0 ? 1.0 : ws);
    double p[2] = {h->pos[e], h->pos[(size_t)N + e]}, ori = h->ori[e], coll;
    xo_maze_move(&ori, p, tr, ws, h->walls + (size_t)t * h->NG * h->NG, in[0], h->NG, db[0], h->collision_dist, &coll);
    h->pos[e] = p[0]; h->pos[(size_t)N + e] = p[1]; h->ori[e] = ori; h->collision[e] = coll;
    const int g0 = (int)(p[0] / db[0]), g1 = (int)(p[1] / db[0]); /* get_loc_grid :220-223 */
    h->grid[e] = g0; h->grid[(size_t)N + e] = g1;
    /* evaluation_rule: maze_base.py:107-119 */
    const int steps = h->steps[e] + 1;
    int age = h->cmd_age[e] + 1, idx = h->cmd_idx[e];
    const int cmd = h->commands[(size_t)t * h->n_cmd + (idx < h->n_cmd ? idx : h->n_cmd - 1)];
    const int32_t* lc = h->lm_coord + ((size_t)t * XO_MAZE_LMAX + cmd) * 2;
    const int at_goal = (idx < h->n_cmd) && lc[0] == g0 && lc[1] == g1;
    /* instant_rewards is a float32 array holding goal_reward at the active command's cell (:61-69, :96) */
    const float r = (at_goal ? (float)db[5] : 0.0f) + (float)db[4];
    int term = 0;
    if (at_goal || age >= 500) { /* reach_goal() or step_limits() -> refresh_command (:54-70) */
      idx += 1; age = 0;
      if (idx > h->n_cmd - 1) term = 1;
    }
    const int trunc = steps > h->max_steps - 1; /* :212-213 */
    h->steps[e] = steps; h->cmd_age[e] = age; h->cmd_idx[e] = idx;
    reward[e] = r; terminated[e] = (uint8_t)term; truncated[e] = (uint8_t)trunc;
    if (term || trunc) {
      if (mode == 2) {
        const double cs = db[0];
        h->grid[e] = in[1]; h->grid[(size_t)N + e] = in[2];
        h->pos[e] = in[1] * cs + 0.5 * cs; h->pos[(size_t)N + e] = in[2] * cs + 0.5 * cs;
        h->ori[e] = 0.0; h->cmd_idx[e] = 0; h->cmd_age[e] = 0; h->steps[e] = 0;
        h->collision[e] = 0.0; /* as xo_maze_reset does */
      } else if (mode == 1) {
        h->need_reset[e] = 1;
      }
    }
  }
}

/* ray_caster_utils.py:11-25 */
static const float MZ_LANDMARK_RGB[XO_MAZE_LMAX][3] = {
    {0, 255, 0}, {255, 0, 0}, {0, 0, 255}, {0, 255, 255}, {255, 0, 255}, {255, 255, 0}, {128, 128, 255},
    {128, 255, 128}, {255, 128, 128}, {0, 96, 128}, {96, 0, 128}, {0, 128, 96}, {96, 128, 0}, {128, 96, 0},
    {128, 0, 96}};

/* interpolate, ray_caster_utils.py:123-140: 4x4 taps, distance-weighted, wrap-around.  `weak`: the types the source takes
 * as plain Python under NumPy 2, where they follow the VALUES: wht = max(0.01, min(w, 1.0)) is numpy's float64 w inside
 * the ramp but the python float 0.01 (weak, i.e. float32 next to a float32 array) where it clamps (w <= 0.01; w > 1.0
 * does not occur off the texel centres, and the wall stage's integer centre tap has w == 1.0 exactly, which min() keeps).
 * So a ramp tap accumulates float32(float64(sum_r) + wht * tex), a clamped one float32(sum_r + float32(0.01f * tex)),
 * and when all 16 clamp, sum_wht stays a python float and sum_r / sum_wht is a float32 division (a magnified ground or
 * ceiling texture).  weak = 0 (numba's typing): every weight float64, the return value float64. */
static void mz_interpolate(const float* tex /*[256][256][3]*/, double i, double j, double d, double px, double py,
                           double out[3], int weak) {
  double d2 = d * d;
  if (d2 < 1.0e-8) d2 = 1.0e-8;
  const int ib = (int)i, jb = (int)j;
  double sum_wht = 0.0;
  int all_weak = weak;
  float sr[3] = {0.0f, 0.0f, 0.0f};
  for (int x = ib - 1; x < ib + 3; ++x)
    for (int y = jb - 1; y < jb + 3; ++y) {
      const double a = ((double)x - i) * px, b = ((double)y - j) * py;
      const double dist = a * a + b * b;
      double wht = 1.0 - 10 * dist / d2;
      if (wht > 1.0) wht = 1.0;
      const int clamped = wht <= 0.01;
      if (clamped) wht = 0.01;
      sum_wht += wht;
      const int xv = ((x % 256) + 256) % 256, yv = ((y % 256) + 256) % 256;
      const float* tp = tex + ((size_t)xv * 256 + yv) * 3;
      if (weak && clamped) {
        for (int c = 0; c < 3; ++c) {
          const float prod = 0.01f * tp[c];
          sr[c] = sr[c] + prod;
        }
      } else {
        all_weak = 0;
        for (int c = 0; c < 3; ++c) sr[c] = (float)((double)sr[c] + wht * (double)tp[c]);
      }
    }
  if (all_weak) {
    const float sw = (float)sum_wht;
    for (int c = 0; c < 3; ++c) out[c] = (double)(sr[c] / sw);
  } else {
    for (int c = 0; c < 3; ++c) out[c] = (double)sr[c] / sum_wht;
  }
}

static inline int32_t mz_clip_int(double v) { /* numpy.clip(v, 0, 255) stored into an int32 array */
  if (v < 0.0) v = 0.0;
  if (v > 255.0) v = 255.0;
  return (int32_t)v;
}

/* maze_view, ray_caster_utils.py:142-320, for one env.  Typing follows the reference as it executes under
 * NumPy >= 2 scalar promotion (python floats are weak): per-column tables are float32, DDA_2D runs entirely
 * in float32 (its python-float operands are weak), floor/ceiling/texture math is float64. */
static void mz_view(const xo_maze* h, int e, int32_t* rgb /*[W][H][3]*/, int typing_f64) {
  const int t = h->env_task[e], W = h->W, H = h->H, NG = h->NG, N = h->n_env;
  const int32_t* in = h->ints + (size_t)t * 8;
  const double* db = h->dbl + (size_t)t * 8;
  const int n = in[0];
  const double cell_size = db[0], ceil_height = db[1], vision_height = db[2], fol = db[3];
  const double visibility = h->visibility, l_focal = 0.20, text_size = 1.0;
  const int8_t* walls = h->walls + (size_t)t * NG * NG;
  const int8_t* transp = h->landmarks + (size_t)t * NG * NG;
  const int32_t* texts = h->texts + (size_t)t * NG * NG;
  const float* ground = h->tex_grounds + (size_t)in[3] * 256 * 256 * 3;
  const float* ceil_t = h->tex_ceilings + (size_t)in[4] * 256 * 256 * 3;
  const float pos[2] = {(float)h->pos[e], (float)h->pos[(size_t)N + e]}; /* maze_continuous_3d.py:97 */
  const double ori = h->ori[e];

  const double half_h = tan(fol / 2) * l_focal;
  const double half_v = half_h * H / W;
  const double pixel_size = 2.0 * half_h / W;
  const double s_ori = sin(ori), c_ori = cos(ori);
  const double pixel_factor = pixel_size / l_focal;
  const double percell = cell_size / text_size;
  const double tps = text_size / 256;

  for (int k = 0; k < W * H * 3; ++k) rgb[k] = 1; /* FAR_RGB */
  float cos_hp_a[1024], cos_abs[1024], sin_abs[1024];
  double tan_hp = (-0.5 - W / 2.0) * pixel_factor;
  for (int d_h = 0; d_h < W; ++d_h) { /* :170-177 */
    tan_hp += pixel_factor;
    const double cos_hp = sqrt(1.0 / (1.0 + tan_hp * tan_hp));
    const double sin_hp = tan_hp * cos_hp;
    sin_abs[d_h] = (float)(sin_hp * c_ori + cos_hp * s_ori);
    cos_abs[d_h] = (float)(cos_hp * c_ori - sin_hp * s_ori);
    cos_hp_a[d_h] = (float)cos_hp;
  }
  double eff_distance = 0.0; /* survives into the wall loop (quirk i) */

  for (int d_v = H - 1; d_v > H / 2; --d_v) { /* floor :180-211 */
    const double v_screen = (d_v + 0.5) * pixel_size - half_v;
    const double distance = vision_height / v_screen * l_focal;
    double light = v_screen / l_focal;
    if (light > 1.0) light = 1.0;
    if (distance > visibility) continue;
    for (int d_h = 0; d_h < W; ++d_h) {
      eff_distance = distance / (double)cos_hp_a[d_h];
      double alpha = 2.0 * eff_distance / visibility - 1.0;
      if (alpha < 0.0) alpha = 0.0;
      if (alpha > 1.0) alpha = 1.0;
      alpha *= light;
      const double hit_x = eff_distance * (double)cos_abs[d_h] + (double)pos[0];
      const double hit_y = eff_distance * (double)sin_abs[d_h] + (double)pos[1];
      double fi = hit_x / cell_size, fj = hit_y / cell_size;
      double d_i = fi - floor(fi), d_j = fj - floor(fj);
      const int i = (int)fi, j = (int)fj;
      const double eff_ps = eff_distance * pixel_size / l_focal;
      if (i < n && i >= 0 && j < n && j >= 0) {
        d_i *= percell; d_j *= percell;
        d_i -= floor(d_i); d_j -= floor(d_j);
        d_i *= 256; d_j *= 256;
        double col[3];
        mz_interpolate(ground, d_i, d_j, eff_ps, tps, tps, col, !typing_f64);
        int32_t* px = rgb + ((size_t)d_h * H + d_v) * 3;
        for (int c = 0; c < 3; ++c) px[c] = mz_clip_int(light * (alpha * 1.0 + (1.0 - alpha) * col[c]));
      }
    }
  }
  for (int d_v = 0; d_v < H / 2; ++d_v) { /* ceiling :214-244 */
    const double v_screen = half_v - (d_v + 0.5) * pixel_size;
    const double distance = (ceil_height - vision_height) / v_screen * l_focal;
    double light = v_screen / l_focal;
    if (light > 1.0) light = 1.0;
    if (distance > visibility) continue;
    for (int d_h = 0; d_h < W; ++d_h) {
      eff_distance = distance / (double)cos_hp_a[d_h];
      double alpha = 2.0 * eff_distance / visibility - 1.0;
      if (alpha < 0.0) alpha = 0.0;
      if (alpha > 1.0) alpha = 1.0;
      const double hit_x = eff_distance * (double)cos_abs[d_h] + (double)pos[0];
      const double hit_y = eff_distance * (double)sin_abs[d_h] + (double)pos[1];
      double fi = hit_x / cell_size, fj = hit_y / cell_size;
      double d_i = fi - floor(fi), d_j = fj - floor(fj);
      const int i = (int)fi, j = (int)fj;
      const double eff_ps = eff_distance * pixel_size / l_focal;
      if (i < n && i >= 0 && j < n && j >= 0) {
        d_i *= percell; d_j *= percell;
        d_i -= floor(d_i); d_j -= floor(d_j);
        d_i *= 256; d_j *= 256;
        double col[3];
        mz_interpolate(ceil_t, d_i, d_j, eff_ps, tps, tps, col, !typing_f64);
        int32_t* px = rgb + ((size_t)d_h * H + d_v) * 3;
        for (int c = 0; c < 3; ++c) px[c] = mz_clip_int(light * (alpha * 1.0 + (1.0 - alpha) * col[c]));
      }
    }
  }
  const float cs_f = (float)cell_size;
  for (int d_h = 0; d_h < W; ++d_h) { /* walls :247-318 */
    if (!typing_f64) {
#define REAL float
#define RFABS fabsf
#define RFLOOR floorf
#include "mz_wall_stage.inc"
#undef REAL
#undef RFABS
#undef RFLOOR
    } else {
#define REAL double
#define RFABS fabs
#define RFLOOR floor
#include "mz_wall_stage.inc"
#undef REAL
#undef RFABS
#undef RFLOOR
    }
  }
  if (h->command_in_observation) { /* maze_continuous_3d.py:23-29,102-107 */
    const int idx = h->cmd_idx[e] < h->n_cmd ? h->cmd_idx[e] : h->n_cmd - 1;
    const int cmd = h->commands[(size_t)t * h->n_cmd + idx];
    const int sx = (int)(0.25 * H), sy = (int)(0.10 * H), ex = (int)(0.25 * H + 0.50 * H), ey = (int)(0.10 * H + 0.05 * W);
    for (int x = sx; x < ex && x < W; ++x)
      for (int y = sy; y < ey && y < H; ++y)
        for (int c = 0; c < 3; ++c) rgb[((size_t)x * H + y) * 3 + c] = (int32_t)MZ_LANDMARK_RGB[cmd][c];
  }
}

/* cell_exposed of maze_view (ray_caster_utils.py:153,250-255): every column's DDA_2D (:47-115) lists the cells its ray
 * crosses within 0.6 * visibility (the agent's own cell first, the wall cell it stops at last) and maze_view marks each
 * listed cell with probability 0.05 (`random.random() < 0.05`, an unseeded stream in the reference).  Here the k-th
 * listed cell of column d_h takes word k & 3 of xo_env_draw_sub(seed, gid, tick, 5, 64 * d_h + (k >> 2)) and is
 * marked iff word * 2^-32 < prob; prob >= 1 marks every listed cell (used to pin the cell lists themselves).
 * Same float32 DDA as mz_view above. */
#define XO_DRAW_EXPOSE 5u
void xo_maze_expose(const xo_maze* h, uint64_t seed, uint64_t gid_base, uint64_t tick, double prob, uint8_t* exposed) {
  const int W = h->W, NG = h->NG, N = h->n_env;
  for (int e = 0; e < N; ++e) {
    const int t = h->env_task[e];
    const int32_t* in = h->ints + (size_t)t * 8;
    const double* db = h->dbl + (size_t)t * 8;
    const int n = in[0];
    const double cell_size = db[0], fol = db[3], visibility = h->visibility, l_focal = 0.20;
    const int8_t* walls = h->walls + (size_t)t * NG * NG;
    uint8_t* ex = exposed + (size_t)e * NG * NG;
    memset(ex, 0, (size_t)NG * NG);
    const float pos[2] = {(float)h->pos[e], (float)h->pos[(size_t)N + e]};
    const double ori = h->ori[e];
    const double half_h = tan(fol / 2) * l_focal;
    const double pixel_size = 2.0 * half_h / W;
    const double s_ori = sin(ori), c_ori = cos(ori);
    const double pixel_factor = pixel_size / l_focal;
    const float cs_f = (float)cell_size, eps_f = (float)1.0e-8, vis_f = (float)visibility;
    const float vis06 = (float)(visibility * 0.60);   /* float32 hit_dist against a Python float: compared in float32 */
    const uint64_t gid = gid_base + (uint64_t)e;
    double tan_hp = (-0.5 - W / 2.0) * pixel_factor;
    for (int d_h = 0; d_h < W; ++d_h) {
      tan_hp += pixel_factor;
      const double cos_hp = sqrt(1.0 / (1.0 + tan_hp * tan_hp));
      const double sin_hp = tan_hp * cos_hp;
      const float so = (float)(sin_hp * c_ori + cos_hp * s_ori);
      const float co = (float)(cos_hp * c_ori - sin_hp * s_ori);
      const int i0 = (int)(pos[0] / cs_f), j0 = (int)(pos[1] / cs_f);
      const float c_sign = co < 0 ? -1.0f : 1.0f, s_sign = so < 0 ? -1.0f : 1.0f;
      const float ddx = fabsf(co) < eps_f ? fabsf(cs_f / eps_f) : fabsf(cs_f / co);
      const float ddy = fabsf(so) < eps_f ? fabsf(cs_f / eps_f) : fabsf(cs_f / so);
      const float d_x = co > 0 ? ((float)((i0 + 1) * cell_size) - pos[0]) : ((float)(i0 * cell_size) - pos[0]);
      const float d_y = so > 0 ? ((float)((j0 + 1) * cell_size) - pos[1]) : ((float)(j0 * cell_size) - pos[1]);
      float sdx = fabsf(co) < eps_f ? c_sign * (d_x / eps_f) : d_x / co;
      float sdy = fabsf(so) < eps_f ? s_sign * (d_y / eps_f) : d_y / so;
      const int di = co > 0 ? 1 : -1, dj = so > 0 ? 1 : -1;
      int hi = i0, hj = j0, k = 0;
      float hit_dist = 0.0f;
      uint32_t w[4] = {0, 0, 0, 0};
#define MZ_EXPOSE(ci, cj)                                                                      \
  do {                                                                                         \
    if ((k & 3) == 0) xo_env_draw_sub(seed, gid, tick, XO_DRAW_EXPOSE, 64u * (uint32_t)d_h + (uint32_t)(k >> 2), w); \
    const int hit_ = prob >= 1.0 || (double)w[k & 3] * (1.0 / 4294967296.0) < prob;            \
    if (hit_ && (ci) >= 0 && (ci) < n && (cj) >= 0 && (cj) < n) ex[(ci) * NG + (cj)] = 1;      \
    if (k < 255) ++k;                                                                          \
  } while (0)
      MZ_EXPOSE(i0, j0);
      while (hit_dist < vis_f) {
        const int xstep = sdx < sdy;
        if (xstep) { hi += di; sdy -= sdx; hit_dist += sdx; }
        else { hj += dj; sdx -= sdy; hit_dist += sdy; }
        if (hi < 0 || hi >= n) { if (hj < 0 || hj >= n) break; }
        else {
          if (hit_dist <= vis06) MZ_EXPOSE(hi, hj);
          if (hj >= 0 && hj < n && walls[hi * NG + hj] > 0) break;
        }
        if (xstep) sdx = ddx; else sdy = ddy;
      }
#undef MZ_EXPOSE
    }
  }
}

void xo_maze_render(const xo_maze* h, uint8_t* frames, float* command_rgb, int n_threads) {
  xo_maze_render_typed(h, frames, command_rgb, n_threads, 0);
}

void xo_maze_render_typed(const xo_maze* h, uint8_t* frames, float* command_rgb, int n_threads, int typing_f64) {
  const size_t fsz = (size_t)h->W * h->H * 3;
  (void)n_threads;
#ifdef _OPENMP
#pragma omp parallel for num_threads(n_threads > 0 ? n_threads : 1) schedule(dynamic, 1)
#endif
  for (int e = 0; e < h->n_env; ++e) {
    int32_t* rgb = (int32_t*)malloc(fsz * sizeof(int32_t));
    mz_view(h, e, rgb, typing_f64);
    if (frames)
      for (size_t k = 0; k < fsz; ++k) frames[(size_t)e * fsz + k] = (uint8_t)rgb[k]; /* astype('uint8') :113 */
    free(rgb);
    if (command_rgb) {
      const int t = h->env_task[e];
      const int idx = h->cmd_idx[e] < h->n_cmd ? h->cmd_idx[e] : h->n_cmd - 1;
      const int cmd = h->commands[(size_t)t * h->n_cmd + idx];
      for (int c = 0; c < 3; ++c) command_rgb[(size_t)e * 3 + c] = MZ_LANDMARK_RGB[cmd][c];
    }
  }
}

/* ------------------------------------------------------------------------------------------------
 * AnyMDP POMDP / MTPOMDP — anymdp_env.py:112-132 (token loop :116-126) and get_observation :148-157.
 * Draw order of the reference within one step(): per action token (u, z), then d_obs observation uniforms;
 * a reset draws the s_0 uniform, then d_obs observation uniforms.
 * Philox purposes (free-running): token k -> 32+k (words 0,1: u; 2,3: z); observation token k -> 64+k
 * (words 0,1: after a step; words 2,3: after a reset); s_0 -> 1.
 * ---------------------------------------------------------------------------------------------- */
static void tok_observe(const xo_anymdp_tok* h, int i, const double* u_obs /*[d_obs][n_env]*/, int32_t* obs) {
  const xo_anymdp* m = h->m;
  const int t = m->env_task[i], s = m->state[i];
  for (int k = 0; k < h->d_obs; ++k) {
    const double* row = h->obs_cdf + ((((size_t)t * h->d_obs + k) * m->S) + s) * (size_t)h->n_obs;
    obs[(size_t)i * h->d_obs + k] = xo_upper_bound(row, h->n_obs, u_obs[(size_t)k * m->n_env + i]); /* :150-157 */
  }
}

static void tok_reset_one(xo_anymdp_tok* h, int i, double u_reset, const double* u_obs_reset, int32_t* obs) {
  anymdp_reset_one(h->m, i, u_reset, 0);
  if (obs) tok_observe(h, i, u_obs_reset, obs);
}

void xo_anymdp_tok_reset_injected(xo_anymdp_tok* h, const uint8_t* mask, const double* u_reset,
                                  const double* u_obs_reset, int32_t* obs) {
  for (int i = 0; i < h->m->n_env; ++i)
    if (!mask || mask[i]) tok_reset_one(h, i, u_reset[i], u_obs_reset, obs);
}

static void tok_step_one(xo_anymdp_tok* h, int i, const int32_t* action, const double* u, const float* z,
                         const double* u_obs, double u_reset, const double* u_obs_reset, int32_t* obs,
                         float* reward, float* reward_gt, uint8_t* terminated, uint8_t* truncated,
                         int32_t* final_obs, int mode) {
  xo_anymdp* m = h->m;
  const int S = m->S, A = m->A, N = m->n_env, t = m->env_task[i];
  if (final_obs) for (int k = 0; k < h->d_obs; ++k) final_obs[(size_t)i * h->d_obs + k] = -1;
  if (mode == 1 && m->need_reset[i]) {
    tok_reset_one(h, i, u_reset, u_obs_reset, obs);
    reward[i] = 0.0f; reward_gt[i] = 0.0f; terminated[i] = 0; truncated[i] = 0;
    return;
  }
  if (mode == 0 && is_terminal(m, t, m->state[i])) { /* reference raises (:95-96) */
    m->err_flags |= 2u;
    tok_observe(h, i, u_obs, obs);
    reward[i] = 0.0f; reward_gt[i] = 0.0f; terminated[i] = 1;
    truncated[i] = (uint8_t)(m->steps[i] >= m->max_steps[t]);
    return;
  }
  const int steps = m->steps[i] + 1;            /* :113 once per step, not per token */
  const int trunc = steps >= m->max_steps[t];   /* :114 */
  float rsum = 0.0f, rgsum = 0.0f;
  int term = 0, s = m->state[i];
  for (int k = 0; k < h->d_act; ++k) {          /* :120-126 */
    int a = action[(size_t)i * h->d_act + k];
    if (a < 0 || a >= A) { m->err_flags |= 1u; a = a < 0 ? 0 : A - 1; }
    const size_t row = (((size_t)t * S + s) * A + a) * (size_t)S;
    const int s2 = xo_upper_bound(m->cdf + row, S, u[(size_t)k * N + i]);
    const float r_gt = m->rs[(row + s2) * 2], sg = m->rs[(row + s2) * 2 + 1];
    rsum = rsum + fmaf(sg, z[(size_t)k * N + i], r_gt);
    rgsum = rgsum + r_gt;
    s = s2;
    if (is_terminal(m, t, s2)) { term = 1; break; }
  }
  m->state[i] = s; m->steps[i] = steps;
  reward[i] = rsum; reward_gt[i] = rgsum; terminated[i] = (uint8_t)term; truncated[i] = (uint8_t)trunc;
  tok_observe(h, i, u_obs, obs);
  if (term || trunc) {
    if (mode == 2) {
      if (final_obs) for (int k = 0; k < h->d_obs; ++k) final_obs[(size_t)i * h->d_obs + k] = obs[(size_t)i * h->d_obs + k];
      tok_reset_one(h, i, u_reset, u_obs_reset, obs);
    } else if (mode == 1) {
      m->need_reset[i] = 1;
    }
  }
}

void xo_anymdp_tok_step_injected(xo_anymdp_tok* h, const int32_t* action, const double* u, const float* z,
                                 const double* u_obs, const double* u_reset, const double* u_obs_reset,
                                 int32_t* obs, float* reward, float* reward_gt, uint8_t* terminated,
                                 uint8_t* truncated, int32_t* final_obs, int mode) {
  for (int i = 0; i < h->m->n_env; ++i)
    tok_step_one(h, i, action, u, z, u_obs, u_reset[i], u_obs_reset, obs, reward, reward_gt, terminated,
                 truncated, final_obs, mode);
}

static void tok_draws(const xo_anymdp_tok* h, uint64_t seed, uint64_t gid, uint64_t tick, int i, double* u,
                      float* z, double* u_obs, double* u_reset, double* u_obs_reset) {
  const int N = h->m->n_env;
  uint32_t w[4];
  for (int k = 0; k < h->d_act; ++k) {
    xo_env_draw(seed, gid, tick, 32u + (uint32_t)k, w);
    u[(size_t)k * N + i] = xo_u53(w[0], w[1]);
    xo_box_muller(w[2], w[3], &z[(size_t)k * N + i], 0);
  }
  for (int k = 0; k < h->d_obs; ++k) {
    xo_env_draw(seed, gid, tick, 64u + (uint32_t)k, w);
    u_obs[(size_t)k * N + i] = xo_u53(w[0], w[1]);
    u_obs_reset[(size_t)k * N + i] = xo_u53(w[2], w[3]);
  }
  xo_env_draw(seed, gid, tick, 1, w);
  u_reset[i] = xo_u53(w[0], w[1]);
}

void xo_anymdp_tok_reset(xo_anymdp_tok* h, uint64_t seed, uint64_t gid_base, uint64_t tick, const uint8_t* mask,
                         int32_t* obs) {
  const int N = h->m->n_env;
  double* uo = (double*)malloc(sizeof(double) * (size_t)h->d_obs * N);
  for (int i = 0; i < N; ++i) {
    if (mask && !mask[i]) continue;
    uint32_t w[4];
    for (int k = 0; k < h->d_obs; ++k) {
      xo_env_draw(seed, gid_base + (uint64_t)i, tick, 64u + (uint32_t)k, w);
      uo[(size_t)k * N + i] = xo_u53(w[2], w[3]);
    }
    xo_env_draw(seed, gid_base + (uint64_t)i, tick, 1, w);
    tok_reset_one(h, i, xo_u53(w[0], w[1]), uo, obs);
  }
  free(uo);
}

void xo_anymdp_tok_step(xo_anymdp_tok* h, uint64_t seed, uint64_t gid_base, uint64_t tick, const int32_t* action,
                        int32_t* obs, float* reward, float* reward_gt, uint8_t* terminated, uint8_t* truncated,
                        int32_t* final_obs, int mode) {
  const int N = h->m->n_env;
  double* u = (double*)malloc(sizeof(double) * (size_t)h->d_act * N);
  float* z = (float*)malloc(sizeof(float) * (size_t)h->d_act * N);
  double* uo = (double*)malloc(sizeof(double) * (size_t)h->d_obs * N);
  double* uor = (double*)malloc(sizeof(double) * (size_t)h->d_obs * N);
  double* ur = (double*)malloc(sizeof(double) * (size_t)N);
  for (int i = 0; i < N; ++i) tok_draws(h, seed, gid_base + (uint64_t)i, tick, i, u, z, uo, ur, uor);
  xo_anymdp_tok_step_injected(h, action, u, z, uo, ur, uor, obs, reward, reward_gt, terminated, truncated,
                              final_obs, mode);
  free(u); free(z); free(uo); free(uor); free(ur);
}
