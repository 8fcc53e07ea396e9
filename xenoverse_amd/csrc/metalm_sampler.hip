// metalm_sampler.hip — MetaLMV3 tasks made on the device: xv_metalm_sample_tasks generates a candidate's three networks and
// runs the reference's acceptance protocol (xenoverse/metalang/generator_v3.py sample_and_check_task :25-46) on them in the
// SAME launch, one 256-thread workgroup per candidate.  Host restatement: xenoverse_amd/metalang/sampler_host.py; the
// model, the keys and what is bit-equal to what: DESIGN.md §3.7.0.
//
// The networks.  RandomLM seeds enc, dec and rnn with the same seed, so the three weight matrices are the SAME stream of
// standard normals z, each scaled by its own sqrt(2 / (n_in + n_out)) and by 3, and the RNN's bias is 0.1 z behind its
// weights.  z[i] is member i & 1 of the fp64 Box-Muller pair of the Philox call (seed, candidate, tick 0,
// XV_DRAW_METALM_TASK, sub = i >> 1): a thread forms a pair once and stores it into every table that holds it (up to three),
// in the layouts xv_metalm_set_task takes.  emb is the layer_norm of the encoder's columns, one column per thread, summed
// in numpy's order (lm_np_sum) so that it is numpy's bit for bit: the recurrence is chaotic, and a table 1 ulp off would
// make the task another task.
//
// The protocol.  reset(), policy(1e4), step(cached), policy(1e-6), step(cached) of an engine with this seed, env_id_base =
// the candidate and tick 0: wave 0 runs the query (tick 0) while the others wait; then wave 0 runs the T = 1e4 policy pass
// (tick 1) and wave 1 the T = 1e-6 one (tick 3), each with the label pass over its own answer fused (lm_pass), wave 2 the
// two greedy passes (ticks 2 and 4) and wave 3 the two rnd passes (ticks 2 and 4): every pass starts from the state the
// query left.  They meet at one barrier, behind which the first thread forms both rewards and the status.  The passes'
// XV_DEVERR_* bits go to the candidate's own flags word, never to the engine's.
#define XV_KERNELS_ONLY
#include "metalm.hip"
#undef XV_KERNELS_ONLY
#include "xv_draws.h"

#define XV_DRAW_METALM_TASK 14u

struct LMSample {
  uint64_t cand_base;
  double *emb, *w_h, *b_h, *w_d, *b_d, *enc_w;      // [n_cand] x [V][E], [H+E][H], [H], [H][V], [V], [E][V]
  int32_t* status;         // [n_cand]
  double* reward;          // [n_cand][2]; nullable, as all below
  double* ppl;             // [n_cand][2][3]
  int32_t* query;          // [n_cand][max_len]
  int32_t* query_len;      // [n_cand]
  int32_t* answer;         // [n_cand][2][max_len]
  int32_t* answer_len;     // [n_cand][2]
  uint32_t* flags;         // [n_cand]
};

// sum of f(0) .. f(n - 1) in the order of numpy's add.reduce over a contiguous row of n <= 128 doubles: below 8 elements
// left to right from 0; otherwise eight accumulators over the whole blocks of 8, combined pairwise, then the rest in order
template <class F>
__device__ __forceinline__ double lm_np_sum(int n, F f) {
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; ++i) res += f(i);
    return res;
  }
  double r[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) r[k] = f(k);
  int i = 8;
  for (; i < n - (n & 7); i += 8) {
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] += f(i + k);
  }
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += f(i);
  return res;
}

// sqrt, correctly rounded whatever the library's last bit: one Markstein step (the residual is exact in the FMA)
__device__ __forceinline__ double lm_sqrt_rn(double v) {
  const double s = sqrt(v);
  if (!(s > 0.0) || !(s <= 1.0e300)) return s;
  return fma(fma(-s, s, v), 0.5 / s, s);
}

template <bool TL>
__global__ __launch_bounds__(256) void metalm_sample_kernel(LMArgs P, LMSample S) {
  extern __shared__ double lm_tab[];
  __shared__ double lm_hs[4][LM_H_MAX];
  __shared__ double lm_cache[LM_H_MAX];
  __shared__ double lm_mean[2][3];      // per policy / step pair: ppl, ppl_min, ppl_max
  __shared__ uint32_t lm_err[4];
  __shared__ double lm_tt[18 * 16];
  for (int i = threadIdx.x; i < 18 * 16; i += blockDim.x) lm_tt[i] = __longlong_as_double((long long)lm_tanh_tab[i]);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int V = P.V, E = P.E, H = P.H, max_len = P.max_len;
  const size_t cand = blockIdx.x;
  const uint64_t gid = S.cand_base + (uint64_t)cand;
  double* g_emb = S.emb + cand * V * E;
  double* g_w_h = S.w_h + cand * (H + E) * H;
  double* g_b_h = S.b_h + cand * H;
  double* g_w_d = S.w_d + cand * H * V;
  double* g_b_d = S.b_d + cand * V;
  double* g_enc = S.enc_w + cand * E * V;

  // ---- the networks: element i of the stream goes to enc_w.flat[i], dec_w.flat[i] and rnn_w.flat[i] (rnn_b behind it) ----
  const int n_enc = V * E, n_dec = V * H, n_rnn = H * (H + E);
  const int n_z = max(max(n_enc, n_dec), n_rnn + H);
  const double s_enc = sqrt(2.0 / (double)(V + E)), s_dec = sqrt(2.0 / (double)(H + V)),
               s_rnn = sqrt(2.0 / (double)((E + H) + H));
  for (int p = threadIdx.x; 2 * p < n_z; p += blockDim.x) {
    double z2[2];
    xv_normal2(xv_pair(xv_env_draw_sub(P.seed, gid, 0, XV_DRAW_METALM_TASK, (uint32_t)p)), &z2[0], &z2[1]);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int i = 2 * p + m;
      const double z = z2[m];
      if (i < n_enc) g_enc[i] = (s_enc * z) * 3.0;                                  // enc_w [E][V]
      if (i < n_dec) g_w_d[(i % H) * V + i / H] = (s_dec * z) * 3.0;                // dec_w [V][H], stored transposed
      if (i < n_rnn)
        g_w_h[(i % (H + E)) * H + i / (H + E)] = (s_rnn * z) * 3.0;                 // rnn_w [H][H+E], stored transposed
      else if (i < n_rnn + H)
        g_b_h[i - n_rnn] = 0.1 * z;
    }
  }
  for (int v = threadIdx.x; v < V; v += blockDim.x) g_b_d[v] = 0.0;
  __syncthreads();
  // ---- emb[v] = layer_norm(enc_w[:, v]) as numpy forms it: mean = sum / E, var = sum((x - mean)^2) / E ----
  for (int v = threadIdx.x; v < V; v += blockDim.x) {
    const double* x = g_enc + v;
    const double mean = lm_np_sum(E, [&](int e) { return x[(size_t)e * V]; }) / (double)E;
    const double var = lm_np_sum(E, [&](int e) { const double d = x[(size_t)e * V] - mean; return d * d; }) / (double)E;
    const double den = lm_sqrt_rn(var) + 1.0e-8;
    for (int e = 0; e < E; ++e) g_emb[(size_t)v * E + e] = (x[(size_t)e * V] - mean) / den;
  }
  __syncthreads();

  // ---- the candidate's tables, in LDS where they fit ----
  const double *emb = g_emb, *w_h = g_w_h, *b_h = g_b_h, *w_d = g_w_d, *b_d = g_b_d;
  if (TL) {
    const int n0 = V * E, n1 = n0 + (H + E) * H, n2 = n1 + H, n3 = n2 + H * V, n4 = n3 + V;
    for (int i = threadIdx.x; i < n4; i += blockDim.x)
      lm_tab[i] = i < n0 ? emb[i] : i < n1 ? w_h[i - n0] : i < n2 ? b_h[i - n1] : i < n3 ? w_d[i - n2] : b_d[i - n3];
    emb = lm_tab; w_h = lm_tab + n0; b_h = lm_tab + n1; w_d = lm_tab + n2; b_d = lm_tab + n3;
  }
  __syncthreads();

  uint32_t err = 0u;
  double* hs = lm_hs[wave];
  LMPass A;
  A.skip = false; A.n_ans = 0; A.ans = nullptr; A.u = nullptr; A.gid = gid;
  A.at = A.at2 = 0; A.cap = max_len; A.dst2 = nullptr;
  // ---- reset(): the query from the zero state, tick 0 ----
  if (wave == 0) {
    for (int j = lane; j < H; j += 64) hs[j] = 0.0;
    lm_wave_sync();
    A.kind = LM_QUERY; A.tick = 0; A.temp0 = 10.0; A.temp1 = 1.0; A.fuse = false;
    A.dst = S.query ? S.query + cand * max_len : nullptr;
    lm_pass<true>(P, emb, w_h, b_h, w_d, b_d, hs, lm_tt, lane, A, err);
    if (A.dst)
      for (int i = A.n_out + lane; i < max_len; i += 64) A.dst[i] = 0;
    if (lane == 0 && S.query_len) S.query_len[cand] = A.n_out;
    for (int j = lane; j < H; j += 64) lm_cache[j] = hs[j];
  }
  __syncthreads();
  // ---- policy(1e4), step(cached), policy(1e-6), step(cached): ticks 1 .. 4, every pass from the cached state ----
  const int kind = wave < 2 ? LM_POLICY : wave == 2 ? LM_GREEDY : LM_LOW;
  for (int s = 0; s < (wave < 2 ? 1 : 2); ++s) {
    const int sub = wave < 2 ? wave : s;      // the policy / step pair the pass belongs to
    for (int j = lane; j < H; j += 64) hs[j] = lm_cache[j];
    lm_wave_sync();
    const double temp = kind == LM_POLICY ? (sub == 0 ? 1.0e4 : 1.0e-6) : 1.0;
    A.kind = kind;
    A.tick = (uint64_t)(2 * sub + (kind == LM_POLICY ? 1 : 2));
    A.temp0 = A.temp1 = temp;
    A.fuse = kind == LM_POLICY;
    A.dst = kind == LM_POLICY && S.answer ? S.answer + (cand * 2 + sub) * max_len : nullptr;
    lm_pass<true>(P, emb, w_h, b_h, w_d, b_d, hs, lm_tt, lane, A, err);
    if (A.dst)
      for (int i = A.n_out + lane; i < max_len; i += 64) A.dst[i] = 0;
    if (lane == 0) {
      if (kind == LM_POLICY && S.answer_len) S.answer_len[cand * 2 + sub] = A.n_out;
      const double sum = kind == LM_POLICY ? A.ppl_sum2 : A.ppl_sum;      // a policy wave reports its label pass
      lm_mean[sub][kind == LM_POLICY ? 0 : kind == LM_GREEDY ? 1 : 2] = A.n_step ? sum / (double)A.n_step : 0.0;
    }
  }
  if (lane == 0) lm_err[wave] = err;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t flags = lm_err[0] | lm_err[1] | lm_err[2] | lm_err[3];
    double r[2];
    for (int sub = 0; sub < 2; ++sub) {
      const double ppl = lm_mean[sub][0], ppl_min = lm_mean[sub][1], ppl_max = lm_mean[sub][2];
      r[sub] = (ppl_max - ppl_min) / fmax(ppl - ppl_min + 0.1, 1.0e-3) - 2.0;      // metalangv3.py:32
      if (S.reward) S.reward[cand * 2 + sub] = r[sub];
      if (S.ppl)
        for (int k = 0; k < 3; ++k) S.ppl[(cand * 2 + sub) * 3 + k] = lm_mean[sub][k];
    }
    const bool finite = isfinite(r[0]) && isfinite(r[1]) && !(flags & XV_DEVERR_NONFINITE);
    S.status[cand] = !finite ? XV_METALM_NONFINITE : r[0] > 0.0 ? XV_METALM_REWARD_LOW : r[1] < 2.0 ? XV_METALM_REWARD_HIGH
                                                                                                    : XV_METALM_ACCEPTED;
    if (S.flags) S.flags[cand] = flags;
  }
}

extern "C" int xv_metalm_sample_tasks(xv_engine* e, uint64_t seed, int64_t cand_base, int n_cand, int n_vocab, int n_emb,
                                      int n_hidden, int max_len, int stop_token, const int32_t* function_tokens,
                                      int n_function, double* emb, double* w_h_t, double* b_h, double* w_d_t, double* b_d,
                                      double* enc_w, int32_t* status, double* reward, double* ppl, int32_t* query,
                                      int32_t* query_len, int32_t* answer, int32_t* answer_len, uint32_t* flags) {
  XV_CHECK_ARG(e != nullptr && n_cand >= 1 && cand_base >= 0 && cand_base <= INT64_MAX - n_cand);
  XV_CHECK_ARG(n_function >= 0 && (n_function == 0 || function_tokens != nullptr));
  XV_CHECK_ARG(emb && w_h_t && b_h && w_d_t && b_d && enc_w && status);
  const struct { const char* name; int v, lo, hi; } lim[4] = {{"n_vocab", n_vocab, LM_V_MIN, LM_V_MAX},
                                                              {"n_hidden", n_hidden, 1, LM_H_MAX},
                                                              {"n_emb", n_emb, 1, LM_E_MAX},
                                                              {"max_len", max_len, 1, LM_LEN_MAX}};
  for (int i = 0; i < 4; ++i)
    if (lim[i].v < lim[i].lo || lim[i].v > lim[i].hi) {
      xv_set_error("xv_metalm_sample_tasks: %s = %d is outside the supported range %d .. %d", lim[i].name, lim[i].v,
                   lim[i].lo, lim[i].hi);
      return XV_ERR_UNSUPPORTED;
    }
  XV_CHECK_ARG(stop_token >= 0 && stop_token < n_vocab);
  LMArgs a = LMArgs();
  a.N = n_cand; a.V = n_vocab; a.E = n_emb; a.H = n_hidden; a.max_len = max_len; a.stop = stop_token;
  for (int i = 0; i < n_function; ++i) {
    const int t = function_tokens[i];
    if (t < 0 || t >= n_vocab) {
      xv_set_error("xv_metalm_sample_tasks: function token %d is outside the vocabulary of %d", t, n_vocab);
      return XV_ERR_INVALID;
    }
    a.fmask[t >> 6] |= 1ull << (t & 63);
  }
  const int tab = n_vocab * n_emb + (n_hidden + n_emb) * n_hidden + n_hidden + n_hidden * n_vocab + n_vocab;
  a.tab_n = tab <= LM_TAB_CAP ? tab : 0;
  a.seed = seed;
  LMSample s{(uint64_t)cand_base, emb, w_h_t, b_h, w_d_t, b_d, enc_w, status, reward, ppl, query, query_len, answer,
             answer_len, flags};
  XV_HIP(hipSetDevice(e->device));
  const dim3 grid((unsigned)n_cand), block(256);
  if (a.tab_n)
    hipLaunchKernelGGL(metalm_sample_kernel<true>, grid, block, sizeof(double) * (size_t)a.tab_n, e->stream, a, s);
  else
    hipLaunchKernelGGL(metalm_sample_kernel<false>, grid, block, 0, e->stream, a, s);
  XV_LAUNCH_CHECK();
  return XV_OK;
}
