// metalang_sampler.hip — MetaLangV2 and MetaLangV1 tasks made on the device, in the layouts xv_metalang_set_task and
// xv_metalang1_set_task borrow.  Reference: xenoverse/metalang/task_sampler.py TaskSamplerV2 :22-50 and TaskSamplerV1 :52-73.
// Host restatements the kernels are held to: xenoverse_amd/metalang/sampler_host_v2.py and sampler_host_v1.py; the model
// and what is equal to what: DESIGN.md §3.6 / §3.9 "Tasks made on the device".  The reference has no acceptance test for
// these tasks: every candidate is a task.
//
// Randomness is counter-based, in the index layout of xv_draws.h: xv_index_draw(seed, task, tick, purpose, sub).  Task k of
// (seed, arguments) is a pure function of those: no kernel knows its launch.
//   MS_P_HEAD    tick 0, sub 0: first uniform -> the n-gram choice, list[floor(u m)], of either sampler
//   MS_P_EMB ... MS_P_B_OUT (V2)   tick 0, sub = q >> 1: element q of the array is half q & 1 (cos, sin) of the fp64
//                Box-Muller pair (xv_normal2) of the call
//   MS_P_LENGTH  (V1) tick 0, sub = pattern: first uniform -> Poisson(n_gram) by inversion (ms_poisson)
//   MS_P_TOKEN   (V1) tick = pattern, sub = pos >> 1: token pos is floor(u n_vocab) of half pos & 1 of the call
//
// V2 is one launch over (task, chunk of MS_CHUNK calls): a task's five arrays are one run of calls, array after array, a
// call is one lane's, and the lane stores its pair side by side, so a wave writes 1 KiB without a gap.  An array with an odd
// element count ends in a call whose second half is dropped: nothing is written behind an array.  The input layer is
// padded to NG slots: elements at and beyond the task's own n are exact zeros and cost no draw.
//
// V1 has variable lengths, hence three launches: lengths (a lane per pattern), an exclusive prefix sum (one workgroup,
// 64-bit carry: the total is reported unsaturated so that the caller can refuse more than 2^31 - 1 tokens), tokens (a lane
// per token, which finds its pattern by bisection in the offsets: a token depends on (seed, task, pattern, position) only).
#include <climits>

#include "xv_common.h"
#include "xv_draws.h"

namespace {

constexpr int MS_BLOCK = 256;
constexpr int MS_CHUNK = 2048;      // calls (pairs of elements) per workgroup of the V2 launch
constexpr int MS_SCAN_BLOCK = 1024;
// csrc/metalang.hip's limits (ML_V_MAX, ML_H_MAX, ML_E_MAX, ML_NG_MAX): what xv_metalang_create takes
constexpr int MS_V_MAX = 1024, MS_H_MAX = 128, MS_E_MAX = 64, MS_NG_MAX = 8;

enum : uint32_t { MS_P_HEAD = 0, MS_P_EMB = 1, MS_P_W_IN = 2, MS_P_B_IN = 3, MS_P_W_OUT = 4, MS_P_B_OUT = 5, MS_P_LENGTH = 6,
                  MS_P_TOKEN = 7 };

struct MsList {
  int n;
  int32_t v[XV_METALANG_SAMPLER_LIST_MAX];
  double exp_neg[XV_METALANG_SAMPLER_LIST_MAX];      // V1: exp(-v), formed once by the caller
};

__device__ __forceinline__ int ms_choice(uint64_t seed, uint64_t gid, int m) {
  const int i = xv_floor_int(xv_pair(xv_index_draw(seed, gid, 0, MS_P_HEAD, 0)).a, m);
  return i < m - 1 ? i : m - 1;
}

// ---- V2 ----------------------------------------------------------------------------------------------------------------
struct Ms2Args {
  uint64_t seed, task_base;
  int n_task, V, E, H, NG, chunks;
  double lambda;
  MsList list;
  double *emb, *w_in, *b_in, *w_out, *b_out, *lam;
  int32_t* n_gram;
};

__global__ __launch_bounds__(MS_BLOCK) void ms2_kernel(Ms2Args A) {
  const unsigned task = blockIdx.x / (unsigned)A.chunks, chunk = blockIdx.x % (unsigned)A.chunks;
  if (task >= (unsigned)A.n_task) return;
  const uint64_t gid = A.task_base + task;
  const int n = A.list.v[ms_choice(A.seed, gid, A.list.n)];
  if (chunk == 0 && threadIdx.x == 0) {
    A.n_gram[task] = n;
    A.lam[task] = A.lambda;
  }
  // per array: elements as stored (padded), elements that are drawn, calls
  const int c0 = A.V * A.E, c1 = A.NG * A.E * A.H, c2 = A.NG * A.H, c3 = A.H * A.V, c4 = A.V;
  const int l1 = n * A.E * A.H, l2 = n * A.H;
  const int p0 = (c0 + 1) >> 1, p1 = (c1 + 1) >> 1, p2 = (c2 + 1) >> 1, p3 = (c3 + 1) >> 1, p4 = (c4 + 1) >> 1;
  const int P = p0 + p1 + p2 + p3 + p4;
  const int end = min(P, (int)(chunk + 1) * MS_CHUNK);
  for (int p = (int)chunk * MS_CHUNK + (int)threadIdx.x; p < end; p += MS_BLOCK) {
    int q = p, cnt, live;
    uint32_t purpose;
    double* dst;
    if (q < p0) {
      cnt = live = c0; purpose = MS_P_EMB; dst = A.emb + (size_t)task * c0;
    } else if ((q -= p0) < p1) {
      cnt = c1; live = l1; purpose = MS_P_W_IN; dst = A.w_in + (size_t)task * c1;
    } else if ((q -= p1) < p2) {
      cnt = c2; live = l2; purpose = MS_P_B_IN; dst = A.b_in + (size_t)task * c2;
    } else if ((q -= p2) < p3) {
      cnt = live = c3; purpose = MS_P_W_OUT; dst = A.w_out + (size_t)task * c3;
    } else {
      q -= p3;
      cnt = live = c4; purpose = MS_P_B_OUT; dst = A.b_out + (size_t)task * c4;
    }
    const int e0 = 2 * q;      // e0 < cnt: q is one of the array's (cnt + 1) / 2 calls
    double z0 = 0.0, z1 = 0.0;
    if (e0 < live) xv_normal2(xv_pair(xv_index_draw(A.seed, gid, 0, purpose, (uint32_t)q)), &z0, &z1);
    if (e0 + 1 >= cnt) {
      dst[e0] = z0;
      continue;
    }
    if (e0 + 1 >= live) z1 = 0.0;
    // one 16-byte store where the task's array starts on a 16-byte boundary (task * cnt even), else two of 8
    if ((reinterpret_cast<uintptr_t>(dst + e0) & 15u) == 0) {
      *reinterpret_cast<double2*>(dst + e0) = make_double2(z0, z1);
    } else {
      dst[e0] = z0;
      dst[e0 + 1] = z1;
    }
  }
}

// ---- V1 ----------------------------------------------------------------------------------------------------------------
// Poisson(lam) by inversion on ONE uniform: the smallest k with u < sum_{i <= k} p_i, p_0 = exp(-lam) (handed in), p_i =
// p_{i-1} lam / i.  Products, quotients and sums only, each correctly rounded on host and device alike: the same integer on
// both.  The search stops at k_max = 2 lam + 64 (the sum's rounding leaves the last 1e-16 of the tail unresolved anyway).
__device__ __forceinline__ int ms_poisson(double u, int lam, double exp_neg) {
  const int k_max = 2 * lam + 64;
  const double l = (double)lam;
  double p = exp_neg, s = exp_neg;
  int k = 0;
  while (u >= s && k < k_max) {
    ++k;
    p = p * l / (double)k;
    s += p;
  }
  return k;
}

struct Ms1Args {
  uint64_t seed, task_base;
  int n_task, n_patterns;
  MsList list;
};

__global__ __launch_bounds__(MS_BLOCK) void ms1_length_kernel(Ms1Args A, int32_t* n_gram, int32_t* lengths) {
  const int64_t i = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
  if (i >= (int64_t)A.n_task * A.n_patterns) return;
  const int task = (int)(i / A.n_patterns), j = (int)(i % A.n_patterns);
  const uint64_t gid = A.task_base + (uint64_t)task;
  const int c = ms_choice(A.seed, gid, A.list.n);
  const int lam = A.list.v[c];
  const int k = ms_poisson(xv_pair(xv_index_draw(A.seed, gid, 0, MS_P_LENGTH, (uint32_t)j)).a, lam, A.list.exp_neg[c]);
  lengths[i] = k < 3 ? 3 : k;
  if (j == 0) n_gram[task] = lam;
}

// pattern_token_offset[0 .. n] = the exclusive prefix sum of lengths[0 .. n), saturated at INT32_MAX; *total is the sum
// itself.  task_pattern_offset[k] = k n_patterns.  One workgroup, tiles of MS_SCAN_BLOCK.
__global__ __launch_bounds__(MS_SCAN_BLOCK) void ms1_scan_kernel(const int32_t* lengths, int n, int n_task, int n_patterns,
                                                                 int32_t* task_pattern_offset, int32_t* offsets,
                                                                 int64_t* total) {
  __shared__ long long wave_sum[MS_SCAN_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long carry = 0;
  for (int base = 0; base < n; base += MS_SCAN_BLOCK) {
    const int i = base + tid;
    long long x = i < n ? (long long)lengths[i] : 0;
    for (int d = 1; d < 64; d <<= 1) {
      const long long y = __shfl_up(x, d, 64);
      if (lane >= d) x += y;
    }
    if (lane == 63) wave_sum[wave] = x;
    __syncthreads();
    long long before = 0, tile = 0;
    for (int w = 0; w < MS_SCAN_BLOCK / 64; ++w) {
      const long long s = wave_sum[w];
      if (w < wave) before += s;
      tile += s;
    }
    const long long incl = carry + before + x;
    if (i < n) offsets[i + 1] = incl > (long long)INT32_MAX ? INT32_MAX : (int32_t)incl;
    carry += tile;
    __syncthreads();
  }
  if (tid == 0) {
    offsets[0] = 0;
    *total = carry;
  }
  for (int k = tid; k <= n_task; k += MS_SCAN_BLOCK) task_pattern_offset[k] = k * n_patterns;
}

// token t of [token_base, token_base + n_token): its pattern is the last p of [0, n_pat) with offsets[p] <= t
__global__ __launch_bounds__(MS_BLOCK) void ms1_token_kernel(Ms1Args A, int n_vocab, const int32_t* offsets, int token_base,
                                                             int n_token, int32_t* tokens) {
  const int64_t i = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
  if (i >= n_token) return;
  const int t = token_base + (int)i;
  int lo = 0, hi = A.n_task * A.n_patterns - 1;
  while (lo < hi) {
    const int mid = lo + ((hi - lo + 1) >> 1);
    if (offsets[mid] <= t) lo = mid;
    else hi = mid - 1;
  }
  const int pos = t - offsets[lo];
  const int task = lo / A.n_patterns, j = lo % A.n_patterns;
  const xv_u2 u = xv_pair(xv_index_draw(A.seed, A.task_base + (uint64_t)task, (uint32_t)j, MS_P_TOKEN, (uint32_t)pos >> 1));
  const int v = xv_floor_int((pos & 1) ? u.b : u.a, n_vocab);
  tokens[t] = v < n_vocab - 1 ? v : n_vocab - 1;
}

int ms_list(const char* who, const int32_t* n_gram_list, const double* exp_neg, int n_list, int hi, MsList* out) {
  if (n_list < 1 || n_list > XV_METALANG_SAMPLER_LIST_MAX) {
    xv_set_error("%s: an n_gram list of %d entries is outside the supported range 1 .. %d", who, n_list,
                 XV_METALANG_SAMPLER_LIST_MAX);
    return XV_ERR_UNSUPPORTED;
  }
  *out = MsList();
  out->n = n_list;
  for (int i = 0; i < n_list; ++i) {
    if (n_gram_list[i] < 1 || n_gram_list[i] > hi) {
      xv_set_error("%s: n_gram = %d is outside the supported range 1 .. %d", who, n_gram_list[i], hi);
      return XV_ERR_UNSUPPORTED;
    }
    out->v[i] = n_gram_list[i];
    out->exp_neg[i] = exp_neg ? exp_neg[i] : 0.0;
  }
  return XV_OK;
}

}  // namespace

extern "C" int xv_metalang_sample_tasks(xv_engine* e, uint64_t seed, int64_t task_base, int n_task, int n_vocab, int n_emb,
                                        int n_hidden, const int32_t* n_gram_list, int n_list, int n_gram_max, double lambda,
                                        double* word_emb, double* weights_inputlayer, double* bias_inputlayer,
                                        double* weights_outputlayer, double* bias_outputlayer, double* lambda_out,
                                        int32_t* n_gram) {
  XV_CHECK_ARG(e != nullptr && n_task >= 1 && task_base >= 0 && task_base <= INT64_MAX - n_task);
  XV_CHECK_ARG(n_gram_list != nullptr && word_emb && weights_inputlayer && bias_inputlayer && weights_outputlayer &&
               bias_outputlayer && lambda_out && n_gram);
  const struct { const char* name; int v, hi; } lim[4] = {{"n_vocab", n_vocab, MS_V_MAX}, {"n_hidden", n_hidden, MS_H_MAX},
                                                         {"n_emb", n_emb, MS_E_MAX}, {"n_gram", n_gram_max, MS_NG_MAX}};
  for (int i = 0; i < 4; ++i)
    if (lim[i].v < 1 || lim[i].v > lim[i].hi) {
      xv_set_error("xv_metalang_sample_tasks: %s = %d is outside the supported range 1 .. %d", lim[i].name, lim[i].v,
                   lim[i].hi);
      return XV_ERR_UNSUPPORTED;
    }
  Ms2Args a = Ms2Args();
  const int rc = ms_list("xv_metalang_sample_tasks", n_gram_list, nullptr, n_list, n_gram_max, &a.list);
  if (rc != XV_OK) return rc;
  a.seed = seed; a.task_base = (uint64_t)task_base; a.n_task = n_task;
  a.V = n_vocab; a.E = n_emb; a.H = n_hidden; a.NG = n_gram_max; a.lambda = lambda;
  a.emb = word_emb; a.w_in = weights_inputlayer; a.b_in = bias_inputlayer; a.w_out = weights_outputlayer;
  a.b_out = bias_outputlayer; a.lam = lambda_out; a.n_gram = n_gram;
  const int calls = (n_vocab * n_emb + 1) / 2 + (n_gram_max * n_emb * n_hidden + 1) / 2 + (n_gram_max * n_hidden + 1) / 2 +
                    (n_hidden * n_vocab + 1) / 2 + (n_vocab + 1) / 2;
  a.chunks = xv_div_up(calls, MS_CHUNK);
  if ((int64_t)n_task * a.chunks > (int64_t)INT32_MAX) {
    xv_set_error("xv_metalang_sample_tasks: n_task = %d is more than the %lld tasks of this size one launch takes", n_task,
                 (long long)(INT32_MAX / a.chunks));
    return XV_ERR_UNSUPPORTED;
  }
  XV_HIP(hipSetDevice(e->device));
  hipLaunchKernelGGL(ms2_kernel, dim3((unsigned)(n_task * a.chunks)), dim3(MS_BLOCK), 0, e->stream, a);
  XV_LAUNCH_CHECK();
  return XV_OK;
}

static int ms1_args(const char* who, xv_engine* e, int64_t task_base, int n_task, int n_patterns, Ms1Args* a) {
  XV_CHECK_ARG(e != nullptr && n_task >= 1 && task_base >= 0 && task_base <= INT64_MAX - n_task);
  if (n_patterns < 1 || n_patterns > XV_METALANG1_SAMPLER_PATTERNS_MAX) {
    xv_set_error("%s: n_patterns = %d is outside the supported range 1 .. %d", who, n_patterns,
                 XV_METALANG1_SAMPLER_PATTERNS_MAX);
    return XV_ERR_UNSUPPORTED;
  }
  if ((int64_t)n_task * n_patterns > (int64_t)INT32_MAX - 1) {
    xv_set_error("%s: %lld patterns are more than the supported %d", who, (long long)n_task * n_patterns, INT32_MAX - 1);
    return XV_ERR_UNSUPPORTED;
  }
  a->task_base = (uint64_t)task_base; a->n_task = n_task; a->n_patterns = n_patterns;
  return XV_OK;
}

extern "C" int xv_metalang1_sample_lengths(xv_engine* e, uint64_t seed, int64_t task_base, int n_task, int n_patterns,
                                           const int32_t* n_gram_list, const double* exp_neg_n_gram, int n_list,
                                           int32_t* n_gram, int32_t* lengths) {
  XV_CHECK_ARG(n_gram_list != nullptr && exp_neg_n_gram != nullptr && n_gram != nullptr && lengths != nullptr);
  Ms1Args a = Ms1Args();
  int rc = ms1_args("xv_metalang1_sample_lengths", e, task_base, n_task, n_patterns, &a);
  if (rc != XV_OK) return rc;
  rc = ms_list("xv_metalang1_sample_lengths", n_gram_list, exp_neg_n_gram, n_list, XV_METALANG1_SAMPLER_NGRAM_MAX, &a.list);
  if (rc != XV_OK) return rc;
  for (int i = 0; i < n_list; ++i) XV_CHECK_ARG(exp_neg_n_gram[i] > 0.0 && exp_neg_n_gram[i] < 1.0);
  a.seed = seed;
  XV_HIP(hipSetDevice(e->device));
  const unsigned grid = (unsigned)(((int64_t)n_task * n_patterns + MS_BLOCK - 1) / MS_BLOCK);
  hipLaunchKernelGGL(ms1_length_kernel, dim3(grid), dim3(MS_BLOCK), 0, e->stream, a, n_gram, lengths);
  XV_LAUNCH_CHECK();
  return XV_OK;
}

extern "C" int xv_metalang1_sample_offsets(xv_engine* e, int n_task, int n_patterns, const int32_t* lengths,
                                           int32_t* task_pattern_offset, int32_t* pattern_token_offset,
                                           int64_t* n_token_total) {
  XV_CHECK_ARG(lengths != nullptr && task_pattern_offset != nullptr && pattern_token_offset != nullptr &&
               n_token_total != nullptr);
  Ms1Args a = Ms1Args();
  const int rc = ms1_args("xv_metalang1_sample_offsets", e, 0, n_task, n_patterns, &a);
  if (rc != XV_OK) return rc;
  XV_HIP(hipSetDevice(e->device));
  hipLaunchKernelGGL(ms1_scan_kernel, dim3(1), dim3(MS_SCAN_BLOCK), 0, e->stream, lengths, n_task * n_patterns, n_task,
                     n_patterns, task_pattern_offset, pattern_token_offset, n_token_total);
  XV_LAUNCH_CHECK();
  return XV_OK;
}

extern "C" int xv_metalang1_sample_tokens(xv_engine* e, uint64_t seed, int64_t task_base, int n_task, int n_patterns,
                                          int n_vocab, const int32_t* pattern_token_offset, int token_base, int n_token,
                                          int32_t* tokens) {
  XV_CHECK_ARG(pattern_token_offset != nullptr && tokens != nullptr && n_vocab >= 1);
  XV_CHECK_ARG(token_base >= 0 && n_token >= 1 && token_base <= INT32_MAX - n_token);
  Ms1Args a = Ms1Args();
  const int rc = ms1_args("xv_metalang1_sample_tokens", e, task_base, n_task, n_patterns, &a);
  if (rc != XV_OK) return rc;
  a.seed = seed;
  XV_HIP(hipSetDevice(e->device));
  const unsigned grid = (unsigned)(((int64_t)n_token + MS_BLOCK - 1) / MS_BLOCK);
  hipLaunchKernelGGL(ms1_token_kernel, dim3(grid), dim3(MS_BLOCK), 0, e->stream, a, n_vocab, pattern_token_offset,
                     token_base, n_token, tokens);
  XV_LAUNCH_CHECK();
  return XV_OK;
}
