// anymdp_garnet.hip — the reference's two remaining AnyMDP task makers on the device (gfx950): GarnetTaskSampler
// (xenoverse/anymdp/task_sampler.py:120-160, task_sampler_utils.py:274-313) and the single-state task, the multi-armed bandit
// (task_sampler_utils.py:258-272), written where xv_anymdp_create reads them.  Counter-based draws (xv_draws.h, the index
// layout: index = task or candidate); the model, its counters and the numpy restatement these kernels are pinned to:
// xenoverse_amd/anymdp/sampler_host_garnet.py, DESIGN.md §3.1.2.
//
// Garnet is a store stream with fp64 log / sincos in front of it: one lane per 16-byte record entry, the eighth lane of a
// 128-byte line storing the line's zero tail, so a wave store is 1 KiB contiguous.  A row's b swap steps and the sort of its
// cuts are sequential and tiny: one lane per row does them in LDS (no per-lane array: no scratch) and leaves the row's
// successors sorted by state with their CDF entries for the lanes that store.
#include "xv_common.h"
#include "xv_draws.h"

namespace {

constexpr int GN_BLOCK = 256;
constexpr int GN_ROWS = 32;                        // rows of one task per workgroup
constexpr int GN_B = XV_ANYMDP_GARNET_B_MAX;       // successors per row, at most
constexpr int GN_S_MAX = 512, GN_A_MAX = 64;       // the step engine's limits (xeno.h, "Supported")
enum : uint32_t { GN_P_HEAD = 0, GN_P_PERM = 1, GN_P_SUCC = 2, GN_P_CUT = 3, GN_P_REWARD = 4 };
enum : uint32_t { BD_P_HEAD = 0, BD_P_ROUND = 1 };

struct GnArgs {
  uint64_t seed, task_base;
  int n_task, S, A, m, b, s0_max, row_lines, chunks;      // m: the smallest real state count (S: every task has S)
  double sigma, lower, upper;
  double* rows;
  int32_t* state_map;
  uint64_t* term_mask;
  double* s0_cdf;
  int32_t* s0_ids;
  int32_t* max_steps;
  int32_t* n_real;
  double* transition;
  double* reward;
  double* noise;
};

// element i of a block of uniforms is half i & 1 of call i >> 1: a loop keeps the call's two uniforms in GN_PAIR's scalars
// (two doubles, not an xv_u2 the compiler would index in scratch) and draws at the even elements
#define GN_PAIR(ua, ub, i, draw)         \
  if (!((i) & 1)) {                      \
    const xv_u2 u_ = xv_pair(draw);      \
    ua = u_.a;                           \
    ub = u_.b;                           \
  }
__device__ __forceinline__ double gn_half(double ua, double ub, int i) { return (i & 1) ? ub : ua; }
// floor(u m), clamped to m - 1 (never reached: u <= 1 - 2^-53; the host clamps too)
__device__ __forceinline__ int gn_floor(double u, int m) {
  const int v = xv_floor_int(u, m);
  return v < m - 1 ? v : m - 1;
}

struct GnLds {
  int idx[GN_ROWS][GN_B + 1];         // the row's successors: in draw order, then sorted by state
  int mkey[GN_ROWS][GN_B + 1];        // the positions >= b a swap step has touched, and what they hold
  int mval[GN_ROWS][GN_B + 1];
  double cut[GN_ROWS][GN_B + 1];      // the sorted cuts, then the CDF entry at each successor
  double piece[GN_ROWS][GN_B + 1];    // the successor's probability
  int perm[GN_S_MAX];
};

// one lane: row r of task k with n real states -> L.idx / L.piece / L.cut of slot `sl`
__device__ void gn_row(const GnArgs& P, GnLds& L, int sl, uint64_t k, int r, int n) {
  const int b = P.b;
  int* idx = L.idx[sl];
  int* mkey = L.mkey[sl];
  int* mval = L.mval[sl];
  double* cut = L.cut[sl];
  double* piece = L.piece[sl];
  // partial Fisher-Yates on arange(n): positions below b live in idx, the others are themselves unless the map has them
  for (int i = 0; i < b; ++i) idx[i] = i;
  int nm = 0;
  double ua = 0.0, ub = 0.0;
  for (int i = 0; i < b; ++i) {
    GN_PAIR(ua, ub, i, xv_index_draw(P.seed, k, (uint32_t)r, GN_P_SUCC, (uint32_t)i >> 1));
    const int j = i + gn_floor(gn_half(ua, ub, i), n - i);
    const int vi = idx[i];
    if (j < b) {
      idx[i] = idx[j];
      idx[j] = vi;
    } else {
      int f = -1;
      for (int t = 0; t < nm; ++t)
        if (mkey[t] == j) f = t;
      idx[i] = f >= 0 ? mval[f] : j;
      if (f < 0) {
        f = nm++;
        mkey[f] = j;
      }
      mval[f] = vi;
    }
  }
  // b - 1 cuts, sorted ascending (insertion), then the pieces between 0, the cuts and 1
  for (int j = 0; j < b - 1; ++j) {
    GN_PAIR(ua, ub, j, xv_index_draw(P.seed, k, (uint32_t)r, GN_P_CUT, (uint32_t)j >> 1));
    const double c = gn_half(ua, ub, j);
    int t = j;
    while (t > 0 && cut[t - 1] > c) {
      cut[t] = cut[t - 1];
      --t;
    }
    cut[t] = c;
  }
  for (int j = 0; j < b; ++j) {
    const double hi = j == b - 1 ? 1.0 : cut[j];
    const double lo = j == 0 ? 0.0 : cut[j - 1];
    piece[j] = hi - lo;
  }
  // by state (insertion on the pairs), then cumsum(row) / cumsum(row)[-1] as numpy.random.choice forms it: the zeros between
  // two successors add nothing, so the running sum changes at the successors only
  for (int j = 1; j < b; ++j) {
    const int ki = idx[j];
    const double kp = piece[j];
    int t = j;
    while (t > 0 && idx[t - 1] > ki) {
      idx[t] = idx[t - 1];
      piece[t] = piece[t - 1];
      --t;
    }
    idx[t] = ki;
    piece[t] = kp;
  }
  double c = 0.0;
  for (int j = 0; j < b; ++j) {
    c += piece[j];
    cut[j] = c;
  }
  const double tot = c;
  for (int j = 0; j < b; ++j) cut[j] = cut[j] / tot;
}

// grid: n_task * chunks workgroups; workgroup (task, chunk) owns rows [GN_ROWS chunk, GN_ROWS (chunk + 1)) of the task's S A
// rows (padded states included: build_tables gives them CDF 1.0 and zero pairs), chunk 0 the task's small vectors as well
__global__ __launch_bounds__(GN_BLOCK) void anymdp_garnet_kernel(GnArgs P) {
  __shared__ GnLds L;
  const int tid = threadIdx.x;
  const int task = (int)(blockIdx.x / (unsigned)P.chunks), chunk = (int)(blockIdx.x % (unsigned)P.chunks);
  const uint64_t k = P.task_base + (uint64_t)task;
  const int S = P.S, A = P.A, SA = S * A;
  const xv_u2 head = xv_pair(xv_index_draw(P.seed, k, 0u, GN_P_HEAD, 0u));
  const int n = P.m + (P.m < S ? gn_floor(head.b, S - P.m + 1) : 0);
  const int row0 = chunk * GN_ROWS;
  const int n_row = SA - row0 < GN_ROWS ? SA - row0 : GN_ROWS;

  if (tid < n_row && (row0 + tid) / A < n) gn_row(P, L, tid, k, row0 + tid, n);
  __syncthreads();

  // ---- the store stream: entry t of this workgroup's rows; 8 entries of 16 bytes per line ----
  const int slots = P.row_lines * 8;
  double2* out = reinterpret_cast<double2*>(P.rows) + ((size_t)task * SA + row0) * (size_t)slots;
  const bool dense = P.transition || P.reward || P.noise;
  for (int t = tid; t < n_row * slots; t += GN_BLOCK) {
    const int rl = t / slots, slot = t - rl * slots;
    const int line = slot >> 3, e = slot & 7;
    double cdf = 0.0, pr = 0.0;      // the fence line and a block's last 16 bytes stay zero: xv_anymdp_create completes them
    if (line > 0 && e < 7) {
      const int j = (line - 1) * 7 + e;
      const int r = row0 + rl;
      if (j >= S) {
        cdf = 2.0;
      } else {
        double tv = 0.0, rw = 0.0;
        if (r / A >= n || j >= n) {
          cdf = 1.0;
        } else {
          for (int c = 0; c < P.b; ++c)
            if (L.idx[rl][c] <= j) {
              cdf = L.cut[rl][c];
              tv = L.idx[rl][c] == j ? L.piece[rl][c] : 0.0;
            }
          const uint32_t q = (uint32_t)r * (uint32_t)n + (uint32_t)j;
          double zc, zs;
#ifdef XV_GARNET_PROBE_UNIFORM      // measurement only (scripts/devtools/build_variant.py): the stream without log / sincos
          const xv_u2 uz = xv_pair(xv_index_draw(P.seed, k, 0u, GN_P_REWARD, q >> 1));
          zc = uz.a;
          zs = uz.b;
#elif defined(XV_GARNET_PROBE_CONST)      // measurement only: nor the Philox call, the stores and the row look-up alone
          zc = zs = 1.0;
#else
          xv_normal2(xv_pair(xv_index_draw(P.seed, k, 0u, GN_P_REWARD, q >> 1)), &zc, &zs);
#endif
          rw = ((q & 1u) ? zs : zc) * P.sigma + 0.0;
          pr = __hiloint2double(0, (int)__float_as_uint((float)rw));      // {reward, reward_noise = 0} as fp32
        }
        if (dense) {
          const size_t o = ((size_t)task * SA + r) * (size_t)S + j;
          if (P.transition) P.transition[o] = tv;
          if (P.reward) P.reward[o] = rw;
          if (P.noise) P.noise[o] = 0.0;
        }
      }
    }
    out[t] = make_double2(cdf, pr);
  }
  if (chunk != 0) return;

  // ---- the task's small vectors ----
  for (int i = tid; i < S; i += GN_BLOCK) L.perm[i] = i;
  __syncthreads();
  if (tid == 0) {      // state_mapping: the first n entries of a forward Fisher-Yates on arange(S), sequential by nature
    const int steps = n < S - 1 ? n : S - 1;
    double ua = 0.0, ub = 0.0;
    for (int i = 0; i < steps; ++i) {
      GN_PAIR(ua, ub, i, xv_index_draw(P.seed, k, 0u, GN_P_PERM, (uint32_t)i >> 1));
      const int j = i + gn_floor(gn_half(ua, ub, i), S - i);
      const int v = L.perm[i];
      L.perm[i] = L.perm[j];
      L.perm[j] = v;
    }
    P.max_steps[task] = (int32_t)ceil(P.lower + (P.upper - P.lower) * head.a);
    P.n_real[task] = n;
  }
  __syncthreads();
  for (int i = tid; i < S; i += GN_BLOCK) P.state_map[(size_t)task * S + i] = i < n ? L.perm[i] : 0;
  const int words = (S + 63) / 64;
  for (int w = tid; w < words; w += GN_BLOCK) P.term_mask[(size_t)task * words + w] = 0;      // nothing terminates
  for (int q = tid; q < P.s0_max; q += GN_BLOCK) {      // s_0 = [0], s_0_prob = [1.0]
    P.s0_cdf[(size_t)task * P.s0_max + q] = 1.0;
    P.s0_ids[(size_t)task * P.s0_max + q] = 0;
  }
}

// ---- bandits: one lane per candidate -------------------------------------------------------------------------------------
constexpr int BD_BLOCK = 64;

struct BdArgs {
  uint64_t seed, cand_base;
  int n_cand, A, max_rounds, s0_max;
  double* rows;
  int32_t* state_map;
  uint64_t* term_mask;
  double* s0_cdf;
  int32_t* s0_ids;
  int32_t* max_steps;
  double* reward;
  double* noise;
  int32_t* status;
};

// numpy's pairwise add.reduce of n <= 128 values f(0) .. f(n - 1) (host_draws.np_sum): below 8 left to right from 0; else
// eight accumulators over the whole blocks of 8, combined pairwise, then the rest in order
template <class F>
__device__ __forceinline__ double bd_np_sum(int n, F f) {
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; ++i) res += f(i);
    return res;
  }
  double r0 = f(0), r1 = f(1), r2 = f(2), r3 = f(3), r4 = f(4), r5 = f(5), r6 = f(6), r7 = f(7);
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
    r0 += f(i); r1 += f(i + 1); r2 += f(i + 2); r3 += f(i + 3);
    r4 += f(i + 4); r5 += f(i + 5); r6 += f(i + 6); r7 += f(i + 7);
  }
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; ++i) res += f(i);
  return res;
}

__global__ __launch_bounds__(BD_BLOCK) void anymdp_bandit_kernel(BdArgs P) {
  __shared__ double s_rw[GN_A_MAX][BD_BLOCK];      // the round's rewards, a lane's column (no per-lane array: no scratch)
  const int tid = threadIdx.x;
  const int ci = (int)blockIdx.x * BD_BLOCK + tid;
  if (ci >= P.n_cand) return;
  const uint64_t cand = P.cand_base + (uint64_t)ci;
  const int A = P.A;
  const xv_u2 head = xv_pair(xv_index_draw(P.seed, cand, 0u, BD_P_HEAD, 0u));
  const double e = xv_expo(head.a);
  const double base = e < 0.05 ? 0.05 : (e > 2.0 ? 2.0 : e);
  const double nb = -0.30 + (0.30 - -0.30) * head.b;
  const double noise_base = nb > 0.0 ? nb : 0.0;
  const double lo = 0.5 * base, span = base - lo;
  int status = 1;
  for (int r = 0; r < P.max_rounds && status != 0; ++r) {
    double ua = 0.0, ub = 0.0;
    for (int a = 0; a < A; ++a) {
      GN_PAIR(ua, ub, a, xv_index_draw(P.seed, cand, (uint32_t)r, BD_P_ROUND, (uint32_t)a >> 1));
      s_rw[a][tid] = lo + span * gn_half(ua, ub, a);
    }
    // numpy.std: the mean from a pairwise sum, the squared deviations, their pairwise sum over the count, the root
    const double mean = bd_np_sum(A, [&](int i) { return s_rw[i][tid]; }) / (double)A;
    const double var = bd_np_sum(A, [&](int i) { const double d = s_rw[i][tid] - mean; return d * d; }) / (double)A;
    if (sqrt(var) > 0.01) status = 0;
  }
  P.status[ci] = status;
  if (status == 0) {
    for (int a = 0; a < A; ++a) {
      if (P.reward) P.reward[(size_t)ci * A + a] = s_rw[a][tid];
      if (P.noise) P.noise[(size_t)ci * A + a] = noise_base * s_rw[a][tid];
    }
  }
  if (status != 0 || P.rows == nullptr) return;
  // build_tables' embedding in two inner states (S = 2: a fence line and one block per row): 0 = the state, 1 = an absorbing
  // terminal copy; row (0, a): cdf {0, 1}, the pair on state 1; row (1, a): cdf {1, 1}; entries past S: 2.0
  double2* out = reinterpret_cast<double2*>(P.rows) + (size_t)ci * 2 * A * 16;
  for (int s = 0; s < 2; ++s)
    for (int a = 0; a < A; ++a) {
      double2* rec = out + ((size_t)s * A + a) * 16;
      const double rw = s_rw[a][tid];
      const double pr = __hiloint2double((int)__float_as_uint((float)(noise_base * rw)), (int)__float_as_uint((float)rw));
      for (int q = 0; q < 8; ++q) rec[q] = make_double2(0.0, 0.0);
      rec[8] = make_double2(s == 0 ? 0.0 : 1.0, 0.0);
      rec[9] = make_double2(1.0, s == 0 ? pr : 0.0);
      for (int q = 10; q < 15; ++q) rec[q] = make_double2(2.0, 0.0);
      rec[15] = make_double2(0.0, 0.0);
    }
  P.state_map[(size_t)ci * 2] = 0;
  P.state_map[(size_t)ci * 2 + 1] = 0;
  P.term_mask[ci] = 2;
  for (int q = 0; q < P.s0_max; ++q) {
    P.s0_cdf[(size_t)ci * P.s0_max + q] = 1.0;
    P.s0_ids[(size_t)ci * P.s0_max + q] = 0;
  }
  P.max_steps[ci] = 1;
}

}  // namespace

extern "C" int xv_anymdp_sample_garnet(xv_engine* e, uint64_t seed, int64_t task_base, int n_task, int S, int A, int min_S,
                                       int b, double sigma, int s0_max, void* rows, int32_t* state_map, uint64_t* term_mask,
                                       double* s0_cdf, int32_t* s0_ids, int32_t* max_steps, int32_t* n_real,
                                       double* transition, double* reward, double* reward_noise) {
  XV_CHECK_ARG(e != nullptr && n_task >= 1 && task_base >= 0 && task_base <= INT64_MAX - n_task);
  XV_CHECK_ARG(rows && state_map && term_mask && s0_cdf && s0_ids && max_steps && n_real);
  XV_CHECK_ARG(s0_max >= 1 && s0_max <= 256);
  if (S < 8 || S > GN_S_MAX || A < 2 || A > GN_A_MAX) {
    xv_set_error("xv_anymdp_sample_garnet: S = %d, A = %d is outside the supported range 8 <= S <= %d, 2 <= A <= %d", S, A,
                 GN_S_MAX, GN_A_MAX);
    return XV_ERR_UNSUPPORTED;
  }
  const int m = min_S <= 0 || min_S > S ? S : min_S;      // min_S <= 0: every task has S real states
  if (m < 8) {
    xv_set_error("xv_anymdp_sample_garnet: min_S = %d is below the minimum of 8", min_S);
    return XV_ERR_UNSUPPORTED;
  }
  if (b < 2 || b > GN_B || b > m) {
    xv_set_error("xv_anymdp_sample_garnet: b = %d is outside the supported range 2 .. min(%d, smallest real state count = %d)",
                 b, GN_B, m);
    return XV_ERR_UNSUPPORTED;
  }
  GnArgs P = GnArgs();
  P.seed = seed; P.task_base = (uint64_t)task_base; P.n_task = n_task; P.S = S; P.A = A; P.m = m; P.b = b; P.s0_max = s0_max;
  P.row_lines = XV_ANYMDP_ROW_LINES(S);
  P.chunks = xv_div_up(S * A, GN_ROWS);
  if ((int64_t)n_task * P.chunks > (int64_t)INT32_MAX) {
    xv_set_error("xv_anymdp_sample_garnet: n_task = %d is more than the %lld tasks of this size one launch takes", n_task,
                 (long long)(INT32_MAX / P.chunks));
    return XV_ERR_UNSUPPORTED;
  }
  P.sigma = sigma;
  P.lower = 4.0 * S > 100.0 ? 4.0 * S : 100.0;
  const double cap = 8.0 * S < 500.0 ? 8.0 * S : 500.0;
  P.upper = cap > P.lower + 1.0 ? cap : P.lower + 1.0;
  P.rows = static_cast<double*>(rows); P.state_map = state_map; P.term_mask = term_mask; P.s0_cdf = s0_cdf;
  P.s0_ids = s0_ids; P.max_steps = max_steps; P.n_real = n_real;
  P.transition = transition; P.reward = reward; P.noise = reward_noise;
  XV_HIP(hipSetDevice(e->device));
  hipLaunchKernelGGL(anymdp_garnet_kernel, dim3((unsigned)(n_task * P.chunks)), dim3(GN_BLOCK), 0, e->stream, P);
  XV_LAUNCH_CHECK();
  return XV_OK;
}

extern "C" int xv_anymdp_sample_bandits(xv_engine* e, uint64_t seed, int64_t cand_base, int n_cand, int A, int max_rounds,
                                        int s0_max, void* rows, int32_t* state_map, uint64_t* term_mask, double* s0_cdf,
                                        int32_t* s0_ids, int32_t* max_steps, double* reward, double* reward_noise,
                                        int32_t* status) {
  XV_CHECK_ARG(e != nullptr && status != nullptr && n_cand >= 1 && n_cand <= (1 << 30));
  XV_CHECK_ARG(cand_base >= 0 && cand_base <= INT64_MAX - n_cand);
  XV_CHECK_ARG(s0_max >= 1 && s0_max <= 256);
  if (rows != nullptr) XV_CHECK_ARG(state_map && term_mask && s0_cdf && s0_ids && max_steps);
  if (A < 2 || A > GN_A_MAX) {
    xv_set_error("xv_anymdp_sample_bandits: A = %d is outside the supported range 2 .. %d", A, GN_A_MAX);
    return XV_ERR_UNSUPPORTED;
  }
  if (max_rounds < 1 || max_rounds > XV_ANYMDP_BANDIT_ROUNDS_MAX) {
    xv_set_error("xv_anymdp_sample_bandits: max_rounds = %d is outside the supported range 1 .. %d", max_rounds,
                 XV_ANYMDP_BANDIT_ROUNDS_MAX);
    return XV_ERR_UNSUPPORTED;
  }
  BdArgs P = BdArgs();
  P.seed = seed; P.cand_base = (uint64_t)cand_base; P.n_cand = n_cand; P.A = A; P.max_rounds = max_rounds; P.s0_max = s0_max;
  P.rows = static_cast<double*>(rows); P.state_map = state_map; P.term_mask = term_mask; P.s0_cdf = s0_cdf;
  P.s0_ids = s0_ids; P.max_steps = max_steps; P.reward = reward; P.noise = reward_noise; P.status = status;
  XV_HIP(hipSetDevice(e->device));
  hipLaunchKernelGGL(anymdp_bandit_kernel, dim3((unsigned)xv_div_up(n_cand, BD_BLOCK)), dim3(BD_BLOCK), 0, e->stream, P);
  XV_LAUNCH_CHECK();
  return XV_OK;
}
