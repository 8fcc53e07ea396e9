// linds_sampler.hip — LinDS tasks made on the device: xv_linds_sample_tasks (generation, the start-state rejection
// search, zero-order-hold discretisation, the tables xv_linds_create consumes) and xv_linds_build_zoh (the
// discretisation alone).  One workgroup per candidate / per task, fp64 throughout, Philox4x32-10 counters.
//
// Reference: xenoverse/linds/task_sampler.py sample_variants_ :12-58 and LinearDSSampler :60-132 (the rejection loop
// :107-132), RandomFourier utils/random_nn.py:346-368, build_dynamics_matrices linds_env.py:67-76.
// The numpy restatement of everything below, draw for draw, is xenoverse_amd/linds/sampler_host.py; the counter layout
// is written down in include/xeno.h.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "xv_common.h"
#include "xv_draws.h"

namespace {

constexpr int LS_T = 128;          // threads per candidate: one start attempt per thread and chunk
constexpr int LS_NS = 32, LS_NA = 16, LS_NO = 32, LS_KMAX = XV_LINDS_KMAX;

// head stream (stream 0): draw indices
constexpr uint32_t H_DIMS = 0, H_DIMS2 = 1, H_SCALE = 2, H_TRIM = 3, H_COST = 4, H_REWARD = 5, H_PUNISH = 6, H_TARGET = 7;
constexpr uint32_t H_AB = 0x1000, H_X = 0x2000, H_C = 0x3000, H_VALID = 0x10000;
constexpr int LS_VALID_ROUNDS = 1 << 16;
// attempt stream (stream 1 + a)
constexpr uint32_t S_BORN = 0, S_CMD = 1, S_ORDER_INT = 2, S_ORDER_Z = 8, S_STATIC = 16, S_FOURIER = 64, S_STATES = 1024;

constexpr int ZOH_TERMS = 18;
constexpr double ZOH_THETA = 0.25;
constexpr int ZOH_S_CAP = 40;

struct LsTables {      // xv_linds_tables, written
  float *phiT, *gamT, *cT, *xt, *y0, *valid, *cmd0, *four_coef;
  double *four_omega, *four_period;
  float* scal;
  int32_t* ints;
  float* init;
};

struct LsArgs {
  uint64_t seed;
  int64_t cand_base;
  int n_cand, random_dim, ns, na, no, NS, NA, NO, NI, max_draws;
  double dt;
  LsTables T;
  xv_linds_dense D;
  xv_linds_cand_info* info;
  int32_t* status;
};

struct LsKey {
  uint32_t c0, c1, k0, k1;
};

// LinDS's own layout: counter = {candidate lo, candidate hi, stream, draw}, key = seed
__device__ __forceinline__ xv_u2 ls_u2(const LsKey& k, uint32_t stream, uint32_t draw) {
  return xv_pair(xv_philox4x32_10(k.c0, k.c1, stream, draw, k.k0, k.k1));
}
__device__ __forceinline__ void ls_pair(const LsKey& k, uint32_t stream, uint32_t draw, double* ua, double* ub) {
  const xv_u2 u = ls_u2(k, stream, draw);
  *ua = u.a;
  *ub = u.b;
}
__device__ __forceinline__ void ls_normal2(const LsKey& k, uint32_t stream, uint32_t draw, double* z0, double* z1) {
  xv_normal2(ls_u2(k, stream, draw), z0, z1);
}

// ------------------------------------------------------------------------------------------------
// zero-order hold of one task by the whole workgroup.  A [n][n], B [n][na] in LDS; W: 5 n^2 + n na doubles of LDS.
// M = A h, h = dt / 2^s with |M|_inf <= 0.25; P = sum_{k<18} M^k / (k+1)! by Horner; S = h P; Phi = I + M P; s doublings
// S <- S + Phi S, Phi <- Phi Phi; Gamma = S B.  Every product sums k = 0, 1, ... in order with a separate multiply and add
// (the file is built with -ffp-contract=off), so a task's bits do not depend on its batch.
// Returns the status (0 ok, 1 non-finite, 2 scale cap); *phi / *gam point into W.
// ------------------------------------------------------------------------------------------------
struct ZohShared {
  int status, s;
  double h;
  int bad;
};

__device__ int ls_zoh_block(int n, int na, const double* A, const double* B, double dt, double* W, ZohShared* sh,
                            const double** phi, const double** gam, int* s_out) {
  const int tid = threadIdx.x, nt = blockDim.x, nn = n * n;
  if (tid == 0) {
    bool fin = isfinite(dt);
    double norm = 0.0;
    for (int i = 0; i < n; ++i) {
      double row = 0.0;
      for (int j = 0; j < n; ++j) {
        const double a = A[i * n + j];
        fin = fin && isfinite(a);
        row = row + fabs(a);
      }
      norm = fmax(norm, row);
    }
    for (int i = 0; i < n * na; ++i) fin = fin && isfinite(B[i]);
    int st = 0, s = 0;
    if (!fin) {
      st = 1;
    } else {
      norm = norm * fabs(dt);
      while (norm > ZOH_THETA && s <= ZOH_S_CAP) {
        norm = norm * 0.5;
        ++s;
      }
      if (s > ZOH_S_CAP) st = 2;
    }
    sh->status = st;
    sh->s = s;
    sh->h = st ? 0.0 : ldexp(dt, -s);
    sh->bad = 0;
  }
  __syncthreads();
  const int st0 = sh->status, s = sh->s;
  const double h = sh->h;
  *s_out = s;
  if (st0) return st0;
  double* M = W;
  double* P = W + nn;
  double* Q = W + 2 * nn;
  double* S = W + 3 * nn;
  double* F = W + 4 * nn;
  double* G = W + 5 * nn;
  for (int idx = tid; idx < nn; idx += nt) {
    M[idx] = A[idx] * h;
    P[idx] = (idx / n == idx % n) ? 1.0 : 0.0;
  }
  __syncthreads();
  for (int k = ZOH_TERMS; k > 1; --k) {
    for (int idx = tid; idx < nn; idx += nt) {
      const int i = idx / n, j = idx % n;
      double acc = 0.0;
      for (int q = 0; q < n; ++q) acc = acc + M[i * n + q] * P[q * n + j];
      Q[idx] = (i == j ? 1.0 : 0.0) + acc / (double)k;
    }
    __syncthreads();
    double* t = P; P = Q; Q = t;
  }
  for (int idx = tid; idx < nn; idx += nt) {
    const int i = idx / n, j = idx % n;
    double acc = 0.0;
    for (int q = 0; q < n; ++q) acc = acc + M[i * n + q] * P[q * n + j];
    S[idx] = P[idx] * h;
    F[idx] = (i == j ? 1.0 : 0.0) + acc;
  }
  __syncthreads();
  double* S2 = M;      // M, P, Q are free from here on
  double* F2 = Q;
  for (int r = 0; r < s; ++r) {
    for (int idx = tid; idx < nn; idx += nt) {
      const int i = idx / n, j = idx % n;
      double a1 = 0.0, a2 = 0.0;
      for (int q = 0; q < n; ++q) {
        const double f = F[i * n + q];
        a1 = a1 + f * S[q * n + j];
        a2 = a2 + f * F[q * n + j];
      }
      S2[idx] = S[idx] + a1;
      F2[idx] = a2;
    }
    __syncthreads();
    double* t = S; S = S2; S2 = t;
    t = F; F = F2; F2 = t;
  }
  int bad = 0;
  for (int idx = tid; idx < n * na; idx += nt) {
    const int i = idx / na, j = idx % na;
    double acc = 0.0;
    for (int q = 0; q < n; ++q) acc = acc + S[i * n + q] * B[q * na + j];
    G[idx] = acc;
    bad |= !isfinite(acc);
  }
  for (int idx = tid; idx < nn; idx += nt) bad |= !isfinite(F[idx]);
  if (bad) atomicOr(&sh->bad, 1);
  __syncthreads();
  *phi = F;
  *gam = G;
  return sh->bad ? 1 : 0;
}

// fp32 table slots of one task from Phi / Gamma (or zeros on a failed task: never a NaN table)
__device__ void ls_write_zoh(int n, int na, int NS, int NA, const double* phi, const double* gam, bool ok, float* phiT,
                             float* gamT, double* phi64, double* gam64) {
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int idx = tid; idx < NS * NS; idx += nt) {
    const int k = idx / NS, j = idx % NS;      // phiT[k][j] = Phi[j][k]
    const double v = (ok && k < n && j < n) ? phi[j * n + k] : 0.0;
    phiT[idx] = (float)v;
    if (phi64) phi64[j * NS + k] = v;
  }
  for (int idx = tid; idx < NA * NS; idx += nt) {
    const int k = idx / NS, j = idx % NS;      // gamT[k][j] = Gamma[j][k]
    const double v = (ok && k < na && j < n) ? gam[j * na + k] : 0.0;
    gamT[idx] = (float)v;
    if (gam64) gam64[j * NA + k] = v;
  }
}

__global__ __launch_bounds__(256) void linds_zoh_kernel(int n_task, const int32_t* ns_of, int NS, int NA, const double* A,
                                                         const double* B, const double* X, double dt, float* phiT,
                                                         float* gamT, float* xt, double* phi64, double* gam64,
                                                         int32_t* status) {
  extern __shared__ double lds[];
  __shared__ ZohShared sh;
  const int t = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  if (t >= n_task) return;
  int n = ns_of[t];
  const bool dims_ok = n >= 1 && n <= NS;
  if (!dims_ok) n = 1;
  double* a = lds;                  // [n][n]
  double* b = lds + NS * NS;        // [n][NA]
  double* W = b + NS * NA;
  for (int idx = tid; idx < n * n; idx += nt) a[idx] = A[(size_t)t * NS * NS + (idx / n) * NS + idx % n];
  for (int idx = tid; idx < n * NA; idx += nt) b[idx] = B[(size_t)t * NS * NA + idx];
  __syncthreads();
  const double *phi = nullptr, *gam = nullptr;
  int s = 0;
  int st = ls_zoh_block(n, NA, a, b, dt, W, &sh, &phi, &gam, &s);
  if (!dims_ok) st = 1;
  ls_write_zoh(n, NA, NS, NA, phi, gam, st == 0, phiT + (size_t)t * NS * NS, gamT + (size_t)t * NA * NS,
               phi64 ? phi64 + (size_t)t * NS * NS : nullptr, gam64 ? gam64 + (size_t)t * NS * NA : nullptr);
  for (int j = tid; j < NS; j += nt) {
    const double v = (st == 0 && j < n) ? X[(size_t)t * NS + j] * dt : 0.0;
    xt[(size_t)t * NS + j] = (float)(isfinite(v) ? v : 0.0);
    if (st == 0 && j < n && !isfinite(v)) status[t] = 1;
  }
  if (tid == 0 && st != 0) status[t] = st;
}

// ------------------------------------------------------------------------------------------------
// the candidate's head in LDS
// ------------------------------------------------------------------------------------------------
struct LsHead {
  int ns, na, no, max_steps, a_scale, x_scale, trim, width, type, valid_rounds;
  double action_cost, reward_base, terminate_punish, reward_factor, eps;
};

struct LsStart {      // what a start attempt decides besides its arrays
  int born, delay, n_terms;
  double noise_drift;
};

// One start attempt, evaluated by one thread.  xs / cm are the thread's LDS columns (element j at [j * LS_T]).
// W: the winning attempt is evaluated once more by thread 0 and written out.
template <bool W>
__device__ bool ls_attempt(const LsArgs& P, const LsKey& key, const LsHead& H, const double* C, const double* tv, int a,
                           double* xs, double* cm, int ci, LsStart* out) {
  const uint32_t stream = 1u + (uint32_t)a;
  const int ns = H.ns, no = H.no;
  double ua, ub;
  ls_pair(key, stream, S_BORN, &ua, &ub);
  const double e = xv_expo(ua);
  const int born = (int)fmax(e, 1.0);
  if (born > P.NI) return false;
  const double nd = fmin(fmax(-0.02 + 0.04 * ub, 0.0), 0.02);
  ls_pair(key, stream, S_CMD, &ua, &ub);
  int delay = 0, n_terms = 0;
  if (H.type == 0) {
    const double gate = (double)xv_floor_int(ua, 2);
    for (int p = 0; 2 * p < no; ++p) {
      double z0, z1;
      ls_normal2(key, stream, S_STATIC + p, &z0, &z1);
      cm[(2 * p) * LS_T] = z0 * gate;
      if (2 * p + 1 < no) cm[(2 * p + 1) * LS_T] = z1 * gate;
    }
    if (W) {
      for (int o = 0; o < no; ++o) {
        const double v = cm[o * LS_T];
        if (P.T.cmd0) P.T.cmd0[(size_t)ci * P.NO + o] = (float)v;
        if (P.D.cmd0) P.D.cmd0[(size_t)ci * P.NO + o] = v;
      }
      if (P.T.four_period) P.T.four_period[ci] = 1.0;
    }
  } else {
    const int n_items = 1 + xv_floor_int(ua, 5);
    delay = max(-10 + xv_floor_int(ub, 40), 0);
    n_terms = 1 + n_items;
    const double scale = 2.0 / sqrt((double)n_items);
    const double x = -(double)delay / 1000.0;
    for (int o = 0; o < no; ++o) cm[o * LS_T] = 0.0;
    for (int t = 0; t <= n_items; ++t) {
      double order = 0.0;
      if (t > 0) {
        double oa, ob, z0, z1;
        ls_pair(key, stream, S_ORDER_INT + t, &oa, &ob);
        ls_normal2(key, stream, S_ORDER_Z + t, &z0, &z1);
        order = (double)(1 + xv_floor_int(oa, 16)) + z0;
      }
      const double ang = order * x;
      const double sn = sin(ang), cs = cos(ang);
      if (W) {
        if (P.T.four_omega) P.T.four_omega[(size_t)ci * LS_KMAX + t] = order;
        if (P.D.four_order) P.D.four_order[(size_t)ci * LS_KMAX + t] = order;
      }
      for (int o = 0; o < no; ++o) {
        double z0, z1, ea, eb;
        ls_normal2(key, stream, S_FOURIER + 64 * t + o, &z0, &z1);
        ls_pair(key, stream, S_FOURIER + 64 * t + 32 + o, &ea, &eb);
        const double c0 = z0 * (xv_expo(ea) * scale), c1 = z1 * (xv_expo(eb) * scale);
        const double term = c0 * sn + c1 * cs;
        cm[o * LS_T] = cm[o * LS_T] + term;
        if (W) {
          const size_t at = (((size_t)ci * LS_KMAX + t) * P.NO + o) * 2;
          if (P.T.four_coef) { P.T.four_coef[at] = (float)c0; P.T.four_coef[at + 1] = (float)c1; }
          if (P.D.four_coef) { P.D.four_coef[at] = c0; P.D.four_coef[at + 1] = c1; }
        }
      }
    }
    if (W && P.T.four_period) P.T.four_period[ci] = 1000.0;
  }
  for (int i = 0; i < born; ++i) {
    double x2 = 0.0;
    for (int p = 0; 2 * p < ns; ++p) {
      double z0, z1;
      ls_normal2(key, stream, S_STATES + 16 * i + p, &z0, &z1);
      xs[(2 * p) * LS_T] = z0;
      x2 = x2 + z0 * z0;
      if (2 * p + 1 < ns) {
        xs[(2 * p + 1) * LS_T] = z1;
        x2 = x2 + z1 * z1;
      }
    }
    if (sqrt(x2) > 10.0) return false;
    double dev2 = 0.0;
    for (int o = 0; o < no; ++o) {
      double y = 0.0;
      for (int j = 0; j < ns; ++j) y = y + C[o * ns + j] * xs[j * LS_T];
      const double d = (cm[o * LS_T] - y) * tv[o];      // ld_Y = 0
      dev2 = dev2 + d * d;
    }
    if (sqrt(dev2) > 3.0) return false;
    if (W) {
      for (int j = 0; j < ns; ++j) {
        const double v = xs[j * LS_T];
        if (P.T.init) P.T.init[((size_t)ci * P.NI + i) * P.NS + j] = (float)v;
        if (P.D.init) P.D.init[((size_t)ci * P.NI + i) * P.NS + j] = v;
      }
    }
  }
  if (W) {
    out->born = born;
    out->delay = delay;
    out->n_terms = n_terms;
    out->noise_drift = nd;
  }
  return true;
}

__global__ __launch_bounds__(LS_T) void linds_sampler_kernel(LsArgs P) {
  extern __shared__ double lds[];
  __shared__ LsHead H;
  __shared__ ZohShared zsh;
  __shared__ int sh_win, sh_sum;
  const int ci = blockIdx.x, tid = threadIdx.x;
  if (ci >= P.n_cand) return;
  const uint64_t cand = (uint64_t)(P.cand_base + ci);
  const LsKey key{(uint32_t)cand, (uint32_t)(cand >> 32), (uint32_t)P.seed, (uint32_t)(P.seed >> 32)};

  // ---- head scalars (thread 0), reference sample_variants_ and LinearDSSampler :86-105 ----
  if (tid == 0) {
    double ua[8], ub[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) ls_pair(key, 0u, (uint32_t)d, &ua[d], &ub[d]);
    int ns = P.ns, na = P.na, no = P.no;
    if (P.random_dim) {      // LinearDSSamplerRandomDim :134-154; P.ns / na / no are the maxima
      ns = 1 + xv_floor_int(ua[H_DIMS], P.ns);
      const int min_na = max(1, (ns + 1) / 2), hi_na = max(min(P.na, ns * 3 / 2), min_na);
      const int min_no = max(1, ns / 4), hi_no = max(min(P.no, ns * 3 / 2), min_no);
      na = min_na + xv_floor_int(ub[H_DIMS], hi_na - min_na + 1);
      no = min_no + xv_floor_int(ua[H_DIMS2], hi_no - min_no + 1);
    }
    H.ns = ns; H.na = na; H.no = no;
    H.max_steps = 100 + xv_floor_int(ub[H_DIMS2], 900);
    H.a_scale = xv_floor_int(ua[H_SCALE], 5);
    H.x_scale = xv_floor_int(ub[H_SCALE], 3);
    H.trim = xv_floor_int(ua[H_TRIM], 3);
    H.width = H.trim == 0 ? 2 + xv_floor_int(ub[H_TRIM], max(ns / 2, 3) - 1)
                          : (H.trim == 1 ? -1 + xv_floor_int(ub[H_TRIM], max(ns / 4, 2) + 2) : 0);
    H.action_cost = fmax((-1.0 + 2.0 * ua[H_COST]) * (xv_expo(ub[H_COST]) * 0.05), 0.0);
    H.reward_base = xv_expo(ua[H_REWARD]) * 0.10;
    H.terminate_punish = (xv_expo(ub[H_REWARD]) * 5.0) * (xv_floor_int(ua[H_PUNISH], 3) == 0 ? 0.0 : 1.0);
    H.reward_factor = xv_expo(ub[H_PUNISH]) * 0.50;
    H.eps = fmin(0.2 + ua[H_TARGET], 1.0);
    H.type = xv_floor_int(ub[H_TARGET], 3) < 2 ? 1 : 0;
  }
  __syncthreads();
  const int ns = H.ns, na = H.na, no = H.no;
  double* hA = lds;                          // [ns][ns]
  double* hB = hA + LS_NS * LS_NS;           // [ns][na]
  double* hC = hB + LS_NS * LS_NA;           // [no][ns]
  double* hX = hC + LS_NO * LS_NS;           // [ns]
  double* tv = hX + LS_NS;                   // [no]
  double* work = tv + LS_NO;                 // the search's columns, then the ZOH's matrices

  // ---- target_valid: redrawn while its sum is 0 ----
  int rounds = 0;
  for (int r = 0; r < LS_VALID_ROUNDS; ++r) {
    if (tid == 0) sh_sum = 0;
    __syncthreads();
    if (tid < no) {
      double ua, ub;
      ls_pair(key, 0u, H_VALID + 16u * (uint32_t)r + (uint32_t)(tid >> 1), &ua, &ub);
      const int v = ((tid & 1) ? ub : ua) < H.eps ? 1 : 0;
      tv[tid] = (double)v;
      if (v) atomicAdd(&sh_sum, 1);
    }
    __syncthreads();
    rounds = r + 1;
    const int sum = sh_sum;
    __syncthreads();
    if (sum > 0) break;
  }

  // ---- Xavier-normal AB, X, C with gain 3; the scales and the trim touch A only ----
  {
    const int wab = ns + na, nab = ns * wab;
    const double std_ab = sqrt(2.0 / (double)(2 * ns + na)), std_c = sqrt(2.0 / (double)(ns + no));
    const double asc = H.a_scale == 0 ? 0.01 : H.a_scale == 1 ? 0.02 : H.a_scale == 2 ? 0.05 : H.a_scale == 3 ? 0.1 : 0.2;
    const double xsc = H.x_scale == 0 ? 0.0 : H.x_scale == 1 ? 0.05 : 0.1;
    for (int p = tid; 2 * p < nab; p += LS_T) {
      double z[2];
      ls_normal2(key, 0u, H_AB + (uint32_t)p, &z[0], &z[1]);
      for (int m = 0; m < 2; ++m) {
        const int n = 2 * p + m;
        if (n >= nab) break;
        const int i = n / wab, j = n % wab;
        const double w = z[m] * std_ab * 3.0;
        if (j < ns) {
          double v = w * asc;
          if (H.trim == 0 && H.width < ns && abs(i - j) > H.width) v = 0.0;
          if (H.trim == 1 && H.width < ns && j < i + H.width) v = 0.0;
          hA[i * ns + j] = v;
        } else {
          hB[i * na + (j - ns)] = w;
        }
      }
    }
    for (int p = tid; 2 * p < ns; p += LS_T) {
      double z[2];
      ls_normal2(key, 0u, H_X + (uint32_t)p, &z[0], &z[1]);
      hX[2 * p] = (0.1 * z[0]) * xsc;
      if (2 * p + 1 < ns) hX[2 * p + 1] = (0.1 * z[1]) * xsc;
    }
    for (int p = tid; 2 * p < no * ns; p += LS_T) {
      double z[2];
      ls_normal2(key, 0u, H_C + (uint32_t)p, &z[0], &z[1]);
      hC[2 * p] = z[0] * std_c * 3.0;
      if (2 * p + 1 < no * ns) hC[2 * p + 1] = z[1] * std_c * 3.0;
    }
  }
  __syncthreads();

  // ---- start search: chunks of LS_T attempts, the lowest passing index wins ----
  double* xs = work + tid;                       // [ns] at stride LS_T
  double* cm = work + P.ns * LS_T + tid;         // [no] at stride LS_T (P.ns: the largest ns of the launch)
  int win = INT_MAX;
  for (int base = 0; base < P.max_draws; base += LS_T) {
    if (tid == 0) sh_win = INT_MAX;
    __syncthreads();
    const int a = base + tid;
    if (a < P.max_draws && ls_attempt<false>(P, key, H, hC, tv, a, xs, cm, ci, nullptr)) atomicMin(&sh_win, a);
    __syncthreads();
    win = sh_win;
    __syncthreads();
    if (win != INT_MAX) break;
  }
  const bool found = win != INT_MAX;

  // ---- info record, dense head ----
  xv_linds_cand_info* inf = P.info ? P.info + ci : nullptr;
  if (tid == 0 && inf) {
    inf->status = found ? 0 : 1;
    inf->attempt = found ? win : -1;
    inf->ns = ns; inf->na = na; inf->no = no;
    inf->a_scale = H.a_scale; inf->x_scale = H.x_scale; inf->trim = H.trim; inf->width = H.width;
    inf->max_steps = H.max_steps;
    inf->n_init = 0; inf->n_terms = 0; inf->delay = 0;
    inf->type = H.type;
    inf->valid_rounds = rounds;
    inf->zoh_s = 0;
    for (int o = 0; o < 32; ++o) inf->target_valid[o] = (o < no && tv[o] != 0.0) ? 1 : 0;
    inf->action_cost = H.action_cost; inf->reward_base = H.reward_base;
    inf->terminate_punish = H.terminate_punish; inf->reward_factor = H.reward_factor;
    inf->noise_drift = 0.0;
    inf->eps = H.eps;
  }
  if (P.D.A) {
    for (int idx = tid; idx < ns * ns; idx += LS_T) P.D.A[(size_t)ci * P.NS * P.NS + (idx / ns) * P.NS + idx % ns] = hA[idx];
    for (int idx = tid; idx < ns * na; idx += LS_T) P.D.B[(size_t)ci * P.NS * P.NA + (idx / na) * P.NA + idx % na] = hB[idx];
    for (int idx = tid; idx < no * ns; idx += LS_T) P.D.C[(size_t)ci * P.NO * P.NS + (idx / ns) * P.NS + idx % ns] = hC[idx];
    for (int j = tid; j < ns; j += LS_T) P.D.X[(size_t)ci * P.NS + j] = hX[j];
    for (int o = tid; o < no; o += LS_T) P.D.Y[(size_t)ci * P.NO + o] = 0.0;
  }
  if (!found) {
    if (tid == 0) P.status[ci] = 1;
    return;
  }

  // ---- the winning attempt once more, written out ----
  __shared__ LsStart start;
  if (tid == 0) (void)ls_attempt<true>(P, key, H, hC, tv, win, xs, cm, ci, &start);
  __syncthreads();      // the search's columns are free from here on

  // ---- zero-order hold and the tables ----
  const double *phi = nullptr, *gam = nullptr;
  int zs = 0;
  const int zst = ls_zoh_block(ns, na, hA, hB, P.dt, work, &zsh, &phi, &gam, &zs);
  if (P.T.phiT) {
    ls_write_zoh(ns, na, P.NS, P.NA, phi, gam, zst == 0, P.T.phiT + (size_t)ci * P.NS * P.NS,
                 P.T.gamT + (size_t)ci * P.NA * P.NS, P.D.phi ? P.D.phi + (size_t)ci * P.NS * P.NS : nullptr,
                 P.D.gam ? P.D.gam + (size_t)ci * P.NS * P.NA : nullptr);
    for (int idx = tid; idx < ns * no; idx += LS_T) {
      const int k = idx / no, o = idx % no;      // cT[k][o] = C[o][k]
      P.T.cT[((size_t)ci * P.NS + k) * P.NO + o] = (float)hC[o * ns + k];
    }
    for (int j = tid; j < ns; j += LS_T) P.T.xt[(size_t)ci * P.NS + j] = (float)(hX[j] * P.dt);
    for (int o = tid; o < no; o += LS_T) {
      P.T.y0[(size_t)ci * P.NO + o] = 0.0f;
      P.T.valid[(size_t)ci * P.NO + o] = (float)tv[o];
    }
    if (tid == 0) {
      float* sc = P.T.scal + (size_t)ci * 8;
      sc[0] = (float)H.action_cost; sc[1] = (float)H.reward_base; sc[2] = (float)H.terminate_punish;
      sc[3] = (float)H.reward_factor; sc[4] = (float)(start.noise_drift * P.dt); sc[5] = (float)P.dt;
      sc[6] = 0.0f; sc[7] = 0.0f;
      int32_t* it = P.T.ints + (size_t)ci * 4;
      it[0] = H.max_steps; it[1] = start.delay; it[2] = start.born; it[3] = start.n_terms;
    }
  }
  if (tid == 0) {
    if (inf) {
      inf->status = zst == 0 ? 0 : 2;
      inf->n_init = start.born; inf->n_terms = start.n_terms; inf->delay = start.delay;
      inf->noise_drift = start.noise_drift;
      inf->zoh_s = zs;
    }
    P.status[ci] = zst == 0 ? 0 : 2;
  }
}

constexpr size_t LS_HEAD_DOUBLES = LS_NS * LS_NS + LS_NS * LS_NA + LS_NO * LS_NS + LS_NS + LS_NO;

}  // namespace

#ifndef XV_KERNELS_ONLY

extern "C" int xv_linds_sample_tasks(xv_engine* e, uint64_t seed, int64_t cand_base, int n_cand, int random_dim, int ns,
                                     int na, int no, int NS, int NA, int NO, int NI, double dt, int64_t max_draws,
                                     const xv_linds_tables* tables, const xv_linds_dense* dense,
                                     xv_linds_cand_info* info, int32_t* status) {
  XV_CHECK_ARG(e != nullptr && status != nullptr);
  XV_CHECK_ARG(n_cand > 0 && cand_base >= 0);
  XV_CHECK_ARG(NS >= 1 && NS <= LS_NS && NA >= 1 && NA <= LS_NA && NO >= 1 && NO <= LS_NO && NI >= 1 && NI <= 64);
  XV_CHECK_ARG(ns >= 1 && na >= 1 && no >= 1 && ns <= NS);
  if (random_dim) {      // the dims LinearDSSamplerRandomDim can draw from these maxima must fit the pads
    XV_CHECK_ARG(ns >= 2 && NA >= na && NA >= (ns + 1) / 2 && NO >= no && NO >= ns / 4);
  } else {
    XV_CHECK_ARG(na <= NA && no <= NO);
  }
  XV_CHECK_ARG(max_draws >= 1 && max_draws <= (int64_t)1 << 30);
  XV_CHECK_ARG(dt == dt);
  if (tables != nullptr)
    XV_CHECK_ARG(tables->phiT && tables->gamT && tables->cT && tables->xt && tables->y0 && tables->valid && tables->cmd0 &&
                 tables->four_coef && tables->four_omega && tables->four_period && tables->scal && tables->ints &&
                 tables->init);
  if (dense != nullptr)
    XV_CHECK_ARG(dense->A && dense->B && dense->C && dense->X && dense->Y && dense->init && dense->phi && dense->gam &&
                 dense->four_order && dense->four_coef && dense->cmd0 && tables != nullptr);
  XV_HIP(hipSetDevice(e->device));
  LsArgs P{};
  P.seed = seed; P.cand_base = cand_base; P.n_cand = n_cand; P.random_dim = random_dim ? 1 : 0;
  P.ns = ns; P.na = na; P.no = no; P.NS = NS; P.NA = NA; P.NO = NO; P.NI = NI; P.max_draws = (int)max_draws; P.dt = dt;
  if (tables) {
    P.T.phiT = const_cast<float*>(tables->phiT); P.T.gamT = const_cast<float*>(tables->gamT);
    P.T.cT = const_cast<float*>(tables->cT); P.T.xt = const_cast<float*>(tables->xt);
    P.T.y0 = const_cast<float*>(tables->y0); P.T.valid = const_cast<float*>(tables->valid);
    P.T.cmd0 = const_cast<float*>(tables->cmd0); P.T.four_coef = const_cast<float*>(tables->four_coef);
    P.T.four_omega = const_cast<double*>(tables->four_omega); P.T.four_period = const_cast<double*>(tables->four_period);
    P.T.scal = const_cast<float*>(tables->scal); P.T.ints = const_cast<int32_t*>(tables->ints);
    P.T.init = const_cast<float*>(tables->init);
  }
  if (dense) P.D = *dense;
  P.info = info; P.status = status;
  const size_t search = (size_t)(ns + NO) * LS_T, zoh = (size_t)5 * ns * ns + (size_t)ns * NA;      // ns: the launch's largest
  const size_t lds = sizeof(double) * (LS_HEAD_DOUBLES + (search > zoh ? search : zoh));
  XV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&linds_sampler_kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(linds_sampler_kernel, dim3(n_cand), dim3(LS_T), lds, e->stream, P);
  XV_LAUNCH_CHECK();
  return XV_OK;
}

extern "C" int xv_linds_build_zoh(xv_engine* e, int n_task, const int32_t* ns, int NS, int NA, const double* A,
                                  const double* B, const double* X, double dt, float* phiT, float* gamT, float* xt,
                                  double* phi, double* gam, int32_t* status) {
  XV_CHECK_ARG(e != nullptr && n_task > 0 && ns && A && B && X && phiT && gamT && xt && status);
  XV_CHECK_ARG(NS >= 1 && NS <= LS_NS && NA >= 1 && NA <= LS_NA);
  XV_HIP(hipSetDevice(e->device));
  XV_HIP(hipMemsetAsync(status, 0, sizeof(int32_t) * (size_t)n_task, e->stream));
  const size_t lds = sizeof(double) * ((size_t)6 * NS * NS + 2 * (size_t)NS * NA);
  if (lds > 48 * 1024)
    XV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&linds_zoh_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds));
  hipLaunchKernelGGL(linds_zoh_kernel, dim3(n_task), dim3(256), lds, e->stream, n_task, ns, NS, NA, A, B, X, dt, phiT, gamT,
                     xt, phi, gam, status);
  XV_LAUNCH_CHECK();
  return XV_OK;
}

#endif  // XV_KERNELS_ONLY
