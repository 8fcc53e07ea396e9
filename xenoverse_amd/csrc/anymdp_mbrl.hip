// anymdp_mbrl.hip — model-based agents on the device: the reference's AnyMDPSolverMBRL (xenoverse/anymdp/anymdp_solver_mbrl.py)
// for every env of an xv_anymdp handle, one agent per env, driven by the reference's training loop (anymdp/test_utils.py:
// epoch_run :42-60: policy -> step -> learner, reset on done) with SAME_STEP auto-reset.  Host restatement and the full
// statement of the semantics: xenoverse_amd/anymdp/mbrl.py.  Per agent, in fp64 (states are observations):
//   learner :57-71           cnt = vis_cnt[s,a,ns]; est_r[s,a,ns] = (est_r[s,a,ns] cnt + r) / (cnt + 1); vis_cnt[s,a,ns] += 1;
//                            vis_cnt_sa[s,a] += 1; terminated: vis_cnt[ns] = est_r[ns] = 0; terminated or truncated: estimator
//   update_estimator :42-55  t = vis_cnt / clip(rowsum(vis_cnt), 0.01); b = (_c max(np.std(est_r), 0.01)) / sqrt(vis_cnt_sa);
//                            ONE in-place Gauss-Seidel sweep of vm (solver.py update_value_matrix, max_iteration = 1)
//   policy :73-78            the first argmax of vm[o] (greedy) or of vm[o] + b[o] u
// Everything is + - * / sqrt max in numpy's order and the build keeps -ffp-contract=off: bit for bit the host's.  Row sums
// are numpy's pairwise sum of a length-S row; np.std of the whole [S][A][S] tensor runs in chunks of 8192 elements, each
// pairwise-summed, the chunks added in order (mbrl.py: np_tensor_std).  The learner learns from the step's fp32 reward
// widened to fp64 (the reference's is fp64).
//
// Layout: agent state in HBM, per env contiguous — est_r and vis_cnt fp64 [N][S][A][S], vis_cnt_sa, vm and b fp64 [N][S][A],
// the observation the env's last action was chosen from int32 [N].  A rollout issues from C, per step, the existing step
// launch and then two launches:
//   learn      one lane per env: the scattered update; envs whose episode goes on pick their next action; envs whose episode
//              ended go on a device-side list (atomic counter, no host sync)
//   estimator  one wave per listed env (a grid-stride loop over the list, so the list's order does not matter): zero the
//              terminal slabs; the mean and squared-deviation sums of est_r; b; the sweep; the policy from the new observation
// The sweep, row s: lanes over actions form the row sums of vis_cnt; all lanes form the products
// t[s,a,sn] (gamma max(vm[sn]) + r[s,a,sn]) for every (a, sn) into LDS; lanes over actions sum the prefix sn < s; then each
// action in turn, wave-uniform, continues its chain through the term of sn = s (which reads max(vm[s]) as the actions before
// it moved it) and the suffix sn > s.  The policy draws are Philox purpose 7 keyed by (engine seed, global env id, the launch
// tick of the step that takes the action, sub = a >> 1), so results do not depend on how T is split or envs are sharded.
#define XV_KERNELS_ONLY
#include "anymdp.hip"
#undef XV_KERNELS_ONLY
#include "anymdp_learner.h"

#define XV_DRAW_MBRL_POLICY 7u   // sub = a >> 1: words 0,1 (a even) or 2,3 (a odd) -> the policy's uniform u[a]
#define MBRL_CHUNK 8192          // numpy's ufunc buffer: a whole-array sum runs over chunks of this many elements
#define MBRL_LEAVES 128          // leaves of one chunk's pairwise tree (64..128 elements each above 128): at most 8192 / 64
#define MBRL_OPS 256             // the tree's postfix program: its leaves and one add fewer
#define MBRL_STACK 16            // the program's stack (depth <= 8)
#define MBRL_WAVE 64
#define MBRL_LDS_MAX (64 * 1024)

// a pairwise tree as leaf offsets and a postfix program (op >= 0: push the sum of leaf op; op < 0: add the two on top)
struct MBRLTree {
  int n_leaves, n_ops;
  int leaf_off[MBRL_LEAVES + 1];
  int16_t ops[MBRL_OPS];
};
struct MBRLPlan {
  MBRLTree tree[3];      // 0: a full chunk of the tensor, 1: its last partial chunk (may be empty), 2: a row of S
  int n_full, has_tail;
};

struct xv_anymdp_mbrl {
  xv_anymdp* h;        // borrowed: must outlive the learner
  int device;
  double gamma, c, cc;     // cc = c / (1 - gamma): the reference's _c
  int n_env, S, A;
  double* est_r;       // [n_env][S][A][S]
  double* vis_cnt;     // [n_env][S][A][S]
  double* vis_cnt_sa;  // [n_env][S][A]
  double* vm;          // [n_env][S][A]
  double* b;           // [n_env][S][A]
  int32_t* cur_obs;    // [n_env]
  int32_t* term_ns;    // [n_env] the terminal state of the step just learned, -1: none
  int32_t* list;       // [n_env] envs whose episode ended this step
  uint32_t* count;     // [2] list lengths; the learn launch of a step clears the other one
  int parity;
  MBRLPlan* plan;      // device copy
  double* scratch;     // [grid][A][S] the row's products when they do not fit LDS, else nullptr
  int grid;            // estimator workgroups (one wave each)
  size_t lds;          // estimator LDS bytes
  int u_per_env() const { return A; }   // the policy's uniforms per env and step: one per action
};

struct MBArgs {
  double* est_r;
  double* vis_cnt;
  double* vis_cnt_sa;
  double* vm;
  double* b;
  int32_t* cur_obs;
  int32_t* term_ns;
  int32_t* list;
  uint32_t* count;        // this step's list
  uint32_t* count_next;   // the next step's (cleared by the learn launch)
  const MBRLPlan* plan;
  double* scratch;
  double gamma, cc;
  XvLearnerBind B;
};

// policy() :73-78 of env i from observation o: the first argmax of vm[o] (greedy) or of vm[o] + b[o] u
template <bool INJECT>
__device__ int mbrl_policy(const MBArgs& L, const XvLearnStepIO& io, int i, int o) {
  const size_t row = ((size_t)i * L.B.S + o) * L.B.A;
  const uint64_t tick = xv_launch_tick(L.B.tick, L.B.tick_dev);
  int best = 0;
  double m = 0.0;
  xv_u32x4 w{0u, 0u, 0u, 0u};
  for (int k = 0; k < L.B.A; ++k) {
    double v = L.vm[row + k];
    if (!io.greedy) {
      double u;
      if (INJECT) {
        u = io.u_policy[(size_t)i * L.B.A + k];
      } else {
        if ((k & 1) == 0)
          w = xv_env_draw_sub(L.B.seed, L.B.gid_base + (uint64_t)i, tick, XV_DRAW_MBRL_POLICY, (uint32_t)(k >> 1));
        u = (k & 1) ? xv_u53(w.z, w.w) : xv_u53(w.x, w.y);
      }
      v = v + L.b[row + k] * u;
    }
    if (k == 0 || v > m) { m = v; best = k; }
  }
  return best;
}

template <bool LEARN, bool ACT, bool INJECT>
__global__ __launch_bounds__(256) void anymdp_mbrl_learn_kernel(AnyMDPArgs P, MBArgs L, XvLearnStepIO io) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (LEARN && i == 0) *L.count_next = 0u;      // its last readers (the previous step's estimator) have finished
  if (i >= L.B.n_env) return;
  const int S = L.B.S, A = L.B.A;
  if (LEARN) {   // learner(s, a, ns, r, terminated, truncated) :57-71
    const int s = L.cur_obs[i], a = io.act_prev[i];
    const bool term = io.terminated[i] != 0, done = term || io.truncated[i] != 0;
    const int ns = done ? io.final_obs[i] : io.obs[i];
    const bool ok = (unsigned)s < (unsigned)S && (unsigned)a < (unsigned)A && (unsigned)ns < (unsigned)S;
    if (ok) {
      const size_t sa = ((size_t)i * S + s) * A + a, j = sa * S + ns;
      const double cnt = L.vis_cnt[j];
      L.est_r[j] = (L.est_r[j] * cnt + (double)io.reward[i]) / (cnt + 1.0);
      L.vis_cnt[j] = cnt + 1.0;
      L.vis_cnt_sa[sa] = L.vis_cnt_sa[sa] + 1.0;
    }
    if (done) {   // the terminal reset of row ns, update_estimator() and the next action: the estimator launch
      L.term_ns[i] = (term && ok) ? ns : -1;
      L.cur_obs[i] = io.obs[i];
      L.list[atomicAdd(L.count, 1u)] = i;
      return;
    }
  }
  if (ACT) {
    const int o = xv_learner_act_obs(P, io.obs, i);
    L.cur_obs[i] = o;
    io.action_out[i] = (unsigned)o < (unsigned)S ? mbrl_policy<INJECT>(L, io, i, o) : 0;
  } else if (LEARN) {
    L.cur_obs[i] = io.obs[i];
  }
}

// numpy's pairwise_sum below its split size, over f(off .. off + n - 1): a plain loop below 8, eight partial sums up to 128
template <class F>
__device__ __forceinline__ double mbrl_leaf(const F& f, int off, int n) {
  if (n < 8) {
    double res = 0.0;
    for (int k = 0; k < n; ++k) res += f(off + k);
    return res;
  }
  double r0 = f(off), r1 = f(off + 1), r2 = f(off + 2), r3 = f(off + 3);
  double r4 = f(off + 4), r5 = f(off + 5), r6 = f(off + 6), r7 = f(off + 7);
  const int body = n - (n % 8);
  for (int k = 8; k < body; k += 8) {
    r0 += f(off + k); r1 += f(off + k + 1); r2 += f(off + k + 2); r3 += f(off + k + 3);
    r4 += f(off + k + 4); r5 += f(off + k + 5); r6 += f(off + k + 6); r7 += f(off + k + 7);
  }
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (int k = body; k < n; ++k) res += f(off + k);
  return res;
}

// numpy.sum(row) of one row of n = S values (one lane): a leaf up to 128, else the plan's row tree
__device__ double mbrl_rowsum(const double* p, int n, const MBRLTree& T) {
  auto f = [&](int k) { return p[k]; };
  if (n <= 128) return 0.0 + mbrl_leaf(f, 0, n);
  double stk[MBRL_STACK];
  int sp = 0;
  for (int q = 0; q < T.n_ops; ++q) {
    const int op = T.ops[q];
    if (op >= 0) {
      stk[sp++] = mbrl_leaf(f, T.leaf_off[op], T.leaf_off[op + 1] - T.leaf_off[op]);
    } else {
      const double y = stk[--sp];
      stk[sp - 1] = stk[sp - 1] + y;
    }
  }
  return 0.0 + stk[0];
}

// numpy.sum of one env's whole tensor, f(k) its element k (or that element's squared deviation): each chunk's leaves summed by
// the lanes, the chunk's tree combined by lane 0, the chunks added in order.  -> the sum, in every lane
template <class F>
__device__ double mbrl_tensor_sum(const F& f, const MBRLPlan* plan, double* leaf, double* stk) {
  const int lane = threadIdx.x;
  double acc = 0.0;
  const int n_chunks = plan->n_full + plan->has_tail;
  for (int c = 0; c < n_chunks; ++c) {
    const MBRLTree& T = plan->tree[c < plan->n_full ? 0 : 1];
    const int base = c * MBRL_CHUNK;
    for (int k = lane; k < T.n_leaves; k += MBRL_WAVE)
      leaf[k] = mbrl_leaf([&](int e) { return f(base + e); }, T.leaf_off[k], T.leaf_off[k + 1] - T.leaf_off[k]);
    __syncthreads();
    if (lane == 0) {
      int sp = 0;
      for (int q = 0; q < T.n_ops; ++q) {
        const int op = T.ops[q];
        if (op >= 0) {
          stk[sp++] = leaf[op];
        } else {
          const double y = stk[--sp];
          stk[sp - 1] = stk[sp - 1] + y;
        }
      }
      acc = acc + stk[0];
    }
    __syncthreads();
  }
  if (lane == 0) stk[0] = acc;
  __syncthreads();
  const double r = stk[0];
  __syncthreads();
  return r;
}

// update_estimator() :42-55 (after the terminal reset of :64-66) for the envs on this step's list, one wave each; then the
// policy from the observation the step returned
template <bool ACT, bool INJECT, bool LDS_P>
__global__ __launch_bounds__(64) void anymdp_mbrl_estimator_kernel(MBArgs L, XvLearnStepIO io) {
  extern __shared__ double sm[];
  const int S = L.B.S, A = L.B.A, lane = threadIdx.x;
  double* M = sm;                      // [S] max(vm[sn]) as the sweep stands
  double* den = M + S;                 // [A] clip(rowsum(vis_cnt[s, a]), 0.01) of the current row
  double* pre = den + A;               // [A] 0 + the products of sn < s
  double* vrow = pre + A;              // [A] vm[s, :]
  double* leaf = vrow + A;             // [MBRL_LEAVES]
  double* stk = leaf + MBRL_LEAVES;    // [MBRL_STACK]
  double* Pp = LDS_P ? stk + MBRL_STACK : L.scratch + (size_t)blockIdx.x * A * S;   // [A][S] the current row's products
  const uint32_t n_list = *L.count;
  const int per = S * A * S, per_sa = S * A;
  for (uint32_t q = blockIdx.x; q < n_list; q += gridDim.x) {
    const int i = L.list[q];
    double* er = L.est_r + (size_t)i * per;
    double* vc = L.vis_cnt + (size_t)i * per;
    double* vm = L.vm + (size_t)i * per_sa;
    const int tn = L.term_ns[i];
    if (tn >= 0) {       // learner :64-66: vis_cnt[ns] = 0, est_r[ns] = 0
      for (int k = lane; k < A * S; k += MBRL_WAVE) {
        er[(size_t)tn * A * S + k] = 0.0;
        vc[(size_t)tn * A * S + k] = 0.0;
      }
    }
    __syncthreads();
    // est_r_std = max(np.std(est_r), 0.01); b = _c est_r_std / sqrt(vis_cnt_sa)
    const double mean = mbrl_tensor_sum([&](int k) { return er[k]; }, L.plan, leaf, stk) / (double)per;
    const double var = mbrl_tensor_sum([&](int k) { const double d = er[k] - mean; return d * d; }, L.plan, leaf, stk) /
                       (double)per;
    double sd = sqrt(var);
    sd = 0.01 > sd ? 0.01 : sd;
    const double cb = L.cc * sd;
    for (int k = lane; k < per_sa; k += MBRL_WAVE)
      L.b[(size_t)i * per_sa + k] = cb / sqrt(L.vis_cnt_sa[(size_t)i * per_sa + k]);
    // update_value_matrix(t, r, gamma, vm, max_iteration=1): one Gauss-Seidel sweep, alpha = 1
    for (int sn = lane; sn < S; sn += MBRL_WAVE) {
      const double* row = vm + (size_t)sn * A;
      double m = row[0];
      for (int k = 1; k < A; ++k) m = row[k] > m ? row[k] : m;
      M[sn] = m;
    }
    __syncthreads();
    for (int s = 0; s < S; ++s) {
      const double* ers = er + (size_t)s * A * S;
      const double* vcs = vc + (size_t)s * A * S;
      for (int a = lane; a < A; a += MBRL_WAVE) {
        const double rs = mbrl_rowsum(vcs + (size_t)a * S, S, L.plan->tree[2]);
        den[a] = rs < 0.01 ? 0.01 : rs;      // numpy.clip(rowsum, 0.01, None)
        vrow[a] = vm[(size_t)s * A + a];
      }
      __syncthreads();
      for (int a = 0; a < A; ++a) {
        const double da = den[a];
        for (int sn = lane; sn < S; sn += MBRL_WAVE) {
          const int k = a * S + sn;
          Pp[k] = (vcs[k] / da) * (L.gamma * M[sn] + ers[k]);
        }
      }
      __syncthreads();
      for (int a = lane; a < A; a += MBRL_WAVE) {
        const double* pa = Pp + (size_t)a * S;
        double x = 0.0;
        int sn = 0;
        for (; sn + 8 <= s; sn += 8) {
          const double p0 = pa[sn], p1 = pa[sn + 1], p2 = pa[sn + 2], p3 = pa[sn + 3];
          const double p4 = pa[sn + 4], p5 = pa[sn + 5], p6 = pa[sn + 6], p7 = pa[sn + 7];
          x += p0; x += p1; x += p2; x += p3; x += p4; x += p5; x += p6; x += p7;
        }
        for (; sn < s; ++sn) x += pa[sn];
        pre[a] = x;
      }
      __syncthreads();
      // wave-uniform: every lane runs the same chains (LDS reads of one address broadcast)
      double ms = M[s];
      for (int a = 0; a < A; ++a) {
        const double* pa = Pp + (size_t)a * S;
        const int k = a * S + s;
        double x = pre[a] + (vcs[k] / den[a]) * (L.gamma * ms + ers[k]);
        int sn = s + 1;
        for (; sn + 8 <= S; sn += 8) {
          const double p0 = pa[sn], p1 = pa[sn + 1], p2 = pa[sn + 2], p3 = pa[sn + 3];
          const double p4 = pa[sn + 4], p5 = pa[sn + 5], p6 = pa[sn + 6], p7 = pa[sn + 7];
          x += p0; x += p1; x += p2; x += p3; x += p4; x += p5; x += p6; x += p7;
        }
        for (; sn < S; ++sn) x += pa[sn];
        const double v = vrow[a];
        __syncthreads();
        if (lane == 0) vrow[a] = v + (x - v);     // cur_vm[s, a] += alpha (exp_q - cur_vm[s, a])
        __syncthreads();
        double m = vrow[0];
        for (int kk = 1; kk < A; ++kk) m = vrow[kk] > m ? vrow[kk] : m;
        ms = m;
      }
      for (int a = lane; a < A; a += MBRL_WAVE) vm[(size_t)s * A + a] = vrow[a];
      __syncthreads();
      if (lane == 0) M[s] = ms;
      __syncthreads();
    }
    if (ACT && lane == 0) {
      const int o = L.cur_obs[i];
      io.action_out[i] = (unsigned)o < (unsigned)S ? mbrl_policy<INJECT>(L, io, i, o) : 0;
    }
    __syncthreads();
  }
}

// __init__ :13-40 for the masked agents (nullptr: all): est_r = 0, vis_cnt = 0.01, vis_cnt_sa = 1, and what the first
// update_estimator() makes of that: vm = 0, b = (_c max(std(0), 0.01)) / sqrt(1)
static __global__ __launch_bounds__(256) void anymdp_mbrl_reset_kernel(MBArgs L, const uint8_t* mask) {
  const size_t per = (size_t)L.B.S * L.B.A * L.B.S, per_sa = (size_t)L.B.S * L.B.A, total = (size_t)L.B.n_env * per;
  const double b0 = (L.cc * 0.01) / sqrt(1.0);
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t i = idx / per;
    if (mask && !mask[i]) continue;
    L.est_r[idx] = 0.0;
    L.vis_cnt[idx] = 0.01;
    const size_t j = idx - i * per;
    if (j < per_sa) {
      L.vis_cnt_sa[i * per_sa + j] = 1.0;
      L.vm[i * per_sa + j] = 0.0;
      L.b[i * per_sa + j] = b0;
    }
  }
}

static MBArgs mbrl_args(xv_anymdp_mbrl* m) {
  MBArgs L;
  L.est_r = m->est_r; L.vis_cnt = m->vis_cnt; L.vis_cnt_sa = m->vis_cnt_sa; L.vm = m->vm; L.b = m->b;
  L.cur_obs = m->cur_obs; L.term_ns = m->term_ns; L.list = m->list;
  L.count = m->count + m->parity; L.count_next = m->count + (m->parity ^ 1);
  L.plan = m->plan; L.scratch = m->scratch;
  L.gamma = m->gamma; L.cc = m->cc;
  L.B = xv_learner_bind(m->h);
  return L;
}

// the pairwise tree numpy's pairwise_sum builds over n elements (n <= 8192)
static void mbrl_tree_build(MBRLTree& T, int off, int n) {
  if (n <= 128) {
    T.leaf_off[T.n_leaves] = off;
    T.ops[T.n_ops++] = (int16_t)T.n_leaves++;
    return;
  }
  int n2 = n / 2;
  n2 -= n2 % 8;
  mbrl_tree_build(T, off, n2);
  mbrl_tree_build(T, off + n2, n - n2);
  T.ops[T.n_ops++] = -1;
}

static void mbrl_tree(MBRLTree& T, int n) {
  T.n_leaves = 0;
  T.n_ops = 0;
  if (n > 0) mbrl_tree_build(T, 0, n);
  T.leaf_off[T.n_leaves] = n;
}

static void mbrl_free(xv_anymdp_mbrl* m) {
  void* ps[] = {m->est_r, m->vis_cnt, m->vis_cnt_sa, m->vm, m->b, m->cur_obs, m->term_ns, m->list, m->count, m->plan,
                m->scratch};
  for (void* p : ps)
    if (p) (void)hipFree(p);
  delete m;
}

extern "C" int xv_anymdp_mbrl_reset(xv_anymdp_mbrl* m, const uint8_t* mask) {
  XV_CHECK_ARG(m != nullptr);
  hipLaunchKernelGGL(anymdp_mbrl_reset_kernel, dim3(xv_learner_blocks((size_t)m->n_env * m->S * m->A * m->S)), dim3(256), 0,
                     m->h->eng->stream, mbrl_args(m), mask);
  XV_LAUNCH_CHECK();
  return XV_OK;
}

extern "C" int xv_anymdp_mbrl_create(xv_anymdp* h, double gamma, double c, xv_anymdp_mbrl** out) {
  XV_CHECK_ARG(out != nullptr);
  *out = nullptr;
  XV_CHECK_ARG(h != nullptr && gamma >= 0.0 && gamma < 1.0 && c == c);
  // the tables are indexed by observation id: every id of the task tables must be a row
  int rc = xv_anymdp_learner_check(h, __func__, "the model-based learner takes MDP tasks only (its states are observation ids)",
                                   "the model");
  if (rc != XV_OK) return rc;
  xv_engine* e = h->eng;
  const int n_env = h->a.n_env, S = h->a.S, A = h->a.A;
  // the estimator: one wave per workgroup, 12 per CU (3 per SIMD: what its ~150 VGPRs leave resident); the row's products
  // in LDS when they fit, else a global slab per workgroup
  int cus = 0;
  XV_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device));
  int grid = (cus > 0 ? cus : 256) * 12;
  if (grid > n_env) grid = n_env;
  const size_t lds_base = sizeof(double) * ((size_t)S + 3 * (size_t)A + MBRL_LEAVES + MBRL_STACK);
  const size_t prod = sizeof(double) * (size_t)A * S;
  const bool lds_p = lds_base + prod <= MBRL_LDS_MAX;
  if (!lds_p) {
    const size_t cap = (size_t)256 << 20;      // at most 256 MiB of product slabs
    if ((size_t)grid * prod > cap) grid = (int)(cap / prod > 0 ? cap / prod : 1);
  }
  // the memory check comes before any allocation: N (2 S A S + 3 S A) doubles, the lists, the plan, the slabs
  const double per_env = 8.0 * (2.0 * S * A * S + 3.0 * S * A) + 12.0;
  const double need = per_env * n_env + (lds_p ? 0.0 : (double)grid * prod) + sizeof(MBRLPlan) + 8.0;
  size_t free_b = 0, total_b = 0;
  XV_HIP(hipMemGetInfo(&free_b, &total_b));
  const double margin = 2.0 * (1 << 30);
  if (need + margin > (double)free_b) {
    xv_set_error("xv_anymdp_mbrl_create: %.0f bytes of agent tables (%d envs x %d x %d x %d) do not fit the %zu bytes free "
                 "less a 2 GiB margin", need, n_env, S, A, S, free_b);
    return XV_ERR_NOMEM;
  }
  xv_anymdp_mbrl* m = new (std::nothrow) xv_anymdp_mbrl();
  if (!m) {
    xv_set_error("xv_anymdp_mbrl_create: out of host memory");
    return XV_ERR_NOMEM;
  }
  m->h = h; m->device = e->device; m->gamma = gamma; m->c = c; m->cc = c / (1.0 - gamma);
  m->n_env = n_env; m->S = S; m->A = A; m->parity = 0; m->grid = grid;
  m->lds = lds_base + (lds_p ? prod : 0);
  const size_t nsas = (size_t)n_env * S * A * S, nsa = (size_t)n_env * S * A, n = (size_t)n_env;
  hipError_t r = hipMalloc(&m->est_r, sizeof(double) * nsas);
  if (r == hipSuccess) r = hipMalloc(&m->vis_cnt, sizeof(double) * nsas);
  if (r == hipSuccess) r = hipMalloc(&m->vis_cnt_sa, sizeof(double) * nsa);
  if (r == hipSuccess) r = hipMalloc(&m->vm, sizeof(double) * nsa);
  if (r == hipSuccess) r = hipMalloc(&m->b, sizeof(double) * nsa);
  if (r == hipSuccess) r = hipMalloc(&m->cur_obs, sizeof(int32_t) * n);
  if (r == hipSuccess) r = hipMalloc(&m->term_ns, sizeof(int32_t) * n);
  if (r == hipSuccess) r = hipMalloc(&m->list, sizeof(int32_t) * n);
  if (r == hipSuccess) r = hipMalloc(&m->count, sizeof(uint32_t) * 2);
  if (r == hipSuccess) r = hipMalloc(&m->plan, sizeof(MBRLPlan));
  if (r == hipSuccess && !lds_p) r = hipMalloc(&m->scratch, (size_t)grid * prod);
  if (r != hipSuccess) {
    (void)hipGetLastError();
    xv_set_error("xv_anymdp_mbrl_create: %.0f bytes of agent tables do not fit: %s", need, hipGetErrorString(r));
    mbrl_free(m);
    return r == hipErrorOutOfMemory ? XV_ERR_NOMEM : XV_ERR_HIP;
  }
  MBRLPlan plan;
  const int n_tot = S * A * S;
  plan.n_full = n_tot / MBRL_CHUNK;
  plan.has_tail = n_tot % MBRL_CHUNK ? 1 : 0;
  mbrl_tree(plan.tree[0], MBRL_CHUNK);
  mbrl_tree(plan.tree[1], n_tot % MBRL_CHUNK);
  mbrl_tree(plan.tree[2], S);
  r = hipMemcpyAsync(m->plan, &plan, sizeof(MBRLPlan), hipMemcpyHostToDevice, e->stream);
  if (r == hipSuccess) r = hipMemsetAsync(m->cur_obs, 0, sizeof(int32_t) * n, e->stream);
  if (r == hipSuccess) r = hipMemsetAsync(m->count, 0, sizeof(uint32_t) * 2, e->stream);
  if (r == hipSuccess) r = hipStreamSynchronize(e->stream);     // `plan` lives on this stack frame
  if (r != hipSuccess) {
    xv_set_error("xv_anymdp_mbrl_create: %s", hipGetErrorString(r));
    mbrl_free(m);
    return XV_ERR_HIP;
  }
  rc = xv_anymdp_mbrl_reset(m, nullptr);
  if (rc != XV_OK) {
    mbrl_free(m);
    return rc;
  }
  *out = m;
  return XV_OK;
}

extern "C" int xv_anymdp_mbrl_destroy(xv_anymdp_mbrl* m) { return xv_learner_destroy(m, mbrl_free); }

static int mbrl_copy(xv_anymdp_mbrl* m, bool to_learner, const double* est_r, const double* vis_cnt, const double* vis_cnt_sa,
                     const double* vm, const double* b) {
  const size_t nsa = sizeof(double) * (size_t)m->n_env * m->S * m->A, nsas = nsa * m->S;
  void* const dev[5] = {m->est_r, m->vis_cnt, m->vis_cnt_sa, m->vm, m->b};
  const size_t bytes[5] = {nsas, nsas, nsa, nsa, nsa};
  const void* const user[5] = {est_r, vis_cnt, vis_cnt_sa, vm, b};
  return xv_learner_copy(m->h, to_learner, 5, dev, bytes, user);
}

extern "C" int xv_anymdp_mbrl_get_state(xv_anymdp_mbrl* m, double* est_r, double* vis_cnt, double* vis_cnt_sa, double* vm,
                                        double* b) {
  XV_CHECK_ARG(m != nullptr);
  return mbrl_copy(m, false, est_r, vis_cnt, vis_cnt_sa, vm, b);
}

extern "C" int xv_anymdp_mbrl_set_state(xv_anymdp_mbrl* m, const double* est_r, const double* vis_cnt,
                                        const double* vis_cnt_sa, const double* vm, const double* b) {
  XV_CHECK_ARG(m != nullptr);
  return mbrl_copy(m, true, est_r, vis_cnt, vis_cnt_sa, vm, b);
}

template <bool LEARN, bool ACT, bool INJECT>
static void mbrl_launch_learn(xv_anymdp_mbrl* m, const MBArgs& L, const XvLearnStepIO& io) {
  hipLaunchKernelGGL((anymdp_mbrl_learn_kernel<LEARN, ACT, INJECT>), dim3(xv_div_up(m->n_env, 256)), dim3(256), 0,
                     m->h->eng->stream, m->h->a, L, io);
}

template <bool ACT, bool INJECT>
static void mbrl_launch_estimator(xv_anymdp_mbrl* m, const MBArgs& L, const XvLearnStepIO& io) {
  if (m->scratch)
    hipLaunchKernelGGL((anymdp_mbrl_estimator_kernel<ACT, INJECT, false>), dim3(m->grid), dim3(MBRL_WAVE), m->lds,
                       m->h->eng->stream, L, io);
  else
    hipLaunchKernelGGL((anymdp_mbrl_estimator_kernel<ACT, INJECT, true>), dim3(m->grid), dim3(MBRL_WAVE), m->lds,
                       m->h->eng->stream, L, io);
}

// the first launch: the policy from every env's current observation
template <bool INJECT>
static int mbrl_launch_first(xv_anymdp_mbrl* m, const XvLearnStepIO& io) {
  const MBArgs L = mbrl_args(m);
  mbrl_launch_learn<false, true, INJECT>(m, L, io);
  XV_LAUNCH_CHECK();
  return XV_OK;
}

// after a step: learn (the next action for envs whose episode goes on), then the estimator for those whose episode ended
template <bool ACT, bool INJECT>
static int mbrl_launch_step(xv_anymdp_mbrl* m, const XvLearnStepIO& io) {
  const MBArgs L = mbrl_args(m);
  mbrl_launch_learn<true, ACT, INJECT>(m, L, io);
  mbrl_launch_estimator<ACT, INJECT>(m, L, io);
  m->parity ^= 1;
  XV_LAUNCH_CHECK();
  return XV_OK;
}

static int mbrl_first(xv_anymdp_mbrl* m, const XvLearnStepIO& io) {
  return io.u_policy ? mbrl_launch_first<true>(m, io) : mbrl_launch_first<false>(m, io);
}
static int mbrl_after(xv_anymdp_mbrl* m, const XvLearnStepIO& io, bool act) {
  if (!act) return mbrl_launch_step<false, false>(m, io);
  return io.u_policy ? mbrl_launch_step<true, true>(m, io) : mbrl_launch_step<true, false>(m, io);
}

extern "C" int xv_anymdp_rollout_mbrl(xv_anymdp* h, xv_anymdp_mbrl* m, int T, int greedy, const double* u_policy,
                                      const double* u, const float* z, const double* u_reset, int32_t* action_out,
                                      int32_t* obs, float* reward, float* reward_gt, uint8_t* terminated,
                                      uint8_t* truncated, int32_t* final_obs) {
  return xv_learner_rollout(__func__, mbrl_first, mbrl_after, h, m, T, greedy, u_policy, u, z, u_reset, action_out, obs,
                            reward, reward_gt, terminated, truncated, final_obs);
}
