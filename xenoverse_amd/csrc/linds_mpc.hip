// linds_mpc.hip — the LinDS MPC teacher on the device: the reference's LTISystemMPC (xenoverse/linds/solver.py:16-125) for
// every env of an xv_linds handle, one box-constrained QP per env-step, solved with OSQP's ADMM (A = I) on the matrix unit.
//
// The QP of env e (task t, state x, future commands ref[0..K)):   min 1/2 U^T P_t U + q^T U,  -1 <= U <= 1,
//   q = G_x x + g_0 - G_r vec(ref)   (xenoverse_amd/linds/teacher.py: device_tables; the row-block reversal of Y_ref
//                                    is folded into G_r, solver.py:98-110)
// Iteration (per env, cold start x = z = y = 0, as the reference's OSQP call):
//   x~ = M_t (sigma x - q + rho z - y),        M_t = (P_t + (sigma + rho_t) I)^-1, factored on the host in fp64, fp32 here
//   x  = alpha x~ + (1 - alpha) x,  z = clip(alpha x~ + (1 - alpha) z_old + y / rho),  y = y + rho (alpha x~ + (1 - alpha) z_old - z)
// Every XV_MPC_CHECK iterations an env checks OSQP's residuals (A = I):
//   prim = |x~ - z|_inf   <= eps_abs + eps_rel max(|x~|, |z|) + f
//   dual = |P x~ + q + y|_inf <= eps_abs + eps_rel max(|P x~|, |y|, |q|, |rhs|) + (sigma + rho) f,  P x~ = rhs - (sigma + rho) x~
//          (no second product: the fp32 operator's rounding is relative to |rhs|, hence |rhs| in the scale)
//   f = XV_MPC_FLOOR 2^-24 |M|_inf |rhs|_inf: the rounding floor of x~ = fl32(M rhs).  Without it an env whose M is large
//       against |x~| (a singular P: rho = 1e-3 lambda_max, |M| ~ 1 / rho) jitters at that floor forever and never passes
// and, once they pass, freezes: its x, z, y stop changing.  The test runs at fixed iteration counts and reads the env's own
// values only, and the product treats every column (env) on its own, so an env's result depends on (task, x, ref) alone —
// never on which envs share its tile.  The action is z (the projected iterate: always feasible).
//
// Layout: one workgroup of 4 waves per 16-slot tile of the handle (one task per tile, linds.hip's slot layout); wave w owns
// the output M-tiles w, w + 4, ... of n_pad / 16.  Per iteration every wave writes its rows of rhs to LDS (fragment order:
// float4 L[k / 4][env], k = 16 q + 4 g + r), one barrier, then the product M rhs as a chain of v_mfma_f32_16x16x4_f32 over
// q with the task's M fragments streamed from L2 (xenoverse_amd/linds/teacher.py: _frag); two LDS buffers alternate so one
// barrier per iteration suffices.
#define XV_KERNELS_ONLY
#include "linds.hip"
#undef XV_KERNELS_ONLY

#ifndef XV_MPC_CHECK
#define XV_MPC_CHECK 10   // iterations between residual checks
#endif
#ifndef XV_MPC_FLOOR
#define XV_MPC_FLOOR 1.0f // the residual test's allowance for the rounding of x~ = M rhs, in units of 2^-24 |M|_inf |rhs|_inf
#endif

struct xv_linds_mpc {
  xv_linds* l;
  int K, n_pad, n_in, NOc, max_iter;
  double gamma;
  float sigma, alpha, eps_abs, eps_rel;
  float4 *mfrag, *gfrag;   // owned device copies
  float *g0, *rho, *mnorm;
  int32_t* nu;
  float* cmd_tab;          // [n_task][ct_len][NOc]: get_inner_cmd at tt in [ct_tmin, ct_tmin + ct_len), times target_valid
  int ct_len, ct_tmin;
};

struct MPCArgs {
  const float4* mfrag;     // [n_task][n_pad/16][n_pad/16][64]
  const float4* gfrag;     // [n_task][n_pad/16][n_in/16][64]
  const float* g0;         // [n_task][n_pad]
  const float* rho;        // [n_task]
  const float* mnorm;      // [n_task]  |M|_inf (largest absolute row sum of the fp32 operator)
  const int32_t* nu;       // [n_task]
  const float* cmd_tab;
  int ct_len, ct_tmin;
  int K, n_pad, n_in, NOc, max_iter;
  float sigma, alpha, eps_abs, eps_rel;
  // explicit inputs (xv_linds_mpc_solve) or nullptr: the handle's state and its future commands
  const float* x_in;       // [n_env][NS]
  const float* ref_in;     // [n_env][K][NO]
  // outputs (nullable)
  float* U;                // [n_env][n_pad]
  float* action;           // [n_env][NA]
  int32_t* status;         // [n_env] 1 converged, 0 max_iter
  int32_t* iters;          // [n_env]
};

// four columns c..c+3 of get_inner_cmd(tt) * target_valid (linds_env.py:93-98) with the engine's operations (linds_cmd: same
// per-column fmaf chain, same sin / cos), for a per-lane time tt
__device__ __forceinline__ float4 mpc_cmd4(const LinDSArgs& P, int tu, int nf, int tt, int c) {
  const float* valid = P.T.valid + (size_t)tu * P.NO + c;
  float o[4];
  if (nf == 0) {
    const float* c0 = P.T.cmd0 + (size_t)tu * P.NO + c;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = c0[j] * valid[j];
    return make_float4(o[0], o[1], o[2], o[3]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = 0.0f;
  const double inv_period_t = (double)tt / P.T.four_period[tu];
  for (int k = 0; k < nf; ++k) {
    float sn, cs;
    linds_four_sincos(P, tu, k, inv_period_t, &sn, &cs);
    const float* cf = P.T.four_coef + (((size_t)tu * XV_LINDS_KMAX + k) * P.NO + c) * 2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[j] = fmaf(cf[2 * j], sn, o[j]);
      o[j] = fmaf(cf[2 * j + 1], cs, o[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] *= valid[j];
  return make_float4(o[0], o[1], o[2], o[3]);
}

static __global__ __launch_bounds__(256) void mpc_build_cmd_tab_kernel(LinDSArgs P, float* tab, int ct_len, int ct_tmin, int NOc) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int nq = NOc / 4;
  if (idx >= (size_t)P.n_task * ct_len * nq) return;
  const int c4 = (int)(idx % nq);
  const size_t row = idx / nq;
  const int t = (int)(row / ct_len), k = (int)(row % ct_len);
  const float4 v = mpc_cmd4(P, t, P.T.ints[(size_t)t * 4 + 3], k + ct_tmin, 4 * c4);
  *reinterpret_cast<float4*>(tab + row * NOc + 4 * c4) = v;
}

// float4 entries of one LDS rhs buffer: n_pad / 4 rows of 16 envs, at least 128 (the residual exchange: 2 x 4 waves x 16 envs)
__host__ __device__ __forceinline__ size_t mpc_buf_float4(int n_pad) {
  const size_t r = (size_t)(n_pad >> 2) * 16;
  return r < 128 ? 128 : r;
}

__device__ __forceinline__ float mpc_max4(float v) {   // max over the 4 lane groups (16, 32 lanes apart) of one env
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}

// OWN: M-tiles per wave (n_pad / 16 <= 4 OWN)
template <int OWN>
__global__ __launch_bounds__(256) void linds_mpc_kernel(LinDSArgs P, MPCArgs A) {
  extern __shared__ float4 lds[];   // [2][n_pad / 4][16]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
  const int tile = blockIdx.x, tile0 = 16 * tile;
  if (tile0 >= P.n_slot) return;   // block-uniform
  const int es = tile0 + n;
  int e_raw = es;
  if (P.slot_env != nullptr) e_raw = es < P.n_slot ? P.slot_env[es] : -1;
  const bool valid = es < P.n_slot && e_raw >= 0 && e_raw < P.n_env;
  const int e = valid ? e_raw : 0;
  const int t = P.task_shift >= 4 ? (tile0 >> P.task_shift)
                                  : __builtin_amdgcn_readfirstlane(P.tile_task ? P.tile_task[tile] : P.env_task[tile0]);
  const int MTn = A.n_pad >> 4, QI = A.n_in >> 4;
  const int NS = P.NS, NO = P.NO, NOc = A.NOc, K = A.K;

  // ---- this lane's inputs: the live state and command rows, or the caller's x / ref ----
  const int delay = P.T.ints[(size_t)t * 4 + 1], nf = P.T.ints[(size_t)t * 4 + 3];
  const int steps = (A.x_in == nullptr) ? (int)((uint32_t)P.sn[es] & ~XV_LINDS_NR_BIT) : 0;
  auto input4 = [&](int k) -> float4 {      // rows k..k+3 of w = [x (NS); vec(ref) (K x NOc); 0]
    if (k < NS) {
      if (A.x_in != nullptr) return *reinterpret_cast<const float4*>(A.x_in + (size_t)e * NS + k);
      return *reinterpret_cast<const float4*>(P.x + linds_xidx(es, k, NS >> 4));
    }
    const int kr = k - NS;
    if (kr >= K * NOc) return make_float4(0.f, 0.f, 0.f, 0.f);
    const int j = kr / NOc, c = kr - j * NOc;
    if (A.ref_in != nullptr) return *reinterpret_cast<const float4*>(A.ref_in + ((size_t)e * K + j) * NO + c);
    const int tt = steps - delay + j;           // get_future_inner_cmds (linds_env.py:171-183): cmd(steps - delay + j)
    const int ti = tt - A.ct_tmin;
    if (ti >= 0 && ti < A.ct_len) return *reinterpret_cast<const float4*>(A.cmd_tab + ((size_t)t * A.ct_len + ti) * NOc + c);
    return mpc_cmd4(P, t, nf, tt, c);
  };

  // ---- q = [G_x | -G_r] w + g_0 on this wave's M-tiles ----
  xv_f32x4 qv[OWN], xv[OWN], zv[OWN], yv[OWN];
#pragma unroll
  for (int j = 0; j < OWN; ++j) qv[j] = xv_f32x4{0, 0, 0, 0};
  const float4* gf = A.gfrag + (size_t)t * MTn * QI * 64 + lane;
  for (int qi = 0; qi < QI; ++qi) {
    const float4 b = input4(16 * qi + 4 * g);
#pragma unroll
    for (int j = 0; j < OWN; ++j) {
      const int mt = wave + 4 * j;
      if (mt < MTn) {
        const float4 a = gf[((size_t)mt * QI + qi) * 64];
        qv[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, qv[j], 0, 0, 0);
        qv[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, qv[j], 0, 0, 0);
        qv[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, qv[j], 0, 0, 0);
        qv[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, qv[j], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < OWN; ++j) {
    xv_mfma_settle(qv[j]);
    const int mt = wave + 4 * j;
    const float4 g0 = mt < MTn ? *reinterpret_cast<const float4*>(A.g0 + (size_t)t * A.n_pad + 16 * mt + 4 * g)
                               : make_float4(0.f, 0.f, 0.f, 0.f);
    qv[j][0] += g0.x; qv[j][1] += g0.y; qv[j][2] += g0.z; qv[j][3] += g0.w;
    xv[j] = zv[j] = yv[j] = xv_f32x4{0, 0, 0, 0};
  }

  // ---- ADMM ----
  const float sigma = A.sigma, alpha = A.alpha, beta = 1.0f - A.alpha;
  const float rho = A.rho[t], inv_rho = 1.0f / rho, sr = sigma + rho;
  const float4* mf = A.mfrag + (size_t)t * MTn * MTn * 64 + lane;
  bool frozen = !valid;
  int it_done = A.max_iter;
  const float mfl = XV_MPC_FLOOR * 5.9604644775390625e-8f * A.mnorm[t];   // 2^-24 |M|_inf
  float4* const buf0 = lds;
  float4* const buf1 = lds + mpc_buf_float4(A.n_pad);
  for (int it = 0; it < A.max_iter; ++it) {
    float4* buf = (it & 1) ? buf1 : buf0;
    float4* other = (it & 1) ? buf0 : buf1;
    xv_f32x4 rhs[OWN];
#pragma unroll
    for (int j = 0; j < OWN; ++j) {
      const int mt = wave + 4 * j;
#pragma unroll
      for (int r = 0; r < 4; ++r) rhs[j][r] = fmaf(rho, zv[j][r], fmaf(sigma, xv[j][r], -qv[j][r])) - yv[j][r];
      if (mt < MTn) buf[(4 * mt + g) * 16 + n] = make_float4(rhs[j][0], rhs[j][1], rhs[j][2], rhs[j][3]);
    }
    __syncthreads();
    xv_f32x4 acc[OWN];
#pragma unroll
    for (int j = 0; j < OWN; ++j) acc[j] = xv_f32x4{0, 0, 0, 0};
    for (int qi = 0; qi < MTn; ++qi) {
      const float4 b = buf[(4 * qi + g) * 16 + n];
#pragma unroll
      for (int j = 0; j < OWN; ++j) {
        const int mt = wave + 4 * j;
        if (mt < MTn) {
          const float4 a = mf[((size_t)mt * MTn + qi) * 64];
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc[j], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < OWN; ++j) xv_mfma_settle(acc[j]);
    const bool check = (it % XV_MPC_CHECK) == XV_MPC_CHECK - 1;
    float prim = 0.f, nprim = 0.f, dual = 0.f, ndual = 0.f, nrhs = 0.f;
    xv_f32x4 xn[OWN], zn[OWN], yn[OWN];
#pragma unroll
    for (int j = 0; j < OWN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float xt = acc[j][r];
        const float zr = fmaf(alpha, xt, beta * zv[j][r]);
        xn[j][r] = fmaf(alpha, xt, beta * xv[j][r]);
        zn[j][r] = fminf(fmaxf(fmaf(yv[j][r], inv_rho, zr), -1.0f), 1.0f);
        yn[j][r] = fmaf(rho, zr - zn[j][r], yv[j][r]);
        if (check) {
          const float px = fmaf(-sr, xt, rhs[j][r]);                 // P x~
          prim = fmaxf(prim, fabsf(xt - zn[j][r]));
          nprim = fmaxf(nprim, fmaxf(fabsf(xt), fabsf(zn[j][r])));
          dual = fmaxf(dual, fabsf((px + qv[j][r]) + yn[j][r]));
          ndual = fmaxf(ndual, fmaxf(fmaxf(fabsf(px), fabsf(yn[j][r])), fabsf(qv[j][r])));
          nrhs = fmaxf(nrhs, fabsf(rhs[j][r]));
        }
      }
    bool conv = false;
    if (check) {   // block-uniform branch: every wave reduces its rows, then reads all four waves' maxima of each env
      prim = mpc_max4(prim); nprim = mpc_max4(nprim); dual = mpc_max4(dual); ndual = mpc_max4(ndual); nrhs = mpc_max4(nrhs);
      if (g == 0) {   // the buffer the next iteration writes (at least 128 float4, mpc_buf_float4)
        other[wave * 16 + n] = make_float4(prim, nprim, dual, ndual);
        other[64 + wave * 16 + n] = make_float4(nrhs, 0.f, 0.f, 0.f);
      }
      __syncthreads();
      float4 m = other[n];
      float mr = other[64 + n].x;
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const float4 v = other[w * 16 + n];
        m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
        mr = fmaxf(mr, other[64 + w * 16 + n].x);
      }
      __syncthreads();   // everybody has read before the next iteration overwrites
      const float f = mfl * mr;
      conv = (m.x <= fmaf(A.eps_rel, m.y, A.eps_abs) + f) &&
             (m.z <= fmaf(A.eps_rel, fmaxf(m.w, mr), A.eps_abs) + sr * f);
    }
    if (!frozen) {
#pragma unroll
      for (int j = 0; j < OWN; ++j) { xv[j] = xn[j]; zv[j] = zn[j]; yv[j] = yn[j]; }
      if (conv) { frozen = true; it_done = it + 1; }
    }
    if (check && __ballot(!frozen) == 0ull) break;   // identical in every wave: same values, same decisions
  }

  // ---- outputs: U = z (rows < n_pad), the action u_0 = z[0 .. Nu), status and iterations ----
  if (!valid) return;
  if (A.U != nullptr) {
#pragma unroll
    for (int j = 0; j < OWN; ++j) {
      const int mt = wave + 4 * j;
      if (mt < MTn)
        *reinterpret_cast<float4*>(A.U + (size_t)e * A.n_pad + 16 * mt + 4 * g) = make_float4(zv[j][0], zv[j][1], zv[j][2], zv[j][3]);
    }
  }
  if (wave == 0) {
    const int NA = P.NA, nu = A.nu[t];
    if (A.action != nullptr) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int a = 4 * g + r;
        if (a < NA) A.action[(size_t)e * NA + a] = a < nu ? zv[0][r] : 0.0f;
      }
    }
    if (g == 0) {
      if (A.status) A.status[e] = frozen ? 1 : 0;
      if (A.iters) A.iters[e] = it_done;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
static void mpc_free(xv_linds_mpc* m) {
  if (m->mfrag) (void)hipFree(m->mfrag);
  if (m->gfrag) (void)hipFree(m->gfrag);
  if (m->g0) (void)hipFree(m->g0);
  if (m->rho) (void)hipFree(m->rho);
  if (m->mnorm) (void)hipFree(m->mnorm);
  if (m->nu) (void)hipFree(m->nu);
  if (m->cmd_tab) (void)hipFree(m->cmd_tab);
  delete m;
}

// solver.py:20-92 (LTISystemMPC.__init__ / _pre_build_matrices): the per-task QP data, built on the host
extern "C" int xv_linds_mpc_create(xv_linds* l, int K, double gamma, const xv_linds_mpc_tables* tab, int max_iter,
                                   xv_linds_mpc** out) {
  XV_CHECK_ARG(out != nullptr);
  *out = nullptr;
  XV_CHECK_ARG(l != nullptr && tab != nullptr && K > 0 && max_iter > 0);
  XV_CHECK_ARG(tab->mfrag && tab->gfrag && tab->g0 && tab->rho && tab->mnorm && tab->nu);
  XV_CHECK_ARG(tab->n_pad > 0 && tab->n_pad % 16 == 0 && tab->n_in % 16 == 0 && tab->NOc > 0 && tab->NOc % 4 == 0);
  XV_CHECK_ARG(tab->NOc <= l->a.NO && tab->n_in >= l->a.NS + K * tab->NOc && tab->n_in < l->a.NS + K * tab->NOc + 16);
  if (tab->n_pad > 512) {
    xv_set_error("xv_linds_mpc_create: n = K * action_dim = %d exceeds 512", tab->n_pad);
    return XV_ERR_UNSUPPORTED;
  }
  xv_engine* e = l->eng;
  XV_HIP(hipSetDevice(e->device));
  xv_linds_mpc* m = new (std::nothrow) xv_linds_mpc();
  if (!m) {
    xv_set_error("xv_linds_mpc_create: out of host memory");
    return XV_ERR_NOMEM;
  }
  m->l = l; m->K = K; m->gamma = gamma; m->n_pad = tab->n_pad; m->n_in = tab->n_in; m->NOc = tab->NOc; m->max_iter = max_iter;
  m->sigma = tab->sigma; m->alpha = tab->alpha; m->eps_abs = tab->eps_abs; m->eps_rel = tab->eps_rel;
  const size_t nt = (size_t)l->a.n_task, mt = (size_t)(tab->n_pad / 16);
  const size_t mf_n = nt * mt * mt * 64, gf_n = nt * mt * (size_t)(tab->n_in / 16) * 64;
  hipError_t r = hipMalloc(&m->mfrag, sizeof(float4) * mf_n);
  if (r == hipSuccess) r = hipMalloc(&m->gfrag, sizeof(float4) * gf_n);
  if (r == hipSuccess) r = hipMalloc(&m->g0, sizeof(float) * nt * tab->n_pad);
  if (r == hipSuccess) r = hipMalloc(&m->rho, sizeof(float) * nt);
  if (r == hipSuccess) r = hipMalloc(&m->mnorm, sizeof(float) * nt);
  if (r == hipSuccess) r = hipMalloc(&m->nu, sizeof(int32_t) * nt);
  if (r == hipSuccess) r = hipMemcpy(m->mfrag, tab->mfrag, sizeof(float4) * mf_n, hipMemcpyHostToDevice);
  if (r == hipSuccess) r = hipMemcpy(m->gfrag, tab->gfrag, sizeof(float4) * gf_n, hipMemcpyHostToDevice);
  if (r == hipSuccess) r = hipMemcpy(m->g0, tab->g0, sizeof(float) * nt * tab->n_pad, hipMemcpyHostToDevice);
  if (r == hipSuccess) r = hipMemcpy(m->rho, tab->rho, sizeof(float) * nt, hipMemcpyHostToDevice);
  if (r == hipSuccess) r = hipMemcpy(m->mnorm, tab->mnorm, sizeof(float) * nt, hipMemcpyHostToDevice);
  if (r == hipSuccess) r = hipMemcpy(m->nu, tab->nu, sizeof(int32_t) * nt, hipMemcpyHostToDevice);
  // command table over t in [-delay_max, max_steps_max + K): every time get_future_inner_cmds asks for while auto-reset keeps
  // steps below max_steps (the step kernel's own table stops at max_steps + 2 + delay)
  std::vector<int32_t> ints(nt * 4);
  if (r == hipSuccess) r = hipMemcpy(ints.data(), l->a.T.ints, sizeof(int32_t) * nt * 4, hipMemcpyDeviceToHost);
  if (r == hipSuccess) {
    int ms = 0, dl = 0;
    for (size_t t = 0; t < nt; ++t) {
      ms = ints[t * 4] > ms ? ints[t * 4] : ms;
      dl = ints[t * 4 + 1] > dl ? ints[t * 4 + 1] : dl;
    }
    m->ct_tmin = -dl;
    m->ct_len = ms + K + dl;
    r = hipMalloc(&m->cmd_tab, sizeof(float) * nt * (size_t)m->ct_len * m->NOc);
    if (r == hipSuccess) {
      const size_t nthr = nt * (size_t)m->ct_len * (size_t)(m->NOc / 4);
      hipLaunchKernelGGL(mpc_build_cmd_tab_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, e->stream, l->a,
                         m->cmd_tab, m->ct_len, m->ct_tmin, m->NOc);
      r = hipGetLastError();
    }
  }
  if (r != hipSuccess) {
    xv_set_error("xv_linds_mpc_create: %s", hipGetErrorString(r));
    mpc_free(m);
    return XV_ERR_HIP;
  }
  *out = m;
  return XV_OK;
}

extern "C" int xv_linds_mpc_destroy(xv_linds_mpc* m) {
  if (!m) return XV_OK;
  (void)hipSetDevice(m->l->eng->device);
  (void)hipStreamSynchronize(m->l->eng->stream);
  mpc_free(m);
  return XV_OK;
}

static int mpc_launch(xv_linds_mpc* m, const float* x, const float* ref, float* U, float* action, int32_t* status, int32_t* iters) {
  xv_linds* l = m->l;
  MPCArgs A;
  A.mfrag = m->mfrag; A.gfrag = m->gfrag; A.g0 = m->g0; A.rho = m->rho; A.mnorm = m->mnorm; A.nu = m->nu;
  A.cmd_tab = m->cmd_tab; A.ct_len = m->ct_len; A.ct_tmin = m->ct_tmin;
  A.K = m->K; A.n_pad = m->n_pad; A.n_in = m->n_in; A.NOc = m->NOc; A.max_iter = m->max_iter;
  A.sigma = m->sigma; A.alpha = m->alpha; A.eps_abs = m->eps_abs; A.eps_rel = m->eps_rel;
  A.x_in = x; A.ref_in = ref; A.U = U; A.action = action; A.status = status; A.iters = iters;
  const int MTn = m->n_pad / 16;
  const dim3 grid((unsigned)xv_div_up(l->a.n_slot, 16)), block(256);
  const size_t shm = sizeof(float4) * 2 * mpc_buf_float4(m->n_pad);
  if (MTn <= 4) hipLaunchKernelGGL((linds_mpc_kernel<1>), grid, block, shm, l->eng->stream, l->a, A);
  else if (MTn <= 8) hipLaunchKernelGGL((linds_mpc_kernel<2>), grid, block, shm, l->eng->stream, l->a, A);
  else if (MTn <= 16) hipLaunchKernelGGL((linds_mpc_kernel<4>), grid, block, shm, l->eng->stream, l->a, A);
  else hipLaunchKernelGGL((linds_mpc_kernel<8>), grid, block, shm, l->eng->stream, l->a, A);
  XV_LAUNCH_CHECK();
  return XV_OK;
}

// solver.py:94-125 (solve) driven as test_mpc :127-150 does: x = env._state, ref = env.get_future_inner_cmds(K)
extern "C" int xv_linds_mpc_action(xv_linds_mpc* m, float* action, float* U, int32_t* status, int32_t* iters) {
  XV_CHECK_ARG(m != nullptr && action != nullptr);
  return mpc_launch(m, nullptr, nullptr, U, action, status, iters);
}

// solver.py:94-118 on explicit inputs (parity hook): the full U of every env
extern "C" int xv_linds_mpc_solve(xv_linds_mpc* m, const float* x, const float* ref, float* U, int32_t* status, int32_t* iters) {
  XV_CHECK_ARG(m != nullptr && x != nullptr && ref != nullptr && U != nullptr);
  return mpc_launch(m, x, ref, U, nullptr, status, iters);
}

// test_mpc's loop (solver.py:138-157): T x (solve, step) with SAME_STEP auto-reset, issued from C
extern "C" int xv_linds_rollout_mpc(xv_linds_mpc* m, int T, float* action, float* obs, float* reward, uint8_t* terminated,
                                    uint8_t* truncated, float* cmd, float* error, float* final_obs, int32_t* status, int32_t* iters) {
  XV_CHECK_ARG(m != nullptr && T > 0 && action && obs && reward && terminated && truncated && cmd && error);
  xv_linds* l = m->l;
  const size_t n = (size_t)l->a.n_env, NA = (size_t)l->a.NA, NO = (size_t)l->a.NO;
  for (int t = 0; t < T; ++t) {
    const size_t o = (size_t)t * n;
    int rc = xv_linds_mpc_action(m, action + o * NA, nullptr, status ? status + o : nullptr, iters ? iters + o : nullptr);
    if (rc != XV_OK) return rc;
    if (l->path == XV_LINDS_PATH_SCALAR)
      rc = xv_linds_step(l, action + o * NA, obs + o * NO, reward + o, terminated + o, truncated + o, cmd + o * NO, error + o,
                         final_obs ? final_obs + o * NO : nullptr, XV_AUTORESET_SAME_STEP);
    else
      rc = xv_linds_step_info(l, action + o * NA, obs + o * NO, reward + o, terminated + o, truncated + o, cmd + o * NO,
                              error + o, final_obs ? final_obs + o * NO : nullptr, nullptr, nullptr, XV_AUTORESET_SAME_STEP);
    if (rc != XV_OK) return rc;
  }
  return XV_OK;
}
