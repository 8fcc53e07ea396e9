// metalang.hip — MetaLangV2 on the device: the reference's RandomNGram.forward (xenoverse/metalang/metalangv2.py:31-77), the
// generator of synthetic pseudo-languages.  Host restatement and the full statement of the semantics:
// xenoverse_amd/metalang/host.py.  A GROUP is one task (five fp64 arrays: word_emb [V][E], W_in [n][E][H], b_in [n][H],
// W_out [H][V], b_out [V], and lambda) with B sequences that share one mean and one standard deviation per step.  Per step t
// of a group, in fp64:
//   :57-62  a[g] = emb[window[g]] @ W_in[g] + b_in[g], g = 0 .. n-1; the window holds the last n tokens, oldest first
//   :63     h = (sum_g g tanh(a[g])) / n            (slot 0 has weight 0 and is not evaluated)
//   :64     o = h @ W_out + b_out
//   :37-41  m = mean(o), std = sqrt(mean(o o) - m m) over all B V logits; o = lambda ((1 / std) (o - m))
//   :67-69  e = exp(o), S = sum_v e, token = first v with cumsum(e)[v] / S > u, 0 if there is none
//   :70-71  log p = log(e[token] / S)
//
// Kernel: one workgroup per group (generate) or per (group, chunk of positions) (teacher forcing: log_prob), thread v owns
// vocabulary column v — the block is 64, 256 or 1024 threads, whichever holds V.  W_out[:, v] stays in registers for the whole
// call where H <= 64 and V <= 256 (HR doubles), otherwise it is read through L2 every step.  word_emb and the input layer of
// slots 1 .. n-1 are copied to LDS at the start where the workgroup then stays within 64 KiB (TL), otherwise read through L2.
// Per step: the hidden layer on (b, g, j) items over the block -> LDS; the thread's B logits (a register for B = 1, else LDS,
// or HBM scratch where B V is too large for LDS); the two sums by wave scans (DPP) and one LDS exchange; exp; per b a
// wave-inclusive scan of e, wave totals exchanged through LDS; ballot + first set bit for the first cut above u; the lowest
// hit of the waves is the token.  A step touches LDS only: uniforms (and, teacher-forced, tokens) are fetched and tokens and
// log-probabilities written out once per block of K steps, because a barrier waits for the wave's outstanding loads and
// stores.  The scan adds in tree order where numpy's cumsum adds left to right: a cut may differ by a few 1e-16 (DESIGN.md
// §3.6: the band).  The build keeps -ffp-contract=off: every FMA below is written out.
//
// Free-running draws: u = xv_u53 of Philox words keyed by (engine seed, global sequence id = env_id_base + group * B + b,
// the call's tick, XV_DRAW_METALANG, sub = t >> 1): words 0,1 for even t, 2,3 for odd t.
#include "philox.h"
#include "xv_common.h"

#define XV_DRAW_METALANG 8u

#define ML_V_MAX 1024
#define ML_H_MAX 128
#define ML_E_MAX 64
#define ML_NG_MAX 8
#define ML_B_MAX 64
#define ML_ACT_CAP 512       // doubles of LDS for one pass of the hidden layer's activations (one sequence's if those are more)
#define ML_TAB_CAP 8192      // word_emb, W_in and b_in of the group's task are copied to LDS up to this many doubles
#define ML_O_LDS_CAP 4096    // logits of a group (B * block) kept in LDS up to here, in HBM scratch beyond
#define ML_TEACHER_CHUNK 128 // positions per workgroup of log_prob

struct MLArgs {
  const double* emb;     // [n_task][V][E]
  const double* w_in;    // [n_task][NG][E][H]   rows g >= n_gram[task] unused
  const double* b_in;    // [n_task][NG][H]
  const double* w_out;   // [n_task][H][V]
  const double* b_out;   // [n_task][V]
  const double* lam;     // [n_task]
  const int32_t* n_gram; // [n_task]
  const int32_t* group_task;   // [G]
  int n_task, G, B, V, E, H, NG;
  int act_b;             // sequences per pass of the hidden layer
  int act_n;             // doubles of LDS for a pass: act_b * (NG - 1) * H
  int tab_n;             // doubles of LDS for the task's input tables (TL), 0: they are read through L2
  int K;                 // steps per block: uniforms are fetched, tokens and log-probabilities written out, once per K steps
  int o_lds;             // doubles of LDS for the logits (0: register (B = 1) or scratch)
  double* scratch;       // [blocks][B][block] when the logits do not fit LDS
  uint64_t seed, gid_base, tick;
  const uint64_t* tick_dev;
  uint32_t* err;
};

// One DPP move of a double (two dwords); a lane the control leaves without a source, or a row the mask excludes, reads 0.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double ml_dpp(double x) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, ROW_MASK, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, ROW_MASK, 0xF, false);
  return __hiloint2double(hi, lo);
}

// inclusive scan over the wave's 64 lanes: four shifts inside the rows of 16, then the rows' totals carried over
__device__ __forceinline__ double ml_wave_scan(double x) {
  x += ml_dpp<0x111, 0xF>(x);      // row_shr:1
  x += ml_dpp<0x112, 0xF>(x);      // row_shr:2
  x += ml_dpp<0x114, 0xF>(x);      // row_shr:4
  x += ml_dpp<0x118, 0xF>(x);      // row_shr:8
  x += ml_dpp<0x142, 0xA>(x);      // row_bcast:15 -> rows 1 and 3
  x += ml_dpp<0x143, 0xC>(x);      // row_bcast:31 -> rows 2 and 3
  return x;
}

__device__ __forceinline__ double ml_wave_sum(double x) {      // the scan's last lane, to every lane
  const double s = ml_wave_scan(x);
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(s), 63), __builtin_amdgcn_readlane(__double2loint(s), 63));
}

// tokens: int32 [G][B][L+1], written by generate, read by teacher forcing.  logp: float64 [G][B][L], nullable for generate.
// u_in: float64 [G][B][L] injected uniforms or nullptr (Philox).  Steps [t0, t1) of the group, t0 = blockIdx.y * chunk.
template <int BLOCK, int HR, bool B1, bool TEACHER, bool TL>
__global__ __launch_bounds__(BLOCK) void metalang_kernel(MLArgs P, int L, int chunk, const double* __restrict__ u_in,
                                                         int32_t* tokens, double* __restrict__ logp) {
  extern __shared__ double ml_smem[];
  constexpr int NW = BLOCK / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = blockIdx.x;
  const int B = P.B, V = P.V, E = P.E, H = P.H, NG = P.NG;
  uint32_t err = 0u;
  int task = P.group_task[grp];
  if ((unsigned)task >= (unsigned)P.n_task) { err |= XV_DEVERR_ACTION_RANGE; task = 0; }
  int n = P.n_gram[task];
  if (n < 1 || n > NG) { err |= XV_DEVERR_ACTION_RANGE; n = n < 1 ? 1 : NG; }
  const double lam = P.lam[task];
  const double* emb = P.emb + (size_t)task * V * E;
  const double* w_in = P.w_in + (size_t)task * NG * E * H;
  const double* b_in = P.b_in + (size_t)task * NG * H;
  const double* w_out = P.w_out + (size_t)task * H * V;
  const bool col = tid < V;
  const double bo = col ? P.b_out[(size_t)task * V + tid] : 0.0;

  double* tab = ml_smem;                      // TL: word_emb [V][E], W_in [1 .. NG-1][E][H], b_in [1 .. NG-1][H]
  double* act = tab + (TL ? P.tab_n : 0);     // [act_b][n-1][H]
  double* hs = act + P.act_n;                 // [B][H]
  double* o_l = hs + B * H;                   // [B][BLOCK] when o_lds
  double* tot = o_l + P.o_lds;                // [NW][B] wave totals of e
  const int K = P.K, KT = P.K + NG;
  double* ubuf = tot + NW * B;                // [B][K] the uniforms of the block's steps
  double* lpbuf = ubuf + B * K;               // [B][K] the block's log-probabilities
  double* part = lpbuf + B * K;               // [NW][2] wave sums of o, o o
  int* hit = (int*)(part + 2 * NW);           // [NW][B] first column of the wave above u
  int* win = hit + NW * B;                    // [B][NG] window, oldest first (generate)
  int* tbuf = win + B * NG;                   // [B][K + NG] tokens tb - (NG - 1) .. tb + K of a block that starts at step tb
  double* ob = B1 ? nullptr
                  : (P.o_lds ? o_l : P.scratch + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)B * BLOCK);

  double wc[HR > 0 ? HR : 1];
  if (HR > 0) {
#pragma unroll
    for (int k = 0; k < HR; ++k) wc[k] = (col && k < H) ? w_out[(size_t)k * V + tid] : 0.0;
  }

  const int t0 = blockIdx.y * chunk;
  const int t1 = t0 + chunk < L ? t0 + chunk : L;
  const size_t seq0 = (size_t)grp * B;        // the group's first sequence
  if (!TEACHER) {
    for (int i = tid; i < B * NG; i += BLOCK) win[i] = 0;
    if (tid < B) tokens[(seq0 + tid) * (size_t)(L + 1)] = 0;
  }
  // slot 0 of the window has weight 0: the tables of slots 1 .. n-1 are all a step reads
  const double* embp = emb;
  const double* winp = w_in + (size_t)E * H;
  const double* binp = b_in + H;
  if (TL) {
    double* t_w = tab + V * E;
    double* t_b = t_w + (NG - 1) * E * H;
    for (int i = tid; i < V * E; i += BLOCK) tab[i] = emb[i];
    for (int i = tid; i < (n - 1) * E * H; i += BLOCK) t_w[i] = winp[i];
    for (int i = tid; i < (n - 1) * H; i += BLOCK) t_b[i] = binp[i];
    embp = tab; winp = t_w; binp = t_b;
  }
  __syncthreads();
  const uint64_t tick = TEACHER ? 0 : xv_launch_tick(P.tick, P.tick_dev);
  const double n_logit = (double)(B * V);

  // A barrier waits for the wave's outstanding global loads AND stores, so a step touches LDS only: what it reads from HBM
  // is fetched, and what it produces written out, once per block of K steps.
  for (int tb = t0; tb < t1; tb += K) {
   const int cnt = t1 - tb < K ? t1 - tb : K;
   if (TEACHER) {
     for (int i = tid; i < B * (cnt + NG); i += BLOCK) {
       const int b = i / (cnt + NG), q = i - b * (cnt + NG), ti = tb - (NG - 1) + q;
       int tok = ti < 0 ? 0 : tokens[(seq0 + b) * (size_t)(L + 1) + ti];
       if ((unsigned)tok >= (unsigned)V) { err |= XV_DEVERR_ACTION_RANGE; tok = 0; }
       tbuf[b * KT + q] = tok;
     }
   } else {
     for (int i = tid; i < B * cnt; i += BLOCK) {
       const int b = i / cnt, k = i - b * cnt, t = tb + k;
       double u;
       if (u_in) {
         u = u_in[(seq0 + b) * (size_t)L + t];
       } else {
         const xv_u32x4 w = xv_env_draw_sub(P.seed, P.gid_base + seq0 + b, tick, XV_DRAW_METALANG, (uint32_t)t >> 1);
         u = (t & 1) ? xv_u53(w.z, w.w) : xv_u53(w.x, w.y);
       }
       ubuf[b * K + k] = u;
     }
   }
   __syncthreads();
   for (int t = tb; t < tb + cnt; ++t) {
    const int kq = t - tb;      // the step's slot in ubuf / lpbuf; token t + 1 is tbuf[.][NG + kq]
    // ---- hidden layer: slots 1 .. n-1 of every window, P.act_b sequences per pass ----
    const int nh = (n - 1) * H;
    for (int b0 = 0; b0 < B; b0 += P.act_b) {
      const int nb = B - b0 < P.act_b ? B - b0 : P.act_b;
      for (int idx = tid; idx < nb * nh; idx += BLOCK) {
        const int bb = idx / nh, r = idx - bb * nh, g = 1 + r / H, j = r - (g - 1) * H;
        int tok;
        if (TEACHER) {      // slot g holds token t - (n - 1) + g of the given history
          tok = tbuf[(b0 + bb) * KT + kq - (n - 1) + g + NG - 1];
        } else {
          tok = win[(b0 + bb) * NG + g];
        }
        const double* er = embp + tok * E;
        const double* wg = winp + (g - 1) * E * H + j;
        double a0 = 0.0, a1 = 0.0;
        int e = 0;
        for (; e + 1 < E; e += 2) {
          a0 = fma(er[e], wg[e * H], a0);
          a1 = fma(er[e + 1], wg[(e + 1) * H], a1);
        }
        if (e < E) a0 = fma(er[e], wg[e * H], a0);
        double a = a0 + a1;
        a += binp[(g - 1) * H + j];
        act[idx] = (double)g * tanh(a);
      }
      __syncthreads();
      for (int idx = tid; idx < nb * H; idx += BLOCK) {
        const int bb = idx / H, j = idx - bb * H;
        double s = 0.0;
        for (int g = 1; g < n; ++g) s += act[bb * nh + (g - 1) * H + j];
        hs[(b0 + bb) * H + j] = s / (double)n;
      }
      __syncthreads();
    }
    // ---- logits of column tid, the two sums over the group ----
    double o1 = 0.0, lsum = 0.0, lsq = 0.0;
    if (col) {
      for (int b = 0; b < B; ++b) {
        const double* hb = hs + b * H;
        double a4[4] = {0.0, 0.0, 0.0, 0.0};      // four chains: a dependent fp64 FMA chain of H links is the step's longest
        if (HR > 0) {
#pragma unroll
          for (int k = 0; k < HR; ++k)
            if (k < H) a4[k & 3] = fma(hb[k], wc[k], a4[k & 3]);
        } else {
          for (int k = 0; k < H; ++k) a4[k & 3] = fma(hb[k], w_out[(size_t)k * V + tid], a4[k & 3]);
        }
        double a = (a4[0] + a4[1]) + (a4[2] + a4[3]);
        a += bo;
        if (B1) o1 = a;
        else ob[b * BLOCK + tid] = a;
        lsum += a;
        lsq += a * a;
      }
    }
    lsum = ml_wave_sum(lsum);
    lsq = ml_wave_sum(lsq);
    if (lane == 0) { part[2 * wave] = lsum; part[2 * wave + 1] = lsq; }
    __syncthreads();
    double sum = 0.0, sq = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) { sum += part[2 * w]; sq += part[2 * w + 1]; }
    const double mean = sum / n_logit, msq = sq / n_logit;
    const double sd = sqrt(msq - mean * mean);
    if (!(sd > 0.0) || !(sd <= 1.0e300)) err |= XV_DEVERR_NONFINITE;
    const double inv_sd = 1.0 / sd;
    // ---- exp; wave totals (and, for B = 1, the wave's scan) ----
    double e1 = 0.0, s1 = 0.0;
    if (B1) {
      e1 = col ? exp(lam * (inv_sd * (o1 - mean))) : 0.0;
      if (TEACHER) {
        s1 = ml_wave_sum(e1);
        if (lane == 0) tot[wave] = s1;
      } else {
        s1 = ml_wave_scan(e1);
        if (lane == 63) tot[wave] = s1;
      }
    } else {
      for (int b = 0; b < B; ++b) {
        const double e = col ? exp(lam * (inv_sd * (ob[b * BLOCK + tid] - mean))) : 0.0;
        if (col) ob[b * BLOCK + tid] = e;
        const double s = ml_wave_sum(e);
        if (lane == 0) tot[wave * B + b] = s;
      }
    }
    __syncthreads();
    // ---- the token ----
    if (TEACHER) {
      if (B1) {
        double S = 0.0;
#pragma unroll
        for (int w = 0; w < NW; ++w) S += tot[w];
        if (!(S <= 1.0e300)) err |= XV_DEVERR_NONFINITE;
        if (tid == tbuf[NG + kq]) lpbuf[kq] = log(e1 / S);
      } else if (tid < B) {
        double S = 0.0;
        for (int w = 0; w < NW; ++w) S += tot[w * B + tid];
        if (!(S <= 1.0e300)) err |= XV_DEVERR_NONFINITE;
        lpbuf[tid * K + kq] = log(ob[tid * BLOCK + tbuf[tid * KT + NG + kq]] / S);
      }
      __syncthreads();      // tot, hs and the logits are rewritten by the next position
    } else {
      if (B1) {
        double S = 0.0, off = 0.0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          const double x = tot[w];
          if (w < wave) off += x;
          S += x;
        }
        if (!(S <= 1.0e300)) err |= XV_DEVERR_NONFINITE;
        const unsigned long long m = __ballot(col && (off + s1) / S > ubuf[kq]);
        if (lane == 0) hit[wave] = m ? wave * 64 + (__ffsll((long long)m) - 1) : 0x7fffffff;
        __syncthreads();
        int nxt = 0x7fffffff;
#pragma unroll
        for (int w = 0; w < NW; ++w) nxt = hit[w] < nxt ? hit[w] : nxt;
        if (nxt == 0x7fffffff) nxt = 0;      // argmax of an all-false row
        if (tid == nxt) {
          tbuf[NG + kq] = nxt;
          if (logp) lpbuf[kq] = log(e1 / S);
          for (int g = 1; g < n - 1; ++g) win[g] = win[g + 1];
          win[n - 1] = nxt;
        }
      } else {
        for (int b = 0; b < B; ++b) {
          double S = 0.0, off = 0.0;
          for (int w = 0; w < NW; ++w) {
            const double x = tot[w * B + b];
            if (w < wave) off += x;
            S += x;
          }
          const double s = ml_wave_scan(col ? ob[b * BLOCK + tid] : 0.0);
          const unsigned long long m = __ballot(col && (off + s) / S > ubuf[b * K + kq]);
          if (lane == 0) hit[wave * B + b] = m ? wave * 64 + (__ffsll((long long)m) - 1) : 0x7fffffff;
        }
        __syncthreads();
        if (tid < B) {
          double S = 0.0;
          int nxt = 0x7fffffff;
          for (int w = 0; w < NW; ++w) {
            S += tot[w * B + tid];
            nxt = hit[w * B + tid] < nxt ? hit[w * B + tid] : nxt;
          }
          if (!(S <= 1.0e300)) err |= XV_DEVERR_NONFINITE;
          if (nxt == 0x7fffffff) nxt = 0;
          tbuf[tid * KT + NG + kq] = nxt;
          if (logp) lpbuf[tid * K + kq] = log(ob[tid * BLOCK + nxt] / S);
          int* wb = win + tid * NG;
          for (int g = 1; g < n - 1; ++g) wb[g] = wb[g + 1];
          wb[n - 1] = nxt;
        }
      }
      __syncthreads();      // the window is read, and tot / hit rewritten, by the next step
    }
   }
   for (int i = tid; i < B * cnt; i += BLOCK) {      // the block's results, in rows of cnt
     const int b = i / cnt, k = i - b * cnt;
     if (!TEACHER) tokens[(seq0 + b) * (size_t)(L + 1) + tb + 1 + k] = tbuf[b * KT + NG + k];
     if (logp) logp[(seq0 + b) * (size_t)L + tb + k] = lpbuf[b * K + k];
   }
  }
  if (err) atomicOr(P.err, err);
}

#ifndef XV_KERNELS_ONLY
#include <cstdlib>
#include <new>

struct xv_metalang {
  xv_engine* eng;
  MLArgs a;
  bool task_set;
  double* scratch;
  size_t scratch_bytes;
};

static int ml_block(int V) { return V <= 64 ? 64 : V <= 256 ? 256 : 1024; }

// dynamic LDS of a workgroup (the carve-up at the head of metalang_kernel), with tab_n doubles of tables
static size_t ml_lds_bytes(const MLArgs& a, int tab_n) {
  const int nw = ml_block(a.V) / 64;
  return sizeof(double) * ((size_t)tab_n + a.act_n + (size_t)a.B * a.H + a.o_lds + (size_t)nw * a.B + 2 * (size_t)a.B * a.K +
                           2 * nw) +
         sizeof(int) * ((size_t)nw * a.B + (size_t)a.B * a.NG + (size_t)a.B * (a.K + a.NG));
}

extern "C" int xv_metalang_create(xv_engine* e, int n_group, int seqs_per_group, int n_vocab, int n_emb, int n_hidden,
                                  int n_gram_max, xv_metalang** out) {
  XV_CHECK_ARG(out != nullptr);
  *out = nullptr;
  XV_CHECK_ARG(n_group >= 1);      // e == nullptr: a handle that only describes (xv_metalang_describe), no GPU needed
  const struct { const char* name; int v, hi; } lim[5] = {{"n_vocab", n_vocab, ML_V_MAX}, {"n_hidden", n_hidden, ML_H_MAX},
                                                         {"n_emb", n_emb, ML_E_MAX}, {"n_gram", n_gram_max, ML_NG_MAX},
                                                         {"seqs_per_group", seqs_per_group, ML_B_MAX}};
  for (int i = 0; i < 5; ++i)
    if (lim[i].v < 1 || lim[i].v > lim[i].hi) {
      xv_set_error("xv_metalang_create: %s = %d is outside the supported range 1 .. %d", lim[i].name, lim[i].v, lim[i].hi);
      return XV_ERR_UNSUPPORTED;
    }
  xv_metalang* h = new (std::nothrow) xv_metalang();
  if (!h) {
    xv_set_error("xv_metalang_create: out of host memory");
    return XV_ERR_NOMEM;
  }
  h->eng = e;
  h->task_set = false;
  h->scratch = nullptr;
  h->scratch_bytes = 0;
  MLArgs& a = h->a;
  a = MLArgs();
  a.G = n_group; a.B = seqs_per_group; a.V = n_vocab; a.E = n_emb; a.H = n_hidden; a.NG = n_gram_max;
  const int per_seq = (n_gram_max > 1 ? n_gram_max - 1 : 1) * n_hidden;
  a.act_b = ML_ACT_CAP / per_seq < seqs_per_group ? ML_ACT_CAP / per_seq : seqs_per_group;
  if (a.act_b < 1) a.act_b = 1;
  a.act_n = a.act_b * per_seq;
  a.K = seqs_per_group <= 8 ? 64 : 8;      // LDS: 20 bytes per sequence and step
  // XV_METALANG_TABLES=l2 keeps the input tables out of LDS: the A/B switch of scripts/bench_metalang.py
  const char* where = getenv("XV_METALANG_TABLES");
  const int tab = n_vocab * n_emb + (n_gram_max - 1) * (n_emb * n_hidden + n_hidden);
  a.tab_n = 0;      // set below, once the rest of the workgroup's LDS is known
  const int ob = seqs_per_group * ml_block(n_vocab);
  a.o_lds = seqs_per_group > 1 && ob <= ML_O_LDS_CAP ? ob : 0;
  // the tables go to LDS where the workgroup then stays within 64 KiB (two and more workgroups per CU)
  if (tab <= ML_TAB_CAP && !(where && where[0] == 'l' && where[1] == '2') && ml_lds_bytes(a, tab) <= 65536) a.tab_n = tab;
  a.err = e ? e->d_err : nullptr;
  *out = h;
  return XV_OK;
}

extern "C" int xv_metalang_destroy(xv_metalang* h) {
  if (!h) return XV_OK;
  if (h->eng) {
    (void)hipSetDevice(h->eng->device);
    (void)hipStreamSynchronize(h->eng->stream);
  }
  if (h->scratch) (void)hipFree(h->scratch);
  delete h;
  return XV_OK;
}

extern "C" int xv_metalang_set_task(xv_metalang* h, int n_task, const double* word_emb, const double* weights_inputlayer,
                                    const double* bias_inputlayer, const double* weights_outputlayer,
                                    const double* bias_outputlayer, const double* lambda, const int32_t* n_gram,
                                    const int32_t* group_task) {
  XV_CHECK_ARG(h != nullptr && n_task >= 1);
  XV_CHECK_ARG(word_emb && weights_inputlayer && bias_inputlayer && weights_outputlayer && bias_outputlayer && lambda &&
               n_gram && group_task);
  MLArgs& a = h->a;
  a.n_task = n_task;
  a.emb = word_emb; a.w_in = weights_inputlayer; a.b_in = bias_inputlayer; a.w_out = weights_outputlayer;
  a.b_out = bias_outputlayer; a.lam = lambda; a.n_gram = n_gram; a.group_task = group_task;
  h->task_set = true;
  return XV_OK;
}

// What a call launches: the template parameters of metalang_kernel and the run-time layouts, all of them a function of the
// handle's sizes and of which call it is.  ml_run launches from it and xv_metalang_describe reports it.
struct MLPlan {
  int block;       // threads: 64, 256, 1024
  int hr;          // doubles of the W_out column in registers, 0: read through L2
  bool b1;         // B == 1: the logit is a register
  bool teacher;
  bool tl;         // the input tables are copied to LDS
  int K;           // steps between two rounds of I/O
  int o_where;     // the logits of a group: 0 a register, 1 LDS, 2 HBM scratch
  int act_b;       // sequences per pass of the hidden layer
  size_t lds;      // dynamic LDS of a workgroup; above 65536 the kernel needs hipFuncSetAttribute
  int chunk;       // positions per workgroup, 0: the whole call
};

// the W_out column lives in registers (HR = 16, 32, 64 doubles) for V <= 256 and H <= 64; a 1024-thread block has 128
// VGPRs per lane and a column of H > 64 takes more than 128: those read W_out through L2
static MLPlan ml_plan(const MLArgs& a, bool teacher) {
  MLPlan p;
  p.block = ml_block(a.V);
  p.hr = p.block == 1024 || a.H > 64 ? 0 : a.H <= 16 ? 16 : a.H <= 32 ? 32 : 64;
  p.b1 = a.B == 1;
  p.teacher = teacher;
  p.tl = a.tab_n != 0;
  p.K = a.K;
  p.o_where = a.B == 1 ? 0 : a.o_lds ? 1 : 2;
  p.act_b = a.act_b;
  p.lds = ml_lds_bytes(a, a.tab_n);
  p.chunk = teacher ? ML_TEACHER_CHUNK : 0;
  return p;
}

struct MLCall {
  xv_metalang* h;
  const MLArgs& a;
  const MLPlan& p;
  dim3 grid;
  int L, chunk;
  const double* u;
  int32_t* tokens;
  double* logp;
};

template <int BLOCK, int HR, bool B1, bool TEACHER, bool TL>
static int ml_launch_k(const MLCall& c) {
  auto k = metalang_kernel<BLOCK, HR, B1, TEACHER, TL>;
  if (c.p.lds > 65536) XV_HIP(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.p.lds));
  hipLaunchKernelGGL(k, c.grid, dim3(BLOCK), c.p.lds, c.h->eng->stream, c.a, c.L, c.chunk, c.u, c.tokens, c.logp);
  XV_LAUNCH_CHECK();
  return XV_OK;
}

template <int BLOCK, int HR, bool B1>
static int ml_launch_t(const MLCall& c) {
  if (c.p.tl) return c.p.teacher ? ml_launch_k<BLOCK, HR, B1, true, true>(c) : ml_launch_k<BLOCK, HR, B1, false, true>(c);
  return c.p.teacher ? ml_launch_k<BLOCK, HR, B1, true, false>(c) : ml_launch_k<BLOCK, HR, B1, false, false>(c);
}

template <int BLOCK, int HR>
static int ml_launch_b(const MLCall& c) {
  return c.p.b1 ? ml_launch_t<BLOCK, HR, true>(c) : ml_launch_t<BLOCK, HR, false>(c);
}

template <int BLOCK>
static int ml_launch_h(const MLCall& c) {
  if (c.p.hr == 16) return ml_launch_b<BLOCK, 16>(c);
  if (c.p.hr == 32) return ml_launch_b<BLOCK, 32>(c);
  if (c.p.hr == 64) return ml_launch_b<BLOCK, 64>(c);
  return ml_launch_b<BLOCK, 0>(c);
}

static int ml_run(xv_metalang* h, const char* who, bool teacher, int L, const double* u, int32_t* tokens, double* logp) {
  if (!h->eng) {
    xv_set_error("%s: the handle was made without an engine: it only describes (xv_metalang_describe)", who);
    return XV_ERR_INVALID;
  }
  if (!h->task_set) {
    xv_set_error("%s: no task set (xv_metalang_set_task)", who);
    return XV_ERR_INVALID;
  }
  xv_engine* e = h->eng;
  XV_HIP(hipSetDevice(e->device));
  MLArgs a = h->a;
  const MLPlan p = ml_plan(a, teacher);
  const int chunk = p.chunk ? p.chunk : L;
  const dim3 grid((unsigned)a.G, (unsigned)((L + chunk - 1) / chunk));
  if (p.o_where == 2) {
    const size_t need = sizeof(double) * (size_t)grid.x * grid.y * a.B * p.block;
    if (need > h->scratch_bytes) {
      XV_HIP(hipStreamSynchronize(e->stream));
      if (h->scratch) (void)hipFree(h->scratch);
      h->scratch = nullptr;
      h->scratch_bytes = 0;
      hipError_t r = hipMalloc(&h->scratch, need);
      if (r != hipSuccess) {
        (void)hipGetLastError();
        xv_set_error("%s: %zu bytes of logit scratch do not fit: %s", who, need, hipGetErrorString(r));
        return r == hipErrorOutOfMemory ? XV_ERR_NOMEM : XV_ERR_HIP;
      }
      h->scratch_bytes = need;
    }
    a.scratch = h->scratch;
  }
  if (!teacher) {
    const XvTickBind tb = xv_engine_bind_tick(e, 1);
    a.tick = tb.tick;
    a.tick_dev = tb.tick_dev;
    a.seed = e->seed;
    a.gid_base = e->env_id_base;
  }
  const MLCall c = {h, a, p, grid, L, chunk, u, tokens, logp};
  if (p.block == 64) return ml_launch_h<64>(c);
  if (p.block == 256) return ml_launch_h<256>(c);
  return ml_launch_b<1024, 0>(c);
}

extern "C" int xv_metalang_describe(const xv_metalang* h, int teacher, int32_t out[10]) {
  XV_CHECK_ARG(h != nullptr && out != nullptr && (teacher == 0 || teacher == 1));
  const MLPlan p = ml_plan(h->a, teacher != 0);
  out[0] = p.block; out[1] = p.hr; out[2] = p.b1; out[3] = p.tl; out[4] = p.K; out[5] = p.o_where; out[6] = p.act_b;
  out[7] = (int32_t)p.lds; out[8] = p.lds > 65536; out[9] = p.chunk;
  return XV_OK;
}

extern "C" int xv_metalang_generate(xv_metalang* h, int L, const double* u, int32_t* tokens, double* logp) {
  XV_CHECK_ARG(h != nullptr && L >= 1 && tokens != nullptr);
  return ml_run(h, __func__, false, L, u, tokens, logp);
}

extern "C" int xv_metalang_log_prob(xv_metalang* h, int L, const int32_t* tokens, double* logp) {
  XV_CHECK_ARG(h != nullptr && L >= 1 && tokens != nullptr && logp != nullptr);
  return ml_run(h, __func__, true, L, nullptr, const_cast<int32_t*>(tokens), logp);
}
#endif
