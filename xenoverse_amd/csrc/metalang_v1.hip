// metalang_v1.hip — MetaLangV1 on the device: the reference's pattern-recovery (denoising) generator
// (xenoverse/metalang/metalangv1.py:39-74).  Host restatement and the full statement of the semantics:
// xenoverse_amd/metalang/host_v1.py.  A task is a handful of integer patterns (CSR tables); a sequence is a STREAM of
// positions q = 0 .. L: segment k is pattern p_k followed by one separator (token 0) and starts at start_k = sum_{j<k}
// (len(p_j) + 1); segments are drawn while start_k < L + 1.  features[q] (q < L) is the stream's token corrupted
// (noise_value where u_noise < error_ratio, 0 instead where also u_mask < mask_ratio; separators untouched), labels[q - 1]
// (q >= 1) the clean token.  Integer work and two strict fp64 comparisons: equal to the reference bit for bit.
//
// Kernel: one workgroup of 256 threads per sequence, the stream in tiles of ML1_TILE = 1024 positions (a quad of positions
// per thread: one 16-byte store per row and thread).  Per tile
//   1. wave 0 extends the segment table in LDS until it covers the tile: 64 segments per pass, one pattern index per lane,
//      a wave-inclusive scan of len + 1 with the running start carried from pass to pass; the segment that straddles the
//      tile's start is kept from the tile before, so the table never holds more than ML1_TILE + 2 segments, whatever L is
//   2. every thread finds the segment of its first position by bisection, walks on from there, and puts the clean token, the
//      feature and the kind of its positions into LDS (the clean token of the tile's position ML1_TILE as well: the last label)
//   3. the rows are written from LDS: labels is the clean stream one position later, so both rows of a tile start at the
//      same row offset; 16-byte stores where the address allows, single words at an unaligned head or tail (odd L)
// Stores are the whole cost: 9 bytes per position.
//
// Free-running draws, Philox4x32-10 keyed by (engine seed, global sequence id = env_id_base + sequence, the call's tick,
// purpose, sub) through xv_env_draw_sub (csrc/philox.h):
//   XV_DRAW_ML1_SEGMENT 10  sub = k >> 2, word k & 3 = w: pattern index of segment k = (uint64(w) * n_patterns) >> 32
//   XV_DRAW_ML1_VALUE   11  sub = q >> 2, word q & 3 = w: noise_value of position q = (uint64(w) * n_vocab) >> 32
//   XV_DRAW_ML1_NOISE   12  sub = q >> 1, words 0,1 (q even) or 2,3 (q odd): u_noise = xv_u53
//   XV_DRAW_ML1_MASK    13  sub = q >> 1, likewise: u_mask
// An integer in [0, n) from one word is biased by at most n / 2^32 (relative, per value).
#include "philox.h"
#include "xv_common.h"

#define XV_DRAW_ML1_SEGMENT 10u
#define XV_DRAW_ML1_VALUE 11u
#define XV_DRAW_ML1_NOISE 12u
#define XV_DRAW_ML1_MASK 13u

#define ML1_BLOCK 256
#define ML1_TILE 1024                 // positions per tile: 4 per thread
#define ML1_TAB (ML1_TILE + 2 + 64)   // segments of a tile (each at least one position), the straddling one, one pass of slack
#define ML1_L_MAX (1 << 24)

struct ML1Args {
  const int32_t* task_pattern_start;   // [n_task + 1]
  const int32_t* pattern_start;        // [n_pattern_total + 1]
  const int32_t* pattern_tokens;       // [n_token_total]
  const int32_t* n_vocab;              // [n_task]
  const double* error_ratio;           // [n_task]
  const int32_t* seq_task;             // [n_seq]
  int n_task, n_pattern_total, n_token_total, n_seq;
  uint64_t seed, gid_base, tick;
  const uint64_t* tick_dev;
  uint32_t* err;
};

struct ML1Draws {      // injected: all four or none
  const int32_t* pattern_index;   // [n_seq][n_slot]
  const int32_t* noise_value;     // [n_seq][L + 1]
  const double* u_noise;          // [n_seq][L + 1]
  const double* u_mask;           // [n_seq][L + 1]
  int n_slot;
};

__device__ __forceinline__ int ml1_wave_scan(int x, int lane) {      // inclusive, 64 lanes
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  return x;
}

// n elements of LDS to a row in global memory: 16-byte stores where the address allows, single words before and after
__device__ __forceinline__ void ml1_store_row(int32_t* __restrict__ dst, const int32_t* src, int n, int tid) {
  int head = (int)((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u) >> 2;      // words up to the first 16-byte boundary
  if (head > n) head = n;
  const int nvec = (n - head) >> 2;
  if (tid < head) dst[tid] = src[tid];
  int4* d4 = reinterpret_cast<int4*>(dst + head);
  for (int v = tid; v < nvec; v += ML1_BLOCK) {
    const int32_t* s = src + head + 4 * v;
    d4[v] = make_int4(s[0], s[1], s[2], s[3]);
  }
  const int done = head + 4 * nvec;
  if (tid < n - done) dst[done + tid] = src[done + tid];
}

template <bool INJ>
__global__ __launch_bounds__(ML1_BLOCK) void metalang1_kernel(ML1Args P, ML1Draws D, int L, double mask_ratio,
                                                              int32_t* __restrict__ features, int32_t* __restrict__ labels,
                                                              uint8_t* __restrict__ kinds, int32_t* __restrict__ n_segments) {
  __shared__ int seg_start[ML1_TAB + 1];      // start of the table's segments, and the start of the one after the last
  __shared__ int seg_tok[ML1_TAB];            // offset of the segment's pattern in pattern_tokens
  __shared__ int s_clean[ML1_TILE + 4];
  __shared__ int s_feat[ML1_TILE];
  __shared__ uint8_t s_kind[ML1_TILE];
  __shared__ int s_ntab;
  const int tid = threadIdx.x, lane = tid & 63;
  const int seq = blockIdx.x;
  uint32_t err = 0u;
  int task = P.seq_task[seq];
  if ((unsigned)task >= (unsigned)P.n_task) { err |= XV_DEVERR_ACTION_RANGE; task = 0; }
  // the task's patterns: [p0, p0 + nP) of pattern_start, kept inside the table whatever it holds
  int p0 = P.task_pattern_start[task], nP = P.task_pattern_start[task + 1] - p0;
  if (p0 < 0 || p0 >= P.n_pattern_total || nP < 1 || nP > P.n_pattern_total - p0) {
    err |= XV_DEVERR_ACTION_RANGE;
    p0 = p0 < 0 ? 0 : (p0 >= P.n_pattern_total ? P.n_pattern_total - 1 : p0);
    nP = nP < 1 ? 1 : (nP > P.n_pattern_total - p0 ? P.n_pattern_total - p0 : nP);
  }
  int V = P.n_vocab[task];
  if (V < 1) { err |= XV_DEVERR_ACTION_RANGE; V = 1; }
  const double e_ratio = P.error_ratio[task];
  const uint64_t gid = P.gid_base + (uint64_t)seq;
  const uint64_t tick = INJ ? 0 : xv_launch_tick(P.tick, P.tick_dev);
  const size_t row = (size_t)seq * (size_t)L, drow = (size_t)seq * (size_t)(L + 1);

  // wave 0's running state (uniform over the wave): the next segment to draw and where it starts; entries in the table
  int k_next = 0, pos_next = 0, n_tab = 0;

  for (int tb = 0; tb < L; tb += ML1_TILE) {
    const int te = tb + ML1_TILE < L ? tb + ML1_TILE : L;      // the tile needs positions tb .. te (te <= L) clean
    if (tid < 64) {
      if (n_tab > 1) {      // keep the last segment: it is the only one that reaches position tb
        const int s = seg_start[n_tab - 1], t = seg_tok[n_tab - 1];
        seg_start[0] = s;
        seg_tok[0] = t;
        n_tab = 1;
      }
      while (pos_next <= te) {
        const int k = k_next + lane;
        int pi;
        bool bad = false;
        if (INJ) {
          pi = k < D.n_slot ? D.pattern_index[(size_t)seq * D.n_slot + k] : 0;
          bad = k >= D.n_slot || (unsigned)pi >= (unsigned)nP;
          if ((unsigned)pi >= (unsigned)nP) pi = 0;
        } else {
          const xv_u32x4 w = xv_env_draw_sub(P.seed, gid, tick, XV_DRAW_ML1_SEGMENT, (uint32_t)k >> 2);
          const uint32_t ws = (k & 3) == 0 ? w.x : (k & 3) == 1 ? w.y : (k & 3) == 2 ? w.z : w.w;
          pi = (int)(((uint64_t)ws * (uint64_t)(uint32_t)nP) >> 32);
        }
        int a = P.pattern_start[p0 + pi], len = P.pattern_start[p0 + pi + 1] - a;
        bool bad_tab = false;
        if (a < 0 || a > P.n_token_total || len < 0 || len > P.n_token_total - a) {
          bad_tab = true;
          a = a < 0 ? 0 : (a > P.n_token_total ? P.n_token_total : a);
          len = len < 0 ? 0 : (len > P.n_token_total - a ? P.n_token_total - a : len);
        }
        if (len > L + 1) len = L + 1;      // positions beyond L are never asked for: the sums below stay far from 2^31
        const int incl = ml1_wave_scan(len + 1, lane);
        const int start = pos_next + incl - (len + 1);
        const bool in = start <= te;      // a prefix of the lanes, lane 0 always: these segments are drawn (start < L + 1)
        if (in && (bad || bad_tab)) err |= XV_DEVERR_ACTION_RANGE;
        const int cnt = __popcll(__ballot(in));
        if (in) {
          seg_start[n_tab + lane] = start;
          seg_tok[n_tab + lane] = a;
        }
        pos_next += __shfl(incl, cnt - 1, 64);
        n_tab += cnt;
        k_next += cnt;
      }
      if (lane == 0) {
        seg_start[n_tab] = pos_next;
        s_ntab = n_tab;
      }
    }
    __syncthreads();
    const int nt = s_ntab;
    const int npos = te - tb + 1;      // positions tb .. te; the last one only for its clean token (unless te < ... below)
    for (int i = tid; 4 * i < npos; i += ML1_BLOCK) {
      const int q0 = tb + 4 * i;
      int lo = 0, hi = nt - 1;      // the last segment with seg_start <= q0
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg_start[mid] <= q0) lo = mid; else hi = mid - 1;
      }
      int j = lo;
      xv_u32x4 wv = {0u, 0u, 0u, 0u}, wn = wv, wm = wv;
      if (!INJ) wv = xv_env_draw_sub(P.seed, gid, tick, XV_DRAW_ML1_VALUE, (uint32_t)q0 >> 2);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = q0 + r;
        if (q > te) break;
        if (!INJ && (r & 1) == 0) {      // q is even: one call serves the pair q, q + 1; the mask's only where one is replaced
          wn = xv_env_draw_sub(P.seed, gid, tick, XV_DRAW_ML1_NOISE, (uint32_t)q >> 1);
          if (xv_u53(wn.x, wn.y) < e_ratio || xv_u53(wn.z, wn.w) < e_ratio)
            wm = xv_env_draw_sub(P.seed, gid, tick, XV_DRAW_ML1_MASK, (uint32_t)q >> 1);
        }
        while (j + 1 < nt && seg_start[j + 1] <= q) ++j;
        const int off = q - seg_start[j];
        const int len = seg_start[j + 1] - seg_start[j] - 1;
        const bool sep = off >= len;
        int c = 0;
        if (!sep) c = P.pattern_tokens[seg_tok[j] + off];
        s_clean[q - tb] = c;
        if (q < L && q - tb < ML1_TILE) {
          int f = c, kind = 3;
          if (!sep) {
            int nv;
            double un, um = 1.0;
            if (INJ) {
              nv = D.noise_value[drow + q];
              un = D.u_noise[drow + q];
              um = D.u_mask[drow + q];
              if ((unsigned)nv >= (unsigned)V) { err |= XV_DEVERR_ACTION_RANGE; nv = nv < 0 ? 0 : V - 1; }
            } else {
              const uint32_t ws = r == 0 ? wv.x : r == 1 ? wv.y : r == 2 ? wv.z : wv.w;
              nv = (int)(((uint64_t)ws * (uint64_t)(uint32_t)V) >> 32);
              un = (r & 1) ? xv_u53(wn.z, wn.w) : xv_u53(wn.x, wn.y);
            }
            const bool rep = un < e_ratio;
            if (!INJ && rep) um = (r & 1) ? xv_u53(wm.z, wm.w) : xv_u53(wm.x, wm.y);
            const bool msk = rep && um < mask_ratio;
            f = msk ? 0 : (rep ? nv : c);
            kind = msk ? 2 : (rep ? 1 : 0);
          }
          s_feat[q - tb] = f;
          s_kind[q - tb] = (uint8_t)kind;
        }
      }
    }
    __syncthreads();
    const int nf = (L < tb + ML1_TILE ? L : tb + ML1_TILE) - tb;      // features tb .. tb + nf - 1; labels the same indices
    ml1_store_row(features + row + tb, s_feat, nf, tid);
    ml1_store_row(labels + row + tb, s_clean + 1, nf, tid);
    if (kinds) {
      for (int i = tid; i < nf; i += ML1_BLOCK) kinds[row + tb + i] = s_kind[i];
    }
    // the next tile's table pass touches seg_* only after every wave has passed the barrier above, and its fill writes
    // s_* only after the barrier behind that pass, which every wave reaches with these stores' LDS reads done
  }
  if (n_segments && tid == 0) n_segments[seq] = k_next;
  if (err) atomicOr(P.err, err);
}

#ifndef XV_KERNELS_ONLY
#include <new>

struct xv_metalang1 {
  xv_engine* eng;
  ML1Args a;
  bool task_set;
};

extern "C" int xv_metalang1_create(xv_engine* e, int n_seq, xv_metalang1** out) {
  XV_CHECK_ARG(out != nullptr);
  *out = nullptr;
  XV_CHECK_ARG(e != nullptr && n_seq >= 1);
  xv_metalang1* h = new (std::nothrow) xv_metalang1();
  if (!h) {
    xv_set_error("xv_metalang1_create: out of host memory");
    return XV_ERR_NOMEM;
  }
  h->eng = e;
  h->task_set = false;
  h->a = ML1Args();
  h->a.n_seq = n_seq;
  h->a.err = e->d_err;
  *out = h;
  return XV_OK;
}

extern "C" int xv_metalang1_destroy(xv_metalang1* h) {
  if (!h) return XV_OK;
  (void)hipSetDevice(h->eng->device);
  (void)hipStreamSynchronize(h->eng->stream);
  delete h;
  return XV_OK;
}

extern "C" int xv_metalang1_set_task(xv_metalang1* h, int n_task, int n_pattern_total, int n_token_total,
                                     const int32_t* task_pattern_start, const int32_t* pattern_start,
                                     const int32_t* pattern_tokens, const int32_t* n_vocab, const double* error_ratio,
                                     const int32_t* seq_task) {
  XV_CHECK_ARG(h != nullptr && n_task >= 1 && n_pattern_total >= 1 && n_token_total >= 1);
  XV_CHECK_ARG(task_pattern_start && pattern_start && pattern_tokens && n_vocab && error_ratio && seq_task);
  ML1Args& a = h->a;
  a.n_task = n_task; a.n_pattern_total = n_pattern_total; a.n_token_total = n_token_total;
  a.task_pattern_start = task_pattern_start; a.pattern_start = pattern_start; a.pattern_tokens = pattern_tokens;
  a.n_vocab = n_vocab; a.error_ratio = error_ratio; a.seq_task = seq_task;
  h->task_set = true;
  return XV_OK;
}

extern "C" int xv_metalang1_generate(xv_metalang1* h, int L, double mask_ratio, const int32_t* pattern_index, int n_slot,
                                     const int32_t* noise_value, const double* u_noise, const double* u_mask,
                                     int32_t* features, int32_t* labels, uint8_t* kinds, int32_t* n_segments) {
  XV_CHECK_ARG(h != nullptr && features != nullptr && labels != nullptr);
  if (L < 1 || L > ML1_L_MAX) {
    xv_set_error("xv_metalang1_generate: L = %d is outside the supported range 1 .. %d", L, ML1_L_MAX);
    return XV_ERR_UNSUPPORTED;
  }
  const int given = (pattern_index != nullptr) + (noise_value != nullptr) + (u_noise != nullptr) + (u_mask != nullptr);
  if (given != 0 && given != 4) {
    xv_set_error("xv_metalang1_generate: injected draws are all four arrays or none");
    return XV_ERR_INVALID;
  }
  XV_CHECK_ARG(given == 0 || n_slot >= 1);
  if (!h->task_set) {
    xv_set_error("xv_metalang1_generate: no task set (xv_metalang1_set_task)");
    return XV_ERR_INVALID;
  }
  xv_engine* e = h->eng;
  XV_HIP(hipSetDevice(e->device));
  ML1Args a = h->a;
  const XvTickBind tb = xv_engine_bind_tick(e, 1);
  a.tick = tb.tick;
  a.tick_dev = tb.tick_dev;
  a.seed = e->seed;
  a.gid_base = e->env_id_base;
  ML1Draws d = {pattern_index, noise_value, u_noise, u_mask, n_slot};
  if (given)
    hipLaunchKernelGGL(metalang1_kernel<true>, dim3((unsigned)a.n_seq), dim3(ML1_BLOCK), 0, e->stream, a, d, L, mask_ratio,
                       features, labels, kinds, n_segments);
  else
    hipLaunchKernelGGL(metalang1_kernel<false>, dim3((unsigned)a.n_seq), dim3(ML1_BLOCK), 0, e->stream, a, d, L, mask_ratio,
                       features, labels, kinds, n_segments);
  XV_LAUNCH_CHECK();
  return XV_OK;
}
#endif
