// metalm_pass.h — ONE PASS BY ONE WAVE: the token step of metalm.hip (its header text states the semantics), shared by
// metalm_kernel (one pass per wave and call) and metalm_stream_kernel (pass after pass until the env's training stream is
// full).  Included by metalm.hip behind what the pass is made of: the sizes and LMArgs, the wave primitives and lm_tanh.
#pragma once

// the workgroup's task tables: pointers into global memory, or (TL) into the copy all threads make in lm_tab; false and
// XV_DEVERR_ACTION_RANGE in err where the env's task index is out of range (task 0 then serves)
template <bool TL>
__device__ __forceinline__ void lm_tables(const LMArgs& P, int env, double* lm_tab, uint32_t& err, const double*& emb,
                                          const double*& w_h, const double*& b_h, const double*& w_d, const double*& b_d) {
  const int V = P.V, E = P.E, H = P.H;
  int task = P.env_task[env];
  if ((unsigned)task >= (unsigned)P.n_task) { err |= XV_DEVERR_ACTION_RANGE; task = 0; }
  emb = P.emb + (size_t)task * V * E;
  w_h = P.w_h + (size_t)task * (H + E) * H;
  b_h = P.b_h + (size_t)task * H;
  w_d = P.w_d + (size_t)task * H * V;
  b_d = P.b_d + (size_t)task * V;
  if (TL) {
    const int n0 = V * E, n1 = n0 + (H + E) * H, n2 = n1 + H, n3 = n2 + H * V, n4 = n3 + V;
    for (int i = threadIdx.x; i < n4; i += blockDim.x)
      lm_tab[i] = i < n0 ? emb[i] : i < n1 ? w_h[i - n0] : i < n2 ? b_h[i - n1] : i < n3 ? w_d[i - n2] : b_d[i - n3];
    emb = lm_tab; w_h = lm_tab + n0; b_h = lm_tab + n1; w_d = lm_tab + n2; b_d = lm_tab + n3;
  }
}

// what a pass takes besides the tables, and what it leaves
struct LMPass {
  int kind;                  // LM_QUERY .. LM_LOW
  bool skip;                 // no step at all
  int n_ans;                 // LM_LABEL: the given answer's length
  const int32_t* ans;        // LM_LABEL: the given answer (this env's row)
  const double* u;           // injected uniforms (this env's row of max_len + 1) or nullptr (Philox)
  uint64_t gid, tick;        // the Philox key's env and tick
  double temp0, temp1;       // the temperature of the first token and of the others
  int32_t* dst;              // the pass's tokens (this env's row); nullable
  // STREAM only: the tokens go to dst[at + pos] while at + pos < cap, and a second row dst2 takes, with `fuse`, the
  // n_step label tokens of the pass's own answer (the argmax of exp(logits) at every step), without it the tokens again
  int at, at2, cap;
  int32_t* dst2;
  bool fuse;
  // out
  int n_out, n_step;
  double ppl_sum, ppl_sum2;  // the sums of -log(max(p[token], 1e-10)): the pass's own and, fused, the label pass's
};

// ONE PASS BY ONE WAVE: the token steps from the state in hs (this wave's LDS row) until the stop token, max_len tokens or,
// teacher-forced, the end of the given answer.  STREAM: see LMPass.  With `fuse` a policy pass also does the label pass
// over its own answer: that pass (LM_LABEL given this pass's tokens) starts from the same state and is fed the same tokens,
// so it goes through the same hidden states, echo and stop biases and logits, and what it adds per step is written here
// in its own expressions — e = exp(logits), their sum by the wave scan, p = e / sum, the argmax, p[given] — where the
// given token of the last step is the stop token, also when the pass is cut at max_len.
template <bool STREAM>
__device__ __forceinline__ void lm_pass(const LMArgs& P, const double* emb, const double* w_h, const double* b_h,
                                        const double* w_d, const double* b_d, double* hs, const double* lm_tt, int lane,
                                        LMPass& A, uint32_t& err) {
  const int V = P.V, E = P.E, H = P.H, max_len = P.max_len;
  const int NC = (V + 63) >> 6;
  const int kind = A.kind;
  const int n_ans = A.n_ans;
  const double* u_in = A.u;
  const double temp0 = A.temp0, temp1 = A.temp1;
  const bool fuse = STREAM && A.fuse;

  bool col[LM_NC], fun[LM_NC];
  double bd[LM_NC], echo[LM_NC];
#pragma unroll
  for (int c = 0; c < LM_NC; ++c) {
    const int v = lane + 64 * c;
    col[c] = v < V;
    fun[c] = (P.fmask[c] >> lane) & 1ull;
    bd[c] = col[c] ? b_d[v] : 0.0;
    echo[c] = 0.0;
  }
  double bh[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) bh[r] = lane + 64 * r < H ? b_h[lane + 64 * r] : 0.0;

  // the last (H + E) mod 4 terms of a hidden row's dot product are the BLAS matvec's tail, added in its own order (with
  // H not a multiple of 4 that matvec sums its last H mod 4 rows in yet another order, which is not followed)
  const int m3 = (H & 3) ? 0 : (E & 3);
  double stop_bias = -1.0e+6, ppl_sum = 0.0, ppl_sum2 = 0.0;
  int tok_in = 0, n_out = 0, n_step = 0;
  bool done = A.skip;
  for (int tb = 0; !done; tb += 64) {
    // ---- this block's 64 positions: the uniform (or, teacher-forced, the given token) of position tb + lane ----
    const int pos = tb + lane;
    double u_l = 0.0;
    int a_l = P.stop;
    if (kind == LM_LABEL) {
      if (pos < n_ans) {
        a_l = A.ans[pos];
        if ((unsigned)a_l >= (unsigned)V) { err |= XV_DEVERR_ACTION_RANGE; a_l = P.stop; }
      }
    } else if (pos <= max_len) {
      if (u_in) {
        u_l = u_in[pos];
      } else {
        const xv_u32x4 w = xv_env_draw_sub(P.seed, A.gid, A.tick, XV_DRAW_METALM, ((uint32_t)kind << 16) | ((uint32_t)pos >> 1));
        u_l = (pos & 1) ? xv_u53(w.z, w.w) : xv_u53(w.x, w.y);
      }
    }
    int my_tok = 0, my_tok2 = 0;
    for (int k = 0; k < 64 && !done; ++k) {
      // ---- the hidden state: rows lane and lane + 64 ----
      const double* er = emb + tok_in * E;
      double hn[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int row = lane + 64 * r;
        hn[r] = 0.0;
        if (64 * r < H) {      // wave-uniform
          const double* wr = w_h + (row < H ? row : 0);
          double a4[4] = {0.0, 0.0, 0.0, 0.0};
          int q = 0;
          for (; q + 3 < H; q += 4) {
            a4[0] = fma(wr[(q + 0) * H], hs[q + 0], a4[0]);
            a4[1] = fma(wr[(q + 1) * H], hs[q + 1], a4[1]);
            a4[2] = fma(wr[(q + 2) * H], hs[q + 2], a4[2]);
            a4[3] = fma(wr[(q + 3) * H], hs[q + 3], a4[3]);
          }
          for (; q < H; ++q) a4[q & 3] = fma(wr[q * H], hs[q], a4[q & 3]);
          const double* we = wr + (size_t)H * H;
          for (q = 0; q < E - m3; ++q) a4[(H + q) & 3] = fma(we[q * H], er[q], a4[(H + q) & 3]);
          double a = (a4[0] + a4[2]) + (a4[1] + a4[3]);      // the order of the BLAS matvec behind the host's `@`
          if (m3) {                                           // and of its tail
            const double* wt = we + (E - m3) * H;
            const double* et = er + (E - m3);
            if (m3 == 1) {
              a = fma(wt[0], et[0], a);
            } else {
              double t = fma(wt[0], et[0], wt[H] * et[1]);
              if (m3 == 3) t = fma(wt[2 * H], et[2], t);
              a += t;
            }
          }
          a += bh[r];
          hn[r] = lm_tanh(a, lm_tt);
        }
      }
      lm_wave_sync();
#pragma unroll
      for (int r = 0; r < 2; ++r)
        if (lane + 64 * r < H) hs[lane + 64 * r] = hn[r];
      lm_wave_sync();
      // ---- logits of columns lane + 64 c ----
      double l[LM_NC];
#pragma unroll
      for (int c = 0; c < LM_NC; ++c) {
        l[c] = 0.0;
        if (c < NC) {          // wave-uniform
          const int v = lane + 64 * c;
          const double* wc = w_d + (col[c] ? v : 0);
          double a4[4] = {0.0, 0.0, 0.0, 0.0};
          int q = 0;
          for (; q + 3 < H; q += 4) {
            a4[0] = fma(wc[(q + 0) * V], hs[q + 0], a4[0]);
            a4[1] = fma(wc[(q + 1) * V], hs[q + 1], a4[1]);
            a4[2] = fma(wc[(q + 2) * V], hs[q + 2], a4[2]);
            a4[3] = fma(wc[(q + 3) * V], hs[q + 3], a4[3]);
          }
          for (; q < H; ++q) a4[q & 3] = fma(wc[q * V], hs[q], a4[q & 3]);
          double a = (a4[0] + a4[2]) + (a4[1] + a4[3]);
          a += bd[c];
          a += echo[c];
          if (v == P.stop) a += stop_bias;
          if (fun[c]) a = -1.0e+6;
          l[c] = a;
          if (v == tok_in) echo[c] -= 0.05;
        }
      }
      stop_bias = stop_bias < 0.0 ? 0.02 : stop_bias + 0.02;
      // ---- the decoder's weights e, their sum ----
      const double T = n_step == 0 ? temp0 : temp1;
      double e[LM_NC], part = 0.0;
      if (kind == LM_LOW || kind == LM_LABEL) {
#pragma unroll
        for (int c = 0; c < LM_NC; ++c) {
          double x = l[c];
          if (kind == LM_LOW && lane + 64 * c >= 1 && x < -1.0e+5) x = 0.0;
          e[c] = (c < NC && col[c]) ? exp(x) : 0.0;
          part += e[c];
        }
      } else {
        double m = -1.0e+300;
#pragma unroll
        for (int c = 0; c < LM_NC; ++c)
          if (c < NC && col[c]) m = fmax(m, l[c]);
        m = lm_wave_max(m);
#pragma unroll
        for (int c = 0; c < LM_NC; ++c) {
          e[c] = (c < NC && col[c]) ? exp((l[c] - m) / T) : 0.0;
          part += e[c];
        }
      }
      const double S = lm_lane(lm_wave_scan(part), 63);
      if (!(S > 0.0) || !(S <= 1.0e300)) err |= XV_DEVERR_NONFINITE;
      double p[LM_NC];
#pragma unroll
      for (int c = 0; c < LM_NC; ++c) p[c] = e[c] / S;
      // ---- the token ----
      int sym = 0;
      if (kind != LM_LABEL) {
        const double u = lm_lane(u_l, k);
        double s[LM_NC], run = 0.0;
#pragma unroll
        for (int c = 0; c < LM_NC; ++c) {
          s[c] = run;
          if (c < NC) {
            s[c] = lm_wave_scan(p[c]) + run;
            run = lm_lane(s[c], 63);
          }
        }
        sym = -1;
#pragma unroll
        for (int c = 0; c < LM_NC; ++c) {
          if (c < NC) {
            const unsigned long long hit = __ballot(col[c] && s[c] / run > u);
            if (sym < 0 && hit) sym = 64 * c + (__ffsll((long long)hit) - 1);
          }
        }
        if (sym < 0) sym = V - 1;      // searchsorted past the end: never with u < 1
      }
      if (kind == LM_LABEL || (kind == LM_GREEDY && sym != 0)) {
        double bv = -1.0;
        int bi = 0x7fffffff;
#pragma unroll
        for (int c = 0; c < LM_NC; ++c)
          if (c < NC && col[c] && p[c] > bv) { bv = p[c]; bi = lane + 64 * c; }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
          const double ov = __shfl_xor(bv, m, 64);
          const int oi = __shfl_xor(bi, m, 64);
          if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        sym = bi;
      }
      sym = __builtin_amdgcn_readfirstlane(sym);      // every lane holds the same value: say so
      // the token whose probability is reported: the given one (label) or the chosen one
      const int given = kind == LM_LABEL ? __builtin_amdgcn_readlane(a_l, k) : sym;
      double pg = p[0];
#pragma unroll
      for (int c = 1; c < LM_NC; ++c)
        if ((given >> 6) == c) pg = p[c];
      pg = lm_lane(pg, given & 63);
      ppl_sum += -log(fmax(pg, 1.0e-10));
      if (fuse) {
        // ---- the label pass's step over the same logits: the expressions of kind == LM_LABEL above ----
        double e2[LM_NC], part2 = 0.0;
#pragma unroll
        for (int c = 0; c < LM_NC; ++c) {
          e2[c] = (c < NC && col[c]) ? exp(l[c]) : 0.0;
          part2 += e2[c];
        }
        const double S2 = lm_lane(lm_wave_scan(part2), 63);
        if (!(S2 > 0.0) || !(S2 <= 1.0e300)) err |= XV_DEVERR_NONFINITE;
        double p2[LM_NC];
#pragma unroll
        for (int c = 0; c < LM_NC; ++c) p2[c] = e2[c] / S2;
        double bv = -1.0;
        int bi = 0x7fffffff;
#pragma unroll
        for (int c = 0; c < LM_NC; ++c)
          if (c < NC && col[c] && p2[c] > bv) { bv = p2[c]; bi = lane + 64 * c; }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
          const double ov = __shfl_xor(bv, m, 64);
          const int oi = __shfl_xor(bi, m, 64);
          if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == k) my_tok2 = __builtin_amdgcn_readfirstlane(bi);
        const int given2 = n_out >= max_len ? P.stop : sym;      // a cut pass's last step is labelled against the stop token
        double pg2 = p2[0];
#pragma unroll
        for (int c = 1; c < LM_NC; ++c)
          if ((given2 >> 6) == c) pg2 = p2[c];
        pg2 = lm_lane(pg2, given2 & 63);
        ppl_sum2 += -log(fmax(pg2, 1.0e-10));
      }
      ++n_step;
      if (kind == LM_LABEL) {
        if (lane == k) my_tok = sym;
        ++n_out;
        tok_in = given;
        done = n_step > n_ans;
      } else if (sym == P.stop) {
        done = true;
      } else if (n_out >= max_len) {
        err |= XV_DEVERR_LENGTH;      // the step after max_len tokens did not draw the stop token: the pass is cut
        done = true;
      } else {
        if (lane == k) my_tok = sym;
        ++n_out;
        tok_in = sym;
      }
    }
    if (STREAM) {
      if (A.dst && pos < n_out && A.at + pos < A.cap) A.dst[A.at + pos] = my_tok;
      if (A.dst2 && pos < (fuse ? n_step : n_out) && A.at2 + pos < A.cap) A.dst2[A.at2 + pos] = fuse ? my_tok2 : my_tok;
    } else if (A.dst && pos < n_out) {
      A.dst[pos] = my_tok;
    }
  }
  A.n_out = n_out;
  A.n_step = n_step;
  A.ppl_sum = ppl_sum;
  A.ppl_sum2 = ppl_sum2;
}
