"""MetaLangV2Host: the numpy restatement of the reference's RandomNGram.forward (xenoverse/metalang/metalangv2.py:31-77), in
fp64 and in the reference's order of operations, with the uniforms handed in instead of drawn from numpy's global stream.
It is the CPU-side check of csrc/metalang.hip (tests/test_host_metalang.py pins it to the reference's recorded runs) and the
CPU line of scripts/bench_metalang.py; the product never generates on the CPU.

One step, for the B sequences of a call (a *group*: they share the statistics of line 3):
  1. the window of the last n tokens (n copies of token 0 at the start): a[g] = emb[window[g]] @ W_in[g] + b_in[g]
  2. h = mean_g(g * tanh(a[g]))                  (:62-63; the oldest slot has weight 0)
  3. o = h @ W_out + b_out;  o = lambda * ((1 / std) * (o - mean)), mean and std = sqrt(mean(o^2) - mean(o)^2) over ALL
     B * V logits                                 (:37-41, :64-66)
  4. p = exp(o) / sum(exp(o));  token = first index with cumsum(p) > u, token 0 if there is none   (:67-69)
"""
import numpy as np

from .task_sampler import check_task


class MetaLangV2Host(object):
    def __init__(self, task):
        self.V, self.E, self.H, self.n = check_task(task)
        self.emb = np.asarray(task["word_emb"], np.float64)
        self.w_in = np.asarray(task["weights_inputlayer"], np.float64)
        self.b_in = np.asarray(task["bias_inputlayer"], np.float64)
        self.w_out = np.asarray(task["weights_outputlayer"], np.float64)
        self.b_out = np.asarray(task["bias_outputlayer"], np.float64)
        self.lam = task["_lambda"]
        self.slot_weight = np.arange(self.n).reshape(1, self.n, 1, 1)

    def probabilities(self, window):
        """window int[B, n] (oldest first) -> p float64[B, V] of the next token"""
        x = self.emb[window][:, :, None, :]                                   # [B, n, 1, E]
        act = np.tanh(np.matmul(x, self.w_in) + self.b_in)                    # [B, n, 1, H]
        h = np.mean(self.slot_weight * act, axis=1)                           # [B, 1, H]
        o = np.squeeze(np.matmul(h, self.w_out) + self.b_out, axis=1)         # [B, V]
        m = np.mean(o)
        std = np.sqrt(np.mean(o * o) - m * m)
        e = np.exp(self.lam * ((1.0 / std) * (o - m)))
        return e / np.sum(e, axis=-1, keepdims=True)

    def run(self, u=None, tokens=None):
        """u float64[B, L]: generate (the draws of sequence b in order).  tokens int[B, L + 1]: teacher forcing along that
        history.  -> dict(tokens int32[B, L + 1], prob float64[B, L] of each token given its predecessors, margin
        float64[B, L]: the distance from u to the nearest cut of the CDF it was compared with (generate only))"""
        if (u is None) == (tokens is None):
            raise ValueError("give either the uniforms or the tokens")
        if u is not None:
            u = np.asarray(u, np.float64)
            B, L = u.shape
        else:
            tokens = np.asarray(tokens)
            B, L = tokens.shape[0], tokens.shape[1] - 1
            if tokens.min() < 0 or tokens.max() >= self.V:
                raise ValueError("tokens must lie in [0, %d)" % self.V)
        rows = np.arange(B)
        out = np.zeros((B, L + 1), np.int32)
        prob = np.zeros((B, L))
        margin = np.full((B, L), np.inf)
        window = np.zeros((B, self.n), np.int64)
        for t in range(L):
            window[:, :-1] = window[:, 1:]
            window[:, -1] = out[:, t]
            p = self.probabilities(window)
            if u is not None:
                cdf = p.cumsum(1)
                nxt = (cdf > u[:, t, None]).argmax(1)
                margin[:, t] = np.abs(cdf - u[:, t, None]).min(1)
            else:
                nxt = tokens[:, t + 1]
            out[:, t + 1] = nxt
            prob[:, t] = p[rows, nxt]
        return dict(tokens=out, prob=prob, margin=margin)

    def forward(self, u):
        """u float64[B, L] -> tokens int32[B, L + 1]"""
        return self.run(u=u)["tokens"]

    def log_prob(self, tokens):
        """tokens int[B, L + 1] -> float64[B, L]"""
        return np.log(self.run(tokens=tokens)["prob"])

    @staticmethod
    def perplexity(prob):
        """the reference's "Ground Truth Sequence Perplexity" (:71-75): the mean of -log p over all B * L draws"""
        return float(-np.sum(np.log(prob)) / prob.size)
