"""MetaLMV3 on the host: the reference's RandomLM (xenoverse/utils/random_nn.py:218-344), its three decoders (:193-216) and
TaskSamplerV3 (xenoverse/metalang/task_sampler.py:86-98), restated in plain numpy in the reference's order of operations.

A task is three random networks drawn from ONE seed (each constructor re-seeds with it): enc V -> E (no bias), dec H -> V
(no bias) and a tanh RNN over concat(h, enc_out) with bias 0.1 normal; every weight is normal(0, sqrt(2 / (n_in + n_out))) * 3.
forward(tok), per token:
    enc_out = layer_norm(W_enc[:, tok])                  (x - mean) / (std + 1e-8): the table `emb`, formed once
    h       = tanh(W_h @ concat(h, enc_out) + b_h)
    logits  = W_d @ h + b_d + echo_bias;  logits[stop] += stop_bias;  logits[function tokens] = -1e6
    stop_bias: -1e6 at the first token, then 0.02, 0.04, ...;  echo_bias[tok] -= 0.05
Every decoder draws once per token through numpy.random.choice(p=...): cdf = p.cumsum(); cdf /= cdf[-1];
searchsorted(u, 'right').  Here every drawing method takes `u=`, the uniforms it is to consume (one per token); without it
they come from a private RandomState, so numpy's global generator is never touched.  One RandomState.random_sample() per
choice call replays the reference's stream.

The host also records what the device comparison needs: per draw the MARGIN, the distance from u to the
nearest cut of the CDF, and per argmax the GAP between the two largest probabilities — `last` after every pass."""
import os

import numpy as np

from .._lib import XenoError

# what csrc/metalm.hip supports (xv_metalm_create refuses anything outside as well)
LM_LIMITS = dict(n_vocab=(12, 256), n_hidden=(1, 128), n_emb=(1, 64), max_len=(1, 1024))
FUNCTION_VOCABULARY = {"s": 0, "q": 1, "a": 2, "r1": 3, "r2": 4, "r3": 5, "r4": 6, "r5": 7, "r>": 8, "r=": 9, "r<": 10}


def check_lm_limit(name, value):
    """XenoError unless LM_LIMITS[name] holds value"""
    lo, hi = LM_LIMITS[name]
    if not lo <= int(value) <= hi:
        raise XenoError("MetaLMV3: %s = %d is outside the supported range %d .. %d" % (name, int(value), lo, hi))


def layer_norm(x, eps=1e-8):
    mean = x.mean(axis=-1, keepdims=True)
    std = x.std(axis=-1, keepdims=True)
    return (x - mean) / (std + eps)


def _choice(p, u):
    """numpy.random.choice(arange(len(p)), p=p) with its uniform handed in -> (index, margin)"""
    cdf = p.cumsum()
    cdf /= cdf[-1]
    idx = int(cdf.searchsorted(u, side="right"))
    return min(idx, len(p) - 1), float(np.abs(cdf - u).min())


def _gap(p):
    """the two largest entries' difference: how far argmax(p) is from a tie"""
    top = np.partition(p, len(p) - 2)[-2:]
    return float(top[1] - top[0])


class _Uniforms(object):
    """the uniforms of one pass: injected (consumed in order) or drawn from the LM's private generator"""

    def __init__(self, u, rs):
        self.u = None if u is None else np.asarray(u, np.float64).reshape(-1)
        self.rs, self.n, self.used = rs, 0, []

    def next(self):
        if self.u is None:
            v = float(self.rs.random_sample())
        else:
            if self.n >= len(self.u):
                raise ValueError("the pass needs more than the %d uniforms it was given" % len(self.u))
            v = float(self.u[self.n])
        self.n += 1
        self.used.append(v)
        return v


class RandomLMHost(object):
    """RandomLMHost(enc_w [E,V], rnn_w [H,H+E], rnn_b [H], dec_w [V,H], dec_b [V], stop_token=0, function_tokens=1..10),
    RandomLMHost.from_seed(V, E, H, seed) or RandomLMHost.from_reference(lm) with any object that has the reference's
    attributes (.enc.weights[0], .dec.weights[0], .dec.biases[0], .rnn.wh, .rnn.bh, .stop_token, .function_token_list).

    max_len: None is the reference (a pass runs until the stop token); a number is the device's rule: a pass emits at most
    max_len tokens, the step after them is the last, and `overflow` is set when that step does not draw the stop token."""

    stop_inc = 0.02
    echo_punish = 0.05

    def __init__(self, enc_w, rnn_w, rnn_b, dec_w, dec_b=None, stop_token=0, function_tokens=None, seed=None, max_len=None):
        self.enc_w = np.ascontiguousarray(enc_w, np.float64)
        self.rnn_w = np.ascontiguousarray(rnn_w, np.float64)
        self.rnn_b = np.ascontiguousarray(rnn_b, np.float64)
        self.dec_w = np.ascontiguousarray(dec_w, np.float64)
        self.n_emb, self.n_vocab = self.enc_w.shape
        self.n_hidden = self.rnn_w.shape[0]
        self.dec_b = np.zeros(self.n_vocab) if dec_b is None else np.ascontiguousarray(dec_b, np.float64)
        for k, v in (("n_vocab", self.n_vocab), ("n_hidden", self.n_hidden), ("n_emb", self.n_emb)):
            check_lm_limit(k, v)
        if max_len is not None:
            check_lm_limit("max_len", max_len)
        shapes = dict(rnn_w=(self.n_hidden, self.n_hidden + self.n_emb), rnn_b=(self.n_hidden,),
                      dec_w=(self.n_vocab, self.n_hidden), dec_b=(self.n_vocab,))
        for k, s in shapes.items():
            if getattr(self, k).shape != s:
                raise ValueError("%s has shape %s, the sizes say %s" % (k, getattr(self, k).shape, s))
        self.stop_token = int(stop_token)
        if function_tokens is None:
            function_tokens = [v for k, v in FUNCTION_VOCABULARY.items() if k != "s"]
        self.function_token_list = [int(t) for t in function_tokens]
        for t in [self.stop_token] + self.function_token_list:
            if not 0 <= t < self.n_vocab:
                raise ValueError("token %d is outside the vocabulary of %d" % (t, self.n_vocab))
        self.max_len = max_len
        # the reference's forward() goes one_hot -> enc -> layer_norm per token: enc_w @ one_hot is the token's column,
        # exactly (products with 0 and 1, sums with 0), so the table is the layer_norm of every column, row by row
        self.emb = layer_norm(np.ascontiguousarray(self.enc_w.T))
        self._rs = np.random.RandomState(seed)
        self.hidden_states = np.zeros(self.n_hidden)
        self.cache_states = np.zeros(self.n_hidden)
        self.overflow = False
        self.last = None
        self.reset()

    # ---- construction ---------------------------------------------------------------------------------------------
    @classmethod
    def from_seed(cls, n_vocab, n_emb, n_hidden, seed, **kw):
        """the reference's RandomLM(n_vocab, function_vocab, n_emb, n_hidden, seed): three constructors, each re-seeded"""
        def weights(n_in, n_out, bias):
            rs = np.random.RandomState(seed)
            w = rs.normal(0, np.sqrt(2.0 / (n_in + n_out)), size=(n_out, n_in)) * 3
            return w, (0.1 * rs.normal(size=[n_out]) if bias else np.zeros(shape=[n_out]))
        enc_w, _ = weights(n_vocab, n_emb, False)
        dec_w, dec_b = weights(n_hidden, n_vocab, False)
        rnn_w, rnn_b = weights(n_emb + n_hidden, n_hidden, True)
        return cls(enc_w, rnn_w, rnn_b, dec_w, dec_b, **kw)

    @classmethod
    def from_reference(cls, lm, **kw):
        return cls(lm.enc.weights[0], lm.rnn.wh, lm.rnn.bh, lm.dec.weights[0], lm.dec.biases[0], stop_token=lm.stop_token,
                   function_tokens=lm.function_token_list, **kw)

    def arrays(self):
        return dict(enc_w=self.enc_w, rnn_w=self.rnn_w, rnn_b=self.rnn_b, dec_w=self.dec_w, dec_b=self.dec_b)

    # ---- state (random_nn.py:238-251) ---------------------------------------------------------------------------
    def reset(self):
        self.hidden_states = np.zeros(self.n_hidden)
        self.stop_bias = -1.0e+6
        self.echo_bias = np.zeros((self.n_vocab,))

    def cache(self):
        self.cache_states = self.hidden_states.copy()
        self.stop_bias = -1.0e+6
        self.echo_bias.fill(0.0)

    def restore(self):
        self.hidden_states = self.cache_states.copy()
        self.stop_bias = -1.0e+6
        self.echo_bias.fill(0.0)

    # ---- one token (:253-283) --------------------------------------------------------------------------------------
    def forward(self, inputs):
        encodings = self.emb[inputs]
        n_hidden = np.concatenate([self.hidden_states, encodings], axis=0)
        self.hidden_states = np.tanh(self.rnn_w @ n_hidden + self.rnn_b)
        decodings = self.dec_w @ self.hidden_states.copy() + self.dec_b
        logits = decodings + self.echo_bias
        logits[self.stop_token] += self.stop_bias
        logits[self.function_token_list] = -1.0e+6
        if self.stop_bias < 0:
            self.stop_bias = self.stop_inc
        else:
            self.stop_bias += self.stop_inc
        self.echo_bias[inputs] -= self.echo_punish
        return logits

    __call__ = forward

    @staticmethod
    def _decode(logits, temperature, decode_type, u):
        """-> (token, ppl, margin of the draw, gap of the argmax or inf)"""
        gap = np.inf
        if decode_type == "rnd":
            logits[1:] -= logits[1:] * (logits[1:] < -1.0e+5).astype(np.float32)
            probs = np.exp(logits)
        elif decode_type in ("softmax", "greedy"):
            logits -= np.max(logits)
            probs = np.exp(logits / temperature)
        else:
            raise NotImplementedError("Unknown sampling method: %s" % decode_type)
        probs /= np.sum(probs, axis=-1, keepdims=True)
        symbol, margin = _choice(probs, u)
        if decode_type == "greedy" and symbol != 0:
            symbol = int(np.argmax(probs))
            gap = _gap(probs)
        return int(symbol), -np.log(max(probs[symbol], 1.0e-10)), margin, gap

    def generate_one_step(self, inputs, temperature=1, decode_type="softmax", u=None):
        if u is None:
            u = float(self._rs.random_sample())
        return self._decode(self.forward(inputs), temperature, decode_type, u)[:2]

    def generate_sequence(self, inputs, T_s=1.0, T_c=1.0, decode_type="softmax", u=None):
        draws = _Uniforms(u, self._rs)
        output, ppls, margins, gaps = [], [], [], []
        done = False
        T = T_s
        self.overflow = False
        while not done:
            tok, ppl, margin, gap = self._decode(self.forward(inputs), T, decode_type, draws.next())
            ppls.append(ppl)
            margins.append(margin)
            gaps.append(gap)
            if tok == self.stop_token:
                done = True
            elif self.max_len is not None and len(output) >= self.max_len:
                self.overflow = done = True
            else:
                output.append(tok)
                inputs = tok
            T = T_c
        self.last = dict(u=np.array(draws.used), margin=np.array(margins), gap=np.array(gaps), ppls=np.array(ppls))
        return output, ppls

    # ---- the reference's passes (:306-344) -------------------------------------------------------------------------
    def generate_query(self, u=None):
        self.reset()
        query, _ = self.generate_sequence(0, decode_type="softmax", T_s=10.0, T_c=1.0, u=u)
        return query

    def _answer(self, decode_type, T, u):
        self.cache()
        ans, ppls = self.generate_sequence(0, decode_type=decode_type, T_s=T, T_c=T, u=u)
        self.restore()
        return ans, np.mean(ppls)

    def generate_answer_greedy(self, u=None):
        return self._answer("greedy", 1.0, u)

    def generate_answer_softmax(self, T=1.0, u=None):
        return self._answer("softmax", T, u)

    def generate_answer_low(self, u=None):
        return self._answer("rnd", 1.0, u)

    def label_answer(self, ans):
        self.cache()
        ppls, label_toks, gaps = [], [], []
        prev_token = 0
        for tok in list(ans) + [self.stop_token]:
            logits = self.forward(prev_token)
            probs = np.exp(logits)
            probs /= np.sum(probs)
            label_toks.append(int(np.argmax(probs)))
            gaps.append(_gap(probs))
            ppls.append(-np.log(max(1.0e-10, probs[tok])))
            prev_token = tok
        self.restore()
        self.last = dict(gap=np.array(gaps), ppls=np.array(ppls))
        return label_toks, np.mean(ppls)


def TaskSamplerV3(vocab_size=32, embedding_size=16, hidden_size=32, seed=None):
    """the reference's task dict; "lm" is a RandomLMHost whose arrays equal the reference's RandomLM bit for bit"""
    if seed is None:
        seed = int.from_bytes(os.urandom(4), "little")
    return {"vocabulary": vocab_size,
            "embedding": embedding_size,
            "hidden": hidden_size,
            "function_vocabulary": dict(FUNCTION_VOCABULARY),
            "lm": RandomLMHost.from_seed(vocab_size, embedding_size, hidden_size, seed,
                                         stop_token=FUNCTION_VOCABULARY["s"])}


def reward(ppl, ppl_min, ppl_max):
    """metalangv3.py:32"""
    return (ppl_max - ppl_min) / max(ppl - ppl_min + 0.1, 1.0e-3) - 2.0
