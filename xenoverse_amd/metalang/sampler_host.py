"""Host restatement (numpy, fp64) of the device MetaLMV3 task sampler (csrc/metalm_sampler.hip: xv_metalm_sample_tasks): the
same Philox counters, the same constructions in the same order.  It is what the device is compared with
(tests/test_gpu_metalm_sampler.py), as linds/sampler_host.py is for its family.

The model.  The reference's RandomLM seeds its three networks with ONE seed, so their weights are one
stream of standard normals z under three scales: `arrays_from_normals`.  Fed numpy's own stream
(RandomState(seed).normal(size=...)) it gives RandomLMHost.from_seed(seed) bit for bit; the device feeds it the Philox
normals of (seed, candidate): `task_normals`.  `layer_norm_rows` states the order in which numpy forms the embedding table,
which the device follows to the bit.  `metalm_uniforms` are the free-running draws of the MetaLMV3 kernels (csrc/metalm.hip)
and `candidate_host` runs the acceptance protocol with them over RandomLMHost.
"""
import numpy as np

from ..host_draws import box_muller, env_draw_sub_words, interleave, np_sum, pair
from .lm_host import RandomLMHost
from .stream_host import CHECK_T_HIGH, CHECK_T_LOW, _sub_step

XV_DRAW_METALM, XV_DRAW_METALM_TASK = 9, 14                # csrc/metalm.hip, csrc/metalm_sampler.hip
LM_QUERY, LM_POLICY, LM_LABEL, LM_GREEDY, LM_LOW = 0, 1, 2, 3, 4      # the pass kinds of csrc/metalm.hip

STATUS = ("accepted", "nonfinite", "reward_low", "reward_high")


def _pairs(seed, gid, tick, purpose, sub):
    return pair(env_draw_sub_words(seed, gid, tick, purpose, sub))


def n_normals(V, E, H):
    """the length of the stream a task needs: the longest of the three networks' draws"""
    return max(V * E, V * H, H * (H + E) + H)


def task_normals(seed, cand, n):
    """z[0 .. n) of candidate `cand`: z[i] is member i & 1 (cos, sin) of the fp64 Box-Muller pair of the call with
    sub = i >> 1"""
    i = np.arange(n)
    return interleave(i, *box_muller(*_pairs(seed, cand, 0, XV_DRAW_METALM_TASK, i >> 1)))


def arrays_from_normals(z, V, E, H):
    """the arrays of RandomLM(V, ., E, H, seed) from the seed's standard normals z (at least n_normals(V, E, H) of them):
    every network restarts the stream, so the three weight matrices share its head -> RandomLMHost.arrays()'s dict"""
    z = np.asarray(z, np.float64).reshape(-1)
    if len(z) < n_normals(V, E, H):
        raise ValueError("(%d, %d, %d) needs %d normals, got %d" % (V, E, H, n_normals(V, E, H), len(z)))

    def weights(n_in, n_out):
        return (np.sqrt(2.0 / (n_in + n_out)) * z[:n_in * n_out]).reshape(n_out, n_in) * 3
    n_rnn = H * (H + E)
    return dict(enc_w=weights(V, E), rnn_w=weights(E + H, H), rnn_b=0.1 * z[n_rnn:n_rnn + H], dec_w=weights(H, V),
                dec_b=np.zeros(V))


def layer_norm_rows(x, eps=1e-8):
    """lm_host.layer_norm of a [rows, E] array with its sums in the stated order: mean = sum(x) / E, d = x - mean,
    var = sum(d d) / E, d / (sqrt(var) + eps).  Rows of more than 128 elements are summed recursively, where the device's
    lm_np_sum does not follow: they raise."""
    x = np.ascontiguousarray(x, np.float64)
    if x.shape[1] > 128:
        raise ValueError("rows of more than 128 elements are summed recursively: not restated on the device")
    out = np.empty_like(x)
    E = x.shape[1]
    for k, row in enumerate(x):
        mean = np_sum(row) / E
        d = row - mean
        var = np_sum(d * d) / E
        out[k] = d / (np.sqrt(var) + eps)
    return out


def metalm_uniforms(seed, gid, tick, kind, n):
    """the free-running uniforms of positions 0 .. n - 1 of one pass (csrc/metalm_pass.h): position p is words 0,1 (p even)
    or 2,3 (p odd) of the call (seed, gid, tick, XV_DRAW_METALM, sub = kind << 16 | p >> 1)"""
    p = np.arange(n)
    return interleave(p, *_pairs(seed, gid, tick, XV_DRAW_METALM, (int(kind) << 16) | (p >> 1)))


def status_of(reward_low, reward_high, nonfinite=False):
    """the device's status: the tests in its order"""
    if nonfinite or not (np.isfinite(reward_low) and np.isfinite(reward_high)):
        return 1
    if reward_low > 0.0:
        return 2
    if reward_high < 2.0:
        return 3
    return 0


def arrays_of_tables(tables, i):
    """candidate / task i of a device tables dict (device_sampler.sample_candidates or sample_tasks_device) -> the arrays
    RandomLMHost takes"""
    def host(k):
        t = tables[k][i]
        return np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, np.float64)
    return dict(enc_w=host("enc_w"), rnn_w=np.ascontiguousarray(host("w_h_t").T), rnn_b=host("b_h"),
                dec_w=np.ascontiguousarray(host("w_d_t").T), dec_b=host("b_d"))


class _CutLM(RandomLMHost):
    """RandomLMHost that remembers whether any of its passes was cut at max_len (`overflow` is the last pass's)"""
    cut = False

    def generate_sequence(self, *args, **kw):
        out = RandomLMHost.generate_sequence(self, *args, **kw)
        self.cut = self.cut or self.overflow
        return out


def candidate_host(seed, c, V, E, H, max_len=1024, arrays=None, stop_token=0, function_tokens=None):
    """candidate c of `seed` on the host: its networks (or the given `arrays`, e.g. the device's own: arrays_of_tables) and
    the acceptance protocol reset(), policy(1e4), step(cached), policy(1e-6), step(cached) with the uniforms an engine
    with this seed, env_id_base = c and tick 0 draws (ticks 0 .. 4).  -> dict: arrays, reward [2] (low, high), ppl [2][3]
    (ppl, ppl_min, ppl_max), status, query, answer and label (a list per sub-step), margin and gap: the smallest margin of
    a draw and the smallest gap of an argmax over all passes (lm_host.py), cut: a pass emitted max_len tokens and then did
    not draw the stop token (the device's XV_DEVERR_LENGTH)."""
    if arrays is None:
        arrays = arrays_from_normals(task_normals(seed, c, n_normals(V, E, H)), V, E, H)
    lm = _CutLM(arrays["enc_w"], arrays["rnn_w"], arrays["rnn_b"], arrays["dec_w"], arrays["dec_b"],
                      stop_token=stop_token, function_tokens=function_tokens, max_len=max_len)
    n = int(max_len) + 1

    def u(tick, kind):
        return metalm_uniforms(seed, c, tick, kind, n)
    query = lm.generate_query(u=u(0, LM_QUERY))
    margin = float(lm.last["margin"].min())
    draws = dict(u_policy=[u(1, LM_POLICY), u(3, LM_POLICY)], u_greedy=[u(2, LM_GREEDY), u(4, LM_GREEDY)],
                 u_low=[u(2, LM_LOW), u(4, LM_LOW)])
    subs = []
    gap = np.inf
    for k, T in enumerate((CHECK_T_LOW, CHECK_T_HIGH)):
        _sub_step(lm, T, True, draws, k, subs)
        rec = subs[-1]
        margin = min([margin] + [float(rec[m].min()) for m in ("m_policy", "m_greedy", "m_low")])
        gap = min(gap, float(rec["g_label"].min()), float(rec["g_greedy"].min()))
    rewards = np.array([s["reward"] for s in subs])
    return dict(arrays=arrays, reward=rewards, ppl=np.array([s["ppl"] for s in subs]),
                status=status_of(rewards[0], rewards[1]), query=list(query), answer=[s["action"] for s in subs],
                label=[s["label"] for s in subs], margin=margin, gap=gap, cut=bool(lm.cut))
