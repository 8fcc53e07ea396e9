"""Golden fixtures of MetaLMV3: the REFERENCE's own env (xenoverse/metalang: TaskSamplerV3, MetaLMV3Env over RandomLM) on six
configurations.

Build-container tooling, like scripts/gen_golden_metalang.py: the reference is imported read-only through
oracle/_refimport.py; nothing under oracle/ is modified (the gymnasium stand-in there has no spaces.Sequence, which
MetaLMV3Env.__init__ asks for: the attribute is added to the imported module in this process only).

Per fixture: numpy.random.seed(call_seed), env.reset(), then STEPS times action = env.policy(T), env.step(action, cached)
with T cycling 1e-3, 0.1, 1, 10, 1e4 and every fourth step cached (the reference then returns the query of reset(), while
its language model keeps the state the last generated query left).  The file holds the weight arrays and sizes, both seeds,
and per step the query, action, temperature, label, greedy and low answers, the three ppl means and the reward as the
reference returned them (its RandomLM's methods are wrapped on the instance to record what they return).  The uniforms
every pass consumed are replayed from RandomState(call_seed), one per token, with the host restatement
(xenoverse_amd/metalang/lm_host.py) running alongside: it must give the reference's tokens and ppls bit for bit, or the
script stops.  Along that history it forms every draw's MARGIN (distance from u to the nearest CDF cut) and every argmax's
GAP (top-two probability difference).  A call seed that leaves a margin or gap below 1e-8 is passed over for the next one.

Only data is written: tests/golden/metalm_v3_<name>.npz.  Ragged rows are padded (tokens 0, uniforms 0.5, margins and
gaps inf) next to their lengths.

usage: python scripts/gen_golden_metalm.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import _refimport  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
MIN_MARGIN = 1e-8
TEMPS = (1e-3, 0.1, 1.0, 10.0, 1e4)
STEPS = 24


def _reference():
    _refimport.setup()
    import gymnasium
    if not hasattr(gymnasium.spaces, "Sequence"):
        class Sequence(gymnasium.spaces.Space):
            def __init__(self, space):
                self.feature_space = space
        gymnasium.spaces.Sequence = Sequence
    from xenoverse.metalang.metalangv3 import MetaLMV3Env
    from xenoverse.metalang.task_sampler import TaskSamplerV3
    return MetaLMV3Env, TaskSamplerV3


def _record(lm, log):
    """wrap the four answer passes of this RandomLM instance: log[name] gets every return value"""
    for name in ("label_answer", "generate_answer_greedy", "generate_answer_low", "generate_answer_softmax"):
        def wrapped(*a, _f=getattr(lm, name), _n=name, **k):
            out = _f(*a, **k)
            log.setdefault(_n, []).append(out)
            return out
        setattr(lm, name, wrapped)


def _pad(rows, fill, dtype, width):
    out = np.full((len(rows), width), fill, dtype)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def run(env, host, call_seed, log):
    """one recorded run -> dict of ragged lists; log: what _record's wrappers collect"""
    rs = np.random.RandomState(call_seed)
    np.random.seed(call_seed)
    rec = {k: [] for k in ("query", "u_query", "m_query", "action", "u_policy", "m_policy", "label", "g_label", "greedy",
                           "u_greedy", "m_greedy", "g_greedy", "low", "u_low", "m_low")}
    num = {k: [] for k in ("temperature", "cached", "ppl", "ppl_min", "ppl_max", "reward")}

    def query_pass(ref_query):
        q = host.generate_query(u=[rs.random_sample() for _ in range(len(ref_query) + 1)])
        assert list(q) == list(ref_query), "the host left the reference's query"
        rec["query"].append(q); rec["u_query"].append(host.last["u"]); rec["m_query"].append(host.last["margin"])

    query_pass(env.reset())
    for i in range(STEPS):
        T, cached = TEMPS[i % len(TEMPS)], i % 4 == 3
        action = env.policy(T)
        a, _ = host.generate_answer_softmax(T=T, u=[rs.random_sample() for _ in range(len(action) + 1)])
        assert a == list(action), "the host left the reference's policy answer"
        rec["action"].append(a); rec["u_policy"].append(host.last["u"]); rec["m_policy"].append(host.last["margin"])
        obs, r, term, trunc, info = env.step(action, cached=cached)
        ref_label, ref_ppl = log["label_answer"][-1]
        ref_greedy, ref_min = log["generate_answer_greedy"][-1]
        ref_low, ref_max = log["generate_answer_low"][-1]
        label, ppl = host.label_answer(a)
        rec["label"].append(label); rec["g_label"].append(host.last["gap"])
        g, ppl_min = host.generate_answer_greedy(u=[rs.random_sample() for _ in range(len(ref_greedy) + 1)])
        rec["greedy"].append(g); rec["u_greedy"].append(host.last["u"]); rec["m_greedy"].append(host.last["margin"])
        rec["g_greedy"].append(host.last["gap"])
        lo, ppl_max = host.generate_answer_low(u=[rs.random_sample() for _ in range(len(ref_low) + 1)])
        rec["low"].append(lo); rec["u_low"].append(host.last["u"]); rec["m_low"].append(host.last["margin"])
        assert (label, g, lo) == (list(ref_label), list(ref_greedy), list(ref_low)) and list(info["label"]) == label
        assert (ppl, ppl_min, ppl_max) == (ref_ppl, ref_min, ref_max), "the host's ppl is not the reference's"
        assert term is False and trunc is (i + 1 < STEPS)
        if cached:
            assert list(obs) == list(rec["query"][0])      # the reference hands back the query of reset() (metalangv3.py:24,36)
            rec["query"].append(list(obs)); rec["u_query"].append([]); rec["m_query"].append([])
        else:
            query_pass(list(obs))
        for k, v in (("temperature", T), ("cached", cached), ("ppl", ref_ppl), ("ppl_min", ref_min), ("ppl_max", ref_max),
                     ("reward", r)):
            num[k].append(v)
    assert np.random.random_sample() == rs.random_sample(), "the replayed stream is not where the reference's is"
    rec.update(num)
    return rec


def gen(name, sampler_seed, V, E, H):
    MetaLMV3Env, TaskSamplerV3 = _reference()
    from xenoverse_amd.metalang.lm_host import RandomLMHost
    task = TaskSamplerV3(vocab_size=V, embedding_size=E, hidden_size=H, seed=sampler_seed)
    lm = task["lm"]
    host = RandomLMHost.from_reference(lm)
    log = {}
    _record(lm, log)
    env = MetaLMV3Env(max_steps=STEPS)      # the last step's fourth return value is then False in the reference
    env.set_task(task)
    call_seed = sampler_seed + 1000
    while True:
        log.clear()
        rec = run(env, host, call_seed, log)
        worst = min(min(np.min(r) if len(r) else np.inf for r in rec[k])
                    for k in ("m_query", "m_policy", "m_greedy", "m_low", "g_label", "g_greedy"))
        if worst >= MIN_MARGIN:
            break
        print("%s: call seed %d leaves a margin or gap of %.1e, trying the next" % (name, call_seed, worst))
        call_seed += 1
    width = max(max(len(r) for r in rec[k]) for k in rec if k[:2] in ("u_", "m_", "g_") or k in (
        "query", "action", "label", "greedy", "low"))
    out = dict(enc_w=host.enc_w, rnn_w=host.rnn_w, rnn_b=host.rnn_b, dec_w=host.dec_w, dec_b=host.dec_b,
               n_vocab=np.int64(V), n_emb=np.int64(E), n_hidden=np.int64(H), sampler_seed=np.int64(sampler_seed),
               call_seed=np.int64(call_seed), stop_token=np.int64(lm.stop_token),
               function_tokens=np.array(lm.function_token_list, np.int64), width=np.int64(width))
    for k in ("query", "action", "label", "greedy", "low"):
        out[k] = _pad(rec[k], 0, np.int32, width)
        out[k + "_len"] = np.array([len(r) for r in rec[k]], np.int32)
    for k in ("u_query", "u_policy", "u_greedy", "u_low"):
        out[k] = _pad(rec[k], 0.5, np.float64, width)
        out[k + "_n"] = np.array([len(r) for r in rec[k]], np.int32)
    for k in ("m_query", "m_policy", "m_greedy", "m_low", "g_label", "g_greedy"):
        out[k] = _pad(rec[k], np.inf, np.float64, width)
    for k in ("temperature", "ppl", "ppl_min", "ppl_max", "reward"):
        out[k] = np.array(rec[k], np.float64)
    out["cached"] = np.array(rec["cached"], np.bool_)
    path = os.path.join(GOLD, "metalm_v3_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("%s: call seed %d, width %d, smallest margin or gap %.2e, %d bytes" % (name, call_seed, width, worst,
                                                                                 os.path.getsize(path)))


CONFIGS = [  # name, sampler seed, V, E, H
    ("v32_e16_h32_a", 301, 32, 16, 32),
    ("v32_e16_h32_b", 302, 32, 16, 32),
    ("v64_e16_h64", 303, 64, 16, 64),
    ("v128_e32_h64", 304, 128, 32, 64),
    ("v100_e12_h24", 305, 100, 12, 24),
    ("v256_e16_h64", 306, 256, 16, 64),
]


def main():
    for cfg in CONFIGS:
        gen(*cfg)


if __name__ == "__main__":
    main()
