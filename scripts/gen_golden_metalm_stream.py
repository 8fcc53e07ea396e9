"""Golden fixtures of the MetaLMV3 training streams: the REFERENCE's own generate_data_v3_single_task_qar / _qa / _qara
(xenoverse/metalang/generator_v3.py:48-173) on five configurations.

Build-container tooling, like scripts/gen_golden_metalm.py: the reference is imported read-only through
oracle/_refimport.py and nothing under oracle/ is modified (the gymnasium stand-in's missing spaces.Sequence is added to
the imported module in this process only).

Per fixture: numpy.random.seed(call_seed), then the reference's generator with T_choices = None and the fixture's L.  The
host restatement (xenoverse_amd/metalang/stream_host.py) runs the same stream with its language model's private generator
set to RandomState(call_seed): one random_sample() per token, and rs.choice(T_choices) in lock step with the reference's
numpy.random.choice(T_choices).  It must give the reference's data and label exactly and leave the generator where the
reference's is, or the script stops.  L is chosen from the host's own round lengths: the end of the sixth round plus half
of the seventh, so that the stream spans six full rounds and ends inside one.

A call seed that leaves a draw's margin or an argmax's gap below 1e-8, or a reward within 1e-6 of a threshold of its
token, is passed over for the next one.

Only data is written: tests/golden/metalmstream_<name>.npz with the weights, datatype, L, data and label as the reference
returned them, and per sub-step the temperature index, the consumed uniforms of every pass, the margins and gaps, the
reward and its distance to the nearest threshold.  Ragged rows are padded (uniforms 0.5, margins and gaps inf) next to
their lengths.

usage: python scripts/gen_golden_metalm_stream.py
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
MIN_R_DIST = 1e-6
FULL_ROUNDS = 6
MAX_BYTES = 811543


def _reference():
    _refimport.setup()
    import gymnasium
    if not hasattr(gymnasium.spaces, "Sequence"):
        class Sequence(gymnasium.spaces.Space):
            def __init__(self, space):
                self.feature_space = space
        gymnasium.spaces.Sequence = Sequence
    from xenoverse.metalang import generator_v3
    from xenoverse.metalang.task_sampler import TaskSamplerV3
    return generator_v3, TaskSamplerV3


def _pad(rows, fill, dtype, width):
    out = np.full((len(rows), width), fill, dtype)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def _host(ref_lm, datatype, L, call_seed):
    from xenoverse_amd.metalang.lm_host import RandomLMHost
    from xenoverse_amd.metalang.stream_host import default_T_choices, stream_lm
    host = RandomLMHost.from_reference(ref_lm, seed=call_seed)
    choices = default_T_choices()
    return host, stream_lm(host, datatype, L, lambda k: host._rs.choice(len(choices)), choices)


def gen(name, datatype, sampler_seed, V, E, H):
    generator_v3, TaskSamplerV3 = _reference()
    ref = {"QAR": generator_v3.generate_data_v3_single_task_qar, "QA": generator_v3.generate_data_v3_single_task_qa,
           "QARA": generator_v3.generate_data_v3_single_task_qara}[datatype]
    task = TaskSamplerV3(vocab_size=V, embedding_size=E, hidden_size=H, seed=sampler_seed)
    call_seed = sampler_seed + 2000
    while True:
        # the stream's prefix does not depend on L: the host's round lengths at a generous L give the fixture's
        L = 64
        ends = []
        while len(ends) <= FULL_ROUNDS:
            L *= 2
            _, (_, _, probe) = _host(task["lm"], datatype, L, call_seed)
            ends = [e[0] for e in probe["round_end"]]
        L = ends[FULL_ROUNDS - 1] + max(1, (ends[FULL_ROUNDS] - ends[FULL_ROUNDS - 1]) // 2)
        np.random.seed(call_seed)
        ref_data, ref_label = ref(task, L=L)
        host, (data, label, info) = _host(task["lm"], datatype, L, call_seed)
        if not (np.array_equal(data, ref_data) and np.array_equal(label, ref_label)):
            raise SystemExit("%s: the host restatement left the reference's stream (call seed %d)" % (name, call_seed))
        if np.random.random_sample() != host._rs.random_sample():
            raise SystemExit("%s: the replayed generator is not where the reference's is" % name)
        subs = info["subs"]
        worst = min([float(np.min(info["reset_margin"]))] + [float(np.min(s[k])) for s in subs for k in (
            "m_policy", "m_greedy", "m_low", "m_query", "g_label", "g_greedy") if len(s[k])])
        r_dist = float(info["r_dist"].min())
        if worst >= MIN_MARGIN and r_dist >= MIN_R_DIST:
            break
        print("%s: call seed %d leaves a margin or gap of %.1e and a reward %.1e from a threshold, trying the next" % (
            name, call_seed, worst, r_dist))
        call_seed += 1
    assert info["rounds"] == FULL_ROUNDS + 1 and ends[FULL_ROUNDS - 1] < L < info["round_end"][-1][0]
    lm = host
    width = max([len(info["reset_u"])] + [len(s[k]) for s in subs for k in ("u_policy", "u_greedy", "u_low", "u_query",
                                                                            "g_label")])
    out = dict(enc_w=lm.enc_w, rnn_w=lm.rnn_w, rnn_b=lm.rnn_b, dec_w=lm.dec_w, dec_b=lm.dec_b, n_vocab=np.int64(V),
               n_emb=np.int64(E), n_hidden=np.int64(H), sampler_seed=np.int64(sampler_seed), call_seed=np.int64(call_seed),
               stop_token=np.int64(lm.stop_token), function_tokens=np.array(lm.function_token_list, np.int64),
               width=np.int64(width), datatype=np.array(datatype), L=np.int64(L), data=np.asarray(ref_data, np.int64),
               label=np.asarray(ref_label, np.int64), rounds=np.int64(info["rounds"]),
               round_end=np.array(info["round_end"], np.int64), t_index=info["t_index"], reward=info["reward"],
               r_dist=info["r_dist"], u_reset=info["reset_u"], m_reset=info["reset_margin"])
    from xenoverse_amd.metalang.stream_host import default_T_choices
    out["T_choices"] = default_T_choices()
    for k in ("u_policy", "u_greedy", "u_low", "u_query"):
        out[k] = _pad([s[k] for s in subs], 0.5, np.float64, width)
        out[k + "_n"] = np.array([len(s[k]) for s in subs], np.int32)
    for k in ("m_policy", "m_greedy", "m_low", "m_query", "g_label", "g_greedy"):
        out[k] = _pad([s[k] for s in subs], np.inf, np.float64, width)
    path = os.path.join(GOLD, "metalmstream_%s.npz" % name)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("%s: call seed %d, L %d, %d rounds, %d sub-steps, width %d, smallest margin or gap %.2e, reward distance %.2e, "
          "%d bytes" % (name, call_seed, L, info["rounds"], len(subs), width, worst, r_dist, size))
    if size > MAX_BYTES:
        raise SystemExit("%s: %d bytes is over the cap of %d" % (name, size, MAX_BYTES))


CONFIGS = [  # name, datatype, sampler seed, V, E, H
    ("qar_v32_e16_h32", "QAR", 401, 32, 16, 32),
    ("qa_v32_e16_h32", "QA", 402, 32, 16, 32),
    ("qara_v32_e16_h32", "QARA", 403, 32, 16, 32),
    ("qar_v100_e12_h24", "QAR", 404, 100, 12, 24),
    ("qara_v256_e16_h64", "QARA", 405, 256, 16, 64),
]


def main():
    for cfg in CONFIGS:
        gen(*cfg)


if __name__ == "__main__":
    main()
