"""what the MetaLMV3 stream tests share: the fixtures of scripts/gen_golden_metalm_stream.py (tests/golden/metalmstream_*.npz)
and the splice of policy() / step() results into the three stream formats"""
import numpy as np

from util import golden_files

FILES = golden_files("metalmstream_")
NAMES = ["qa_v32_e16_h32", "qar_v100_e12_h24", "qar_v32_e16_h32", "qara_v256_e16_h64", "qara_v32_e16_h32"]
WEIGHTS = ("enc_w", "rnn_w", "rnn_b", "dec_w", "dec_b")
PASSES = ("u_policy", "u_greedy", "u_low", "u_query")
MARGINS = ("m_reset", "m_policy", "m_greedy", "m_low", "m_query", "g_label", "g_greedy")


def fixture_id(path):
    return path.rsplit("metalmstream_", 1)[-1][:-4]


def load(path):
    """-> (fixture dict, task dict)"""
    from xenoverse_amd.metalang import FUNCTION_VOCABULARY, RandomLMHost
    g = dict(np.load(path, allow_pickle=False))
    lm = RandomLMHost(*(g[k] for k in WEIGHTS), stop_token=int(g["stop_token"]),
                      function_tokens=[int(t) for t in g["function_tokens"]])
    task = dict(vocabulary=int(g["n_vocab"]), embedding=int(g["n_emb"]), hidden=int(g["n_hidden"]),
                function_vocabulary=dict(FUNCTION_VOCABULARY), lm=lm)
    return g, task


def host_draws(g):
    """the recorded uniforms as generate_data_v3_host takes them"""
    d = {k: [g[k][i, :int(g[k + "_n"][i])] for i in range(len(g["reward"]))] for k in PASSES}
    d["u_reset"] = g["u_reset"]
    return d


def smallest_margin(g):
    return min(float(g[k].min()) for k in MARGINS)


def splice(datatype, obs, subs, tokens):
    """one round of the reference's loop (generator_v3.py:72-91, 114-142, 156-172) appended to tokens = (data, label).
    obs: the round's query; subs: per sub-step (answer, label, reward), all as lists"""
    from xenoverse_amd.metalang import FUNCTION_VOCABULARY as v
    from xenoverse_amd.metalang.stream_host import qar_reward_token, qara_reward_token
    data, label = tokens
    s, q, a = v["s"], v["q"], v["a"]
    if datatype == "QARA":
        (act1, lab1, r1), (act2, lab2, r2) = subs
        rt = qara_reward_token(r1, r2)
        data += [q] + obs + [s, a] + act1 + [s, rt, a] + act2 + [s]
        label += obs + [s, a] + lab1 + [s, rt, a] + lab2 + [s, q]
    elif datatype == "QAR":
        (act, lab, r), = subs
        rt = qar_reward_token(r)
        data += [q] + obs + [s, a] + act + [s, rt]
        label += obs + [s, a] + lab + [s, rt, q]
    else:
        (act, lab, r), = subs
        data += [q] + obs + [s, a] + act + [s]
        label += obs + [s, a] + act + [s, q]


def row_of(tokens, L):
    """a spliced list as the device's row: cut to L, zeros behind"""
    out = np.zeros(L, np.int32)
    n = min(len(tokens), L)
    out[:n] = tokens[:n]
    return out
