"""The MetaLMV3 training streams on the host: the reference's generate_data_v3_single_task_qa / _qar / _qara
(xenoverse/metalang/generator_v3.py:48-173) over RandomLMHost, and its sample_and_check_task (:25-46).

A ROUND is one pass of the reference's while loop; a SUB-STEP is one policy() + step() pair (QA and QAR: one per round, QARA:
two).  Per round, with q s a the marker tokens, obs the current query, act an answer, LABEL the len(act) + 1 tokens of
label_answer(act) and r the reward token:
    data    QAR  q obs s a act s r          QA  q obs s a act s        QARA  q obs s a act1 s r a act2 s
    label   QAR  obs s a LABEL s r q        QA  obs s a act s q        QARA  obs s a LABEL1 s r a LABEL2 s q
so the label stream runs ahead of the data stream by one token per round in QAR and by two in QARA; in QA the two stay
aligned.  Kept verbatim from the reference:
  - data and label are cut to L independently; the loop ends when len(data) >= L, so the last round is usually cut;
  - the QAR reward token: r1 for r < 0, r2 for r < 0.5, r3 for r < 1, r4 for r < 2, r5 otherwise;
  - the QARA reward token in the reference's order: r> if r1 - r2 > 0.20, otherwise r< if r1 - r2 < 0.5, otherwise r=
    (which only a NaN reaches);
  - QARA's first sub-step is cached (no new query, the language model's state stays); its second generates the next query;
  - QA answers at T = 1e-3 and never uses the reward; QAR and QARA draw a temperature per answer from T_choices
    (default numpy.logspace(-1, 4, num=20)).
Uniforms and temperature choices are arguments, as everywhere in lm_host.py, indexed by sub-step k: t_index[k] and
draws["u_policy" | "u_greedy" | "u_low" | "u_query"][k] (the query draws of QARA's first sub-step are unused), with
draws["u_reset"] for the query of reset().  What is not given comes from the language model's private generator."""
import numpy as np

from .lm_host import FUNCTION_VOCABULARY, RandomLMHost, TaskSamplerV3, reward

DATATYPES = ("QA", "QAR", "QARA")
SHORTEST_ROUND = {"QA": 4, "QAR": 5, "QARA": 7}      # data tokens of a round whose query and answers are empty
QAR_THRESHOLDS = (0.0, 0.5, 1.0, 2.0)
QARA_THRESHOLD = 0.20      # the only comparison of the QARA token that a finite difference can fall on either side of
QA_TEMPERATURE = 1.0e-3


def default_T_choices():
    return np.logspace(-1, 4, num=20)


def qar_reward_token(r, vocab=FUNCTION_VOCABULARY):
    if r < 0:
        return vocab["r1"]
    elif r < 0.5:
        return vocab["r2"]
    elif r < 1.0:
        return vocab["r3"]
    elif r < 2.0:
        return vocab["r4"]
    return vocab["r5"]


def qara_reward_token(r1, r2, vocab=FUNCTION_VOCABULARY):
    deta = r1 - r2
    if deta > 0.20:
        return vocab["r>"]
    elif deta < 0.5:
        return vocab["r<"]
    return vocab["r="]


def marks_of(vocab=FUNCTION_VOCABULARY):
    """the 11 marker tokens in the order the C-ABI takes them: s q a r1..r5 r> r= r<"""
    return [int(vocab[k]) for k in ("s", "q", "a", "r1", "r2", "r3", "r4", "r5", "r>", "r=", "r<")]


def _sub_step(lm, T, cached, draws, k, subs):
    """policy(T) and step(answer, cached) of the reference's env (metalangv3.py:28-42) -> (answer, label, reward, query or
    None); appends the sub-step's record to subs"""
    def u(key):
        if draws is None or draws.get(key) is None:
            return None
        return draws[key][k]
    rec = {}
    ans, _ = lm.generate_answer_softmax(T=T, u=u("u_policy"))
    rec["u_policy"], rec["m_policy"] = lm.last["u"], lm.last["margin"]
    label, ppl = lm.label_answer(ans)
    rec["g_label"] = lm.last["gap"]
    _, ppl_min = lm.generate_answer_greedy(u=u("u_greedy"))
    rec["u_greedy"], rec["m_greedy"], rec["g_greedy"] = lm.last["u"], lm.last["margin"], lm.last["gap"]
    _, ppl_max = lm.generate_answer_low(u=u("u_low"))
    rec["u_low"], rec["m_low"] = lm.last["u"], lm.last["margin"]
    r = reward(ppl, ppl_min, ppl_max)
    query = None
    rec["u_query"], rec["m_query"] = np.zeros(0), np.zeros(0)
    if not cached:
        query = lm.generate_query(u=u("u_query"))
        rec["u_query"], rec["m_query"] = lm.last["u"], lm.last["margin"]
    rec.update(action=ans, label=label, reward=float(r), ppl=(float(ppl), float(ppl_min), float(ppl_max)))
    subs.append(rec)
    return ans, label, float(r), query


def stream_lm(lm, datatype, L, next_t, T_choices, draws=None, vocab=FUNCTION_VOCABULARY):
    """the three generators over one RandomLMHost.  next_t(k) -> the index into T_choices of sub-step k's temperature.
    -> data, label (int64 [L] each: the loop runs until data has L tokens, and label is never the shorter), info"""
    if datatype not in DATATYPES:
        raise ValueError("datatype must be one of QAR, QA, QARA")
    if int(L) < 1:
        raise ValueError("L must be at least 1")
    L = int(L)
    s, q, a = vocab["s"], vocab["q"], vocab["a"]
    data, label, subs, round_end, t_used, r_dist = [], [], [], [], [], []
    obs = lm.generate_query(u=None if draws is None or draws.get("u_reset") is None else draws["u_reset"])
    info = dict(reset_u=lm.last["u"], reset_margin=lm.last["margin"])
    k = 0

    def temperature():
        if datatype == "QA":
            t_used.append(-1)
            return QA_TEMPERATURE
        i = int(next_t(k))
        t_used.append(i)
        return float(T_choices[i])

    while len(data) < L:
        if datatype == "QARA":
            act1, label1, r1, _ = _sub_step(lm, temperature(), True, draws, k, subs)
            k += 1
            act2, label2, r2, nxt = _sub_step(lm, temperature(), False, draws, k, subs)
            k += 1
            r_token = qara_reward_token(r1, r2, vocab)
            r_dist += [np.inf, abs((r1 - r2) - QARA_THRESHOLD)]
            data += [q] + list(obs) + [s, a] + act1 + [s, r_token, a] + act2 + [s]
            label += list(obs) + [s, a] + label1 + [s, r_token, a] + label2 + [s, q]
        else:
            act, lab, r, nxt = _sub_step(lm, temperature(), False, draws, k, subs)
            k += 1
            if datatype == "QAR":
                r_token = qar_reward_token(r, vocab)
                r_dist.append(min(abs(r - t) for t in QAR_THRESHOLDS))
                data += [q] + list(obs) + [s, a] + act + [s, r_token]
                label += list(obs) + [s, a] + lab + [s, r_token, q]
            else:
                r_dist.append(np.inf)
                data += [q] + list(obs) + [s, a] + act + [s]
                label += list(obs) + [s, a] + act + [s, q]
        obs = nxt
        round_end.append((len(data), len(label)))
    info.update(subs=subs, round_end=round_end, rounds=len(round_end), t_index=np.array(t_used, np.int32),
                reward=np.array([x["reward"] for x in subs]), r_dist=np.array(r_dist))
    return np.array(data[:L]), np.array(label[:L]), info


def generate_data_v3_host(task, datatype, L, t_index=None, T_choices=None, draws=None):
    """-> data, label, info.  task: the dict of TaskSamplerV3 (its language model is copied, not used).  t_index: the index
    into T_choices per sub-step (None: drawn); draws: see the module's text.  info: per sub-step `subs` (answer, label,
    reward, the consumed uniforms, every draw's margin and every argmax's gap), `reward`, `t_index`, `r_dist` (the
    distance of the reward to the nearest threshold of its token), `round_end` (the lengths of data and label after every
    round) and `rounds`."""
    src = task["lm"] if isinstance(task["lm"], RandomLMHost) else RandomLMHost.from_reference(task["lm"])
    lm = RandomLMHost(src.enc_w, src.rnn_w, src.rnn_b, src.dec_w, src.dec_b, stop_token=src.stop_token,
                      function_tokens=src.function_token_list, max_len=src.max_len)
    T_choices = default_T_choices() if T_choices is None else np.asarray(T_choices, np.float64).reshape(-1)
    n = len(T_choices)
    if t_index is None or datatype == "QA":      # QA answers at its fixed temperature
        def next_t(k):
            return min(int(lm._rs.random_sample() * n), n - 1)
    else:
        t_index = [int(i) for i in np.asarray(t_index).reshape(-1)]
        if any(not 0 <= i < n for i in t_index):
            raise ValueError("t_index must hold indices into the %d T_choices" % n)

        def next_t(k):
            if k >= len(t_index):
                raise ValueError("the stream needs more than the %d temperature indices it was given" % len(t_index))
            return t_index[k]
    vocab = task.get("function_vocabulary") or FUNCTION_VOCABULARY
    return stream_lm(lm, datatype, L, next_t, T_choices, draws, vocab)


# ---- task acceptance (generator_v3.py:25-46) ---------------------------------------------------------------------------
CHECK_T_LOW, CHECK_T_HIGH = 10000, 1.0e-6


def accepts(reward_low, reward_high):
    """the reference's loop condition, negated: while (reward_high < 2.0 or reward_low > 0.0)"""
    return not (reward_high < 2.0 or reward_low > 0.0)


def check_task_host(task):
    """reset, policy(T=10000), step(cached), policy(T=1e-6), step(cached) on the host -> (reward_low, reward_high)"""
    src = task["lm"]
    lm = RandomLMHost(src.enc_w, src.rnn_w, src.rnn_b, src.dec_w, src.dec_b, stop_token=src.stop_token,
                      function_tokens=src.function_token_list, seed=0)
    lm.generate_query()
    subs = []
    _, _, low, _ = _sub_step(lm, CHECK_T_LOW, True, None, 0, subs)
    _, _, high, _ = _sub_step(lm, CHECK_T_HIGH, True, None, 1, subs)
    return low, high


def sample_tasks_host(n, vocab_size, embedding_size, hidden_size, seed):
    """the host path of sample_and_check_tasks -> (tasks, the seeds they came from)"""
    tasks, seeds = [], []
    while len(tasks) < n:
        task = TaskSamplerV3(vocab_size, embedding_size, hidden_size, seed=seed)
        if accepts(*check_task_host(task)):
            tasks.append(task)
            seeds.append(seed)
        seed += 1
    return tasks, seeds
