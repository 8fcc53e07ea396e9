"""Host restatement (numpy) of the device Garnet and bandit task samplers (csrc/anymdp_garnet.hip: xv_anymdp_sample_garnet,
xv_anymdp_sample_bandits): the same Philox counters and constructions (host_draws.py), and the tables `build_tables` forms
from the tasks.  The device equals it bit for bit in everything made of integers and fp64 sums, differences, products and
quotients (the transition tensor, every CDF entry, state_map, max_steps, n_real, the bandit statuses away from the
threshold) and to the device-sampler tolerance where `log`, `cos` and `sin` enter (reward, reward_noise)
(tests/test_gpu_garnet_bandit_sampler.py).  It is also the CPU-side proof that the models are the reference's
GarnetTaskSampler (xenoverse/anymdp/task_sampler.py:120-160, task_sampler_utils.py:274-313) and its single-state task
(task_sampler_utils.py:258-272) (tests/test_host_garnet_bandit_sampler.py).

Task k of (seed, arguments) is a pure function of those, whatever the batch — but not the task numpy's stream gives for
that seed (for that, `GarnetTaskSampler(seed=...)` / `AnyMDPTaskSampler(state_space=1, seed=...)`).

Garnet: every index is a task.  The draws (index layout, key = seed, counter = {k lo, k hi, sub, purpose | tick << 8}):
  purpose 0, tick 0, sub 0: first uniform -> max_steps = uniform(u, lower, upper); second -> n = m + floor(u (S - m + 1))
  purpose 1, tick 0, sub = i >> 1: step i of the state_mapping Fisher-Yates on arange(S), i = 0 .. n - 1 (at most S - 2):
      swap position i with i + floor(u (S - i)), u half i & 1 of the call; the first n positions are final after n steps
  purpose 2, tick = row s A + a, sub = i >> 1: step i = 0 .. b - 1 of the row's partial Fisher-Yates on arange(n)
  purpose 3, tick = row, sub = j >> 1: cut j = 0 .. b - 2 of the row (a u53 uniform), half j & 1; sorted ascending
  purpose 4, tick 0, sub = q >> 1: reward element q = (s A + a) n + s' is the cos (q even) or sin (q odd) member of the
      call's Box-Muller pair
Every floor(u m) is clamped to m - 1 (never reached: u <= 1 - 2^-53), on both sides.

Bandit: index = candidate.  purpose 0, tick 0, sub 0: first uniform -> base = clip(expo(u), 0.05, 2.0), second ->
noise_base = max(uniform(u, -0.30, 0.30), 0); purpose 1, tick = round r, sub = a >> 1: reward[a] = uniform(u, 0.5 base,
base), u half a & 1.  The first round with numpy.std(reward) > 0.01 is accepted (std in numpy's order: host_draws.np_sum
twice); none within max_rounds: status 1, "no_spread", and the candidate is skipped.  Task k is the k-th accepted candidate.
"""
import numpy as np

from ..host_draws import M64, Draws, box_muller, expo, floor_int, interleave, np_sum, pair, philox4x32_10, uniform
from .tables import A_MAX, S_MAX, build_tables

P_HEAD, P_PERM, P_SUCC, P_CUT, P_REWARD = 0, 1, 2, 3, 4        # csrc/anymdp_garnet.hip GN_P_*
B_HEAD, B_ROUND = 0, 1                                         # csrc/anymdp_garnet.hip BD_P_*
B_MAX = 32                                                     # include/xeno.h XV_ANYMDP_GARNET_B_MAX
ROUNDS_MAX = 1 << 16                                           # include/xeno.h XV_ANYMDP_BANDIT_ROUNDS_MAX
BANDIT_STATUS = ("accepted", "no_spread")
STD_MIN = 0.01


def check_garnet_args(state_space, action_space, min_state_space, b):
    """-> (S, A, m): m the smallest real state count, S when min_state_space is None.  ValueError naming the limit for
    anything the device sampler does not take"""
    S, A, b = int(state_space), int(action_space), int(b)
    if not 8 <= S <= S_MAX:
        raise ValueError("Garnet: state_space = %d is outside the supported range 8 .. %d" % (S, S_MAX))
    if not 2 <= A <= A_MAX:
        raise ValueError("Garnet: action_space = %d is outside the supported range 2 .. %d" % (A, A_MAX))
    m = S if min_state_space is None else min(int(min_state_space), S)
    if m < 8:
        raise ValueError("Garnet: min_state_space = %d is below the minimum of 8" % m)
    if not 2 <= b <= min(B_MAX, m):
        raise ValueError("Garnet: b = %d is outside the supported range 2 .. min(%d, smallest real state count = %d)"
                         % (b, B_MAX, m))
    return S, A, m


def max_steps_bounds(S):
    lower = max(4.0 * S, 100)
    return lower, max(min(8.0 * S, 500), lower + 1)


def _floor_clamped(u, m):
    return np.minimum(floor_int(u, m), np.asarray(m, np.int64) - 1)


def _row_block(seed, k, purpose, rows, count):
    """`count` uniforms for each of `rows` rows -> float64[rows, count]: element i of row r is half i & 1 of the call
    {purpose, tick = r, sub = i >> 1} (Draws.block with the row as the tick, all rows at once)"""
    seed, k = int(seed) & M64, int(k) & M64
    i = np.arange(int(count))
    ctr = np.empty((int(rows), int(count), 4), np.uint32)
    ctr[..., 0], ctr[..., 1] = k & 0xFFFFFFFF, k >> 32
    ctr[..., 2] = (i >> 1)[None, :]
    ctr[..., 3] = int(purpose) | (np.arange(int(rows), dtype=np.uint32)[:, None] << np.uint32(8))
    a, b = pair(philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32)))
    return interleave(i[None, :], a, b)


def garnet_task(seed, k, state_space=128, action_space=5, min_state_space=None, b=2, sigma=0.1):
    """task k -> the reference's task dict (the model: DESIGN.md §3.1.2)"""
    S, A, m = check_garnet_args(state_space, action_space, min_state_space, b)
    b = int(b)
    d = Draws(seed, k)
    u0, u1 = d.pairs(P_HEAD, 0)
    lower, upper = max_steps_bounds(S)
    max_steps = uniform(float(u0), lower, upper)
    n = S if min_state_space is None else m + int(_floor_clamped(u1, S - m + 1))
    # state_mapping: the first n entries of a forward Fisher-Yates on arange(S)
    perm = np.arange(S)
    steps = min(n, S - 1)
    up = d.block(P_PERM, steps)
    for i in range(steps):
        j = i + int(_floor_clamped(up[i], S - i))
        perm[i], perm[j] = perm[j], perm[i]
    # successors and cuts of every row
    rows = n * A
    i_b = np.arange(b)
    off = _floor_clamped(_row_block(seed, k, P_SUCC, rows, b), n - i_b[None, :])          # [rows, b]
    cuts = np.sort(_row_block(seed, k, P_CUT, rows, b - 1), axis=1)
    cuts = np.concatenate([np.zeros((rows, 1)), cuts, np.ones((rows, 1))], axis=1)
    pieces = cuts[:, 1:] - cuts[:, :-1]
    transition = np.zeros((rows, n))
    arr = np.empty(n, np.int64)
    for r in range(rows):
        arr[:] = np.arange(n)
        for i in range(b):
            j = i + int(off[r, i])
            arr[i], arr[j] = arr[j], arr[i]
        transition[r, arr[:b]] = pieces[r]
    q = np.arange(rows * n)
    zc, zs = box_muller(*d.pairs(P_REWARD, q >> 1))
    reward = (interleave(q, zc, zs) * float(sigma) + 0.0).reshape(n, A, n)
    return {"ns": S, "na": A, "max_steps": max_steps, "state_mapping": perm[:n].copy(), "task_type": "MDP",
            "s_0": np.array([0]), "s_0_prob": np.array([1.0]), "s_e": np.array([], dtype=int),
            "transition": transition.reshape(n, A, n), "reward": reward, "reward_noise": np.zeros((n, A, n)),
            "final_goal_terminate": False}


def garnet_tasks(n_tasks, state_space=128, action_space=5, min_state_space=None, b=2, sigma=0.1, seed=0, task_base=0):
    return [garnet_task(seed, int(task_base) + i, state_space, action_space, min_state_space, b, sigma)
            for i in range(int(n_tasks))]


def _with_dense(tab, tasks, S, A):
    """the dense tensors of a table dict: fp64 [n_task, S, A, S], zero outside a task's real states"""
    for key in ("transition", "reward", "reward_noise"):
        out = np.zeros((len(tasks), S, A, S))
        for i, t in enumerate(tasks):
            n = t[key].shape[0]
            out[i, :n, :, :n] = t[key]
        tab[key] = out
    return tab


def sample_tables(n_tasks, state_space=128, action_space=5, min_state_space=None, b=2, sigma=0.1, seed=0, s0_max=4,
                  task_base=0):
    """tasks task_base .. task_base + n_tasks - 1 -> what build_tables(task dicts, s0_max=s0_max) returns for them, at
    S = state_space whatever their real state counts, + n_real int32[n_tasks] and the dense transition / reward /
    reward_noise fp64 [n_tasks, S, A, S]"""
    S, A, _ = check_garnet_args(state_space, action_space, min_state_space, b)
    tasks = garnet_tasks(n_tasks, S, A, min_state_space, b, sigma, seed, task_base)
    tab = build_tables(tasks, s0_max=s0_max)
    if tab["S"] != S:      # no task of the batch drew the full size: pad to the sampler's S, as build_tables pads a ragged batch
        tab = pad_tables(tab, S)
    tab["n_real"] = np.array([t["transition"].shape[0] for t in tasks], np.int32)
    return _with_dense(tab, tasks, S, A)


def pad_tables(tab, S):
    """a build_tables dict at its own S -> the same tasks at a larger S, by build_tables' padding rules (CDF 1.0, zero
    pairs, state_map 0)"""
    from .tables import to_blocked
    n_task, S0, A = tab["cdf"].shape[:3]
    cdf = np.ones((n_task, S, A, S))
    cdf[:, :S0, :, :S0] = tab["cdf"]
    rs = np.zeros((n_task, S, A, S, 2), np.float32)
    rs[:, :S0, :, :S0] = tab["rs"]
    state_map = np.zeros((n_task, S), np.int32)
    state_map[:, :S0] = tab["state_map"]
    term_mask = np.zeros((n_task, (S + 63) // 64), np.uint64)
    term_mask[:, :tab["term_mask"].shape[1]] = tab["term_mask"]
    return dict(tab, S=S, cdf=cdf, rs=rs, rows=to_blocked(cdf, rs), state_map=state_map, term_mask=term_mask)


# ---- bandits ----------------------------------------------------------------------------------------------------------------

def check_bandit_args(action_space, max_rounds):
    A, R = int(action_space), int(max_rounds)
    if not 2 <= A <= A_MAX:
        raise ValueError("bandit: action_space = %d is outside the supported range 2 .. %d" % (A, A_MAX))
    if not 1 <= R <= ROUNDS_MAX:
        raise ValueError("bandit: max_rounds = %d is outside the supported range 1 .. %d" % (R, ROUNDS_MAX))
    return A, R


def np_std(x):
    """numpy.std of a contiguous fp64 vector in numpy's order of operations (numpy/_core/_methods.py _var): the mean from a
    pairwise sum, the squared deviations, their pairwise sum over the count, the root"""
    x = np.asarray(x, np.float64).reshape(-1)
    mean = np_sum(x) / float(len(x))
    dev = x - mean
    return float(np.sqrt(np_sum(dev * dev) / float(len(x))))


def bandit_candidate(seed, cand, action_space=5, max_rounds=1024):
    """candidate `cand` -> (status, task dict or None, record): record has base, noise_base, the deciding round and the
    std of every round looked at"""
    A, R = check_bandit_args(action_space, max_rounds)
    d = Draws(seed, cand)
    u0, u1 = d.pairs(B_HEAD, 0)
    base = float(np.clip(expo(float(u0)), 0.05, 2.0))
    noise_base = max(uniform(float(u1), -0.30, 0.30), 0.0)
    stds = []
    for r in range(R):
        reward = uniform(d.block(B_ROUND, A, tick=r), 0.5 * base, base)
        stds.append(np_std(reward))
        if stds[-1] > STD_MIN:
            break
    rec = dict(base=base, noise_base=noise_base, round=len(stds) - 1, stds=np.array(stds))
    if not stds[-1] > STD_MIN:
        return 1, None, rec
    task = {"ns": 1, "na": A, "max_steps": 1, "state_mapping": np.array([0]), "task_type": "MDP",
            "transition": np.ones((1, A, 1), dtype=float), "reward": reward.reshape(1, A, 1),
            "reward_noise": (noise_base * reward).reshape(1, A, 1), "s_0": np.array([0]), "s_e": np.array([]),
            "s_0_prob": np.array([1.0])}
    return 0, task, rec


def bandit_candidates(seed, cand_base, n_cand, action_space=5, max_rounds=1024):
    """-> (status int32[n_cand], tasks (None where rejected), records)"""
    res = [bandit_candidate(seed, int(cand_base) + i, action_space, max_rounds) for i in range(int(n_cand))]
    return np.array([r[0] for r in res], np.int32), [r[1] for r in res], [r[2] for r in res]


def bandit_tasks(n_tasks, action_space=5, seed=0, max_rounds=1024, batch=64):
    """the first n_tasks accepted candidates -> (task dicts, status histogram over the candidates looked at); the batch
    does not matter"""
    tasks, hist, base = [], np.zeros(len(BANDIT_STATUS), np.int64), 0
    while len(tasks) < n_tasks:
        st, ts, _ = bandit_candidates(seed, base, batch, action_space, max_rounds)
        for s, t in zip(st, ts):
            hist[s] += 1
            if s == 0:
                tasks.append(t)
                if len(tasks) == n_tasks:
                    break
        base += batch
    return tasks, hist


def bandit_tables(tasks, s0_max=4):
    """bandit task dicts -> build_tables' two-inner-state embedding + the dense reward / reward_noise fp64 [n, 1, A, 1]
    and transition (ones)"""
    tab = build_tables(tasks, s0_max=s0_max)
    tab["n_real"] = np.ones(len(tasks), np.int32)
    for key in ("transition", "reward", "reward_noise"):
        tab[key] = np.stack([np.asarray(t[key], np.float64) for t in tasks])
    return tab


def sample_bandit_tables(n_tasks, action_space=5, seed=0, max_rounds=1024, s0_max=4):
    tasks, hist = bandit_tasks(n_tasks, action_space, seed, max_rounds)
    tab = bandit_tables(tasks, s0_max)
    tab["stats"] = dict(candidates=int(hist.sum()), accepted=int(hist[0]),
                        status={k: int(v) for k, v in zip(BANDIT_STATUS, hist)})
    return tab
