"""Host task samplers (CPU): the reference's dict schemas and invariants; tasks flow through the table builders."""
import os

import numpy as np
import pytest

from xenoverse_amd.linds import LinearDSSampler, LinearDSSamplerRandomDim, build_tables as linds_tables
from xenoverse_amd.mazeworld import MazeTaskSampler, Resampler, build_tables as maze_tables
from xenoverse_amd.mazeworld.task_sampler import genmaze


def _connected(w):
    free = np.argwhere(w == 0)
    seen = {tuple(free[0])}
    stack = [tuple(free[0])]
    while stack:
        i, j = stack.pop()
        for d in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            c = (i + d[0], j + d[1])
            if w[c] == 0 and c not in seen:
                seen.add(c); stack.append(c)
    return len(seen) == len(free)


def test_genmaze_connected_border_density():
    for n in (7, 15, 25):
        for loops in (False, True):
            w = genmaze(n, np.random.RandomState(n), allow_loops=loops, wall_density=0.3)
            assert w.shape == (n, n) and w.dtype == np.int8
            assert w[0].all() and w[-1].all() and w[:, 0].all() and w[:, -1].all()
            assert _connected(w)
            if loops:
                assert w[1:-1, 1:-1].mean() <= 0.45


def test_maze_task_schema_and_determinism():
    keys = {"start", "cell_walls", "cell_texts", "cell_size", "ground_text", "ceiling_text", "step_reward",
            "goal_reward", "collision_reward", "wall_height", "agent_height", "fol_angle", "commands_sequence",
            "landmarks_coordinates", "cell_landmarks"}
    t = MazeTaskSampler(n_range=(15, 16), seed=3)
    assert set(t) == keys and t["cell_walls"].shape == (15, 15)
    assert 1.5 <= t["cell_size"] <= 4.5 and 2 <= t["wall_height"] <= 6 and 1.6 <= t["agent_height"] <= 2.0
    assert len(t["commands_sequence"]) == 200 and 5 <= len(t["landmarks_coordinates"]) <= 14
    assert np.all(np.diff(t["commands_sequence"]) != 0)
    assert t["cell_walls"][t["start"]] == 0 and t["cell_landmarks"][t["start"]] == -1
    for q, c in enumerate(t["landmarks_coordinates"]):
        assert t["cell_walls"][c] == 0 and t["cell_landmarks"][c] == q
    assert abs(t["goal_reward"] - 15 * np.sqrt(15) / 60) < 1e-12
    t2 = MazeTaskSampler(n_range=(15, 16), seed=3)
    assert np.array_equal(t["cell_walls"], t2["cell_walls"]) and t["start"] == t2["start"]
    r = Resampler(t, seed=1)
    assert np.array_equal(r["cell_walls"], t["cell_walls"]) and not np.array_equal(r["commands_sequence"], t["commands_sequence"])
    tab = maze_tables([t, MazeTaskSampler(n_range=(9, 10), seed=4)])
    assert tab["NG"] == 15 and tab["walls"].shape == (2, 15, 15) and np.all(tab["walls"][1, 9:, :] == 1)


def test_seeded_maze_sampler_reproduces_reference_tasks():
    """MazeTaskSampler(seed=k) equals the reference's task for that seed: the three 15x15 tasks inside the maze fixtures
    and 24 more over the default size range, with and without loops (tests/golden/sampler_refmazes.npz): topology with
    its large rooms, textures, landmarks, start, commands, scalars"""
    import os
    from util import GOLD, golden_files, load_maze_golden
    kw = dict(n_wall_textures=8, n_ground_textures=4, n_ceiling_textures=4)
    for k, p in enumerate(golden_files("maze_")):
        g, ref = load_maze_golden(p)
        t = MazeTaskSampler(n_range=(15, 16), seed=k, **kw)
        for key in ("cell_walls", "cell_texts", "commands_sequence", "cell_landmarks"):
            assert np.array_equal(np.asarray(t[key]), np.asarray(ref[key])), (k, key)
        for key in ("cell_size", "wall_height", "agent_height", "fol_angle", "goal_reward", "ground_text", "ceiling_text"):
            assert float(t[key]) == float(ref[key]), (k, key)
        assert tuple(t["start"]) == tuple(ref["start"])
        assert [tuple(x) for x in t["landmarks_coordinates"]] == [tuple(x) for x in ref["landmarks_coordinates"]]
    g = np.load(os.path.join(GOLD, "sampler_refmazes.npz"))
    rooms = 0
    for k, seed in enumerate(g["seed"]):
        t = MazeTaskSampler(seed=int(seed), allow_loops=bool(g["allow_loops"][k]), commands_sequence=32, **kw)
        n = int(g["n"][k])
        assert t["cell_walls"].shape == (n, n)
        assert np.array_equal(t["cell_walls"], g["cell_walls"][k][:n, :n]), seed
        assert np.array_equal(t["cell_texts"], g["cell_texts"][k][:n, :n]) and np.array_equal(t["cell_landmarks"], g["cell_landmarks"][k][:n, :n])
        assert tuple(t["start"]) == tuple(g["start"][k]) and np.array_equal(t["commands_sequence"], g["commands"][k])
        nl = int(g["n_landmarks"][k])
        assert [tuple(x) for x in t["landmarks_coordinates"]] == [tuple(x) for x in g["landmarks"][k][:nl]]
        sc = [t["cell_size"], t["wall_height"], t["agent_height"], t["fol_angle"], t["goal_reward"], t["ground_text"], t["ceiling_text"]]
        assert np.array_equal(np.asarray(sc, np.float64), g["scalars"][k])
        w = t["cell_walls"]          # a 2x2 block of open cells can only come from a large room (or loops at low density)
        rooms += int(((w[:-1, :-1] + w[1:, :-1] + w[:-1, 1:] + w[1:, 1:]) == 0).any())
    assert rooms >= len(g["seed"]) // 2


def test_linds_sampler_follows_the_reference_stream():
    """tests/golden/sampler_reflinds.npz: 14 tasks of the reference's LinearDSSampler with its (timestamp-based) seeding
    function pinned to numpy.random.seed(seed) — LinearDSSampler(seed=k) consumes a RandomState(k) in the same order and
    returns the same task, including the cases where the rejection loop ran for dozens of draws"""
    import os
    from util import GOLD
    g = np.load(os.path.join(GOLD, "sampler_reflinds.npz"))
    for k, seed in enumerate(g["seed"]):
        ns, na, no = [int(x) for x in g["dims"][k]]
        t = LinearDSSampler(ns, na, no, seed=int(seed))
        assert t["max_steps"] == g["max_steps"][k]
        assert np.array_equal(t["ld_A"], g["A"][k][:ns, :ns]) and np.array_equal(t["ld_B"], g["B"][k][:ns, :na])
        assert np.array_equal(t["ld_C"], g["C"][k][:no, :ns]) and np.array_equal(t["ld_X"], g["X"][k][:ns])
        assert np.array_equal(t["ld_Y"], g["Y"][k][:no])
        assert np.array_equal([t["action_cost"], t["reward_base"], t["terminate_punish"], t["reward_factor"]], g["scal"][k])
        assert np.array_equal(t["target_valid"], g["valid"][k][:no])
        assert (t["target_type"] == "dynamic_target") == bool(g["is_dyn"][k])
        n0 = int(g["n_init"][k])
        assert len(t["initial_states"]) == n0 and np.array_equal(np.asarray(t["initial_states"])[:8], g["init"][k][:min(8, n0), :ns])
        assert float(t["noise_drift"]) == g["noise_drift"][k] and t["target_delay"] == g["delay"][k]
        if g["is_dyn"][k]:
            assert len(t["command"].coeffs) == g["four_n"][k]
            for i, (o, c) in enumerate(t["command"].coeffs):
                assert float(o) == g["four_orders"][k][i] and np.array_equal(c, g["four_coeffs"][k][i][:no])
        else:
            assert np.array_equal(t["command"], g["cmd"][k][:no])


def test_linds_task_schema_all_dims_terminate():
    for dims in ((16, 8, 8), (32, 8, 8), (32, 8, 16), (4, 2, 3)):
        t = LinearDSSampler(*dims, seed=dims[0])
        assert t["ld_A"].shape == (dims[0], dims[0]) and t["ld_B"].shape == (dims[0], dims[1])
        assert t["ld_C"].shape == (dims[2], dims[0]) and 100 <= t["max_steps"] < 1000
        assert t["target_type"] in ("static_target", "dynamic_target") and len(t["initial_states"]) >= 1
        cmd = t["command"] if t["target_type"] == "static_target" else t["command"](-t["target_delay"])
        for x0 in t["initial_states"]:
            assert np.linalg.norm((cmd - t["ld_C"] @ x0 - t["ld_Y"]) * t["target_valid"]) <= 3.0
        tab = linds_tables([t], pad_observation_dim=16)
        assert tab["phiT"].shape[1] == dims[0]
    t = LinearDSSamplerRandomDim(seed=5)
    assert t["state_dim"] <= 16


def test_anymdp_task_sampler_schema_and_validity():
    import time
    from xenoverse_amd.anymdp import AnyMDPTaskSampler, AnyPOMDPTaskSampler, MultiTokensAnyPOMDPTaskSampler
    from xenoverse_amd.anymdp import build_obs_tables, build_tables, validate_task
    from xenoverse_amd.anymdp.task_sampler import check_task
    t0 = time.time()
    t = AnyMDPTaskSampler(16, 4, seed=0)
    assert set(t) >= {"ns", "na", "max_steps", "state_mapping", "task_type", "s_0", "s_0_prob", "s_e", "transition",
                      "reward", "reward_noise", "final_goal_terminate"}
    assert t["transition"].shape == (16, 4, 16) == t["reward"].shape == t["reward_noise"].shape
    assert 100 <= t["max_steps"] <= 128 and sorted(t["state_mapping"]) == list(range(16))
    validate_task(t)                                  # the checks AnyMDPEnv.set_task performs
    assert check_task(t)
    assert np.all(t["transition"][list(t["s_e"])] == 0) and np.all(t["reward_noise"] >= 0)
    t2 = AnyMDPTaskSampler(16, 4, seed=0)
    assert np.array_equal(t["transition"], t2["transition"]) and t["max_steps"] == t2["max_steps"]
    t64 = AnyMDPTaskSampler(64, 8, seed=1)            # the reference needs ~9 minutes for this without numba
    validate_task(t64)
    assert time.time() - t0 < 120
    nnz = (t64["transition"] > 0).sum(-1)
    assert nnz.max() <= 64 // 2 + 64 // 4 + 4          # banded rows
    p = AnyPOMDPTaskSampler(16, 4, observation_space=16, seed=2)
    assert p["task_type"] == "POMDP" and p["observation_transition"].shape == (16, 16)
    assert np.allclose(p["observation_transition"].sum(1), 1.0)
    m = MultiTokensAnyPOMDPTaskSampler(16, 4, observation_space=16, seed=3)
    assert m["task_type"] == "MTPOMDP" and len(m["observation_transition"]) == m["do"] == 4 and m["da"] == 2
    tab = build_tables([m])
    cdf, n_obs, d_obs, d_act = build_obs_tables([m], tab["S"])
    assert cdf.shape == (1, 4, 16, 16) and (n_obs, d_obs, d_act) == (16, 4, 2)


def _numpy_matches_fixture_host():
    """The fixtures were written on a host whose NumPy evaluates exp/log with its AVX512 kernels; those differ from the
    scalar/AVX2 kernels in the last bit for a few per cent of the arguments, so the reference itself gives (slightly)
    different task tensors per machine class.  Bit-for-bit equality is asserted where this fingerprint matches."""
    x = np.linspace(-30.0, 0.0, 4097)
    import hashlib
    return hashlib.sha256(np.exp(x).tobytes()).hexdigest()[:16] == "b3409591d6bdf429"


def _same(a, b, exact):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array_equal(a, b) if exact else (a.shape == b.shape and np.allclose(a, b, rtol=1e-9, atol=1e-12))


@pytest.mark.parametrize("name,ns,na,seed", [("anymdp_16x4_seed0", 16, 4, 0), ("anymdp_16x4_seed1", 16, 4, 1),
                                             ("anymdp_16x4_seed2", 16, 4, 2), ("anymdp_16x4_seed3", 16, 4, 3),
                                             ("anymdp_64x8_seed1", 64, 8, 1)])
def test_seeded_anymdp_sampler_reproduces_the_reference_task(name, ns, na, seed):
    """AnyMDPTaskSampler(ns, na, seed) == the task the reference's sampler returned for that seed (the fixtures' task
    tensors): same random stream, same draw order, same value-iteration arithmetic in the repair loop"""
    import os
    from util import GOLD, load_anymdp_golden
    from xenoverse_amd.anymdp import AnyMDPTaskSampler
    g, ref = load_anymdp_golden(os.path.join(GOLD, name + ".npz"))
    t = AnyMDPTaskSampler(ns, na, seed=seed)
    exact = _numpy_matches_fixture_host()
    assert float(t["max_steps"]) == float(ref["max_steps"])
    for k in ("state_mapping", "s_0", "s_e"):
        assert np.array_equal(np.asarray(t[k]).reshape(-1), np.asarray(ref[k]).reshape(-1)), k
    for k in ("s_0_prob", "transition", "reward", "reward_noise"):
        assert _same(t[k], ref[k], exact), k


@pytest.mark.parametrize("name,kind,seed", [("anymdptok_pomdp_16x4_seed5", "pomdp", 5),
                                            ("anymdptok_mtpomdp_16x4_seed0", "mt", 0),
                                            ("anymdptok_mtpomdp_16x4_seed6", "mt", 6)])
def test_seeded_pomdp_samplers_reproduce_the_reference_tasks(name, kind, seed):
    """the emission matrices come from the SAME stream, right after the MDP (task_sampler.py:78-87,103-117)"""
    import os
    from util import GOLD, load_anymdp_tok_golden
    from xenoverse_amd.anymdp import AnyPOMDPTaskSampler, MultiTokensAnyPOMDPTaskSampler
    g, ref = load_anymdp_tok_golden(os.path.join(GOLD, name + ".npz"))
    fn = AnyPOMDPTaskSampler if kind == "pomdp" else MultiTokensAnyPOMDPTaskSampler
    t = fn(16, 4, observation_space=16, seed=seed)
    exact = _numpy_matches_fixture_host()
    assert np.array_equal(t["state_mapping"], ref["state_mapping"]) and np.array_equal(t["s_e"], ref["s_e"])
    for k in ("transition", "reward", "reward_noise"):
        assert _same(t[k], ref[k], exact), k
    assert _same(np.asarray(t["observation_transition"]), np.asarray(ref["observation_transition"]), True)


def test_seeded_sampler_reproduces_32_reference_sampled_tasks():
    """tests/golden/sampler_refpop_16x4.npz: 128 tasks of the reference's sampler (seeds 100..227) with its own
    candidate / unrepairable / rejected counts — the build's sampler walks the same candidates"""
    import os
    from util import GOLD
    from xenoverse_amd.anymdp import task_sampler as ts
    g = np.load(os.path.join(GOLD, "sampler_refpop_16x4.npz"))
    exact = _numpy_matches_fixture_host()
    counts = {"cand": 0, "none": 0, "rej": 0}
    real_cand, real_acc = ts._ReferenceStream.candidate, ts.reference_acceptance

    def cand(self, *a, **k):
        r = real_cand(self, *a, **k)
        counts["cand"] += 1
        counts["none"] += r is None
        return r

    def acc(task):
        ok = real_acc(task)
        counts["rej"] += not ok
        return ok
    ts._ReferenceStream.candidate, ts.reference_acceptance = cand, acc
    try:
        for k, seed in enumerate(g["seed"]):
            for c in counts:
                counts[c] = 0
            t = ts.AnyMDPTaskSampler(16, 4, seed=int(seed))
            assert (counts["cand"], counts["none"], counts["rej"]) == (g["n_cand"][k], g["n_none"][k], g["n_rej"][k]), seed
            assert float(t["max_steps"]) == float(g["max_steps"][k])
            assert np.array_equal(np.nonzero(g["s_e_mask"][k])[0], np.asarray(t["s_e"], np.int64).reshape(-1))
            assert bool(t["final_goal_terminate"]) == bool(g["goal"][k])
            for kk in ("transition", "reward", "reward_noise"):
                assert _same(t[kk], g[kk][k], exact), (seed, kk)
    finally:
        ts._ReferenceStream.candidate, ts.reference_acceptance = real_cand, real_acc


def test_acceptance_rule_agrees_with_reference_when_available():
    """the reference's check_valuefunction and value iteration vs this restatement, on the reference's stored results
    (oracle/gen_golden.py anymdp, anymdp_vi, anymdp_accept): every task the reference sampled passes check_task here,
    value_iteration agrees with its update_value_matrix, and the tasks sampled here are the ones its own test accepted"""
    from xenoverse_amd.anymdp import AnyMDPTaskSampler
    from xenoverse_amd.anymdp.task_sampler import check_task, value_iteration
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    gamma = 2.0 ** (-1.0 / 16)
    vi = np.load(os.path.join(gold, "sampler_vi_ref.npz"))
    for seed in range(4):
        g = np.load(os.path.join(gold, "anymdp_16x4_seed%d.npz" % seed))
        task = {k: g[k] for k in ("transition", "reward", "max_steps", "s_0", "s_0_prob", "s_e")}
        assert check_task(task), seed                 # every task the reference accepted passes here too
        if seed in (0, 2):                            # the reference's update_value_matrix at check_valuefunction's gamma
            assert np.array_equal(vi["T%d" % seed], task["transition"])
            assert vi["gamma%d" % seed][1] == gamma
            q_ref = vi["vm_s%d_g1_1" % seed]
            q = value_iteration(task["transition"], task["reward"], gamma)
            assert np.max(np.abs(q - q_ref)) < 5e-3 * (1 + np.abs(q_ref).max())
    acc = np.load(os.path.join(gold, "sampler_accept_ref_16x4.npz"))
    for k, seed in enumerate(acc["seed"]):
        mine = AnyMDPTaskSampler(16, 4, seed=int(seed))
        T, R = np.asarray(mine["transition"], np.float64), np.asarray(mine["reward"], np.float64)
        assert _same(T, acc["transition%d" % k], False) and _same(R, acc["reward%d" % k], False), seed
        assert bool(acc["accepted%d" % k]), seed     # and a task sampled here passes the reference's own test
        assert check_task(mine), seed
        for key, greedy in (("vm_opt", True), ("vm_rnd", False)):
            q_ref = acc["%s%d" % (key, k)]
            q = value_iteration(T, R, gamma, greedy=greedy)
            assert np.max(np.abs(q - q_ref)) < 5e-3 * (1 + np.abs(q_ref).max()), (seed, key)


def test_sample_batch_returns_stacked_tables():
    """every sampler module has sample_batch(n, **kw) -> one dict of stacked arrays, which
    set_task accepts as it is; task k equals the k-th individually sampled task"""
    from xenoverse_amd.anymdp import task_sampler as a_ts
    from xenoverse_amd.anymdp.tables import build_tables as a_build, row_lines
    from xenoverse_amd.linds import task_sampler as l_ts
    from xenoverse_amd.mazeworld import task_sampler as m_ts
    b = a_ts.sample_batch(3, seed=5, state_space=16, action_space=4)
    assert b["rows"].shape == (3, 16, 4, row_lines(16), 16) and b["state_map"].shape == (3, 16)
    one = a_build([a_ts.AnyMDPTaskSampler(16, 4, seed=6)])
    assert np.array_equal(b["rows"][1], one["rows"][0]) and np.array_equal(b["max_steps"][1:2], one["max_steps"])
    lb = l_ts.sample_batch(2, seed=1, state_dim=16, action_dim=8, observation_dim=8)
    assert lb["phiT"].shape[0] == 2 and lb["NS"] == 16
    mb = m_ts.sample_batch(2, seed=3, n_range=(9, 10))
    assert mb["walls"].shape[0] == 2 and mb["walls"].shape[1:] == (9, 9)


def test_garnet_sampler_reproduces_the_reference_task():
    """GarnetTaskSampler(8, 2, b=2, sigma=0.1, seed=3) equals the task the reference sampled (fixture from
    oracle/gen_golden.py garnet), bit for bit; structure: b non-zeros per row summing to 1, no terminal states"""
    import os
    from xenoverse_amd.anymdp import GarnetTaskSampler
    from xenoverse_amd.anymdp.tables import build_tables
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "garnet_8x2_seed3.npz"))
    t = GarnetTaskSampler(8, 2, b=2, sigma=0.1, seed=3)
    assert float(t["max_steps"]) == float(g["max_steps"])
    assert np.array_equal(t["state_mapping"], g["state_mapping"])
    assert np.array_equal(t["transition"], g["transition"]) and np.array_equal(t["reward"], g["reward"])
    big = GarnetTaskSampler(32, 5, min_state_space=10, b=3, seed=1)
    T = big["transition"]
    assert np.all((T > 0).sum(-1) == 3) and np.allclose(T.sum(-1), 1.0) and len(big["s_e"]) == 0
    tab = build_tables([big])
    assert tab["S"] == T.shape[0] and tab["A"] == 5
    with pytest.raises(ValueError):
        GarnetTaskSampler(8, 2, b=1)


def test_vi_summation_orders():
    """`update_value_matrix` is @njit in the reference: numba reduces np.mean sequentially, the interpreter pairwise.  The
    C++ Gauss-Seidel offers both; the sequential order is checked against a plain Python restatement of the sweep
    (solver.py:57-82) with sequential sums, the default stays the pairwise one the fixtures pin."""
    from xenoverse_amd.anymdp.task_sampler import gauss_seidel_values, set_vi_summation
    rng = np.random.RandomState(5)
    ns, na = 6, 9                                   # na >= 8: the two orders can differ
    T = rng.rand(ns, na, ns) * (rng.rand(ns, na, ns) < 0.6)
    T[..., 0] += 1e-3
    T /= T.sum(-1, keepdims=True)
    R = rng.randn(ns, na, ns)
    gamma = 0.9

    def seq_mean(v):
        acc = 0.0
        for x in v:
            acc += float(x)
        return acc / len(v)

    def sweep_sequential():
        vm = np.zeros((ns, na))
        diff, alpha = 1.0, 1.0
        while diff > 1e-4:
            old = vm.copy()
            for s in range(ns):
                for a in range(na):
                    exp_q = 0.0
                    for sn in range(ns):
                        if T[s, a, sn] == 0.0:
                            continue
                        exp_q += T[s, a, sn] * (gamma * seq_mean(vm[sn]) + R[s, a, sn])
                    vm[s, a] += alpha * (exp_q - vm[s, a])
            diff = np.sqrt(seq_mean(((old - vm) ** 2).ravel()))
            alpha = max(0.80 * alpha, 0.50)
        return vm

    try:
        set_vi_summation("numba")
        got = gauss_seidel_values(T, R, gamma, greedy=False)
        assert np.array_equal(got, sweep_sequential())
    finally:
        set_vi_summation("numpy")
    ref = gauss_seidel_values(T, R, gamma, greedy=False)
    assert np.allclose(ref, got, rtol=0, atol=1e-9)
    with pytest.raises(KeyError):
        set_vi_summation("other")


def test_maze_sampler_defaults_are_the_reference_texture_counts():
    """tests/golden/sampler_refmazes_refcounts.npz: tasks of the reference's MazeTaskSampler sampled with ITS OWN texture
    folder behind it (37 wall / 29 ground / 21 ceiling images — only the counts enter a task).  MazeTaskSampler(seed=k)
    with its default library sizes returns the same task, all keys."""
    import os
    from util import GOLD
    from xenoverse_amd.mazeworld import REFERENCE_TEXTURE_COUNTS
    g = np.load(os.path.join(GOLD, "sampler_refmazes_refcounts.npz"))
    assert tuple(int(c) for c in g["counts"]) == REFERENCE_TEXTURE_COUNTS == (37, 29, 21)
    big_ids = 0
    for k, seed in enumerate(g["seed"]):
        t = MazeTaskSampler(seed=int(seed), commands_sequence=32)
        n = int(g["n"][k])
        assert t["cell_walls"].shape == (n, n) and np.array_equal(t["cell_walls"], g["cell_walls"][k][:n, :n]), seed
        assert np.array_equal(t["cell_texts"], g["cell_texts"][k][:n, :n]), seed
        assert np.array_equal(t["cell_landmarks"], g["cell_landmarks"][k][:n, :n])
        assert tuple(t["start"]) == tuple(g["start"][k]) and np.array_equal(t["commands_sequence"], g["commands"][k])
        nl = int(g["n_landmarks"][k])
        assert [tuple(x) for x in t["landmarks_coordinates"]] == [tuple(x) for x in g["landmarks"][k][:nl]]
        sc = [t["cell_size"], t["wall_height"], t["agent_height"], t["fol_angle"], t["goal_reward"], t["ground_text"], t["ceiling_text"]]
        assert np.array_equal(np.asarray(sc, np.float64), g["scalars"][k])
        big_ids += int(t["cell_texts"].max() >= 8)
    assert big_ids == len(g["seed"])          # texture ids beyond the old 8-texture default really occur
    # and the default procedural library holds them: what MazeWorldVecEnv.set_task checks before uploading
    from xenoverse_amd.mazeworld.textures import texture_counts
    assert texture_counts(dict(walls=np.zeros((37, 1)), grounds=np.zeros((29, 1)), ceilings=np.zeros((21, 1)))) == (37, 29, 21)


def test_load_texture_library_reads_a_folder_like_the_reference(tmp_path):
    """load_texture_library: sorted file order, wall* / ground* / ceiling* prefixes, everything else ignored, RGB decoded
    and handed out with pygame.surfarray.array3d's (W, H, 3) axes as float32 (task_sampler.py:60-77)"""
    from PIL import Image
    from xenoverse_amd.mazeworld import load_texture_library, texture_counts
    rng = np.random.RandomState(0)
    W, H = 256, 256                 # the engine's texture size (and that of every image of the reference's folder)
    imgs = {}
    for name in ("wall_b.png", "wall_a.png", "ground_1.png", "ceiling_z.png", "ceiling_y.png", "ceiling_x.png",
                 "notes.txt", "mywall.png"):
        if name.endswith(".txt"):
            (tmp_path / name).write_text("not an image")
            continue
        a = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)        # PIL's (H, W, 3)
        Image.fromarray(a).save(tmp_path / name)
        imgs[name] = a
    Image.fromarray(rng.randint(0, 256, (H, W)).astype(np.uint8), mode="L").save(tmp_path / "ground_0_gray.png")
    lib = load_texture_library(str(tmp_path))
    assert texture_counts(lib) == (2, 2, 3)
    assert lib["walls"].dtype == np.float32 and lib["walls"].shape == (2, W, H, 3)
    assert np.array_equal(lib["walls"][0], imgs["wall_a.png"].transpose(1, 0, 2))         # sorted: a before b
    assert np.array_equal(lib["walls"][1], imgs["wall_b.png"].transpose(1, 0, 2))
    assert np.array_equal(lib["ceilings"][2], imgs["ceiling_z.png"].transpose(1, 0, 2))
    assert np.array_equal(lib["grounds"][1], imgs["ground_1.png"].transpose(1, 0, 2))
    gray = lib["grounds"][0]                                        # a grey-scale file is converted to RGB
    assert np.array_equal(gray[..., 0], gray[..., 1]) and np.array_equal(gray[..., 1], gray[..., 2])
    (tmp_path / "sub").mkdir()
    with pytest.raises(ValueError, match="no wall"):
        load_texture_library(str(tmp_path / "sub"))
    # the reference's own folder, by its file names (tests/golden/sampler_reftexture_names.npz; the images are not kept)
    ref_dir = tmp_path / "ref"
    ref_dir.mkdir()
    blank = Image.fromarray(np.zeros((256, 256, 3), np.uint8))
    for name in np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_reftexture_names.npz"))["names"]:
        if str(name).startswith(("wall", "ground", "ceiling")):
            blank.save(ref_dir / str(name))
        else:                                                       # (.DS_Store, .gitattributes: not read)
            (ref_dir / str(name)).write_bytes(b"")
    assert texture_counts(load_texture_library(str(ref_dir))) == (37, 29, 21)


def test_texture_libraries_of_another_size_are_refused_or_resampled(tmp_path):
    """the ray caster addresses textures as 256 x 256 x 3: an image of another size must never reach it as it is"""
    from PIL import Image
    from xenoverse_amd.mazeworld import load_texture_library
    from xenoverse_amd.mazeworld.textures import check_texture_library, make_texture_library
    rng = np.random.RandomState(1)
    for name, (w, h) in (("wall_0.png", (256, 256)), ("wall_1.png", (64, 48)), ("ground_0.png", (256, 256)),
                         ("ceiling_0.png", (300, 256))):
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(tmp_path / name)
    with pytest.raises(ValueError, match="ceiling_0.png is 300 x 256"):
        load_texture_library(str(tmp_path))
    lib = load_texture_library(str(tmp_path), resize=True)
    assert lib["walls"].shape == (2, 256, 256, 3) and lib["ceilings"].shape == (1, 256, 256, 3)
    assert lib["walls"].min() >= 0 and lib["walls"].max() <= 255
    check_texture_library(lib)
    check_texture_library(make_texture_library(2, 1, 1, seed=0))
    bad = dict(lib, grounds=np.zeros((1, 128, 128, 3), np.float32))
    with pytest.raises(ValueError, match=r"'grounds' has shape \(1, 128, 128, 3\)"):
        check_texture_library(bad)
    with pytest.raises(ValueError, match="lacks 'ceilings'"):
        check_texture_library({"walls": lib["walls"], "grounds": lib["grounds"]})


def test_acrobot_kernel_sincos_construction_is_within_one_ulp_of_libm():
    """csrc/acrobot.hip: ac_sincos (Cody-Waite reduction + minimax kernels) with the constants read from the source,
    restated in NumPy: at most 1 ulp from glibc's sin / cos over +-1000 (the oracle calls glibc; states are compared at 1e-9)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_ac_sincos", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "scripts", "devtools", "check_ac_sincos.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    worst, same = m.check(100000)
    assert worst <= 1.0 and same > 0.95, (worst, same)
