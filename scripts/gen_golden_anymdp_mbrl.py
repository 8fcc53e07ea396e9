"""Golden fixtures of the AnyMDP model-based agent: the REFERENCE's own training loop (xenoverse/anymdp/test_utils.py:
train, epoch_run :42-60) with AnyMDPEnv and AnyMDPSolverMBRL (xenoverse/anymdp/anymdp_solver_mbrl.py), reset on done.

Build-container tooling, like scripts/gen_golden_anymdp_qlearn.py: the reference is imported read-only through
oracle/_refimport.py with the stand-ins of oracle/stubs; nothing under oracle/ is modified.  numpy's global RandomState is
seeded before every reset, step and policy call, and the numbers each call consumed are replayed from RandomState(seed) and
stored: the policy's A uniforms (random.uniform(0, 1, A) = random_sample(A)), the step's transition uniform and reward
normal, the reset's uniform.  update_value_matrix's one random.random() inside learner() (the loop guard, always < 1) is
therefore harmless.  Tasks: tests/golden/anymdp_16x4_seed<k>.npz, anymdp_64x8_seed1.npz, and a 20x3 and a 48x5 task from
the project's seeded sampler (xenoverse_amd.anymdp.AnyMDPTaskSampler, which reproduces the reference's).  Per step the
fixture holds (obs, action, next_obs, r, terminated, truncated, is_test), the draws and the MARGIN of the policy's choice:
the gap between the two largest entries of vm[o] + b[o] u (of vm[o] on greedy steps); snapshots of vm, b and vis_cnt_sa, and
of est_r and vis_cnt at fewer points.

A second file, mbrl_value_sweep.npz, holds random (t, r, vm) inputs and the reference's
update_value_matrix(t, r, gamma, vm, max_iteration=1) of each.

Only data is written: tests/golden/mbrl_anymdp_<name>.npz, tests/golden/mbrl_value_sweep.npz.

usage: python scripts/gen_golden_anymdp_mbrl.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import _refimport  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
TASK_KEYS = ("ns", "na", "max_steps", "state_mapping", "s_0", "s_0_prob", "s_e", "transition", "reward", "reward_noise")


def _task_from_file(src):
    g = dict(np.load(os.path.join(GOLD, src + ".npz"), allow_pickle=False))
    return {k: g[k] for k in TASK_KEYS}


def _task_sampled(S, A, seed):
    from xenoverse_amd.anymdp import AnyMDPTaskSampler
    t = AnyMDPTaskSampler(state_space=S, action_space=A, seed=seed)
    out = {k: np.asarray(t[k]) for k in TASK_KEYS}
    out["ns"], out["na"], out["max_steps"] = np.int64(t["ns"]), np.int64(t["na"]), np.float64(t["max_steps"])
    return out


def _margin(solver, state, u, is_test):
    v = np.array(solver.value_matrix[state], np.float64)
    if not is_test:
        v = v + solver.b_mat[state] * u
    s = np.sort(v)
    return float(s[-1] - s[-2])


def gen(name, task_arrays, T, seed0, gamma=0.99, c=0.05, test_interval=None, test_epochs=3, snaps=10, full_snaps=3):
    AnyMDPEnv, _ = _refimport.anymdp()
    import xenoverse.anymdp.anymdp_env as envmod
    from xenoverse.anymdp.anymdp_solver_mbrl import AnyMDPSolverMBRL

    task = dict(task_arrays)
    task["ns"], task["na"], task["max_steps"] = int(task["ns"]), int(task["na"]), float(task["max_steps"])
    task["task_type"] = "MDP"
    env = AnyMDPEnv(max_steps=5000)
    env.set_task(task)
    solver = AnyMDPSolverMBRL(env, gamma=gamma, c=c)
    A = int(task["na"])

    inject = {"seed": 0}
    envmod.pseudo_random_seed = lambda *a, **k: inject["seed"]

    def ref_reset(seed):
        inject["seed"] = int(seed)
        obs, _ = env.reset()
        return obs, np.random.RandomState(int(seed)).random_sample()

    snap_at = sorted(set(int(x) for x in np.linspace(T // snaps, T, snaps)))
    full_at = sorted(set(int(x) for x in np.linspace(T // full_snaps, T, full_snaps)))
    rec = {k: np.zeros(T, np.int64) for k in ("obs", "action", "next_obs", "is_test")}
    rec.update({k: np.zeros(T) for k in ("r", "u", "z", "u_reset", "margin")})
    rec.update({k: np.zeros(T, np.uint8) for k in ("terminated", "truncated")})
    rec["u_policy"] = np.zeros((T, A))
    snap = {k: [] for k in ("vm", "b", "vis_cnt_sa", "est_r", "vis_cnt")}

    state, init_u = ref_reset(seed0)
    init_obs = state
    episode, is_test = 0, False
    for t in range(T):
        if is_test:
            u_pol = np.zeros(A)
            action = solver.policy(state, is_test=True)
        else:
            sp = seed0 + 1000000 + t
            np.random.seed(sp)
            action = solver.policy(state, is_test=False)
            u_pol = np.random.RandomState(sp).random_sample(A)
        rec["margin"][t] = _margin(solver, state, u_pol, is_test)
        ss = seed0 + 2000000 + t
        np.random.seed(ss)
        next_state, reward, terminated, truncated, info = env.step(int(action))
        rs = np.random.RandomState(ss)
        rec["u"][t] = rs.random_sample()
        rec["z"][t] = rs.standard_normal()
        solver.learner(state, action, next_state, reward, terminated, truncated)
        rec["obs"][t], rec["action"][t], rec["next_obs"][t], rec["r"][t] = state, action, next_state, reward
        rec["terminated"][t], rec["truncated"][t], rec["is_test"][t] = terminated, truncated, is_test
        rec["u_policy"][t] = u_pol
        state = next_state
        if terminated or truncated:
            state, rec["u_reset"][t] = ref_reset(seed0 + 3000000 + t)
            episode += 1
            if test_interval is not None:
                is_test = episode % (test_interval + test_epochs) >= test_interval
        if t + 1 in snap_at:
            snap["vm"].append(np.array(solver.value_matrix))
            snap["b"].append(np.array(solver.b_mat))
            snap["vis_cnt_sa"].append(np.array(solver.vis_cnt_sa))
        if t + 1 in full_at:
            snap["est_r"].append(np.array(solver.est_r))
            snap["vis_cnt"].append(np.array(solver.vis_cnt))

    out = dict(gamma=np.float64(gamma), c=np.float64(c), init_u=np.float64(init_u), init_obs=np.int64(init_obs),
               snap_at=np.array(snap_at, np.int64), full_at=np.array(full_at, np.int64), **rec)
    for k, v in snap.items():
        out["snap_" + k] = np.stack(v)
    for k in TASK_KEYS:
        out[k] = task_arrays[k]
    path = os.path.join(GOLD, "mbrl_anymdp_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("%s: %d steps, %d episodes, %d terminated, %d truncated, %d greedy steps, min margin %.2e, steps with margin "
          "< 1e-4: %d, %d bytes" % (name, T, episode, rec["terminated"].sum(), rec["truncated"].sum(), rec["is_test"].sum(),
                                    rec["margin"].min(), int((rec["margin"] < 1e-4).sum()), os.path.getsize(path)), flush=True)


def gen_sweeps():
    _refimport.setup()
    from xenoverse.anymdp.solver import update_value_matrix
    rng = np.random.RandomState(17)
    out = {}
    k = 0
    for S, A in ((4, 2), (16, 4), (20, 3), (48, 5), (64, 8)):
        for rep in range(2):
            t = rng.random_sample((S, A, S)) * (rng.random_sample((S, A, S)) < 0.3)
            t = t / np.maximum(t.sum(-1, keepdims=True), 0.01)
            r = rng.randn(S, A, S) * (t > 0)
            vm = rng.randn(S, A) * (rep + 1)
            gamma = 0.99 if rep == 0 else 0.9
            out["t%d" % k], out["r%d" % k], out["vm%d" % k], out["gamma%d" % k] = t, r, vm, np.float64(gamma)
            out["out%d" % k] = np.array(update_value_matrix(t, r, gamma, vm, max_iteration=1))
            k += 1
    out["n"] = np.int64(k)
    np.savez_compressed(os.path.join(GOLD, "mbrl_value_sweep.npz"), **out)
    print("mbrl_value_sweep: %d cases" % k)


def main():
    only = sys.argv[1:]
    jobs = [("16x4_seed0", lambda: _task_from_file("anymdp_16x4_seed0"), dict(T=2000, seed0=30000)),
            ("16x4_seed1", lambda: _task_from_file("anymdp_16x4_seed1"), dict(T=2000, seed0=37919, test_interval=8)),
            ("16x4_seed2_c1", lambda: _task_from_file("anymdp_16x4_seed2"), dict(T=2000, seed0=45838, c=1.0,
                                                                                   test_interval=6, test_epochs=2)),
            ("16x4_seed3", lambda: _task_from_file("anymdp_16x4_seed3"), dict(T=2000, seed0=53757, test_interval=8)),
            ("20x3_s5", lambda: _task_sampled(20, 3, 5), dict(T=1500, seed0=70000, test_interval=5)),
            ("48x5_s7", lambda: _task_sampled(48, 5, 7), dict(T=1200, seed0=80000, test_interval=4, full_snaps=2)),
            ("64x8_seed1", lambda: _task_from_file("anymdp_64x8_seed1"), dict(T=1500, seed0=60000, test_interval=3,
                                                                              full_snaps=2))]
    for name, task, kw in jobs:
        if not only or name in only:
            gen(name, task(), **kw)
    if not only or "sweep" in only:
        gen_sweeps()


if __name__ == "__main__":
    main()
