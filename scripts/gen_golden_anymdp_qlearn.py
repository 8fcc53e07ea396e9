"""Golden fixtures of the AnyMDP Q-learning agent: the REFERENCE's own training loop (xenoverse/anymdp/test_utils.py: train,
epoch_run :42-60) with AnyMDPEnv and AnyMDPSolverQ (xenoverse/anymdp/anymdp_solver_q.py), reset on done.

Build-container tooling, like oracle/gen_golden.py: the reference is imported read-only through oracle/_refimport.py with
the stand-ins of oracle/stubs; nothing under oracle/ is modified.  The reference draws from numpy's global legacy RandomState
and reseeds it from OS entropy at every reset (anymdp_env.py:87), so the global state is seeded before every reset, step and
policy call and the numbers each call consumed are replayed from RandomState(seed) and stored: the policy's uniform (one
random_sample per numpy.random.choice), the step's transition uniform and reward normal, the reset's uniform.  Tasks are
those of tests/golden/anymdp_<S>x<A>_seed<k>.npz.  Per step the fixture holds (obs, action, next_obs, r, terminated,
truncated; `reward` is the task's reward tensor), the draws, and the MARGIN of the policy's choice — the distance from u to
the nearest cut of the CDF numpy.random.choice searched (greedy test-epoch steps: the gap between the row's largest Q value
and the nearest other nonzero gap); the learner state (Q, sa_visits, s_visits) at a few snapshots and the state it
started from.

Only data is written: tests/golden/qlearn_anymdp_<name>.npz.

usage: python scripts/gen_golden_anymdp_qlearn.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import _refimport  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def _task(path):
    g = dict(np.load(path, allow_pickle=False))
    task = dict(ns=int(g["ns"]), na=int(g["na"]), max_steps=float(g["max_steps"]), state_mapping=g["state_mapping"],
                task_type="MDP", s_0=g["s_0"], s_0_prob=g["s_0_prob"], s_e=g["s_e"], transition=g["transition"],
                reward=g["reward"], reward_noise=g["reward_noise"])
    return g, task


def _policy_margin(solver, state, u, is_test):
    """the CDF numpy.random.choice searched for this draw, formed with the reference's own expressions (:51-59) -> margin"""
    q = np.array(solver.value_matrix[state], np.float64)
    if is_test:
        gaps = np.abs(np.delete(q, int(np.argmax(q))) - q.max())
        gaps = gaps[gaps > 0]
        return float(gaps.min()) if gaps.size else np.inf
    value = q - np.max(q)
    stiffness = min((solver.max_steps + solver.s_visitied[state]) / (solver.max_steps + 1), 10.0)
    value = value / max(np.std(value), 1.0e-2) * stiffness
    p = np.exp(value) / np.sum(np.exp(value))
    cdf = p.cumsum()
    cdf /= cdf[-1]
    return float(np.min(np.abs(cdf[:-1] - u))) if len(cdf) > 1 else np.inf


def gen(name, src, T, seed0, learner_max_steps=4000, gamma=0.99, alpha=0.5, test_interval=None, test_epochs=3,
        init_sa=None, snaps=12):
    """T steps of train()'s loop: `test_interval` training episodes, then `test_epochs` greedy ones, and so on (None: all
    training).  init_sa: sa_visitied the agent starts from (default: the reference's ones)."""
    AnyMDPEnv, _ = _refimport.anymdp()
    import xenoverse.anymdp.anymdp_env as envmod
    from xenoverse.anymdp.anymdp_solver_q import AnyMDPSolverQ

    g, task = _task(os.path.join(GOLD, src + ".npz"))
    env = AnyMDPEnv(max_steps=5000)
    env.set_task(task)
    solver = AnyMDPSolverQ(env, gamma=gamma, alpha=alpha, max_steps=learner_max_steps)
    if init_sa is not None:
        solver.sa_visitied[...] = init_sa
    init_q, init_sa_v, init_s_v = (np.array(x) for x in (solver.value_matrix, solver.sa_visitied, solver.s_visitied))

    inject = {"seed": 0}
    envmod.pseudo_random_seed = lambda *a, **k: inject["seed"]

    def ref_reset(seed):
        inject["seed"] = int(seed)
        obs, _ = env.reset()
        return obs, np.random.RandomState(int(seed)).random_sample()

    snap_at = sorted(set(int(x) for x in np.linspace(T // snaps, T, snaps)))       # after these many steps
    rec = {k: np.zeros(T, np.int64) for k in ("obs", "action", "next_obs", "is_test")}
    rec.update({k: np.zeros(T) for k in ("r", "u_policy", "u", "z", "u_reset", "margin")})
    rec.update({k: np.zeros(T, np.uint8) for k in ("terminated", "truncated")})
    snap_q, snap_sa, snap_s = [], [], []

    state, init_u = ref_reset(seed0)
    init_obs = state
    episode, is_test = 0, False
    for t in range(T):
        if is_test:
            action = solver.policy(state, is_test=True)
            u_pol = 0.0
        else:
            sp = seed0 + 1000000 + t
            np.random.seed(sp)
            action = solver.policy(state, is_test=False)
            u_pol = np.random.RandomState(sp).random_sample()
        rec["margin"][t] = _policy_margin(solver, state, u_pol, is_test)
        ss = seed0 + 2000000 + t
        np.random.seed(ss)
        next_state, reward, terminated, truncated, info = env.step(int(action))
        rs = np.random.RandomState(ss)
        rec["u"][t] = rs.random_sample()
        rec["z"][t] = rs.standard_normal()
        solver.learner(state, action, next_state, reward, terminated, truncated)
        rec["obs"][t], rec["action"][t], rec["next_obs"][t], rec["r"][t] = state, action, next_state, reward
        rec["terminated"][t], rec["truncated"][t], rec["u_policy"][t], rec["is_test"][t] = terminated, truncated, u_pol, is_test
        state = next_state
        if terminated or truncated:
            state, rec["u_reset"][t] = ref_reset(seed0 + 3000000 + t)
            episode += 1
            if test_interval is not None:
                k = episode % (test_interval + test_epochs)
                is_test = k >= test_interval
        if t + 1 in snap_at:
            snap_q.append(np.array(solver.value_matrix))
            snap_sa.append(np.array(solver.sa_visitied))
            snap_s.append(np.array(solver.s_visitied))

    out = dict(task_src=np.array(src), gamma=np.float64(gamma), alpha=np.float64(alpha),
               learner_max_steps=np.int64(learner_max_steps), init_u=np.float64(init_u), init_obs=np.int64(init_obs),
               init_q=init_q, init_sa=init_sa_v.astype(np.int64), init_s=init_s_v.astype(np.int64),
               snap_at=np.array(snap_at, np.int64), snap_q=np.stack(snap_q), snap_sa=np.stack(snap_sa).astype(np.int64),
               snap_s=np.stack(snap_s).astype(np.int64), **rec)
    for k in ("ns", "na", "max_steps", "state_mapping", "s_0", "s_0_prob", "s_e", "transition", "reward", "reward_noise"):
        out[k] = g[k]
    np.savez_compressed(os.path.join(GOLD, "qlearn_anymdp_%s.npz" % name), **out)
    print("%s: %d steps, %d episodes, %d terminated, %d truncated, %d greedy steps, min margin %.2e, steps with margin "
          "< 1e-4: %d, lr floor reached: %s, stiffness cap reached: %s" % (
              name, T, episode, rec["terminated"].sum(), rec["truncated"].sum(), rec["is_test"].sum(), rec["margin"].min(),
              int((rec["margin"] < 1e-4).sum()), bool((snap_sa[-1] > 1000 * (learner_max_steps + 1) - learner_max_steps).any()),
              bool((snap_s[-1] >= 9 * learner_max_steps + 10).any())))


def main():
    for k in range(4):
        gen("16x4_seed%d" % k, "anymdp_16x4_seed%d" % k, T=3000, seed0=20000 + 7919 * k,
            test_interval=(8 if k in (1, 3) else None))
    # learner max_steps = 1: the stiffness cap (s_visits >= 19) is met within a few steps; sa_visits starting at 1990-1999
    # cross the lr floor (sa_visits > 1999) on their first visits
    rng = np.random.RandomState(5)
    gen("16x4_m1", "anymdp_16x4_seed2", T=2000, seed0=90000, learner_max_steps=1,
        init_sa=1990 + rng.randint(0, 10, (16, 4)).astype(np.float64), test_interval=6, test_epochs=2)
    gen("64x8_seed1", "anymdp_64x8_seed1", T=3000, seed0=60000, test_interval=10)
    # 12 actions: the row sums of the policy (mean, std, softmax) take numpy's eight partial sums and a tail of four
    gen("24x12_seed0", "anymdp_24x12_seed0", T=3000, seed0=130000, test_interval=8)


if __name__ == "__main__":
    main()
