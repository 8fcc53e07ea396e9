"""Golden fixture of the ground-truth teacher on the POMDP / multi-token POMDP tasks: the REFERENCE's
AnyMDPSolverOpt(env, gamma=0.99) (xenoverse/anymdp/anymdp_solver_opt.py) on each tests/golden/anymdptok_*.npz task — its
value_matrix (S x A float64) and value_matrix.argmax(1), the table its policy() reads at env.inner_state (:38-51).

Build-container tooling, like scripts/gen_golden_anymdp_qlearn.py: the reference is imported read-only through
oracle/_refimport.py with the stand-ins of oracle/stubs; nothing under oracle/ is modified.

Checked here, on the CPU, before anything is written: the reference's argmax equals
xenoverse_amd.anymdp.teacher.optimal_policy_table at every state that is not in s_e (terminal states are never acted
from; their rows are all-zero transitions and the two solvers may leave different values there).  The script also prints
max |Q_ref - Q_ours| (the reference's Gauss-Seidel sweep stops early) and the smallest top-two margin on a live state.

Only data is written: tests/golden/teacher_anymdptok_ref.npz (keys q_<task>, greedy_<task>, gamma).  The name puts the
family last, as mbrl_anymdp_* and qlearn_anymdp_* do: the tests of the token tasks enumerate tests/golden/anymdptok_*.npz as
TASK fixtures, and this file is not one.

usage: python scripts/gen_golden_anymdp_tok_teacher.py
"""
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import _refimport  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
GAMMA = 0.99


def load_task(path):
    """the task dict of an anymdptok_* fixture (as tests/util.py: load_anymdp_tok_golden)"""
    g = dict(np.load(path, allow_pickle=False))
    mt = bool(g["is_mt"])
    task = dict(ns=int(g["ns"]), na=int(g["na"]), max_steps=float(g["max_steps"]), state_mapping=g["state_mapping"],
                task_type="MTPOMDP" if mt else "POMDP", s_0=g["s_0"], s_0_prob=g["s_0_prob"], s_e=g["s_e"],
                transition=g["transition"], reward=g["reward"], reward_noise=g["reward_noise"], no=int(g["no"]))
    if mt:
        task.update(do=int(g["do"]), da=int(g["da"]), observation_transition=[m for m in g["observation_transition"]])
    else:
        task["observation_transition"] = g["observation_transition"][0]
    return task


def main():
    AnyMDPEnv, _ = _refimport.anymdp()
    from xenoverse.anymdp.anymdp_solver_opt import AnyMDPSolverOpt
    from xenoverse_amd.anymdp.teacher import optimal_policy_table, optimal_q

    out = {"gamma": np.float64(GAMMA)}
    for path in sorted(glob.glob(os.path.join(GOLD, "anymdptok_*.npz"))):
        name = os.path.basename(path)[:-4]
        task = load_task(path)
        env = AnyMDPEnv(max_steps=5000)
        env.set_task(task)
        q = np.array(AnyMDPSolverOpt(env, gamma=GAMMA).value_matrix, np.float64)
        greedy = q.argmax(1)
        ours = optimal_policy_table(task, gamma=GAMMA)[0]
        live = np.ones(q.shape[0], bool)
        live[np.asarray(task["s_e"], np.int64)] = False
        assert np.array_equal(greedy[live], ours[:q.shape[0]][live]), name
        srt = np.sort(q[live], axis=1)
        print("%s: S x A = %d x %d, %d live states, max |dQ| = %.3g, smallest top-two margin = %.3g" % (
            name, q.shape[0], q.shape[1], int(live.sum()), float(np.abs(q - optimal_q(task, GAMMA))[live].max()),
            float((srt[:, -1] - srt[:, -2]).min())))
        out["q_" + name] = q
        out["greedy_" + name] = greedy.astype(np.uint8)
    dst = os.path.join(GOLD, "teacher_anymdptok_ref.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
