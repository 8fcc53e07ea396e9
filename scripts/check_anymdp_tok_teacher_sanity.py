"""CPU evidence for tests/test_gpu_anymdp_tok_rollout.py::test_teacher_beats_random: on each tests/golden/anymdptok_*.npz task
(one action token per step, the task's own max_steps) 200 envs x 2,000 steps of oracle.AnyMDPTokOracle under SAME_STEP,
driven by the reference's greedy table (tests/golden/teacher_anymdptok_ref.npz) and by uniformly random actions.  Prints the
mean reward_gt of both and the gap in standard errors (per-env means, 200 independent envs).

usage: python scripts/check_anymdp_tok_teacher_sanity.py
"""
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle  # noqa: E402
from util import GOLD, load_anymdp_tok_golden  # noqa: E402
from xenoverse_amd.anymdp.tables import build_obs_tables, build_tables  # noqa: E402

N, T, SEED, BASE = 200, 2000, 77, 1000


def run(task, greedy):
    tab = build_tables([task])
    obs_cdf, _, _, d_act = build_obs_tables([task], tab["S"])
    env_task = np.zeros(N, np.int32)
    ora = oracle.AnyMDPTokOracle(tab, env_task, obs_cdf, d_act)
    ora.tok_reset(SEED, BASE, 0)
    rng = np.random.RandomState(1)
    total = np.zeros(N)
    for ts in range(T):
        a = greedy[ora.state] if greedy is not None else rng.randint(0, tab["A"], N)
        o = ora.tok_step(SEED, BASE, 1 + ts, a.astype(np.int32).reshape(N, 1), 2)
        total += o[2]
    return total / T


def main():
    ref = np.load(os.path.join(GOLD, "teacher_anymdptok_ref.npz"))
    for path in sorted(glob.glob(os.path.join(GOLD, "anymdptok_*.npz"))):
        name = os.path.basename(path)[:-4]
        task = dict(load_anymdp_tok_golden(path)[1])
        if "da" in task:
            task["da"] = 1
        te, ra = run(task, ref["greedy_" + name]), run(task, None)
        se = np.sqrt(te.var(ddof=1) / N + ra.var(ddof=1) / N)
        print("%s: teacher %.4f  random %.4f  gap %.4f = %.1f standard errors" % (name, te.mean(), ra.mean(), te.mean() - ra.mean(),
                                                                                 (te.mean() - ra.mean()) / se))


if __name__ == "__main__":
    main()
