"""The ground-truth teacher's table on the POMDP / multi-token POMDP fixtures against the reference's AnyMDPSolverOpt
(tests/golden/teacher_anymdptok_ref.npz, scripts/gen_golden_anymdp_tok_teacher.py)."""
import os

import numpy as np
import pytest

from xenoverse_amd.anymdp.teacher import optimal_policy_table
from util import GOLD, golden_files, load_anymdp_tok_golden

FILES = golden_files("anymdptok_")


def test_fixture_covers_the_three_tasks():
    ref = np.load(os.path.join(GOLD, "teacher_anymdptok_ref.npz"))
    assert len(FILES) == 3
    for p in FILES:
        name = os.path.basename(p)[:-4]
        g, _ = load_anymdp_tok_golden(p)
        q = ref["q_" + name]
        assert q.shape == (int(g["ns"]), int(g["na"])) and q.dtype == np.float64
        assert np.array_equal(ref["greedy_" + name], q.argmax(1))      # numpy.argmax: the first maximum, as policy() takes it
    assert float(ref["gamma"]) == 0.99


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(p)[:-4] for p in FILES])
def test_reference_argmax_equals_optimal_policy_table(path):
    """every state the teacher can act from: all but the terminal ones (s_e), whose rows are never read"""
    ref = np.load(os.path.join(GOLD, "teacher_anymdptok_ref.npz"))
    _, task = load_anymdp_tok_golden(path)
    greedy = ref["greedy_" + os.path.basename(path)[:-4]]
    live = np.ones(len(greedy), bool)
    live[np.asarray(task["s_e"], np.int64)] = False
    assert live.sum() >= len(greedy) - len(task["s_e"]) and live.any()
    ours = optimal_policy_table(task, gamma=0.99)[0]
    assert np.array_equal(ours[live], greedy[live])
