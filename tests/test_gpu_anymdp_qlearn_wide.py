"""The device Q-learner (csrc/anymdp_qlearn.hip) at wide action counts, against the host restatement
(xenoverse_amd/anymdp/qlearner.py): every register row of the policy (AM = 8, 16, 32, 64 doubles) and every part of the
device's restatement of numpy's pairwise sum (xv_np_sum: the plain loop below 8 elements, the accumulation rounds
r[k & 7] += f(k), the tail of n % 8 terms), which the mean, the std and the softmax sum of a row of A > 8 actions go
through.  The reference recordings have A <= 12; these are random tasks (util.anymdp_random_task)."""
import numpy as np
import pytest

from util import anymdp_env as _env, anymdp_random_task as _random_task, to_np as _np
from xenoverse_amd.anymdp import AnyMDPQLearner, QLearnerHost
from xenoverse_amd.anymdp.qlearner import policy_cdf

pytestmark = pytest.mark.gpu
N, T = 1024, 256
TIE = 1e-9          # the host's own margin below which an env's draw counts as a tie (the device's exp may differ from
#                     numpy's in the last bit: ~1e-16 relative on a probability)
MAX_LEFT_OUT = N // 1000      # at most 0.1 % of the envs

# (S, A): the register row AM and what of xv_np_sum a row of A values reaches
CASES = [(12, 5),     # AM 8: the plain loop at a non-power of two
         (12, 9),     # AM 16: no accumulation round, tail of 1
         (10, 16),    # AM 16: one accumulation round, no tail
         (10, 17),    # AM 32: one accumulation round, tail of 1
         (8, 31),     # AM 32: two accumulation rounds, tail of 7
         (8, 33),     # AM 64: three accumulation rounds, tail of 1
         (6, 63),     # AM 64: six accumulation rounds, tail of 7
         (6, 64)]     # AM 64: the full row, no tail


def _draws(rng, T_, n):
    return dict(u_policy=rng.random_sample((T_, n)), u=rng.random_sample((T_, n)),
                z=rng.standard_normal((T_, n)).astype(np.float32), u_reset=rng.random_sample((T_, n)))


def _train_against_host(S, A, greedy_T=0):
    """N envs over two random tasks (one with two terminal states, one with none; max_steps = 40), T steps with injected
    draws; the host is fed the device's observations, fp32 rewards and flags.  An env is left out from the first step at
    which the HOST's margin (the distance from u to the nearest cut of its policy_cdf) is below TIE.  Every other env:
    every action equal, Q and the counts bit-equal at the end.  greedy_T: that many greedy steps after the training, the
    actions against host.policy(greedy=True), the tables again."""
    tasks = [_random_task(S, A, seed=100 * S + A, max_steps=40, n_terminal=2),
             _random_task(S, A, seed=100 * S + A + 1, max_steps=40)]
    env = _env(tasks, N, seed=5)
    env.reset()
    obs = _np(env.state).astype(np.int64)
    ql = AnyMDPQLearner(env)
    draws = _draws(np.random.RandomState(1000 * S + A), T, N)
    out = {k: _np(v) for k, v in env.rollout_learner(ql, T, draws=draws).items()}
    host = QLearnerHost(N, S, A)
    idx = np.arange(N)
    live = np.ones(N, bool)

    def learn(o, t):
        term = o["terminated"][t].astype(bool)
        done = term | o["truncated"][t].astype(bool)
        host.learn(obs, o["action"][t], np.where(done, o["final_obs"][t], o["obs"][t]), o["reward"][t].astype(np.float64), term)
        return o["obs"][t].astype(np.int64)

    for t in range(T):
        cdf = policy_cdf(host.q[idx, obs], host.s_visits[idx, obs], host.max_steps)
        u = draws["u_policy"][t]
        a = (cdf <= u[:, None]).sum(-1)                   # QLearnerHost.policy's own expression on the same CDF
        live &= np.abs(cdf[:, :-1] - u[:, None]).min(-1) >= TIE
        bad = np.nonzero((a != out["action"][t]) & live)[0]
        assert len(bad) == 0, (t, bad[:4], a[bad[:4]], out["action"][t][bad[:4]])
        obs = learn(out, t)           # the device's action: the host stays on the device's trajectory in every env
    print("%dx%d: %d of %d envs left out, %d terminated, %d truncated, actions taken: %d" % (
        S, A, int((~live).sum()), N, int(out["terminated"].sum()), int(out["truncated"].sum()), len(np.unique(out["action"]))))
    assert int((~live).sum()) <= MAX_LEFT_OUT
    assert np.array_equal(np.unique(out["action"]), np.arange(A))
    assert out["terminated"].sum() > 0 and out["truncated"].sum() > 0

    def tables_equal():
        q, sa, sv = (_np(x) for x in ql.get_state())
        assert np.array_equal(q[live], host.q[live])
        assert np.array_equal(sa[live], host.sa_visits[live]) and np.array_equal(sv[live], host.s_visits[live])

    tables_equal()
    if greedy_T:
        gd = _draws(np.random.RandomState(7), greedy_T, N)
        gout = {k: _np(v) for k, v in env.rollout_learner(ql, greedy_T, greedy=True, draws=gd).items()}
        for t in range(greedy_T):
            a = host.policy(obs, greedy=True)
            assert np.array_equal(a[live], gout["action"][t][live]), t
            obs = learn(gout, t)
        assert len(np.unique(gout["action"][:, live])) > 1      # the argmax is of trained rows, not of equal ones
        tables_equal()
    assert env.check_errors() == 0
    ql.close()
    env.close()


@pytest.mark.parametrize("S,A", CASES)
def test_device_equals_host_restatement_at_wide_rows(S, A):
    _train_against_host(S, A)


def test_greedy_after_training_at_33_actions():
    """the (8, 33) learner after its training: 32 greedy steps (numpy.argmax: the first maximum of a row of 33)"""
    _train_against_host(8, 33, greedy_T=32)


def test_action_equal_to_A_at_64_actions_sets_the_error_bit():
    """A = 64 is the widest row: actions 0..63 are in range, 64 is not"""
    n = 8
    env = _env([_random_task(6, 64, seed=3)], n, seed=1)
    env.reset()
    env.step(np.full(n, 63, np.int32))
    assert env.check_errors() == 0
    a = np.full(n, 63, np.int32)
    a[5] = 64
    env.step(a)
    assert env.check_errors() & 1                    # action out of range
    env.step(np.zeros(n, np.int32))
    assert env.check_errors() == 0
    env.close()
