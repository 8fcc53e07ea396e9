"""Q-learning agents for AnyMDP: the host restatement of the reference's `AnyMDPSolverQ`
(xenoverse/anymdp/anymdp_solver_q.py), vectorised over N independent agents, in fp64 with numpy's order of operations.

It is the CPU oracle of the device learner (csrc/anymdp_qlearn.hip, `AnyMDPQLearner`, `AnyMDPVecEnv.rollout_learner`) and
what the golden fixtures are replayed with.  Per agent (states are observations, MDP tasks only, :17):

    __init__ :8-27   Q = 1 / (1 - gamma), sa_visits = 1, s_visits = 1  (avg_r, avg_r2, r_std, r_cnt are never read: not kept)
    learner  :30-49  lr = sqrt(max((M + 1) / (M + sa_visits[s, a]), 1e-3))          (before the counts move)
                     terminated: Q[ns, :] = 0, target = r;  else target = r + gamma max(Q[ns])   (truncation bootstraps)
                     Q[s, a] += alpha lr (target - Q[s, a]);  sa_visits[s, a] += 1;  s_visits[s] += 1
    policy   :51-59  greedy: the first argmax of Q[state];  else
                     v = Q[state] - max;  k = min((M + s_visits[state]) / (M + 1), 10);  v = v / max(std(v), 1e-2) * k
                     p = exp(v) / sum(exp(v));  numpy.random.choice(A, p=p) = #{cumsum(p) / cumsum(p)[-1] <= u}

with M the learner's own max_steps (4000), not the env's.  Sums, means and the population std follow numpy's pairwise
summation of a length-A row (`np_sum`, learner.py): a plain loop below 8 elements, eight partial sums from 8 up (A <= 64 < 128).
"""
import numpy as np

from .learner import _DeviceLearner, np_rowsum as np_sum  # noqa: F401  (np_sum: numpy's sum of each row of x[..., n])

A_MAX = 64   # the widest row the device learner takes (xv_anymdp_create: A <= 64)


def policy_cdf(q_rows, s_visits, max_steps):
    """the normalised CDF numpy.random.choice searches, for rows q_rows[N, A] with visit counts s_visits[N]"""
    q_rows = np.asarray(q_rows, np.float64)
    A = q_rows.shape[-1]
    v = q_rows - q_rows.max(-1, keepdims=True)
    k = np.minimum((max_steps + np.asarray(s_visits, np.float64)) / (max_steps + 1), 10.0)
    mean = np_sum(v) / A
    d = v - mean[..., None]
    std = np.sqrt(np_sum(d * d) / A)
    v = v / np.maximum(std, 1.0e-2)[..., None] * k[..., None]
    e = np.exp(v)
    p = e / np_sum(e)[..., None]
    cdf = np.cumsum(p, -1)      # numpy.cumsum: one sequential pass
    return cdf / cdf[..., -1:]


class QLearnerHost(object):
    """N independent AnyMDPSolverQ agents over S observations and A actions (fp64 tables, counts as integers)."""

    def __init__(self, n, S, A, gamma=0.99, alpha=0.5, max_steps=4000):
        if not (2 <= A <= A_MAX) or S < 1:
            raise ValueError("QLearnerHost: need S >= 1 and 2 <= A <= %d" % A_MAX)
        self.n, self.S, self.A = int(n), int(S), int(A)
        self.gamma, self.alpha, self.max_steps = float(gamma), float(alpha), int(max_steps)
        self.q = np.zeros((self.n, self.S, self.A))
        self.sa_visits = np.zeros((self.n, self.S, self.A), np.int64)
        self.s_visits = np.zeros((self.n, self.S), np.int64)
        self.reset()

    def reset(self, mask=None):
        m = np.ones(self.n, bool) if mask is None else np.asarray(mask, bool)
        self.q[m] = 1.0 / (1.0 - self.gamma)
        self.sa_visits[m] = 1
        self.s_visits[m] = 1

    def policy(self, obs, u=None, greedy=False):
        """actions int64[N] for observations obs[N]; u[N]: the uniform numpy.random.choice draws (ignored when greedy)"""
        idx = np.arange(self.n)
        obs = np.asarray(obs, np.int64)
        rows = self.q[idx, obs]
        if greedy:
            return rows.argmax(-1)      # the first maximum
        cdf = policy_cdf(rows, self.s_visits[idx, obs], self.max_steps)
        return (cdf <= np.asarray(u, np.float64)[:, None]).sum(-1).astype(np.int64)   # searchsorted(cdf, u, 'right')

    def learn(self, s, a, ns, r, term, trunc=None):
        """one learner() call per agent: transition (s, a) -> ns with reward r (fp64), terminated flags `term`.
        Truncation takes the bootstrapped path, so `trunc` does not enter."""
        idx = np.arange(self.n)
        s, a, ns = (np.asarray(x, np.int64) for x in (s, a, ns))
        r = np.asarray(r, np.float64)
        term = np.asarray(term, bool)
        M = self.max_steps
        lr = np.sqrt(np.maximum((M + 1) / (M + self.sa_visits[idx, s, a].astype(np.float64)), 1.0e-3))
        self.q[idx[term], ns[term]] = 0.0
        target = np.where(term, r, r + self.gamma * self.q[idx, ns].max(-1))
        err = target - self.q[idx, s, a]
        self.q[idx, s, a] = self.q[idx, s, a] + self.alpha * lr * err
        self.sa_visits[idx, s, a] += 1
        self.s_visits[idx, s] += 1

    def get_state(self):
        return self.q.copy(), self.sa_visits.copy(), self.s_visits.copy()

    def set_state(self, q, sa_visits, s_visits):
        self.q[...] = q
        self.sa_visits[...] = sa_visits
        self.s_visits[...] = s_visits


class AnyMDPQLearner(_DeviceLearner):
    """One AnyMDPSolverQ agent per env of an AnyMDPVecEnv, on the device (csrc/anymdp_qlearn.hip): the reference's
    AnyMDPSolverQ(env, gamma, alpha, max_steps) for every env at once.  Drive it with `env.rollout_learner(learner, T)`.

    `q` (float64[N, S, A]), `sa_visits` (int32[N, S, A]) and `s_visits` (int32[N, S]) are device copies of one table of the
    agent state taken when read; `get_state` copies all three, `set_state` writes them; `reset` restores __init__'s state
    (Q = 1 / (1 - gamma), counts 1).  The learner lives as long as its env's tasks: `env.set_task` and `env.close` close it
    (any later use raises).  Rows are indexed by observation id.  MDP tasks only (the reference asserts task_type == "MDP");
    the env must have been set a task, and a sub-batch made by split() cannot carry learners (make them on the env it was
    split from)."""
    _ABI = "xv_anymdp_qlearn"
    _ROLLOUT = "xv_anymdp_rollout_qlearn"
    _TABLES = (("q", "float64", "NSA"), ("sa_visits", "int32", "NSA"), ("s_visits", "int32", "NS"))
    _NOT_MDP = (AssertionError, "The solver only works for MDP")       # anymdp_solver_q.py:17

    def __init__(self, env, gamma=0.99, alpha=0.5, max_steps=4000):
        self._check_env(env)
        if not (0.0 <= gamma < 1.0) or int(max_steps) < 0:
            raise ValueError("AnyMDPQLearner: need 0 <= gamma < 1 and max_steps >= 0")
        self.gamma, self.alpha, self.max_steps = float(gamma), float(alpha), int(max_steps)
        self._create(env, self.gamma, self.alpha, self.max_steps)
