"""Model-based agents for AnyMDP: the host restatement of the reference's `AnyMDPSolverMBRL`
(xenoverse/anymdp/anymdp_solver_mbrl.py), vectorised over N independent agents, in fp64 with numpy's order of operations.

It is the CPU oracle of the device learner (csrc/anymdp_mbrl.hip, `AnyMDPMBRLLearner`, `AnyMDPVecEnv.rollout_learner`) and
what the golden fixtures are replayed with.  Per agent (states are observations, MDP tasks only):

    __init__ :13-40          est_r = 0[S, A, S], vis_cnt = 0.01[S, A, S], vis_cnt_sa = 1[S, A], vm = 0[S, A],
                             _c = c / (1 - gamma), then one update_estimator() (-> vm = 0, b = _c 0.01)
    learner :57-71           cnt = vis_cnt[s, a, ns]; est_r[s, a, ns] = (est_r[s, a, ns] cnt + r) / (cnt + 1);
                             vis_cnt[s, a, ns] += 1; vis_cnt_sa[s, a] += 1;
                             terminated: vis_cnt[ns] = 0, est_r[ns] = 0;  terminated or truncated: update_estimator()
    update_estimator :42-55  t = vis_cnt / clip(rowsum(vis_cnt), 0.01); std = max(np.std(est_r), 0.01);
                             b = (_c std) / sqrt(vis_cnt_sa)  (a snapshot: vis_cnt_sa moves on between episode ends);
                             vm = update_value_matrix(t, est_r, gamma, vm, max_iteration=1)
    update_value_matrix      (solver.py:58-82) with max_iteration = 1: ONE in-place Gauss-Seidel sweep, alpha = 1:
                             for s, a: exp_q = 0 + sum_sn t[s, a, sn] (gamma max(vm[sn]) + r[s, a, sn]) left to right;
                             vm[s, a] += exp_q - vm[s, a]   (max(vm[sn]) reads the rows this sweep already moved)
    policy :73-78            greedy: the first argmax of vm[o];  else the first argmax of vm[o] + b[o] u, u = A uniforms

The row sum is numpy's pairwise sum of a length-S row (`pairwise_sum`, learner.py).  np.std of the whole [S, A, S] tensor runs in
buffered chunks of 8192 elements: each chunk is pairwise-summed and the chunks are added in order (`np_tensor_sum`), for
the mean and again for the squared deviations.  Everything is + - * / sqrt max, so the device can be bit-exact.
"""
import numpy as np

from .learner import _DeviceLearner, np_rowsum, pairwise_sum  # noqa: F401

NP_BUFSIZE = 8192    # numpy's default ufunc buffer: the inner-loop length of a whole-array reduction


def np_tensor_sum(x):
    """numpy.sum of each whole x[i] (flattened, contiguous): chunks of NP_BUFSIZE pairwise-summed, added in order"""
    x = x.reshape(x.shape[0], -1)
    n = x.shape[1]
    acc = np.zeros(x.shape[0])
    for c0 in range(0, n, NP_BUFSIZE):
        acc = acc + pairwise_sum(x[:, c0:c0 + NP_BUFSIZE])
    return acc


def np_tensor_std(x):
    """numpy.std of each whole x[i]: mean = sum / n; d = x - mean; sqrt(sum(d * d) / n), both sums np_tensor_sum's"""
    flat = x.reshape(x.shape[0], -1)
    n = flat.shape[1]
    mean = np_tensor_sum(flat) / n
    d = flat - mean[:, None]
    return np.sqrt(np_tensor_sum(d * d) / n)


def gauss_seidel_sweep(t, r, gamma, vm):
    """update_value_matrix(t, r, gamma, vm, max_iteration=1) for each agent: one in-place sweep, alpha = 1.
    t, r: [N, S, A, S]; vm: [N, S, A] (not modified) -> the swept copy"""
    vm = np.array(vm, np.float64)
    n, S, A = vm.shape
    zero = np.zeros((n, 1))
    m = vm.max(-1)                  # max(cur_vm[sn]) of every row as it stands
    for s in range(S):
        for a in range(A):
            terms = t[:, s, a, :] * (gamma * m + r[:, s, a, :])
            exp_q = np.cumsum(np.concatenate([zero, terms], 1), 1)[:, -1]     # 0.0 + terms[0] + ... left to right
            vm[:, s, a] = vm[:, s, a] + 1.0 * (exp_q - vm[:, s, a])
            m[:, s] = vm[:, s].max(-1)
    return vm


class MBRLHost(object):
    """N independent AnyMDPSolverMBRL agents over S observations and A actions (all tables fp64)."""

    def __init__(self, n, S, A, gamma=0.99, c=1.0):
        if S < 1 or A < 2:
            raise ValueError("MBRLHost: need S >= 1 and A >= 2")
        self.n, self.S, self.A = int(n), int(S), int(A)
        self.gamma, self.c = float(gamma), float(c)
        self._c = self.c / (1.0 - self.gamma)
        self.est_r = np.zeros((self.n, self.S, self.A, self.S))
        self.vis_cnt = np.zeros((self.n, self.S, self.A, self.S))
        self.vis_cnt_sa = np.zeros((self.n, self.S, self.A))
        self.vm = np.zeros((self.n, self.S, self.A))
        self.b = np.zeros((self.n, self.S, self.A))
        self.reset()

    def reset(self, mask=None):
        """__init__'s state for the agents where mask (bool[N]) is set (None: all)"""
        m = np.ones(self.n, bool) if mask is None else np.asarray(mask, bool)
        self.est_r[m] = 0.0
        self.vis_cnt[m] = 0.01
        self.vis_cnt_sa[m] = 1.0
        self.vm[m] = 0.0
        self.update_estimator(m)

    def update_estimator(self, mask):
        """update_estimator() of the agents where mask (bool[N]) is set"""
        idx = np.nonzero(np.asarray(mask, bool))[0]
        if len(idx) == 0:
            return
        vc = self.vis_cnt[idx]
        t = vc / np.maximum(np_rowsum(vc), 0.01)[..., None]      # numpy.clip(rowsum, 0.01, None)
        r = self.est_r[idx]
        std = np_tensor_std(r)
        std = np.where(0.01 > std, 0.01, std)                     # python max(std, 0.01)
        self.b[idx] = (self._c * std)[:, None, None] / np.sqrt(self.vis_cnt_sa[idx])
        self.vm[idx] = gauss_seidel_sweep(t, r, self.gamma, self.vm[idx])

    def scores(self, obs, u=None, greedy=False):
        """the row the policy takes the first argmax of: vm[o] (greedy) or vm[o] + b[o] u"""
        i = np.arange(self.n)
        obs = np.asarray(obs, np.int64)
        if greedy:
            return self.vm[i, obs].copy()
        return self.vm[i, obs] + self.b[i, obs] * np.asarray(u, np.float64)

    def policy(self, obs, u=None, greedy=False):
        """actions int64[N] for observations obs[N]; u[N, A]: the policy's uniforms (ignored when greedy)"""
        return self.scores(obs, u, greedy).argmax(-1)

    def learn(self, s, a, ns, r, term, trunc):
        """one learner() call per agent: transition (s, a) -> ns with reward r (fp64), flags term and trunc"""
        i = np.arange(self.n)
        s, a, ns = (np.asarray(x, np.int64) for x in (s, a, ns))
        r = np.asarray(r, np.float64)
        term, trunc = np.asarray(term, bool), np.asarray(trunc, bool)
        cnt = self.vis_cnt[i, s, a, ns]
        self.est_r[i, s, a, ns] = (self.est_r[i, s, a, ns] * cnt + r) / (cnt + 1)
        self.vis_cnt[i, s, a, ns] = cnt + 1
        self.vis_cnt_sa[i, s, a] += 1
        self.vis_cnt[i[term], ns[term]] = 0.0
        self.est_r[i[term], ns[term]] = 0.0
        self.update_estimator(term | trunc)

    def get_state(self):
        """-> (est_r, vis_cnt, vis_cnt_sa, vm, b) copies"""
        return tuple(x.copy() for x in (self.est_r, self.vis_cnt, self.vis_cnt_sa, self.vm, self.b))

    def set_state(self, est_r=None, vis_cnt=None, vis_cnt_sa=None, vm=None, b=None):
        for dst, src in zip((self.est_r, self.vis_cnt, self.vis_cnt_sa, self.vm, self.b), (est_r, vis_cnt, vis_cnt_sa, vm, b)):
            if src is not None:
                dst[...] = src


class AnyMDPMBRLLearner(_DeviceLearner):
    """One AnyMDPSolverMBRL agent per env of an AnyMDPVecEnv, on the device (csrc/anymdp_mbrl.hip): the reference's
    AnyMDPSolverMBRL(env, gamma, c) for every env at once (the reference's train() passes c = 0.05; the class default is 1).
    Drive it with `env.rollout_learner(learner, T)`; there draws["u_policy"] is [T, N, A].

    `est_r`, `vis_cnt` (float64[N, S, A, S]), `vis_cnt_sa`, `vm` and `b` (float64[N, S, A]) are device copies of one table of
    the agent state taken when read; `get_state` copies all five, `set_state` writes any of them.  `b` is the exploration
    bonus the last episode end computed.  The learner lives as long as its env's tasks: `env.set_task` and `env.close` close
    it (any later use raises).  Rows are indexed by observation id, so MDP tasks only; the env must have been set a task, and
    a sub-batch made by split() cannot carry learners (make them on the env it was split from)."""
    _ABI = "xv_anymdp_mbrl"
    _ROLLOUT = "xv_anymdp_rollout_mbrl"
    _TABLES = (("est_r", "float64", "NSAS"), ("vis_cnt", "float64", "NSAS"), ("vis_cnt_sa", "float64", "NSA"),
               ("vm", "float64", "NSA"), ("b", "float64", "NSA"))
    _U_POLICY = "TNA"
    _NOT_MDP = (ValueError, "AnyMDPMBRLLearner: MDP tasks only (the model's states are observation ids)")

    def __init__(self, env, gamma=0.99, c=1.0):
        self._check_env(env)
        if not (0.0 <= gamma < 1.0) or c != c:
            raise ValueError("AnyMDPMBRLLearner: need 0 <= gamma < 1 and a number c")
        self.gamma, self.c = float(gamma), float(c)
        self._create(env, self.gamma, self.c)
