"""What every device learner of AnyMDP (AnyMDPQLearner, AnyMDPMBRLLearner) owes AnyMDPVecEnv.rollout_learner, whatever it
learns: a rollout equals stepping its actions, splitting T changes nothing, refusals come before any launch, and a learner
does not outlive its env's tasks.  What differs between the kinds (sizes, arguments, which tables to look at) is in KINDS;
the learning rules themselves are tested in test_gpu_anymdp_qlearn.py and test_gpu_anymdp_mbrl.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from util import anymdp_env as _env, anymdp_random_task as _random_task, anymdp_tasks16 as _tasks16, to_np as _np
from util import golden_files, load_anymdp_golden, load_anymdp_tok_golden
from xenoverse_amd import _lib
from xenoverse_amd.anymdp import AnyMDPMBRLLearner, AnyMDPQLearner, AnyMDPVecEnv, MBRLHost, QLearnerHost
from xenoverse_amd.anymdp.qlearner import policy_cdf

pytestmark = pytest.mark.gpu


def _q_fresh(ql):
    q, sa, sv = (_np(x) for x in ql.get_state())
    assert np.all(sa == 1) and np.all(sv == 1)


def _q_visits_after_8_steps(ql):
    sv = _np(ql.s_visits)
    assert sv.shape == (8, 16) and int(sv.sum()) == 8 * 16 + 8 * 8      # one visit per env-step on top of the ones
    assert np.array_equal(_np(ql.sa_visits).sum(axis=(1, 2)), 64 + np.full(8, 8))


def _mbrl_fresh(ml):
    assert np.all(_np(ml.vis_cnt_sa) == 1)


def _mbrl_visits_after_8_steps(ml):
    assert np.array_equal(_np(ml.vis_cnt_sa).sum(axis=(1, 2)), np.full(8, 16 * 4 + 8.0))


def _mbrl_too_large():
    """too large N S A S: refused with XV_ERR_NOMEM before anything is allocated"""
    big = AnyMDPVecEnv(1 << 20, seed=1, autoreset_mode="same_step")     # 2^20 x 64 x 8 x 64 x 16 B = 512 GiB of tables
    big.set_task([load_anymdp_golden(golden_files("anymdp_64x8")[0])[1]])
    free = torch.cuda.mem_get_info()[0]
    with pytest.raises(_lib.XenoError) as ex:
        AnyMDPMBRLLearner(big)
    assert ex.value.code == _lib.XV_ERR_NOMEM
    assert abs(torch.cuda.mem_get_info()[0] - free) < (1 << 30)
    big.close()


KINDS = dict(
    q=dict(
        make=AnyMDPQLearner, kw={},                       # kw: the arguments of the two tests with long rollouts
        step_T=96, step_needs_episode_end=False, split_T=128, split_parts=2, split_needs_episode_end=False,
        pomdp_error=AssertionError,       # the reference asserts task_type == "MDP" (anymdp_solver_q.py:17)
        c_create=lambda lib, h, out: lib.xv_anymdp_qlearn_create(h, 0.99, 0.5, 4000, out),
        u_policy=(4, 8), bad_u_policy=(4, 7), fresh=_q_fresh, more_refusals=lambda: None,
        tables=("q", "s_visits"), set_kw=dict(q=np.zeros((8, 16, 4))), visits_after_8_steps=_q_visits_after_8_steps),
    mbrl=dict(
        make=AnyMDPMBRLLearner, kw=dict(c=0.05),
        step_T=160, step_needs_episode_end=True, split_T=240, split_parts=3, split_needs_episode_end=True,
        pomdp_error=ValueError,
        c_create=lambda lib, h, out: lib.xv_anymdp_mbrl_create(h, 0.99, 1.0, out),
        u_policy=(4, 8, 4), bad_u_policy=(4, 8), fresh=_mbrl_fresh, more_refusals=_mbrl_too_large,
        tables=("vm", "est_r"), set_kw=dict(vm=np.zeros((8, 16, 4))), visits_after_8_steps=_mbrl_visits_after_8_steps),
)
kinds = pytest.mark.parametrize("kind", sorted(KINDS))


@kinds
def test_rollout_equals_stepping_its_actions(kind):
    """a twin env with the same seed and tasks stepped through step() with the rollout's actions returns the same outputs"""
    K = KINDS[kind]
    n, T = 256, K["step_T"]
    a_env = _env(_tasks16(), n, seed=9)
    a_env.reset()
    lr = K["make"](a_env, **K["kw"])
    ro = {k: _np(v) for k, v in a_env.rollout_learner(lr, T).items()}
    b_env = _env(_tasks16(), n, seed=9)
    b_env.reset()
    for t in range(T):
        obs, r, term, trunc, info = b_env.step(ro["action"][t])
        assert np.array_equal(_np(obs), ro["obs"][t]), t
        assert np.array_equal(_np(r), ro["reward"][t]) and np.array_equal(_np(info["reward_gt"]), ro["reward_gt"][t])
        assert np.array_equal(_np(term).astype(np.uint8), ro["terminated"][t])
        assert np.array_equal(_np(trunc).astype(np.uint8), ro["truncated"][t])
        done = (ro["terminated"][t] | ro["truncated"][t]).astype(bool)
        assert np.array_equal(_np(info["final_obs"])[done], ro["final_obs"][t][done])
    assert len(np.unique(ro["action"])) == 4
    assert not K["step_needs_episode_end"] or (ro["terminated"] | ro["truncated"]).sum() > 0
    assert a_env.check_errors() == 0 and b_env.check_errors() == 0
    lr.close()
    a_env.close()
    b_env.close()


@kinds
def test_splitting_T_changes_nothing(kind):
    """several calls of T / parts equal one call of T bit for bit (free-running draws), agent state included"""
    K = KINDS[kind]
    n, T = 512, K["split_T"]
    res = []
    for parts in (1, K["split_parts"]):
        env = _env(_tasks16(), n, seed=21)
        env.reset()
        lr = K["make"](env, **K["kw"])
        outs = [env.rollout_learner(lr, T // parts) for _ in range(parts)]
        res.append(({k: np.concatenate([_np(o[k]) for o in outs]) for k in outs[0]}, [_np(x) for x in lr.get_state()]))
        assert env.check_errors() == 0
        lr.close()
        env.close()
    (o1, s1), (o2, s2) = res
    assert not K["split_needs_episode_end"] or (o1["terminated"] | o1["truncated"]).sum() > 0
    for k in o1:
        assert np.array_equal(o1[k], o2[k]), k
    for x, y in zip(s1, s2):
        assert np.array_equal(x, y)


def _q_uniforms(seed, gid, tick, A):
    """anymdp_qlearn.hip: purpose 4 (XV_DRAW_QPOLICY), words 0,1 -> the one uniform numpy.random.choice searches"""
    w = oracle.env_draw(seed, gid, tick, 4)
    return oracle.u53(w[0], w[1])


def _mbrl_uniforms(seed, gid, tick, A):
    """anymdp_mbrl.hip: purpose 7 (XV_DRAW_MBRL_POLICY), sub = a >> 1, words 0,1 (a even) or 2,3 (a odd) -> u[a]; an odd
    A uses only the first word pair of its last draw"""
    u = np.zeros(A)
    for sub in range((A + 1) // 2):
        w = oracle.env_draw_sub(seed, gid, tick, 7, sub)
        u[2 * sub] = oracle.u53(w[0], w[1])
        if 2 * sub + 1 < A:
            u[2 * sub + 1] = oracle.u53(w[2], w[3])
    return u


PHILOX = dict(
    q=dict(make=AnyMDPQLearner, host=lambda n, S, A: QLearnerHost(n, S, A), uniforms=_q_uniforms,
           learn=lambda h, s, a, ns, r, term, trunc: h.learn(s, a, ns, r, term)),
    mbrl=dict(make=AnyMDPMBRLLearner, host=lambda n, S, A: MBRLHost(n, S, A), uniforms=_mbrl_uniforms,
              learn=lambda h, s, a, ns, r, term, trunc: h.learn(s, a, ns, r, term, trunc)))


@pytest.mark.parametrize("kind,A", [("q", 12), ("mbrl", 5), ("mbrl", 12)])
def test_free_running_policy_draws_are_the_documented_philox_draws(kind, A):
    """no injected draws, a nonzero engine seed and env_id_base: the policy's uniforms recomputed on the host from the key
    both kernels document — (engine seed, env_id_base + env, the launch tick of the step that takes the action, purpose,
    [sub]); step t of a rollout is launched with the tick the engine had before the rollout plus t (a learner launch binds
    the tick of the NEXT step launch without advancing it, anymdp_learner.h: xv_learner_bind) — and fed to the host
    restatement along the device's trajectory: every action equal (Q: but for envs from the first step at which the host's
    own margin to a cut of its CDF is below 1e-9, at most 0.1 % of them; the device's exp may differ from numpy's in the
    last bit), the learner tables bit-equal at the end; and two calls of T / 2 equal one call of T bit for bit"""
    K = PHILOX[kind]
    S, n, T, seed, base = 10, 256, 48, 77, 3000
    tasks = [_random_task(S, A, seed=40 + A, max_steps=20, n_terminal=2), _random_task(S, A, seed=41 + A, max_steps=20)]
    res = []
    for parts in (1, 2):
        env = _env(tasks, n, seed=seed, env_id_base=base)
        env.reset()
        obs0 = _np(env.state).astype(np.int64)
        lr = K["make"](env)
        tick0 = env.engine.tick
        outs = [env.rollout_learner(lr, T // parts) for _ in range(parts)]
        assert env.engine.tick == tick0 + T          # one tick per step launch, none for a learner launch
        res.append(({k: np.concatenate([_np(o[k]) for o in outs]) for k in outs[0]}, [_np(x) for x in lr.get_state()]))
        assert env.check_errors() == 0
        lr.close()
        env.close()
    (out, state), (out2, state2) = res
    for k in out:
        assert np.array_equal(out[k], out2[k]), k
    for x, y in zip(state, state2):
        assert np.array_equal(x, y)
    host = K["host"](n, S, A)
    obs, live, idx = obs0, np.ones(n, bool), np.arange(n)
    for t in range(T):
        u = np.array([K["uniforms"](seed, base + i, tick0 + t, A) for i in range(n)])
        if kind == "q":
            cdf = policy_cdf(host.q[idx, obs], host.s_visits[idx, obs], host.max_steps)
            live &= np.abs(cdf[:, :-1] - u[:, None]).min(-1) >= 1e-9
        a = host.policy(obs, u)
        bad = np.nonzero((a != out["action"][t]) & live)[0]
        assert len(bad) == 0, (t, bad[:4], a[bad[:4]], out["action"][t][bad[:4]])
        term, trunc = out["terminated"][t].astype(bool), out["truncated"][t].astype(bool)
        K["learn"](host, obs, out["action"][t], np.where(term | trunc, out["final_obs"][t], out["obs"][t]),
                   out["reward"][t].astype(np.float64), term, trunc)
        obs = out["obs"][t].astype(np.int64)
    assert int((~live).sum()) <= n // 1000
    assert np.array_equal(np.unique(out["action"]), np.arange(A))
    assert out["terminated"].sum() > 0 and out["truncated"].sum() > 0
    for name, x, y in zip(K["make"]._TABLES, state, host.get_state()):
        assert np.array_equal(x[live], y[live]), name[0]


@kinds
def test_refusals_before_any_launch(kind):
    K = KINDS[kind]
    make, tasks = K["make"], _tasks16()
    # POMDP: the learner's states are observation ids; the C-ABI refuses as well
    _, ptask = load_anymdp_tok_golden(golden_files("anymdptok_pomdp")[0])
    penv = AnyMDPVecEnv(4, autoreset_mode="same_step")
    penv.set_task(ptask)
    with pytest.raises(K["pomdp_error"]):
        make(penv)
    h = C.c_void_p()
    assert K["c_create"](penv.lib, penv._h, C.byref(h)) == _lib.XV_ERR_UNSUPPORTED
    assert not h.value
    penv.close()
    # auto-reset modes other than SAME_STEP
    for mode in ("disabled", "next_step"):
        env = _env(tasks, 8, seed=1, mode=mode)
        env.reset()
        lr = make(env)
        with pytest.raises(ValueError):
            env.rollout_learner(lr, 4)
        lr.close()
        env.close()
    env = _env(tasks, 8, seed=1)
    env.reset()
    lr = make(env)
    tick = env.engine.tick
    # wrong shapes, a missing draw, T < 1, another env's learner
    good = dict(u_policy=np.zeros(K["u_policy"]), u=np.zeros((4, 8)), z=np.zeros((4, 8), np.float32),
                u_reset=np.zeros((4, 8)))
    for k in good:
        bad = dict(good)
        bad[k] = np.zeros(K["bad_u_policy"]) if k == "u_policy" else np.zeros((4, 7))
        with pytest.raises(ValueError):
            env.rollout_learner(lr, 4, draws=bad)
        bad.pop(k)
        with pytest.raises(ValueError):
            env.rollout_learner(lr, 4, draws=bad)
    with pytest.raises(ValueError):
        env.rollout_learner(lr, 0)
    other = _env(tasks, 8, seed=1)
    other.reset()
    olr = make(other)
    with pytest.raises(ValueError):
        env.rollout_learner(olr, 4)
    # sub-batches (split) are refused: learners live on the whole env
    subs = env.split(2)
    with pytest.raises(ValueError):
        make(subs[0])
    with pytest.raises(ValueError):
        subs[0].rollout_learner(lr, 4)
    assert env.engine.tick == tick     # nothing was launched
    K["fresh"](lr)
    env._drop_views()
    K["more_refusals"]()
    # a learner of an env that was given new tasks is refused
    env.set_task(tasks)
    env.reset()
    with pytest.raises(ValueError):
        env.rollout_learner(lr, 4)
    assert env.check_errors() == 0 and other.check_errors() == 0
    olr.close()
    lr.close()
    other.close()
    env.close()


@kinds
def test_learner_does_not_outlive_its_env_tasks(kind):
    """set_task (twice: a recycled handle address must not revive the learner) and close release the learner before the
    env's handle goes; every later use raises, a new learner works"""
    K = KINDS[kind]
    tasks = _tasks16()
    env = _env(tasks, 8, seed=2)
    env.reset()
    lr = K["make"](env)
    env.rollout_learner(lr, 4)
    for _ in range(2):
        env.set_task(tasks)
        env.reset()
    uses = (lambda: env.rollout_learner(lr, 4), lr.get_state, lr.reset, lambda: getattr(lr, K["tables"][0]),
            lambda: getattr(lr, K["tables"][1]), lambda: lr.set_state(**K["set_kw"]))
    for use in uses:
        with pytest.raises(ValueError, match="new tasks"):
            use()
    lr2 = K["make"](env)
    out = env.rollout_learner(lr2, 8)
    assert out["action"].shape == (8, 8)
    K["visits_after_8_steps"](lr2)
    assert env.check_errors() == 0
    env.close()
    for use in (lambda: lr2.get_state(), lr2.reset):
        with pytest.raises(ValueError, match="closed"):
            use()
    lr2.close()
