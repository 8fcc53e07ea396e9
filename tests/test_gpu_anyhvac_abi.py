"""The host side of AnyHVAC's C-ABI (csrc/anyhvac.hip below "host side of the C-ABI"): what the seven step entry points
refuse and with which code, the get/set copies of all four buffer groups (env, start, act, pid), and the lifetime of the
lazily allocated groups.  2 envs of the `rot` room (6 coolers), 2 inner iterations per step."""
import ctypes as C

import numpy as np
import pytest
import torch

import anyhvac_util as U
from xenoverse_amd import _lib
from xenoverse_amd.anyhvac import HVACVecEnv
from xenoverse_amd.anyhvac.actions import COST_TABLE
from xenoverse_amd.engine import Engine

pytestmark = pytest.mark.gpu
N = 2
OK, INVALID, UNSUPPORTED = 0, _lib.XV_ERR_INVALID, _lib.XV_ERR_UNSUPPORTED
DISABLED, NEXT_STEP = 0, 1
DIFF = dict(action_mode="diff", discretize_rl_action_space=True, add_action_cost=True)


def _env(engine=None, reset=True, **kw):
    g, task, settings, gen = U.load("rot")
    env = HVACVecEnv(N, autoreset_mode="disabled", engine=engine, **dict(settings, iter_per_step=2, max_steps=16, **kw))
    env.set_task([task], generate_task=gen)
    if reset:
        env.reset_injected(np.repeat(g["init_grid"][None], N, axis=0))
    return env


def _actions(env, k):
    """step k's actions: bins under the diff mode, the recording's box actions otherwise"""
    if env.action_mode == "diff":
        return torch.full((N, env.dims[2]), (3 + 2 * k) % 13, dtype=torch.int32, device=env.device)
    return torch.from_numpy(np.repeat(U.load("rot")[0]["action"][k][None], N, axis=0)).float().to(env.device)


def _all_state(env):
    st = dict(env.get_state())
    if env.action_mode != "box":
        st.update(env.get_act_state())
    if env._pid is not None:
        st.update(env.get_pid_state())
    return {k: v.cpu().numpy() for k, v in st.items()}


def _flat(out):
    obs, r, te, tr, info = out
    d = {"obs." + k: v for k, v in obs.items() if k != "counts"}
    d.update(reward=r, terminated=te, truncated=tr)
    for k, v in info.items():
        if isinstance(v, dict):
            d.update({k + "." + q: w for q, w in v.items() if q != "counts"})
        else:
            d[k] = v
    return {k: v.cpu().numpy() for k, v in d.items()}


def _same(a, b, label):
    assert set(a) == set(b), label
    for k in a:
        assert U.same_bits(a[k], b[k]), label + k


# ---- the refusal table ---------------------------------------------------------------------------------------------------
ENTRIES = ("step", "step_injected", "rollout", "step_mapped", "step_mapped_injected", "rollout_mapped", "rollout_pid")
FAMILY = dict(step="box", step_injected="box", rollout="box", step_mapped="diff", step_mapped_injected="diff",
              rollout_mapped="diff", rollout_pid="box")
# case -> what the entry points of the HANDLE'S OWN family answer (None: the case does not exist for the entry point);
# an entry point of the other family answers XV_ERR_INVALID to every case, the unbuilt autoreset mode included: the
# invalid-argument checks come first
REFUSALS = {
    "null_io":         dict.fromkeys(ENTRIES, INVALID),
    "null_reward":     dict.fromkeys(ENTRIES, INVALID),
    "null_terminated": dict.fromkeys(ENTRIES, INVALID),
    "null_truncated":  dict.fromkeys(ENTRIES, INVALID),
    "null_reset_grid": dict(step=None, step_injected=INVALID, rollout=None, step_mapped=None, step_mapped_injected=INVALID,
                            rollout_mapped=None, rollout_pid=None),
    "T_zero":          dict(step=None, step_injected=None, rollout=INVALID, step_mapped=None, step_mapped_injected=None,
                            rollout_mapped=INVALID, rollout_pid=INVALID),
    "next_step":       dict.fromkeys(ENTRIES, UNSUPPORTED),
    "null_io_and_next_step": dict.fromkeys(ENTRIES, INVALID),
    "valid":           dict.fromkeys(ENTRIES, OK),
}


def _call(env, entry, case):
    """one call of lib.xv_anyhvac_<entry> on the env's handle with the env's own buffers, spoilt as `case` says"""
    T = 0 if case == "T_zero" else 2
    lead = (2,) if entry.startswith("rollout") else ()
    b = env._buffers(lead, False)
    a = idx = None
    if entry != "rollout_pid":
        acts = torch.stack([_actions(env, 0), _actions(env, 1)]) if lead else _actions(env, 0)
        a, idx = (None, acts) if acts.dtype == torch.int32 else (acts, None)
    io = env._io(b, a)
    for k in ("reward", "terminated", "truncated"):
        if case == "null_" + k:
            setattr(io, k, None)
    io_p = None if case.startswith("null_io") else C.byref(io)
    act = _lib.AnyHVACActIO()
    act.action_index = _lib.ptr(idx)
    for k in _lib.AnyHVACActIO.FIELDS[1:]:
        if k in b:
            setattr(act, k, b[k].data_ptr())
    grid = None if case == "null_reset_grid" else env._pad_grid(np.repeat(U.load("rot")[0]["init_grid"][None], N, axis=0))
    mode = NEXT_STEP if case.endswith("next_step") else DISABLED
    out = torch.zeros(lead + (N, env.dims[2]), dtype=torch.float32, device=env.device)
    lib, h = env.lib, env._h
    args = dict(step=(h, io_p, mode), step_injected=(h, io_p, _lib.ptr(grid), mode), rollout=(h, T, io_p, mode),
                step_mapped=(h, io_p, C.byref(act), mode), step_mapped_injected=(h, io_p, C.byref(act), _lib.ptr(grid), mode),
                rollout_mapped=(h, T, io_p, C.byref(act), mode), rollout_pid=(h, T, io_p, _lib.ptr(out), None, mode))[entry]
    rc = getattr(lib, "xv_anyhvac_" + entry)(*args)
    env.engine.sync()
    return rc


@pytest.mark.parametrize("family", ("box", "diff"))
def test_step_entry_points_refuse_with_the_documented_codes_and_touch_nothing(family):
    """every entry point x every case of REFUSALS on a box handle (with a PID set) and on a diff handle: the return code,
    and after a refusal get_state() / get_act_state() / get_pid_state() bit-identical and the engine's tick unmoved"""
    env = _env(**(DIFF if family == "diff" else {}))
    if family == "box":
        env.set_pid()
    for k in range(2):
        env.step(_actions(env, k))
    for entry in ENTRIES:
        for case, row in REFUSALS.items():
            if row[entry] is None:
                continue
            want = row[entry] if FAMILY[entry] == family else INVALID
            before, tick = _all_state(env), env.engine.tick
            rc = _call(env, entry, case)
            assert rc == want, "%s handle, xv_anyhvac_%s, %s: %d (expected %d)" % (family, entry, case, rc, want)
            if want != OK:
                assert env.engine.tick == tick, "%s %s: the tick moved" % (entry, case)
                _same(before, _all_state(env), "%s %s: " % (entry, case))
            else:      # (0 ticks for an injected call, T otherwise)
                assert env.engine.tick - tick == (0 if entry.endswith("injected") else 2 if entry.startswith("rollout") else 1)
    assert env.check_errors() == 0
    env.close()


def test_rollout_pid_needs_a_controller():
    env = _env()
    assert _call(env, "rollout_pid", "valid") == INVALID
    assert _call(env, "rollout_pid", "next_step") == INVALID
    env.close()


# ---- the state round trip ---------------------------------------------------------------------------------------------
# name -> (group, dtype, shape); from HVACVecEnv.get_state / get_act_state / get_pid_state's docstrings
def _listing(env):
    NW, NL, Cc, S = env.dims[:4]
    f64, f32, i32, i16, i64 = np.float64, np.float32, np.int32, np.int16, np.int64
    return {
        "grid": ("env", f64, (N, NW * NL)), "t": ("env", f64, (N,)), "last_call": ("env", f64, (N,)),
        "episode_step": ("env", i32, (N,)), "warning_count": ("env", i32, (N,)), "rest_idx": ("env", i32, (N,)),
        "rest_start": ("env", f64, (N, Cc)), "value": ("env", f32, (N, Cc)), "filter": ("env", f64, (N, Cc)),
        "ring_t": ("env", f64, (N, 256)), "ring_v": ("env", f64, (N, 256, Cc)), "head": ("env", i32, (N, Cc)),
        "tail": ("env", i32, (N,)),
        "last_fail": ("start", f64, (N,)), "history": ("start", i16, (N, 128)), "history_count": ("start", i32, (N,)),
        "window": ("act", i64, (N, Cc)),
        "acc_diff": ("pid", f64, (N, S)), "last_obs": ("pid", f32, (N, S)), "fresh": ("pid", i32, (N,)),
    }


def _round(env, k):
    if env._pid is not None:
        return _flat(env.step(env.pid_action()))
    return _flat(env.step(_actions(env, k)))


@pytest.mark.parametrize("family", ("diff", "box_pid"))
def test_state_of_all_four_groups_round_trips_through_a_second_env(family):
    """3 steps, every entry of every group read, written into a second env that only had set_task, 2 more steps on both:
    every output and every state entry bit-equal; each entry's shape and dtype as listed"""
    kw = DIFF if family == "diff" else {}
    a = _env(**kw)
    a.set_random_start_t(True)      # (the start group records the steps that did not fail)
    if family == "box_pid":
        a.set_pid(kind="loc", kp=0.02)
    for k in range(3):
        _round(a, k)
    groups = dict(env=a.get_state())
    groups["start"] = {k: groups["env"].pop(k) for k in ("last_fail", "history", "history_count")}
    if family == "diff":
        groups["act"] = a.get_act_state()
    else:
        groups["pid"] = a.get_pid_state()
    listing = _listing(a)
    want = {k: v for k, v in listing.items() if v[0] in groups}
    assert {k: grp for grp, d in groups.items() for k in d} == {k: v[0] for k, v in want.items()}
    for grp, d in groups.items():
        for k, v in d.items():
            assert tuple(v.shape) == listing[k][2] and v.cpu().numpy().dtype == listing[k][1], k
    assert int(groups["start"]["history_count"][0]) > 0 and int(groups["env"]["episode_step"][0]) == 3
    if family == "diff":
        assert int(groups["act"]["window"].ne(0).sum()) > 0
    else:
        assert int(groups["pid"]["fresh"].sum()) == 0 and float(groups["pid"]["acc_diff"].abs().sum()) > 0

    b = _env(reset=False, **kw)
    b.set_random_start_t(True)
    b.set_state(**groups["env"], **groups["start"])
    if family == "diff":
        b.set_act_state(**groups["act"])
    else:
        b.set_pid(kind="loc", kp=0.02)
        b.set_pid_state(**groups["pid"])
    b.engine.tick = a.engine.tick
    _same(_all_state(a), _all_state(b), family + " after the write: ")
    for k in range(3, 5):
        _same(_round(a, k), _round(b, k), "%s step %d: " % (family, k + 1))
    _same(_all_state(a), _all_state(b), family + " after two more steps: ")
    assert a.check_errors() == 0 and b.check_errors() == 0
    a.close()
    b.close()


# ---- lifetime ------------------------------------------------------------------------------------------------------------
def test_lazy_groups_allocate_once_clear_when_they_must_and_free_on_every_combination():
    engine = Engine("cuda:0", seed=0)
    table = np.ascontiguousarray(COST_TABLE, np.float64)
    tp = table.ctypes.data_as(C.c_void_p)

    env = _env(engine, **DIFF)      # env + start + act
    for k in range(3):
        env.step(_actions(env, k))
    w = env.get_act_state()["window"].cpu().numpy()
    assert (w != 0).any()
    env.set_too_cold_limit(False)      # the flags alone change: the windows stay
    assert U.same_bits(env.get_act_state()["window"].cpu().numpy(), w)
    _lib.check(env.lib.xv_anyhvac_set_action_mode(env._h, 1, 0, tp))      # discrete: another mode clears them
    assert not env.get_act_state()["window"].cpu().numpy().any()
    _lib.check(env.lib.xv_anyhvac_set_action_mode(env._h, 2, 3, tp))
    assert not env.get_act_state()["window"].cpu().numpy().any()
    env.step(_actions(env, 3))
    env.close()

    env = _env(engine)      # env + start + pid
    env.set_pid()
    for k in range(2):
        env.step(env.pid_action())
    st = env.get_pid_state()
    assert int(st["fresh"].sum()) == 0 and float(st["acc_diff"].abs().sum()) > 0
    env.set_pid(kp=0.01)      # again: the same buffers, a new controller
    st = env.get_pid_state()
    assert int(st["fresh"].sum()) == N and not st["acc_diff"].cpu().numpy().any() and not st["last_obs"].cpu().numpy().any()
    env.rollout_teacher(2)
    env.close()

    env = _env(engine, reset=False)      # env + start alone, never reset
    env.close()
    env = _env(engine, reset=False, **DIFF)      # with the act group, never stepped
    env.close()
    assert engine.error_flags() == 0
    engine.close()
