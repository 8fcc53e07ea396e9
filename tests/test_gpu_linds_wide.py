"""GPU parity of the LinDS kernels at the wide pads.  xv_linds_create takes NS in {16, 32}, NA in {8, 16}, NO in {16, 32}
and csrc/linds.hip instantiates every step / roll-out / reset / table kernel for the eight combinations
(key = 4 [NS = 32] + 2 [NA = 16] + 1 [NO = 32]); the other LinDS tests reach keys 0 and 4 only.  Here:

  * the reference's own trajectories at pad 16 / 32 (tests/golden/lindswide_*.npz, 1e-5 relative per step from the
    reference's state) pin keys 3 and 7 on both step paths;
  * the CPU oracle, pinned to the same fixtures by test_oracle_linds_wide.py, pins all eight keys (state and
    observation bit for bit), with tasks cut from the two fixtures to fewer actions / observations;
  * the scalar and the MFMA path, the command table and the direct Fourier evaluation, the fused roll-out, step_many and
    single steps pin each other bit for bit at the wide keys.
"""
import numpy as np
import pytest
import torch

import oracle
from xenoverse_amd.linds import LinDSVecEnv, build_tables, pad_tables
from util import FourierCommand, close_rel, golden_files, load_linds_golden
from test_oracle_linds import _before_states

pytestmark = pytest.mark.gpu
FILES = golden_files("lindswide_")           # [16x12x24 (zero-padded), 32x16x32 (every row and column live)]
MODES = {"disabled": 0, "next_step": 1, "same_step": 2}
KEYS = [(ns, na, no) for ns in (16, 32) for na in (8, 16) for no in (16, 32)]      # KEYS[key] = (NS, NA, NO)
KEY_IDS = ["key%d_%dx%dx%d" % ((k,) + KEYS[k]) for k in range(8)]
WIDE = dict(pad_action_dim=16, pad_observation_dim=32, pad_command_dim=32)


def _np(t):
    return t.detach().cpu().numpy()


def _pads(key):
    NS, NA, NO = KEYS[key]
    return dict(pad_action_dim=NA, pad_observation_dim=NO, pad_command_dim=NO)


def _cut(task, na, no, max_steps):
    """the task with its first `na` actions and first `no` observations only"""
    c = task["command"]
    t = dict(task, action_dim=na, observation_dim=no, max_steps=max_steps, ld_B=task["ld_B"][:, :na],
             ld_C=task["ld_C"][:no], ld_Y=task["ld_Y"][:no], target_valid=task["target_valid"][:no])
    t["command"] = FourierCommand([o for o, _ in c.coeffs], [f[:no] for _, f in c.coeffs], c.max_steps)
    return t


def _key_tasks(key, max_steps=(37, 23, 29, 17)):
    """four tasks that make xv_linds_create choose `key`: the first fills the pads as far as its fixture allows, the
    others are odd cuts; at NS = 32 the 16-state fixture rides along zero-padded"""
    NS, NA, NO = KEYS[key]
    w16, w32 = (load_linds_golden(p)[1] for p in FILES)
    if NS == 16:
        src = [w16] * 4
        nas = {8: (8, 5, 7, 8), 16: (12, 9, 11, 10)}[NA]
        nos = {16: (16, 11, 13, 15), 32: (24, 17, 21, 23)}[NO]
    else:
        src = [w32, w16, w32, w16]
        nas = {8: (8, 7, 6, 8), 16: (16, 12, 13, 9)}[NA]
        nos = {16: (16, 13, 11, 16), 32: (32, 24, 29, 19)}[NO]
    return [_cut(s, a, o, m) for s, a, o, m in zip(src, nas, nos, max_steps)]


def _key_batch(key, layout, seed=3, **kw):
    tasks = _key_tasks(key, **kw)
    tab = pad_tables(build_tables(tasks, **_pads(key)))
    assert (tab["NS"], tab["NA"], tab["NO"]) == KEYS[key]
    rng = np.random.RandomState(seed)
    if layout == "grouped64":
        env_task = np.repeat(np.arange(4, dtype=np.int32), 64)
    elif layout == "odd_counts":       # padded tiles in the slot layout, lanes of one wave on different tasks
        env_task = np.array([0] * 1 + [1] * 33 + [2] * 64 + [3] * 7, np.int32)
        rng.shuffle(env_task)
    elif layout == "scattered":
        env_task = rng.randint(0, 4, 250).astype(np.int32)
    return tasks, tab, env_task, rng


def _env(key, tasks, env_task, mode, path=None, **kw):
    env = LinDSVecEnv(len(env_task), autoreset_mode=mode, **_pads(key), **kw)
    env.set_task(tasks, env_task_index=env_task)
    assert (env.NS, env.NA, env.NO) == KEYS[key]          # the kernels of this key run
    if path is not None:
        env.set_path(path)
    return env


# -- a. the reference's trajectories at the wide pads ---------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["mfma", "scalar"])
@pytest.mark.parametrize("path", FILES, ids=["key3_16x12x24", "key7_32x16x32"])
def test_golden_every_step_from_reference_state(path, kernel):
    g, task = load_linds_golden(path)
    T, ns = g["tr_x"].shape
    xb, sb = _before_states(g)
    env = LinDSVecEnv(T, autoreset_mode="disabled", **WIDE)
    env.set_task(task)
    env.set_path(kernel)
    assert (env.NS, env.NA, env.NO) == (KEYS[3] if ns == 16 else KEYS[7])
    env.set_state(x=xb.T.astype(np.float32), steps=sb, need_reset=np.zeros(T))
    obs, r, term, trunc, info = env.step_injected(g["tr_action"], g["tr_z"].T, np.zeros(T))
    x, st, _ = env.get_state()
    assert np.array_equal(_np(term).astype(np.uint8), g["tr_term"])
    assert np.array_equal(_np(trunc).astype(np.uint8), g["tr_trunc"])
    assert np.array_equal(_np(st), g["tr_steps"])
    assert close_rel(_np(x)[:ns].T, g["tr_x"])
    assert _np(obs).shape == g["tr_obs"].shape == (T, 32)
    assert close_rel(_np(obs), g["tr_obs"])
    assert close_rel(_np(info["command"]), g["tr_cmd"])
    assert close_rel(_np(info["error"]), g["tr_error"])
    assert close_rel(_np(r), g["tr_reward"])
    assert env.check_errors() == 0
    env.close()


@pytest.mark.parametrize("path", FILES, ids=["key3_16x12x24", "key7_32x16x32"])
def test_golden_reset(path):
    g, task = load_linds_golden(path)
    done = np.nonzero(g["tr_term"] | g["tr_trunc"])[0]
    idx = np.concatenate([[int(g["init_idx"])], g["tr_reset_idx"][done]]).astype(np.int32)
    env = LinDSVecEnv(len(idx), autoreset_mode="disabled", **WIDE)
    env.set_task(task)
    obs, info = env.reset_injected(idx)
    assert _np(obs).shape == (len(idx), 32)
    assert close_rel(_np(obs), np.concatenate([g["init_obs"][None], g["tr_reset_obs"][done]]))
    assert close_rel(_np(info["command"]), np.concatenate([g["init_cmd"][None], g["tr_reset_cmd"][done]]))
    assert close_rel(_np(info["error"]), np.concatenate([[float(g["init_err"])], g["tr_reset_err"][done]]))
    env.close()


# -- b. all eight keys against the oracle, injected draws -----------------------------------------------------------------
def _cmp(dev, ora, exact_state=True):
    obs, r, term, trunc, info = dev
    assert np.array_equal(_np(term).astype(np.uint8), ora["terminated"])
    assert np.array_equal(_np(trunc).astype(np.uint8), ora["truncated"])
    no = _np(obs).shape[1]
    if exact_state:
        assert np.array_equal(_np(obs), ora["obs"][:, :no])
    else:
        assert close_rel(_np(obs), ora["obs"][:, :no])
    assert close_rel(_np(info["command"]), ora["cmd"][:, :no], 1e-5, 2e-6)
    assert close_rel(_np(info["error"]), ora["error"], 1e-5, 2e-6)
    assert close_rel(_np(r), ora["reward"], 1e-5, 2e-6)


_B_CASES = [(key, mode) for key in range(8) for mode in (("disabled", "next_step", "same_step") if key in (3, 7)
                                                          else ("same_step",))]


@pytest.mark.parametrize("path", ["mfma", "scalar"])
@pytest.mark.parametrize("layout", ["grouped64", "odd_counts"])
@pytest.mark.parametrize("key,mode", _B_CASES, ids=["%s-%s" % (KEY_IDS[k], m) for k, m in _B_CASES])
def test_batch_injected_vs_oracle(key, mode, layout, path):
    NS, NA, NO = KEYS[key]
    tasks, tab, env_task, rng = _key_batch(key, layout)
    n = len(env_task)
    env = _env(key, tasks, env_task, mode, path)
    ora = oracle.LinDSOracle(tab, env_task)
    n_init = tab["ints"][env_task, 2]
    idx0 = (rng.random_sample(n) * n_init).astype(np.int32)
    obs, info = env.reset_injected(idx0)
    o0 = ora.reset_injected(idx0)
    assert _np(obs).shape == (n, NO) and np.array_equal(_np(obs), o0["obs"])
    assert close_rel(_np(info["command"]), o0["cmd"], 1e-5, 2e-6) and close_rel(_np(info["error"]), o0["error"], 1e-5, 2e-6)
    ended = 0
    for t in range(60):
        a = rng.uniform(-1.4, 1.4, (n, NA)).astype(np.float32)
        z = rng.standard_normal((NS, n)).astype(np.float32)
        idx = (rng.random_sample(n) * n_init).astype(np.int32)
        d = env.step_injected(a, z, idx)
        o = ora.step_injected(a, z, idx, MODES[mode])
        _cmp(d, o)
        x, st, nr = env.get_state()
        assert np.array_equal(_np(x), ora.x) and np.array_equal(_np(st), ora.steps)
        assert np.array_equal(_np(nr), ora.need_reset)
        done = (o["terminated"] | o["truncated"]).astype(bool)
        ended += int(done.sum())
        if mode == "same_step":
            fo = _np(d[4]["final_obs"])
            assert fo.shape == (n, NO) and np.array_equal(fo[done], o["final_obs"][done])
        if mode == "disabled" and done.any():
            env.reset_injected(idx, mask=done.astype(np.uint8))
            ora.reset_injected(idx, mask=done.astype(np.uint8))
    assert ended > 20
    assert env.check_errors() == 0
    env.close()


# -- c. the two step paths, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("key", range(8), ids=KEY_IDS)
def test_mfma_equals_scalar_on_every_output(key):
    """include/xeno.h, xv_linds_set_path: "results are identical" — on obs, reward, the flags, command, error, final_obs,
    steps, the done mask and the state, free-running (the other tests of the scalar kernel inject their draws: another
    instantiation), in waves that hold several tasks.  Key 7 is what the issue asks for; the scalar kernel's waterfall
    lost the command rows of lanes that had left it there (csrc/linds.hip, linds_step_kernel), and every key has the same
    loop, so every key is checked."""
    NS, NA, NO = KEYS[key]
    tasks, tab, env_task, rng = _key_batch(key, "odd_counts", seed=21)
    n = len(env_task)
    acts = rng.uniform(-1.3, 1.3, (60, n, NA)).astype(np.float32)
    recs = []
    for path in ("mfma", "scalar"):
        env = _env(key, tasks, env_task, "same_step", path, seed=5)
        obs, info = env.reset()
        rec, ended = [_np(obs), _np(info["command"]), _np(info["error"])], 0
        for t in range(60):
            o, r, te, tr, info = env.step(acts[t])
            done = _np(te) | _np(tr)
            x, st, nr = env.get_state()
            rec += [_np(o), _np(r), _np(te), _np(tr), _np(info["command"]), _np(info["error"]), _np(info["steps"]),
                    _np(info["_final_obs"]), _np(info["final_obs"])[done], _np(x), _np(st), _np(nr)]
            ended += int(done.sum())
        assert ended > 20 and env.check_errors() == 0
        recs.append(rec)
        env.close()
    assert len(recs[0]) == len(recs[1])
    for i, (a, b) in enumerate(zip(*recs)):
        assert np.array_equal(a, b), i


# -- d. command table on and off, past the table's end --------------------------------------------------------------------
@pytest.mark.parametrize("path", ["mfma", "scalar"])
@pytest.mark.parametrize("key", [1, 3, 7], ids=[KEY_IDS[k] for k in (1, 3, 7)])
def test_command_table_equals_direct_evaluation(key, path):
    """as test_gpu_linds.py's: auto-reset disabled, 70 steps with max_steps <= 40 (the last 30 run outside the command
    table, the branch the note above xv_mfma_settle is about), a masked reset at step 20.  The MFMA records' observations
    equal the oracle's bit for bit, the second tile (components 16..31) included."""
    NS, NA, NO = KEYS[key]
    tasks, tab, env_task, rng = _key_batch(key, "grouped64", seed=8, max_steps=(40, 33, 37, 29))
    n = len(env_task)
    acts = rng.uniform(-0.3, 0.3, (70, n, NA)).astype(np.float32)
    zs = rng.standard_normal((70, NS, n)).astype(np.float32)
    n_init = tab["ints"][env_task, 2]
    idxs = (rng.random_sample((70, n)) * n_init).astype(np.int32)
    m = np.zeros(n, np.uint8); m[::3] = 1
    ora = oracle.LinDSOracle(tab, env_task)
    ora_obs = [ora.reset_injected(idxs[0])["obs"]]
    for t in range(70):
        ora_obs.append(ora.step_injected(acts[t], zs[t], idxs[t], 0)["obs"])
        if t == 20:
            ora.reset_injected(idxs[t], mask=m)
    outs = []
    for table in (True, False):
        env = _env(key, tasks, env_task, "disabled", path)
        env.set_command_table(table)
        obs, info = env.reset_injected(idxs[0])
        rec, dev_obs = [_np(obs), _np(info["command"])], [_np(obs)]
        for t in range(70):
            o, r, te, tr, info = env.step_injected(acts[t], zs[t], idxs[t])
            rec += [_np(o), _np(r), _np(info["command"]), _np(info["error"]), _np(te), _np(tr)]
            dev_obs.append(_np(o))
            if t == 20:
                env.reset_injected(idxs[t], mask=m)
        assert int(_np(env.get_state()[1]).max()) > 45
        assert env.check_errors() == 0
        if path == "mfma":
            for t, (a, b) in enumerate(zip(dev_obs, ora_obs)):
                assert a.shape == (n, NO)
                assert np.array_equal(a[:, 16:], b[:, 16:]) and np.array_equal(a, b), (table, t)
        outs.append(rec)
        env.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


# -- e. fused roll-out and step_many equal single steps -------------------------------------------------------------------
def _rows(o, r, te, tr, info):
    return dict(obs=_np(o), reward=_np(r), terminated=_np(te).astype(np.uint8), truncated=_np(tr).astype(np.uint8),
                command=_np(info["command"]), error=_np(info["error"]), final_obs=_np(info["final_obs"]))


@pytest.mark.parametrize("layout", ["grouped64", "scattered"])
@pytest.mark.parametrize("key", [3, 7], ids=[KEY_IDS[k] for k in (3, 7)])
def test_fused_rollout_equals_single_steps(key, layout):
    NS, NA, NO = KEYS[key]
    tasks, tab, env_task, rng = _key_batch(key, layout, seed=2, max_steps=(23, 23, 19, 23))
    n, T = len(env_task), 70
    acts = np.random.RandomState(3).uniform(-1.3, 1.3, (T, n, NA)).astype(np.float32)
    recs = []
    for fused in (False, True):
        env = _env(key, tasks, env_task, "same_step", seed=77, env_id_base=123)
        env.reset()
        if fused:
            a = env.rollout(acts[:30])
            b = env.rollout(acts[30:])          # a second launch continues where the first stopped
            rec = {k: np.concatenate([_np(a[k]), _np(b[k])]) for k in a}
        else:
            rows = [_rows(*env.step(acts[t])) for t in range(T)]
            rec = {k: np.stack([row[k] for row in rows]) for k in rows[0]}
        x, st, nr = env.get_state()
        rec.update(x=_np(x), steps=_np(st), tick=np.int64(env.engine.tick))
        assert env.check_errors() == 0
        recs.append(rec)
        env.close()
    assert recs[0]["truncated"].sum() > 0 and recs[0]["obs"].shape == (T, n, NO)
    assert set(recs[0]) == set(recs[1])
    for k in recs[0]:
        assert np.array_equal(recs[0][k], recs[1][k]), k


@pytest.mark.parametrize("layout", ["grouped64", "scattered"])
@pytest.mark.parametrize("key", [3, 7], ids=[KEY_IDS[k] for k in (3, 7)])
def test_step_many_equals_single_steps(key, layout):
    NS, NA, NO = KEYS[key]
    tasks, tab, env_task, rng = _key_batch(key, layout, seed=4, max_steps=(23, 17, 19, 13))
    n, P, K = len(env_task), 8, 21
    acts = np.random.RandomState(11).uniform(-1.2, 1.2, (P, n, NA)).astype(np.float32)
    extra = np.random.RandomState(12).uniform(-1, 1, (n, NA)).astype(np.float32)
    recs = []
    for many in (False, True):
        env = _env(key, tasks, env_task, "same_step", seed=5, env_id_base=64)
        env.reset()
        if many:
            ring = env.step_many(K, acts)                 # 2 ring cycles + 5 steps
            env.step(extra)                               # an ordinary step in between moves the engine tick
            ring = env.step_many(2 * P, acts, out=ring)   # the same ring buffers again
            rec = {k: _np(v) for k, v in ring.items()}
        else:
            rows = [None] * P
            seq = [acts[k % P] for k in range(K)] + [extra] + [acts[k % P] for k in range(2 * P)]
            for q, a in enumerate(seq):
                row = _rows(*env.step(a))
                if q == K:
                    continue
                k = q if q < K else q - K - 1
                rows[k % P] = row
            rec = {k: np.stack([row[k] for row in rows]) for k in rows[0]}
        x, st, nr = env.get_state()
        rec.update(x=_np(x), steps=_np(st), tick=np.int64(env.engine.tick))
        assert env.check_errors() == 0
        recs.append(rec)
        env.close()
    done = (recs[0]["terminated"] | recs[0]["truncated"]).astype(bool)
    assert done.sum() > 0 and recs[0]["obs"].shape == (P, n, NO)
    assert set(recs[0]) == set(recs[1])
    for k in recs[0]:
        a, b = recs[0][k], recs[1][k]
        if k == "final_obs":            # the ring's rows are written by finished envs only (earlier cycles may linger)
            a, b = a[done], b[done]
        assert np.array_equal(a, b), k


# -- f. state accessors ---------------------------------------------------------------------------------------------------
def test_state_accessors_under_the_slot_layout():
    tasks, tab, env_task, rng = _key_batch(7, "odd_counts", seed=12)
    n = len(env_task)
    env = _env(7, tasks, env_task, "disabled")
    ora = oracle.LinDSOracle(tab, env_task)
    idx = np.zeros(n, np.int32)
    env.reset_injected(idx); ora.reset_injected(idx)
    x0 = rng.uniform(-0.2, 0.2, (32, n)).astype(np.float32)
    st0 = rng.randint(0, 12, n).astype(np.int32)
    env.set_state(x=x0, steps=st0, need_reset=np.zeros(n, np.uint8))
    ora.x[:] = x0; ora.steps[:] = st0; ora.need_reset[:] = 0
    x, st, nr = env.get_state()
    assert np.array_equal(_np(x), x0) and np.array_equal(_np(st), st0) and not _np(nr).any()
    assert np.array_equal(_np(env.state), x0.T)
    for path in ("mfma", "scalar"):
        env.set_path(path)
        a = rng.uniform(-1, 1, (n, 16)).astype(np.float32)
        z = rng.standard_normal((32, n)).astype(np.float32)
        _cmp(env.step_injected(a, z, idx), ora.step_injected(a, z, idx, 0))
        x, st, nr = env.get_state()
        assert np.array_equal(_np(x), ora.x) and np.array_equal(_np(st), ora.steps)
    env.close()


# -- g. free-running draws ------------------------------------------------------------------------------------------------
def test_free_running_philox_vs_oracle():
    tasks, tab, env_task, rng = _key_batch(7, "grouped64", seed=5)
    n = len(env_task)
    seed, base = 987654321, 5000
    env = _env(7, tasks, env_task, "same_step", seed=seed, env_id_base=base)
    ora = oracle.LinDSOracle(tab, env_task)
    tick = env.engine.tick
    obs, info = env.reset()
    o0 = ora.reset(seed, base, tick)
    assert np.array_equal(_np(obs), o0["obs"])
    ended = 0
    for t in range(60):
        a = rng.uniform(-1.2, 1.2, (n, 16)).astype(np.float32)
        tick = env.engine.tick
        d = env.step(a)
        o = ora.step(seed, base, tick, a, 2)
        _cmp(d, o, exact_state=False)      # Box-Muller: device logf/sincospif vs host double -> 1e-5
        x, st, _ = env.get_state()
        assert close_rel(_np(x), ora.x, 1e-5, 2e-6) and np.array_equal(_np(st), ora.steps)
        ora.x[:] = _np(x)                  # re-sync so tolerance does not compound over the trajectory
        ended += int((o["terminated"] | o["truncated"]).sum())
    assert ended > 20
    env.close()


# -- h. a user width between the compiled ones ----------------------------------------------------------------------------
def test_partial_user_width():
    """pads 12 / 24: the kernels of key 3 run, the caller sees 24 columns and gives 12"""
    g, task = load_linds_golden(FILES[0])
    task["max_steps"] = 9
    pads = dict(pad_action_dim=12, pad_observation_dim=24, pad_command_dim=24)
    tab = pad_tables(build_tables([task], **pads))
    n = 70
    env = LinDSVecEnv(n, autoreset_mode="same_step", **pads)
    env.set_task(task)
    assert (env.NS, env.NA, env.NO) == KEYS[3] and env.user_dims == (12, 24)
    assert env.single_observation_space.shape == (24,) and env.single_action_space.shape == (12,)
    ora = oracle.LinDSOracle(tab, np.zeros(n, np.int32))
    rng = np.random.RandomState(6)
    idx = rng.randint(0, 3, n).astype(np.int32)
    obs, info = env.reset_injected(idx)
    o0 = ora.reset_injected(idx)
    assert _np(obs).shape == (n, 24) and _np(info["command"]).shape == (n, 24)
    assert np.array_equal(_np(obs), o0["obs"][:, :24])
    with pytest.raises(AssertionError, match="Action shape mismatch"):
        env.step(np.zeros((n, 16), np.float32))
    ended = 0
    for path in ("mfma", "scalar"):
        env.set_path(path)
        for t in range(10):
            a = rng.uniform(-1.4, 1.4, (n, 12)).astype(np.float32)
            z = rng.standard_normal((16, n)).astype(np.float32)
            idx = rng.randint(0, 3, n).astype(np.int32)
            d = env.step_injected(a, z, idx)
            a16 = np.zeros((n, 16), np.float32); a16[:, :12] = a
            o = ora.step_injected(a16, z, idx, 2)
            _cmp(d, o)
            fo = _np(d[4]["final_obs"])
            done = (o["terminated"] | o["truncated"]).astype(bool)
            assert _np(d[0]).shape == (n, 24) and _np(d[4]["command"]).shape == (n, 24) and fo.shape == (n, 24)
            assert np.array_equal(fo[done], o["final_obs"][done][:, :24])
            assert not o["obs"][:, 24:].any() and not o["cmd"][:, 24:].any()
            ended += int(done.sum())
    assert ended > 20
    o, r, te, tr, info = env.step(np.zeros((n, 12), np.float32))
    assert _np(o).shape == (n, 24)
    env.close()


# -- i. device-made tasks at the wide pads --------------------------------------------------------------------------------
def test_device_tasks_step_like_the_same_tasks_from_the_host():
    """sample_tasks_device at (16, 12, 24) writes NA = 16 / NO = 32 tables; the same tasks through task dicts and the host
    table builder step the same"""
    from xenoverse_amd.engine import Engine
    from xenoverse_amd.linds import sample_tasks_device, task_dicts_from_device
    eng = Engine("cuda:0")
    out = sample_tasks_device(8, 16, 12, 24, seed=1224, max_draws=4096, batch=64, engine=eng, dense=True)
    assert (out["NS"], out["NA"], out["NO"]) == KEYS[3] and out["phiT"].shape == (8, 16, 16)
    assert out["gamT"].shape == (8, 16, 16) and out["cT"].shape == (8, 16, 32)
    assert np.all(out["info"]["na"] == 12) and np.all(out["info"]["no"] == 24)
    tasks = task_dicts_from_device(out)
    ref = build_tables(tasks, dt=0.1, pad_observation_dim=out["NO"], pad_action_dim=out["NA"], pad_command_dim=out["NO"])
    n = 16 * 8
    env_d = LinDSVecEnv(n, seed=5, engine=eng, **WIDE)
    env_h = LinDSVecEnv(n, seed=5, engine=eng, **WIDE)
    env_d.set_task(out)
    env_h.set_task(ref)
    assert (env_d.NS, env_d.NA, env_d.NO) == (env_h.NS, env_h.NA, env_h.NO) == KEYS[3]
    rng = np.random.RandomState(3)
    idx = np.zeros(n, np.int32)
    od, fd = env_d.reset_injected(idx)
    oh, fh = env_h.reset_injected(idx)
    assert torch.equal(od, oh) and torch.equal(fd["command"], fh["command"]) and torch.equal(fd["error"], fh["error"])
    for _ in range(20):
        a = rng.uniform(-1, 1, (n, 16)).astype(np.float32)
        z = rng.randn(16, n).astype(np.float32)
        d, h = env_d.step_injected(a, z, idx), env_h.step_injected(a, z, idx)
        for k, (x, y) in enumerate(zip(d[:4], h[:4])):
            assert torch.equal(x, y), k
        for k in ("command", "error", "final_obs", "steps"):
            assert torch.equal(d[4][k], h[4][k]), k
        assert torch.isfinite(d[0]).all()
    xd, sd, _ = env_d.get_state()
    xh, sh, _ = env_h.get_state()
    assert torch.equal(xd, xh) and torch.equal(sd, sh)
    env_d.close()
    env_h.close()
    eng.close()


# -- j. the MPC teacher at pad_action_dim = 16 ----------------------------------------------------------------------------
def test_mpc_action_matches_host_solve():
    """test_gpu_linds_mpc.py's comparison with the host's exact optimum, on the 16x12x24 fixture's task at the wide pads"""
    from xenoverse_amd.linds import teacher
    from test_gpu_linds_mpc import _host_job
    K = 20
    g, task = load_linds_golden(FILES[0])
    n = 16
    env = LinDSVecEnv(n, autoreset_mode="disabled", seed=3, **WIDE)
    env.set_task(task)
    assert (env.NS, env.NA, env.NO) == KEYS[3]
    rng = np.random.RandomState(0)
    env.reset_injected(np.arange(n) % 3)                  # the three initial states near the command
    for _ in range(4):
        env.step_injected(rng.uniform(-1, 1, (n, 16)).astype(np.float32), rng.standard_normal((16, n)).astype(np.float32),
                          np.zeros(n, np.int32))
    st = _np(env.get_state()[1]).copy()
    st[n // 2:] = int(task["max_steps"]) - 3              # near truncation: the future commands run past max_steps
    env.set_state(steps=st)
    a, info = env.mpc_action(K=K, return_info=True)
    a, U, status = _np(a), _np(info["U"]), _np(info["status"])
    x = _np(env.state)
    ref = env.get_future_inner_cmds(K)
    m = teacher.model_from_task(task, pad_action_dim=16)
    assert (m.Nu, m.Ny) == (12, 24) and a.shape == (n, 16) and ref.shape == (n, K, 32)
    assert np.all(np.abs(a) <= 1.0) and np.all(np.abs(U) <= 1.0)
    assert np.all(a[:, 12:] == 0.0)                       # the padded action columns
    nk = K * m.Nu
    n_u0 = 0
    for i in (0, 1, 2, 9, 13):
        Us, Js, P, q, kappa = _host_job((m, K, x[i, :m.Nx].astype(np.float64), ref[i, :, :m.Ny].astype(np.float64)))
        assert np.all(U[i, nk:] == 0.0)
        assert np.array_equal(a[i, :m.Nu], U[i, :m.Nu])          # the action is u_0 of the plan
        u = U[i, :nk].astype(np.float64)
        gap = (0.5 * u @ P @ u + q @ u - Js) / (1.0 + abs(Js))    # every env, whatever its status
        assert gap <= 1e-4, (i, gap, kappa, status[i])
        if kappa <= 1e4:
            assert np.abs(a[i, :m.Nu] - Us[:m.Nu]).max() <= 1e-3, (i, kappa, status[i])
            n_u0 += 1
    print("kappa <= 1e4 in %d of 5 QPs; converged %.3f" % (n_u0, np.mean(status == 1)))
    assert np.mean(status == 1) >= 0.99
    env.close()
