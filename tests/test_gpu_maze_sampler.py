"""The device MazeWorld task sampler and resampler (xv_maze_sample_tasks, xv_maze_resample_tasks, csrc/maze_sampler.hip)
against their numpy restatement (mazeworld/sampler_host.py), bit for bit, across launch geometries, and end to end through
the step engine and the device teacher.  The restatement of the two larger 256-candidate batches is recorded under
tests/golden/ (scripts/gen_golden_maze_sampler.py; tests/test_host_maze_sampler.py re-makes some of its entries)."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

from xenoverse_amd import _lib
from xenoverse_amd.engine import Engine
from xenoverse_amd.mazeworld import (MazeWorldVecEnv, SmartSLAMAgent, build_tables, make_texture_library,
                                     resample_tasks_device, sample_candidates, sample_tasks_device, task_dicts_from_device)
from xenoverse_amd.mazeworld import device_sampler as ds
from xenoverse_amd.mazeworld import sampler_host as sh

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SLOTS = ds.SLOT_KEYS
N_CAND = 256
TEX = dict(n_wall_textures=8, n_ground_textures=4, n_ceiling_textures=4)


@pytest.fixture(scope="module")
def engine():
    e = Engine("cuda:0")
    yield e
    e.close()


def _host(r):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}


def _check_tan(dbl):
    want = np.array([np.tan(float(f) / 2) for f in dbl[:, 3]])
    assert np.array_equal(dbl[:, 7], want)


@pytest.mark.parametrize("kwargs", [dict(n_range=(7, 8)), dict(n_range=(9, 10)), dict(n_range=(9, 10), allow_loops=False)],
                         ids=["n7", "n9", "n9_no_loops"])
def test_device_equals_host_small(engine, kwargs):
    """every slot, the status and the info record of 256 candidates against sample_candidate_host: n = 7 (one cell per
    lane, never a room), n = 9 (rooms appear; with and without loops)"""
    got = _host(sample_candidates(engine, 31, 5, N_CAND, info=True, **kwargs))
    want = sh.sample_slots_host(31, 5, N_CAND, **kwargs)
    assert got["NG"] == want["NG"] and got["n_cmd"] == want["n_cmd"]
    assert np.array_equal(got["info"], want["info"]) and np.array_equal(got["status"], want["status"])
    for k in SLOTS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    _check_tan(got["dbl"])
    rooms = want["info"]["rooms"]
    assert (rooms == 0).all() if kwargs["n_range"][0] == 7 else (rooms > 0).any()
    assert (want["status"] == 0).all()


@pytest.mark.parametrize("name", ["default", "n63"])
def test_device_equals_host_recorded(engine, name):
    """the default n_range (9, 25) — mixed n in one batch, padding to NG = 25 — and n_range (63, 64), the largest grid and
    63 cells per lane: 256 candidates each against the recorded restatement (info records word for word, every slot by its
    SHA-256), dbl[:, 7] against numpy.tan"""
    g = np.load(os.path.join(GOLDEN, "sampler_maze_host_%s.npz" % name))
    n_range = tuple(int(v) for v in g["n_range"])
    got = _host(sample_candidates(engine, int(g["seed"]), 0, N_CAND, info=True, n_range=n_range))
    assert got["NG"] == sh.grid_pitch(n_range) and got["walls"].shape == (N_CAND, got["NG"], got["NG"])
    words = np.frombuffer(got["info"].tobytes(), np.int32).reshape(N_CAND, 6)
    assert np.array_equal(words, g["info_words"])
    assert np.array_equal(got["status"], g["info_words"][:, 0])
    bad = [q for q in range(N_CAND) if not np.array_equal(sh.slots_digest(got, q), g["digest"][q])]
    assert not bad, bad
    _check_tan(got["dbl"])
    ns = g["info_words"][:, 1]
    assert len(set(ns.tolist())) > (4 if name == "default" else 0) and ns.max() == got["NG"]
    q = int(np.argmin(ns))      # padding beyond the smallest task's n
    n = int(ns[q])
    assert got["walls"][q, n:].all() and got["walls"][q, :, n:].all() and (got["landmarks"][q, n:] == -1).all()
    assert not got["texts"][q, n:].any() and not got["texts"][q, :, n:].any()


def test_launch_geometry(engine):
    """300 candidates in one launch, as 7 + 293, and as 300 launches of one: the same bytes"""
    kw = dict(n_range=(9, 16), **TEX)
    whole = _host(sample_candidates(engine, 3, 40, 300, info=True, **kw))
    a, b = (_host(sample_candidates(engine, 3, 40, 7, info=True, **kw)),
            _host(sample_candidates(engine, 3, 47, 293, info=True, **kw)))
    ones = [_host(sample_candidates(engine, 3, 40 + q, 1, info=True, **kw)) for q in range(300)]
    for k in SLOTS + ("status", "info"):
        assert np.array_equal(whole[k], np.concatenate([a[k], b[k]])), k
        assert np.array_equal(whole[k], np.concatenate([o[k] for o in ones])), k


def test_batch_size_does_not_change_the_tasks(engine):
    a = sample_tasks_device(64, seed=6, engine=engine, batch=16, **TEX)
    b = sample_tasks_device(64, seed=6, engine=engine, batch=256, **TEX)
    for k in SLOTS:
        assert a[k].is_cuda and torch.equal(a[k], b[k]), k
    assert np.array_equal(a["info"], b["info"]) and a["NG"] == b["NG"] == 25 and a["n_cmd"] == 200
    assert a["stats"]["accepted"] == 64 and a["stats"]["candidates"] == b["stats"]["candidates"] >= 64
    with pytest.raises(RuntimeError):
        sample_tasks_device(64, seed=6, engine=engine, batch=16, max_candidates=32, **TEX)


@pytest.fixture(scope="module")
def tables(engine):
    """128 device-made tasks of mixed n, and their task dicts"""
    t = sample_tasks_device(128, seed=12, engine=engine, n_range=(9, 20), commands_sequence=50, **TEX)
    return t, task_dicts_from_device(t)


def test_task_dicts_round_trip(tables):
    t, tasks = tables
    assert len(set(int(n) for n in t["info"]["n"])) > 3
    again = build_tables(tasks)
    for k in SLOTS:
        got = t[k].cpu().numpy()
        n = again["NG"]
        if k in ("walls", "texts", "landmarks"):
            assert np.array_equal(got[:, :n, :n], again[k]), k
        else:
            assert np.array_equal(got, again[k]), k
    assert isinstance(tasks[0]["start"], tuple) and isinstance(tasks[0]["landmarks_coordinates"][0], tuple)
    assert tasks[0]["cell_walls"].shape == (int(t["info"]["n"][0]),) * 2


@pytest.mark.parametrize("cmd,start,lm", list(itertools.product((False, True), (False, True), ("keep", "new", "color"))))
def test_resampler_equals_host(engine, tables, cmd, start, lm):
    t, tasks = tables
    flags = dict(resample_cmd=cmd, resample_start=start, resample_landmarks=lm == "new",
                 resample_landmarks_color=lm == "color")
    new = resample_tasks_device(t, seed=77, episode=9, engine=engine, index_base=1000, **flags)
    for k in ("walls", "texts", "dbl"):
        assert new[k].data_ptr() == t[k].data_ptr()       # shared, not copied
    want = build_tables([sh.resample_host(task, 77, 1000 + i, 9, **flags) for i, task in enumerate(tasks)])
    n = want["NG"]
    assert np.array_equal(new["landmarks"].cpu().numpy()[:, :n, :n], want["landmarks"])
    assert (new["landmarks"].cpu().numpy()[:, n:] == -1).all()
    for k in ("lm_coord", "ints", "commands"):
        assert np.array_equal(new[k].cpu().numpy(), want[k]), k
    old = build_tables(tasks)
    assert np.array_equal(want["commands"], old["commands"]) != cmd
    assert np.array_equal(want["ints"][:, 1:3], old["ints"][:, 1:3]) != start
    assert np.array_equal(want["landmarks"], old["landmarks"]) == (lm == "keep")
    assert np.array_equal(t["commands"].cpu().numpy(), old["commands"])      # the given tables are left as they were


def _run(env, actions):
    out = []
    obs, info = env.reset()
    out.append((obs.cpu().numpy().copy(), info["command"].cpu().numpy().copy()))
    for a in actions:
        o, r, te, tr, info = env.step(a)
        d, ang = env.get_target_location()
        out.append(tuple(np.array(v.cpu().numpy()) for v in (o, r, te, tr, info["command"], d, ang)))
    return out


def test_end_to_end_frames_do_not_depend_on_who_built_the_tables(engine):
    """64 envs set from device tables as they are, 64 from build_tables(task_dicts_from_device(...)): 20 steps under the
    same seed and actions give the same frames, rewards, flags and target locations, byte for byte; again after
    resample_tasks_device"""
    lib = make_texture_library(8, 4, 4, seed=0)
    t = sample_tasks_device(64, seed=2, engine=engine, **TEX)
    rng = np.random.RandomState(0)
    actions = [rng.randint(0, 16, 64).astype(np.int32) for _ in range(20)]
    for tab in (t, resample_tasks_device(t, seed=5, episode=3, engine=engine, resample_landmarks=True)):
        runs = []
        for given in (tab, build_tables(task_dicts_from_device(tab))):
            env = MazeWorldVecEnv(64, resolution=(32, 32), textures=lib, seed=9, max_steps=15)
            env.set_task(given)
            if given is tab:
                assert env._tab["walls"].data_ptr() == tab["walls"].data_ptr()      # no host copy
            runs.append(_run(env, actions))
            env.close()
        for a, b in zip(*runs):
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        assert any(step[2].any() or step[3].any() for step in runs[0][1:])      # episodes ended and restarted on the way


def test_device_agent_runs_on_device_made_tables(engine):
    lib = make_texture_library(8, 4, 4, seed=0)
    t = sample_tasks_device(16, seed=4, engine=engine, n_range=(9, 16), **TEX)
    env = MazeWorldVecEnv(16, resolution=(32, 32), textures=lib, seed=1)
    env.set_task(t)
    obs, _ = env.reset()
    agent = SmartSLAMAgent(maze_env=env)
    for _ in range(5):
        a = agent.step(obs, None)
        assert a.shape == (16,) and int(a.min()) >= 0 and int(a.max()) < 16
        obs = env.step(a)[0]
    assert int(agent.inspect()["mask"].sum()) > 0 and env.check_errors() == 0
    agent.close(); env.close()


def test_bad_arguments_launch_nothing(engine):
    lib = engine.lib
    a = sh.sampler_arguments()
    out = ds._slot_tensors(4, 25, 200, engine.device)
    status = torch.full((4,), -7, dtype=torch.int32, device=engine.device)
    out["walls"].fill_(5)

    def call(NG=25, null=None, **change):
        p = ds._params(dict(a, **change))
        slots = ds._Slots(*[None if k == null else _lib.ptr(out[k]) for k in SLOTS])
        return lib.xv_maze_sample_tasks(engine.handle, 1, 0, 4, NG, C.cast(C.byref(p), C.c_void_p),
                                        C.cast(C.byref(slots), C.c_void_p), None, _lib.ptr(status))

    lib.xv_last_error.restype = C.c_char_p
    for kw in (dict(NG=24), dict(NG=26, n_range=(9, 27)), dict(n_range=(5, 25)), dict(NG=65, n_range=(9, 66)),
               dict(landmarks_number_range=(1, 15)), dict(null="walls"), dict(null="lm_coord")):
        assert call(**kw) < 0, kw
        assert b"xv_maze_sampler_check: invalid argument" in lib.xv_last_error(), kw
    assert lib.xv_maze_sample_tasks(engine.handle, 1, 0, 4, 25, None, None, None, None) < 0
    engine.sync()
    assert (status.cpu().numpy() == -7).all() and (out["walls"].cpu().numpy() == 5).all()      # nothing ran
    assert call() == 0
    engine.sync()
    assert (status.cpu().numpy() == 0).all()
    with pytest.raises(ValueError):
        resample_tasks_device(dict(walls=np.zeros((1, 9, 9), np.int8)))
    t = sample_tasks_device(4, seed=1, engine=engine, **TEX)
    with pytest.raises(_lib.XenoError):
        resample_tasks_device(t, episode=1 << 24, engine=engine)
