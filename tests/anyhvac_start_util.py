"""what the AnyHVAC episode-protocol tests share: the fixtures of scripts/gen_golden_anyhvac_start.py
(tests/golden/start_anyhvac_*.npz) and the walk over a fixture's resets and steps.

A reset's start time, resting cooler, history length and last failure are integers or exact float64 values formed from
integers, the injected draws and one correctly rounded square root: device, host and recording agree on them exactly, and
the tests ask for that.  Everything a step computes is held to the derived bounds of anyhvac_util.py (and
anyhvac_act_util.py for `rl`), imported as they are.
"""
import os

import numpy as np

from util import golden_files
from xenoverse_amd.anyhvac.actions import DiffActionHost
from xenoverse_amd.anyhvac.host import HVACHost

FILES = {os.path.basename(p)[len("start_anyhvac_"):-4]: p for p in golden_files("start_anyhvac_")}
RUNS = ("inv", "choice", "back", "early", "trunc", "record", "rl")
SIZE_CAP = 400 * 1024      # "a few hundred KB at most, like its siblings"
OBS = ("sensor_readings", "heat_readings", "action_temp")
RL_OPTS = dict(discretize_rl_action_space=True, add_action_cost=False, too_cold_limit=False)      # run_rl.py:41
_cache = {}


def load(name):
    """-> (fixture dict, flat task dict, env settings, flags (random start, record, no-terminate))"""
    if name not in _cache:
        g = dict(np.load(FILES[name], allow_pickle=False))
        if bool(g["rl"]):
            g["action"] = g["applied_value"]      # (the name anyhvac_util.check_step knows the cooler count by)
        task = {k[5:]: (v if v.ndim else v[()]) for k, v in g.items() if k.startswith("task_")}
        settings = dict(max_steps=int(g["set_max_steps"]), iter_per_step=int(g["set_iter_per_step"]),
                        sec_per_iter=float(g["set_sec_per_iter"]), reward_mode=int(g["set_reward_mode"]))
        flags = (bool(g["flag_random_start_t"]), bool(g["flag_generate_record"]), bool(g["flag_overheat_no_terminated"]))
        _cache[name] = (g, task, settings, flags)
    return _cache[name]


def events(g):
    """the fixture's order of events: ("reset", j) and ("step", k)"""
    at = g["reset_at"].tolist()
    out = []
    for k in range(int(g["n_steps"]) + 1):
        out += [("reset", j) for j, a in enumerate(at) if a == k]
        if k < int(g["n_steps"]):
            out.append(("step", k))
    return out


def raw_action(g, k):
    return g["raw_action"][k] if bool(g["rl"]) else g["action"][k]


def host_of(name):
    """the fixture's host class with its task and flags set (not reset)"""
    g, task, settings, flags = load(name)
    if bool(g["rl"]):
        h = DiffActionHost(**settings)
        h.set_task(task, generate_task=bool(g["generate_task"]), **RL_OPTS)
    else:
        h = HVACHost(**settings)
        h.set_task(task, generate_task=bool(g["generate_task"]))
    h.set_random_start_t(flags[0])
    h.set_generate_record(flags[1])
    h.set_overheat_no_termiated_training_only(flags[2])
    return h
