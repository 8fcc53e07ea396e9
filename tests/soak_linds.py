"""Randomised soak of the LinDS step kernels against the CPU oracle (not collected by pytest; run as a script on a GPU box,
`PYTHONPATH=.:tests python tests/soak_linds.py [seconds]`): tasks drawn by the package's seed-compatible sampler with random
dimensions — up to 32 states, 16 actions and 32 observations, the env padded to the compiled sizes that hold them, so that a
run visits all eight (NS, NA, NO) kernel keys — random env -> task maps and counts (partial tiles, one-env tasks), both
kernels, the three auto-reset modes, injected draws — state and observation bit for bit, command / error / reward within 1e-5
as the unit tests."""
import sys
import time

import numpy as np

import oracle
from xenoverse_amd.linds import LinDSVecEnv, build_tables, pad_tables, task_sampler
from xenoverse_amd.linds.task_sampler import LinearDSSampler
from xenoverse_amd.linds.tables import _pad_to
from util import close_rel

# With 20 or more tracked observations hardly any draw of initial states starts within 3 of the command, and the sampler's
# 20,000 rejected draws per task would be the soak's whole run time: it goes to its shrinking fallback after 200 here.
task_sampler.MAX_DRAWS = 200

MODES = {"disabled": 0, "next_step": 1, "same_step": 2}


def _np(t):
    return t.detach().cpu().numpy()


class Mismatch(Exception):
    pass


def _check(ok, what):
    if not ok:
        raise Mismatch(what)


def soak(rng, seed):
    n_task = int(rng.randint(1, 7))
    ns = int(rng.choice([rng.randint(2, 17), rng.randint(17, 33)]))
    same_dims = rng.random_sample() < 0.5
    na_top, no_top = int(rng.randint(1, 17)), int(rng.randint(1, 33))      # this configuration's largest dims
    tasks = []
    for k in range(n_task):
        d = ns if same_dims else int(rng.randint(2, ns + 1))
        t = LinearDSSampler(state_dim=d, action_dim=int(rng.randint(1, na_top + 1)), observation_dim=int(rng.randint(1, no_top + 1)),
                            seed=seed + k)
        t["max_steps"] = int(rng.randint(5, 40))
        tasks.append(t)
    NA = _pad_to(max(t["action_dim"] for t in tasks), (8, 16))
    NO = _pad_to(max(t["observation_dim"] for t in tasks), (16, 32))
    pads = dict(pad_action_dim=NA, pad_observation_dim=NO, pad_command_dim=NO)
    tab = pad_tables(build_tables(tasks, **pads))
    key = (4 if tab["NS"] == 32 else 0) | (2 if NA == 16 else 0) | (1 if NO == 32 else 0)      # csrc/linds.hip: LINDS_DISPATCH
    counts = [int(rng.choice([1, rng.randint(1, 20), 64, rng.randint(20, 200)])) for _ in range(n_task)]
    env_task = np.repeat(np.arange(n_task, dtype=np.int32), counts)
    layout = str(rng.choice(["grouped", "shuffled"]))
    if layout == "shuffled":
        rng.shuffle(env_task)
    n = len(env_task)
    mode = str(rng.choice(list(MODES)))
    path = str(rng.choice(["mfma", "mfma", "scalar"]))
    env = LinDSVecEnv(n, autoreset_mode=mode, seed=seed, **pads)
    env.set_task(tasks, env_task_index=env_task)
    env.set_path(path)
    _check((env.NS, env.NA, env.NO) == (tab["NS"], NA, NO), "kernel key")
    ora = oracle.LinDSOracle(tab, env_task)
    n_init = tab["ints"][env_task, 2]
    idx0 = (rng.random_sample(n) * n_init).astype(np.int32)
    obs, info = env.reset_injected(idx0)
    o0 = ora.reset_injected(idx0)
    no = _np(obs).shape[1]
    _check(np.array_equal(_np(obs), o0["obs"][:, :no]), "reset obs")
    T = int(rng.randint(10, 60))
    na = tab["NA"]
    for t in range(T):
        a = rng.uniform(-1.4, 1.4, (n, na)).astype(np.float32)
        z = rng.standard_normal((tab["NS"], n)).astype(np.float32)
        idx = (rng.random_sample(n) * n_init).astype(np.int32)
        d = env.step_injected(a, z, idx)
        o = ora.step_injected(a, z, idx, MODES[mode])
        obs, r, term, trunc, info = d
        _check(np.array_equal(_np(term).astype(np.uint8), o["terminated"]), "terminated")
        _check(np.array_equal(_np(trunc).astype(np.uint8), o["truncated"]), "truncated")
        _check(np.array_equal(_np(obs), o["obs"][:, :no]), "obs")
        _check(close_rel(_np(info["command"]), o["cmd"][:, :no], 1e-5, 2e-6), "command")
        _check(close_rel(_np(info["error"]), o["error"], 1e-5, 2e-6), "error")
        _check(close_rel(_np(r), o["reward"], 1e-5, 2e-6), "reward")
        x, st, nr = env.get_state()
        _check(np.array_equal(_np(x), ora.x) and np.array_equal(_np(st), ora.steps), "state / steps")
        _check(np.array_equal(_np(nr), ora.need_reset), "need_reset")
        done = (o["terminated"] | o["truncated"]).astype(bool)
        if mode == "same_step" and done.any():
            _check(np.array_equal(_np(info["final_obs"])[done], o["final_obs"][done][:, :no]), "final_obs")
        if mode == "disabled" and done.any():
            env.reset_injected(idx, mask=done.astype(np.uint8))
            ora.reset_injected(idx, mask=done.astype(np.uint8))
    _check(env.check_errors() == 0, "device error flags")
    env.close()
    return "linds tasks=%d ns<=%d (NS %d NA %d NO %d key %d) envs=%d %s path=%s mode=%s steps=%d" % (
        n_task, ns, tab["NS"], tab["NA"], tab["NO"], key, n, layout, path, mode, T)


if __name__ == "__main__":
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    t_end = time.time() + budget
    master = np.random.RandomState(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    n, keys = 0, set()
    while time.time() < t_end:
        seed = int(master.randint(1, 1 << 30))
        try:
            line = soak(np.random.RandomState(seed), seed)
        except Mismatch as ex:
            print("MISMATCH with seed %d: %s" % (seed, ex), flush=True)
            sys.exit(1)
        n += 1
        keys.add(int(line.split(" key ")[1].split(")")[0]))
        print("ok seed=%d %s" % (seed, line), flush=True)
    print("TOTAL %d configurations, 0 mismatches, keys visited %s" % (n, sorted(keys)))
