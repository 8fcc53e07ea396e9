"""Shared helpers for the parity tests (golden loading, task-dict rebuilding)."""
import glob
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_files(prefix):
    return sorted(glob.glob(os.path.join(GOLD, prefix + "*.npz")))


def anymdp_fixture_task(g):
    """the MDP task dict of a loaded anymdp_* / qlearn_anymdp_* / mbrl_anymdp_* fixture"""
    return dict(ns=int(g["ns"]), na=int(g["na"]), max_steps=float(g["max_steps"]), state_mapping=g["state_mapping"],
                task_type="MDP", s_0=g["s_0"], s_0_prob=g["s_0_prob"], s_e=g["s_e"], transition=g["transition"],
                reward=g["reward"], reward_noise=g["reward_noise"])


def load_anymdp_golden(path):
    g = dict(np.load(path, allow_pickle=False))
    return g, anymdp_fixture_task(g)


def anymdp_tasks16():
    return [load_anymdp_golden(p)[1] for p in golden_files("anymdp_16x4")[:4]]


def anymdp_random_task(S, A, seed, max_steps=50, n_terminal=0):
    """a random MDP: every (s, a) row reaches 6 next states; s_0 = the first 4 states.  n_terminal: the last n_terminal
    states are terminal (s_e; none of them in s_0) and their rows are all zero, as in the reference's tasks (build_tables
    makes such rows CDF 1.0: they are never sampled from).  The draws do not depend on n_terminal."""
    assert S >= 6 and S - n_terminal >= 4
    rng = np.random.RandomState(seed)
    T = np.zeros((S, A, S))
    for s in range(S):
        for a in range(A):
            T[s, a, rng.choice(S, 6, replace=False)] = rng.random_sample(6) + 0.1
    T /= T.sum(-1, keepdims=True)
    s_e = np.arange(S - n_terminal, S, dtype=np.int64)
    task = dict(ns=S, na=A, max_steps=float(max_steps), state_mapping=rng.permutation(S), task_type="MDP",
                s_0=np.arange(4), s_0_prob=np.full(4, 0.25), s_e=s_e, transition=T,
                reward=rng.randn(S, A, S) * (T > 0), reward_noise=np.full((S, A, S), 0.1))
    task["transition"][s_e] = 0.0
    task["reward"][s_e] = 0.0
    return task


def anymdp_env(tasks, n, seed, mode="same_step", env_id_base=0):
    from xenoverse_amd.anymdp import AnyMDPVecEnv
    env = AnyMDPVecEnv(n, seed=seed, env_id_base=env_id_base, autoreset_mode=mode)
    env.set_task(tasks)
    return env


def to_np(t):
    import torch
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def close_f32(a, b, rel=1e-5, abs_=1e-6):
    """north_star tolerance for float dynamics: 1e-5 relative (plus a float32 absolute floor)."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.all(np.abs(a - b) <= rel * np.abs(b) + abs_)


class FourierCommand(object):
    """Duck-type of the reference's RandomFourier (utils/random_nn.py:346-368): `.coeffs`, `.max_steps`."""

    def __init__(self, orders, coeffs, max_steps):
        self.coeffs = [(float(o), np.asarray(c, np.float64)) for o, c in zip(orders, coeffs)]
        self.max_steps = float(max_steps)

    def __call__(self, t):
        x = t / self.max_steps
        y = 0
        for order, coeff in self.coeffs:
            y = y + coeff[:, 0] * np.sin(order * x) + coeff[:, 1] * np.cos(order * x)
        return y


def load_linds_golden(path):
    g = dict(np.load(path, allow_pickle=False))
    dyn = bool(g["is_dynamic"])
    task = dict(state_dim=int(g["state_dim"]), observation_dim=int(g["observation_dim"]),
                action_dim=int(g["action_dim"]), max_steps=int(g["max_steps"]), ld_A=g["ld_A"], ld_B=g["ld_B"],
                ld_C=g["ld_C"], ld_X=g["ld_X"], ld_Y=g["ld_Y"], action_cost=float(g["action_cost"]),
                reward_base=float(g["reward_base"]), terminate_punish=float(g["terminate_punish"]),
                reward_factor=float(g["reward_factor"]), target_valid=g["target_valid"],
                target_type="dynamic_target" if dyn else "static_target",
                initial_states=[x for x in g["initial_states"]], noise_drift=float(g["noise_drift"]),
                target_delay=int(g["target_delay"]))
    task["command"] = (FourierCommand(g["four_orders"], g["four_coeffs"], g["four_period"]) if dyn
                       else g["command"])
    return g, task


def close_rel(a, b, rel=1e-5, abs_=1e-5):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return bool(np.all(np.abs(a - b) <= rel * np.abs(b) + abs_))


def load_maze_golden(path):
    g = dict(np.load(path, allow_pickle=False))
    task = dict(start=tuple(int(x) for x in g["start"]), cell_walls=g["cell_walls"], cell_texts=g["cell_texts"],
                cell_size=float(g["cell_size"]), ground_text=int(g["ground_text"]), ceiling_text=int(g["ceiling_text"]),
                step_reward=float(g["step_reward"]), goal_reward=float(g["goal_reward"]),
                collision_reward=float(g["collision_reward"]), wall_height=float(g["wall_height"]),
                agent_height=float(g["agent_height"]), fol_angle=float(g["fol_angle"]),
                commands_sequence=g["commands_sequence"],
                landmarks_coordinates=[tuple(int(v) for v in x) for x in g["landmarks_coordinates"]],
                cell_landmarks=g["cell_landmarks"])
    return g, task


def frame_mismatch(a, b):
    """fraction of channel values that differ, and the largest absolute difference"""
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))
    return float(np.mean(d > 0)), int(d.max())


def load_anymdp_tok_golden(path):
    g = dict(np.load(path, allow_pickle=False))
    mt = bool(g["is_mt"])
    task = dict(ns=int(g["ns"]), na=int(g["na"]), max_steps=float(g["max_steps"]), state_mapping=g["state_mapping"],
                task_type="MTPOMDP" if mt else "POMDP", s_0=g["s_0"], s_0_prob=g["s_0_prob"], s_e=g["s_e"],
                transition=g["transition"], reward=g["reward"], reward_noise=g["reward_noise"], no=int(g["no"]))
    if mt:
        task.update(do=int(g["do"]), da=int(g["da"]), observation_transition=[m for m in g["observation_transition"]])
    else:
        task["observation_transition"] = g["observation_transition"][0]
    return g, task


def load_raycast_ref(path):
    """tests/golden/raycast_ref_<W>x<H>_seed<k>.npz (oracle/gen_golden.py raycast_ref) and the maze_15 task its poses are in"""
    g = dict(np.load(path, allow_pickle=False))
    _, task = load_maze_golden(os.path.join(GOLD, "maze_15_seed%d.npz" % int(g["task"])))
    return g, task
