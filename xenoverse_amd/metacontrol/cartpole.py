"""CartPoleVecEnv — N domain-randomised CartPoles per kernel launch.

Mirrors xenoverse/metacontrol/random_cartpole.py: sample_cartpole :13-29, RandomCartPoleEnv.__init__ :33-44
(frameskip, reset_bounds_scale), set_task :46-50, step :52-61, reset :63-75; registered id
`random-cartpole-v0` uses frameskip=1, reset_bounds_scale=[0.45, 0.90, 0.13, 1.0] (metacontrol/__init__.py:20-26).
The physics is gymnasium's CartPoleEnv (not installed here): parity unpinned, see include/xeno.h.
"""
import numpy as np

from ..spaces import Box, Discrete
from .base import ControlVecEnv, _versatile


def sample_cartpole(gravity_scope=True, masscart_scope=True, masspole_scope=True, length_scope=True, seed=None):
    """Same ranges and keys as the reference sampler (random_cartpole.py:13-29).  The reference is
    time-seeded and not reproducible; `seed` (optional) makes this one reproducible."""
    rng = np.random.RandomState(seed)
    return {"gravity": _versatile(gravity_scope, (1, 11), 9.8, rng),
            "masscart": _versatile(masscart_scope, (0.5, 2.0), 1.0, rng),
            "masspole": _versatile(masspole_scope, (0.05, 0.20), 0.1, rng),
            "length": _versatile(length_scope, (0.25, 1.0), 0.5, rng)}


class CartPoleVecEnv(ControlVecEnv):
    PREFIX = "xv_cartpole"
    OBS_DIM = 4
    TASK_KEYS = ("gravity", "masscart", "masspole", "length")

    def __init__(self, num_envs, frameskip=5, reset_bounds_scale=(0.45, 0.90, 0.13, 1.0), max_steps=0,
                 device="cuda:0", seed=0, env_id_base=0, autoreset_mode="same_step", to_numpy=False,
                 engine=None, copy=True):
        hi = np.array([4.8, np.finfo(np.float32).max, 0.41887903, np.finfo(np.float32).max], np.float32)
        super().__init__(num_envs, frameskip, reset_bounds_scale, max_steps, Box(-hi, hi, dtype=np.float32), Discrete(2),
                         device=device, seed=seed, env_id_base=env_id_base, autoreset_mode=autoreset_mode,
                         to_numpy=to_numpy, engine=engine, copy=copy)

    def _read_scale(self, scale):
        rs = list(scale)
        assert len(rs) == 4, "reset_bounds_scale should be a list of 4 elements"
        return np.asarray(rs, np.float64)
