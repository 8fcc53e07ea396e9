"""AcrobotVecEnv — N domain-randomised Acrobots per kernel launch.

Mirrors xenoverse/metacontrol/random_acrobot.py: sample_acrobot :14-39, RandomAcrobotEnv.__init__ :43-55
(frameskip, reset_bounds_scale), _dsdt :58-96, _terminal :98-101, set_task :103-106, step :108-117, reset :119-130;
registered id `random-acrobot-v0` uses frameskip=1, reset_bounds_scale=0.10 (metacontrol/__init__.py:27-33).
The integrator around _dsdt is gymnasium's AcrobotEnv (not installed here): that part is unpinned, see
include/xeno.h.
"""
import numpy as np

from ..spaces import Box, Discrete
from .base import ControlVecEnv, _versatile

TASK_KEYS = ("link_length_1", "link_length_2", "link_mass_1", "link_mass_2", "link_com_1", "link_com_2", "gravity")


def sample_acrobot(link_length_1=True, link_length_2=True, link_mass_1=True, link_mass_2=True, link_com_1=True,
                   link_com_2=True, gravity=True, seed=None):
    """Same ranges and keys as the reference sampler (random_acrobot.py:14-39).  The reference is time-seeded
    and not reproducible; `seed` (optional) makes this one reproducible."""
    rng = np.random.RandomState(seed)
    l1 = _versatile(link_length_1, (0.5, 3.0), 1.0, rng)
    l2 = _versatile(link_length_2, (0.5, 3.0), 1.0, rng)
    m1 = _versatile(link_mass_1, (0.5, 3.0), 1.0, rng)
    m2 = _versatile(link_mass_2, (0.5, 3.0), 1.0, rng)
    c1 = _versatile(link_com_1, (0.25, 0.75), 0.5, rng) * l1
    c2 = _versatile(link_com_2, (0.25, 0.75), 0.5, rng) * l2
    g = _versatile(gravity, (1.0, 15.0), 9.8, rng)
    return {"link_length_1": l1, "link_length_2": l2, "link_mass_1": m1, "link_mass_2": m2, "link_com_1": c1,
            "link_com_2": c2, "gravity": g}


class AcrobotVecEnv(ControlVecEnv):
    PREFIX = "xv_acrobot"
    OBS_DIM = 6
    TASK_KEYS = TASK_KEYS

    def __init__(self, num_envs, frameskip=5, reset_bounds_scale=0.10, max_steps=0, device="cuda:0", seed=0,
                 env_id_base=0, autoreset_mode="same_step", to_numpy=False, engine=None, copy=True):
        hi = np.array([1.0, 1.0, 1.0, 1.0, 4 * np.pi, 9 * np.pi], np.float32)   # AcrobotEnv.observation_space
        super().__init__(num_envs, frameskip, reset_bounds_scale, max_steps, Box(-hi, hi, dtype=np.float32), Discrete(3),
                         device=device, seed=seed, env_id_base=env_id_base, autoreset_mode=autoreset_mode,
                         to_numpy=to_numpy, engine=engine, copy=copy)

    def _read_scale(self, scale):
        # a scalar scale multiplies in float32 as the reference's does, a vector in float64 (random_acrobot.py:123-125)
        self._scale_is_vector = isinstance(scale, (list, tuple, np.ndarray))
        if self._scale_is_vector:
            assert len(scale) == 4, "reset_bounds_scale should be a list of 4 elements"
            return np.asarray(scale, np.float64)
        return np.full(4, float(scale), np.float64)

    def _create_extras(self):
        return (1 if self._scale_is_vector else 0,)
