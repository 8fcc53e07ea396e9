"""LinDS on MI355X.  Drop-in for the step/reset path of `xenoverse.linds` (reference package)."""
from .tables import build_dynamics_matrices, build_tables, pad_tables  # noqa: F401
from .vec_env import LinDSVecEnv  # noqa: F401
from .task_sampler import LinearDSSampler, LinearDSSamplerRandomDim, RandomFourier  # noqa: F401
from .teacher import LTISystemMPC  # noqa: F401
from .device_sampler import (build_tables_device, build_zoh_device, sample_candidates,  # noqa: F401
                             sample_tasks_device, task_dicts_from_device)
