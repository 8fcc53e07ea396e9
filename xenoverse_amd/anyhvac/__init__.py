"""AnyHVAC: batched data-centre thermal environments (the reference's anyhvac family).

    from xenoverse_amd.anyhvac import HVACEnv, HVACTaskSampler      # the reference's line with the package name changed

HVACTaskSampler / task_from_reference: tasks as flat dicts (task_sampler.py); HVACHost: the fp64 numpy restatement, pinned
bit for bit to recorded runs of the reference (host.py); HVACVecEnv: the batched device env (vec_env.py); HVACEnv: the
one-room env with the reference's surface (single_env.py);
PIDHost / pid_weights / pid_search_host: the reference's PID teachers restated on the host (pid.py);
HVACSolverGTPID / HVACSolverLOCPID / HVACSolverGridSearchPID: the teachers on the device (solvers.py);
DiscreteActionHost / DiffActionHost: the reference's RL action spaces restated on the host (actions.py);
HVACEnvDiscreteAction / HVACEnvDiffAction: the same on the device (single_env.py), HVACVecEnv(action_mode=...) batched
(vec_env.py);
sample_tasks_device / sample_candidates / task_dicts_from_device: tasks made on the device as the table rows set_task
borrows (device_sampler.py), sample_candidate_host / sample_rows_host: their numpy restatement (sampler_host.py).
"""
from .actions import ActionMapHost, DiffActionHost, DiscreteActionHost            # noqa: F401
from .config import DEFAULTS                                                      # noqa: F401
from .device_sampler import sample_candidates, sample_tasks_device, task_dicts_from_device   # noqa: F401
from .sampler_host import sample_candidate_host, sample_rows_host, table_dims, wind_diffuser_host   # noqa: F401
from .host import HVACHost, average_total_heat, check_settings, heater_powers    # noqa: F401
from .pid import PIDHost, pid_search_host, pid_weights                            # noqa: F401
from .task_sampler import HVACTaskSampler, task_from_reference, wind_diffuser    # noqa: F401
from .tables import build_tables                                                  # noqa: F401
from .single_env import HVACEnv, HVACEnvDiffAction, HVACEnvDiscreteAction       # noqa: F401
from .solvers import HVACSolverGridSearchPID, HVACSolverGTPID, HVACSolverLOCPID   # noqa: F401
from .vec_env import HVACVecEnv                                                   # noqa: F401
