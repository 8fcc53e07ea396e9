"""Who destroys a device learner's C handle, and when (xenoverse_amd/anymdp/learner.py: close; vec_env.py:
_release_learners), on stand-ins for the library and the env: the C learner borrows the env's handle, so it must be destroyed
exactly once and never after that handle.  The cyclic collector clears the env's weak references to its learners before it
runs any finaliser; an env finalised first must still destroy them, and their own finalisers must then leave them alone.
CPU only."""
import ctypes as C
import gc
import weakref

from xenoverse_amd.anymdp.learner import _DeviceLearner
from xenoverse_amd.anymdp.vec_env import AnyMDPVecEnv


class _Lib(object):
    def __init__(self, env):
        self.env, self.destroyed, self.next = env, [], 100

    def xv_stub_create(self, env_h, out):
        self.next += 1
        out._obj.value = self.next
        return 0

    def xv_stub_destroy(self, h):
        self.destroyed.append((h.value, self.env._h is not None and self.env.engine.handle is not None))
        return 0


class _Engine(object):
    handle = 1


class _Env(object):
    num_envs, S, A, task_type, _parent = 4, 3, 2, "MDP", None
    _release_learners = AnyMDPVecEnv._release_learners

    def __init__(self):
        self._h, self.engine, self.lib = C.c_void_p(7), _Engine(), _Lib(self)
        self._learners, self._learner_handles = weakref.WeakSet(), {}

    def _require_task(self):
        pass

    def close(self):                      # AnyMDPVecEnv.close_extras: the learners first, then the handle
        self._release_learners("its env was closed")
        self._h = None

    def __del__(self):
        self.close()


class _Learner(_DeviceLearner):
    _ABI = "xv_stub"

    def __init__(self, env):
        self._check_env(env)
        self._create(env)


def test_close_destroys_once_and_the_env_forgets_the_handle():
    env = _Env()
    a, b = _Learner(env), _Learner(env)
    a.close()
    a.close()
    assert env.lib.destroyed == [(101, True)] and list(env._learner_handles) == [102]
    env.close()
    assert env.lib.destroyed == [(101, True), (102, True)] and env._learner_handles == {}
    b.close()
    assert len(env.lib.destroyed) == 2


def test_env_finalised_first_with_its_weak_references_cleared():
    """what the cyclic collector does when it takes an env and its learner together and runs the env's finaliser first"""
    env = _Env()
    lr = _Learner(env)
    env._learners = weakref.WeakSet()     # the collector has cleared the weak references
    env.close()
    assert env.lib.destroyed == [(101, True)]
    lr.close()                            # the learner's finaliser: the env's handle is gone, the C learner too
    assert env.lib.destroyed == [(101, True)]


def test_collected_together_in_either_order():
    lib_logs = []
    for _ in range(8):
        env = _Env()
        lrs = [_Learner(env), _Learner(env)]
        lib_logs.append(env.lib.destroyed)
        cycle = [env, lrs]
        cycle.append(cycle)               # env and learners die in one pass of the cyclic collector
        del env, lrs, cycle
    gc.collect()
    for log in lib_logs:
        assert sorted(h for h, _ in log) == [101, 102], log      # each exactly once
        assert all(alive for _, alive in log), log                # and while the env's handle and the engine lived
