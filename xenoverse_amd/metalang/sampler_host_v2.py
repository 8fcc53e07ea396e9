"""Host restatement (numpy, fp64) of the device MetaLangV2 task sampler (csrc/metalang_sampler.hip: xv_metalang_sample_tasks):
the same Philox counters and the same constructions (host_draws.py), in the layout xv_metalang_set_task reads.  It is what
the device is compared with (tests/test_gpu_metalang_sampler.py) and the CPU-side proof that the model is the reference's
TaskSamplerV2 (xenoverse/metalang/task_sampler.py:22-50): the n-gram choice when n_gram is a list, then five arrays of
standard normals (tests/test_host_metalang_sampler.py checks the moments).

Task k of (seed, sizes, n_gram) is a pure function of those, whatever the batch — but not the task numpy's stream gives
for that seed (for that, `TaskSamplerV2(seed=...)`).  There is no acceptance test in the reference: every candidate is a
task.  The draws (index layout, host_draws.Draws(seed, k)):
  purpose 0, sub 0: n_gram = list[floor(u m)], u the first uniform of the call
  purposes 1 .. 5 (TASK_ARRAYS' order), sub = q >> 1: element q of the array's flat is half q & 1 of the fp64 Box-Muller pair
"""
import numpy as np

from ..host_draws import Draws, box_muller, floor_int, interleave
from .task_sampler import TASK_ARRAYS, check_limit

P_HEAD = 0
P_ARRAY = dict(zip(TASK_ARRAYS, range(1, 6)))      # csrc/metalang_sampler.hip MS_P_EMB .. MS_P_B_OUT
LIST_MAX = 16                                      # include/xeno.h XV_METALANG_SAMPLER_LIST_MAX


def n_gram_list(n_gram, limit, who="MetaLangV2"):
    """n_gram, an int or a list of ints -> the list; XenoError (the limit named) for an entry outside 1 .. limit or a list
    outside 1 .. LIST_MAX entries"""
    from .._lib import XenoError
    lst = [int(g) for g in n_gram] if isinstance(n_gram, (list, tuple, np.ndarray)) else [int(n_gram)]
    if not 1 <= len(lst) <= LIST_MAX:
        raise XenoError("%s: an n_gram list of %d entries is outside the supported range 1 .. %d" % (who, len(lst), LIST_MAX))
    for g in lst:
        if not 1 <= g <= limit:
            raise XenoError("%s: n_gram = %d is outside the supported range 1 .. %d" % (who, g, limit))
    return lst


def choice(seed, k, m):
    """the index into an n-gram list of m entries that task k draws"""
    return min(int(floor_int(Draws(seed, k).pairs(P_HEAD, 0)[0], m)), m - 1)


def normals(seed, k, purpose, n):
    """z[0 .. n) of one array of task k"""
    q = np.arange(n)
    return interleave(q, *box_muller(*Draws(seed, k).pairs(purpose, q >> 1)))


def check_sizes(n_vocab, n_emb, n_hidden):
    for name, v in (("n_vocab", n_vocab), ("n_hidden", n_hidden), ("n_emb", n_emb)):
        check_limit(name, v)


def sample_tables(n_tasks, n_emb=16, n_hidden=64, n_vocab=256, n_gram=3, _lambda=5.0, seed=0, task_base=0):
    """tasks task_base .. task_base + n_tasks - 1 -> the numpy tables dict in sample_tasks_v2_device's layout: word_emb
    [n, V, E], weights_inputlayer [n, NG, E, H] and bias_inputlayer [n, NG, H] (NG = max of the n-gram list; zeros at and
    beyond a task's n), weights_outputlayer [n, H, V], bias_outputlayer [n, V], _lambda [n], n_gram int32[n]"""
    from .task_sampler import LIMITS
    V, E, H, n_tasks = int(n_vocab), int(n_emb), int(n_hidden), int(n_tasks)
    check_sizes(V, E, H)
    lst = n_gram_list(n_gram, LIMITS["n_gram"])
    NG = max(lst)
    out = dict(word_emb=np.zeros((n_tasks, V, E)), weights_inputlayer=np.zeros((n_tasks, NG, E, H)),
               bias_inputlayer=np.zeros((n_tasks, NG, H)), weights_outputlayer=np.zeros((n_tasks, H, V)),
               bias_outputlayer=np.zeros((n_tasks, V)), _lambda=np.full(n_tasks, float(_lambda)),
               n_gram=np.zeros(n_tasks, np.int32))
    for i in range(n_tasks):
        k = int(task_base) + i
        n = lst[choice(seed, k, len(lst))]
        out["n_gram"][i] = n
        live = dict(word_emb=V * E, weights_inputlayer=n * E * H, bias_inputlayer=n * H, weights_outputlayer=H * V,
                    bias_outputlayer=V)
        for name in TASK_ARRAYS:
            out[name][i].reshape(-1)[:live[name]] = normals(seed, k, P_ARRAY[name], live[name])
    out.update(n_vocab=V, n_emb=E, n_hidden=H, n_gram_max=NG, seed=int(seed))
    return out
