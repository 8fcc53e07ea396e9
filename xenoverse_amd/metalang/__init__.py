"""MetaLang on the device: the reference's MetaLangV2 (xenoverse/metalang: random n-gram networks that emit synthetic
pseudo-languages), csrc/metalang.hip, and its MetaLMV3Env (a random recurrent language model that poses queries, answers
them and rewards answers by perplexity), csrc/metalm.hip, with the V3 generator's QA / QAR / QARA training streams
(generator_v3.py: MetaLMV3VecEnv.stream assembles them in one launch) and its task acceptance test (device_sampler.py makes
and tests candidates in one launch, csrc/metalm_sampler.hip); and its MetaLangV1 (chains of random integer patterns to be
recovered from a noisy copy), csrc/metalang_v1.hip, with generator_v1.py.  MetaLangV2 and MetaLangV1 tasks are made on the
device as well (device_sampler_v2.py, device_sampler_v1.py, csrc/metalang_sampler.hip): sample_tasks_v2_device,
sample_tasks_v1_device; the unqualified sample_tasks_device is MetaLMV3's."""
from .task_sampler import LIMITS, TaskSamplerV1, TaskSamplerV2  # noqa: F401
from .host import MetaLangV2Host  # noqa: F401
from .host_v1 import LIMITS_V1, MetaLangV1Host  # noqa: F401
from .batch import MetaLangV2, MetaLangV2Batch, describe_dispatch  # noqa: F401
from .batch_v1 import MetaLangV1, MetaLangV1Batch  # noqa: F401
from .lm_host import FUNCTION_VOCABULARY, LM_LIMITS, RandomLMHost, TaskSamplerV3  # noqa: F401
from .lm_env import MetaLMV3Env, MetaLMV3VecEnv  # noqa: F401
from .stream_host import generate_data_v3_host  # noqa: F401
from .device_sampler import sample_candidates, sample_tasks_device  # noqa: F401
from .device_sampler import task_dicts_from_device as _task_dicts_from_device_v3
from .device_sampler_v1 import is_tables_v1, sample_tasks_v1_device, task_dicts_from_device_v1  # noqa: F401
from .device_sampler_v2 import is_tables_v2, sample_tasks_v2_device, task_dicts_from_device_v2  # noqa: F401
from .generator_v3 import (generate_data_v3_batch, generate_data_v3_single_task_qa,  # noqa: F401
                           generate_data_v3_single_task_qar, generate_data_v3_single_task_qara, metalang_generator_v3,
                           sample_and_check_task, sample_and_check_tasks)


def task_dicts_from_device(tables, index=None):
    """the tasks of a device sampler's tables dict as the host sampler's dicts: TaskSamplerV2's for sample_tasks_v2_device's
    tables, TaskSamplerV1's for sample_tasks_v1_device's, TaskSamplerV3's for sample_tasks_device's"""
    if is_tables_v2(tables):
        return task_dicts_from_device_v2(tables, index)
    if is_tables_v1(tables):
        return task_dicts_from_device_v1(tables, index)
    return _task_dicts_from_device_v3(tables, index)
