"""MetaLang on the device: the reference's MetaLangV2 (xenoverse/metalang: random n-gram networks that emit synthetic
pseudo-languages), csrc/metalang.hip, and its MetaLMV3Env (a random recurrent language model that poses queries, answers
them and rewards answers by perplexity), csrc/metalm.hip, with the V3 generator's QA / QAR / QARA training streams
(generator_v3.py: MetaLMV3VecEnv.stream assembles them in one launch) and its task acceptance test (device_sampler.py makes
and tests candidates in one launch, csrc/metalm_sampler.hip); and its MetaLangV1 (chains of random integer patterns to be
recovered from a noisy copy), csrc/metalang_v1.hip, with generator_v1.py."""
from .task_sampler import LIMITS, TaskSamplerV1, TaskSamplerV2  # noqa: F401
from .host import MetaLangV2Host  # noqa: F401
from .host_v1 import LIMITS_V1, MetaLangV1Host  # noqa: F401
from .batch import MetaLangV2, MetaLangV2Batch  # noqa: F401
from .batch_v1 import MetaLangV1, MetaLangV1Batch  # noqa: F401
from .lm_host import FUNCTION_VOCABULARY, LM_LIMITS, RandomLMHost, TaskSamplerV3  # noqa: F401
from .lm_env import MetaLMV3Env, MetaLMV3VecEnv  # noqa: F401
from .stream_host import generate_data_v3_host  # noqa: F401
from .device_sampler import sample_candidates, sample_tasks_device, task_dicts_from_device  # noqa: F401
from .generator_v3 import (generate_data_v3_batch, generate_data_v3_single_task_qa,  # noqa: F401
                           generate_data_v3_single_task_qar, generate_data_v3_single_task_qara, metalang_generator_v3,
                           sample_and_check_task, sample_and_check_tasks)
