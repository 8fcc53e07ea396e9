"""MetaLang on the device: the reference's MetaLangV2 (xenoverse/metalang: random n-gram networks that emit synthetic
pseudo-languages), csrc/metalang.hip, and its MetaLMV3Env (a random recurrent language model that poses queries, answers
them and rewards answers by perplexity), csrc/metalm.hip.  MetaLangV1 and the V3 stream assembler (generator_v3.py) are
not provided."""
from .task_sampler import LIMITS, TaskSamplerV2  # noqa: F401
from .host import MetaLangV2Host  # noqa: F401
from .batch import MetaLangV2, MetaLangV2Batch  # noqa: F401
from .lm_host import FUNCTION_VOCABULARY, LM_LIMITS, RandomLMHost, TaskSamplerV3  # noqa: F401
from .lm_env import MetaLMV3Env, MetaLMV3VecEnv  # noqa: F401
