"""MetaLang on the device: the reference's MetaLangV2 (xenoverse/metalang: random n-gram networks that emit synthetic
pseudo-languages), csrc/metalang.hip.  MetaLangV1 and MetaLMV3Env are not provided."""
from .task_sampler import LIMITS, TaskSamplerV2  # noqa: F401
from .host import MetaLangV2Host  # noqa: F401
from .batch import MetaLangV2, MetaLangV2Batch  # noqa: F401
