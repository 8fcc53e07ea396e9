"""what the MetaLMV3 task-sampler tests share: the shapes (each the smallest that reaches its path), the seeds, and the host
candidates, computed once"""
import numpy as np

from xenoverse_amd.metalang import sampler_host as sh

# name: ((V, E, H), candidates per launch).  Every H is a multiple of 4: the host follows the device only there.
SHAPES = {
    "min_vocab": ((12, 3, 4), 64),        # minimum vocabulary; E < 8: the plain-loop sum; most candidates rejected
    "default": ((32, 16, 32), 64),        # tables in LDS
    "ragged": ((100, 12, 24), 64),        # E mod 8 != 0: the remainder of the sum; a ragged last column chunk
    "limits": ((256, 64, 128), 16),       # tables through L2, two hidden rows per lane, four column chunks, z beyond LDS
}
NAMES = list(SHAPES)
MAX_LEN = 256
CAND_BASE = 3
# chosen on the host (candidate_host over candidates CAND_BASE ...): accepted and rejected candidates both occur, no draw's
# margin and no argmax's gap is below TAU, and no reward is within 0.03 of a threshold
SEEDS = {"min_vocab": 2, "default": 2, "ragged": 16, "limits": 4}

TAU = 1e-9               # tests/metalm_util.py
PPL_RTOL = 5e-12         # tests/test_gpu_metalm.py; the reward's tolerance is 1e3 PPL_RTOL relative to max(1, |r|)
RTOL, ATOL = 1e-9, 1e-12      # the project's device-sampler tolerance (tests/test_gpu_sampler.py)

_HOST = {}


def host_candidates(name):
    """candidate_host of every candidate of the shape's launch, from the host's own networks"""
    if name not in _HOST:
        (V, E, H), n = SHAPES[name]
        _HOST[name] = [sh.candidate_host(SEEDS[name], CAND_BASE + c, V, E, H, MAX_LEN) for c in range(n)]
    return _HOST[name]


def fake_tables(n, V, E, H, seed=0):
    """a tables dict as sample_tasks_device returns it, on CPU tensors, from the host's candidates 0 .. n - 1 (accepted or
    not)"""
    import torch
    from xenoverse_amd.metalang import FUNCTION_VOCABULARY
    from xenoverse_amd.metalang.lm_host import layer_norm
    arrays = [sh.arrays_from_normals(sh.task_normals(seed, c, sh.n_normals(V, E, H)), V, E, H) for c in range(n)]
    host = dict(emb=[layer_norm(np.ascontiguousarray(a["enc_w"].T)) for a in arrays], w_h_t=[a["rnn_w"].T for a in arrays],
                b_h=[a["rnn_b"] for a in arrays], w_d_t=[a["dec_w"].T for a in arrays], b_d=[a["dec_b"] for a in arrays],
                enc_w=[a["enc_w"] for a in arrays])
    out = {k: torch.from_numpy(np.ascontiguousarray(np.stack(v))) for k, v in host.items()}
    out.update(vocabulary=V, embedding=E, hidden=H, function_vocabulary=dict(FUNCTION_VOCABULARY), max_len=MAX_LEN, seed=seed,
               candidate=torch.arange(n), reward_low=torch.zeros(n, dtype=torch.float64),
               reward_high=torch.full((n,), 2.0, dtype=torch.float64))
    return out, arrays
