"""MetaLMV3 on the device: the recurrence h <- tanh(W_h concat(h, emb) + b_h) is the host's BIT FOR BIT.

The recurrence is chaotic, so a hidden state one ulp off the host's leaves it for good within a few hundred tokens.
csrc/metalm.hip therefore sums a hidden row's dot product in the order of the BLAS matrix-vector product behind numpy's `@`
(four FMA chains over k mod 4, then its tail of (H + E) mod 4 terms) and takes tanh as numpy's float64 loop does.  Here the
hidden state a query leaves — after up to several hundred token steps — is compared with RandomLMHost's with ==, at sizes
with (H + E) mod 4 = 0, 1, 2 and 3 (H a multiple of 4: otherwise the BLAS product has a third order, which is not followed).

The host side of the comparison is numpy's `@` and `np.tanh`: tests/test_host_metalm_order.py states which numpy and BLAS
that takes, and fails on the CPU where they are another."""
import numpy as np
import pytest

from metalm_util import TAU
from util import to_np as _np
from xenoverse_amd.metalang import MetaLMV3VecEnv, RandomLMHost, TaskSamplerV3

pytestmark = pytest.mark.gpu
N_ENV = 8
MAX_LEN = 1024
SIZES = [(32, 16, 32), (64, 16, 64), (128, 32, 64), (256, 64, 128), (40, 13, 20), (40, 10, 20), (48, 7, 24)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "v%d_e%d_h%d" % s)
def test_hidden_state_after_a_query_is_the_hosts(size):
    V, E, H = size
    task = TaskSamplerV3(V, E, H, seed=7000 + V + E + H)
    u = np.random.RandomState([V, E, H]).random_sample((N_ENV, MAX_LEN + 1))
    env = MetaLMV3VecEnv(N_ENV, max_len=MAX_LEN)
    env.set_task(task)
    query, query_len = env.reset(draws=dict(u_query=u))
    cache = _np(env.get_state()["cache"])
    flags = env.check_errors()
    env.close()
    longest = 0
    for e in range(N_ENV):
        lm = RandomLMHost(*task["lm"].arrays().values(), max_len=MAX_LEN)
        want = lm.generate_query(u=u[e])
        assert lm.last["margin"].min() >= TAU      # no draw of the host's is within the band: every token must be equal
        assert [int(t) for t in _np(query)[e, :int(_np(query_len)[e])]] == want
        assert cache[e].tobytes() == lm.hidden_states.tobytes()
        longest = max(longest, len(want))
    print("%s: %d queries, the longest of %d tokens: hidden states equal bit for bit" % (size, N_ENV, longest))
    assert flags == 0
