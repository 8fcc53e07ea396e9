"""Record the numpy restatement of the device maze sampler (mazeworld/sampler_host.py) over the two 256-candidate batches
whose restatement is too slow for a test (the default n_range: ~15 s; n = 63: minutes): info records in full, the slots
as SHA-256 digests -> tests/golden/sampler_maze_host_{default,n63}.npz.  tests/test_host_maze_sampler.py makes a few of
the recorded candidates again; tests/test_gpu_maze_sampler.py compares the device with all of them.

usage: python scripts/gen_golden_maze_sampler.py [--jobs 8]
"""
import argparse
import os
import sys
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xenoverse_amd.mazeworld import sampler_host as sh  # noqa: E402

CASES = {"default": dict(seed=21, n_range=(9, 25)), "n63": dict(seed=22, n_range=(63, 64))}
N_CAND = 256


def one(args):
    name, q = args
    c = CASES[name]
    s = sh.sample_slots_host(c["seed"], q, 1, n_range=c["n_range"])
    return np.frombuffer(s["info"].tobytes(), np.int32).copy(), sh.slots_digest(s, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    with Pool(a.jobs) as pool:
        for name, c in CASES.items():
            rows = pool.map(one, [(name, q) for q in range(N_CAND)], chunksize=4)
            path = os.path.join(ROOT, "tests", "golden", "sampler_maze_host_%s.npz" % name)
            np.savez_compressed(path, seed=np.int64(c["seed"]), n_range=np.array(c["n_range"], np.int64),
                                info_words=np.stack([r[0] for r in rows]), digest=np.stack([r[1] for r in rows]))
            print("wrote", path)


if __name__ == "__main__":
    main()
