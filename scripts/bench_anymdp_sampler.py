"""AnyMDP task sampler (`xv_anymdp_sample_tasks`): candidates per second and SHA-256 digests of what it writes, for one
tree, and the comparison of two trees' runs.  The digests pin the bits of a tree against another's (a refactor's parent);
the rates are the sampler's throughput record.

Measure (one process, one tree):
    python scripts/bench_anymdp_sampler.py [--tree <built checkout>] [--samples 5] [--no-digests] --out run.json
    (--batches-from run.json: a tree from before `device_sampler.launch_batch` launches the batches of that run)
  * digests, per shape of tests/test_gpu_sampler.py::test_candidates_equal_the_oracle at that test's seed, base and
    candidate count: `status`, the info records' bytes, the dense tensors whole, and the table tensors gathered at the
    ACCEPTED candidates (the slots of the others are never written);
  * rates at 16x4, 64x8, 128x5 and 256x5, tables only (what `sample_tasks_device` launches): a shape is warmed up with two
    launches, the second of which is timed to choose the launch count; a sample is that many launches of `batch`
    candidates each — `device_sampler.launch_batch`, so as few launches as memory allows — covering at
    least `--seconds` of device work, behind one device synchronise.  Every sample draws the same candidates.
    Clock: time.perf_counter.
Compare (no GPU):
    python scripts/bench_anymdp_sampler.py --merge parent_1.json new_1.json parent_2.json ... --out ab.json
  runs are told apart by their `label` and given in the order they ran; all samples are kept.  Pass: the sides alternate
  (each consecutive pair of runs holds both), every digest equal, and per shape at least five samples a side and the new
  median rate not below the parent's median by more than the parent's own max - min spread.  Exit status 1 otherwise.
"""
import argparse
import hashlib
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DIGEST_CASES = [(16, 4, 192), (8, 2, 64), (24, 5, 48), (32, 8, 40), (64, 8, 24), (64, 5, 16), (40, 12, 12), (96, 4, 10),
                (128, 5, 8), (256, 5, 4), (64, 12, 8), (200, 20, 3), (72, 32, 4), (65, 8, 6)]
TIMING_SHAPES = [(16, 4), (64, 8), (128, 5), (256, 5)]
TABLES = ("rows", "state_map", "term_mask", "s0_cdf", "s0_ids", "max_steps")
DENSE = ("transition", "reward", "reward_noise")


def _sha(t):
    import numpy as np
    a = t if isinstance(t, np.ndarray) else t.detach().cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digests(ds, eng):
    out = {}
    for S, A, n in DIGEST_CASES:
        r = ds.sample_candidates(eng, 20251003 + S, 1000, n, S, A, s0_max=4, tables=True, dense=True, info=True)
        eng.sync()
        acc = (r["status"] == 0).nonzero().flatten()
        d = dict(status=_sha(r["status"]), info=_sha(r["info"]), accepted=int(acc.numel()))
        d.update({k: _sha(r[k]) for k in DENSE})
        d.update({k: _sha(r[k][acc]) for k in TABLES})
        out["%dx%d" % (S, A)] = d
    return out


def rates(ds, eng, samples, seconds, batches=None):
    import torch
    out = {}
    for S, A in TIMING_SHAPES:
        batch = batches["%dx%d" % (S, A)] if batches else ds.launch_batch(S, A)

        def run(launches):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(launches):
                st = ds.sample_candidates(eng, 7, i * batch, batch, S, A, tables=True)["status"]
            torch.cuda.synchronize()
            return time.perf_counter() - t0, int((st == 0).sum())

        run(1)
        t1, _ = run(1)
        launches = max(1, math.ceil(1.2 * seconds / t1))
        got = [run(launches) for _ in range(samples)]
        out["%dx%d" % (S, A)] = dict(batch=batch, launches=launches, warmup_launch_s=t1, accepted_in_last_launch=got[-1][1],
                                     sample_s=[t for t, _ in got], candidates_per_s=[launches * batch / t for t, _ in got])
        print("%dx%d" % (S, A), json.dumps(out["%dx%d" % (S, A)]), flush=True)
    return out


def merge(paths, out_path):
    runs = [json.load(open(p)) for p in paths]
    sides = {}
    for r in runs:
        sides.setdefault(r["label"], []).append(r)
    if sorted(sides) != ["new", "parent"]:
        raise SystemExit("--merge needs runs labelled `parent` and `new`, got %s" % sorted(sides))
    out = dict(device=runs[0]["device"], clock=runs[0]["clock"], order=[r["label"] for r in runs], digests={}, rates={})
    ok = all(set(out["order"][i:i + 2]) == {"parent", "new"} for i in range(0, len(runs), 2))
    out["alternating"] = ok
    for label, rs in sides.items():
        ds_ = [r["digests"] for r in rs if r.get("digests")]
        if not ds_ or any(d != ds_[0] for d in ds_):
            raise SystemExit("side %s: no digests, or digests that differ between its own runs" % label)
        out["digests"][label] = ds_[0]
    out["digests"]["equal"] = out["digests"]["parent"] == out["digests"]["new"]
    ok &= out["digests"]["equal"]
    for S, A in TIMING_SHAPES:
        k = "%dx%d" % (S, A)
        e = {label: dict(batch=rs[0]["rates"][k]["batch"], launches=[r["rates"][k]["launches"] for r in rs],
                         sample_s=sum((r["rates"][k]["sample_s"] for r in rs), []),
                         candidates_per_s=sum((r["rates"][k]["candidates_per_s"] for r in rs), []))
             for label, rs in sides.items()}
        for v in e.values():
            v["median"] = statistics.median(v["candidates_per_s"])
        p = e["parent"]["candidates_per_s"]
        e["parent_spread"] = max(p) - min(p)
        e["pass"] = (min(len(v["candidates_per_s"]) for v in (e["parent"], e["new"])) >= 5
                     and e["new"]["median"] >= e["parent"]["median"] - e["parent_spread"])
        ok &= e["pass"]
        out["rates"][k] = e
        print(k, "parent %.4g new %.4g candidates/s, parent spread %.3g, %s" % (
            e["parent"]["median"], e["new"]["median"], e["parent_spread"], "pass" if e["pass"] else "FAIL"))
    out["pass"] = bool(ok)
    print("digests", "equal" if out["digests"]["equal"] else "DIFFER", "| runs", "alternate" if out["alternating"] else "DO NOT ALTERNATE")
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="the built checkout to measure (default: this one)")
    ap.add_argument("--label", default="new")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--no-digests", action="store_true")
    ap.add_argument("--batches-from", help="a run's record: launch its batches")
    ap.add_argument("--merge", nargs="+")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anymdp_sampler.json"))
    a = ap.parse_args()
    if a.merge:
        sys.exit(merge(a.merge, a.out))
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_anymdp_sampler.py measures on the GPU; none found")
    from xenoverse_amd.anymdp import device_sampler as ds
    from xenoverse_amd.engine import Engine
    eng = Engine("cuda:0")
    out = dict(label=a.label, device=torch.cuda.get_device_name(0),
               clock="time.perf_counter around launches behind a device synchronise")
    if not a.no_digests:
        out["digests"] = digests(ds, eng)
    batches = a.batches_from and {k: v["batch"] for k, v in json.load(open(a.batches_from))["rates"].items()}
    out["rates"] = rates(ds, eng, a.samples, a.seconds, batches)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
