"""ChemVerse on the device (csrc/chemverse.hip, xenoverse_amd.chemverse.ChemVerseBatch): condition scans of 4,096 and of 65,536
experiments on the medium fixture world (tests/golden/chemverse_world_b.json) — every reaction's own charge (its reactants and
catalysts, with a solvent that lists its non-solvent reactants) over a grid of temperatures, durations (5 - 600 s: 1 - 120
steps), equipment and scales — one launch per call.

Reported per batch size: the kernel's milliseconds between two events on the engine's stream (median of 7 launches after a
warm-up, every launch's figure kept), the whole simulate() call's wall-clock milliseconds (host preparation, uploads, launch,
un-permutation: what a caller sees), experiments/s and simulated steps/s from both.  Against it, on the same box and one CPU
core, over the same 256-experiment sample of the scan: the host restatement's loop (xenoverse_amd.chemverse.host) and, where
the reference is importable (the build container), the reference's own loop.  The sample is drawn with a fixed RandomState; its
mean number of steps run is reported next to the batch's, since an experiment's cost follows its steps.

usage: python scripts/bench_chemverse.py [--quick] [--gpu-only] [--out profiles/chemverse_sim.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WORLD = os.path.join(ROOT, "tests", "golden", "chemverse_world_b.json")
SIZES = (4096, 65536)
SAMPLE = 256
REPS = 7


def scan_experiments(world, n, seed=0):
    """n experiments: reaction charges x a grid of conditions, in a fixed shuffled order"""
    chems, rxns = world["chemicals"], list(world["reactions"].values())
    equip = list(world["equipment"].keys())
    charges = []
    for x in rxns:
        a = {c: 10.0 * k for c, k in x["reactants"]}
        for c in x["catalysts"]:
            a[c] = 1.0
        non_solv = [c for c, _ in x["reactants"] if not chems[c].get("is_solvent")]
        solv = [s for s, c in chems.items() if c.get("is_solvent") and all(s in chems[q].get("solubility", {}) for q in non_solv)]
        if solv and solv[0] not in a:
            a[solv[0]] = 40.0
        charges.append(a)
    rs = np.random.RandomState(seed)
    temps = np.linspace(0.0, 250.0, 26)
    durs = np.array([5.0, 30.0, 60.0, 150.0, 300.0, 600.0])
    scales = np.array([0.5, 1.0, 2.0, 4.0])
    pick = lambda m: rs.randint(0, m, n)      # noqa: E731
    ic, it, idur, ie, isc = pick(len(charges)), pick(len(temps)), pick(len(durs)), pick(len(equip)), pick(len(scales))
    amounts = [{c: g * scales[s] for c, g in charges[k].items()} for k, s in zip(ic, isc)]
    return dict(amounts=amounts, temperature_C=temps[it], pressure_atm=np.where(np.array(equip)[ie] == "open_beaker", 0.5, 1.0),
                duration_s=durs[idur], equipment=[equip[e] for e in ie])


def cpu_lines(world, sample):
    from xenoverse_amd.chemverse import build_tables, prepare_experiments, simulate_chain_host
    tab = build_tables(world)
    x = prepare_experiments([tab], 0, sample["amounts"], sample["temperature_C"], sample["pressure_atm"], sample["duration_s"],
                            sample["equipment"])
    exps = [dict(amounts=[(int(c), float(x["grams"][i, c])) for c in x["order"][i, :x["n_initial"][i]]],
                 temperature_C=float(x["T"][i]), pressure_atm=float(x["P"][i]), duration_s=float(x["duration"][i]),
                 equipment=int(x["equipment"][i])) for i in range(x["n"])]
    t0 = time.perf_counter()
    res = simulate_chain_host(tab, exps, record="none")
    host_s = time.perf_counter() - t0
    out = {"sample": len(exps), "sample_mean_steps_run": float(res["steps_run"].mean()),
           "host_loop_seconds": host_s, "host_loop_experiments_per_s": len(exps) / host_s,
           "host_loop_ms_per_experiment": 1e3 * host_s / len(exps)}
    print("host restatement, one core: %.2f ms per experiment (%d experiments, %.1f steps run on average)"
          % (out["host_loop_ms_per_experiment"], len(exps), out["sample_mean_steps_run"]), flush=True)
    try:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import _refimport
        _refimport.setup()
        from xenoverse.chemverse.environment.simulator import simulate_chain_reaction
        from xenoverse.chemverse.world_gen.models import World
    except Exception as ex:
        out["reference_loop"] = "not importable here (%s)" % type(ex).__name__
        return out
    w = World.from_dict(world)
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        for i in range(len(exps)):
            simulate_chain_reaction(w, dict(sample["amounts"][i]), float(sample["temperature_C"][i]),
                                    float(sample["pressure_atm"][i]), float(sample["duration_s"][i]),
                                    equipment=sample["equipment"][i])
    ref_s = time.perf_counter() - t0
    out.update({"reference_loop_seconds": ref_s, "reference_loop_experiments_per_s": len(exps) / ref_s,
                "reference_loop_ms_per_experiment": 1e3 * ref_s / len(exps)})
    print("reference, one core: %.2f ms per experiment" % out["reference_loop_ms_per_experiment"], flush=True)
    return out


def gpu_lines(world, sizes, reps):
    import torch
    from xenoverse_amd.chemverse import ChemVerseBatch
    from xenoverse_amd.build import source_hash
    res = {"device": torch.cuda.get_device_name(0), "kernel_source_hash": source_hash(["chemverse.hip"]), "repeats": reps}
    batch = ChemVerseBatch([world], max(sizes))
    batch.time_kernel = True
    for n in sizes:
        x = scan_experiments(world, n)
        args = dict(world_index=0, **x)
        out = batch.simulate(**args)      # warm-up: code object, allocator blocks
        steps = float(out["steps_run"].double().mean().item())
        fired = float((out["fired"].sum(dim=1) > 0).double().mean().item())
        del out
        kernel_ms, call_ms = [], []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = batch.simulate(**args)
            torch.cuda.synchronize()
            call_ms.append(1e3 * (time.perf_counter() - t0))
            kernel_ms.append(batch.last_kernel_ms)
            del out
        k, c = statistics.median(kernel_ms), statistics.median(call_ms)
        res["n%d" % n] = {"experiments": n, "mean_steps_run": steps, "share_fired": fired, "kernel_ms": kernel_ms,
                          "call_ms": call_ms, "kernel_ms_median": k, "call_ms_median": c,
                          "kernel_experiments_per_s": n / (k * 1e-3), "kernel_steps_per_s": n * steps / (k * 1e-3),
                          "call_experiments_per_s": n / (c * 1e-3)}
        print("n = %d: kernel %.3f ms (%.3e experiments/s, %.3e steps/s), whole call %.1f ms; %.1f steps run on average, "
              "%.0f %% fired" % (n, k, n / (k * 1e-3), n * steps / (k * 1e-3), c, steps, 100 * fired), flush=True)
    res["device_errors"] = int(batch.check_errors())
    batch.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--gpu-only", action="store_true")
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    with open(WORLD) as f:
        world = json.load(f)
    sizes = (4096,) if args.quick else SIZES
    res = {"world": os.path.basename(WORLD), "chemicals": len(world["chemicals"]), "reactions": len(world["reactions"])}
    if not args.gpu_only:
        big = scan_experiments(world, max(sizes))
        idx = np.random.RandomState(1).choice(max(sizes), 32 if args.quick else SAMPLE, replace=False)
        sample = {k: [v[i] for i in idx] for k, v in big.items()}
        res.update(cpu_lines(world, sample))
    if not args.cpu_only:
        res.update(gpu_lines(world, sizes, 3 if args.quick else REPS))
        top = res.get("n%d" % max(sizes))
        if top and "host_loop_experiments_per_s" in res:
            res["kernel_vs_host_loop"] = top["kernel_experiments_per_s"] / res["host_loop_experiments_per_s"]
            res["call_vs_host_loop"] = top["call_experiments_per_s"] / res["host_loop_experiments_per_s"]
        if top and "reference_loop_experiments_per_s" in res:
            res["kernel_vs_reference_loop"] = top["kernel_experiments_per_s"] / res["reference_loop_experiments_per_s"]
            res["call_vs_reference_loop"] = top["call_experiments_per_s"] / res["reference_loop_experiments_per_s"]
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
