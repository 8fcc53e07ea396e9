"""Scan one synthesis route's conditions on the GPU: load a ChemVerse world JSON, take one reaction's charge, run the grid
temperature x duration x equipment x scale as ONE batch (xenoverse_amd.chemverse.scan) and print the best yield.

usage: python examples/chemverse_scan.py [world.json] [reaction id]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from xenoverse_amd.chemverse import build_tables, scan  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "chemverse_world_b.json")
    with open(path) as f:
        world = json.load(f)
    tab = build_tables(world)
    rid = sys.argv[2] if len(sys.argv) > 2 else tab["rxn_ids"][0]
    rxn = world["reactions"][rid]
    chems = world["chemicals"]
    charge = {c: 10.0 * k for c, k in rxn["reactants"]}
    for c in rxn["catalysts"]:
        charge[c] = 1.0
    non_solvent = [c for c, _ in rxn["reactants"] if not chems[c].get("is_solvent")]
    solvents = [s for s, c in chems.items() if c.get("is_solvent") and all(s in chems[q].get("solubility", {}) for q in non_solvent)]
    if solvents and solvents[0] not in charge:
        charge[solvents[0]] = 40.0
    temperatures = np.linspace(0.0, 250.0, 26)
    durations = (30.0, 60.0, 150.0, 300.0, 600.0)
    equipment = [e for e in tab["equip_names"] if e != "open_beaker"]
    scales = (0.5, 1.0, 2.0)
    res = scan(world, charge, temperatures, durations, equipment, scales)
    product = tab["chem_ids"].index(rxn["products"][0][0])
    grams = res["final_pool"][..., product].cpu().numpy()      # [temperature, duration, equipment, scale]
    per_scale = grams / np.array(scales)
    failed = res["failure"].cpu().numpy() != 0
    per_scale[failed] = -1.0
    it, idur, ie, isc = np.unravel_index(int(np.argmax(per_scale)), per_scale.shape)
    print("%s, reaction %s: %d experiments in one launch, %d destroyed their batch" % (
        os.path.basename(path), rid, per_scale.size, int(failed.sum())))
    print("best: %.3f g of %s per unit charge at %.0f C, %.0f s, %s, scale %.1f (final %.1f C, %.3f atm)" % (
        per_scale[it, idur, ie, isc], rxn["products"][0][0], temperatures[it], durations[idur], equipment[ie], scales[isc],
        float(res["final_T"][it, idur, ie, isc]), float(res["final_P"][it, idur, ie, isc])))


if __name__ == "__main__":
    main()
