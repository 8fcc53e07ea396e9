"""The ground-truth cost oracle of a ChemVerse world on the GPU: load a world JSON, ask for the cheapest way to make a qualifying
compound (xenoverse_amd.chemverse.compute_optimal_cost — every candidate route and one-pot charge is one lane of one set of
launches) and print the optimal route and what it costs.

usage: python examples/chemverse_optimal.py [world.json] [min_medicinal_value] [max_toxicity] [min_yield_g]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from xenoverse_amd.chemverse import compute_optimal_cost  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "chemverse_world_b.json")
    med, tox, grams = (float(a) for a in (sys.argv[2:5] + ["3.0", "4.0", "0.5"][len(sys.argv[2:5]):]))
    with open(path) as f:
        world = json.load(f)
    res = compute_optimal_cost(world, min_medicinal_value=med, max_toxicity=tox, min_yield_g=grams)
    print("%s: %s" % (os.path.basename(path), res["message"] if "message" in res else res))
    if not res["found"]:
        return
    detail = res["route_detail"]
    if detail.get("strategy") == "one_pot":
        print("one pot at %.1f C for %.0f s, layer-1 charge %.4f g each" % (detail["temperature_C"], detail["total_time"],
                                                                           detail["m1_scale_g"]))
    for step in detail.get("steps", []):
        print("  %s at %.1f C for %.1f s: %s -> %s (process %.2f, purification %.2f)" % (
            step["reaction_id"], step["temperature_C"], step["duration_s"], step["reactants_g"], step["products_g"],
            step["process_cost"], step["purification_cost"]))
    if "purchase_cost" in detail:
        print("purchase %.4f + process %.4f + purification %.4f = %.4f credits" % (
            detail["purchase_cost"], detail["process_cost"], detail["purification_cost"], detail["total_cost"]))


if __name__ == "__main__":
    main()
