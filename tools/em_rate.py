"""Extra Mileage on the device: wall time of the farthest pair and of the construction, stale rescans per insertion,
and which form ran (1 one launch, 2 one launch pair per step), per instance and form.

    python tools/em_rate.py [--forms 1,2] [--instances pr1002,fnl4461,rand16384,pla85900]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import travellingsalesmanoptimization_amd as T  # noqa: E402
from travellingsalesmanoptimization_amd.tsplib import read as read_tsplib  # noqa: E402


def points(name):
    """-> (xy, edge-weight kind): randNNN = NNN uniform integer points (EUC_2D), else a TSPLIB file of tests/golden/data"""
    if name.startswith("rand"):
        import numpy as np
        rng = np.random.default_rng(123)
        return rng.integers(0, 10000, size=(int(name[4:]), 2)).astype("float64"), T.EUC_2D
    xy, kind = read_tsplib(os.path.join(ROOT, "tests", "golden", "data", name + ".tsp"))
    return xy, {"EUC_2D": T.EUC_2D, "ATT": T.ATT, "CEIL_2D": T.CEIL_2D}.get(kind, kind)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forms", default="1,2")
    ap.add_argument("--instances", default="pr1002,fnl4461,rand16384,pla85900")
    ap.add_argument("--per-step-max-n", type=int, default=1 << 20, help="skip the per-step form above this n")
    args = ap.parse_args()
    for name in args.instances.split(","):
        xy, kind = points(name)
        for form in [int(f) for f in args.forms.split(",")]:
            if form == 2 and len(xy) > args.per_step_max_n:
                continue
            eng = T.Engine(0)
            eng.set_option(T.OPT_EM_FORM, form)
            eng.set_points(xy, kind)
            eng.build_costs()
            eng.extra_mileage(0, 1)                       # warm-up (code objects, allocations)
            t0 = time.perf_counter()
            a, b, _ = eng.farthest_pair()
            t1 = time.perf_counter()
            succ, cost, rc = eng.extra_mileage(a, b)
            t2 = time.perf_counter()
            info = eng.info()
            print(json.dumps({"instance": name, "n": len(xy), "kind": kind, "matrix_free": info["matrix_free"], "elem": info["elem"],
                              "form": info["em_form"], "farthest_ms": round((t1 - t0) * 1e3, 3),
                              "construction_ms": round((t2 - t1) * 1e3, 3), "cost": cost, "rc": rc,
                              "stale_per_step": round(info["em_stale"] / max(1, info["em_steps"]), 2)}), flush=True)
            eng.close()


if __name__ == "__main__":
    main()
