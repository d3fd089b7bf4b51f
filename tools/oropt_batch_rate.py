"""The 2-opt + Or-opt descent from many starts: the batched call (Engine.multistart_local_search) next to the per-start
loop (tour_nn + tour_local_search per start, one tour at a time) on the same starts, and the winner next to
multistart_nn_2opt + a polish of its winner.

    python tools/oropt_batch_rate.py [--cases pr1002:64,pr1002:1002,rand4096:64] [--no-loop]

Per case one JSON line:
  batched_ms           wall time of multistart_local_search (after a warm-up on two starts), its winner, totals and the R of
                       the first Or-opt round (tspgpu_info 30) next to the single-tour R (31)
  slots_ms             the same descent through tours_local_search on NN tours already in the slots, which returns the rounds
                       per tour; us_per_tour_sweep = slots_ms / (2-opt sweeps + Or-opt moves + one closing Or-opt sweep per
                       round and tour)
  nn_2opt_polish_*     multistart_nn_2opt + local_search on its winner
  per_start_loop_*     tour_nn + tour_local_search per start, one tour at a time
--no-loop skips the per-start loop; --loop-only runs nothing else (the form that also runs on a tree without the batched calls).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import travellingsalesmanoptimization_amd as T  # noqa: E402
from travellingsalesmanoptimization_amd.tsplib import read as read_tsplib  # noqa: E402
from oropt_rate import reference_points  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="pr1002:64,pr1002:1002,rand4096:64")
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--loop-only", action="store_true")
    args = ap.parse_args()
    cases = [(c.split(":")[0], int(c.split(":")[1])) for c in args.cases.split(",") if c]
    pts = {int(name[4:]): reference_points(int(name[4:])) for name, _ in cases if name.startswith("rand")}
    for name, nstarts in cases:
        xy = pts[int(name[4:])] if name.startswith("rand") else read_tsplib(os.path.join(ROOT, "tests", "golden", "data", name + ".tsp"))[0]
        n = len(xy)
        starts = np.arange(nstarts, dtype=np.int32) * (n // nstarts)
        eng = T.Engine(0)
        eng.set_points(xy)
        eng.build_costs()
        out = {"instance": name, "n": n, "starts": nstarts, "elem": eng.info()["elem"]}
        if not args.loop_only:
            eng.multistart_local_search(starts[:2])               # warm-up (code objects, allocations)
            t0 = time.perf_counter()
            r = eng.multistart_local_search(starts)
            dt = time.perf_counter() - t0
            info = eng.info()
            out.update({"batched_ms": round(dt * 1e3, 3), "cost": r["cost"], "start": r["start"], "two_opt_sweeps": r["two_opt_sweeps"],
                        "or_moves": r["or_moves"], "R": info["or_batch_r"], "single_R": info["or_single_r"]})
            for s in range(min(nstarts, 1024)):
                eng.tour_nn(s, int(starts[s]))
            m = min(nstarts, 1024)
            t0 = time.perf_counter()
            b = eng.tours_local_search(0, m)
            dtb = time.perf_counter() - t0
            sw = int(b["two_opt_sweeps"].sum() + b["or_moves"].sum() + b["rounds"].sum())
            out.update({"slots_ms": round(dtb * 1e3, 3), "rounds_total": int(b["rounds"].sum()), "rounds_max": int(b["rounds"].max()),
                        "us_per_tour_sweep": round(dtb * 1e6 / sw, 3)})
            t0 = time.perf_counter()
            p = eng.multistart_nn_2opt(starts)
            path = p["path"].copy()
            q = eng.local_search(path)
            out.update({"nn_2opt_polish_ms": round((time.perf_counter() - t0) * 1e3, 3), "nn_2opt_cost": p["cost"],
                        "nn_2opt_polish_cost": q["cost"]})
        if not args.no_loop:
            eng.tour_nn(0, int(starts[0]))
            eng.tour_local_search(0)                              # warm-up
            best = None
            t0 = time.perf_counter()
            for s in starts:
                eng.tour_nn(0, int(s))
                eng.tour_local_search(0)
                _, c, _ = eng.tour_store(0, want_path=False)
                if best is None or c < best:
                    best = c
            out.update({"per_start_loop_ms": round((time.perf_counter() - t0) * 1e3, 3), "per_start_loop_cost": best})
        print(json.dumps(out), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
