#!/usr/bin/env python3
"""Neighbour-list 3-opt on the device next to the two other list sweeps and the descent without it: for pr1002,
fnl4461, d18512 and pla85900 (matrix-free), at K = 8,

  * on the slot that holds the local optimum of local_search_nl from NN(0): the mean time of the candidate sweep, compaction
    and selection of the 3-opt (tspgpu_time_three_nl_sweep, W = 5 and 8) next to tspgpu_time_nl_sweep and
    tspgpu_time_or_nl_sweep;
  * wall time, counters and final cost of local_search_nl3 (W = 5 and 8) next to local_search_nl, both from NN(0).

    python tools/three_opt_nl_rate.py [--reps 10] [--time-limit 120] [--step-timeout 900] [--cases pr1002,fnl4461] [--out FILE]

No threshold is set on these times: the parent of this family has nothing comparable.  Every case is a GPU step of its own: a
child process under its own time limit, and the first one that fails or runs out of time ends the run (nothing more is started
on the device).  Only a complete run of all cases writes profiles/three_opt_nl_rate.txt, with the date and the repetition
count; DESIGN 4.19 quotes that file and says "not measured" while it is absent.
"""
import argparse
import datetime
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from nl2opt_rate import points  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "three_opt_nl_rate.txt")
CASES = ["pr1002", "fnl4461", "d18512", "pla85900"]
K, WIDTHS = 8, (5, 8)


def step(name, reps, time_limit):
    import travellingsalesmanoptimization_amd as T
    xy, kind = points(name)
    eng = T.Engine(0)
    eng.set_points(xy, kind)
    eng.build_costs()
    info = eng.info()
    row = {"instance": name, "n": len(xy), "K": K, "matrix_free": info["matrix_free"], "elem": info["elem"], "reps": reps,
           "three_nl_nodes": info["three_nl_nodes"]}
    start, row["nn_cost"] = eng.nn_tour(0)
    eng.neighbours_build(K)                         # (the first launch loads the code object)
    path = start.copy()
    t0 = time.perf_counter()
    d = eng.local_search_nl(path, time_left_s=time_limit)
    row["local_search_nl"] = {"s": round(time.perf_counter() - t0, 4), "cost": d["cost"], "rc": d["rc"], "rounds": d["rounds"],
                              "two_opt_sweeps": d["two_opt_sweeps"], "or_sweeps": d["or_sweeps"]}
    eng.tour_load(0, path)
    row["nl_sweep_ms"] = round(eng.time_nl_sweep(0, reps), 4)
    row["or_nl_sweep_ms"] = round(eng.time_or_nl_sweep(0, reps), 4)
    for W in WIDTHS:
        eng.tour_load(0, path)
        r = {"three_nl_sweep_ms": round(eng.time_three_nl_sweep(0, W, reps), 4)}
        tour = start.copy()
        t0 = time.perf_counter()
        d = eng.local_search_nl3(tour, W, time_left_s=time_limit)
        r.update({"local_search_nl3_s": round(time.perf_counter() - t0, 4), "cost": d["cost"], "rc": d["rc"], "rounds": d["rounds"],
                  "two_opt_sweeps": d["two_opt_sweeps"], "or_sweeps": d["or_sweeps"], "three_sweeps": d["three_sweeps"],
                  "three_moves": d["three_moves"], "three_phases": d["three_phases"],
                  "max_moves_per_sweep": eng.info()["three_nl_max_moves"]})
        row["W%d" % W] = r
    eng.close()
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--time-limit", type=float, default=120.0, help="seconds for each descent (rc 4 once it passes)")
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        step(args.step, args.reps, args.time_limit)
        return 0
    cases = [c for c in args.cases.split(",") if c]
    lines = []
    for name in cases:              # one GPU step at a time, each under its own limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name,
               "--reps", str(args.reps), "--time-limit", str(args.time_limit)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            print("%s: exit code %d (124 / 137: no result within %d s); stopping" % (name, r.returncode, args.step_timeout), file=sys.stderr)
            return 1
        lines.append(r.stdout.strip())
    if cases != CASES:
        print("a partial run: %s is not written" % args.out)
        return 0
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/three_opt_nl_rate.py --reps %d --time-limit %g, %s\n" % (args.reps, args.time_limit, datetime.date.today().isoformat()))
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
