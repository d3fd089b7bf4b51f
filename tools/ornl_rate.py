#!/usr/bin/env python3
"""Neighbour-list Or-opt on the device next to the existing Or-opt and descent: for n = 4096 and n = 16 384
uniform-random points, fnl4461, d18512 and pla85900, from the NN(0) tour after two_opt_nl (no polish),

  * the mean time of the candidate sweep, compaction and selection (tspgpu_time_or_nl_sweep, K = 5, 8, 12) next to the mean
    time of the existing Or-opt sweep on the same slot (tspgpu_time_or_sweep; absent where that sweep refuses the instance);
  * wall time, sweeps, moves, rounds and final cost of local_search_nl from the NN(0) tour (K = 5, 8, 12) next to
    two_opt_nl + local_search, the existing descent.  Where the existing descent passes --existing-limit (60 s) its row holds
    instead the time of its first 100 Or-opt moves on the two_opt_nl tour.

    python tools/ornl_rate.py [--reps 10] [--time-limit 120] [--step-timeout 900] [--cases n4096,fnl4461] [--out FILE]

The yardstick is the existing descent, not the code under test.  Every case is a GPU step of its own: a child process under its
own time limit, and the first one that fails or runs out of time ends the run (nothing more is started on the device).  Only a
complete run of all cases writes profiles/ornl_rate.txt, with the date; DESIGN 4.15 quotes that file and says "not measured"
while it is absent.
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
from nl2opt_rate import CASES, KS, points  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "ornl_rate.txt")


def step(name, reps, time_limit, existing_limit):
    import travellingsalesmanoptimization_amd as T
    from travellingsalesmanoptimization_amd import TspGpuError
    xy, kind = points(name)
    eng = T.Engine(0)
    eng.set_points(xy, kind)
    eng.build_costs()
    info = eng.info()
    if info["matrix_free"]:
        eng.set_option(T._lib.OPT_OR_MATRIX_FREE, 1)        # (the existing descent's own switch; the new one does not need it)
    row = {"instance": name, "n": len(xy), "matrix_free": info["matrix_free"], "elem": info["elem"], "or_nl_starts": info["or_nl_starts"]}
    start, row["nn_cost"] = eng.nn_tour(0)
    eng.neighbours_build(KS[0])                     # (the first launch loads the code object)
    for K in KS:
        eng.neighbours_build(K)
        tour = start.copy()
        t0 = time.perf_counter()
        d = eng.two_opt_nl(tour, time_left_s=time_limit, polish=False)
        r = {"two_opt_nl_s": round(time.perf_counter() - t0, 4), "two_opt_nl_cost": d["cost"], "two_opt_nl_rc": d["rc"]}
        eng.tour_load(0, tour)
        r["or_nl_sweep_ms"] = round(eng.time_or_nl_sweep(0, reps), 4)
        try:
            r["or_sweep_ms"] = round(eng.time_or_sweep(0, reps), 4)
        except TspGpuError as e:                    # the existing sweep keeps four matrix rows in LDS: it refuses some sizes
            r["or_sweep_refused"] = e.code
        path = start.copy()
        t0 = time.perf_counter()
        d = eng.local_search_nl(path, time_left_s=time_limit)
        r.update({"local_search_nl_s": round(time.perf_counter() - t0, 4), "cost": d["cost"], "rc": d["rc"], "rounds": d["rounds"],
                  "two_opt_sweeps": d["two_opt_sweeps"], "two_opt_moves": d["two_opt_moves"], "or_sweeps": d["or_sweeps"],
                  "or_moves": d["or_moves"], "max_moves_per_sweep": eng.info()["or_nl_max_moves"]})
        # the yardstick: the existing descent from the same two_opt_nl tour
        try:
            path = tour.copy()
            t0 = time.perf_counter()
            e = eng.local_search(path, time_left_s=existing_limit)
            r.update({"existing_s": round(r["two_opt_nl_s"] + time.perf_counter() - t0, 4), "existing_cost": e["cost"], "existing_rc": e["rc"],
                      "existing_or_moves": e["or_moves"], "existing_rounds": e["rounds"]})
            if e["rc"] != 0:                        # past the limit: the time of its first 100 Or-opt moves instead
                eng.tour_load(0, tour)
                t0 = time.perf_counter()
                moves, rc = eng.tour_or_opt(0, max_moves=100)
                r.update({"existing_first_100_or_moves_s": round(time.perf_counter() - t0, 4), "existing_first_moves": moves})
        except TspGpuError as e:
            r["existing_refused"] = e.code
        row["K%d" % K] = r
    eng.close()
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--time-limit", type=float, default=120.0, help="seconds for each new descent (rc 4 once it passes)")
    ap.add_argument("--existing-limit", type=float, default=60.0, help="seconds for the existing descent")
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        step(args.step, args.reps, args.time_limit, args.existing_limit)
        return 0
    cases = [c for c in args.cases.split(",") if c]
    lines = []
    for name in cases:              # one GPU step at a time, each under its own limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name,
               "--reps", str(args.reps), "--time-limit", str(args.time_limit), "--existing-limit", str(args.existing_limit)]
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
        f.write("# tools/ornl_rate.py --reps %d --time-limit %g --existing-limit %g, %s\n"
                % (args.reps, args.time_limit, args.existing_limit, datetime.date.today().isoformat()))
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
