#!/usr/bin/env python3
"""Neighbour-list 2-opt on the device (tspgpu_two_opt_nl) next to the one-move and the parallel-move descent: for
n = 4096 and n = 16 384 uniform-random points, fnl4461, d18512 and pla85900, from the same NN(0) tour, the list build time
(K = 5, 8, 12), the sweeps, moves, wall time and final cost of two_opt_nl without and with the polish, the same of two_opt and
two_opt_multi, and the mean time of the candidate sweep plus selection (tspgpu_time_nl_sweep: HIP events, after a warm-up,
nothing applied).

    python tools/nl2opt_rate.py [--reps 10] [--time-limit 120] [--step-timeout 900] [--cases n4096,fnl4461] [--out FILE]

Every case is a GPU step of its own: a child process under its own time limit, and the first one that fails or runs out of
time ends the run (nothing more is started on the device).  Only a complete run of all cases writes
profiles/nl2opt_rate.txt, with the date; DESIGN 4.14 quotes that file and says "not measured" while it is absent.  A descent
that passes --time-limit returns rc 4 with the tour it has: its row says so.
"""
import argparse
import ctypes
import datetime
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "nl2opt_rate.txt")
CASES = ["n4096", "n16384", "fnl4461", "d18512", "pla85900"]
KS = (5, 8, 12)


def reference_points(n, seed=123):
    """the reference's generator (src/tsp.c:468-476): the point sets of bench.py; drawn before the first GPU call"""
    libc = ctypes.CDLL(None)
    libc.srand(ctypes.c_uint(seed))
    xy = np.empty((n, 2), dtype=np.float64)
    for i in range(n):
        xy[i, 0] = (libc.rand() / 2147483647) * 10000 + (-5000)
        xy[i, 1] = (libc.rand() / 2147483647) * 10000 + (-5000)
    return xy


def points(name):
    if name.startswith("n") and name[1:].isdigit():
        return reference_points(int(name[1:])), 0
    from travellingsalesmanoptimization_amd.tsplib import read as read_tsplib
    xy, kind = read_tsplib(os.path.join(ROOT, "tests", "golden", "data", name + ".tsp"))
    return np.asarray(xy, dtype=np.float64), kind


def step(name, reps, time_limit):
    import travellingsalesmanoptimization_amd as T
    xy, kind = points(name)
    eng = T.Engine(0)
    eng.set_points(xy, kind)
    eng.build_costs()
    info = eng.info()
    row = {"instance": name, "n": len(xy), "matrix_free": info["matrix_free"], "elem": info["elem"], "nl_nodes": info["nl_nodes"]}
    start, row["nn_cost"] = eng.nn_tour(0)
    eng.neighbours_build(KS[0])                     # (the first launch loads the code object)
    for K in KS:
        t0 = time.perf_counter()
        eng.neighbours_build(K)                     # returns behind a stream synchronise
        r = {"build_ms": round(1e3 * (time.perf_counter() - t0), 3)}
        eng.tour_load(0, start)
        r["sweep_ms"] = round(eng.time_nl_sweep(0, reps), 4)
        for polish in (False, True):
            path = start.copy()
            t0 = time.perf_counter()
            d = eng.two_opt_nl(path, time_left_s=time_limit, polish=polish)
            tag = "polished" if polish else "nl"
            r.update({tag + "_s": round(time.perf_counter() - t0, 4), tag + "_cost": d["cost"], tag + "_rc": d["rc"]})
            if polish:
                r.update({"polish_sweeps": d["polish_sweeps"], "polish_moves": d["polish_moves"]})
            else:
                r.update({"nl_sweeps": d["sweeps"], "nl_moves": d["moves"]})
        row["K%d" % K] = r
    path = start.copy()
    t0 = time.perf_counter()
    cost, sweeps, moves, rc = eng.two_opt_multi(path, time_left_s=time_limit)
    row.update({"multi_s": round(time.perf_counter() - t0, 3), "multi_sweeps": sweeps, "multi_moves": moves, "multi_cost": cost, "multi_rc": rc})
    path = start.copy()
    t0 = time.perf_counter()
    cost, sweeps, rc = eng.two_opt(path, time_left_s=time_limit)
    row.update({"two_opt_s": round(time.perf_counter() - t0, 3), "two_opt_sweeps": sweeps, "two_opt_cost": cost, "two_opt_rc": rc})
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
        f.write("# tools/nl2opt_rate.py --reps %d --time-limit %g, %s\n" % (args.reps, args.time_limit, datetime.date.today().isoformat()))
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
