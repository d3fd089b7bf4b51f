#!/usr/bin/env python3
"""Matrix-free Or-opt on the device (TSPGPU_OPT_OR_MATRIX_FREE = 1, k_oropt_sweep_otf): the sweep kernel alone in both
forms -- hook 90 = 2, every candidate evaluated, and 1, the exact early-out -- on pla85900 and on 85 900 uniform-random
integer points, CEIL_2D and EUC_2D each: us per sweep (HIP events, after a warm-up) and candidates per second, on the
NN(0) tour and on its 2-opt optimum (where the early-out has something to skip); then the wall time of local_search from
NN(0), its moves, rounds and gain over two_opt.

    python tools/oropt_otf_rate.py [--reps 20] [--time-limit 300] [--step-timeout 900] [--no-descent]

Every case is a GPU step of its own: a child process under its own time limit, and the first one that fails or runs out
of time ends the run (nothing more is started on the device).  Only a complete run writes profiles/oropt_otf_rate.txt,
with the date; DESIGN 4.12 quotes that file.  Candidates of one sweep: n (5 n - 16).
"""
import argparse
import datetime
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "oropt_otf_rate.txt")
CASES = [("pla85900", "CEIL_2D"), ("pla85900", "EUC_2D"), ("random85900", "CEIL_2D"), ("random85900", "EUC_2D")]


def points(name):
    if name == "random85900":
        return np.random.default_rng(85900).integers(0, 1000000, (85900, 2)).astype(np.float64)
    from travellingsalesmanoptimization_amd.tsplib import read as read_tsplib
    return np.asarray(read_tsplib(os.path.join(ROOT, "tests", "golden", "data", name + ".tsp"))[0], dtype=np.float64)


def step(name, kind, reps, time_limit, descent):
    import travellingsalesmanoptimization_amd as T
    xy = points(name)
    n = len(xy)
    eng = T.Engine(0)
    eng.set_option(T.OPT_MATRIX_FREE, 1)
    eng.set_option(T._lib.OPT_OR_MATRIX_FREE, 1)
    eng.set_points(xy, getattr(T, kind))
    eng.build_costs()
    cand = n * (5 * n - 16)
    row = {"instance": name, "kind": kind, "n": n, "ceil_int": eng.info()["ceil_int"]}
    eng.tour_nn(0, 0)
    for tour in ("nn", "two_opt"):
        if tour == "two_opt":
            if not descent:
                break
            t0 = time.perf_counter()
            sweeps, rc = eng.tour_two_opt(0, time_left_s=time_limit)
            row["two_opt_s"], row["two_opt_sweeps"], row["two_opt_rc"] = round(time.perf_counter() - t0, 3), sweeps, rc
            row["two_opt_cost"] = eng.tour_store(0, want_path=False)[1]
        for form, label in ((2, "full"), (1, "early")):
            eng.set_option(90, form)
            us = eng.time_or_sweep(0, reps) * 1e3
            assert eng.info()["or_otf"] == (1 if form == 2 else 2)
            row["%s_%s_us" % (tour, label)] = round(us, 1)
            row["%s_%s_gcand_per_s" % (tour, label)] = round(cand / us / 1e3, 2)
    row["R"] = eng.info()["or_otf_R"]
    if descent:
        eng.set_option(90, 0)
        path, _ = eng.nn_tour(0)
        t0 = time.perf_counter()
        got = eng.local_search(path, time_left_s=time_limit)
        row["local_search_s"] = round(time.perf_counter() - t0, 3)
        row.update({"local_search_" + k: v for k, v in got.items()})
        row["gain_over_two_opt"] = row["two_opt_cost"] - got["cost"]
    eng.close()
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--time-limit", type=float, default=300.0, help="seconds for each descent (rc 4 once it passes)")
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--no-descent", action="store_true")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        name, kind = args.step.split(":")
        step(name, kind, args.reps, args.time_limit, not args.no_descent)
        return 0
    lines = []
    for name, kind in CASES:        # one GPU step at a time, each under its own limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--step", "%s:%s" % (name, kind), "--reps", str(args.reps),
               "--time-limit", str(args.time_limit)] + (["--no-descent"] if args.no_descent else [])
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            print("%s %s: no result within %d s; stopping" % (name, kind, args.step_timeout), file=sys.stderr)
            return 1
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            print("%s %s: exit code %d; stopping" % (name, kind, r.returncode), file=sys.stderr)
            return 1
        lines.append(r.stdout.strip())
    with open(OUT, "w") as f:
        f.write("# tools/oropt_otf_rate.py %s, %s\n" % (" ".join(sys.argv[1:]), datetime.date.today().isoformat()))
        f.write("\n".join(lines) + "\n")
    print("wrote", OUT)
    return 0


if __name__ == "__main__":
    sys.exit(main())
