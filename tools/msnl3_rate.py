#!/usr/bin/env python3
"""The batched neighbour-list descent with a 3-opt phase on the device next to what exists: wall time, total
sweeps and best cost for pr1002 (all 1002 starts), fnl4461 (512 starts), d18512 (64 starts, matrix mode) and pla85900 (16
starts, matrix-free), at K = W = 8, of

  (a) multistart_local_search_nl3, the batch;
  (b) the same starts one slot after the other in the same process, tour_nn + tour_local_search_nl3: what the single-tour entry
      points offer for a multi-start.  This is the yardstick; (a) and (b) must report the same sweeps and the same best cost;
  (c) multistart_local_search_nl on the same starts: the batch without the phase, for the cost and the time the phase adds;

and, with --vns, pr1002 from the All-NN tour, 64 walks of 20 iterations: vns_walks_nl against vns_walks_nl3, time and best
incumbent.

    python tools/msnl3_rate.py [--reps 5] [--step-timeout 900] [--cases pr1002,fnl4461] [--vns] [--out FILE]

Every call returns behind a synchronisation of the engine's stream, so the wall times are bounded by the device's work.  One
warm call of each path comes first (code object load, allocations); then --reps timed repetitions of each, all of them reported
(`*_s`: the list, `*_med_s`: its median).  Every case is a GPU step of its own: a child process under its own time limit, and
the first one that fails or runs out of time ends the run.  Only a complete run of all cases with --vns writes the output file
(default profiles/msnl3_rate.txt), with the date; a partial run prints its rows only.
"""
import argparse
import datetime
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from nl2opt_rate import points  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "msnl3_rate.txt")
CASES = {"pr1002": 1002, "fnl4461": 512, "d18512": 64, "pla85900": 16}     # instance -> starts
K = W = 8
SWEEPS = ("two_opt_sweeps", "or_sweeps", "three_sweeps")


def timed(reps, fn):
    out, last = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        last = fn()
        out.append(round(time.perf_counter() - t0, 4))
    return out, last


def engine(name):
    import travellingsalesmanoptimization_amd as T
    xy, kind = points(name)
    eng = T.Engine(0)
    if name == "pla85900":
        eng.set_option(T.OPT_MATRIX_FREE, 1)
    eng.set_points(xy, kind)
    eng.build_costs()
    eng.neighbours_build(K)
    return T, eng, xy


def step(name, reps):
    nstarts = CASES[name]
    starts = list(range(nstarts))
    T, eng, xy = engine(name)
    eng.set_option(T.OPT_MAX_TOURS, max(1024, nstarts))
    info = eng.info()
    row = {"instance": name, "n": len(xy), "starts": nstarts, "K": K, "W": W, "matrix_free": info["matrix_free"], "elem": info["elem"],
           "reps": reps}

    def one_by_one():
        tot, best = 0, None
        for s in starts:
            eng.tour_nn(0, s)
            r = eng.tour_local_search_nl3(0, W)
            tot += sum(r[k] for k in SWEEPS)
            cost = eng.tour_store(0, want_path=False)[1]
            best = cost if best is None or cost < best else best
        return tot, best

    eng.multistart_local_search_nl3(W, starts[:2])          # warm: every path once
    eng.multistart_local_search_nl(starts[:2])
    eng.tour_nn(0, 0)
    eng.tour_local_search_nl3(0, W)
    ta, a = timed(reps, lambda: eng.multistart_local_search_nl3(W, starts))
    i = eng.info()
    tc, c = timed(reps, lambda: eng.multistart_local_search_nl(starts))
    tb, b = timed(reps, one_by_one)
    row.update({"batch_s": ta, "batch_med_s": statistics.median(ta), "batch_sweeps": sum(a[k] for k in SWEEPS),
                "batch_three_sweeps": a["three_sweeps"], "batch_three_moves": a["three_moves"], "batch_cost": a["cost"],
                "batch_start": a["start"], "batch_rc": a["rc"], "batch_launches": i["nl_batch_launches"],
                "batch_three_max_moves": i["nl3_batch_max_moves"],
                "one_by_one_s": tb, "one_by_one_med_s": statistics.median(tb), "one_by_one_sweeps": b[0], "one_by_one_cost": b[1],
                "speedup_med_over_med": round(statistics.median(tb) / statistics.median(ta), 2),
                "same_sweeps_and_cost": sum(a[k] for k in SWEEPS) == b[0] and a["cost"] == b[1],
                "two_phase_s": tc, "two_phase_med_s": statistics.median(tc), "two_phase_cost": c["cost"],
                "two_phase_sweeps": c["two_opt_sweeps"] + c["or_sweeps"],
                "phase_time_ratio": round(statistics.median(ta) / statistics.median(tc), 3)})
    eng.close()
    print(json.dumps(row), flush=True)


def step_vns(reps, walks=64, k=20):
    T, eng, xy = engine("pr1002")
    start, cost0, _ = eng.nn_all()
    rng = np.random.default_rng(1)
    rv = rng.integers(0, 2 ** 31 - 1, (walks, 64 * k + 4096)).astype(np.int32)

    def run(width):
        paths = np.ascontiguousarray(np.tile(start, (walks, 1)), np.int32)
        bests, bc = paths.copy(), np.full(walks, float(cost0))
        r = eng.vns_walks_nl3(paths, k, rv, bests, bc, width) if width else eng.vns_walks_nl(paths, k, rv, bests, bc)
        return r["rc"], float(bc.min()), {t: int(v.sum()) for t, v in r["totals"].items()}

    row = {"instance": "pr1002", "walks": walks, "iterations": k, "K": K, "W": W, "start_cost": float(cost0), "reps": reps}
    for name, width in (("walks_nl", 0), ("walks_nl3", W)):
        run(width)
        t, (rc, best, totals) = timed(reps, lambda: run(width))
        row[name] = {"s": t, "med_s": statistics.median(t), "rc": rc, "best": best, "totals": totals}
    eng.close()
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--vns", action="store_true")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        step_vns(args.reps) if args.step == "vns" else step(args.step, args.reps)
        return 0
    cases = [c for c in args.cases.split(",") if c]
    steps = cases + (["vns"] if args.vns else [])
    lines = []
    for name in steps:              # one GPU step at a time, each under its own limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            print("%s: exit code %d (124 / 137: no result within %d s); stopping" % (name, r.returncode, args.step_timeout), file=sys.stderr)
            return 1
        lines.append(r.stdout.strip())
    if steps != list(CASES) + ["vns"]:
        print("a partial run: %s is not written" % args.out)
        return 0
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/msnl3_rate.py --reps %d --vns, %s\n" % (args.reps, datetime.date.today().isoformat()))
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
