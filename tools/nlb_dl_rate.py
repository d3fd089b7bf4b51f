#!/usr/bin/env python3
"""The walks and the multi-start with don't-look bits next to the plain ones, on the same numbers: for pr1002
(256 walks of 50 iterations), fnl4461 (64 x 20) and pla85900 (16 x 5, matrix-free), K = W = 8, from the nearest-neighbour tour
of node 0,

  vns_walks_nl3 (the yardstick) against vns_walks_nl3_dl with closing = 0 and with closing = 1;

and for pr1002 (1002 starts), fnl4461 (512) and pla85900 (16)

  multistart_local_search_nl3 against multistart_local_search_nl3_dl with closing = 0 and 1.

    python tools/nlb_dl_rate.py [--reps 5] [--step-timeout 900] [--cases pr1002,fnl4461] [--out FILE]

Per column: whole calls, one warm call first, then --reps timed ones: the list, its median, minimum and maximum; seconds per
walk-iteration (of the median); sweeps; `looked` against n x sweeps; the best incumbent.  The trajectories of the columns differ
by rule (a walk with looks sees fewer candidates behind a kick), so costs are reported, not compared.  Every call returns behind
a synchronisation of the engine's stream.  Every case is a GPU step of its own: a child process under its own time limit; the
first one that fails or runs out of time ends the run.  Only a complete run writes the output file (default
profiles/nlb_dl_rate.txt), with the date.
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

OUT = os.path.join(ROOT, "profiles", "nlb_dl_rate.txt")
CASES = {"pr1002": (256, 50, 1002), "fnl4461": (64, 20, 512), "pla85900": (16, 5, 16)}     # instance -> walks, iterations, starts
K = W = 8
SWEEPS = ("two_opt_sweeps", "or_sweeps", "three_sweeps")


def timed(reps, fn):
    out, last = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        last = fn()
        out.append(round(time.perf_counter() - t0, 4))
    return {"s": out, "med_s": statistics.median(out), "min_s": min(out), "max_s": max(out)}, last


def step(name, reps):
    import travellingsalesmanoptimization_amd as T
    xy, kind = points(name)
    walks, k, nstarts = CASES[name]
    eng = T.Engine(0)
    if name == "pla85900":
        eng.set_option(T.OPT_MATRIX_FREE, 1)
    eng.set_points(xy, kind)
    eng.build_costs()
    eng.neighbours_build(K)
    eng.set_option(T.OPT_MAX_TOURS, max(1024, nstarts))
    n = len(xy)
    start, cost0 = eng.nn_tour(0)
    rv = np.random.default_rng(1).integers(0, 2 ** 31 - 1, (walks, 64 * k + 4096)).astype(np.int32)
    row = {"instance": name, "n": n, "walks": walks, "k": k, "starts": nstarts, "K": K, "W": W, "matrix_free": eng.info()["matrix_free"],
           "reps": reps}

    def walk(closing, count=walks):
        paths = np.ascontiguousarray(np.tile(start, (count, 1)), np.int32)
        bests, bc = paths.copy(), np.full(count, float(cost0))
        if closing is None:
            r = eng.vns_walks_nl3(paths, k, rv[:count], bests, bc, W)
        else:
            r = eng.vns_walks_nl3_dl(paths, k, rv[:count], bests, bc, W, closing)
        assert r["rc"] == 0
        return {t: int(v.sum()) for t, v in r["totals"].items()}, float(bc.min())

    def ms(closing, starts):
        r = eng.multistart_local_search_nl3(W, starts) if closing is None else eng.multistart_local_search_nl3_dl(W, closing, starts)
        assert r["rc"] == 0
        return r

    for col, closing in (("plain", None), ("dl_closing0", 0), ("dl_closing1", 1)):
        walk(closing, 2)                    # warm: code object load, allocations
        t, (tot, best) = timed(reps, lambda: walk(closing))
        sweeps = sum(tot[s] for s in SWEEPS)
        row["walks_" + col] = dict(t, s_per_walk_iteration=t["med_s"] / (walks * k), sweeps=sweeps, looked=tot.get("looked", n * sweeps),
                                   n_x_sweeps=n * sweeps, best=best)
    starts = list(range(nstarts))
    for col, closing in (("plain", None), ("dl_closing0", 0), ("dl_closing1", 1)):
        ms(closing, starts[:2])
        t, r = timed(reps, lambda: ms(closing, starts))
        sweeps = sum(r[s] for s in SWEEPS)
        row["multistart_" + col] = dict(t, sweeps=sweeps, looked=r.get("looked", n * sweeps), n_x_sweeps=n * sweeps, best=r["cost"])
    eng.close()
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        step(args.step, args.reps)
        return 0
    cases = [c for c in args.cases.split(",") if c]
    lines = []
    for name in cases:              # one GPU step at a time, each under its own limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            print("%s: exit code %d (124 / 137: no result within %d s); stopping" % (name, r.returncode, args.step_timeout), file=sys.stderr)
            return 1
        lines.append(r.stdout.strip())
    if cases != list(CASES):
        print("a partial run: %s is not written" % args.out)
        return 0
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/nlb_dl_rate.py --reps %d, %s\n" % (args.reps, datetime.date.today().isoformat()))
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
