#!/usr/bin/env python3
"""The neighbour-list VNS on the device next to what exists: seconds, seconds per walk-iteration, sweeps per
iteration and best cost for pr1002 (256 walks of 50 iterations), fnl4461 (64 x 20) and pla85900 (16 x 5, matrix-free), all at
K = 8 and from the nearest-neighbour tour of node 0, of

  (a) vns_walks_nl, the batch of walks;
  (b) the same walks on the same numbers one at a time through the existing entry points: tour_load + tour_local_search_nl +
      tour_store per iteration, the kick on the host (make_golden_vns_nl.kick_phase_port).  This is the yardstick; its time is
      given whole (`one_by_one_s`) and without the host kicks (`one_by_one_device_s`: the three entry points only);
  (c) vns_search with the same k on one walk (the full 2-opt sweep in every iteration).

    python tools/vns_nl_rate.py [--reps 2] [--step-timeout 900] [--cases pr1002,fnl4461] [--out FILE]

Every call returns behind a synchronisation of the engine's stream, so the wall times are bounded by the device's work.  One
warm call of each path comes first (code object load, allocations), then --reps timed repetitions, all of them reported
(`*_s`: the list, `*_min_s`: its minimum).  The numbers of walk w are a seeded stream of its own, the same for (a) and (b), so
both must end with the same tours: `same_result` says whether they did.  Every case is a GPU step of its own: a child process
under its own time limit, in which (a), (b) and (c) run one after the other; the first case that fails or runs out of time
ends the run.  Only a complete run of all cases writes the output file (default profiles/vns_nl_rate.txt), with the date.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_vns_nl import kick_phase_port  # noqa: E402
from nl2opt_rate import points  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "vns_nl_rate.txt")
CASES = {"pr1002": (256, 50), "fnl4461": (64, 20), "pla85900": (16, 5)}     # instance -> walks, iterations
K = 8


def step(name, reps):
    import travellingsalesmanoptimization_amd as T
    xy, kind = points(name)
    W, k = CASES[name]
    eng = T.Engine(0)
    if name == "pla85900":
        eng.set_option(T.OPT_MATRIX_FREE, 1)
    eng.set_points(xy, kind)
    eng.build_costs()
    eng.neighbours_build(K)
    info = eng.info()
    n = len(xy)
    start, cost0 = eng.nn_tour(0)
    nrand = 32 * k + 1024
    rv = np.random.default_rng(1).integers(0, 2 ** 31 - 1, (W, nrand)).astype(np.int32)
    row = {"instance": name, "n": n, "walks": W, "k": k, "K": K, "matrix_free": info["matrix_free"], "elem": info["elem"], "reps": reps}

    def batch(walks):
        paths = np.ascontiguousarray(np.tile(start, (walks, 1)), np.int32)
        bests = paths.copy()
        r = eng.vns_walks_nl(paths, k, rv[:walks], bests, np.full(walks, cost0))
        assert r["rc"] == 0
        return r, paths

    device = [0.0]

    def one_by_one(walks):
        sweeps, best, finals = 0, cost0, []
        for w in range(walks):
            path, cur = start.copy(), 0
            for _ in range(k):
                t0 = time.perf_counter()
                eng.tour_load(0, path)
                d = eng.tour_local_search_nl(0)
                path, cost, _ = eng.tour_store(0)
                device[0] += time.perf_counter() - t0
                sweeps += d["two_opt_sweeps"] + d["or_sweeps"]
                best = min(best, cost)
                cur, _ = kick_phase_port(path, rv[w], cur)
            finals.append(path)
        return sweeps, best, finals

    batch(2)                                    # warm: every path once
    one_by_one(1)
    ta, tb, tbd = [], [], []
    for _ in range(reps):                       # (a) and (b) in turn
        t0 = time.perf_counter()
        a, paths = batch(W)
        ta.append(round(time.perf_counter() - t0, 4))
        ia = eng.info()
        device[0] = 0.0
        t0 = time.perf_counter()
        b = one_by_one(W)
        tb.append(round(time.perf_counter() - t0, 4))
        tbd.append(round(device[0], 4))
    its = W * k
    sa = int(a["totals"]["two_opt_sweeps"].sum() + a["totals"]["or_sweeps"].sum())
    row["batch"] = {"s": ta, "min_s": min(ta), "s_per_walk_iteration": min(ta) / its, "sweeps_per_iteration": round(sa / its, 2),
                    "best_cost": float(a["best_costs"].min()), "rounds": ia["vns_nl_rounds"], "max_live": ia["vns_nl_max_live"]}
    row["one_by_one"] = {"s": tb, "min_s": min(tb), "device_s": tbd, "device_min_s": min(tbd), "s_per_walk_iteration": min(tb) / its,
                         "device_s_per_walk_iteration": min(tbd) / its, "sweeps_per_iteration": round(b[0] / its, 2), "best_cost": b[1]}
    row["same_result"] = bool(all(np.array_equal(paths[w], b[2][w]) for w in range(W)) and b[1] == float(a["best_costs"].min()) and b[0] == sa)
    row["speedup_min_over_min"] = round(min(tb) / min(ta), 2)
    row["speedup_device_min_over_min"] = round(min(tbd) / min(ta), 2)

    def single():
        path, best = start.copy(), start.copy()
        return eng.vns_search(path, k, rv[0], best, cost0)
    single()
    tc = []
    for _ in range(reps):
        t0 = time.perf_counter()
        c = single()
        tc.append(round(time.perf_counter() - t0, 4))
    ic = eng.info()
    row["vns_search"] = {"s": tc, "min_s": min(tc), "s_per_walk_iteration": min(tc) / k, "best_cost": c["best_cost"], "rc": c["rc"],
                         "vns_mode": ic["vns_mode"],
                         "sweeps_per_iteration": round(ic["persist_sweeps"] / k, 2) if ic["vns_mode"] == 1 else "not measured"}
    eng.close()
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
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
        f.write("# tools/vns_nl_rate.py --reps %d, %s\n" % (args.reps, datetime.date.today().isoformat()))
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
