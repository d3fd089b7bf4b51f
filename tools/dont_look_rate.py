#!/usr/bin/env python3
"""Don't-look bits on the device next to the plain descent over the lists: for pr1002 and fnl4461 (matrix mode) and
pla85900 (matrix-free), at K = W = 8,

  (a) the descent from NN(0): tour_local_search_nl3 against tour_local_search_nl3_dl with closing 0 and 1 -- seconds, sweeps,
      full sweeps, units looked at and the final cost;
  (b) `--kicks` kicks at fixed positions (seed 2024), each followed by a descent, all on the slot: the plain slot descent behind
      tour_kick (the yardstick: the code the parent commit has, plus the kick), _dl with closing 0, _dl with closing 1 --
      seconds per iteration, units looked at per iteration and the final cost;
  (c) `--step NAME --trace` runs the closing = 0 descent from NN(0) and (b)'s closing = 0 loop once and nothing else: the child
      to put behind `rocprofv3 --kernel-trace --stats --output-format csv --` in a run of its own for the mean time of
      k_look_queue and k_look_wake (profiles/dont_look_kernel_stats_pla85900.csv is its kernel_stats file).

    python tools/dont_look_rate.py [--reps 5] [--kicks 200] [--step-timeout 900] [--cases pr1002,fnl4461] [--out FILE]

Every timed item is repeated `--reps` times from the same state (host clock around the calls, the stream drained by the call's
own read-back); the file keeps the minimum, the median and the maximum.  No threshold is set on these times.  Every case is a
GPU step of its own: a child process under its own time limit, and the first one that fails or runs out of time ends the run.
Only a complete run of all cases writes profiles/dont_look_rate.txt, with the date and the repetition count.
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

OUT = os.path.join(ROOT, "profiles", "dont_look_rate.txt")
CASES = ["pr1002", "fnl4461", "pla85900"]
K = W = 8
COUNTERS = ("two_opt_sweeps", "or_sweeps", "three_sweeps")


def spread(ts):
    return {"min_s": round(min(ts), 6), "median_s": round(statistics.median(ts), 6), "max_s": round(max(ts), 6)}


def kick_positions(n, count, seed=2024):
    rng = np.random.default_rng(seed)
    return [tuple(int(v) for v in sorted(rng.choice(n, 3, replace=False))) for _ in range(count)]


def descend(eng, how):
    """one descent on slot 0 -> (sweeps, looked, full sweeps)"""
    if how == "plain":
        d = eng.tour_local_search_nl3(0, W)
        s = sum(d[k] for k in COUNTERS)
        return s, s * eng.n, s
    d = eng.tour_local_search_nl3_dl(0, W, 1 if how == "dl_closing1" else 0)
    return sum(d[k] for k in COUNTERS), d["looked"], d["full_sweeps"]


def kick_loop(eng, how, kicks):
    """slot 1 holds the start (a local optimum of `how`'s own descent); the kicks and descents run on a copy in slot 0"""
    eng.tour_copy(0, 1)
    eng.tour_store(0, want_path=False)              # (drains the stream)
    sweeps = looked = 0
    t0 = time.perf_counter()
    for i, j, k in kicks:
        eng.tour_kick(0, i, j, k)
        s, q, _ = descend(eng, how)
        sweeps, looked = sweeps + s, looked + q
    cost = eng.tour_store(0, want_path=False)[1]
    return time.perf_counter() - t0, sweeps, looked, cost


def step(name, reps, nkicks, trace):
    import travellingsalesmanoptimization_amd as T
    xy, kind = points(name)
    eng = T.Engine(0)
    eng.set_points(xy, kind)
    eng.build_costs()
    info = eng.info()
    n = len(xy)
    row = {"instance": name, "n": n, "K": K, "W": W, "matrix_free": info["matrix_free"], "elem": info["elem"], "reps": reps, "kicks": nkicks}
    start, row["nn_cost"] = eng.nn_tour(0)
    eng.neighbours_build(K)
    kicks = kick_positions(n, nkicks)
    if trace:
        eng.tour_load(1, start)
        eng.tour_copy(0, 1)
        descend(eng, "dl_closing0")
        eng.tour_copy(1, 0)
        kick_loop(eng, "dl_closing0", kicks)
        eng.close()
        return
    for how in ("plain", "dl_closing0", "dl_closing1"):
        eng.tour_load(1, start)
        eng.tour_copy(0, 1)
        descend(eng, how)                           # (warm: the first launches load the code object)
        ts = []
        for _ in range(reps):
            eng.tour_copy(0, 1)
            eng.tour_store(0, want_path=False)
            t0 = time.perf_counter()
            s, q, full = descend(eng, how)
            cost = eng.tour_store(0, want_path=False)[1]
            ts.append(time.perf_counter() - t0)
        r = {"descent": dict(spread(ts), sweeps=s, looked=q, full_sweeps=full, cost=cost)}
        eng.tour_copy(1, 0)                         # the kicks start from this descent's optimum
        ts = []
        for _ in range(reps):
            t, s, q, cost = kick_loop(eng, how, kicks)
            ts.append(t / nkicks)
        r["kicks"] = dict({k + "_per_iteration": v for k, v in spread(ts).items()}, sweeps_per_iteration=round(s / nkicks, 2),
                          looked_per_iteration=round(q / nkicks, 1), cost=cost)
        row[how] = r
    row["dl_max_wgs"] = eng.info()["dl_max_wgs"]
    eng.close()
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kicks", type=int, default=200)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--step", default=None, help="one case in this process")
    ap.add_argument("--trace", action="store_true", help="with --step: the closing = 0 kick loop once, for a kernel trace")
    args = ap.parse_args()
    if args.step:
        step(args.step, args.reps, args.kicks, args.trace)
        return 0
    cases = [c for c in args.cases.split(",") if c]
    lines = []
    for name in cases:              # one GPU step at a time, each under its own limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name,
               "--reps", str(args.reps), "--kicks", str(args.kicks)]
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
        f.write("# tools/dont_look_rate.py --reps %d --kicks %d, %s\n" % (args.reps, args.kicks, datetime.date.today().isoformat()))
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
