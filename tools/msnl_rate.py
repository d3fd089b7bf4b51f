#!/usr/bin/env python3
"""The batched neighbour-list descent and its multi-start on the device next to what exists: wall time, total
sweeps and best cost for pr1002 (all 1002 starts), fnl4461 (512 starts), d18512 (64 starts, matrix mode) and pla85900 (16
starts, matrix-free), at K = 5, 8 and 12, of

  (a) multistart_local_search_nl, the batch;
  (b) the same starts one slot after the other in the same process, tour_nn + tour_local_search_nl: what the single-tour entry
      points offer for a multi-start.  This is the yardstick;
  (c) multistart_local_search and multistart_nn_2opt (they do not depend on K: measured once), where they take the instance,
      under --existing-limit seconds (rc 4: the limit passed, the figures are those of the starts done until then).

    python tools/msnl_rate.py [--reps 3] [--existing-limit 60] [--step-timeout 900] [--cases pr1002,fnl4461] [--out FILE]

Every call returns behind a synchronisation of the engine's stream, so the wall times are bounded by the device's work.  One
warm call of each path comes first (code object load, allocations); then --reps timed repetitions of (a) and (b) each, all of
them reported (`*_s`: the list, `*_min_s`: its minimum), and one of each leg of (c).  Every case is a GPU step of its own: a
child process under its own time limit, and the first one that fails or runs out of time ends the run.  Only a complete run
of all cases writes the output file (default profiles/msnl_rate.txt), with the date; a partial run prints its rows only.
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
from nl2opt_rate import KS, points  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "msnl_rate.txt")
CASES = {"pr1002": 1002, "fnl4461": 512, "d18512": 64, "pla85900": 16}     # instance -> starts


def timed(reps, fn):
    out, last = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        last = fn()
        out.append(round(time.perf_counter() - t0, 4))
    return out, last


def step(name, reps, existing_limit):
    import travellingsalesmanoptimization_amd as T
    from travellingsalesmanoptimization_amd import TspGpuError
    xy, kind = points(name)
    nstarts = CASES[name]
    starts = list(range(nstarts))
    eng = T.Engine(0)
    if name == "pla85900":
        eng.set_option(T.OPT_MATRIX_FREE, 1)
    eng.set_points(xy, kind)
    eng.build_costs()
    eng.set_option(T.OPT_MAX_TOURS, max(1024, nstarts))
    info = eng.info()
    row = {"instance": name, "n": len(xy), "starts": nstarts, "matrix_free": info["matrix_free"], "elem": info["elem"], "reps": reps}

    def one_by_one():
        tot, best = 0, None
        for s in starts:
            eng.tour_nn(0, s)
            r = eng.tour_local_search_nl(0)
            tot += r["two_opt_sweeps"] + r["or_sweeps"]
            cost = eng.tour_store(0, want_path=False)[1]
            best = cost if best is None or cost < best else best
        return tot, best

    for K in KS:
        eng.neighbours_build(K)
        eng.multistart_local_search_nl(starts[:2])          # warm: both paths once
        eng.tour_nn(0, 0)
        eng.tour_local_search_nl(0)
        ta, a = timed(reps, lambda: eng.multistart_local_search_nl(starts))
        i = eng.info()
        tb, b = timed(reps, one_by_one)
        row["K%d" % K] = {"batch_s": ta, "batch_min_s": min(ta), "batch_sweeps": a["two_opt_sweeps"] + a["or_sweeps"], "batch_cost": a["cost"],
                          "batch_start": a["start"], "batch_rc": a["rc"], "batch_launches": i["nl_batch_launches"],
                          "one_by_one_s": tb, "one_by_one_min_s": min(tb), "one_by_one_sweeps": b[0], "one_by_one_cost": b[1],
                          "speedup_min_over_min": round(min(tb) / min(ta), 2)}
    for leg, call in (("multistart_local_search", eng.multistart_local_search), ("multistart_nn_2opt", eng.multistart_nn_2opt)):
        try:
            call(starts[:2])
            t0 = time.perf_counter()
            e = call(starts, time_left_s=existing_limit)
            row[leg] = {"s": round(time.perf_counter() - t0, 4), "cost": e["cost"], "rc": e["rc"],
                        "sweeps": e.get("two_opt_sweeps", e.get("sweeps")), "or_moves": e.get("or_moves")}
        except TspGpuError as e:
            row[leg] = {"refused": e.code}
    eng.close()
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--existing-limit", type=float, default=60.0, help="seconds for each leg of (c)")
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        step(args.step, args.reps, args.existing_limit)
        return 0
    cases = [c for c in args.cases.split(",") if c]
    lines = []
    for name in cases:              # one GPU step at a time, each under its own limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name,
               "--reps", str(args.reps), "--existing-limit", str(args.existing_limit)]
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
        f.write("# tools/msnl_rate.py --reps %d --existing-limit %g, %s\n" % (args.reps, args.existing_limit, datetime.date.today().isoformat()))
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
