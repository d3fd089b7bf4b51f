#!/usr/bin/env python3
"""The greedy-edge construction on the device next to the nearest-neighbour tour from node 0, and the descents over
the lists started from either: for pr1002 and fnl4461 (matrix mode) and pla85900 (matrix-free), at K = W = 8,

  (a) tour_greedy against tour_nn(0) -- seconds, the rounds of the two phases, the tour's cost;
  (b) tour_local_search_nl3 and tour_local_search_nl3_dl (closing = 0) from the greedy-edge tour and from NN(0) -- seconds, sweeps,
      units looked at and the final cost.

    python tools/greedy_rate.py [--reps 5] [--step-timeout 900] [--cases pr1002,fnl4461] [--out FILE]
    python tools/greedy_rate.py --instance pla85900 --reps 1 --construct-only      # one case in this process, (a) only

Every timed item is repeated `--reps` times from the same state (host clock around the calls, the stream drained by a read-back
on either side); the file keeps the minimum, the median and the maximum.  No threshold is set on these times.  Every case is a GPU
step of its own: a child process under its own time limit, and the first one that fails or runs out of time ends the run.  Only a
complete run of all cases writes profiles/greedy_rate.txt, with the date and the repetition count.
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
from dont_look_rate import COUNTERS, spread  # noqa: E402
from make_golden_two_opt_nl import digest  # noqa: E402
from nl2opt_rate import points  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "greedy_rate.txt")
CASES = ["pr1002", "fnl4461", "pla85900"]
K = W = 8


def timed(eng, reps, body):
    """body() `reps` times behind one warm call, the stream drained on either side -> (spread, the last result)"""
    out = body()
    ts = []
    for _ in range(reps):
        eng.tour_store(0, want_path=False)
        t0 = time.perf_counter()
        out = body()
        eng.tour_store(0, want_path=False)
        ts.append(time.perf_counter() - t0)
    return spread(ts), out


def step(name, reps, construct_only):
    import travellingsalesmanoptimization_amd as T
    xy, kind = points(name)
    eng = T.Engine(0)
    eng.set_points(xy, kind)
    eng.build_costs()
    info = eng.info()
    row = {"instance": name, "n": len(xy), "K": K, "W": W, "matrix_free": info["matrix_free"], "elem": info["elem"], "reps": reps}
    eng.neighbours_build(K)
    row["nn"], _ = timed(eng, reps, lambda: eng.tour_nn(0, 0))
    row["nn_cost"] = eng.tour_store(0, want_path=False)[1]
    eng.tour_copy(1, 0)
    row["greedy"], _ = timed(eng, reps, lambda: eng.tour_greedy(0))
    path, row["greedy_cost"], _ = eng.tour_store(0)
    row["greedy_path_sha256"] = digest(path)
    info = eng.info()
    row.update({"rounds1": info["greedy_rounds1"], "rounds2": info["greedy_rounds2"], "edges1": info["greedy_edges1"], "free": info["greedy_free"]})
    eng.tour_copy(2, 0)
    if not construct_only:
        for start, slot in (("from_greedy", 2), ("from_nn", 1)):
            for how in ("plain", "dl_closing0"):
                def descend():
                    eng.tour_copy(0, slot)
                    if how == "plain":
                        d = eng.tour_local_search_nl3(0, W)
                        s = sum(d[k] for k in COUNTERS)
                        return s, s * eng.n
                    d = eng.tour_local_search_nl3_dl(0, W, 0)
                    return sum(d[k] for k in COUNTERS), d["looked"]
                t, (s, q) = timed(eng, reps, descend)
                row["%s_%s" % (how, start)] = dict(t, sweeps=s, looked=q, cost=eng.tour_store(0, want_path=False)[1])
    eng.close()
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--instance", default=None, help="one case in this process")
    ap.add_argument("--construct-only", action="store_true", help="with --instance: the constructions only, no descent")
    args = ap.parse_args()
    if args.instance:
        step(args.instance, args.reps, args.construct_only)
        return 0
    cases = [c for c in args.cases.split(",") if c]
    lines = []
    for name in cases:              # one GPU step at a time, each under its own limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--instance", name, "--reps", str(args.reps)]
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
        f.write("# tools/greedy_rate.py --reps %d, %s\n" % (args.reps, datetime.date.today().isoformat()))
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
