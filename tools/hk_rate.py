#!/usr/bin/env python3
"""The Held-Karp lower bound on the device next to the CPU model (tests/held_karp_model.c), the only comparison
there is: for pr1002, 4096 uniform points and fnl4461 (matrix mode) and pla85900 (matrix-free),

  (a) one 1-tree at pi = 0 (tspgpu_one_tree without the edge and degree read-back) -- seconds and Boruvka rounds;
  (b) the ascent, 300 iterations at patience 10 (pla85900: 20) from the cost of NN(0) (pr1002: 275 427, the golden's) -- seconds,
      seconds per iteration evaluated, the bound, the reason;
  (c) the model on this host: one 1-tree, and the ascent's seconds per iteration over its first 20 iterations (pla85900: the tree only).

    python tools/hk_rate.py [--reps 5] [--step-timeout 900] [--cases pr1002,fnl4461] [--out FILE]
    python tools/hk_rate.py --instance pla85900 --reps 1      # one case in this process

Every timed item is repeated `--reps` times (host clock around the calls, which return with the stream drained); the file keeps
the minimum, the median and the maximum.  The model runs once.  No threshold is set on these times.  Every case is a GPU step of
its own: a child process under its own time limit, and the first one that fails or runs out of time ends the run.  Only a
complete run of all cases writes profiles/hk_rate.txt, with the date and the repetition count.
"""
import argparse
import ctypes as C
import datetime
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dont_look_rate import spread  # noqa: E402
from make_golden_held_karp import model, model_ascent, model_one_tree  # noqa: E402
from nl2opt_rate import points  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "hk_rate.txt")
CASES = ["pr1002", "n4096", "fnl4461", "pla85900"]
UPPER = {"pr1002": 275427}
ITERS = {"pla85900": 20}
MODEL_ITERS = 20


def timed(reps, body):
    """body() `reps` times behind one warm call -> (spread, the last result)"""
    out = body()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = body()
        ts.append(time.perf_counter() - t0)
    return spread(ts), out


def step(name, reps):
    import travellingsalesmanoptimization_amd as T
    xy, kind = points(name)
    n = len(xy)
    eng = T.Engine(0)
    eng.set_points(xy, kind)
    eng.build_costs()
    info = eng.info()
    upper = UPPER.get(name) or int(eng.nn_tour(0)[1])
    iters = ITERS.get(name, 300)
    row = {"instance": name, "n": n, "matrix_free": info["matrix_free"], "elem": info["elem"], "reps": reps, "upper": upper, "iters_asked": iters}

    def tree():
        w = C.c_long()
        assert eng.L.tspgpu_one_tree(eng.ctx, None, None, None, C.byref(w)) == 0
        return w.value
    row["tree"], row["L0"] = timed(reps, tree)
    row["rounds"], row["rounds_enqueued"] = eng.info()["hk_rounds"], max(1, (n - 2).bit_length())
    row["ascent"], r = timed(reps, lambda: eng.lower_bound(upper, iters, 10))
    row.update({"bound": r.bound, "reason": r.reason, "iters": r.iters, "iteration_median_s": round(row["ascent"]["median_s"] / r.iters, 9)})
    eng.close()
    model()                         # (compiled before the clock starts)
    t0 = time.perf_counter()
    assert model_one_tree(xy=xy, kind=kind)["L"] == row["L0"]
    row["model_tree_s"] = round(time.perf_counter() - t0, 6)
    if n <= 10000:
        t0 = time.perf_counter()
        m = model_ascent(upper, MODEL_ITERS, 10, xy=xy, kind=kind)
        row["model_iteration_s"] = round((time.perf_counter() - t0) / m["iters"], 6)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--instance", default=None, help="one case in this process")
    args = ap.parse_args()
    if args.instance:
        step(args.instance, args.reps)
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
        f.write("# tools/hk_rate.py --reps %d, %s\n" % (args.reps, datetime.date.today().isoformat()))
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
