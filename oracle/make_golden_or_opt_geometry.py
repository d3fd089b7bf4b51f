#!/usr/bin/env python3
"""tests/golden/golden_or_opt_geometry.json: the model results of tests/test_or_opt_geometry.py that are too slow to compute
at test time (more than about 5 s): the first K Or-opt moves from the identity tour at the large sweep sizes (traces only),
and per-slot cost, counters and a SHA-256 of the final path of the large batch cases.  CPU only; the model, the instances
and the case lists are the test module's own.  Prints the seconds each case took.
--measure: time the model side of EVERY case of the module, golden or not (nothing is written)."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)
import test_or_opt_geometry as G


def walk(n):
    t0 = time.time()
    cost, trace = G.model_sweep_walk(n)
    print("walk  n = %5d: %6.1f s, %d moves" % (n, time.time() - t0, len(trace)), flush=True)
    return {"cost": cost, "trace": [list(mv) for mv in trace]}


def batch(n):
    t0 = time.time()
    c, starts = G.batch_instance(n)
    t1 = time.time()
    res = G.batch_model(c, starts)
    print("batch n = %5d: %6.1f s (matrix and starts %.1f s), or_moves %s rounds %s" %
          (n, time.time() - t0, t1 - t0, [r["or_moves"] for r in res], [r["rounds"] for r in res]), flush=True)
    return [{k: r[k] for k in ("cost", "two_opt_sweeps", "or_moves", "rounds", "sha256")} for r in res]


def main():
    if "--measure" in sys.argv:
        for n in sorted({c[1] for c in G.SWEEP_CASES}):
            walk(n)
        for n in sorted({c[1] for c in G.BATCH_CASES}):
            batch(n)
        return
    out = {"_generator": "oracle/make_golden_or_opt_geometry.py", "K": G.K,
           "walks": {str(n): walk(n) for n in G.GOLDEN_WALKS}, "batches": {str(n): batch(n) for n in G.GOLDEN_BATCHES}}
    dst = os.path.join(HERE, "..", "tests", "golden", "golden_or_opt_geometry.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("written", os.path.normpath(dst))


if __name__ == "__main__":
    main()
