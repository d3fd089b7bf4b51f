"""Or-opt on the device: the sweep kernel alone (HIP events, after a warm-up) at n = 1024, 4096, 16384 with uint16 cells, next
to the one-launch-per-sweep 2-opt kernel (tspgpu_time_sweep) at the same n in the same process; then the wall time of
local_search and what it gains over plain two_opt per instance.

    python tools/oropt_rate.py [--sizes 1024,4096,16384] [--instances pr1002,fnl4461,rand4096] [--reps 50]

Candidates of one Or-opt sweep: per segment start n - 2 places for L = 1, 2 (n - 3) for L = 2 (both orientations),
2 (n - 4) for L = 3: n (5 n - 16).  The bound of the sweep is one read of the n x n matrix (both the head's and the
tail's row of every segment are needed) at the 6.3 TB/s a streaming kernel reaches on an MI355X.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import travellingsalesmanoptimization_amd as T  # noqa: E402
from travellingsalesmanoptimization_amd.tsplib import read as read_tsplib  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def reference_points(n, seed=123):
    """the reference's generator (src/tsp.c:468-476): the point sets of bench.py; drawn before the first GPU call"""
    libc = ctypes.CDLL(None)
    libc.srand(ctypes.c_uint(seed))
    xy = np.empty((n, 2), dtype=np.float64)
    for i in range(n):
        xy[i, 0] = (libc.rand() / 2147483647) * 10000 + (-5000)
        xy[i, 1] = (libc.rand() / 2147483647) * 10000 + (-5000)
    return xy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--instances", default="pr1002,fnl4461,rand4096")
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",") if s]
    names = [s for s in args.instances.split(",") if s]
    pts = {n: reference_points(n) for n in sorted(set(sizes) | {int(s[4:]) for s in names if s.startswith("rand")})}
    for n in sizes:
        eng = T.Engine(0)
        eng.set_option(T.OPT_ELEM, T.ELEM_U16)
        eng.set_points(pts[n])
        eng.build_costs()
        eng.tour_nn(0, 0)
        eng.set_option(T.OPT_PERSIST, 0)              # tspgpu_time_sweep: the one-launch-per-sweep plan
        eng.set_option(T.OPT_STREAM_PERSIST, 0)
        or_us = eng.time_or_sweep(0, args.reps) * 1e3
        two_us = eng.time_sweep(0, args.reps) * 1e3
        cand = n * (5 * n - 16)
        bound_us = 2.0 * n * n / HBM_BYTES_PER_S * 1e6
        print(json.dumps({"n": n, "elem": eng.info()["elem"], "or_sweep_us": round(or_us, 2), "or_candidates": cand,
                          "or_candidates_per_s": round(cand / (or_us * 1e-6), 0), "matrix_read_us": round(bound_us, 2),
                          "bound_fraction": round(bound_us / or_us, 4), "two_opt_sweep_us": round(two_us, 2),
                          "two_opt_pairs_per_s": round(T.evals_per_sweep(n) / (two_us * 1e-6), 0)}), flush=True)
        eng.close()
    for name in names:
        xy = pts[int(name[4:])] if name.startswith("rand") else read_tsplib(os.path.join(ROOT, "tests", "golden", "data", name + ".tsp"))[0]
        eng = T.Engine(0)
        eng.set_points(xy)
        eng.build_costs()
        nn, _ = eng.nn_tour(0)
        eng.local_search(nn.copy())                   # warm-up (code objects, allocations)
        p = nn.copy()
        t0 = time.perf_counter()
        c2, sweeps, _ = eng.two_opt(p)
        t1 = time.perf_counter()
        p = nn.copy()
        t2 = time.perf_counter()
        r = eng.local_search(p)
        t3 = time.perf_counter()
        print(json.dumps({"instance": name, "n": len(xy), "two_opt_cost": c2, "two_opt_sweeps": sweeps, "two_opt_ms": round((t1 - t0) * 1e3, 3),
                          "local_search_cost": r["cost"], "local_search_ms": round((t3 - t2) * 1e3, 3), "rounds": r["rounds"],
                          "ls_two_opt_sweeps": r["two_opt_sweeps"], "or_moves": r["or_moves"],
                          "gain_percent": round(100.0 * (c2 - r["cost"]) / c2, 3)}), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
