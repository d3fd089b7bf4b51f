#!/usr/bin/env python3
"""Golden of the parallel-move 2-opt model (tests/two_opt_multi_model.c) where the model takes more than a few seconds, and
the CPU measurements DESIGN 4.13 quotes.  CPU only.

    python tools/make_golden_two_opt_multi.py            # writes tests/golden/golden_two_opt_multi.json
    python tools/make_golden_two_opt_multi.py --measure  # prints sweeps / moves / final cost of the model's descent from NN(0)

The golden: 66 000 uniform integer points (seed 66000, EUC_2D), the tour that walks them in vertical stripes, one sweep --
the number of accepted moves, the sum of their deltas, the cost and SHA-256 digests of the start, the move list and the
resulting successor array (tests/test_two_opt_multi.py: test_gpu_large_instance_one_sweep builds the same start).
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "golden_two_opt_multi.json")
_dp = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_ip = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")


def model():
    d = tempfile.mkdtemp(prefix="two_opt_multi_model_")
    so = os.path.join(d, "two_opt_multi_model.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", "-o", so,
                    os.path.join(ROOT, "tests", "two_opt_multi_model.c"), "-lm"], check=True)
    lib = C.CDLL(so)
    lib.tom_sweep.restype = C.c_int
    lib.tom_sweep.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, _ip, C.c_int, _dp, _ip, C.POINTER(C.c_int), _ip, _ip, _ip, _ip,
                              _dp, _ip, C.POINTER(C.c_int), _ip, _dp, C.POINTER(C.c_double), C.c_int]
    lib.tom_descent.restype = C.c_int
    lib.tom_descent.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, _ip, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_long),
                                C.POINTER(C.c_long), C.POINTER(C.c_int), C.POINTER(C.c_long)]
    return lib


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.int32).tobytes()).hexdigest()


def euc(xy, a, b):
    d = xy[b] - xy[a]
    sq = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
    return (np.sqrt(sq.astype(np.float32)).astype(np.float64) + 0.5).astype(np.int64)


def large_points(n, seed):
    return np.random.default_rng(seed).integers(0, 30000, (n, 2)).astype(np.float64)


def stripe_tour(xy, width=300.0):
    """successor array of the tour through vertical stripes of `width`, upwards in even stripes and downwards in odd ones"""
    stripe = np.floor(xy[:, 0] / width).astype(np.int64)
    y = np.where(stripe % 2 == 0, xy[:, 1], -xy[:, 1])
    order = np.lexsort((np.arange(len(xy)), y, stripe)).astype(np.int32)
    path = np.empty(len(xy), np.int32)
    path[order] = np.roll(order, -1)
    return path


def nn0(xy):
    """h_greedyutil from node 0 (EUC_2D): the nearest unvisited node, ties to the lowest label"""
    n = len(xy)
    left = np.ones(n, bool)
    path = np.empty(n, np.int32)
    v = 0
    left[0] = False
    for _ in range(n - 1):
        w = np.where(left, euc(xy, v, np.arange(n)), np.iinfo(np.int64).max)
        u = int(np.argmin(w))
        path[v] = u
        left[u] = False
        v = u
    path[v] = 0
    return path


def reference_points(n, seed=123):
    """the reference's generator (src/tsp.c:468-476): the point sets of bench.py"""
    libc = C.CDLL(None)
    libc.srand(C.c_uint(seed))
    xy = np.empty((n, 2), dtype=np.float64)
    for i in range(n):
        xy[i, 0] = (libc.rand() / 2147483647) * 10000 + (-5000)
        xy[i, 1] = (libc.rand() / 2147483647) * 10000 + (-5000)
    return xy


def one_sweep(lib, xy, path, cost, threads):
    n = len(xy)
    xy = np.ascontiguousarray(xy.reshape(-1))
    raw_d, cdl, deltas = np.empty(n), np.empty(n), np.empty(n)
    raw_b, ca, cb, ci, cj, acc = (np.empty(n, np.int32) for _ in range(6))
    mv = np.empty(2 * n, np.int32)
    m, k, cc = C.c_int(), C.c_int(), C.c_double(cost)
    assert lib.tom_sweep(None, xy.ctypes.data, n, 0, path, threads, raw_d, raw_b, C.byref(m), ca, cb, ci, cj, cdl, acc, C.byref(k), mv,
                         deltas, C.byref(cc), 1) == 0
    return cc.value, mv[:2 * k.value].reshape(-1, 2).copy(), deltas[:k.value].copy(), m.value


def measure(lib, threads):
    from travellingsalesmanoptimization_amd.tsplib import read as read_tsplib
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "golden.json")))
    for name, key in (("pr1002", "pr1002"), ("fnl4461", "fnl4461"), ("n4096_s123", "n4096_s123")):
        xy = reference_points(4096, 123) if name.startswith("n4096") else \
            np.asarray(read_tsplib(os.path.join(ROOT, "tests", "golden", "data", name + ".tsp"))[0], dtype=np.float64)
        path = nn0(xy)
        flat = np.ascontiguousarray(xy.reshape(-1))
        cc, sw, mv, mk, mu = C.c_double(), C.c_long(), C.c_long(), C.c_int(), C.c_long()
        t0 = time.perf_counter()
        assert lib.tom_descent(None, flat.ctypes.data, len(xy), 0, path, threads, C.byref(cc), C.byref(sw), C.byref(mv), C.byref(mk),
                               C.byref(mu)) == 0
        ref = (golden["instances"].get(key) or golden["random"].get(key) or {}).get("two_opt", {})
        print(json.dumps({"instance": name, "n": len(xy), "model_sweeps": sw.value, "model_moves": mv.value, "model_max_moves": mk.value,
                          "model_cost": cc.value, "reference_sweeps": ref.get("sweeps"), "reference_cost": ref.get("final_cost"),
                          "cpu_s": round(time.perf_counter() - t0, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--threads", type=int, default=min(32, os.cpu_count() or 1))
    a = ap.parse_args()
    lib = model()
    if a.measure:
        measure(lib, a.threads)
        return
    n, seed = 66000, 66000
    xy = large_points(n, seed)
    path = stripe_tour(xy)
    start = digest(path)
    cost0 = float(euc(xy, np.arange(n), path).sum())
    cost, mv, dl, m = one_sweep(lib, xy, path, cost0, a.threads)
    out = {"n66000": {"n": n, "seed": seed, "kind": "EUC_2D", "start": "stripe_tour(width 300)", "start_sha256": start, "start_cost": cost0,
                      "candidates": m, "moves": len(mv), "delta_sum": float(dl.sum()), "cost": cost, "moves_sha256": digest(mv),
                      "path_sha256": digest(path), "max_label": int(mv.max())}}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
