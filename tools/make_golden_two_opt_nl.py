#!/usr/bin/env python3
"""Golden of the neighbour-list 2-opt model (tests/two_opt_nl_model.c) and the CPU measurements DESIGN 4.14 quotes.  CPU only.

    python tools/make_golden_two_opt_nl.py            # writes tests/golden/golden_two_opt_nl.json
    python tools/make_golden_two_opt_nl.py --measure  # prints the table of DESIGN 4.14 (K = 5, 8, 12)

The golden: pr1002 and fnl4461 from NN(0) with K = 5 and K = 8 -- sweeps, moves, cost and the SHA-256 digest of the successor
array after the neighbour-list phase, and the same after the polish; pr1002 with K = 8 from the best nearest-neighbour tour
(what `tsp -alg VNS -k 1` hands to ref_2opt); and 66 000 uniform integer points (seed 66000, EUC_2D, K = 8): the digest of the
lists and one sweep from the stripe tour.  tests/test_two_opt_nl.py imports the model wrappers below.
"""
import argparse
import ctypes as C
import functools
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
OUT = os.path.join(ROOT, "tests", "golden", "golden_two_opt_nl.json")
DATA = os.path.join(ROOT, "tests", "golden", "data")
_dp = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_ip = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_pi, _pl, _pd = C.POINTER(C.c_int), C.POINTER(C.c_long), C.POINTER(C.c_double)
THREADS = min(16, os.cpu_count() or 1)


@functools.lru_cache(maxsize=None)
def model():
    """tests/two_opt_nl_model.c (which includes two_opt_multi_model.c) compiled into a scratch directory"""
    d = tempfile.mkdtemp(prefix="two_opt_nl_model_")
    so = os.path.join(d, "two_opt_nl_model.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", "-o", so,
                    os.path.join(ROOT, "tests", "two_opt_nl_model.c"), "-lm"], check=True)
    lib = C.CDLL(so)
    lib.nlm_lists.restype = C.c_int
    lib.nlm_lists.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _dp, _pi]
    sweep = [_dp, _ip, _pi, _ip, _ip, _ip, _ip, _dp, _ip, _pi, _ip, _dp, _pd, C.c_int]
    lib.nlm_sweep.restype = C.c_int
    lib.nlm_sweep.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _ip, _ip] + sweep
    lib.tom_sweep.restype = C.c_int
    lib.tom_sweep.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, _ip, C.c_int] + sweep
    lib.nlm_descent.restype = C.c_int
    lib.nlm_descent.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _ip, _ip, C.c_int, C.c_int, _pd, _pl, _pl, _pd,
                                C.c_void_p, _pl, _pl]
    lib.tom_descent.restype = C.c_int
    lib.tom_descent.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, _ip, C.c_int, _pd, _pl, _pl, _pi, _pl]
    return lib


def _src(costs, xy):
    if costs is not None:
        costs = np.ascontiguousarray(costs, np.float64)
        return costs, costs.ctypes.data, None, len(costs)
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1)
    return xy, None, xy.ctypes.data, len(xy) // 2


def model_lists(K, costs=None, xy=None, kind=0, threads=THREADS):
    """-> (nodes [n][K'], weights [n][K']) of the C model"""
    keep, cp, xp, n = _src(costs, xy)
    kp = min(K, n - 1)
    nodes, w, got = np.empty((n, kp), np.int32), np.empty((n, kp)), C.c_int()
    assert model().nlm_lists(cp, xp, n, kind, K, threads, nodes.reshape(-1), w.reshape(-1), C.byref(got)) == 0 and got.value == kp
    return nodes, w


def model_sweep(path, cost, nodes=None, costs=None, xy=None, kind=0, apply=True, threads=THREADS):
    """one sweep of the C model over the lists `nodes` (None: the parallel-move sweep, every b); path in place when apply
    -> dict(cost, moves [k][2], deltas [k], raw_d, raw_b, cand, acc)"""
    keep, cp, xp, n = _src(costs, xy)
    raw_d, cdl, deltas = np.empty(n), np.empty(n), np.empty(n)
    raw_b, ca, cb, ci, cj, acc = (np.empty(n, np.int32) for _ in range(6))
    mv = np.empty(2 * n, np.int32)
    m, k, cc = C.c_int(), C.c_int(), C.c_double(cost)
    tail = (raw_d, raw_b, C.byref(m), ca, cb, ci, cj, cdl, acc, C.byref(k), mv, deltas, C.byref(cc), 1 if apply else 0)
    if nodes is None:
        rc = model().tom_sweep(cp, xp, n, kind, path, threads, *tail)
    else:
        nodes = np.ascontiguousarray(nodes, np.int32)
        rc = model().nlm_sweep(cp, xp, n, kind, nodes.shape[1], nodes.reshape(-1), path, *tail)
    assert rc == 0
    m, k = m.value, k.value
    cand = [(float(cdl[x]), int(ca[x]), int(cb[x]), int(ci[x]), int(cj[x])) for x in range(m)]
    return {"cost": cc.value, "moves": mv[:2 * k].reshape(-1, 2).copy(), "deltas": deltas[:k].copy(), "raw_d": raw_d, "raw_b": raw_b,
            "cand": cand, "acc": [int(v) for v in acc[:m]]}


def model_descent(path, nodes, polish, costs=None, xy=None, kind=0, threads=THREADS):
    """the descent of the C model; path in place -> dict(cost, sweeps, moves, nl_cost, nl_path, polish_sweeps, polish_moves)"""
    keep, cp, xp, n = _src(costs, xy)
    nodes = np.ascontiguousarray(nodes, np.int32)
    cc, nc, sw, mv, ps, pm = C.c_double(), C.c_double(), C.c_long(), C.c_long(), C.c_long(), C.c_long()
    mid = np.empty(n, np.int32)
    assert model().nlm_descent(cp, xp, n, kind, nodes.shape[1], nodes.reshape(-1), path, 1 if polish else 0, threads, C.byref(cc), C.byref(sw),
                               C.byref(mv), C.byref(nc), mid.ctypes.data, C.byref(ps), C.byref(pm)) == 0
    return {"cost": cc.value, "sweeps": sw.value, "moves": mv.value, "nl_cost": nc.value, "nl_path": mid, "polish_sweeps": ps.value,
            "polish_moves": pm.value}


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


def nn_from(xy, start):
    """h_greedyutil from `start` (EUC_2D): the nearest unvisited node, ties to the lowest label -> (path, cost)"""
    n = len(xy)
    left = np.ones(n, bool)
    path = np.empty(n, np.int32)
    v, cost = start, 0
    left[start] = False
    for _ in range(n - 1):
        w = np.where(left, euc(xy, v, np.arange(n)), np.iinfo(np.int64).max)
        u = int(np.argmin(w))
        path[v] = u
        cost += int(w[u])
        left[u] = False
        v = u
    path[v] = start
    return path, cost + int(euc(xy, v, start))


def best_nn(xy):
    """h_Greedy_iterative: the first strictly cheapest nearest-neighbour tour over all starts"""
    best, bc = None, None
    for s in range(len(xy)):
        p, c = nn_from(xy, s)
        if bc is None or c < bc:
            best, bc = p, c
    return best


def tsplib_points(name):
    from travellingsalesmanoptimization_amd.tsplib import read as read_tsplib
    return np.asarray(read_tsplib(os.path.join(DATA, name + ".tsp"))[0], dtype=np.float64)


def reference_points(n, seed=123):
    """the reference's generator (src/tsp.c:468-476): the point sets of bench.py"""
    libc = C.CDLL(None)
    libc.srand(C.c_uint(seed))
    xy = np.empty((n, 2), dtype=np.float64)
    for i in range(n):
        xy[i, 0] = (libc.rand() / 2147483647) * 10000 + (-5000)
        xy[i, 1] = (libc.rand() / 2147483647) * 10000 + (-5000)
    return xy


def descent_entry(xy, start, K, polish=True):
    """the golden's record of one descent (EUC_2D, from the coordinates)"""
    nodes, _ = model_lists(K, xy=xy)
    path = start.copy()
    r = model_descent(path, nodes, polish, xy=xy)
    out = {"K": K, "sweeps": r["sweeps"], "moves": r["moves"], "cost": r["nl_cost"], "path_sha256": digest(r["nl_path"])}
    if polish:
        out.update({"polish_sweeps": r["polish_sweeps"], "polish_moves": r["polish_moves"], "polished_cost": r["cost"],
                    "polished_path_sha256": digest(path)})
    return out


def large_entry(n=66000, seed=66000, K=8):
    xy = large_points(n, seed)
    nodes, _ = model_lists(K, xy=xy)
    path = stripe_tour(xy)
    start = digest(path)
    cost0 = float(euc(xy, np.arange(n), path).sum())
    r = model_sweep(path, cost0, nodes, xy=xy)
    return {"n": n, "seed": seed, "K": K, "kind": "EUC_2D", "start": "stripe_tour(width 300)", "start_sha256": start, "start_cost": cost0,
            "lists_sha256": digest(nodes), "candidates": len(r["cand"]), "moves": len(r["moves"]), "delta_sum": float(r["deltas"].sum()),
            "cost": r["cost"], "moves_sha256": digest(r["moves"]), "path_sha256": digest(path), "max_label": int(r["moves"].max())}


def measure():
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "golden.json")))
    for name in ("pr1002", "fnl4461", "n4096_s123"):
        xy = reference_points(4096, 123) if name.startswith("n4096") else tsplib_points(name)
        start = nn_from(xy, 0)[0]
        flat = np.ascontiguousarray(xy.reshape(-1))
        p = start.copy()
        cc, sw, mv, mk, mu = C.c_double(), C.c_long(), C.c_long(), C.c_int(), C.c_long()
        assert model().tom_descent(None, flat.ctypes.data, len(xy), 0, p, THREADS, C.byref(cc), C.byref(sw), C.byref(mv), C.byref(mk), C.byref(mu)) == 0
        ref = (golden["instances"].get(name) or golden["random"].get(name) or {}).get("two_opt", {})
        for K in (5, 8, 12):
            t0 = time.perf_counter()
            e = descent_entry(xy, start, K)
            print(json.dumps({"instance": name, "n": len(xy), "K": K, "nl_sweeps": e["sweeps"], "nl_moves": e["moves"], "nl_cost": e["cost"],
                              "polish_sweeps": e["polish_sweeps"], "polish_moves": e["polish_moves"], "polished_cost": e["polished_cost"],
                              "gap_unpolished_to_polished_pct": round(100.0 * (e["cost"] - e["polished_cost"]) / e["polished_cost"], 3),
                              "two_opt_multi_model_sweeps": sw.value, "two_opt_multi_model_cost": cc.value,
                              "reference_sweeps": ref.get("sweeps"), "reference_cost": ref.get("final_cost"),
                              "cpu_s": round(time.perf_counter() - t0, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    a = ap.parse_args()
    if a.measure:
        measure()
        return
    out = {}
    for name in ("pr1002", "fnl4461"):
        xy = tsplib_points(name)
        start = nn_from(xy, 0)[0]
        out[name] = {"n": len(xy), "start": "NN(0)", "start_sha256": digest(start), "descents": [descent_entry(xy, start, K) for K in (5, 8)]}
    xy = tsplib_points("pr1002")
    start = best_nn(xy)
    out["pr1002_best_nn"] = {"n": len(xy), "start": "best nearest-neighbour tour", "start_sha256": digest(start),
                             "descents": [descent_entry(xy, start, 8)]}
    out["n66000"] = large_entry()
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
