#!/usr/bin/env python3
"""Golden of the neighbour-list Or-opt model (tests/or_opt_nl_model.c) and the CPU counts DESIGN 4.15 quotes.  CPU only.

    python tools/make_golden_or_opt_nl.py            # writes tests/golden/golden_or_opt_nl.json
    python tools/make_golden_or_opt_nl.py --measure  # prints the table of DESIGN 4.15 (K = 5, 8, 12)

The golden: pr1002 from NN(0) with K = 5 and K = 8 -- the counters, the cost and the SHA-256 digest of the successor array of
the descent of rule 8; pr1002 with K = 8 from the best nearest-neighbour tour, and from the 2-opt local optimum ref_2opt makes of
that tour (what `TSP_OR_OPT=1 tsp -alg VNS -k 1` hands to its polish); and 66 000 uniform integer points (seed 66000, EUC_2D, K = 8): the first three Or-opt sweeps from the stripe tour.
tests/test_or_opt_nl.py imports the model wrappers below.
"""
import argparse
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_two_opt_nl as N  # noqa: E402
from make_golden_two_opt_nl import _src, digest, model_lists  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "golden_or_opt_nl.json")
_dp = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_ip = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_pi, _pl, _pd = C.POINTER(C.c_int), C.POINTER(C.c_long), C.POINTER(C.c_double)


@functools.lru_cache(maxsize=None)
def model():
    """tests/or_opt_nl_model.c (which includes two_opt_nl_model.c) compiled into a scratch directory"""
    d = tempfile.mkdtemp(prefix="or_opt_nl_model_")
    so = os.path.join(d, "or_opt_nl_model.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", "-o", so,
                    os.path.join(ROOT, "tests", "or_opt_nl_model.c"), "-lm"], check=True)
    lib = C.CDLL(so)
    lib.onl_sweep.restype = C.c_int
    lib.onl_sweep.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _ip, _ip,
                              _dp, _ip, _pi, _ip, _ip, _ip, _ip, _dp, _ip, _pi, _ip, _dp, _pd, C.c_int]
    lib.onl_descent.restype = C.c_int
    lib.onl_descent.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _ip, _ip, C.c_long, _pd, _pl, _pl, _pl, _pl, _pi, _pi]
    return lib


def unpack(pk):
    """the packed (L, q, rev) of a candidate -> (L, q, rev)"""
    return int(pk) >> 18, (int(pk) >> 1) & 0x1ffff, int(pk) & 1


def model_or_sweep(path, cost, nodes, costs=None, xy=None, kind=0, apply=True):
    """one Or-opt sweep of the C model over the lists `nodes`; path in place when apply ->
    dict(cost, moves [k][4] (s, L, q, rev), deltas [k], raw_d, raw_b (packed, -1: none), cand [(delta, s, packed, lo, hi)], acc)"""
    keep, cp, xp, n = _src(costs, xy)
    nodes = np.ascontiguousarray(nodes, np.int32)
    raw_d, cdl, deltas = np.empty(n), np.empty(n), np.empty(n)
    raw_b, cs, cb, ci, cj, acc = (np.empty(n, np.int32) for _ in range(6))
    mv = np.empty(4 * n, np.int32)
    m, k, cc = C.c_int(), C.c_int(), C.c_double(cost)
    rc = model().onl_sweep(cp, xp, n, kind, nodes.shape[1], nodes.reshape(-1), path, raw_d, raw_b, C.byref(m), cs, cb, ci, cj, cdl, acc,
                           C.byref(k), mv, deltas, C.byref(cc), 1 if apply else 0)
    assert rc == 0
    m, k = m.value, k.value
    cand = [(float(cdl[x]), int(cs[x]), int(cb[x]), int(ci[x]), int(cj[x])) for x in range(m)]
    return {"cost": cc.value, "moves": mv[:4 * k].reshape(-1, 4).copy(), "deltas": deltas[:k].copy(), "raw_d": raw_d, "raw_b": raw_b,
            "cand": cand, "acc": [int(v) for v in acc[:m]]}


def model_ls_descent(path, nodes, costs=None, xy=None, kind=0, limit_sweeps=0):
    """the descent of rule 8 in the C model; path in place ->
    dict(cost, two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, rounds, max_moves)"""
    keep, cp, xp, n = _src(costs, xy)
    nodes = np.ascontiguousarray(nodes, np.int32)
    cc, tw, tm, os_, om, nr, mk = C.c_double(), C.c_long(), C.c_long(), C.c_long(), C.c_long(), C.c_int(), C.c_int()
    rc = model().onl_descent(cp, xp, n, kind, nodes.shape[1], nodes.reshape(-1), path, limit_sweeps, C.byref(cc), C.byref(tw), C.byref(tm),
                             C.byref(os_), C.byref(om), C.byref(nr), C.byref(mk))
    assert rc == 0, "the model's descent did not end (rc %d)" % rc
    return {"cost": cc.value, "two_opt_sweeps": tw.value, "two_opt_moves": tm.value, "or_sweeps": os_.value, "or_moves": om.value,
            "rounds": nr.value, "max_moves": mk.value}


def descent_entry(xy, start, K):
    """the golden's record of one descent (EUC_2D, from the coordinates)"""
    nodes, _ = model_lists(K, xy=xy)
    path = start.copy()
    r = model_ls_descent(path, nodes, xy=xy)
    return dict(r, K=K, path_sha256=digest(path))


def two_opt_descent(xy, path):
    """ref_2opt on the EUC_2D weights (include/tspgpu.h, tspgpu_two_opt): per sweep the first strict minimum of delta(a, b) over
    a < b in row order, applied while it is below -1e-7; path in place -> (sweeps, cost)"""
    n = len(xy)
    idx = np.arange(n)
    c = N.euc(xy, idx[:, None], idx[None, :]).astype(np.float64)
    upper = idx[:, None] < idx[None, :]
    sweeps = 0
    while True:
        sa = path.astype(np.int64)
        here = c[idx, sa]
        d = (c + c[sa][:, sa]) - (here[:, None] + here[None, :])
        ok = upper & (sa[:, None] != sa[None, :]) & (idx[:, None] != sa[None, :]) & (idx[None, :] != sa[:, None])
        d = np.where(ok, d, np.inf)
        a, b = divmod(int(np.argmin(d)), n)
        sweeps += 1
        if not d[a, b] < -1.0e-7:
            return sweeps, float(c[idx, path].sum())
        prev = np.empty(n, np.int64)
        prev[path] = idx
        first, last, v = int(path[a]), int(path[b]), b
        path[a] = b
        while v != first:
            path[v] = prev[v]
            v = int(prev[v])
        path[first] = last


def large_entry(n=66000, seed=66000, K=8, sweeps=3):
    xy = N.large_points(n, seed)
    nodes, _ = model_lists(K, xy=xy)
    path = N.stripe_tour(xy)
    start = digest(path)
    cost = float(N.euc(xy, np.arange(n), path).sum())
    out = {"n": n, "seed": seed, "K": K, "kind": "EUC_2D", "start": "stripe_tour(width 300)", "start_sha256": start, "start_cost": cost,
           "lists_sha256": digest(nodes), "sweeps": []}
    for _ in range(sweeps):
        r = model_or_sweep(path, cost, nodes, xy=xy)
        cost = r["cost"]
        out["sweeps"].append({"candidates": len(r["cand"]), "moves": len(r["moves"]), "delta_sum": float(r["deltas"].sum()), "cost": cost,
                              "moves_sha256": digest(r["moves"]), "path_sha256": digest(path), "max_label": int(r["moves"][:, [0, 2]].max())})
    return out


def measure():
    for name in ("pr1002", "fnl4461", "n4096_s123"):
        xy = N.reference_points(4096, 123) if name.startswith("n4096") else N.tsplib_points(name)
        start = N.nn_from(xy, 0)[0]
        for K in (5, 8, 12):
            t0 = time.perf_counter()
            nodes, _ = model_lists(K, xy=xy)
            only2 = start.copy()
            two = N.model_descent(only2, nodes, False, xy=xy)
            e = descent_entry(xy, start, K)
            print(json.dumps({"instance": name, "n": len(xy), "K": K, "two_opt_nl_cost": two["cost"], "two_opt_sweeps": e["two_opt_sweeps"],
                              "two_opt_moves": e["two_opt_moves"], "or_sweeps": e["or_sweeps"], "or_moves": e["or_moves"],
                              "rounds": e["rounds"], "max_moves_per_or_sweep": e["max_moves"], "cost": e["cost"],
                              "gain_over_two_opt_nl_pct": round(100.0 * (two["cost"] - e["cost"]) / two["cost"], 3),
                              "cpu_s": round(time.perf_counter() - t0, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    a = ap.parse_args()
    if a.measure:
        measure()
        return
    out = {}
    xy = N.tsplib_points("pr1002")
    start = N.nn_from(xy, 0)[0]
    out["pr1002"] = {"n": len(xy), "start": "NN(0)", "start_sha256": digest(start), "descents": [descent_entry(xy, start, K) for K in (5, 8)]}
    start = N.best_nn(xy)
    out["pr1002_best_nn"] = {"n": len(xy), "start": "best nearest-neighbour tour", "start_sha256": digest(start),
                             "descents": [descent_entry(xy, start, 8)]}
    sweeps, cost = two_opt_descent(xy, start)
    out["pr1002_best_nn_two_opt"] = {"n": len(xy), "start": "ref_2opt on the best nearest-neighbour tour", "two_opt_sweeps": sweeps,
                                     "start_cost": cost, "start_sha256": digest(start), "descents": [descent_entry(xy, start, 8)]}
    out["n66000"] = large_entry()
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
