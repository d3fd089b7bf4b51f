#!/usr/bin/env python3
"""Golden of the neighbour-list 3-opt model (tests/three_opt_nl_model.c) and the CPU counts DESIGN 4.19 quotes.  CPU only.

    python tools/make_golden_three_opt_nl.py            # writes tests/golden/golden_three_opt_nl.json
    python tools/make_golden_three_opt_nl.py --measure  # prints the counts of DESIGN 4.19

The golden: kroA100 and pr1002 from NN(0) with K = 8 and W = 5, 8 -- the counters, the cost and the SHA-256 digest of the
successor array of the descent of rule 10, and the state at the end of its first rule-8 part; and 66 000 uniform integer points
(seed 66000, EUC_2D, K = 8, W = 8): the first three 3-opt sweeps from the stripe tour.
tests/test_three_opt_nl.py imports the model wrappers below.
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
from make_golden_or_opt_nl import model_ls_descent  # noqa: E402
from make_golden_two_opt_nl import _src, digest, model_lists  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "golden_three_opt_nl.json")
_dp = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_ip = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_pi, _pl, _pd = C.POINTER(C.c_int), C.POINTER(C.c_long), C.POINTER(C.c_double)


@functools.lru_cache(maxsize=None)
def model():
    """tests/three_opt_nl_model.c (which includes or_opt_nl_model.c) compiled into a scratch directory"""
    d = tempfile.mkdtemp(prefix="three_opt_nl_model_")
    so = os.path.join(d, "three_opt_nl_model.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", "-o", so,
                    os.path.join(ROOT, "tests", "three_opt_nl_model.c"), "-lm"], check=True)
    lib = C.CDLL(so)
    lib.t3m_sweep.restype = C.c_int
    lib.t3m_sweep.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip,
                              _dp, _ip, _pi, _ip, _ip, _ip, _ip, _dp, _ip, _pi, _ip, _dp, _pd, C.c_int]
    lib.t3m_descent.restype = C.c_int
    lib.t3m_descent.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, C.c_long, _pd,
                                _pl, _pl, _pl, _pl, _pi, _pl, _pl, _pi, _pi, _ip, _dp]
    return lib


def pack(s2, j3, s4, j5, s6):
    return 1 << 30 | s2 << 10 | j3 << 6 | s4 << 5 | j5 << 1 | s6


def unpack(code):
    """the code of a chain -> (s2, j3, s4, j5, s6)"""
    code = int(code)
    return (code >> 10) & 1, (code >> 6) & 15, (code >> 5) & 1, (code >> 1) & 15, code & 1


def model_three_sweep(path, cost, nodes, width, costs=None, xy=None, kind=0, apply=True):
    """one 3-opt sweep of the C model over the first min(width, K') entries of the lists `nodes`; path in place when apply ->
    dict(cost, moves [k][4] (i, j, k, kind), deltas [k], raw_d, raw_b (the code, -1: none), cand [(delta, t1, code, i, k)], acc)"""
    keep, cp, xp, n = _src(costs, xy)
    nodes = np.ascontiguousarray(nodes, np.int32)
    raw_d, cdl, deltas = np.empty(n), np.empty(n), np.empty(n)
    raw_b, cs, cb, ci, cj, acc = (np.empty(n, np.int32) for _ in range(6))
    mv = np.empty(4 * n, np.int32)
    m, k, cc = C.c_int(), C.c_int(), C.c_double(cost)
    rc = model().t3m_sweep(cp, xp, n, kind, nodes.shape[1], int(width), nodes.reshape(-1), path, raw_d, raw_b, C.byref(m), cs, cb, ci, cj,
                           cdl, acc, C.byref(k), mv, deltas, C.byref(cc), 1 if apply else 0)
    assert rc == 0
    m, k = m.value, k.value
    cand = [(float(cdl[x]), int(cs[x]), int(cb[x]), int(ci[x]), int(cj[x])) for x in range(m)]
    return {"cost": cc.value, "moves": mv[:4 * k].reshape(-1, 4).copy(), "deltas": deltas[:k].copy(), "raw_d": raw_d, "raw_b": raw_b,
            "cand": cand, "acc": [int(v) for v in acc[:m]]}


def model_ls3_descent(path, nodes, width, costs=None, xy=None, kind=0, limit_sweeps=0):
    """the descent of rule 10 in the C model; path in place -> dict(cost, two_opt_sweeps, two_opt_moves, or_sweeps, or_moves,
    rounds, three_sweeps, three_moves, three_phases, max_moves, first: the same six and the path at the end of the first
    rule-8 part)"""
    keep, cp, xp, n = _src(costs, xy)
    nodes = np.ascontiguousarray(nodes, np.int32)
    cc, tw, tm, os_, om, nr = C.c_double(), C.c_long(), C.c_long(), C.c_long(), C.c_long(), C.c_int()
    ts, tmv, tp, mk = C.c_long(), C.c_long(), C.c_int(), C.c_int()
    fpath, first = np.empty(n, np.int32), np.zeros(6)
    rc = model().t3m_descent(cp, xp, n, kind, nodes.shape[1], int(width), nodes.reshape(-1), path, limit_sweeps, C.byref(cc),
                             C.byref(tw), C.byref(tm), C.byref(os_), C.byref(om), C.byref(nr), C.byref(ts), C.byref(tmv), C.byref(tp),
                             C.byref(mk), fpath, first)
    assert rc == 0, "the model's descent did not end (rc %d)" % rc
    return {"cost": cc.value, "two_opt_sweeps": tw.value, "two_opt_moves": tm.value, "or_sweeps": os_.value, "or_moves": om.value,
            "rounds": nr.value, "three_sweeps": ts.value, "three_moves": tmv.value, "three_phases": tp.value, "max_moves": mk.value,
            "first": {"cost": float(first[0]), "two_opt_sweeps": int(first[1]), "two_opt_moves": int(first[2]), "or_sweeps": int(first[3]),
                      "or_moves": int(first[4]), "rounds": int(first[5]), "path": fpath}}


def descent_entry(xy, start, K, width):
    """the golden's record of one descent (EUC_2D, from the coordinates)"""
    nodes, _ = model_lists(K, xy=xy)
    path = start.copy()
    r = model_ls3_descent(path, nodes, width, xy=xy)
    first = r.pop("first")
    first["path_sha256"] = digest(first.pop("path"))
    return dict(r, K=K, W=width, path_sha256=digest(path), first=first)


def large_entry(n=66000, seed=66000, K=8, width=8, sweeps=3):
    xy = N.large_points(n, seed)
    nodes, _ = model_lists(K, xy=xy)
    path = N.stripe_tour(xy)
    start = digest(path)
    cost = float(N.euc(xy, np.arange(n), path).sum())
    out = {"n": n, "seed": seed, "K": K, "W": width, "kind": "EUC_2D", "start": "stripe_tour(width 300)", "start_sha256": start,
           "start_cost": cost, "lists_sha256": digest(nodes), "sweeps": []}
    for _ in range(sweeps):
        r = model_three_sweep(path, cost, nodes, width, xy=xy)
        cost = r["cost"]
        out["sweeps"].append({"candidates": len(r["cand"]), "moves": len(r["moves"]), "delta_sum": float(r["deltas"].sum()), "cost": cost,
                              "moves_sha256": digest(r["moves"]), "path_sha256": digest(path),
                              "kinds": sorted({int(v) for v in r["moves"][:, 3]})})
    return out


def measure():
    """the table of DESIGN 4.19: at the rule-8 optimum from NN(0), K = 8, the improving candidates of one 3-opt sweep, the distinct
    moves among them, and the 3-opt phase alone run from there"""
    for name, widths in (("berlin52", (8,)), ("kroA100", (8,)), ("pr1002", (5, 8))):
        xy = N.tsplib_points(name)
        nodes, _ = model_lists(8, xy=xy)
        opt = N.nn_from(xy, 0)[0]
        base = model_ls_descent(opt, nodes, xy=xy)
        for W in widths:
            t0 = time.perf_counter()
            r = model_three_sweep(opt.copy(), base["cost"], nodes, W, xy=xy, apply=False)
            path, cost, sweeps, moves = opt.copy(), base["cost"], 0, 0
            while True:
                s = model_three_sweep(path, cost, nodes, W, xy=xy)
                cost, sweeps, moves = s["cost"], sweeps + 1, moves + len(s["moves"])
                if not len(s["moves"]):
                    break
            full = descent_entry(xy, N.nn_from(xy, 0)[0], 8, W)
            print(json.dumps({"instance": name, "n": len(xy), "K": 8, "W": W, "rule8_cost": base["cost"], "improving_candidates": len(r["cand"]),
                              "distinct_ranges": len({c[3:] for c in r["cand"]}), "accepted_first_sweep": len(r["moves"]),
                              "phase_sweeps": sweeps, "phase_moves": moves, "phase_cost": cost, "descent_cost": full["cost"],
                              "descent_three_moves": full["three_moves"], "descent_three_phases": full["three_phases"],
                              "cpu_s": round(time.perf_counter() - t0, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    a = ap.parse_args()
    if a.measure:
        measure()
        return
    out = {}
    for name in ("kroA100", "pr1002"):
        xy = N.tsplib_points(name)
        start = N.nn_from(xy, 0)[0]
        out[name] = {"n": len(xy), "start": "NN(0)", "start_sha256": digest(start),
                     "descents": [descent_entry(xy, start, 8, W) for W in (5, 8)]}
    out["n66000"] = large_entry()
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
