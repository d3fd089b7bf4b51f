#!/usr/bin/env python3
"""Golden of the don't-look model (tests/dont_look_model.c) and the CPU counts DESIGN 4.20 quotes.  CPU only.

    python tools/make_golden_dont_look.py            # writes tests/golden/golden_dont_look.json

The golden: pr1002 (EUC_2D, from the coordinates) with K = W = 8 -- the descent with looks from NN(0) with closing = 1 and with
closing = 0, then, behind the closing = 0 descent, 20 kicks at listed positions, each followed by the descent with looks
(closing = 0); per iteration the cost, the SHA-256 digest of the successor array, sweeps, moves, looked and full sweeps.  The
same loop with the plain descent (tests/three_opt_nl_model.c on the running cost) stands beside it.  The model's total `looked`
of the kicks must lie strictly below the plain loop's n x sweeps: a condition on the rule, checked here.  The generator also
searches seeds at n = 64 for a 2-opt sweep with looks in which a rejected candidate lies inside an accepted reversal, and stores
that case.  tests/test_dont_look.py imports the model wrappers below.
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_two_opt_nl as N  # noqa: E402
from make_golden_two_opt_nl import _src, digest, model_lists  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "golden_dont_look.json")
_dp = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_ip = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_bp = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")
_lp = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
_pi, _pl, _pd = C.POINTER(C.c_int), C.POINTER(C.c_long), C.POINTER(C.c_double)
FAMILIES = ("two_opt", "or_opt", "three_opt")


@functools.lru_cache(maxsize=None)
def model():
    """tests/dont_look_model.c (which includes the three plain models) compiled into a scratch directory"""
    d = tempfile.mkdtemp(prefix="dont_look_model_")
    so = os.path.join(d, "dont_look_model.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", "-o", so,
                    os.path.join(ROOT, "tests", "dont_look_model.c"), "-lm"], check=True)
    lib = C.CDLL(so)
    head = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _ip]
    lib.dlm_sweep.restype = C.c_int
    lib.dlm_sweep.argtypes = head + [C.c_int, _ip, _bp, _pd, _pi, _pi, C.c_void_p]
    lib.dlm_phase.restype = C.c_int
    lib.dlm_phase.argtypes = head + [C.c_int, C.c_int, C.c_long, _ip, _bp, _pd, _lp, _pl]
    lib.dlm_descent.restype = C.c_int
    lib.dlm_descent.argtypes = head + [C.c_int, _ip, _bp, _pd, _lp, _pi, _pi]
    lib.dlm_kick.restype = C.c_int
    lib.dlm_kick.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, _ip, C.c_int, C.c_int, C.c_int, C.c_void_p, _pd, _pd]
    return lib


def all_awake(n):
    return np.ones(3 * n, np.uint8)


def model_dl_sweep(f, path, cost, awake, nodes, width, costs=None, xy=None, kind=0):
    """one sweep with looks of family f; path and awake [3 n] in place -> dict(cost, moves, looked, Q: the looked units [n])"""
    keep, cp, xp, n = _src(costs, xy)
    nodes = np.ascontiguousarray(nodes, np.int32)
    cc, k, q = C.c_double(cost), C.c_int(), C.c_int()
    Q = np.zeros(n, np.uint8)
    rc = model().dlm_sweep(cp, xp, n, kind, nodes.shape[1], int(width), nodes.reshape(-1), f, path, awake, C.byref(cc), C.byref(k), C.byref(q),
                           Q.ctypes.data)
    assert rc == 0
    return {"cost": cc.value, "moves": k.value, "looked": q.value, "Q": Q}


def model_dl_phase(f, path, cost, awake, nodes, width, closing, max_sweeps=-1, costs=None, xy=None, kind=0):
    """the phase with looks (rule 6); path and awake in place -> dict(cost, sweeps, moves, looked, full_sweeps)"""
    keep, cp, xp, n = _src(costs, xy)
    nodes = np.ascontiguousarray(nodes, np.int32)
    cc, mv, cnt = C.c_double(cost), C.c_long(), np.zeros(4, np.int64)
    rc = model().dlm_phase(cp, xp, n, kind, nodes.shape[1], int(width), nodes.reshape(-1), f, int(closing), int(max_sweeps), path, awake,
                           C.byref(cc), cnt, C.byref(mv))
    assert rc == 0
    return {"cost": cc.value, "sweeps": int(cnt[0]), "moves": int(cnt[1]), "looked": int(cnt[2]), "full_sweeps": int(cnt[3])}


def model_dl_descent(path, cost, awake, nodes, width, closing, costs=None, xy=None, kind=0):
    """the descent with looks (rule 8) on the running cost; path and awake in place -> dict(cost, the nine counters of
    local_search_nl3, looked, full_sweeps)"""
    keep, cp, xp, n = _src(costs, xy)
    nodes = np.ascontiguousarray(nodes, np.int32)
    cc, cnt, nr, np3 = C.c_double(cost), np.zeros(12, np.int64), C.c_int(), C.c_int()
    rc = model().dlm_descent(cp, xp, n, kind, nodes.shape[1], int(width), nodes.reshape(-1), int(closing), path, awake, C.byref(cc), cnt,
                             C.byref(nr), C.byref(np3))
    assert rc == 0
    cnt = cnt.reshape(3, 4)
    return {"cost": cc.value, "two_opt_sweeps": int(cnt[0][0]), "two_opt_moves": int(cnt[0][1]), "or_sweeps": int(cnt[1][0]),
            "or_moves": int(cnt[1][1]), "rounds": nr.value, "three_sweeps": int(cnt[2][0]), "three_moves": int(cnt[2][1]),
            "three_phases": np3.value, "looked": int(cnt[:, 2].sum()), "full_sweeps": int(cnt[:, 3].sum())}


def model_kick(path, cost, i, j, k, awake=None, costs=None, xy=None, kind=0):
    """rule 9; path (and awake) in place -> (cost, delta)"""
    keep, cp, xp, n = _src(costs, xy)
    cc, d = C.c_double(cost), C.c_double()
    rc = model().dlm_kick(cp, xp, n, kind, path, int(i), int(j), int(k), awake.ctypes.data if awake is not None else None, C.byref(cc),
                          C.byref(d))
    assert rc == 0
    return cc.value, d.value


def kick_positions(n, count, seed=2024):
    """`count` sorted triples 0 <= i < j < k <= n - 1"""
    rng = np.random.default_rng(seed)
    return [tuple(int(v) for v in sorted(rng.choice(n, 3, replace=False))) for _ in range(count)]


def entry(r, path):
    keys = ("cost", "two_opt_sweeps", "two_opt_moves", "or_sweeps", "or_moves", "rounds", "three_sweeps", "three_moves", "three_phases",
            "looked", "full_sweeps")
    out = {k: r[k] for k in keys if k in r}
    out["sweeps"] = r["two_opt_sweeps"] + r["or_sweeps"] + r["three_sweeps"]
    out["moves"] = r["two_opt_moves"] + r["or_moves"] + r["three_moves"]
    out["path_sha256"] = digest(path)
    return out


def plain_descent_running(path, cost, nodes, width, xy):
    """the plain descent of rule 10 of "Neighbour-list 3-opt" on the running cost (the slot form)"""
    from make_golden_three_opt_nl import model_ls3_descent
    before = float(N.euc(xy, np.arange(len(path)), path).sum())
    r = model_ls3_descent(path, nodes, width, xy=xy)
    r.pop("first"); r.pop("max_moves")
    r["cost"] = cost + (r["cost"] - before)     # integer weights: exact
    return r


def loop(name="pr1002", K=8, W=8, kicks=20):
    xy = N.tsplib_points(name)
    n = len(xy)
    nodes, _ = model_lists(K, xy=xy)
    start, cost0 = N.nn_from(xy, 0)
    out = {"n": n, "K": K, "W": W, "start": "NN(0)", "start_sha256": digest(start), "start_cost": float(cost0),
           "kicks": kick_positions(n, kicks)}
    for closing in (1, 0):
        path, awake = start.copy(), all_awake(n)
        r = model_dl_descent(path, float(cost0), awake, nodes, W, closing, xy=xy)
        out["descent_closing%d" % closing] = entry(r, path)
    its, cost = [], r["cost"]                   # the kicks go on from the closing = 0 descent
    for i, j, k in out["kicks"]:
        cost, delta = model_kick(path, cost, i, j, k, awake, xy=xy)
        r = model_dl_descent(path, cost, awake, nodes, W, 0, xy=xy)
        cost = r["cost"]
        its.append(dict(entry(r, path), kick_delta=delta))
    out["iterations"] = its
    path = start.copy()
    r = plain_descent_running(path, float(cost0), nodes, W, xy)
    out["plain_descent"] = entry(r, path)
    pits, cost = [], r["cost"]
    for i, j, k in out["kicks"]:
        cost, delta = model_kick(path, cost, i, j, k, xy=xy)
        r = plain_descent_running(path, cost, nodes, W, xy)
        cost = r["cost"]
        pits.append(dict(entry(r, path), kick_delta=delta))
    out["plain_iterations"] = pits
    looked = sum(it["looked"] for it in its)
    plain_units = n * sum(it["sweeps"] for it in pits)
    assert looked < plain_units, (looked, plain_units)
    out["kicks_looked"] = looked
    out["kicks_plain_units"] = plain_units
    return out


def rejected_inside_reversal(n=64, K=5, seeds=range(400)):
    """a seed at n = 64 (uniform integer points, EUC_2D, a random tour) and the first 2-opt sweep with looks from all awake in
    which a candidate that was not accepted has its node a strictly inside the positions of an accepted reversal"""
    from make_golden_two_opt_nl import model_sweep
    for seed in seeds:
        rng = np.random.default_rng(seed)
        xy = rng.integers(0, 1000, (n, 2)).astype(np.float64)
        nodes, _ = model_lists(K, xy=xy)
        perm = rng.permutation(n)
        path = np.empty(n, np.int32)
        path[perm] = np.roll(perm, -1)
        r = model_sweep(path.copy(), 0.0, nodes, xy=xy)
        acc = [c for c, a in zip(r["cand"], r["acc"]) if a]
        rej = [c for c, a in zip(r["cand"], r["acc"]) if not a]
        P = np.empty(n, np.int64)
        v = 0
        for p in range(n):
            P[v] = p
            v = int(path[v])
        for _, a, b, i, j in rej:
            for _, _, _, ai, aj in acc:
                if ai < min(P[a], P[b]) and max(P[a], P[b]) < aj:
                    return {"n": n, "K": K, "seed": int(seed), "rejected": [int(a), int(b)], "inside": [int(ai), int(aj)],
                            "start_sha256": digest(path)}
    raise SystemExit("no seed shows a rejected candidate inside an accepted reversal")


def main():
    out = {"pr1002": loop(), "rejected_inside_reversal": rejected_inside_reversal()}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    p = out["pr1002"]
    print(json.dumps({"kicks_looked": p["kicks_looked"], "kicks_plain_units": p["kicks_plain_units"],
                      "ratio": p["kicks_plain_units"] / p["kicks_looked"],
                      "descent_looked": p["descent_closing1"]["looked"], "descent_sweeps": p["descent_closing1"]["sweeps"],
                      "plain_descent_sweeps": p["plain_descent"]["sweeps"], "costs": [p["descent_closing1"]["cost"],
                      p["descent_closing0"]["cost"], p["plain_descent"]["cost"]], "case": out["rejected_inside_reversal"]}))


if __name__ == "__main__":
    main()
