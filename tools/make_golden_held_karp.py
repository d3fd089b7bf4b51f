#!/usr/bin/env python3
"""Golden of the Held-Karp lower bound model (tests/held_karp_model.c).  CPU only.

    python tools/make_golden_held_karp.py            # writes tests/golden/golden_held_karp.json

The golden: the ascent (300 iterations, patience 10) on berlin52, kroA100, eil51, att48 and pr1002 from the upper bounds below --
bound, reason, iterations, final h, the best L, L at pi = 0, the SHA-256 digest of pi* and, on reason 1, of the tour and its
cost; and one 1-tree each on fnl4461 and pla85900 at pi = 0 and at a fixed random pi (numpy default_rng(seed), integers in
+-2^20) -- L and the digest of the edge array.  tests/test_held_karp.py imports the model wrappers below.
"""
import ctypes as C
import functools
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_two_opt_nl import _src, digest  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "golden_held_karp.json")
DATA = os.path.join(ROOT, "tests", "golden", "data")
S = 128
ASCENTS = (("berlin52", 8980), ("kroA100", 27807), ("eil51", 450), ("att48", 12000), ("pr1002", 275427))
OPTIMA = {"berlin52": 7542, "kroA100": 21282, "eil51": 426, "att48": 10628, "pr1002": 259045}
TREES = (("fnl4461", 4461), ("pla85900", 85900))        # (instance, seed of the fixed pi)
ITERS, PATIENCE = 300, 10
_lp = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
_ip = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_pi, _pll = C.POINTER(C.c_int), C.POINTER(C.c_longlong)


@functools.lru_cache(maxsize=None)
def model():
    """tests/held_karp_model.c (which includes two_opt_multi_model.c) compiled into a scratch directory"""
    d = tempfile.mkdtemp(prefix="held_karp_model_")
    so = os.path.join(d, "held_karp_model.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", "-o", so,
                    os.path.join(ROOT, "tests", "held_karp_model.c"), "-lm"], check=True)
    lib = C.CDLL(so)
    lib.hkm_one_tree.restype = C.c_int
    lib.hkm_one_tree.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, _ip, _ip, _pll]
    lib.hkm_ascent.restype = C.c_int
    lib.hkm_ascent.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_void_p, _pll, _lp, _ip, _pi, _pi, _pi]
    return lib


def digest64(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.int64).tobytes()).hexdigest()


def bound_of(best):
    return -((-int(best)) // S)             # ceil(best / S)


def _pi_arg(pi, n):
    if pi is None:
        return None, None
    pi = np.ascontiguousarray(pi, np.int64)
    assert pi.shape == (n,)
    return pi, pi.ctypes.data


def model_one_tree(costs=None, xy=None, kind=0, pi=None):
    """T(pi) -> dict(L, edges [n][2] ascending by pair, deg [n])"""
    keep, cp, xp, n = _src(costs, xy)
    keep_pi, pp = _pi_arg(pi, n)
    edges, deg, L = np.empty(2 * n, np.int32), np.empty(n, np.int32), C.c_longlong()
    rc = model().hkm_one_tree(cp, xp, n, kind, pp, edges, deg, C.byref(L))
    assert rc == 0, rc
    return {"L": L.value, "edges": edges.reshape(n, 2), "deg": deg}


def model_ascent(upper, iters=ITERS, patience=PATIENCE, costs=None, xy=None, kind=0, pi=None):
    """rule 3 -> dict(bound, best, reason, iters, h, pi [n] int64, path [n] (reason 1 only))"""
    keep, cp, xp, n = _src(costs, xy)
    keep_pi, pp = _pi_arg(pi, n)
    out, path = np.zeros(n, np.int64), np.full(n, -1, np.int32)
    best, it, why, h = C.c_longlong(), C.c_int(), C.c_int(), C.c_int()
    rc = model().hkm_ascent(cp, xp, n, kind, int(upper), iters, patience, pp, C.byref(best), out, path, C.byref(it), C.byref(why), C.byref(h))
    assert rc == 0, rc
    r = {"bound": bound_of(best.value), "best": best.value, "reason": why.value, "iters": it.value, "h": h.value, "pi": out}
    if why.value == 1:
        r["path"] = path
    return r


def tsplib_instance(name):
    """-> (xy, kind) of a file of tests/golden/data"""
    from travellingsalesmanoptimization_amd.tsplib import read as read_tsplib
    xy, kind = read_tsplib(os.path.join(DATA, name + ".tsp"))[:2]
    return np.asarray(xy, dtype=np.float64), int(kind)


def fixed_pi(n, seed):
    return np.random.default_rng(seed).integers(-(1 << 20), (1 << 20) + 1, n).astype(np.int64)


def ascent_entry(name, upper):
    xy, kind = tsplib_instance(name)
    r = model_ascent(upper, xy=xy, kind=kind)
    e = {"instance": name, "n": len(xy), "kind": kind, "upper": upper, "iters_asked": ITERS, "patience": PATIENCE, "bound": r["bound"],
         "best": r["best"], "reason": r["reason"], "iters": r["iters"], "h": r["h"], "pi_sha256": digest64(r["pi"]),
         "L0": model_one_tree(xy=xy, kind=kind)["L"], "optimum": OPTIMA[name]}
    if r["reason"] == 1:
        assert r["best"] % S == 0           # (a tour's L is S times its cost)
        e["path_sha256"] = digest(r["path"])
        e["tour_cost"] = r["best"] // S
    return e


def tree_entry(name, seed):
    xy, kind = tsplib_instance(name)
    out = {"instance": name, "n": len(xy), "kind": kind, "seed": seed}
    for tag, pi in (("zero", None), ("fixed", fixed_pi(len(xy), seed))):
        r = model_one_tree(xy=xy, kind=kind, pi=pi)
        out[tag] = {"L": r["L"], "edges_sha256": digest(r["edges"])}
    return out


def build():
    return {"ascent": {name: ascent_entry(name, ub) for name, ub in ASCENTS}, "tree": {name: tree_entry(name, seed) for name, seed in TREES}}


def main():
    out = build()
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
