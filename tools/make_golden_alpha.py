#!/usr/bin/env python3
"""Golden of the alpha-nearness model (tests/alpha_model.c).  CPU only.

    python tools/make_golden_alpha.py            # writes tests/golden/golden_alpha.json

The golden: on berlin52, kroA100, att48, eil51 and pr1002, at pi = 0 and at the pi* of tests/golden/golden_held_karp.json (the model's
ascent is run again and its digest compared), for K = 5 and 8 the SHA-256 digest of the lists' nodes, and alpha of eight fixed pairs
(numpy default_rng(n): a permutation's first 16 nodes, paired).  tests/test_alpha_nearness.py imports the model wrappers below.
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
from make_golden_two_opt_nl import _src, digest  # noqa: E402
from make_golden_held_karp import _pi_arg, digest64, model_ascent, tsplib_instance  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "golden_alpha.json")
HK_GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_held_karp.json")
INSTANCES = ("berlin52", "kroA100", "att48", "eil51", "pr1002")
KS = (5, 8)
_lp = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
_ip = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")


@functools.lru_cache(maxsize=None)
def model():
    """tests/alpha_model.c (which includes held_karp_model.c) compiled into a scratch directory"""
    d = tempfile.mkdtemp(prefix="alpha_model_")
    so = os.path.join(d, "alpha_model.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", "-o", so,
                    os.path.join(ROOT, "tests", "alpha_model.c"), "-lm"], check=True)
    lib = C.CDLL(so)
    lib.alm_all_pairs.restype = C.c_int
    lib.alm_all_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, _lp]
    lib.alm_row.restype = C.c_int
    lib.alm_row.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, _ip, C.c_int, _lp, _lp]
    lib.alm_lists.restype = C.c_int
    lib.alm_lists.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, _ip, _lp]
    return lib


def model_alpha(costs=None, xy=None, kind=0, pi=None):
    """alpha of every ordered pair -> [n][n] int64, the diagonal 0"""
    keep, cp, xp, n = _src(costs, xy)
    keep_pi, pp = _pi_arg(pi, n)
    out = np.empty((n, n), np.int64)
    rc = model().alm_all_pairs(cp, xp, n, kind, pp, out.reshape(-1))
    assert rc == 0, rc
    return out


def model_alpha_row(edges, v, costs=None, xy=None, kind=0, pi=None):
    """alpha(v, .) and c[v][.] over the 1-tree `edges` [n][2] -> (alpha [n] int64, cost [n] int64; cost[v] = -1)"""
    keep, cp, xp, n = _src(costs, xy)
    keep_pi, pp = _pi_arg(pi, n)
    edges = np.ascontiguousarray(edges, np.int32).reshape(-1)
    al, co = np.empty(n, np.int64), np.empty(n, np.int64)
    rc = model().alm_row(cp, xp, n, kind, pp, edges, int(v), al, co)
    assert rc == 0, rc
    return al, co


def model_alpha_lists(K, costs=None, xy=None, kind=0, pi=None):
    """A(v) of rule 3 -> (nodes [n][K'] int32, costs [n][K'] int64)"""
    keep, cp, xp, n = _src(costs, xy)
    keep_pi, pp = _pi_arg(pi, n)
    kp = min(K, n - 1)
    nodes, co = np.empty((n, kp), np.int32), np.empty((n, kp), np.int64)
    rc = model().alm_lists(cp, xp, n, kind, pp, int(K), nodes.reshape(-1), co.reshape(-1))
    assert rc == 0, rc
    return nodes, co


def row_list(al, co, v, K):
    """the K' first of row v under the key (alpha, c, u) -> nodes"""
    u = np.array([x for x in range(len(al)) if x != v])
    order = np.lexsort((u, co[u], al[u]))
    return u[order[:min(K, len(u))]].astype(np.int32)


def golden_pairs(n):
    return np.random.default_rng(n).permutation(n)[:16].reshape(8, 2).astype(np.int32)


def star_pi(name):
    """pi* of the Held-Karp golden: the model's ascent again, its digest checked"""
    g = json.load(open(HK_GOLDEN))["ascent"][name]
    xy, kind = tsplib_instance(name)
    r = model_ascent(g["upper"], g["iters_asked"], g["patience"], xy=xy, kind=kind)
    assert digest64(r["pi"]) == g["pi_sha256"], name
    return r["pi"]


def entry(name):
    xy, kind = tsplib_instance(name)
    n = len(xy)
    pairs = golden_pairs(n)
    out = {"instance": name, "n": n, "kind": kind, "pairs": pairs.tolist()}
    for tag, pi in (("zero", None), ("star", star_pi(name))):
        rows = {int(a): model_alpha_row(_edges(xy, kind, pi), int(a), xy=xy, kind=kind, pi=pi)[0] for a in pairs[:, 0]}
        e = {"alpha": [int(rows[int(a)][int(b)]) for a, b in pairs]}
        for K in KS:
            nodes, co = model_alpha_lists(K, xy=xy, kind=kind, pi=pi)
            e["K%d" % K] = {"nodes_sha256": digest(nodes), "costs_sha256": digest64(co)}
        out[tag] = e
    return out


def _edges(xy, kind, pi):
    from make_golden_held_karp import model_one_tree
    return model_one_tree(xy=xy, kind=kind, pi=pi)["edges"]


def build():
    return {name: entry(name) for name in INSTANCES}


def main():
    out = build()
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
