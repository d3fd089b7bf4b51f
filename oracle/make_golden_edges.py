#!/usr/bin/env python3
"""Golden vectors for the matrix-free path at the top of its label range: n = 131 071 (k_sweep_otf8, 17-bit labels up to
0x1fffe) and n = 131 072 (the engine's largest n, k_sweep_otf), uniform integer points in a square of side 23 000 (EUC_2D
weights below 32 767: the NN grid kernel packs (weight << 17 | node) into one 32-bit key, node 131 071 next to its "none"
key).  From the oracle: the NN(0) tour (cost and FNV-1a digest) and the first 3 best-improvement moves.  The instances are
regenerated from (n, side, seed) by edge_points() -- the recipe tests/test_gpu_edges.py repeats.
Takes ~5 minutes of CPU.  Writes tests/golden/golden_edges.json."""
import json, os, sys, time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import oracle as O
ROOT = os.path.dirname(HERE)
SIDE = 23000
SIZES = (131071, 131072)


def edge_points(n, side, seed):
    """n integer points in [0, side]^2, the two corners first (they fix the bounding box)"""
    r = np.random.RandomState(seed)
    return np.ascontiguousarray(np.concatenate([[[0.0, 0.0], [side, side]], r.randint(0, side + 1, size=(n - 2, 2))]).astype(np.float64))


def one(n):
    t0 = time.time()
    xy = edge_points(n, SIDE, n)
    succ, nn_cost = O.nn_tour_xy(xy, O.EUC_2D, 0)
    print(n, "nn", nn_cost, round(time.time() - t0, 1), flush=True)
    g = {"n": n, "side": SIDE, "seed": n, "kind": "EUC_2D", "nn_cost": nn_cost, "nn_fnv": f"{O.fnv1a(succ):016x}", "moves": []}
    cost = nn_cost
    for s in range(3):
        d, mv = O.two_opt_best_move_xy(xy, O.EUC_2D, succ, threads=4)
        assert d < -1e-7
        O.apply_move(succ, None, mv[0], mv[1])
        cost += d
        g["moves"].append({"a": mv[0], "b": mv[1], "delta": d, "cost": cost, "fnv": f"{O.fnv1a(succ):016x}"})
        print(n, "sweep", s, mv, d, cost, round(time.time() - t0, 1), flush=True)
    assert cost == O.tour_cost_xy(xy, O.EUC_2D, succ)
    return g


if __name__ == "__main__":
    with ProcessPoolExecutor(len(SIZES)) as ex:
        res = list(ex.map(one, SIZES))
    out = {"_generator": "oracle/make_golden_edges.py (oracle, EUC_2D)"}
    for g in res:
        out[f"n{g['n']}"] = g
    json.dump(out, open(os.path.join(ROOT, "tests", "golden", "golden_edges.json"), "w"), indent=1)
    print("done")
