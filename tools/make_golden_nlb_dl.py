#!/usr/bin/env python3
"""Golden of the walks with don't-look bits (include/tspgpu.h "Batched don't-look bits").  CPU only, from the
project's models alone.

    python tools/make_golden_nlb_dl.py            # writes tests/golden/golden_nlb_dl.json

The model of a walk with looks is make_golden_vns_nl.model_walk -- its kicks, its incumbent, its trace -- with the descent of
tests/dont_look_model.c (model_dl_descent) in step 1 and the difference rule in the place of rule 7: behind a kick phase the
three sets hold exactly the nodes whose unordered pair of tour neighbours differs from the local optimum's.  The first descent
of a walk starts all awake.  The golden: pr1002 (EUC_2D), K = W = 8, 8 walks of 6 iterations from NN(0), closing 0 and 1; per walk
the totals, `looked` and the full sweeps, the trace, the numbers consumed and the digests of tour and incumbent.
tests/test_nlb_dl.py imports the wrappers below.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_two_opt_nl as N  # noqa: E402
import make_golden_vns_nl as GV  # noqa: E402
from make_golden_dont_look import all_awake, model_dl_descent  # noqa: E402
from make_golden_two_opt_nl import digest, model_lists  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "golden_nlb_dl.json")
K = W = 8
WALKS, ITERATIONS = 8, 6
TOTALS = GV.TOTALS + GV.THREE_TOTALS + ("looked", "full_sweeps")


def pred_of(path):
    pred = np.empty(len(path), np.int64)
    pred[np.asarray(path, np.int64)] = np.arange(len(path))
    return pred


def difference_set(before, after):
    """the nodes v whose unordered pair {pred v, succ v} differs between the two tours -> uint8 [n]"""
    b, a = np.asarray(before, np.int64), np.asarray(after, np.int64)
    pb, pa = pred_of(b), pred_of(a)
    same = ((pb == pa) & (b == a)) | ((pb == a) & (b == pa))
    return (~same).astype(np.uint8)


def load_cost(path, costs=None, xy=None):
    """the cost of a freshly loaded tour (integer weights: the order of the sum does not matter)"""
    idx = np.arange(len(path))
    if costs is not None:
        return float(np.asarray(costs)[idx, np.asarray(path, np.int64)].sum())
    return float(N.euc(xy, idx, path).sum())


def model_walk_dl(start, best_cost, nodes, k, seed, width, closing, kick=None, log=None, **src):
    """model_walk with the descent with looks and the difference rule -> its dict with looked and full_sweeps summed as well.
    log (a list): per iteration (the set the descent entered with, its looked, its sweeps)"""
    n = len(start)
    state = {"opt": None, "looked": 0, "full_sweeps": 0}

    def descent(path, nodes, **s):
        one = all_awake(n) if state["opt"] is None else difference_set(state["opt"], path)
        awake = np.ascontiguousarray(np.tile(one[:n], 3) if state["opt"] is not None else one)
        entered = awake[:n].copy()
        r = model_dl_descent(path, load_cost(path, **s), awake, nodes, width, closing, **s)
        state["opt"] = path.copy()
        state["looked"] += r["looked"]
        state["full_sweeps"] += r["full_sweeps"]
        if log is not None:
            log.append((entered, r["looked"], r["two_opt_sweeps"] + r["or_sweeps"] + r["three_sweeps"]))
        return r
    m = GV.model_walk(start, best_cost, nodes, k, seed, kick=kick, descent=descent, **src)
    for t in GV.THREE_TOTALS:
        m.setdefault(t, 0)
    return dict(m, looked=state["looked"], full_sweeps=state["full_sweeps"])


def walk_entry(xy, nodes, start, cost0, k, w, closing):
    log = []
    r = model_walk_dl(start, cost0, nodes, k, 1 + w, W, closing, log=log, xy=xy)
    return dict({t: r[t] for t in TOTALS}, walk=w, seed=1 + w, cost=load_cost(r["path"], xy=xy), best_cost=r["best_cost"], trace=r["trace"],
                consumed=r["consumed"], path_sha256=digest(r["path"]), best_path_sha256=digest(r["best_path"]),
                awake_at_entry=[int(e.sum()) for e, _, _ in log], looked_by_iteration=[q for _, q, _ in log],
                sweeps_by_iteration=[s for _, _, s in log])


def main():
    xy = N.tsplib_points("pr1002")
    nodes, _ = model_lists(K, xy=xy)
    start, cost0 = N.nn_from(xy, 0)
    out = {"instance": "pr1002", "n": len(xy), "K": K, "W": W, "walks": WALKS, "k": ITERATIONS, "start_sha256": digest(start),
           "start_cost": float(cost0)}
    for closing in (0, 1):
        out["closing%d" % closing] = [walk_entry(xy, nodes, start, float(cost0), ITERATIONS, w, closing) for w in range(WALKS)]
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for closing in (0, 1):
        es = out["closing%d" % closing]
        print("closing", closing, "looked behind kicks", sum(sum(e["looked_by_iteration"][1:]) for e in es), "against n x sweeps",
              out["n"] * sum(sum(e["sweeps_by_iteration"][1:]) for e in es), "awake at entry", [e["awake_at_entry"] for e in es[:2]])


if __name__ == "__main__":
    main()
