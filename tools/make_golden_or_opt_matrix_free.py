#!/usr/bin/env python3
"""Writes tests/golden/golden_or_opt_matrix_free.json: the Or-opt moves tests/test_or_opt_matrix_free.py expects past the
sizes at which a cost matrix can be held -- the first three moves on 66 000 uniform-random integer points (EUC_2D) from
the boustrophedon tour, and one sweep at the size limit n = 131 072.  The points and the start tour are built by the
test module's own functions (big_points, boustrophedon); the moves come from the threaded C restatement over coordinates
tests/or_opt_model_xy.c, which the CPU tests pin to the plain model at n = 200.  Needs no GPU; prints each case's seconds.

    python tools/make_golden_or_opt_matrix_free.py [threads]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_or_opt_matrix_free as M  # noqa: E402  (the test module's own functions: its inputs, model and checks)

O = M.O


def case(n, moves, threads):
    t0 = time.time()
    xy = M.big_points(n)
    path = M.boustrophedon(xy)
    assert O.valid_tour(path)
    out = {"n": n, "kind": "EUC_2D", "points_sha": M.sha(xy), "start_sha": M.sha(path), "moves": [],
           "costs": [O.tour_cost_xy(xy, M.EUC_2D, path)]}
    for _ in range(moves):
        mv = M.best_move_xy(xy, M.EUC_2D, path, threads)
        assert mv[0] < M.EPS, mv
        M.apply_move(path, *mv[1:])
        cost = out["costs"][-1] + mv[0]
        assert O.valid_tour(path) and O.tour_cost_xy(xy, M.EUC_2D, path) == cost
        out["moves"].append(list(mv))
        out["costs"].append(cost)
    print("n = %d: %d moves %s, %.1f s on %d threads" % (n, moves, out["moves"], time.time() - t0, threads), flush=True)
    return out


def main():
    threads = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    golden = {"n66000": case(66000, 3, threads), "n131072": case(131072, 1, threads)}
    with open(M.GOLDEN, "w") as f:
        json.dump(golden, f, indent=1)
        f.write("\n")
    print("wrote", M.GOLDEN)


if __name__ == "__main__":
    main()
