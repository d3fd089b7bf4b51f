#!/usr/bin/env python3
"""Golden of the batched neighbour-list descent with a 3-opt phase, from the CPU model of the single-tour
descent.  CPU only.

    python tools/make_golden_nl3_batch.py            # writes tests/golden/golden_nl3_batch.json (about 10 s)

The golden: pr1002 (EUC_2D), K = W = 8, the nearest-neighbour tours from the starts 0 .. 31, each taken through the descent of
rule 10 of "Neighbour-list 3-opt" (tests/three_opt_nl_model.c through make_golden_three_opt_nl.model_ls3_descent, the lists from
make_golden_two_opt_nl.model_lists): per start the cost, the eight counters and the SHA-256 digest of the successor array; the
totals; and the winner -- the lowest cost, ties to the earliest start.  A batch is nothing but its tours, so no new model is
needed.  tests/test_nl3_batch.py imports start_entry.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_two_opt_nl as N  # noqa: E402
from make_golden_three_opt_nl import model_ls3_descent  # noqa: E402
from make_golden_two_opt_nl import digest, model_lists  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "golden_nl3_batch.json")
INSTANCE, K, W, STARTS = "pr1002", 8, 8, 32
COUNTERS = ("two_opt_sweeps", "two_opt_moves", "or_sweeps", "or_moves", "rounds", "three_sweeps", "three_moves", "three_phases")
TOTALS = tuple(k for k in COUNTERS if k not in ("rounds", "three_phases"))


def start_entry(xy, nodes, start, width=W):
    """the golden's record of the descent from the nearest-neighbour tour of `start` -> (record, path)"""
    path = N.nn_from(xy, start)[0]
    r = model_ls3_descent(path, nodes, width, xy=xy)
    return dict({k: r[k] for k in COUNTERS}, start=start, cost=r["cost"], path_sha256=digest(path)), path


def main():
    xy = N.tsplib_points(INSTANCE)
    nodes, _ = model_lists(K, xy=xy)
    starts = [start_entry(xy, nodes, s)[0] for s in range(STARTS)]
    costs = [e["cost"] for e in starts]
    win = costs.index(min(costs))               # (the first of equal costs)
    out = {"instance": INSTANCE, "n": len(xy), "K": K, "W": W, "kind": "EUC_2D", "lists_sha256": digest(nodes), "starts": starts,
           "totals": {k: sum(e[k] for e in starts) for k in TOTALS},
           "winner": {"start": win, "cost": costs[win], "path_sha256": starts[win]["path_sha256"]}}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
