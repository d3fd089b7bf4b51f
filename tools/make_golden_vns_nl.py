#!/usr/bin/env python3
"""CPU model and golden of the neighbour-list VNS (include/tspgpu.h "Neighbour-list VNS").  CPU only.

    python tools/make_golden_vns_nl.py            # writes tests/golden/golden_vns_nl.json (about a minute)

The model of a walk is a loop of
    make_golden_or_opt_nl.model_ls_descent      (rule 8 of "Neighbour-list Or-opt"; it recomputes the cost)
    the strict-< incumbent
    r = rand() % 9 - 2, and r kicks
on glibc's rand() stream after srand(seed), one walk after the other.  The kick is passed in: the tests hand the checker's
restatement of vns_kick (metaheuristic.c:344-409, which draws from the same glibc stream); the default is kick_port, the
Python port of vns_kick_host (csrc/tspgpu.hip), which tests/test_vns_nl.py holds equal to that restatement in tour and in
draws consumed.  The numbers a device walk is handed are the first draws of the same stream (libc_draws), and the model's
count of consumed numbers is found by looking up the draws that follow the walk in them.

The golden: per instance (EUC_2D, K = 8) W walks of k iterations from the nearest-neighbour tour of node 0, seeds 1 + w:
costs, counters, traces, consumed counts, and SHA-256 digests of the paths only.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_two_opt_nl as N  # noqa: E402
from make_golden_or_opt_nl import model_ls_descent  # noqa: E402
from make_golden_two_opt_nl import digest, model_lists  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "golden_vns_nl.json")
K = 8
CASES = (("pr1002", 16, 12), ("d1291", 3, 5), ("fnl4461", 2, 3))        # instance, walks, iterations
TOTALS = ("two_opt_sweeps", "two_opt_moves", "or_sweeps", "or_moves", "rounds", "kicks")
THREE_TOTALS = ("three_sweeps", "three_moves", "three_phases")       # ... of a walk whose descent has a 3-opt phase
_libc = C.CDLL(None)


def libc_srand(seed):
    _libc.srand(C.c_uint(seed))


def libc_rand():
    return int(_libc.rand())


def libc_draws(seed, count):
    """the first `count` values of glibc's rand() after srand(seed)"""
    libc_srand(seed)
    return np.array([_libc.rand() for _ in range(count)], dtype=np.int32)


def draws_for(k):
    """numbers that k iterations cannot exhaust in practice: a kick phase takes 1 + 3 * 6 draws plus its rejections"""
    return 64 * k + 4096


def kick_port(succ, draw):
    """vns_kick_host of csrc/tspgpu.hip, line by line; succ in place.  draw() -> the next number, or None when there is none
    left -> False (succ untouched), else True"""
    n = len(succ)
    tour, v = [0] * n, 0
    for p in range(n):
        tour[p] = v
        v = int(succ[v])

    def at(p):
        return 0 if p < 0 else ((-2 if (n & 3) == 2 else 0) if p >= n else tour[p])
    pick = []
    for i in range(3):
        r = -1
        while r < 0:
            x = draw()
            if x is None:
                return False
            r = x % n
            for q in pick:
                if r == q or r == at(q - 1) or r == at(q + 1):
                    r = -1
                    break
        pick.append(r)
        pick.sort()
    a, sa = tour[pick[0]], tour[(pick[0] + 1) % n]
    b, sb = tour[pick[1]], tour[(pick[1] + 1) % n]
    c, sc = tour[pick[2]], tour[(pick[2] + 1) % n]
    succ[a] = sb
    succ[c] = sa
    succ[b] = sc
    return True


def kick_phase_port(succ, rv, cur):
    """one kick phase of a walk on the numbers rv[cur:] -> (the cursor behind it, kicks), or None when the numbers run out (succ
    is then left as it was): what tspgpu_vns_search and the walks do between two descents"""
    before = succ.copy()
    state = [cur]

    def draw():
        if state[0] >= len(rv):
            return None
        state[0] += 1
        return int(rv[state[0] - 1])
    x = draw()
    kicks = None if x is None else max(x % 9 - 2, 0)
    if kicks is not None:
        for _ in range(kicks):
            if not kick_port(succ, draw):
                kicks = None
                break
    if kicks is None:
        succ[:] = before
        return None
    return state[0], kicks


def consumed_of(rv, nxt, nxt2):
    """how many of the draws rv a walk used, from the two draws that follow it"""
    at = [int(i) for i in np.nonzero(rv[:-1] == nxt)[0] if rv[i + 1] == nxt2]
    assert len(at) == 1, "the draws behind the walk are not in the numbers drawn ahead"
    return at[0]


def model_walk(start, best_cost, nodes, k, seed, kick=None, descent=None, **src):
    """k iterations from `start` on glibc's stream of `seed`; kick(succ) draws from that stream itself (None: kick_port);
    descent(path, nodes, **src) is the descent of an iteration (None: model_ls_descent; one that also answers three_sweeps,
    three_moves and three_phases has them summed too) -> dict(path, best_path, best_cost, trace, consumed, and the totals)"""
    rv = libc_draws(seed, draws_for(k))
    libc_srand(seed)
    path, best = start.copy(), start.copy()
    out = {t: 0 for t in TOTALS}
    trace = []
    for _ in range(k):
        r = (descent or model_ls_descent)(path, nodes, **src)
        for t in TOTALS[:5] + THREE_TOTALS:
            if t in r:
                out[t] = out.get(t, 0) + r[t]
        trace.append(r["cost"])
        if r["cost"] < best_cost:
            best_cost, best = r["cost"], path.copy()
        kicks = libc_rand() % 9 - 2
        for _ in range(kicks):
            if kick is None:
                kick_port(path, libc_rand)
            else:
                kick(path)
        out["kicks"] += max(kicks, 0)
    return dict(out, path=path, best_path=best, best_cost=best_cost, trace=trace, consumed=consumed_of(rv, libc_rand(), libc_rand()))


def walk_entry(xy, nodes, start, cost0, k, w, kick=None):
    """the golden's record of walk w (seed 1 + w) from the tour `start` of cost cost0"""
    r = model_walk(start, cost0, nodes, k, 1 + w, kick=kick, xy=xy)
    cost = float(N.euc(xy, np.arange(len(xy)), r["path"]).sum())
    return dict({t: r[t] for t in TOTALS}, walk=w, seed=1 + w, cost=cost, best_cost=r["best_cost"], trace=r["trace"], consumed=r["consumed"],
                path_sha256=digest(r["path"]), best_path_sha256=digest(r["best_path"]))


def instance_entry(name, walks, k):
    xy = N.tsplib_points(name)
    nodes, _ = model_lists(K, xy=xy)
    start, cost0 = N.nn_from(xy, 0)
    return {"instance": name, "n": len(xy), "K": K, "kind": "EUC_2D", "walks": walks, "k": k, "lists_sha256": digest(nodes),
            "start_sha256": digest(start), "start_cost": float(cost0),
            "entries": [walk_entry(xy, nodes, start, float(cost0), k, w) for w in range(walks)]}


def main():
    out = {name: instance_entry(name, walks, k) for name, walks, k in CASES}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, e in out.items():
        print(name, [(x["walk"], x["best_cost"], x["consumed"]) for x in e["entries"]])


if __name__ == "__main__":
    main()
