#!/usr/bin/env python3
"""Where the fetches of the shaped k_lds2opt are, on the CPU: the oracle's descent from NN(0) move by move, every move decoded
with the kernel's own arithmetic (csrc/tspgpu_lds2opt.inc: the shorter arc [lo, lo + M) is reversed, k0 = E * wg, an own cell
whose mirror cell lies more than E cells behind k0 needs a fetched row), and per sweep the largest number of rows that one
workgroup fetches.   python tests/lds_overlap_step0.py [n [seed [E]]]      (defaults: the headline, 4096 123 16)"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import oracle as O

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 123
E = int(sys.argv[3]) if len(sys.argv) > 3 else 16
W = n // E
c = O.cost_matrix(O.random_points(n, seed))
succ, cost = O.nn_tour(c, 0)

ord_ = np.empty(n, dtype=np.int64)          # the kernel's array: the visiting order from node 0, dir = +1
v = 0
for p in range(n):
    ord_[p] = v; v = succ[v]
pos = np.empty(n, dtype=np.int64); pos[ord_] = np.arange(n)
dirn = 1
k0 = np.arange(W)[:, None] * E
r = np.arange(E + 1)[None, :]
rows = []                                   # per moving sweep: (M, workgroups that fetch, max rows of one workgroup, rows over all)
while True:
    d, cost, (a, b) = O.two_opt_once(c, succ, cost)
    if d >= 0:
        break
    ea = pos[a] if dirn > 0 else (pos[a] - 1) % n          # the cell of the edge whose tail (in the tour's direction) is a
    eb = pos[b] if dirn > 0 else (pos[b] - 1) % n
    s1, s2 = (ea, eb) if dirn > 0 else (eb, ea)
    L = (s2 - s1) % n
    other = n - L < L
    M = n - L if other else L
    lo = ((s2 if other else s1) + 1) % n
    if other:
        dirn = -dirn
    rel = (k0 - lo + r) % n                 # [W][E + 1]
    rm = ((lo + M - 1 - rel) % n - k0) % n
    need = (rel < M) & (rm > E)
    cnt = need.sum(axis=1)
    rows.append((M, int((cnt > 0).sum()), int(cnt.max()), int(cnt.sum())))
    idx = (lo + np.arange(M)) % n
    ord_[idx] = ord_[idx][::-1]
    pos[ord_[idx]] = idx
nxt = np.roll(ord_, -1) if dirn > 0 else np.roll(ord_, 1)
assert np.array_equal(succ[ord_], nxt), "the array model lost the oracle's tour"
rows = np.array(rows)
M, wgs, mx, tot = rows.T
print(f"n={n} seed={seed} E={E}: {len(rows)} moving sweeps (+ the final one), cost {cost:.0f}")
print(f"sweeps with a fetching workgroup: {(mx > 0).sum()} of {len(rows)}; rows fetched per workgroup over the descent: mean {tot.sum() / W:.0f}")
print("max over workgroups of popcount(need) -> sweeps:")
for k in range(E + 2):
    if (mx == k).any():
        print(f"  {k:2d}: {(mx == k).sum():4d}")
for capv in (4, 8):
    print(f"sweeps with a fetch and max <= {capv}: {((mx > 0) & (mx <= capv)).sum()}")
print("by the length of the reversed range: sweeps, with a fetch, with a fetch of at most 4 / 8 rows, mean workgroups fetching")
for lo_, hi_ in ((2, 8), (8, 16), (16, 64), (64, 256), (256, 1024), (1024, 4096)):
    s = (M >= lo_) & (M < hi_)
    if s.any():
        f = s & (mx > 0)
        print(f"  {lo_:4d} <= M < {hi_:4d}: {s.sum():4d} {f.sum():4d} {(f & (mx <= 4)).sum():4d} {(f & (mx <= 8)).sum():4d}   {wgs[f].mean() if f.any() else 0:.1f}")
