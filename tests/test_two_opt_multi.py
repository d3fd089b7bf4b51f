"""Parallel-move 2-opt (include/tspgpu.h "Parallel-move 2-opt"): a sweep keeps one candidate per tour edge and
applies every candidate that beats all candidates it conflicts with.

The reference has nothing of the kind, so the model lives here: tests/two_opt_multi_model.c (rules 1-6 in plain C over a
double matrix or over coordinates), compiled into a scratch directory, and brute_sweep, a Python restatement of the same rules
that it is pinned to.
CPU: model against restatement, the smallest key against the oracle's 2-opt move, the descent's end against the oracle's
sweep, the header and the exported symbols.
GPU: move by move in every cell type and weight form, planted conflicts, rotation and direction of the slot, the slot's
invariants under the other descents, the descent, one sweep at n = 66 000, refusals, the host binary's TSP_2OPT_MULTI."""
import ctypes as C
import functools
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import oracle as O  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")
PKG = os.path.join(ROOT, "travellingsalesmanoptimization_amd")
HOST = os.path.join(PKG, "host")
TSP_BIN = os.path.join(HOST, "tsp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_two_opt_multi.json")
EPS = -1.0e-7
NEW_SYMBOLS = ["tspgpu_two_opt_multi_once", "tspgpu_two_opt_multi", "tspgpu_tour_two_opt_multi", "tspgpu_time_multi_sweep"]
EUC_2D, ATT, CEIL_2D = 0, 1, 2

_dp = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_ip = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")


# ---------------------------------------------------------------------------------------------------------------- model
@functools.lru_cache(maxsize=None)
def c_model():
    """tests/two_opt_multi_model.c compiled into a scratch directory (kept for the process)"""
    d = tempfile.mkdtemp(prefix="two_opt_multi_model_")
    so = os.path.join(d, "two_opt_multi_model.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", "-o", so,
                    os.path.join(ROOT, "tests", "two_opt_multi_model.c"), "-lm"], check=True)
    lib = C.CDLL(so)
    lib.tom_sweep.restype = C.c_int
    lib.tom_sweep.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, _ip, C.c_int, _dp, _ip, C.POINTER(C.c_int), _ip, _ip, _ip, _ip,
                              _dp, _ip, C.POINTER(C.c_int), _ip, _dp, C.POINTER(C.c_double), C.c_int]
    lib.tom_descent.restype = C.c_int
    lib.tom_descent.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, _ip, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_long),
                                C.POINTER(C.c_long), C.POINTER(C.c_int), C.POINTER(C.c_long)]
    return lib


def _src(costs, xy):
    if costs is not None:
        costs = np.ascontiguousarray(costs, np.float64)
        return costs, costs.ctypes.data, None, len(costs)
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1)
    return xy, None, xy.ctypes.data, len(xy) // 2


def model_sweep(path, cost, costs=None, xy=None, kind=EUC_2D, apply=True, threads=8):
    """one sweep of the C model; path in place when apply -> dict(cost, moves [k][2], deltas [k], raw_d, raw_b, cand, acc)"""
    keep, cp, xp, n = _src(costs, xy)
    raw_d, cdl, deltas = np.empty(n), np.empty(n), np.empty(n)
    raw_b, ca, cb, ci, cj, acc = (np.empty(n, np.int32) for _ in range(6))
    mv = np.empty(2 * n, np.int32)
    m, k, cc = C.c_int(), C.c_int(), C.c_double(cost)
    rc = c_model().tom_sweep(cp, xp, n, kind, path, threads, raw_d, raw_b, C.byref(m), ca, cb, ci, cj, cdl, acc, C.byref(k), mv, deltas,
                             C.byref(cc), 1 if apply else 0)
    assert rc == 0
    m, k = m.value, k.value
    cand = [(float(cdl[x]), int(ca[x]), int(cb[x]), int(ci[x]), int(cj[x])) for x in range(m)]
    return {"cost": cc.value, "moves": mv[:2 * k].reshape(-1, 2).copy(), "deltas": deltas[:k].copy(), "raw_d": raw_d, "raw_b": raw_b,
            "cand": cand, "acc": [int(v) for v in acc[:m]]}


def model_descent(path, costs=None, xy=None, kind=EUC_2D, threads=8):
    """rule 6 in the C model; path in place -> dict(cost, sweeps, moves, max_k, multi)"""
    keep, cp, xp, n = _src(costs, xy)
    cc, sw, mv, mk, mu = C.c_double(), C.c_long(), C.c_long(), C.c_int(), C.c_long()
    assert c_model().tom_descent(cp, xp, n, kind, path, threads, C.byref(cc), C.byref(sw), C.byref(mv), C.byref(mk), C.byref(mu)) == 0
    return {"cost": cc.value, "sweeps": sw.value, "moves": mv.value, "max_k": mk.value, "multi": mu.value}


def model_walk(start, costs=None, xy=None, kind=EUC_2D, limit=100000):
    """the sweeps of the descent from `start`, one record per sweep (the last one accepts nothing)"""
    path = start.copy()
    cost = tour_cost(path, costs, xy, kind)
    out = []
    while len(out) < limit:
        r = model_sweep(path, cost, costs, xy, kind)
        cost = r["cost"]
        out.append((r["moves"], r["deltas"], path.copy(), cost))
        if len(r["moves"]) == 0:
            break
    return out


def weight_matrix(xy, kind):
    return O.cost_matrix(xy, kind)


def tour_cost(path, costs=None, xy=None, kind=EUC_2D):
    c = costs if costs is not None else weight_matrix(xy, kind)
    return float(sum(c[i][int(path[i])] for i in range(len(path))))


def brute_sweep(c, path):
    """rules 1-5 as plain Python over lists -> dict like model_sweep's plus the conflict matrix"""
    n = len(path)
    path = [int(v) for v in path]
    P, order, v = [0] * n, [0] * n, 0
    for i in range(n):
        P[v], order[i] = i, v
        v = path[v]
    raw_d, raw_b = [None] * n, [-1] * n
    for a in range(n):
        sa = path[a]
        for b in range(n):
            sb = path[b]
            if sa == sb or a == sb or b == sa:
                continue
            d = (c[a][b] + c[sa][sb]) - (c[a][sa] + c[b][sb])
            if raw_d[a] is None or d < raw_d[a]:
                raw_d[a], raw_b[a] = d, b
    cand, seen = [], set()
    for a in range(n):
        b = raw_b[a]
        if b < 0 or not raw_d[a] < EPS or frozenset((a, b)) in seen:
            continue
        seen.add(frozenset((a, b)))
        lo, hi = (a, b) if P[a] < P[b] else (b, a)
        cand.append((raw_d[a], lo, hi, P[lo], P[hi]))
    key = [(d, min(a, b), max(a, b)) for d, a, b, _, _ in cand]
    conflict = [[x != y and cand[y][3] <= cand[x][4] and cand[x][3] <= cand[y][4] for y in range(len(cand))] for x in range(len(cand))]
    acc = [int(all(key[x] < key[y] for y in range(len(cand)) if conflict[x][y])) for x in range(len(cand))]
    sel = sorted((x for x in range(len(cand)) if acc[x]), key=lambda x: key[x])
    for x in sel:
        i, j = cand[x][3], cand[x][4]
        order[i + 1:j + 1] = order[i + 1:j + 1][::-1]
    new = [0] * n
    for i in range(n):
        new[order[i]] = order[(i + 1) % n]
    return {"raw_d": raw_d, "raw_b": raw_b, "cand": cand, "acc": acc, "conflict": conflict,
            "moves": [(cand[x][1], cand[x][2]) for x in sel], "deltas": [cand[x][0] for x in sel], "path": new}


def random_tour(n, rng):
    perm = rng.permutation(n)
    path = np.empty(n, np.int32)
    path[perm] = np.roll(perm, -1)
    return path


def sym_int_matrix(n, rng, hi=1000):
    a = rng.integers(0, hi, (n, n)).astype(np.float64)
    a = np.triu(a, 1)
    a = a + a.T
    np.fill_diagonal(a, -1.0)
    return a


def planted(n, moves, seed=5):
    """base 1000 + noise off the tour, 990 on the identity tour 0 -> 1 -> ... -> n - 1 -> 0, and for every (i, j, gain) the two
    cells c[i][j], c[i + 1][j + 1] at 1000 - gain / 2: delta(i, j) = 20 - gain exactly, the neighbours (i - 1, j - 1) and
    (i + 1, j + 1) get 20 - gain / 2 + noise, every other pair stays above +20."""
    rng = np.random.default_rng(seed)
    c = 1000.0 + sym_int_matrix(n, rng, hi=10)
    for i in range(n):
        c[i][(i + 1) % n] = c[(i + 1) % n][i] = 990.0
    for i, j, gain in moves:
        for u, v in ((i, j), (i + 1, (j + 1) % n)):
            c[u][v] = c[v][u] = 1000.0 - gain / 2
    np.fill_diagonal(c, -1.0)
    return c, np.roll(np.arange(n, dtype=np.int32), -1)


# (name, planted moves, the accepted set of the first sweep written out)
PLANTED = [
    # {2, 8} and {8, 14} share the tour edge at position 8; {17, 21} is clear of both
    ("shared_edge", [(2, 8, 600), (8, 14, 400), (17, 21, 300)], [(2, 8), (17, 21)]),
    # {2, 10} and {6, 14} cross
    ("crossing", [(2, 10, 600), (6, 14, 400), (17, 21, 300)], [(2, 10), (17, 21)]),
    # {5, 9} lies inside {2, 14} and has the smaller key; then the other way round
    ("nested_inner_wins", [(2, 14, 400), (5, 9, 600), (17, 21, 300)], [(5, 9), (17, 21)]),
    ("nested_outer_wins", [(2, 14, 600), (5, 9, 400), (17, 21, 300)], [(2, 14), (17, 21)]),
    # two disjoint candidates of equal delta -480: both accepted, the labels order them
    ("equal_delta", [(12, 16, 500), (2, 6, 500)], [(2, 6), (12, 16)]),
    # 3 and 9 choose each other: one candidate, once
    ("mutual_best", [(3, 9, 600)], [(3, 9)]),
]


def small_cases():
    rng = np.random.default_rng(77)
    for n in range(5, 13):
        for rep in range(6):
            yield "random%d_%d" % (n, rep), sym_int_matrix(n, rng), random_tour(n, rng)
        yield "fewvalues%d" % n, sym_int_matrix(n, rng, hi=3), random_tour(n, rng)
        xy = rng.uniform(0, 30, (n, 2))
        yield "points%d" % n, O.cost_matrix(xy), random_tour(n, rng)
        yield "real%d" % n, sym_int_matrix(n, rng) + symmetric_noise(n, rng), random_tour(n, rng)
    for name, moves, _ in PLANTED:
        yield (name,) + planted(24, moves)


def symmetric_noise(n, rng):
    a = np.triu(rng.uniform(0, 1, (n, n)), 1)
    return a + a.T


# ------------------------------------------------------------------------------------------------------------ CPU tests
def test_model_equals_brute_force_restatement():
    """every delta, key, interval, conflict (through the accepted flags of all candidates) and accepted set, and the path"""
    multi = 0
    for name, c, path in small_cases():
        want = brute_sweep(c.tolist(), path)
        got_path = path.copy()
        got = model_sweep(got_path, 0.0, costs=c)
        assert [float(v) for v in got["raw_d"]] == [float(v) for v in want["raw_d"]], name
        assert [int(v) for v in got["raw_b"]] == want["raw_b"], name
        assert got["cand"] == [(float(d), a, b, i, j) for d, a, b, i, j in want["cand"]], name
        assert got["acc"] == want["acc"], name
        assert [tuple(int(v) for v in mv) for mv in got["moves"]] == want["moves"], name
        assert [float(v) for v in got["deltas"]] == [float(v) for v in want["deltas"]], name
        assert [int(v) for v in got_path] == want["path"] and O.valid_tour(got_path), name
        assert got["cost"] == sum(want["deltas"]), name
        # rule 4 from the conflict matrix: accepted candidates are pairwise free of conflicts
        sel = [x for x, a in enumerate(want["acc"]) if a]
        assert not any(want["conflict"][x][y] for x in sel for y in sel), name
        multi += len(sel) >= 2
    assert multi >= 10


def test_model_coordinate_variant_equals_the_matrix_model():
    rng = np.random.default_rng(3)
    for kind in (EUC_2D, ATT, CEIL_2D):
        for n in (5, 9, 40, 130):
            xy = rng.uniform(0, 500, (n, 2)) if kind != CEIL_2D or n % 2 else rng.integers(0, 500, (n, 2)).astype(np.float64)
            c = weight_matrix(xy, kind)
            p1 = random_tour(n, rng)
            p2 = p1.copy()
            a, b = model_sweep(p1, 0.0, costs=c), model_sweep(p2, 0.0, xy=xy, kind=kind)
            assert a["cand"] == b["cand"] and a["acc"] == b["acc"] and np.array_equal(p1, p2) and a["cost"] == b["cost"]


def test_planted_conflicts_in_the_model():
    for name, moves, want in PLANTED:
        c, path = planted(24, moves)
        r = model_sweep(path, 0.0, costs=c)
        assert [tuple(int(v) for v in mv) for mv in r["moves"]] == want, name
        pairs = [frozenset(x[1:3]) for x in r["cand"]]
        assert len(set(pairs)) == len(pairs), name
        for i, j, gain in moves:
            assert (20.0 - gain, i, j, i, j) in r["cand"], name
    c, _ = planted(24, PLANTED[4][1])
    assert model_sweep(np.roll(np.arange(24, dtype=np.int32), -1), 0.0, costs=c, apply=False)["deltas"].tolist() == [-480.0, -480.0]


def test_smallest_key_is_the_oracles_move():
    rng = np.random.default_rng(11)
    for rep in range(40):
        n = int(rng.integers(5, 60))
        c = sym_int_matrix(n, rng) if rep % 2 else O.cost_matrix(rng.uniform(0, 100, (n, 2)))
        path = random_tour(n, rng)
        p2 = path.copy()
        d, _, (a, b) = O.two_opt_once(c, p2, 0.0)
        r = model_sweep(path, 0.0, costs=c, apply=False)
        if d < EPS:
            assert r["deltas"][0] == d and {int(r["moves"][0][0]), int(r["moves"][0][1])} == {a, b}
        else:
            assert len(r["moves"]) == 0


def test_descent_ends_in_a_two_opt_optimum():
    rng = np.random.default_rng(12)
    for n in (5, 6, 17, 64, 200):
        c = O.cost_matrix(O.random_points(n, 40 + n))
        path = random_tour(n, rng)
        r = model_descent(path, costs=c)
        assert O.valid_tour(path) and r["cost"] == O.tour_cost(c, path)
        d, _, _ = O.two_opt_once(c, path.copy(), r["cost"])
        assert not d < EPS
        assert r["sweeps"] >= 1 and (n < 17 or r["multi"] >= 1)


def test_header_and_libraries_declare_the_entry_points():
    from travellingsalesmanoptimization_amd import _lib
    text = open(os.path.join(ROOT, "include", "tspgpu.h")).read()
    for s in NEW_SYMBOLS:
        assert ("int %s(tspgpu_ctx *ctx" % s) in text, s
        assert s in _lib.SIGNATURES and hasattr(_lib.load(), s), s
    # the conventions of tests/test_abi.py: the section names the reference lines its rule restates
    assert "src/algorithms/refinment.c:55" in text and "refinment.c:60-62" in text and "refinment.c:6-9" in text
    import travellingsalesmanoptimization_amd as T
    for m in ("two_opt_multi_once", "two_opt_multi", "tour_two_opt_multi", "time_multi_sweep"):
        assert hasattr(T.Engine, m)


def test_no_context_means_14():
    from travellingsalesmanoptimization_amd import _lib
    L = _lib.load()
    null = C.c_void_p()
    path = np.roll(np.arange(8, dtype=np.int32), -1)
    cost, k, sw, mv, ms = C.c_double(8.0), C.c_int(), C.c_long(), C.c_long(), C.c_float()
    ab, dl = np.zeros(16, np.int32), np.zeros(8)
    assert L.tspgpu_two_opt_multi_once(null, path, C.byref(cost), C.byref(k), ab, dl, 8) == _lib.UNAVAILABLE
    assert L.tspgpu_two_opt_multi(null, path, C.byref(cost), -1.0, C.byref(sw), C.byref(mv)) == _lib.UNAVAILABLE
    assert L.tspgpu_tour_two_opt_multi(null, 0, -1, -1.0, C.byref(sw), C.byref(mv)) == _lib.UNAVAILABLE
    assert L.tspgpu_time_multi_sweep(null, 0, 1, C.byref(ms)) == _lib.UNAVAILABLE
    assert np.array_equal(path, np.roll(np.arange(8), -1)) and cost.value == 8.0       # and no CPU fallback ran


# ------------------------------------------------------------------------------------------------------------ GPU tests
MODES = ["u16", "i32", "f64", "mf_euc", "mf_att", "mf_ceil", "mf_ceil_int"]
ELEM = {"u16": 3, "i32": 2, "f64": 1}


def points_for(mode, n, seed):
    """-> (xy, kind): integer points for the integer CEIL_2D form, real ones for the generic form; weights stay below 65 535"""
    rng = np.random.default_rng(1000 * n + seed)
    if mode == "mf_ceil":
        return rng.uniform(0, 3000, (n, 2)), CEIL_2D
    if mode == "mf_ceil_int":
        return rng.integers(0, 3000, (n, 2)).astype(np.float64), CEIL_2D
    if mode == "mf_att":
        return rng.integers(0, 8000, (n, 2)).astype(np.float64), ATT
    return rng.integers(0, 3000, (n, 2)).astype(np.float64), EUC_2D


def engine_for(mode, xy=None, kind=EUC_2D, costs=None):
    import travellingsalesmanoptimization_amd as T
    eng = T.Engine(0)
    eng.set_option(T.OPT_ELEM, ELEM.get(mode, 0))
    eng.set_option(T.OPT_MATRIX_FREE, 1 if mode.startswith("mf") else 2)
    if costs is not None:
        eng.set_costs(costs)
    else:
        eng.set_points(xy, kind)
        eng.build_costs()
        info = eng.info()
        assert info["matrix_free"] == (1 if mode.startswith("mf") else 0)
        assert info["ceil_int"] == (1 if mode == "mf_ceil_int" else 0) or not mode.startswith("mf_ceil")
    return eng


def nn0(c):
    return O.nn_tour(c, 0)[0]


def check_walk(eng, start, trace, what):
    """two_opt_multi_once repeated to the optimum against the model's sweeps: list, order, deltas, path, cost"""
    path = start.copy()
    cost = trace["cost0"]
    for t, (moves, deltas, want_path, want_cost) in enumerate(trace["sweeps"]):
        cost, mv, dl = eng.two_opt_multi_once(path, cost)
        assert np.array_equal(mv, moves), (what, t)
        assert np.array_equal(dl, deltas), (what, t)
        assert np.array_equal(path, want_path), (what, t)
        assert cost == want_cost, (what, t)
    assert len(trace["sweeps"][-1][0]) == 0
    info = eng.info()
    assert (info["multi_sweeps"], info["multi_moves"], info["multi_max_moves"]) == (1, 0, 0)


def walk_case(mode, n, seed=0, need_multi=True):
    """an instance of n nodes for `mode` and the model's walks from NN(0) and from a random permutation.  Every instance must
    show the model a sweep that accepts two or more moves (the seed is advanced until one does); five nodes cannot hold two
    disjoint ranges of three positions, so n = 5 is the one size exempt."""
    for s in range(seed, seed + 400):
        xy, kind = points_for(mode, n, s)
        c = weight_matrix(xy, kind)
        src = dict(xy=xy, kind=kind) if mode.startswith("mf") else dict(costs=c)
        starts = [nn0(c), random_tour(n, np.random.default_rng(s))]
        traces = []
        for st in starts:
            traces.append({"cost0": tour_cost(st, costs=c), "sweeps": model_walk(st, **src)})
        if n == 5 or not need_multi or any(len(sw[0]) >= 2 for tr in traces for sw in tr["sweeps"]):
            return xy, kind, c, starts, traces
    raise AssertionError("no instance of %d nodes with a sweep of two moves" % n)


def run_walks(mode, n):
    xy, kind, c, starts, traces = walk_case(mode, n)
    assert n == 5 or any(len(sw[0]) >= 2 for tr in traces for sw in tr["sweeps"])
    eng = engine_for(mode, xy, kind)
    for st, tr in zip(starts, traces):
        check_walk(eng, st, tr, (mode, n))
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 6, 7, 8, 9, 12, 63, 64, 65, 200])
@pytest.mark.parametrize("mode", MODES)
def test_gpu_move_by_move(mode, n):
    run_walks(mode, n).close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_move_by_move_at_the_geometry_boundaries(mode):
    """one below, at and one above a multiple of the sweep's run (tour positions per workgroup) and of its block (threads: the
    stride over b), both read from the plan of the instance itself"""
    eng = run_walks(mode, 200)
    info = eng.info()
    R, BT = info["multi_r"], info["multi_block"]
    eng.close()
    assert R >= 1 and BT >= 64
    for n in (9 * R - 1, 9 * R, 9 * R + 1, BT - 1, BT, BT + 1):
        eng = run_walks(mode, n)
        info = eng.info()
        assert (info["multi_r"], info["multi_block"]) == (R, BT), n       # the boundaries are those of this size's plan too
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("start", ["nn0", "random"])
@pytest.mark.parametrize("n", [1000, 1100])
@pytest.mark.parametrize("mode", MODES)
def test_gpu_move_by_move_more_than_a_block(mode, n, start):
    """more than one block of b: from NN(0), and from a random permutation, whose first sweeps hold hundreds of long, nested
    and crossing ranges"""
    xy, kind = points_for(mode, n, 0)
    c = weight_matrix(xy, kind)
    # (the 500 to 600 sweeps from the random start go through the matrix model in every mode: the same sweeps as the coordinate
    # model's, test_model_coordinate_variant_equals_the_matrix_model, at a quarter of its time)
    src = dict(xy=xy, kind=kind) if mode.startswith("mf") and start == "nn0" else dict(costs=c)
    st = nn0(c) if start == "nn0" else random_tour(n, np.random.default_rng(n))
    tr = {"cost0": tour_cost(st, costs=c), "sweeps": model_walk(st, **src)}
    assert any(len(sw[0]) >= 2 for sw in tr["sweeps"])
    eng = engine_for(mode, xy, kind)
    check_walk(eng, st, tr, (mode, n))
    eng.close()


# the matrix sweep's plan changes where a row's 16-byte vectors (V cells each) pass 256 and 1024 (threads 256 -> 512 -> 1024) and
# where vectors / threads passes 1, 2 and 4 (the template's vectors per thread 1 -> 2 -> 4 -> 10): in units of V cells
M2_SWITCHES = [("threads_256_512", 256), ("nch_1_2", 512), ("threads_512_1024", 1024), ("nch_2_4", 2048), ("nch_4_10", 4096)]


@pytest.mark.gpu
@pytest.mark.parametrize("switch", M2_SWITCHES, ids=[sw[0] for sw in M2_SWITCHES])
@pytest.mark.parametrize("mode", ["u16", "i32", "f64"])
def test_gpu_one_sweep_across_the_plan_switches(mode, switch):
    """one sweep from the stripe tour (thousands of candidates, tens of accepted moves) at the last size of a plan and at the first of the next, for every change of the
    matrix sweep's block size and of its template instance (k_m2_sweep<T, 1 / 2 / 4 / 10>), in every cell type.  The plan is
    read back (tspgpu_info 39 - 41) and must differ across the switch; the largest sizes also run a run length above the
    minimum that does not divide n.  The model works from the coordinates (the same costs, see
    test_model_coordinate_variant_equals_the_matrix_model): no host matrix at these sizes."""
    name, vectors = switch
    V = {"u16": 8, "i32": 4, "f64": 2}[mode]
    plans = []
    for n in (vectors * V, vectors * V + 1):
        xy, kind = points_for(mode, n, 1)
        eng = engine_for(mode, xy, kind)
        info = eng.info()
        assert info["elem"] == ELEM[mode] and info["matrix_free"] == 0
        plans.append((info["multi_block"], info["multi_nch"], info["multi_r"]))
        start = stripe_tour(xy)
        want = start.copy()
        r = model_sweep(want, 0.0, xy=xy, kind=kind, threads=16)
        assert len(r["moves"]) >= 2
        path = start.copy()
        cost, mv, dl = eng.two_opt_multi_once(path, 0.0)
        assert np.array_equal(mv, r["moves"]) and np.array_equal(dl, r["deltas"]), n
        assert np.array_equal(path, want) and cost == r["cost"], n
        eng.close()
    (bt0, nch0, _), (bt1, nch1, r1) = plans
    if name.startswith("threads"):
        assert (bt0, bt1) == tuple(int(v) for v in name.split("_")[1:]), plans
    else:
        assert (nch0, nch1) == tuple(int(v) for v in name.split("_")[1:]) and bt0 == bt1, plans
    if vectors >= 2048:
        assert r1 > 4 and (vectors * V + 1) % r1 != 0, plans      # the last workgroup's run is cut short, at a run above the minimum


@pytest.mark.gpu
@pytest.mark.parametrize("case", PLANTED, ids=[p[0] for p in PLANTED])
def test_gpu_planted_conflicts(case):
    name, moves, want = case
    c, path = planted(24, moves)
    mpath = path.copy()
    r = model_sweep(mpath, 990.0 * 24, costs=c)
    assert [tuple(int(v) for v in mv) for mv in r["moves"]] == want
    eng = engine_for("f64", costs=c)
    cost, mv, dl = eng.two_opt_multi_once(path, 990.0 * 24)
    assert [tuple(int(v) for v in m) for m in mv] == want
    assert np.array_equal(dl, r["deltas"]) and np.array_equal(path, mpath) and cost == r["cost"]
    eng.close()


def slot_after_two_opt(c, start, sweeps):
    """a mirror of the slot after `sweeps` moves of the device's 2-opt on `start` (loaded with ord from node 0, dir = +1): the
    oracle's moves, each applied to the ord array as k_apply does -- a = the smaller label, L the cells from succ a to b
    forwards; the shorter arc is reversed in place, and when that is the other arc (n - L < L) dir is toggled
    -> (dir, cell of node 0, successor array)"""
    n = len(start)
    path = start.copy()
    ord_, v = [], 0
    for _ in range(n):
        ord_.append(v)
        v = int(path[v])
    d = 1
    for _ in range(sweeps):
        delta, _, (a, b) = O.two_opt_once(c, path, 0.0)
        assert delta < EPS
        a, b = min(a, b), max(a, b)
        i, j = ord_.index(a), ord_.index(b)
        L = ((j - i) * d) % n
        other = n - L < L
        M = n - L if other else L
        first = (j + d) % n if other else (i + d) % n
        lo = first if d > 0 else (first - (M - 1)) % n
        cells = [(lo + k) % n for k in range(M)]
        vals = [ord_[q] for q in cells][::-1]
        for q, v in zip(cells, vals):
            ord_[q] = v
        if other:
            d = -d
    return d, ord_.index(0), path


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["u16", "f64", "mf_euc"])
def test_gpu_rotation_and_direction(mode):
    """the same tour in a slot that 2-opt moves left with dir = -1 and a rotated ord gives the accepted set of the freshly
    loaded successor array.  Direction and rotation of the slot are the mirror's (slot_after_two_opt), whose tour the
    device's must equal; both directions and a node 0 off cell 0 must occur."""
    n = 300
    xy, kind = points_for(mode, n, 4)
    c = weight_matrix(xy, kind)
    eng = engine_for(mode, xy, kind)
    seen_multi = False
    dirs, rotated = set(), False
    for sweeps in (1, 2, 3, 5, 8):
        d, cell0, mirror = slot_after_two_opt(c, random_tour(n, np.random.default_rng(9)), sweeps)
        dirs.add(d)
        rotated |= cell0 != 0
        eng.tour_load(0, random_tour(n, np.random.default_rng(9)))
        eng.tour_two_opt(0, max_sweeps=sweeps)          # the shorter arc is reversed: the other arc toggles dir
        tour, cost, _ = eng.tour_store(0)
        assert np.array_equal(tour, mirror)
        fresh = tour.copy()
        fcost, fmv, fdl = eng.two_opt_multi_once(fresh, cost)      # slot 0 reloaded from the successor array: dir = +1, ord from node 0
        eng.tour_load(1, random_tour(n, np.random.default_rng(9)))
        eng.tour_two_opt(1, max_sweeps=sweeps)
        sw, mv, rc = eng.tour_two_opt_multi(1, max_sweeps=1)
        got, gcost, gdelta = eng.tour_store(1)
        want = tour.copy()
        r = model_sweep(want, cost, costs=c)
        assert (sw, mv, rc) == (1, len(r["moves"]), 0)
        assert np.array_equal(fmv, r["moves"]) and np.array_equal(fdl, r["deltas"])
        assert np.array_equal(got, want) and np.array_equal(fresh, want) and gcost == r["cost"] == fcost
        assert gdelta == (r["deltas"][0] if len(r["deltas"]) else 0.0)
        seen_multi |= len(r["moves"]) >= 2
    assert seen_multi and dirs == {1, -1} and rotated
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["u16", "i32", "f64", "mf_euc"])
def test_gpu_state_invariants(mode):
    from test_or_opt import apply_move, or_opt_best_move
    import travellingsalesmanoptimization_amd as T
    n = 400
    xy, kind = points_for(mode, n, 2)
    c = weight_matrix(xy, kind)
    start = nn0(c)
    eng = engine_for(mode, xy, kind)
    if mode.startswith("mf"):
        eng.set_option(T._lib.OPT_OR_MATRIX_FREE, 1)
    for sweeps in (1, 2, 3):
        want = start.copy()
        cost = tour_cost(want, costs=c)
        for _ in range(sweeps):
            cost = model_sweep(want, cost, costs=c)["cost"]
        eng.tour_load(0, start)
        sw, mv, rc = eng.tour_two_opt_multi(0, max_sweeps=sweeps)
        got, gcost, _ = eng.tour_store(0)
        assert (sw, rc) == (sweeps, 0) and np.array_equal(got, want) and gcost == cost
        # the ordinary 2-opt sweep on the rewritten slot makes the oracle's move
        eng.tour_copy(1, 0)
        eng.tour_two_opt(1, max_sweeps=1)
        got2, gcost2, gd2 = eng.tour_store(1)
        w2 = want.copy()
        d2, c2, _ = O.two_opt_once(c, w2, cost)
        assert np.array_equal(got2, w2) and gcost2 == c2 and gd2 == d2
        # ... and so does Or-opt
        moves, rc = eng.tour_or_opt(0, max_moves=1)
        got3, gcost3, _ = eng.tour_store(0)
        d3, s, L, q, rev = or_opt_best_move(c, want)
        w3 = want.copy()
        if d3 < EPS:
            apply_move(w3, s, L, q, rev)
        assert moves == (1 if d3 < EPS else 0) and np.array_equal(got3, w3) and gcost3 == cost + (d3 if d3 < EPS else 0.0)
    # the full descent, and tspgpu_two_opt on its result: one sweep, the same path
    path = start.copy()
    cost, sw, mv, rc = eng.two_opt_multi(path)
    want = start.copy()
    r = model_descent(want, costs=c)
    assert rc == 0 and (cost, sw, mv) == (r["cost"], r["sweeps"], r["moves"]) and np.array_equal(path, want)
    again = path.copy()
    cost2, sweeps2, rc2 = eng.two_opt(again)
    assert (cost2, sweeps2, rc2) == (cost, 1, 0) and np.array_equal(again, path)
    eng.close()


@pytest.mark.gpu
def test_gpu_descent_pr1002():
    xy = O.read_tsplib(os.path.join(DATA, "pr1002.tsp"))[0]
    c = O.cost_matrix(xy)
    eng = engine_for("u16", xy, EUC_2D)
    assert eng.info()["elem"] == 3
    start = nn0(c)
    want = start.copy()
    r = model_descent(want, costs=c)
    path = start.copy()
    cost, sw, mv, rc = eng.two_opt_multi(path)
    assert rc == 0 and np.array_equal(path, want) and (cost, sw, mv) == (r["cost"], r["sweeps"], r["moves"])
    info = eng.info()
    assert (info["multi_sweeps"], info["multi_moves"], info["multi_max_moves"]) == (r["sweeps"], r["moves"], r["max_k"])
    assert r["max_k"] >= 2
    eng.close()


@pytest.mark.gpu
def test_gpu_descent_double_matrix_with_real_costs():
    """a 64-node matrix of doubles with non-integer costs (Euclidean weights scaled by per-edge factors, as
    h_Greedy_2opt_mod_costs hands over): path, sweeps and moves are the model's; the cost is the sum of the accepted deltas on
    the recomputed start cost, within 1e-9 relative of the tour's cost recomputed from the matrix"""
    rng = np.random.default_rng(64)
    n = 64
    c = O.cost_matrix(O.random_points(n, 64)) * (1.0 + symmetric_noise(n, rng))
    np.fill_diagonal(c, -1.0)
    start = random_tour(n, rng)
    want = start.copy()
    r = model_descent(want, costs=c)
    assert r["multi"] >= 1
    eng = engine_for("f64", costs=c)
    path = start.copy()
    cost, sw, mv, rc = eng.two_opt_multi(path)
    assert rc == 0 and np.array_equal(path, want) and (sw, mv) == (r["sweeps"], r["moves"])
    exact = O.tour_cost(c, path)
    assert abs(cost - exact) <= 1e-9 * exact
    eng.close()


def path_digest(path):
    return hashlib.sha256(np.ascontiguousarray(path, np.int32).tobytes()).hexdigest()


def large_instance(n, seed):
    return np.random.default_rng(seed).integers(0, 30000, (n, 2)).astype(np.float64)


def stripe_tour(xy, width=300.0):
    """the start of tools/make_golden_two_opt_multi.py: vertical stripes of `width`, upwards in even stripes, downwards in odd ones"""
    stripe = np.floor(xy[:, 0] / width).astype(np.int64)
    y = np.where(stripe % 2 == 0, xy[:, 1], -xy[:, 1])
    order = np.lexsort((np.arange(len(xy)), y, stripe)).astype(np.int32)
    path = np.empty(len(xy), np.int32)
    path[order] = np.roll(order, -1)
    return path


def test_large_golden_start_is_reproducible():
    g = json.load(open(GOLDEN))["n66000"]
    assert path_digest(stripe_tour(large_instance(g["n"], g["seed"]))) == g["start_sha256"]
    assert g["n"] == 66000 and g["moves"] >= 2 and g["max_label"] >= 65536


@pytest.mark.gpu
def test_gpu_large_instance_one_sweep():
    """n = 66 000, matrix-free, EUC_2D, one sweep from the stripe tour against the golden of tools/make_golden_two_opt_multi.py
    (the C model over the coordinates): labels of 17 bits and a candidate array past 65 536"""
    g = json.load(open(GOLDEN))["n66000"]
    n = g["n"]
    xy = large_instance(n, g["seed"])
    eng = engine_for("mf_euc", xy, EUC_2D)
    path = stripe_tour(xy)
    assert path_digest(path) == g["start_sha256"]
    cost, mv, dl = eng.two_opt_multi_once(path, g["start_cost"])
    assert len(mv) == g["moves"] and cost == g["cost"]
    assert path_digest(mv) == g["moves_sha256"] and float(dl.sum()) == g["delta_sum"] and path_digest(path) == g["path_sha256"]
    assert int(mv.max()) >= 65536
    eng.close()


@pytest.mark.gpu
def test_gpu_refusals_and_limits():
    from travellingsalesmanoptimization_amd import TspGpuError
    eng = engine_for("u16", O.random_points(4, 3), EUC_2D)
    with pytest.raises(TspGpuError) as e:
        eng.two_opt_multi(np.roll(np.arange(4, dtype=np.int32), -1))
    assert e.value.code == 3
    # an asymmetric matrix: 9, and the context works afterwards
    rng = np.random.default_rng(1)
    n = 40
    c = sym_int_matrix(n, rng)
    asym = c.copy()
    asym[3][7] += 5.0
    eng.set_costs(asym)
    path = random_tour(n, rng)
    keep = path.copy()
    with pytest.raises(TspGpuError) as e:
        eng.two_opt_multi(path)
    assert e.value.code == 9 and np.array_equal(path, keep)
    with pytest.raises(TspGpuError) as e:
        eng.two_opt_multi_once(path, 0.0)
    assert e.value.code == 9
    eng.set_costs(c)
    want = path.copy()
    r = model_descent(want, costs=c)
    cost, sw, mv, rc = eng.two_opt_multi(path)
    assert rc == 0 and np.array_equal(path, want) and (cost, sw, mv) == (r["cost"], r["sweeps"], r["moves"])
    info = eng.info()
    assert (info["multi_sweeps"], info["multi_moves"], info["multi_max_moves"]) == (r["sweeps"], r["moves"], r["max_k"])
    # cap below the accepted count: 8, the path and the cost as they were
    c, path = planted(24, PLANTED[0][1])
    eng.set_costs(c)
    keep = path.copy()
    with pytest.raises(TspGpuError) as e:
        eng.two_opt_multi_once(path, 123.0, cap=1)
    assert e.value.code == 8 and np.array_equal(path, keep)
    cost, mv, dl = eng.two_opt_multi_once(path, 123.0, cap=2)
    assert len(mv) == 2 and cost == 123.0 + dl.sum()
    # a deadline of 0: 4, a valid tour and its cost
    xy = O.random_points(500, 8)
    cc = O.cost_matrix(xy)
    eng.set_points(xy)
    eng.build_costs()
    path = nn0(cc)
    cost, sw, mv, rc = eng.two_opt_multi(path, time_left_s=0.0)
    assert rc == 4 and O.valid_tour(path) and cost == O.tour_cost(cc, path)
    eng.tour_load(0, path)
    sw, mv, rc = eng.tour_two_opt_multi(0, time_left_s=0.0)
    assert rc == 4
    assert eng.time_multi_sweep(0, 2) > 0.0
    got, gcost, _ = eng.tour_store(0)
    assert np.array_equal(got, path) and gcost == cost        # timing applies nothing
    eng.close()


# ----------------------------------------------------------------------------------------------------------------- host
def run_tsp(*args, multi=None, timeout=300):
    env = dict(os.environ)
    env.pop("TSP_2OPT_MULTI", None)
    if multi is not None:
        env["TSP_2OPT_MULTI"] = multi
    os.makedirs(os.path.join(ROOT, "results"), exist_ok=True)
    r = subprocess.run([TSP_BIN, *args], capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    return r.returncode, r.stdout.strip(), r.stderr


class Solution(C.Structure):   # utils.h:42-47
    _fields_ = [("cost", C.c_double), ("path", C.POINTER(C.c_int)), ("ncomp", C.c_int), ("comp", C.POINTER(C.c_int))]


@pytest.mark.gpu
def test_host_vns_runs_the_parallel_move_descent():
    """mh_VNS's host loop with the model as the local search and the host library's vns_kick on the same glibc stream"""
    k, seed = 3, 1
    xy = O.read_tsplib(os.path.join(DATA, "pr1002.tsp"))[0]
    c = O.cost_matrix(xy)
    n = len(c)
    host = C.CDLL(os.path.join(HOST, "libtsphost.so"))
    host.tsp_init()
    host.err_setverbosity(0)
    from test_host_c import Instance
    Instance.in_dll(host, "tsp_inst").nnodes = n
    host.tsp_srand.argtypes = [C.c_uint]
    host.tsp_srand(seed)
    host.vns_kick.argtypes = [C.POINTER(Solution)]
    s, cost, _ = O.nn_all(c)
    best = cost
    for it in range(k):
        cost = model_descent(s, costs=c)["cost"]
        best = min(best, cost)
        kicks = host.tsp_rand() % 9 - 2
        sol = Solution(cost, s.ctypes.data_as(C.POINTER(C.c_int)), 0, None)
        for _ in range(kicks):
            assert host.vns_kick(C.byref(sol)) == 0
    rc, out, err = run_tsp("-f", os.path.join(DATA, "pr1002.tsp"), "-alg", "VNS", "-k", str(k), "-seed", str(seed), "-q", multi="1")
    assert rc == 0, err
    assert out == "Cost: %.2f" % best
    rc, out, err = run_tsp("-f", os.path.join(DATA, "pr1002.tsp"), "-alg", "VNS", "-k", str(k), "-seed", str(seed), multi="1")
    assert rc == 0 and "TSP_2OPT_MULTI=1" in out + err and "differ from the reference" in out + err


@pytest.mark.gpu
def test_host_switch_values(golden):
    rc, out, err = run_tsp("-f", os.path.join(DATA, "kroA100.tsp"), "-alg", "VNS", "-k", "200", "-q", multi="2")
    assert rc != 0 and "TSP_2OPT_MULTI" in err and "expected 0 or 1" in err
    want = "Cost: %.2f" % golden["algs"]["kroA100_vns_k200"]["cost"]
    outs = []
    for multi in (None, "0"):
        rc, out, err = run_tsp("-f", os.path.join(DATA, "kroA100.tsp"), "-alg", "VNS", "-k", "200", "-q", multi=multi)
        assert rc == 0 and out == want, err
        outs.append((out, err))
    assert outs[0] == outs[1]
