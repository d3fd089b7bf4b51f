"""Neighbour-list 3-opt (include/tspgpu.h "Neighbour-list 3-opt"): pure 3-opt moves whose new edges come from the
K-nearest-neighbour lists, every independent move of a sweep applied at once, and the descent that runs the 3-opt phase behind
the alternation of "Neighbour-list Or-opt".

The model is tests/three_opt_nl_model.c (wrappers in tools/make_golden_three_opt_nl.py), pinned here to a brute-force Python
restatement written from the move side (brute_sweep: every i < j < k and kind of rule 2, rule 4's degeneracy test, the
membership of rule 5 over the writings of the alternating cycle, the ranges, one selection round, the apply by slicing).
CPU: model against restatement, deltas against tour costs, the four kinds, rule 11, the end of a phase, rule 10 against
tools/make_golden_or_opt_nl.model_ls_descent, the golden, the header and the exported symbols.
GPU: move by move in every cell type and weight form, real-valued cells, the sweep's workgroup boundaries, planted moves around
the apply's thread count in both slot directions, the slot's invariants, the descents against the golden, n = 66 000,
refusals, the host binary's TSP_3OPT_WIDTH."""
import ctypes as C
import functools
import itertools
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import oracle as O  # noqa: E402
import make_golden_three_opt_nl as G  # noqa: E402
import make_golden_two_opt_nl as G2  # noqa: E402
from make_golden_or_opt_nl import model_ls_descent  # noqa: E402
from make_golden_three_opt_nl import model_ls3_descent, model_three_sweep, pack  # noqa: E402
from make_golden_two_opt_nl import digest, model_lists  # noqa: E402
from test_two_opt_multi import (EPS, EUC_2D, MODES, engine_for, nn0, points_for, random_tour, sym_int_matrix,  # noqa: E402
                                symmetric_noise, tour_cost, weight_matrix)
from test_two_opt_nl import brute_lists, check_cap_refusal, source_of, stripe_tour  # noqa: E402
from test_or_opt_nl import rect_lattice, run_tsp, tour_from_zero  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_three_opt_nl.json")
NEW_SYMBOLS = ["tspgpu_three_opt_nl_once", "tspgpu_three_opt_nl", "tspgpu_tour_three_opt_nl", "tspgpu_local_search_nl3",
               "tspgpu_tour_local_search_nl3", "tspgpu_time_three_nl_sweep"]
# rule 2: the added edges of a kind as pairs of roles; the removed edges are (a, a'), (b, b'), (c, c')
ROLES = ("a", "a'", "b", "b'", "c", "c'")
ADDED = {0: (("a", "b"), ("a'", "c"), ("b'", "c'")), 1: (("a", "b'"), ("c", "a'"), ("b", "c'")),
         2: (("a", "c"), ("b'", "a'"), ("b", "c'")), 3: (("a", "b'"), ("c", "b"), ("a'", "c'"))}
REMOVED_MATE = {"a": "a'", "a'": "a", "b": "b'", "b'": "b", "c": "c'", "c'": "c"}


# --------------------------------------------------------------------------------------------------------- restatement
def new_order(order, i, j, k, kind):
    """rule 2: the positions i+1 .. k refilled"""
    A, B = order[i + 1:j + 1], order[j + 1:k + 1]
    mid = {0: A[::-1] + B[::-1], 1: B + A, 2: B[::-1] + A, 3: B + A[::-1]}[kind]
    return order[:i + 1] + mid + order[k + 1:]


def move_nodes(order, i, j, k):
    n = len(order)
    return {"a": order[i], "a'": order[i + 1], "b": order[j], "b'": order[j + 1], "c": order[k], "c'": order[(k + 1) % n]}


def degenerate(v, kind):
    """rule 4 (iii): an added edge with two equal ends, or one that is a removed edge as a node pair"""
    removed = [{v["a"], v["a'"]}, {v["b"], v["b'"]}, {v["c"], v["c'"]}]
    return any(v[x] == v[y] or {v[x], v[y]} in removed for x, y in ADDED[kind])


def writings(kind):
    """the alternating cycle of a kind written as chains of roles: every start and both directions, kept where the first edge
    is a removed one -> [(r1 .. r6)]"""
    mate = {}
    for x, y in ADDED[kind]:
        mate[x], mate[y] = y, x
    out = []
    for start in ROLES:
        for first_removed in (True, False):
            chain, removed = [start], first_removed
            for _ in range(5):
                chain.append(REMOVED_MATE[chain[-1]] if removed else mate[chain[-1]])
                removed = not removed
            if first_removed and len(set(chain)) == 6:
                out.append(tuple(chain))
    return out


WRITINGS = {kind: writings(kind) for kind in range(4)}
assert all(len(w) == 6 for w in WRITINGS.values())


# (kind, the chain as indices into ROLES, its three directions: 0 where the chain walks an edge tail first, as succ does)
FLAT = [(kind, tuple(ROLES.index(r) for r in w), tuple(0 if w[2 * m + 1] == w[2 * m] + "'" else 1 for m in range(3)))
        for kind in range(4) for w in WRITINGS[kind]]


def all_moves(c, path, lists, W):
    """every writing (delta, t1, code, i, j, k, kind) of every move of rule 2 that passes rule 4 (iii) and has the membership
    property of rule 5 for that writing"""
    n = len(path)
    P, order = tour_from_zero(path)
    at = [{u: j for j, u in enumerate(lists[v][:W])} for v in range(n)]
    for i, j, k in itertools.combinations(range(n), 3):
        vv = (order[i], order[i + 1], order[j], order[j + 1], order[k], order[(k + 1) % n])
        for kind, w, s in FLAT:
            j3 = at[vv[w[1]]].get(vv[w[2]])
            if j3 is None:
                continue
            j5 = at[vv[w[3]]].get(vv[w[4]])
            if j5 is None or degenerate(dict(zip(ROLES, vv)), kind):
                continue
            t = [vv[r] for r in w]
            d = ((c[t[1]][t[2]] + c[t[3]][t[4]]) + c[t[5]][t[0]]) - ((c[t[0]][t[1]] + c[t[2]][t[3]]) + c[t[4]][t[5]])
            yield d, t[0], pack(s[0], j3, s[1], j5, s[2]), i, j, k, kind


def brute_sweep(c, path, lists, W):
    """rules 1-8 as plain Python -> dict like model_three_sweep's plus the resulting path and what the sweep shows"""
    n = len(path)
    P, order = tour_from_zero(path)
    raw, dup = [None] * n, {}
    for d, t1, code, i, j, k, kind in all_moves(c, path, lists, W):
        if raw[t1] is None or (d, code) < raw[t1][:2]:
            raw[t1] = (d, code, i, j, k, kind)
    cand = [(raw[t][0], t, raw[t][1], raw[t][2], raw[t][4]) for t in range(n) if raw[t] is not None and raw[t][0] < EPS]
    what = {(t, raw[t][1]): raw[t][2:] for t in range(n) if raw[t] is not None}
    for x in cand:
        dup.setdefault(what[x[1], x[2]], []).append(x)
    key = [x[:3] for x in cand]
    m = len(cand)
    conflict = [[x != y and cand[y][3] <= cand[x][4] and cand[x][3] <= cand[y][4] for y in range(m)] for x in range(m)]
    acc = [int(all(key[x] < key[y] for y in range(m) if conflict[x][y])) for x in range(m)]
    sel = sorted((x for x in range(m) if acc[x]), key=lambda x: key[x])
    moves = [what[cand[x][1], cand[x][2]] for x in sel]
    assert len(set(moves)) == len(moves)                    # duplicate writings: exactly one accepted
    for mv, ws in dup.items():
        assert sum(acc[cand.index(x)] for x in ws) <= 1
    new = list(order)
    for i, j, k, kind in moves:                             # the ranges are disjoint
        new[i + 1:k + 1] = new_order(order, i, j, k, kind)[i + 1:k + 1]
    succ = [0] * n
    for p in range(n):
        succ[new[p]] = new[(p + 1) % n]
    ends = sorted((mv[0], mv[2]) for mv in moves)
    return {"raw_d": [r[0] if r else None for r in raw], "raw_b": [r[1] if r else -1 for r in raw], "cand": cand, "acc": acc,
            "moves": moves, "deltas": [cand[x][0] for x in sel], "path": succ,
            "tie": any(acc[x] and conflict[x][y] and cand[x][0] == cand[y][0] for x in range(m) for y in range(m)),
            "dups": sum(len(ws) >= 2 for ws in dup.values()), "shared": any(a[1] + 1 == b[0] for a, b in zip(ends, ends[1:]))}


def small_cases():
    """random tours on integer-rounded points, a real-valued matrix and few distinct values at n = 8 .. 40, and lattices, where
    ties occur; (K, W) over {1, 3, 8, 16}^2 with W <= K on the points and the lattices at the small sizes, a few pairs elsewhere
    (the restatement takes n^3 steps per sweep)"""
    rng = np.random.default_rng(2026)
    pairs = [(K, W) for K in (1, 3, 8, 16) for W in (1, 3, 8, 16) if W <= K]
    some, few = [(3, 3), (8, 3), (16, 8), (16, 16)], [(8, 8), (16, 3)]
    for n in (8, 9, 17, 18, 40):
        yield "points%d" % n, O.cost_matrix(rng.integers(0, 40, (n, 2)).astype(np.float64)), random_tour(n, rng), pairs if n <= 18 else few
        yield "real%d" % n, sym_int_matrix(n, rng) + symmetric_noise(n, rng), random_tour(n, rng), some if n <= 18 else few[:1]
        if n <= 18:
            yield "fewvalues%d" % n, sym_int_matrix(n, rng, hi=3), random_tour(n, rng), some
    for w, h in ((4, 2), (3, 3), (6, 3)):
        yield "lattice%d" % (w * h), O.cost_matrix(rect_lattice(w, h)), random_tour(w * h, rng), pairs
    yield "lattice40", O.cost_matrix(rect_lattice(8, 5)), random_tour(40, rng), few[:1]


# ------------------------------------------------------------------------------------------------------------ CPU tests
def test_model_equals_brute_force_restatement():
    """every 3-opt sweep of a phase (rule 9): candidates per node, compacted candidates with their ranges, accepted flags,
    moves, deltas, path, cost; each accepted delta is the difference of the tour costs for a single applied move (exact for
    integer costs); at the end no improving move with the membership property is left.  The counts at the end are the
    model's own on these seeds, not measurements of the device."""
    kinds, most, shared, ties, multi, dups = set(), 0, 0, 0, 0, 0
    for name, c, start, kw in small_cases():
        cl = c.tolist()
        integer = not name.startswith("real")
        for K, W in kw:
            lists = brute_lists(cl, K)
            nodes, _ = model_lists(K, costs=c)
            assert nodes.tolist() == lists, (name, K)
            path = start.copy()
            cost = tour_cost(path, costs=c)
            for sweep in range(10 * len(c)):
                tag = (name, K, W, sweep)
                before = path.copy()
                want = brute_sweep(cl, path, lists, W)
                got = model_three_sweep(path, cost, nodes, W, costs=c)
                assert [int(v) for v in got["raw_b"]] == want["raw_b"], tag
                assert all(float(gd) == wd for gd, wd in zip(got["raw_d"], want["raw_d"]) if wd is not None), tag
                assert got["cand"] == [(float(d), t, code, i, k) for d, t, code, i, k in want["cand"]], tag
                assert got["acc"] == want["acc"], tag
                assert [tuple(int(v) for v in mv) for mv in got["moves"]] == want["moves"], tag
                assert [float(v) for v in got["deltas"]] == [float(v) for v in want["deltas"]], tag
                assert [int(v) for v in path] == want["path"] and O.valid_tour(path), tag
                _, order = tour_from_zero(before)
                for (i, j, k, kind), d in zip(want["moves"], want["deltas"]):
                    one = new_order(order, i, j, k, kind)
                    diff = sum(cl[one[p]][one[(p + 1) % len(one)]] for p in range(len(one))) - tour_cost(before, costs=c)
                    assert diff == d if integer else abs(diff - d) <= 1e-9 * abs(cost), tag
                if integer:
                    assert got["cost"] == cost + sum(want["deltas"]) == tour_cost(path, costs=c), tag
                cost = got["cost"]
                kinds |= {mv[3] for mv in want["moves"]}
                most = max(most, len(want["moves"]))
                shared += want["shared"]
                ties += want["tie"]
                dups += want["dups"]
                multi += len(want["moves"]) >= 2
                if not want["moves"]:
                    break
            else:
                raise AssertionError("no end of the 3-opt phase: %s" % (tag,))
            assert [mv for mv in all_moves(cl, path, lists, W) if mv[0] < EPS] == [], (name, K, W)
    assert kinds == {0, 1, 2, 3} and most >= 2 and ties >= 1 and multi >= 5 and dups >= 5, (kinds, most, shared, ties, multi, dups)


def test_model_coordinate_variant_equals_the_matrix_model():
    rng = np.random.default_rng(3)
    for kind in (EUC_2D, 1, 2):
        for n in (8, 9, 40, 130):
            xy = rng.uniform(0, 500, (n, 2)) if kind != 2 or n % 2 else rng.integers(0, 500, (n, 2)).astype(np.float64)
            c = weight_matrix(xy, kind)
            nodes, _ = model_lists(8, costs=c)
            p1 = random_tour(n, rng)
            p2 = p1.copy()
            a, b = model_three_sweep(p1, 0.0, nodes, 5, costs=c), model_three_sweep(p2, 0.0, nodes, 5, xy=xy, kind=kind)
            assert a["cand"] == b["cand"] and a["acc"] == b["acc"] and np.array_equal(p1, p2) and a["cost"] == b["cost"]


def test_full_lists_give_the_best_pure_three_opt_move():
    """rule 11.  K = W = 16 at n <= 17 (K' = n - 1): the smallest key's delta is the minimum over every (i, j, k, kind) that
    passes rule 4 (iii), by brute force over the tour costs (integer costs: every writing of a move has the same delta)"""
    rng = np.random.default_rng(19)
    checked = 0
    for n in range(8, 18):
        c = O.cost_matrix(rng.integers(0, 30, (n, 2)).astype(np.float64))
        cl = c.tolist()
        nodes, _ = model_lists(16, costs=c)
        assert nodes.shape[1] == n - 1
        path = random_tour(n, rng)
        for sweep in range(10 * n):
            _, order = tour_from_zero(path)
            base = tour_cost(path, costs=c)
            best = min(sum(cl[o[p]][o[(p + 1) % n]] for p in range(n)) - base
                       for i, j, k in itertools.combinations(range(n), 3) for kind in range(4)
                       if not degenerate(move_nodes(order, i, j, k), kind) for o in (new_order(order, i, j, k, kind),))
            r = model_three_sweep(path, base, nodes, 16, costs=c)
            if best < EPS:
                assert r["deltas"][0] == best, (n, sweep)
                checked += 1
            else:
                assert len(r["moves"]) == 0, (n, sweep)
                break
    assert checked >= 30


def test_descent_begins_as_the_descent_over_the_lists():
    """rule 10: the state at the end of the first rule-8 part is model_ls_descent's, the final cost is not above it and strictly
    below iff a 3-opt move was applied, and the result has no improving 3-opt move with the membership property"""
    improved = 0
    for n, K, W in ((8, 3, 3), (9, 2, 1), (17, 3, 3), (30, 8, 8), (40, 4, 4), (64, 5, 5), (250, 8, 5), (350, 8, 8), (500, 5, 5)):
        c = O.cost_matrix(rect_lattice(8, 5)) if n == 40 else O.cost_matrix(O.random_points(n, 40 + n))
        nodes, _ = model_lists(K, costs=c)
        start = random_tour(n, np.random.default_rng(n + K + W))
        p1, p3 = start.copy(), start.copy()
        r1 = model_ls_descent(p1, nodes, costs=c, limit_sweeps=100 * n)
        r3 = model_ls3_descent(p3, nodes, W, costs=c, limit_sweeps=100 * n)
        first = r3["first"]
        assert np.array_equal(first["path"], p1) and all(first[k] == r1[k] for k in r1 if k != "max_moves"), (n, K, W)
        assert O.valid_tour(p3) and r3["cost"] == O.tour_cost(c, p3) <= r1["cost"]
        assert (r3["cost"] < r1["cost"]) == (r3["three_moves"] >= 1)
        assert r3["three_phases"] >= 1 and r3["three_sweeps"] >= r3["three_phases"] and r3["rounds"] >= r3["three_phases"]
        if n <= 40:
            assert [mv for mv in all_moves(c.tolist(), p3, nodes.tolist(), W) if mv[0] < EPS] == []
        again = p3.copy()
        r = model_ls3_descent(again, nodes, W, costs=c)
        assert np.array_equal(again, p3) and (r["rounds"], r["three_phases"], r["three_sweeps"], r["three_moves"]) == (1, 1, 1, 0)
        improved += r3["three_moves"] >= 1
    assert improved >= 3


@functools.lru_cache(maxsize=None)
def golden():
    return json.load(open(GOLDEN))


def test_golden_is_reproducible_from_the_model():
    g = golden()
    for name in ("kroA100", "pr1002"):
        xy = G2.tsplib_points(name)
        start = G2.nn_from(xy, 0)[0]
        assert digest(start) == g[name]["start_sha256"] and [(d["K"], d["W"]) for d in g[name]["descents"]] == [(8, 5), (8, 8)]
        for want in g[name]["descents"]:
            got = G.descent_entry(xy, start, want["K"], want["W"])
            assert got == want, (name, want["W"])
            if want["W"] == 8:
                assert want["three_moves"] >= 1 and want["cost"] < want["first"]["cost"]
            assert (want["cost"] < want["first"]["cost"]) == (want["three_moves"] >= 1)
    big = g["n66000"]
    assert digest(stripe_tour(G2.large_points(big["n"], big["seed"]))) == big["start_sha256"] and big["n"] == 66000
    assert len(big["sweeps"]) == 3 and big["sweeps"][0]["moves"] >= 2 and all(s["moves"] >= 1 for s in big["sweeps"])


def test_header_and_libraries_declare_the_entry_points():
    from travellingsalesmanoptimization_amd import _lib
    text = open(os.path.join(ROOT, "include", "tspgpu.h")).read()
    assert "Neighbour-list 3-opt" in text and text.index("---- Neighbour-list 3-opt") > text.index("---- Neighbour-list Or-opt")
    for s in NEW_SYMBOLS:
        assert ("int %s(tspgpu_ctx *ctx" % s) in text, s
        assert s in _lib.SIGNATURES and hasattr(_lib.load(), s), s
    section = text[text.index("---- Neighbour-list 3-opt"):]
    for word in ("Positions", "Chain and delta", "Membership", "Range", "Conflict and selection", "Full lists", "refinment.c:6-9"):
        assert word in section, word
    import travellingsalesmanoptimization_amd as T
    for m in ("three_opt_nl_once", "three_opt_nl", "tour_three_opt_nl", "local_search_nl3", "tour_local_search_nl3", "time_three_nl_sweep"):
        assert hasattr(T.Engine, m)


def test_no_context_means_14():
    from travellingsalesmanoptimization_amd import _lib
    L = _lib.load()
    null = C.c_void_p()
    path = np.roll(np.arange(8, dtype=np.int32), -1)
    cost, k, nr, tp, ms = C.c_double(8.0), C.c_int(-7), C.c_int(-7), C.c_int(-7), C.c_float(-7.0)
    cnt = [C.c_long(-7) for _ in range(6)]
    a, b, c, d, e, f = (C.byref(x) for x in cnt)
    mv, dl = np.full(32, -7, np.int32), np.full(8, -7.0)
    assert L.tspgpu_three_opt_nl_once(null, 8, path, C.byref(cost), C.byref(k), mv, dl, 8) == _lib.UNAVAILABLE
    assert L.tspgpu_three_opt_nl(null, 8, path, C.byref(cost), -1.0, a, b) == _lib.UNAVAILABLE
    assert L.tspgpu_tour_three_opt_nl(null, 0, 8, -1, -1.0, a, b) == _lib.UNAVAILABLE
    assert L.tspgpu_local_search_nl3(null, 8, path, C.byref(cost), -1.0, a, b, c, d, C.byref(nr), e, f, C.byref(tp)) == _lib.UNAVAILABLE
    assert L.tspgpu_tour_local_search_nl3(null, 0, 8, -1.0, a, b, c, d, C.byref(nr), e, f, C.byref(tp)) == _lib.UNAVAILABLE
    assert L.tspgpu_time_three_nl_sweep(null, 0, 8, 1, C.byref(ms)) == _lib.UNAVAILABLE
    assert np.array_equal(path, np.roll(np.arange(8), -1)) and cost.value == 8.0       # and no CPU fallback ran
    assert all(x.value == -7 for x in cnt) and (k.value, nr.value, tp.value, ms.value) == (-7, -7, -7, -7.0)
    assert np.all(mv == -7) and np.all(dl == -7.0)


# ------------------------------------------------------------------------------------------------------------ GPU tests
def model_phase(start, nodes, W, c, **src):
    """the sweeps of the model's 3-opt phase from `start`, one record per sweep (the last one accepts nothing)"""
    path = start.copy()
    cost = tour_cost(path, costs=c)
    out = []
    while True:
        r = model_three_sweep(path, cost, nodes, W, **src)
        cost = r["cost"]
        out.append((r["moves"], r["deltas"], path.copy(), cost))
        if len(r["moves"]) == 0:
            return out


def check_phase(eng, start, W, Weff, c, sweeps, what, exact_cost=True):
    """three_opt_nl_once repeated to the end of the phase against the model's sweeps: list, order, deltas, path, cost, info"""
    path = start.copy()
    cost = tour_cost(path, costs=c)
    for t, (moves, deltas, want_path, want_cost) in enumerate(sweeps):
        cost, mv, dl = eng.three_opt_nl_once(path, cost, W)
        assert np.array_equal(mv, moves), (what, t, mv, moves)
        assert np.array_equal(dl, deltas), (what, t)
        assert np.array_equal(path, want_path), (what, t)
        if exact_cost:
            assert cost == want_cost, (what, t)
        else:
            assert abs(cost - want_cost) <= 1e-9 * abs(want_cost), (what, t)
        info = eng.info()
        assert (info["three_nl_w"], info["three_nl_sweeps"], info["three_nl_moves"], info["three_nl_max_moves"]) == \
            (Weff, 1, len(moves), len(moves)), (what, t)
    return sum(len(s[0]) >= 2 for s in sweeps)


KW = ((16, 1), (16, 8), (16, 16), (5, 5))


def run_phases(mode, n, kw, seed=0, first_only=False):
    xy, kind = points_for(mode, n, seed)
    c = weight_matrix(xy, kind)
    src = source_of(mode, xy, kind, c)
    eng = engine_for(mode, xy, kind)
    multi = 0
    for K, W in kw:
        eng.neighbours_build(K)
        nodes, _ = model_lists(K, **src)
        st = random_tour(n, np.random.default_rng(n + K + W))
        sweeps = model_phase(st, nodes, W, c, **src)
        multi += check_phase(eng, st, W, min(W, nodes.shape[1]), c, sweeps[:1] if first_only else sweeps, (mode, n, K, W))
    return eng, multi


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 9, 17, 18, 40])
@pytest.mark.parametrize("mode", MODES)
def test_gpu_move_by_move(mode, n):
    """from a random tour to the end of the 3-opt phase, K = 16 with W = 1, 8, 16 (K' = n - 1 up to n = 17) and K = W = 5"""
    eng, multi = run_phases(mode, n, KW)
    assert n < 40 or multi >= 1
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode,seed", [("u16", 26), ("mf_euc", 26)])
def test_gpu_cap_below_the_accepted_count(mode, seed):
    """(width 8 = K: every list entry)"""
    check_cap_refusal(mode, seed, 4, lambda p, c, nodes, **src: model_three_sweep(p, c, nodes, 8, **src),
                      lambda eng, *a: eng.L.tspgpu_three_opt_nl_once(eng.ctx, 8, *a),
                      lambda eng, p, c, cap: eng.three_opt_nl_once(p, c, 8, cap=cap))


@pytest.mark.gpu
def test_gpu_move_by_move_with_real_costs():
    """f64 cells that hold non-integer costs: lists, moves, deltas (bit-exact) and paths are the model's; the cost is a sum of
    the accepted deltas in an order that is not the model's: within 1e-9 relative of it"""
    rng = np.random.default_rng(64)
    for n in (9, 18, 40, 64):
        c = O.cost_matrix(O.random_points(n, 64 + n)) * (1.0 + symmetric_noise(n, rng))
        np.fill_diagonal(c, -1.0)
        eng = engine_for("f64", costs=c)
        multi = 0
        for K, W in ((3, 3), (8, 8), (8, 5)):
            eng.neighbours_build(K)
            nodes, _ = model_lists(K, costs=c)
            st = random_tour(n, rng)
            multi += check_phase(eng, st, W, min(W, nodes.shape[1]), c, model_phase(st, nodes, W, c, costs=c), (n, K, W), exact_cost=False)
        assert n < 40 or multi >= 1
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["u16", "mf_euc"])
def test_gpu_one_sweep_at_the_workgroup_boundaries(mode):
    """one below, at and one above a multiple of the sweep's nodes per workgroup, read from the library"""
    eng, _ = run_phases(mode, 40, ((5, 5),), first_only=True)
    G_ = eng.info()["three_nl_nodes"]
    eng.close()
    assert G_ >= 1
    for n in (9 * G_ - 1, 9 * G_, 9 * G_ + 1):
        eng, _ = run_phases(mode, n, ((8, 5),), seed=1, first_only=True)
        eng.close()


# ---- the apply: planted moves around the thread count of the apply workgroup, in both slot directions
APPLY_BT = 256          # threads of the apply workgroup (tspgpu_nl3opt.inc)
APPLY_STRIDE = 256      # workgroups of the apply's grid, at most (M2_APPLY_WGS)


def planted_moves(n, spec, first=0):
    """spec: a list of (|A|, |B|, gap to the previous range; None: the range ends at n - 1) -> [(i, j, k, kind)] in positions
    counted from node 0, ranges ascending, the kinds cycling.  A block of one node leaves kind 1 only: the kinds that reverse
    the other block alone are degenerate there, and the one that reverses this block is kind 1 written differently"""
    out, at = [], first - 1
    for x, (la, lb, gap) in enumerate(spec):
        i = n - 1 - la - lb if gap is None else at + 1 + gap
        assert i > at or (i == 0 and at == -1), (n, spec[:8])
        j, k = i + la, i + la + lb
        assert k <= n - 1, (n, spec[:8])
        out.append((i, j, k, 1 if 1 in (la, lb) else x % 4))
        at = k
    return out


def canonical(mv, n):
    """(i, j, k, kind) with the kind that reverses a block of one node named as kind 1, the same order of i + 1 .. k; and,
    where the range is the whole tour (a = c' = node 0), kind 1 named as kind 0: the same edges, the cycle walked the other way"""
    i, j, k, kind = (int(v) for v in mv)
    if (kind == 3 and j - i == 1) or (kind == 2 and k - j == 1):
        kind = 1
    return (i, j, k, 0 if kind == 1 and i == 0 and k == n - 1 else kind)


def planted_matrix(path, f, moves):
    """1000 + noise, the tour's edges 100, the three edges every planted move adds 1 (test_or_opt_nl.planted_matrix for the
    moves of this rule)"""
    import test_or_opt_geometry as OG
    n = len(path)
    c = OG.noise_matrix(n).copy()
    idx = np.arange(n)
    c[idx, path] = 100.0
    c[path, idx] = 100.0
    for i, j, k, kind in moves:
        v = move_nodes([int(x) for x in f], i, j, k)
        assert not degenerate(v, kind), (i, j, k, kind)
        for x, y in ADDED[kind]:
            c[v[x], v[y]] = c[v[y], v[x]] = 1.0
    return c


def apply_specs(n):
    if n < 1000:            # every block shorter than the workgroup
        return [[(2, 2, 0), (1, 2, 1), (2, 1, 0), (2, 2, 2), (40, 2, 1), (2, 60, 0), (3, 3, None)],       # i = 0, adjacent, k = n - 1
                [(30, 30, 1), (2, 3, 0), (2, 2, 0), (5, 1, 3), (1, 7, 1)]]
    big = (255, 256, 257, 513)
    return [[(255, 2, 1), (2, 256, 0), (257, 1, 2), (2, 2, 0)],
            [(256, 257, 0), (513, 2, None)],                                                               # i = 0 and k = n - 1 in one sweep
            [(1, 513, 3), (255, 255, 0), (2, 2, 1)],
            [(1, 2, 0) if x % 2 else (2, 1, 0) for x in range(APPLY_STRIDE + 10)]] + \
           [[(n - 1 - la, la, 0)] for la in big[:1]]                                                       # one move over the whole tour: i = 0, k = n - 1


def apply_cases(n):
    """-> dicts: tour0, flip (a, b, delta) or None, the matrix, the model's sweep on the tour after the flip"""
    import test_or_opt_geometry as OG
    tour0 = random_tour(n, np.random.default_rng(40 + n))
    for spec in apply_specs(n):
        for flipped in (False, True):
            fl = OG.long_arc_flip(tour0)[0] if flipped else None
            lay, path = OG.Layout(tour0), tour0.copy()
            if fl:
                assert O.apply_move(path, None, fl[0], fl[1]) == fl[2]
                lay.flip(*fl)
            f = OG.forward_order(path)
            moves = planted_moves(n, spec)
            c = planted_matrix(path, f, moves)
            cost0, cost = O.tour_cost(c, tour0), O.tour_cost(c, path)
            nodes, _ = model_lists(4, costs=c)
            start = path.copy()
            r = model_three_sweep(path, cost, nodes, 4, costs=c)
            # every planted move is accepted, and nothing else: three edges of 1 for three of 100
            assert sorted(canonical(mv, n) for mv in r["moves"]) == sorted(canonical(mv, n) for mv in moves), (n, spec[:8])
            assert np.all(r["deltas"] == -297.0)
            yield {"tour0": tour0, "flip": (fl[0], fl[1], cost - cost0) if fl else None, "c": c, "start": (start, cost), "sweep": r,
                   "after": path, "dir": lay.dir, "cell0": int(np.nonzero(lay.ord == 0)[0][0]), "spec": spec, "moves": moves}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [150, 1100])
@pytest.mark.parametrize("mode", ["u16", "f64"])
def test_gpu_apply_geometry(mode, n):
    """several planted moves per launch: every kind, blocks of 1, 2, 255, 256, 257 and 513 nodes, ranges that begin at position
    0, end at n - 1 or both, adjacent ranges, more moves than the apply has workgroups; on a freshly loaded slot and on one a
    2-opt move left with dir = -1 and a rotated ord.  Behind the sweep one reference 2-opt sweep (reads the edge costs by
    position) and one neighbour-list Or-opt sweep (reads successors and edge costs by node) must equal their models"""
    from make_golden_or_opt_nl import model_or_sweep
    import travellingsalesmanoptimization_amd as T
    eng = T.Engine(0)
    eng.set_option(T.OPT_ELEM, {"u16": 3, "f64": 1}[mode])
    dirs, rotated, seen, kinds, most = set(), False, set(), set(), 0
    for case in apply_cases(n):
        c = case["c"]
        eng.set_costs(c)
        eng.neighbours_build(4)
        eng.tour_load(0, case["tour0"])
        if case["flip"]:
            eng.tour_apply_move(0, *case["flip"])
        path, cost, _ = eng.tour_store(0)
        assert np.array_equal(path, case["start"][0]) and cost == case["start"][1]
        r = case["sweep"]
        sw, mv, rc = eng.tour_three_opt_nl(0, 4, max_sweeps=1)
        assert (sw, mv, rc) == (1, len(r["moves"]), 0), case["spec"][:8]
        path, cost, delta = eng.tour_store(0)
        assert np.array_equal(path, case["after"]) and (cost, delta) == (r["cost"], -297.0), case["spec"][:8]
        assert eng.info()["three_nl_max_moves"] == len(r["moves"])
        eng.tour_copy(1, 0)
        two = path.copy()
        d2, c2, _ = O.two_opt_once(c, two, r["cost"])
        assert eng.tour_two_opt(1, max_sweeps=1) == (1, 0)
        got, gcost, gdelta = eng.tour_store(1)
        assert np.array_equal(got, two) and (gcost, gdelta) == (c2, d2), case["spec"][:8]
        nodes, _ = model_lists(4, costs=c)
        o = model_or_sweep(path, r["cost"], nodes, costs=c)
        assert eng.tour_or_opt_nl(0, max_sweeps=1) == (1, len(o["moves"]), 0)
        got, gcost, _ = eng.tour_store(0)
        assert np.array_equal(got, path) and gcost == o["cost"], case["spec"][:8]
        dirs.add(case["dir"])
        rotated |= case["cell0"] != 0
        most = max(most, len(r["moves"]))
        for i, j, k, kind in case["moves"]:
            seen |= {j - i, k - j}
            kinds.add((kind, i == 0, k == n - 1))
    assert dirs == {1, -1} and rotated and eng.info()["elem"] == {"u16": 3, "f64": 1}[mode]
    assert {kd for kd, _, _ in kinds} == {0, 1, 2, 3} and any(a and not b for _, a, b in kinds) and any(b and not a for _, a, b in kinds)
    if n >= 1000:
        assert {1, 2, 255, 256, 257, 513} <= seen and most > APPLY_STRIDE and any(a and b for _, a, b in kinds)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["u16", "f64", "mf_euc"])
def test_gpu_slot_invariants(mode):
    """after every 3-opt sweep of a short phase on a slot whose direction and rotation a 2-opt descent changed: the stored
    tour and cost are the model's, the cost is the tour's recomputed one, and the slot's order, positions, successors and edge
    weights serve the other slot calls -- one reference 2-opt sweep (edge costs by position), one neighbour-list 2-opt sweep and
    one neighbour-list Or-opt sweep (successors and edge costs by node) equal their models on the stored tour"""
    from make_golden_or_opt_nl import model_or_sweep
    from make_golden_two_opt_nl import model_sweep
    import travellingsalesmanoptimization_amd as T
    n, K, W = 200, 8, 6
    xy, kind = points_for(mode, n, 2)
    c = weight_matrix(xy, kind)
    eng = engine_for(mode, xy, kind)
    eng.neighbours_build(K)
    nodes, _ = model_lists(K, costs=c)
    want = random_tour(n, np.random.default_rng(5))
    eng.tour_load(0, want)
    eng.tour_two_opt(0, max_sweeps=3)               # (the shorter arc is reversed: direction and rotation of the slot change)
    want, cost, _ = eng.tour_store(0)
    applied = 0
    for sweep in range(4):
        r = model_three_sweep(want, cost, nodes, W, costs=c)
        cost = r["cost"]
        assert eng.tour_three_opt_nl(0, W, max_sweeps=1) == (1, len(r["moves"]), 0)
        got, gcost, gdelta = eng.tour_store(0)
        assert np.array_equal(got, want) and gcost == cost == tour_cost(got, costs=c), sweep
        assert gdelta == (r["deltas"][0] if len(r["deltas"]) else 0.0), sweep
        applied += len(r["moves"])
        eng.tour_copy(1, 0)
        assert eng.tour_two_opt(1, max_sweeps=1) == (1, 0)
        w = want.copy()
        d, wc, _ = O.two_opt_once(c, w, cost)
        got, gcost, gdelta = eng.tour_store(1)
        assert np.array_equal(got, w) and (gcost, gdelta) == (wc, d), sweep
        for call, model in ((eng.tour_two_opt_nl, lambda p: model_sweep(p, cost, nodes, costs=c)),
                            (eng.tour_or_opt_nl, lambda p: model_or_sweep(p, cost, nodes, costs=c))):
            eng.tour_copy(1, 0)
            w = want.copy()
            m = model(w)
            assert call(1, max_sweeps=1) == (1, len(m["moves"]), 0)
            got, gcost, _ = eng.tour_store(1)
            assert np.array_equal(got, w) and gcost == m["cost"], sweep
    assert applied >= 3, "the walk is too short for this test"
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["u16", "mf_euc"])
@pytest.mark.parametrize("W", [5, 8])
@pytest.mark.parametrize("name", ["kroA100", "pr1002"])
def test_gpu_descent(name, W, mode):
    """local_search_nl3 from NN(0) at K = 8 against the golden of the model: every counter, the cost and the tour; not above
    local_search_nl on the same engine, strictly below where the golden applied a 3-opt move; the slot form too"""
    g = golden()[name]
    want = next(d for d in g["descents"] if d["W"] == W)
    xy = O.read_tsplib(os.path.join(DATA, name + ".tsp"))[0]
    eng = engine_for(mode, xy, EUC_2D)
    eng.neighbours_build(8)
    start, _ = eng.nn_tour(0)
    assert digest(start) == g["start_sha256"]
    base = start.copy()
    r0 = eng.local_search_nl(base)
    first = want["first"]
    assert r0["rc"] == 0 and all(r0[k] == first[k] for k in r0 if k != "rc") and digest(base) == first["path_sha256"]
    path = start.copy()
    r = eng.local_search_nl3(path, W)
    keys = ("cost", "two_opt_sweeps", "two_opt_moves", "or_sweeps", "or_moves", "rounds", "three_sweeps", "three_moves", "three_phases")
    assert r["rc"] == 0 and {k: r[k] for k in keys} == {k: want[k] for k in keys}
    assert digest(path) == want["path_sha256"]
    assert r["cost"] <= r0["cost"] and (r["cost"] < r0["cost"]) == (want["three_moves"] >= 1)
    info = eng.info()
    assert (info["three_nl_w"], info["three_nl_sweeps"], info["three_nl_moves"], info["three_nl_max_moves"], info["three_nl_phases"]) == \
        (W, want["three_sweeps"], want["three_moves"], want["max_moves"], want["three_phases"])
    assert (info["or_nl_sweeps"], info["or_nl_moves"], info["or_nl_rounds"]) == (want["or_sweeps"], want["or_moves"], want["rounds"])
    eng.tour_load(1, start)
    r1 = eng.tour_local_search_nl3(1, W)
    got, gcost, _ = eng.tour_store(1)
    assert r1["rc"] == 0 and {k: r1[k] for k in keys[1:]} == {k: want[k] for k in keys[1:]}
    assert np.array_equal(got, path) and gcost == want["cost"]
    # the 3-opt phase alone on the result: one empty sweep, the caller's cost kept
    cost, sw, mv, rc = eng.three_opt_nl(path, 123.0, W)
    assert (cost, sw, mv, rc) == (123.0, 1, 0, 0) and digest(path) == want["path_sha256"]
    eng.close()


@pytest.mark.gpu
def test_gpu_large_instance_three_sweeps():
    """n = 66 000, matrix-free, EUC_2D, K = W = 8: the first three 3-opt sweeps from the stripe tour against the golden"""
    g = golden()["n66000"]
    n = g["n"]
    xy = G2.large_points(n, g["seed"])
    eng = engine_for("mf_euc", xy, EUC_2D)
    eng.neighbours_build(g["K"])
    nodes, _ = eng.neighbours_get()
    assert digest(nodes) == g["lists_sha256"]
    path = stripe_tour(xy)
    assert digest(path) == g["start_sha256"]
    cost = g["start_cost"]
    for t, want in enumerate(g["sweeps"]):
        cost, mv, dl = eng.three_opt_nl_once(path, cost, g["W"])
        assert len(mv) == want["moves"] and cost == want["cost"], t
        assert digest(mv) == want["moves_sha256"] and float(dl.sum()) == want["delta_sum"] and digest(path) == want["path_sha256"], t
    eng.close()


@pytest.mark.gpu
def test_gpu_refusals_and_limits():
    from travellingsalesmanoptimization_amd import TspGpuError
    rng = np.random.default_rng(1)
    n = 40
    c = sym_int_matrix(n, rng)
    path = random_tour(n, rng)
    keep = path.copy()
    eng = engine_for("u16", costs=c)
    eng.tour_load(0, path)

    def calls(W):
        return (lambda: eng.three_opt_nl_once(path, 0.0, W), lambda: eng.three_opt_nl(path, 0.0, W), lambda: eng.local_search_nl3(path, W),
                lambda: eng.tour_three_opt_nl(0, W), lambda: eng.tour_local_search_nl3(0, W), lambda: eng.time_three_nl_sweep(0, W, 1))

    def refused(code, word=None, W=8):
        for call in calls(W):
            with pytest.raises(TspGpuError) as e:
                call()
            assert e.value.code == code and (word is None or word in str(e.value)) and np.array_equal(path, keep)
    # no lists yet: 9 with the text of nl_check
    refused(9, "no neighbour lists: call tspgpu_neighbours_build first")
    # a width outside 1 .. 16: 3, with lists in place
    eng.neighbours_build(8)
    refused(3, "width", W=0)
    refused(3, "width", W=17)
    # lists of another cost source: 9, with the reason
    eng.set_costs(sym_int_matrix(n, rng))
    eng.tour_load(0, path)
    refused(9, "invalidated by a new cost source")
    eng.set_points(O.random_points(n, 5), EUC_2D)
    eng.build_costs()
    eng.neighbours_build(8)
    eng.set_points(O.random_points(n, 6), EUC_2D)
    eng.build_costs()
    eng.tour_load(0, path)
    refused(9, "invalidated by a new cost source")
    # an asymmetric matrix: 9
    asym = c.copy()
    asym[3][7] += 5.0
    eng.set_costs(asym)
    eng.tour_load(0, path)
    refused(9, "symmetric")
    # n = 7: 3, with lists in place
    eng.set_points(O.random_points(7, 3), EUC_2D)
    eng.build_costs()
    eng.neighbours_build(16)
    small = np.roll(np.arange(7, dtype=np.int32), -1)
    for call in (lambda: eng.three_opt_nl(small, 0.0, 8), lambda: eng.local_search_nl3(small, 8), lambda: eng.three_opt_nl_once(small, 0.0, 8)):
        with pytest.raises(TspGpuError) as e:
            call()
        assert e.value.code == 3 and "8 nodes" in str(e.value) and np.array_equal(small, np.roll(np.arange(7), -1))
    # cap below the accepted count: 8, the path and the cost as they were, nothing written
    n = 300
    xy = O.random_points(n, 8)
    cc = O.cost_matrix(xy)
    eng.set_points(xy)
    eng.build_costs()
    eng.neighbours_build(8)
    nodes, _ = model_lists(8, costs=cc)
    path = nn0(cc)
    O.two_opt(cc, path)                     # (from a 2-opt optimum the improving moves are short: several fit one sweep)
    keep = path.copy()
    k = len(model_three_sweep(path.copy(), 0.0, nodes, 8, costs=cc)["moves"])
    assert k >= 2
    L = eng.L
    mv, dl = np.full(4 * n, -7, np.int32), np.full(n, -7.0)
    cost, cnt = C.c_double(123.0), C.c_int(-7)
    assert L.tspgpu_three_opt_nl_once(eng.ctx, 8, path, C.byref(cost), C.byref(cnt), mv, dl, k - 1) == 8
    assert np.array_equal(path, keep) and cost.value == 123.0 and cnt.value == -7 and np.all(mv == -7) and np.all(dl == -7.0)
    cost, mv, dl = eng.three_opt_nl_once(path, 123.0, 8, cap=k)
    assert len(mv) == k and cost == 123.0 + dl.sum() and O.valid_tour(path)
    # a deadline of 0: 4, a valid tour and its cost
    path = random_tour(n, np.random.default_rng(9))
    keep = path.copy()
    r = eng.local_search_nl3(path, 8, time_left_s=0.0)
    assert r["rc"] == 4 and np.array_equal(path, keep) and r["cost"] == O.tour_cost(cc, path)
    cost, sw, mv, rc = eng.three_opt_nl(path, 55.0, 8, time_left_s=0.0)
    assert (rc, cost, sw, mv) == (4, 55.0, 0, 0) and np.array_equal(path, keep)
    eng.tour_load(0, path)
    assert eng.tour_three_opt_nl(0, 8, time_left_s=0.0)[2] == 4 and eng.tour_local_search_nl3(0, 8, time_left_s=0.0)["rc"] == 4
    assert eng.time_three_nl_sweep(0, 8, 2) > 0.0
    got, gcost, _ = eng.tour_store(0)
    assert np.array_equal(got, path) and gcost == r["cost"]        # timing applies nothing
    eng.close()


# ----------------------------------------------------------------------------------------------------------------- host
def run_tsp3(*args, env_set=None):
    env_set = dict(env_set or {})
    if "TSP_3OPT_WIDTH" not in env_set:
        os.environ.pop("TSP_3OPT_WIDTH", None)
    return run_tsp(*args, env_set=env_set)


@pytest.mark.gpu
def test_host_binary_runs_the_descent_with_the_three_opt_phase():
    """`-alg GREEDY` (the nearest-neighbour tour from node 0) on kroA100 with TSP_OR_OPT=1 and TSP_OR_OPT_NEIGHBOURS=8: the polish is the descent over the lists;
    TSP_3OPT_WIDTH=8 makes it the descent of rule 10 from the same tour, whose cost is the model's; a bad width is refused
    loudly, and without the two Or-opt switches the width says that it has no effect"""
    data = os.path.join(DATA, "kroA100.tsp")
    args = ("-f", data, "-alg", "GREEDY", "-q")
    env = {"TSP_OR_OPT": "1", "TSP_OR_OPT_NEIGHBOURS": "8"}
    rc0, plain, err0 = run_tsp3(*args)
    rc1, out1, err1 = run_tsp3(*args, env_set=env)
    rc3, out3, err3 = run_tsp3(*args, env_set=dict(env, TSP_3OPT_WIDTH="8"))
    assert (rc0, rc1, rc3) == (0, 0, 0) and all(o.startswith("Cost: ") for o in (plain, out1, out3)), (err0, err1, err3)
    assert float(out3[6:]) <= float(out1[6:]) <= float(plain[6:])
    # the polish starts from NN(0), the heuristic's result: the golden's descent, reproduced from the model in the CPU tests
    want = next(d for d in golden()["kroA100"]["descents"] if (d["K"], d["W"]) == (8, 8))
    xy = G2.tsplib_points("kroA100")
    start, cost = G2.nn_from(xy, 0)
    assert digest(start) == golden()["kroA100"]["start_sha256"] and plain == "Cost: %.2f" % cost
    assert out1 == "Cost: %.2f" % want["first"]["cost"] and out3 == "Cost: %.2f" % want["cost"] and want["three_moves"] >= 1
    assert run_tsp3(*args, env_set=dict(env, TSP_3OPT_WIDTH="0")) == (rc1, out1, err1)
    for bad in ("17", "x", "-1", ""):
        rc, out, err = run_tsp3(*args, env_set=dict(env, TSP_3OPT_WIDTH=bad))
        assert rc != 0 and "TSP_3OPT_WIDTH" in err and "1 to 16" in err, bad
    rc, out, err = run_tsp3(*args[:-1], env_set={"TSP_3OPT_WIDTH": "8"})
    assert rc == 0 and "TSP_3OPT_WIDTH=8 has no effect" in out + err
    rc, out, err = run_tsp3(*args, env_set={"TSP_3OPT_WIDTH": "8"})
    assert rc == 0 and out == plain
