"""Neighbour-list Or-opt (include/tspgpu.h "Neighbour-list Or-opt"): Or-opt candidates from the K-nearest-neighbour
lists, every independent move of a sweep applied at once, and the descent that alternates it with the neighbour-list 2-opt.

The model is tests/or_opt_nl_model.c (wrappers in tools/make_golden_or_opt_nl.py), pinned here to a brute-force Python
restatement of rules 1-6 (brute_sweep: every (s, L, q, rev) of rule 1 filtered by the membership property of rule 3, the
apply in position space by rule 4).
CPU: model against restatement, rule 9 against tests/or_opt_model.c, rule 3 and the double local optimum at the end of the
descents, the golden, the header and the exported symbols.
GPU: move by move in every cell type and weight form, real-valued cells, the sweep's workgroup boundaries, planted moves around
the apply's chunk size in both slot directions, the slot's invariants, the descents against the model and the golden,
n = 66 000, refusals, the host binary's TSP_OR_OPT_NEIGHBOURS."""
import ctypes as C
import functools
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
import make_golden_or_opt_nl as G  # noqa: E402
import make_golden_two_opt_nl as G2  # noqa: E402
from make_golden_or_opt_nl import model_ls_descent, model_or_sweep, unpack  # noqa: E402
from make_golden_two_opt_nl import digest, model_lists, model_sweep  # noqa: E402
from test_two_opt_multi import (CEIL_2D, EPS, EUC_2D, MODES, engine_for, nn0, points_for, random_tour,  # noqa: E402
                                sym_int_matrix, symmetric_noise, tour_cost, weight_matrix)
from test_two_opt_nl import brute_lists, check_cap_refusal, restricted_improving_pairs, source_of, stripe_tour  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_or_opt_nl.json")
NEW_SYMBOLS = ["tspgpu_or_opt_nl_once", "tspgpu_or_opt_nl", "tspgpu_tour_or_opt_nl", "tspgpu_local_search_nl",
               "tspgpu_tour_local_search_nl", "tspgpu_time_or_nl_sweep"]
KINDS = {(1, 0), (2, 0), (2, 1), (3, 0), (3, 1)}


# --------------------------------------------------------------------------------------------------------- restatement
def pack(L, q, rev):
    return L << 18 | q << 1 | rev


def tour_from_zero(path):
    n = len(path)
    P, order, v = [0] * n, [0] * n, 0
    for i in range(n):
        P[v], order[i] = i, v
        v = int(path[v])
    return P, order


def all_moves(c, path, lists=None):
    """every (delta, s, L, q, rev) rule 1 allows whose segment avoids node 0; lists: only those with the membership property"""
    n = len(path)
    path = [int(v) for v in path]
    pred = {path[v]: v for v in range(n)}
    for s in range(1, n):
        seg = [s, path[s], path[path[s]]]
        p = pred[s]
        for L in (1, 2, 3):
            if 0 in seg[:L]:
                break
            t = seg[L - 1]
            x = path[t]
            for q in range(n):
                if q in seg[:L] or q == p:
                    continue
                qn = path[q]
                for rev in ((0, 1) if L > 1 else (0,)):
                    h, e = (t, s) if rev else (s, t)
                    if lists is not None and not (q in lists[h] or qn in lists[e]):        # rule 3
                        continue
                    d = ((c[p][x] + c[q][h]) + c[e][qn]) - ((c[p][s] + c[t][x]) + c[q][qn])
                    yield d, s, L, q, rev


def brute_sweep(c, path, lists):
    """rules 1-6 as plain Python -> dict like model_or_sweep's plus the resulting path and what the sweep shows"""
    n = len(path)
    P, order = tour_from_zero(path)
    raw = [None] * n
    for d, s, L, q, rev in all_moves(c, path, lists):
        k = (d, L, q, rev)
        if raw[s] is None or k < raw[s]:
            raw[s] = k
    cand = []
    for s in range(n):
        if raw[s] is None or not raw[s][0] < EPS:
            continue
        d, L, q, rev = raw[s]
        i, j = P[s], P[q]
        lo, hi = min(i - 1, j), max(i + L - 1, j)
        assert 0 <= lo < hi <= n - 1
        cand.append((d, s, pack(L, q, rev), lo, hi))
    key = [x[:3] for x in cand]
    m = len(cand)
    conflict = [[x != y and cand[y][3] <= cand[x][4] and cand[x][3] <= cand[y][4] for y in range(m)] for x in range(m)]
    acc = [int(all(key[x] < key[y] for y in range(m) if conflict[x][y])) for x in range(m)]
    sel = sorted((x for x in range(m) if acc[x]), key=lambda x: key[x])
    tie = any(acc[x] and conflict[x][y] and cand[x][0] == cand[y][0] for x in range(m) for y in range(m))
    new_order = list(order)
    front = behind = 0
    for x in sel:                           # rule 4, in position space: the ranges are disjoint
        d, s, pk, lo, hi = cand[x]
        L, q, rev = unpack(pk)
        i, j = P[s], P[q]
        seg = order[i:i + L][::-1] if rev else order[i:i + L]
        if j > i:
            new_order[i - 1:j + 1] = [order[i - 1]] + order[i + L:j + 1] + seg
            behind += 1
        else:
            new_order[j:i + L] = [order[j]] + seg + order[j + 1:i]
            front += 1
    new = [0] * n
    for i in range(n):
        new[new_order[i]] = new_order[(i + 1) % n]
    ends = sorted((cand[x][3], cand[x][4]) for x in sel)
    shared = any(a[1] + 1 == b[0] for a, b in zip(ends, ends[1:]))
    return {"raw_d": [r[0] if r else None for r in raw], "raw_b": [pack(*r[1:]) if r else -1 for r in raw], "cand": cand, "acc": acc,
            "moves": [(cand[x][1],) + unpack(cand[x][2]) for x in sel], "deltas": [cand[x][0] for x in sel], "path": new,
            "tie": tie, "front": front, "behind": behind, "shared": shared}


def rect_lattice(w, h, step=10.0):
    return np.array([(x * step, y * step) for y in range(h) for x in range(w)], dtype=np.float64)


def small_cases():
    """the families of test_two_opt_nl.small_cases at the sizes of this rule: integer-rounded points, a real-valued matrix, few
    distinct values, and the lattice (17 is prime: no lattice of that size)"""
    rng = np.random.default_rng(2025)
    for n in (8, 9, 17, 18, 40):
        yield "points%d" % n, O.cost_matrix(rng.integers(0, 40, (n, 2)).astype(np.float64)), random_tour(n, rng)
        yield "real%d" % n, sym_int_matrix(n, rng) + symmetric_noise(n, rng), random_tour(n, rng)
        yield "fewvalues%d" % n, sym_int_matrix(n, rng, hi=3), random_tour(n, rng)
    for w, h in ((4, 2), (3, 3), (6, 3), (8, 5)):
        yield "lattice%d" % (w * h), O.cost_matrix(rect_lattice(w, h)), random_tour(w * h, rng)


def restricted_improving_moves(c, path, lists):
    """every Or-opt move with the membership property, a segment without node 0 and delta < EPS, by brute force"""
    return [mv for mv in all_moves(c, path, lists) if mv[0] < EPS]


# ------------------------------------------------------------------------------------------------------------ CPU tests
def test_model_equals_brute_force_restatement():
    """every Or-opt sweep of the phase of rule 7: candidates per start, compacted candidates with their ranges, accepted flags,
    moves, deltas, path, cost.  The conditions at the end are the model's own on these seeds, not measurements of the device."""
    kinds, front, behind, most, shared, ties, multi = set(), 0, 0, 0, 0, 0, 0
    for name, c, start in small_cases():
        cl = c.tolist()
        integer = not name.startswith("real")
        for K in (1, 3, 8, 16):
            lists = brute_lists(cl, K)
            nodes, _ = model_lists(K, costs=c)
            assert nodes.tolist() == lists, (name, K)
            path = start.copy()
            cost = tour_cost(path, costs=c)
            for sweep in range(10 * len(c)):
                want = brute_sweep(cl, path, lists)
                got = model_or_sweep(path, cost, nodes, costs=c)
                tag = (name, K, sweep)
                assert [int(v) for v in got["raw_b"]] == want["raw_b"], tag
                assert all(float(gd) == wd for gd, wd in zip(got["raw_d"], want["raw_d"]) if wd is not None), tag
                assert got["cand"] == [(float(d), s, pk, lo, hi) for d, s, pk, lo, hi in want["cand"]], tag
                assert got["acc"] == want["acc"], tag
                assert [tuple(int(v) for v in mv) for mv in got["moves"]] == want["moves"], tag
                assert [float(v) for v in got["deltas"]] == [float(v) for v in want["deltas"]], tag
                assert [int(v) for v in path] == want["path"] and O.valid_tour(path), tag
                if integer:
                    assert got["cost"] == cost + sum(want["deltas"]) == tour_cost(path, costs=c), tag
                cost = got["cost"]
                kinds |= {(mv[1], mv[3]) for mv in want["moves"]}
                front, behind = front + want["front"], behind + want["behind"]
                most = max(most, len(want["moves"]))
                shared += want["shared"]
                ties += want["tie"]
                multi += len(want["moves"]) >= 2
                if not want["moves"]:
                    break
            else:
                raise AssertionError("no end of the Or-opt phase: %s" % (tag,))
            assert restricted_improving_moves(cl, path, lists) == [], (name, K)
    assert kinds == KINDS and front >= 10 and behind >= 10 and most >= 3 and shared >= 1 and ties >= 1 and multi >= 10


def test_model_coordinate_variant_equals_the_matrix_model():
    rng = np.random.default_rng(3)
    for kind in (EUC_2D, 1, CEIL_2D):
        for n in (8, 9, 40, 130):
            xy = rng.uniform(0, 500, (n, 2)) if kind != CEIL_2D or n % 2 else rng.integers(0, 500, (n, 2)).astype(np.float64)
            c = weight_matrix(xy, kind)
            nodes, _ = model_lists(8, costs=c)
            p1 = random_tour(n, rng)
            p2 = p1.copy()
            a, b = model_or_sweep(p1, 0.0, nodes, costs=c), model_or_sweep(p2, 0.0, nodes, xy=xy, kind=kind)
            assert a["cand"] == b["cand"] and a["acc"] == b["acc"] and np.array_equal(p1, p2) and a["cost"] == b["cost"]


def test_full_lists_give_the_or_opt_sweeps_move():
    """rule 9.  K' = n - 1: the smallest key of a sweep is the move of tests/or_opt_model.c whenever that move's segment does
    not contain node 0"""
    from test_or_opt import best_move
    rng = np.random.default_rng(19)
    checked = skipped = 0
    for n in range(8, 18):
        for c in (O.cost_matrix(rng.integers(0, 30, (n, 2)).astype(np.float64)), sym_int_matrix(n, rng) + symmetric_noise(n, rng)):
            nodes, _ = model_lists(16, costs=c)
            assert nodes.shape[1] == n - 1
            path = random_tour(n, rng)
            for sweep in range(10 * n):
                d, s, L, q, rev = best_move(c, path)
                seg = [s, int(path[s]), int(path[path[s]])][:max(L, 1)]
                r = model_or_sweep(path, 0.0, nodes, costs=c)
                if d < EPS and 0 not in seg:
                    assert tuple(int(v) for v in r["moves"][0]) == (s, L, q, rev) and r["deltas"][0] == d, (n, sweep)
                    checked += 1
                else:
                    skipped += 1
                if not len(r["moves"]):
                    break
    assert checked >= 50 and skipped >= 10


def test_descent_ends_in_an_optimum_of_both_list_neighbourhoods():
    """rule 8: the model's descent ends (the sweep limit is a safety net), counts as the rule says, and leaves no improving
    move with the membership property of either neighbourhood (rule 3 by brute force over all candidates)"""
    rng = np.random.default_rng(12)
    several = 0
    for n, K in ((8, 3), (9, 2), (17, 3), (64, 1), (64, 3), (64, 8), (200, 2), (200, 5), (40, 4)):
        c = O.cost_matrix(rect_lattice(8, 5)) if n == 40 else O.cost_matrix(O.random_points(n, 40 + n))
        nodes, _ = model_lists(K, costs=c)
        lists = nodes.tolist()
        path = random_tour(n, rng)
        r = model_ls_descent(path, nodes, costs=c, limit_sweeps=100 * n)
        assert O.valid_tour(path) and r["cost"] == O.tour_cost(c, path)
        assert r["rounds"] >= 1 and r["two_opt_sweeps"] >= r["rounds"] and r["or_sweeps"] >= r["rounds"]
        assert restricted_improving_pairs(c.tolist(), path, lists) == []
        assert restricted_improving_moves(c.tolist(), path, lists) == []
        again = path.copy()
        r2 = model_ls_descent(again, nodes, costs=c)
        assert np.array_equal(again, path) and (r2["rounds"], r2["two_opt_sweeps"], r2["or_sweeps"], r2["or_moves"]) == (1, 1, 1, 0)
        several += r["rounds"] >= 2
    assert several >= 3


@functools.lru_cache(maxsize=None)
def golden():
    return json.load(open(GOLDEN))


def test_golden_is_reproducible_from_the_model():
    g = golden()
    xy = G2.tsplib_points("pr1002")
    start = G2.nn_from(xy, 0)[0]
    assert digest(start) == g["pr1002"]["start_sha256"] and [d["K"] for d in g["pr1002"]["descents"]] == [5, 8]
    for want in g["pr1002"]["descents"]:
        got = G.descent_entry(xy, start, want["K"])
        assert got == want, want["K"]
        assert want["rounds"] >= 2 and want["or_moves"] >= 10 and want["max_moves"] >= 3
    big = g["n66000"]
    assert digest(stripe_tour(G2.large_points(big["n"], big["seed"]))) == big["start_sha256"] and big["n"] == 66000
    assert len(big["sweeps"]) == 3 and all(s["moves"] >= 2 for s in big["sweeps"])


def test_header_and_libraries_declare_the_entry_points():
    from travellingsalesmanoptimization_amd import _lib
    text = open(os.path.join(ROOT, "include", "tspgpu.h")).read()
    assert "Neighbour-list Or-opt" in text and text.index("Neighbour-list Or-opt") > text.index("Neighbour-list 2-opt")
    for s in NEW_SYMBOLS:
        assert ("int %s(tspgpu_ctx *ctx" % s) in text, s
        assert s in _lib.SIGNATURES and hasattr(_lib.load(), s), s
    section = text[text.index("Neighbour-list Or-opt"):]
    for word in ("Membership", "Range", "Conflict and selection", "Equality with the full rule", "refinment.c:6-9", "47 / 48"):
        assert word in section, word
    import travellingsalesmanoptimization_amd as T
    for m in ("or_opt_nl_once", "or_opt_nl", "tour_or_opt_nl", "local_search_nl", "tour_local_search_nl", "time_or_nl_sweep"):
        assert hasattr(T.Engine, m)


def test_no_context_means_14():
    from travellingsalesmanoptimization_amd import _lib
    L = _lib.load()
    null = C.c_void_p()
    path = np.roll(np.arange(8, dtype=np.int32), -1)
    cost, k, nr, ms = C.c_double(8.0), C.c_int(), C.c_int(), C.c_float()
    a, b, c, d = C.c_long(), C.c_long(), C.c_long(), C.c_long()
    mv, dl = np.zeros(32, np.int32), np.zeros(8)
    assert L.tspgpu_or_opt_nl_once(null, path, C.byref(cost), C.byref(k), mv, dl, 8) == _lib.UNAVAILABLE
    assert L.tspgpu_or_opt_nl(null, path, C.byref(cost), -1.0, C.byref(a), C.byref(b)) == _lib.UNAVAILABLE
    assert L.tspgpu_tour_or_opt_nl(null, 0, -1, -1.0, C.byref(a), C.byref(b)) == _lib.UNAVAILABLE
    assert L.tspgpu_local_search_nl(null, path, C.byref(cost), -1.0, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(nr)) == _lib.UNAVAILABLE
    assert L.tspgpu_tour_local_search_nl(null, 0, -1.0, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(nr)) == _lib.UNAVAILABLE
    assert L.tspgpu_time_or_nl_sweep(null, 0, 1, C.byref(ms)) == _lib.UNAVAILABLE
    assert np.array_equal(path, np.roll(np.arange(8), -1)) and cost.value == 8.0       # and no CPU fallback ran


# ------------------------------------------------------------------------------------------------------------ GPU tests
def model_phase(start, nodes, c, **src):
    """the sweeps of the model's Or-opt phase from `start`, one record per sweep (the last one accepts nothing)"""
    path = start.copy()
    cost = tour_cost(path, costs=c)
    out = []
    while True:
        r = model_or_sweep(path, cost, nodes, **src)
        cost = r["cost"]
        out.append((r["moves"], r["deltas"], path.copy(), cost))
        if len(r["moves"]) == 0:
            return out


def check_phase(eng, start, c, sweeps, what, exact_cost=True):
    """or_opt_nl_once repeated to the end of the phase against the model's sweeps: list, order, deltas, path, cost"""
    path = start.copy()
    cost = tour_cost(path, costs=c)
    for t, (moves, deltas, want_path, want_cost) in enumerate(sweeps):
        cost, mv, dl = eng.or_opt_nl_once(path, cost)
        assert np.array_equal(mv, moves), (what, t)
        assert np.array_equal(dl, deltas), (what, t)
        assert np.array_equal(path, want_path), (what, t)
        if exact_cost:
            assert cost == want_cost, (what, t)
        else:
            assert abs(cost - want_cost) <= 1e-9 * abs(want_cost), (what, t)
        info = eng.info()
        assert (info["or_nl_sweeps"], info["or_nl_moves"], info["or_nl_max_moves"]) == (1, len(moves), len(moves)), (what, t)
    return sum(len(s[0]) >= 2 for s in sweeps)


def run_phases(mode, n, Ks, seed=0):
    xy, kind = points_for(mode, n, seed)
    c = weight_matrix(xy, kind)
    src = source_of(mode, xy, kind, c)
    eng = engine_for(mode, xy, kind)
    multi = 0
    for K in Ks:
        eng.neighbours_build(K)
        nodes, _ = model_lists(K, **src)
        st = random_tour(n, np.random.default_rng(n + K))
        multi += check_phase(eng, st, c, model_phase(st, nodes, c, **src), (mode, n, K))
    return eng, multi


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 9, 17, 18, 40])
@pytest.mark.parametrize("mode", MODES)
def test_gpu_move_by_move(mode, n):
    """from a random tour to the end of the Or-opt phase, K = 1, 8, 16 (K' = n - 1 up to n = 17)"""
    eng, multi = run_phases(mode, n, (1, 8, 16))
    assert n < 40 or multi >= 1
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode,seed", [("u16", 2), ("mf_euc", 2)])
def test_gpu_cap_below_the_accepted_count(mode, seed):
    check_cap_refusal(mode, seed, 4, model_or_sweep,
                      lambda eng, *a: eng.L.tspgpu_or_opt_nl_once(eng.ctx, *a), lambda eng, p, c, cap: eng.or_opt_nl_once(p, c, cap=cap))


@pytest.mark.gpu
def test_gpu_move_by_move_with_real_costs():
    """f64 cells that hold non-integer costs: lists, moves, deltas (bit-exact) and paths are the model's; the cost is a sum of
    the accepted deltas in an order that is not specified: within 1e-9 relative of the model's"""
    rng = np.random.default_rng(64)
    for n in (9, 18, 40, 64):
        c = O.cost_matrix(O.random_points(n, 64 + n)) * (1.0 + symmetric_noise(n, rng))
        np.fill_diagonal(c, -1.0)
        eng = engine_for("f64", costs=c)
        multi = 0
        for K in (3, 8):
            eng.neighbours_build(K)
            nodes, _ = model_lists(K, costs=c)
            st = random_tour(n, rng)
            multi += check_phase(eng, st, c, model_phase(st, nodes, c, costs=c), (n, K), exact_cost=False)
        assert n < 40 or multi >= 1
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["u16", "mf_euc"])
def test_gpu_one_sweep_at_the_workgroup_boundaries(mode):
    """one below, at and one above a multiple of the sweep's segment starts per workgroup, read from the library"""
    eng, _ = run_phases(mode, 40, (5,))
    G_ = eng.info()["or_nl_starts"]
    eng.close()
    assert G_ >= 1
    for n in (9 * G_ - 1, 9 * G_, 9 * G_ + 1):
        xy, kind = points_for(mode, n, 1)
        c = weight_matrix(xy, kind)
        src = source_of(mode, xy, kind, c)
        eng = engine_for(mode, xy, kind)
        eng.neighbours_build(5)
        nodes, _ = model_lists(5, **src)
        st = random_tour(n, np.random.default_rng(n))
        check_phase(eng, st, c, model_phase(st, nodes, c, **src)[:1], (mode, n))
        eng.close()


# ---- the apply: planted moves around the chunk of the apply workgroup, in both slot directions
APPLY_CHUNK = 256       # threads of the apply workgroup = cells per chunk of the shifted block (tspgpu_ornl.inc)
LR = ((1, 0), (2, 0), (2, 1), (3, 0), (3, 1))


def planted_moves(n, spec):
    """spec: a list of ('behind' | 'front', cells of the shifted block, gap to the previous range) -> the moves
    [(i, L, j, rev)] in positions counted from node 0, ranges in ascending order, (L, rev) cycling through its five values"""
    out, at = [], 0
    for k, (where, m, gap) in enumerate(spec):
        L, rev = LR[k % 5]
        lo = at + gap
        if where == "behind":               # range [i - 1, j]: the block i + L .. j has m cells
            i = lo + 1
            j = i + L + m - 1
            hi = j
        else:                               # range [j, i + L - 1]: the block j + 1 .. i - 1 has m cells
            j = lo
            i = j + m + 1
            hi = i + L - 1
        assert hi <= n - 1, (n, spec)
        out.append((i, L, j, rev))
        at = hi
    return out


def planted_matrix(path, f, moves):
    """1000 + noise, the tour's edges 100, the three edges every planted move adds 1 (the matrix of
    test_or_opt_geometry.planted_move_matrix, for several moves at once)"""
    import test_or_opt_geometry as OG
    n = len(path)
    c = OG.noise_matrix(n).copy()
    idx = np.arange(n)
    c[idx, path] = 100.0
    c[path, idx] = 100.0
    for i, L, j, rev in moves:
        s, t, q = int(f[i]), int(f[i + L - 1]), int(f[j])
        p, x, qn = int(f[i - 1]), int(f[(i + L) % n]), int(f[(j + 1) % n])
        h, e = (t, s) if rev else (s, t)
        for u, v in ((p, x), (q, h), (e, qn)):
            c[u, v] = c[v, u] = 1.0
    return c


def apply_specs(n):
    ch = APPLY_CHUNK
    if n < 4 * ch:          # every block shorter than the chunk
        return [[("behind", 1, 1), ("behind", 2, 2), ("behind", 3, 2), ("behind", 40, 2), ("behind", 60, 2)],
                [("front", 1, 1), ("front", 2, 2), ("front", 3, 2), ("front", 40, 2), ("front", 60, 2)],
                [("behind", 5, 0), ("front", 7, 1), ("front", 1, 1), ("behind", 30, 3), ("front", 50, 2)]]
    return [[("behind", 1, 1), ("behind", 3, 2), ("behind", ch - 1, 2), ("behind", ch, 2), ("behind", ch + 1, 2)],
            [("front", 1, 1), ("front", 3, 2), ("front", ch - 1, 2), ("front", ch, 2), ("front", ch + 1, 2)],
            [("behind", 3 * ch + 5, 2), ("front", 2, 1), ("behind", 2, 1)],
            [("front", 3 * ch + 5, 0), ("behind", 7, 1), ("front", 9, 3)]]


def apply_cases(n):
    """-> dicts: tour0, flip (a, b, delta) or None, the matrix, the model's sweep on the tour after the flip, and the follow-ups"""
    import test_or_opt_geometry as OG
    from test_or_opt import best_move
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
            assert fl is None or cost - cost0 < EPS
            nodes, _ = model_lists(4, costs=c)
            start = path.copy()
            r = model_or_sweep(path, cost, nodes, costs=c)
            # every planted move is accepted (under its own name or that of the same exchange seen from the other block): three
            # edges of 1 for three of 100 -- but where the shifted block is one node next to the segment's end that faces it, the
            # edge between the two is removed and added again, and it is planted at 1: two edges of 100 go
            want = sorted(-198.0 if m == 1 and (L == 1 or rev == 1) else -297.0 for (_, m, _), (_, L, _, rev) in zip(spec, moves))
            assert sorted(r["deltas"]) == want, (n, spec, r["deltas"])
            two = path.copy()
            d2, c2, _ = O.two_opt_once(c, two, r["cost"])
            d3 = best_move(c, path)
            yield {"tour0": tour0, "flip": (fl[0], fl[1], cost - cost0) if fl else None, "c": c, "start": (start, cost), "sweep": r,
                   "after": path, "two": (two, c2, d2), "or": d3, "dir": lay.dir, "cell0": int(np.nonzero(lay.ord == 0)[0][0]),
                   "spec": spec}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [150, 1100])
@pytest.mark.parametrize("mode", ["u16", "f64"])
def test_gpu_apply_geometry(mode, n):
    """several planted moves per launch: shifted blocks shorter than, equal to and several times the apply workgroup's chunk,
    insertion behind and in front, on a freshly loaded slot and on one a 2-opt move left with dir = -1 and a rotated ord; then
    one 2-opt sweep (reads the edge costs by position) and one Or-opt move (reads successors and edge costs by node)"""
    from test_or_opt import apply_move
    import travellingsalesmanoptimization_amd as T
    eng = T.Engine(0)
    eng.set_option(T.OPT_ELEM, {"u16": 3, "f64": 1}[mode])
    dirs, rotated, blocks = set(), False, set()
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
        sw, mv, rc = eng.tour_or_opt_nl(0, max_sweeps=1)
        assert (sw, mv, rc) == (1, len(r["moves"]), 0), case["spec"]
        path, cost, delta = eng.tour_store(0)
        assert np.array_equal(path, case["after"]) and (cost, delta) == (r["cost"], -297.0) and r["deltas"][0] == -297.0, case["spec"]
        assert eng.info()["or_nl_max_moves"] == len(r["moves"]) >= 2
        eng.tour_copy(1, 0)
        assert eng.tour_two_opt(1, max_sweeps=1) == (1, 0)
        path, cost, delta = eng.tour_store(1)
        assert np.array_equal(path, case["two"][0]) and (cost, delta) == case["two"][1:], case["spec"]
        d3, s, L, q, rev = case["or"]
        want = case["after"].copy()
        if d3 < EPS:
            apply_move(want, s, L, q, rev)
        assert eng.tour_or_opt(0, max_moves=1) == (1 if d3 < EPS else 0, 0)
        path, cost, _ = eng.tour_store(0)
        assert np.array_equal(path, want) and cost == r["cost"] + (d3 if d3 < EPS else 0.0), case["spec"]
        dirs.add(case["dir"])
        rotated |= case["cell0"] != 0
        blocks |= {m for _, m, _ in case["spec"]}
    assert dirs == {1, -1} and rotated and eng.info()["elem"] == {"u16": 3, "f64": 1}[mode]
    assert n < 4 * APPLY_CHUNK or {APPLY_CHUNK - 1, APPLY_CHUNK, APPLY_CHUNK + 1, 3 * APPLY_CHUNK + 5} <= blocks
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["u16", "f64", "mf_euc"])
def test_gpu_slot_invariants(mode):
    """after every neighbour-list Or-opt sweep of a short descent, one call each of the other slot calls equals its model on
    the stored tour: tour_two_opt (one sweep), tour_or_opt (one move), tour_two_opt_nl and tour_two_opt_multi (one sweep)"""
    from test_or_opt import apply_move, best_move
    import travellingsalesmanoptimization_amd as T
    n, K = 200, 6
    xy, kind = points_for(mode, n, 2)
    c = weight_matrix(xy, kind)
    eng = engine_for(mode, xy, kind)
    if mode.startswith("mf"):
        eng.set_option(T._lib.OPT_OR_MATRIX_FREE, 1)
    eng.neighbours_build(K)
    nodes, _ = model_lists(K, costs=c)
    want = random_tour(n, np.random.default_rng(5))
    cost = tour_cost(want, costs=c)
    eng.tour_load(0, want)
    eng.tour_two_opt(0, max_sweeps=3)               # (the shorter arc is reversed: direction and rotation of the slot change)
    want, cost, _ = eng.tour_store(0)
    for sweep in range(4):
        r = model_or_sweep(want, cost, nodes, costs=c)
        cost = r["cost"]
        assert eng.tour_or_opt_nl(0, max_sweeps=1) == (1, len(r["moves"]), 0)
        got, gcost, gdelta = eng.tour_store(0)
        assert np.array_equal(got, want) and gcost == cost and gdelta == (r["deltas"][0] if len(r["deltas"]) else 0.0), sweep
        assert len(r["moves"]) >= 1, "the walk is too short for this test"
        # the reference's sweep
        eng.tour_copy(1, 0)
        assert eng.tour_two_opt(1, max_sweeps=1) == (1, 0)
        w = want.copy()
        d, wc, _ = O.two_opt_once(c, w, cost)
        got, gcost, gdelta = eng.tour_store(1)
        assert np.array_equal(got, w) and (gcost, gdelta) == (wc, d), sweep
        # Or-opt's move
        eng.tour_copy(1, 0)
        d, s, L, q, rev = best_move(c, want)
        w = want.copy()
        if d < EPS:
            apply_move(w, s, L, q, rev)
        assert eng.tour_or_opt(1, max_moves=1) == (1 if d < EPS else 0, 0)
        got, gcost, _ = eng.tour_store(1)
        assert np.array_equal(got, w) and gcost == cost + (d if d < EPS else 0.0), sweep
        # the neighbour-list 2-opt sweep and the parallel-move sweep
        for call, lists in ((eng.tour_two_opt_nl, nodes), (eng.tour_two_opt_multi, None)):
            eng.tour_copy(1, 0)
            w = want.copy()
            m = model_sweep(w, cost, lists, costs=c)
            assert call(1, max_sweeps=1) == (1, len(m["moves"]), 0)
            got, gcost, _ = eng.tour_store(1)
            assert np.array_equal(got, w) and gcost == m["cost"], (sweep, lists is None)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["u16", "mf_euc"])
@pytest.mark.parametrize("K", [5, 8])
def test_gpu_descent_pr1002(mode, K):
    """local_search_nl from NN(0) against the golden of the model: counters, rounds, tour and cost; the slot form too"""
    g = golden()["pr1002"]
    want = next(d for d in g["descents"] if d["K"] == K)
    xy = O.read_tsplib(os.path.join(DATA, "pr1002.tsp"))[0]
    eng = engine_for(mode, xy, EUC_2D)
    eng.neighbours_build(K)
    start, _ = eng.nn_tour(0)
    assert digest(start) == g["start_sha256"]
    path = start.copy()
    r = eng.local_search_nl(path)
    keys = ("cost", "two_opt_sweeps", "two_opt_moves", "or_sweeps", "or_moves", "rounds")
    assert r["rc"] == 0 and {k: r[k] for k in keys} == {k: want[k] for k in keys}
    assert digest(path) == want["path_sha256"]
    info = eng.info()
    assert (info["or_nl_sweeps"], info["or_nl_moves"], info["or_nl_max_moves"], info["or_nl_rounds"]) == \
        (want["or_sweeps"], want["or_moves"], want["max_moves"], want["rounds"])
    eng.tour_load(1, start)
    r1 = eng.tour_local_search_nl(1)
    got, gcost, _ = eng.tour_store(1)
    assert r1["rc"] == 0 and {k: r1[k] for k in keys[1:]} == {k: want[k] for k in keys[1:]}
    assert np.array_equal(got, path) and gcost == want["cost"]
    # the Or-opt phase alone on the result: one empty sweep, the caller's cost kept
    cost, sw, mv, rc = eng.or_opt_nl(path, 123.0)
    assert (cost, sw, mv, rc) == (123.0, 1, 0, 0) and digest(path) == want["path_sha256"]
    eng.close()


@pytest.mark.gpu
def test_gpu_large_instance_three_sweeps():
    """n = 66 000, matrix-free, EUC_2D, K = 8: the first three Or-opt sweeps from the stripe tour against the golden"""
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
        cost, mv, dl = eng.or_opt_nl_once(path, cost)
        assert len(mv) == want["moves"] and cost == want["cost"], t
        assert digest(mv) == want["moves_sha256"] and float(dl.sum()) == want["delta_sum"] and digest(path) == want["path_sha256"], t
    eng.close()


@pytest.mark.gpu
def test_gpu_refusals_and_limits():
    from travellingsalesmanoptimization_amd import TspGpuError
    import travellingsalesmanoptimization_amd as T
    rng = np.random.default_rng(1)
    n = 40
    c = sym_int_matrix(n, rng)
    path = random_tour(n, rng)
    keep = path.copy()
    eng = engine_for("u16", costs=c)
    eng.tour_load(0, path)
    calls = (lambda: eng.or_opt_nl_once(path, 0.0), lambda: eng.or_opt_nl(path, 0.0), lambda: eng.local_search_nl(path),
             lambda: eng.tour_or_opt_nl(0), lambda: eng.tour_local_search_nl(0), lambda: eng.time_or_nl_sweep(0, 1))

    def refused(code, word=None):
        for call in calls:
            with pytest.raises(TspGpuError) as e:
                call()
            assert e.value.code == code and (word is None or word in str(e.value)) and np.array_equal(path, keep)
    # no lists yet: 9 with the text of nl_check
    refused(9, "no neighbour lists: call tspgpu_neighbours_build first")
    # lists of another cost source: 9, with the reason
    eng.neighbours_build(8)
    eng.set_costs(sym_int_matrix(n, rng))
    eng.tour_load(0, path)
    refused(9, "invalidated by a new cost source")
    # an asymmetric matrix: 9
    asym = c.copy()
    asym[3][7] += 5.0
    eng.set_costs(asym)
    eng.tour_load(0, path)
    refused(9, "symmetric")
    # no costs: 9
    fresh = T.Engine(0)
    with pytest.raises(TspGpuError) as e:
        fresh.or_opt_nl(np.roll(np.arange(8, dtype=np.int32), -1), 0.0)
    assert e.value.code == 9
    fresh.close()
    # n = 7: 3, with lists in place
    eng.set_points(O.random_points(7, 3), EUC_2D)
    eng.build_costs()
    eng.neighbours_build(16)
    small = np.roll(np.arange(7, dtype=np.int32), -1)
    for call in (lambda: eng.or_opt_nl(small, 0.0), lambda: eng.local_search_nl(small), lambda: eng.or_opt_nl_once(small, 0.0)):
        with pytest.raises(TspGpuError) as e:
            call()
        assert e.value.code == 3 and "8 nodes" in str(e.value)
    # cap below the accepted count: 8, the path and the cost as they were, nothing written
    n = 300
    xy = O.random_points(n, 8)
    cc = O.cost_matrix(xy)
    eng.set_points(xy)
    eng.build_costs()
    eng.neighbours_build(8)
    nodes, _ = model_lists(8, costs=cc)
    path = nn0(cc)
    O.two_opt(cc, path)                     # (from a 2-opt optimum the improving segment moves are short: several fit one sweep)
    keep = path.copy()
    k = len(model_or_sweep(path.copy(), 0.0, nodes, costs=cc)["moves"])
    assert k >= 2
    L = eng.L
    mv, dl = np.full(4 * n, -7, np.int32), np.full(n, -7.0)
    cost, cnt = C.c_double(123.0), C.c_int(-7)
    assert L.tspgpu_or_opt_nl_once(eng.ctx, path, C.byref(cost), C.byref(cnt), mv, dl, k - 1) == 8
    assert np.array_equal(path, keep) and cost.value == 123.0 and cnt.value == -7 and np.all(mv == -7) and np.all(dl == -7.0)
    cost, mv, dl = eng.or_opt_nl_once(path, 123.0, cap=k)
    assert len(mv) == k and cost == 123.0 + dl.sum() and O.valid_tour(path)
    # a deadline of 0: 4, a valid tour and its cost
    path = random_tour(n, np.random.default_rng(9))
    keep = path.copy()
    r = eng.local_search_nl(path, time_left_s=0.0)
    assert r["rc"] == 4 and np.array_equal(path, keep) and r["cost"] == O.tour_cost(cc, path)
    cost, sw, mv, rc = eng.or_opt_nl(path, 55.0, time_left_s=0.0)
    assert (rc, cost, sw, mv) == (4, 55.0, 0, 0) and np.array_equal(path, keep)
    eng.tour_load(0, path)
    assert eng.tour_or_opt_nl(0, time_left_s=0.0)[2] == 4 and eng.tour_local_search_nl(0, time_left_s=0.0)["rc"] == 4
    assert eng.time_or_nl_sweep(0, 2) > 0.0
    got, gcost, _ = eng.tour_store(0)
    assert np.array_equal(got, path) and gcost == r["cost"]        # timing applies nothing
    # matrix-free mode needs no TSPGPU_OPT_OR_MATRIX_FREE here, and the existing entry points keep their code 12
    mf = engine_for("mf_euc", xy, EUC_2D)
    mf.neighbours_build(8)
    p1, p2 = keep.copy(), keep.copy()
    r = mf.local_search_nl(p1)
    m = model_ls_descent(p2, nodes, costs=cc)
    assert r["rc"] == 0 and np.array_equal(p1, p2) and r["cost"] == m["cost"]
    with pytest.raises(TspGpuError) as e:
        mf.local_search(keep.copy())
    assert e.value.code == 12
    mf.close()
    eng.close()


# ----------------------------------------------------------------------------------------------------------------- host
def run_tsp(*args, env_set=None, timeout=300):
    import subprocess
    env = dict(os.environ)
    for k in ("TSP_2OPT_MULTI", "TSP_2OPT_NEIGHBOURS", "TSP_2OPT_NEIGHBOURS_POLISH", "TSP_OR_OPT", "TSP_OR_OPT_NEIGHBOURS",
              "TSP_OR_OPT_MATRIX_FREE", "TSP_OR_OPT_EVERY_START"):
        env.pop(k, None)
    env.update(env_set or {})
    os.makedirs(os.path.join(ROOT, "results"), exist_ok=True)
    r = subprocess.run([os.path.join(ROOT, "travellingsalesmanoptimization_amd", "host", "tsp"), *args], capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=ROOT)
    return r.returncode, r.stdout.strip(), r.stderr


@pytest.mark.gpu
def test_host_binary_runs_the_descent_over_the_lists():
    """`-alg VNS -k 1` leaves ref_2opt's local optimum of the best nearest-neighbour tour as the incumbent; with TSP_OR_OPT=1
    and TSP_OR_OPT_NEIGHBOURS=8 the polish is the golden's descent from that tour.  The golden's start is checked against the
    device's nearest-neighbour tours and the oracle's 2-opt, so that a difference below is the polish's"""
    g = golden()["pr1002_best_nn_two_opt"]
    want = g["descents"][0]
    assert want["K"] == 8 and want["cost"] < g["start_cost"]
    xy = O.read_tsplib(os.path.join(DATA, "pr1002.tsp"))[0]
    eng = engine_for("u16", xy, EUC_2D)
    start, _, _ = eng.nn_all()
    eng.close()
    _, cost = O.two_opt(O.cost_matrix(xy), start)
    assert digest(start) == g["start_sha256"] and cost == g["start_cost"]
    args = ("-f", os.path.join(DATA, "pr1002.tsp"), "-alg", "VNS", "-k", "1", "-seed", "1")
    rc, out, err = run_tsp(*args, "-q")
    assert rc == 0 and out == "Cost: %.2f" % g["start_cost"], err
    rc, out, err = run_tsp(*args, "-q", env_set={"TSP_OR_OPT": "1", "TSP_OR_OPT_NEIGHBOURS": "8"})
    assert rc == 0 and out == "Cost: %.2f" % want["cost"], err
    # the same lists for both switches: ref_2opt runs the neighbour-list 2-opt, the polish goes on from its optimum
    both = golden()["pr1002_best_nn"]["descents"][0]
    rc, out, err = run_tsp(*args, "-q", env_set={"TSP_OR_OPT": "1", "TSP_OR_OPT_NEIGHBOURS": "8", "TSP_2OPT_NEIGHBOURS": "8",
                                                 "TSP_2OPT_NEIGHBOURS_POLISH": "0"})
    assert rc == 0 and out == "Cost: %.2f" % both["cost"], err
    # without TSP_OR_OPT=1 it says that it has no effect, and has none
    rc, out, err = run_tsp(*args, "-q", env_set={"TSP_OR_OPT_NEIGHBOURS": "8"})
    assert rc == 0 and out == "Cost: %.2f" % g["start_cost"], err
    rc, out, err = run_tsp(*args, env_set={"TSP_OR_OPT_NEIGHBOURS": "8"})
    assert rc == 0 and "TSP_OR_OPT_NEIGHBOURS=8 has no effect" in out + err


@pytest.mark.gpu
def test_host_switch_values():
    args = ("-f", os.path.join(DATA, "kroA100.tsp"), "-alg", "VNS", "-k", "20", "-q")
    for bad in ("17", "-1", "eight", ""):
        rc, out, err = run_tsp(*args, env_set={"TSP_OR_OPT": "1", "TSP_OR_OPT_NEIGHBOURS": bad})
        assert rc != 0 and "TSP_OR_OPT_NEIGHBOURS" in err and "1 to 16" in err, bad
    rc, out, err = run_tsp(*args, env_set={"TSP_OR_OPT": "1", "TSP_OR_OPT_NEIGHBOURS": "8", "TSP_2OPT_NEIGHBOURS": "5"})
    assert rc != 0 and "TSP_OR_OPT_NEIGHBOURS=8" in err and "TSP_2OPT_NEIGHBOURS=5" in err
    plain = run_tsp(*args, env_set={"TSP_OR_OPT": "1"})
    assert plain[0] == 0 and run_tsp(*args, env_set={"TSP_OR_OPT": "1", "TSP_OR_OPT_NEIGHBOURS": "0"}) == plain
    # a matrix-free instance is taken without TSP_OR_OPT_MATRIX_FREE
    mf = {"TSP_OR_OPT": "1", "TSP_OR_OPT_NEIGHBOURS": "8", "TSP_MATRIX_FREE": "1"}
    rc, out, err = run_tsp(*args[:-1], env_set=mf)
    assert rc == 0 and "the polish is skipped" not in out + err
    rc, out, err = run_tsp(*args, env_set=mf)
    rc0, out0, _ = run_tsp(*args, env_set={"TSP_MATRIX_FREE": "1"})
    assert rc == 0 and rc0 == 0 and out.startswith("Cost: ") and float(out[6:]) <= float(out0[6:]), (out, out0)
