"""Neighbour-list 2-opt (include/tspgpu.h "Neighbour-list 2-opt"): K-nearest-neighbour lists, a candidate sweep
over them, and the parallel-move selection and apply behind it.

The model is tests/two_opt_nl_model.c (wrappers in tools/make_golden_two_opt_nl.py), pinned here to a brute-force Python
restatement (brute_lists, brute_sweep).
CPU: model against restatement, equality with the parallel-move model at K' = n - 1, the membership property, the end of the
descent and of the polish, the golden, the header and the exported symbols.
GPU: the lists in every cell type and weight form, move by move to the local optimum, equality with tspgpu_two_opt_multi_once,
rotation and direction of the slot, the slot's invariants, the descents against the golden, n = 66 000, refusals, the host
binary's TSP_2OPT_NEIGHBOURS."""
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
import make_golden_two_opt_nl as G  # noqa: E402
from make_golden_two_opt_nl import model_descent, model_lists, model_sweep  # noqa: E402
from test_two_opt_multi import (CEIL_2D, EPS, EUC_2D, MODES, engine_for, nn0, points_for, random_tour,  # noqa: E402
                                slot_after_two_opt, sym_int_matrix, symmetric_noise, tour_cost, weight_matrix)

DATA = os.path.join(ROOT, "tests", "golden", "data")
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_two_opt_nl.json")
NEW_SYMBOLS = ["tspgpu_neighbours_build", "tspgpu_neighbours_get", "tspgpu_two_opt_nl_once", "tspgpu_two_opt_nl",
               "tspgpu_tour_two_opt_nl", "tspgpu_time_nl_sweep"]


# --------------------------------------------------------------------------------------------------------- restatement
def brute_lists(c, K):
    n = len(c)
    return [[u for _, u in sorted((c[v][u], u) for u in range(n) if u != v)[:min(K, n - 1)]] for v in range(n)]


def candidates_of(path, lists, a):
    """B(a) before the reference's skip test"""
    pred = {int(path[v]): v for v in range(len(path))}
    return set(lists[a]) | {pred[x] for x in lists[int(path[a])]}


def brute_sweep(c, path, lists):
    """the rule as plain Python over lists -> dict like model_sweep's plus the resulting path"""
    n = len(path)
    path = [int(v) for v in path]
    P, order, v = [0] * n, [0] * n, 0
    for i in range(n):
        P[v], order[i] = i, v
        v = path[v]
    raw_d, raw_b = [None] * n, [-1] * n
    for a in range(n):
        sa = path[a]
        for b in sorted(candidates_of(path, lists, a)):
            sb = path[b]
            if sa == sb or a == sb or b == sa:
                continue
            d = (c[a][b] + c[sa][sb]) - (c[a][sa] + c[b][sb])
            if raw_d[a] is None or d < raw_d[a]:
                raw_d[a], raw_b[a] = d, b
    cand, seen = [], set()
    for a in range(n):
        b = raw_b[a]
        if b < 0 or not raw_d[a] < EPS or (raw_b[b] == a and frozenset((a, b)) in seen):
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
    return {"raw_d": raw_d, "raw_b": raw_b, "cand": cand, "acc": acc, "moves": [(cand[x][1], cand[x][2]) for x in sel],
            "deltas": [cand[x][0] for x in sel], "path": new}


def lattice(side, step=10.0):
    g = np.arange(side) * step
    return np.array([(x, y) for y in g for x in g], dtype=np.float64)


def small_cases():
    """(name, matrix, start): integer-rounded points, a real-valued matrix, few distinct values, and the 6 x 6 lattice"""
    rng = np.random.default_rng(2024)
    for n in (5, 8, 17, 40):
        yield "points%d" % n, O.cost_matrix(rng.integers(0, 40, (n, 2)).astype(np.float64)), random_tour(n, rng)
        yield "real%d" % n, sym_int_matrix(n, rng) + symmetric_noise(n, rng), random_tour(n, rng)
        yield "fewvalues%d" % n, sym_int_matrix(n, rng, hi=3), random_tour(n, rng)
    yield "lattice36", O.cost_matrix(lattice(6)), random_tour(36, rng)
    yield "lattice36_nn", O.cost_matrix(lattice(6)), nn0(O.cost_matrix(lattice(6)))


def restricted_improving_pairs(c, path, lists):
    """every pair with the membership property and delta < EPS, by brute force over all pairs"""
    n = len(path)
    out = []
    for a in range(n):
        sa = int(path[a])
        for b in range(a + 1, n):
            sb = int(path[b])
            if sa == sb or a == sb or b == sa:
                continue
            if not (b in lists[a] or a in lists[b] or sb in lists[sa] or sa in lists[sb]):
                continue
            if (c[a][b] + c[sa][sb]) - (c[a][sa] + c[b][sb]) < EPS:
                out.append((a, b))
    return out


# ------------------------------------------------------------------------------------------------------------ CPU tests
def test_model_equals_brute_force_restatement():
    """the lists, and every sweep of the descent: candidates per node, compacted candidates, accepted flags, moves, path"""
    multi = ties = 0
    for name, c, start in small_cases():
        cl = c.tolist()
        for K in (1, 3, 8, 16):
            want_lists = brute_lists(cl, K)
            nodes, w = model_lists(K, costs=c)
            assert nodes.tolist() == want_lists, (name, K)
            assert all(w[v][j] == cl[v][u] for v in range(len(c)) for j, u in enumerate(want_lists[v])), (name, K)
            ties += any(w[v][j] == w[v][j + 1] for v in range(len(c)) for j in range(nodes.shape[1] - 1))
            path = start.copy()
            cost = tour_cost(path, costs=c)
            for sweep in range(10 * len(c)):
                want = brute_sweep(cl, path, want_lists)
                got = model_sweep(path, cost, nodes, costs=c)
                tag = (name, K, sweep)
                assert [int(v) for v in got["raw_b"]] == want["raw_b"], tag
                assert all(wd is None or float(gd) == wd for gd, wd in zip(got["raw_d"], want["raw_d"])), tag
                assert got["cand"] == [(float(d), a, b, i, j) for d, a, b, i, j in want["cand"]], tag
                assert got["acc"] == want["acc"], tag
                assert [tuple(int(v) for v in mv) for mv in got["moves"]] == want["moves"], tag
                assert [float(v) for v in got["deltas"]] == [float(v) for v in want["deltas"]], tag
                assert [int(v) for v in path] == want["path"] and O.valid_tour(path), tag
                cost = got["cost"]
                multi += len(want["moves"]) >= 2
                if not want["moves"]:
                    break
            else:
                raise AssertionError("no end of the descent: %s" % (tag,))
    assert multi >= 10 and ties >= 10


def test_model_coordinate_variant_equals_the_matrix_model():
    rng = np.random.default_rng(3)
    for kind in (EUC_2D, 1, CEIL_2D):
        for n in (5, 9, 40, 130):
            xy = rng.uniform(0, 500, (n, 2)) if kind != CEIL_2D or n % 2 else rng.integers(0, 500, (n, 2)).astype(np.float64)
            c = weight_matrix(xy, kind)
            n1, w1 = model_lists(8, costs=c)
            n2, w2 = model_lists(8, xy=xy, kind=kind)
            assert np.array_equal(n1, n2) and np.array_equal(w1, w2)
            p1 = random_tour(n, rng)
            p2 = p1.copy()
            a, b = model_sweep(p1, 0.0, n1, costs=c), model_sweep(p2, 0.0, n2, xy=xy, kind=kind)
            assert a["cand"] == b["cand"] and a["acc"] == b["acc"] and np.array_equal(p1, p2) and a["cost"] == b["cost"]


def test_full_lists_give_the_parallel_move_sweep():
    """K' = n - 1: B(a) is everything the full rule looks at, the sweep is the parallel-move model's move for move"""
    rng = np.random.default_rng(17)
    for n in range(5, 18):
        for c in (O.cost_matrix(rng.integers(0, 30, (n, 2)).astype(np.float64)), sym_int_matrix(n, rng) + symmetric_noise(n, rng)):
            nodes, _ = model_lists(16, costs=c)
            assert nodes.shape[1] == n - 1
            path = random_tour(n, rng)
            for sweep in range(10 * n):
                p1, p2 = path.copy(), path.copy()
                a, b = model_sweep(p1, 0.0, nodes, costs=c), model_sweep(p2, 0.0, None, costs=c)
                assert np.array_equal(a["raw_b"], b["raw_b"]) and np.array_equal(a["raw_d"], b["raw_d"]), (n, sweep)
                assert a["cand"] == b["cand"] and a["acc"] == b["acc"] and np.array_equal(a["moves"], b["moves"]), (n, sweep)
                assert np.array_equal(a["deltas"], b["deltas"]) and np.array_equal(p1, p2), (n, sweep)
                path = p1
                if not len(a["moves"]):
                    break


def test_membership_property():
    """{a, b} is in B(a) or B(b) iff (a, b) or (sa, sb) joins a node to a member of its own list, in either direction"""
    rng = np.random.default_rng(23)
    checked = inside = 0
    for n, K in ((8, 1), (8, 3), (17, 3), (40, 5), (40, 8), (36, 4)):
        c = (O.cost_matrix(lattice(6)) if n == 36 else O.cost_matrix(rng.integers(0, 60, (n, 2)).astype(np.float64))).tolist()
        lists = brute_lists(c, K)
        path = random_tour(n, rng)
        B = [candidates_of(path, lists, a) for a in range(n)]
        for a in range(n):
            sa = int(path[a])
            for b in range(n):
                sb = int(path[b])
                if b == a or sa == sb or a == sb or b == sa:
                    continue
                edges = b in lists[a] or a in lists[b] or sb in lists[sa] or sa in lists[sb]
                assert (b in B[a] or a in B[b]) == edges, (n, K, a, b)
                checked += 1
                inside += edges
    assert 0 < inside < checked


def test_descent_ends_in_a_list_optimum_and_the_polish_in_a_two_opt_optimum():
    rng = np.random.default_rng(12)
    gaps = 0
    for n, K in ((5, 3), (6, 2), (17, 3), (64, 1), (64, 3), (64, 8), (200, 2), (200, 5), (36, 4)):
        c = O.cost_matrix(lattice(6)) if n == 36 else O.cost_matrix(O.random_points(n, 40 + n))
        nodes, _ = model_lists(K, costs=c)
        lists = nodes.tolist()
        start = random_tour(n, rng)
        path = start.copy()
        r = model_descent(path, nodes, False, costs=c)
        assert O.valid_tour(path) and r["cost"] == O.tour_cost(c, path) and r["sweeps"] >= 1 and r["polish_sweeps"] == 0
        assert restricted_improving_pairs(c.tolist(), path, lists) == []
        full = start.copy()
        p = model_descent(full, nodes, True, costs=c)
        assert np.array_equal(p["nl_path"], path) and (p["nl_cost"], p["sweeps"], p["moves"]) == (r["cost"], r["sweeps"], r["moves"])
        assert O.valid_tour(full) and p["cost"] == O.tour_cost(c, full) and p["polish_sweeps"] >= 1
        d, _, _ = O.two_opt_once(c, full.copy(), p["cost"])
        assert not d < EPS
        gaps += p["polish_moves"] > 0
    assert gaps >= 1        # the list optimum is in general not a 2-opt optimum


def test_golden_is_reproducible_from_the_model():
    g = json.load(open(GOLDEN))
    for name in ("pr1002", "fnl4461"):
        xy = G.tsplib_points(name)
        start = G.nn_from(xy, 0)[0]
        assert G.digest(start) == g[name]["start_sha256"] and [d["K"] for d in g[name]["descents"]] == [5, 8]
        for want in g[name]["descents"]:
            polish = name == "pr1002"       # (fnl4461: the polish phase is the n^2 model, checked on the device against this file)
            got = G.descent_entry(xy, start, want["K"], polish=polish)
            assert all(want[k] == v for k, v in got.items()), (name, want["K"])
    big = g["n66000"]
    xy = G.large_points(big["n"], big["seed"])
    assert G.digest(G.stripe_tour(xy)) == big["start_sha256"] and big["n"] == 66000 and big["moves"] >= 2 and big["max_label"] >= 65536


def test_header_and_libraries_declare_the_entry_points():
    from travellingsalesmanoptimization_amd import _lib
    text = open(os.path.join(ROOT, "include", "tspgpu.h")).read()
    assert "Neighbour-list 2-opt" in text and text.index("Neighbour-list 2-opt") > text.index("Parallel-move 2-opt")
    for s in NEW_SYMBOLS:
        assert ("int %s(tspgpu_ctx *ctx" % s) in text, s
        assert s in _lib.SIGNATURES and hasattr(_lib.load(), s), s
    host = C.CDLL(os.path.join(ROOT, "travellingsalesmanoptimization_amd", "host", "libtsphost.so"))
    assert hasattr(host, "ref_2opt")
    assert "src/algorithms/refinment.c:55" in text and "refinment.c:60-62" in text and "refinment.c:6-9" in text
    import travellingsalesmanoptimization_amd as T
    for m in ("neighbours_build", "neighbours_get", "two_opt_nl_once", "two_opt_nl", "tour_two_opt_nl", "time_nl_sweep"):
        assert hasattr(T.Engine, m)


def test_no_context_means_14():
    from travellingsalesmanoptimization_amd import _lib
    L = _lib.load()
    null = C.c_void_p()
    path = np.roll(np.arange(8, dtype=np.int32), -1)
    cost, k, sw, mv, ps, pm, ms = C.c_double(8.0), C.c_int(), C.c_long(), C.c_long(), C.c_long(), C.c_long(), C.c_float()
    ab, dl, nodes = np.zeros(16, np.int32), np.zeros(8), np.zeros(64, np.int32)
    assert L.tspgpu_neighbours_build(null, 8) == _lib.UNAVAILABLE
    assert L.tspgpu_neighbours_get(null, nodes, None) == _lib.UNAVAILABLE
    assert L.tspgpu_two_opt_nl_once(null, path, C.byref(cost), C.byref(k), ab, dl, 8) == _lib.UNAVAILABLE
    assert L.tspgpu_two_opt_nl(null, path, C.byref(cost), -1.0, 1, C.byref(sw), C.byref(mv), C.byref(ps), C.byref(pm)) == _lib.UNAVAILABLE
    assert L.tspgpu_tour_two_opt_nl(null, 0, -1, -1.0, C.byref(sw), C.byref(mv)) == _lib.UNAVAILABLE
    assert L.tspgpu_time_nl_sweep(null, 0, 1, C.byref(ms)) == _lib.UNAVAILABLE
    assert np.array_equal(path, np.roll(np.arange(8), -1)) and cost.value == 8.0       # and no CPU fallback ran


# ------------------------------------------------------------------------------------------------------------ GPU tests
def source_of(mode, xy, kind, c):
    return dict(xy=xy, kind=kind) if mode.startswith("mf") else dict(costs=c)


def check_lists(eng, K, c, what, **src):
    eng.neighbours_build(K)
    nodes, w = eng.neighbours_get()
    want, _ = model_lists(K, **src)
    assert eng.info()["nl_k"] == want.shape[1] == min(K, len(want) - 1), what
    assert np.array_equal(nodes, want), what
    if c is not None:
        assert np.array_equal(w, c[np.arange(len(c))[:, None], want]), what


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 6, 17, 63, 64, 65, 200, 1025])
@pytest.mark.parametrize("mode", MODES)
def test_gpu_lists(mode, n):
    """nodes, order and weights of the lists; the build has one loop over a row's 16-byte vectors, 64 per trip: a row of 32
    (n <= 32), of 64 and of 96 cells (n = 63, 64 | 65) is one trip with idle lanes, exactly one vector per lane in u16 / i32 /
    f64 cells at n = 512 / 256 / 128 -- 200 and 1025 lie on either side -- and 1025 is several trips"""
    xy, kind = points_for(mode, n, 0)
    c = weight_matrix(xy, kind)
    eng = engine_for(mode, xy, kind)
    for K in (1, 2, 8, 15, 16):
        check_lists(eng, K, c, (mode, n, K), **source_of(mode, xy, kind, c))
    eng.neighbours_build(0)
    assert eng.info()["nl_k"] == 0
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_lists_on_the_lattice(mode):
    """a 12 x 12 lattice: every list is full of equal distances, the order among them is the labels'"""
    xy = lattice(12)
    kind = {"mf_att": 1, "mf_ceil": CEIL_2D, "mf_ceil_int": CEIL_2D}.get(mode, EUC_2D)
    if mode == "mf_ceil":
        xy = xy + 0.5           # real coordinates: the generic CEIL_2D form
    c = weight_matrix(xy, kind)
    eng = engine_for(mode, xy, kind)
    for K in (1, 4, 8, 16):
        check_lists(eng, K, c, (mode, K), **source_of(mode, xy, kind, c))
    nodes, w = eng.neighbours_get()
    assert np.any(w[:, :-1] == w[:, 1:])
    eng.close()


@pytest.mark.gpu
def test_gpu_lists_of_a_real_valued_matrix():
    rng = np.random.default_rng(5)
    for n in (17, 130):
        c = sym_int_matrix(n, rng, hi=4) + np.round(symmetric_noise(n, rng), 1)      # doubles, many of them equal
        np.fill_diagonal(c, -1.0)
        eng = engine_for("f64", costs=c)
        for K in (3, 16):
            check_lists(eng, K, c, (n, K), costs=c)
        eng.close()


def large_instance(n, seed):
    return np.random.default_rng(seed).integers(0, 30000, (n, 2)).astype(np.float64)


def stripe_tour(xy, width=300.0):
    """the start of tools/make_golden_two_opt_nl.py: vertical stripes of `width`, upwards in even stripes, downwards in odd ones"""
    stripe = np.floor(xy[:, 0] / width).astype(np.int64)
    y = np.where(stripe % 2 == 0, xy[:, 1], -xy[:, 1])
    order = np.lexsort((np.arange(len(xy)), y, stripe)).astype(np.int32)
    path = np.empty(len(xy), np.int32)
    path[order] = np.roll(order, -1)
    return path


@pytest.mark.gpu
def test_gpu_large_instance_lists_and_one_sweep():
    """n = 66 000, matrix-free, EUC_2D, K = 8 against the golden of tools/make_golden_two_opt_nl.py (the C model over the
    coordinates): labels of 17 bits in the lists, the candidates and the moves"""
    g = json.load(open(GOLDEN))["n66000"]
    n = g["n"]
    xy = large_instance(n, g["seed"])
    eng = engine_for("mf_euc", xy, EUC_2D)
    eng.neighbours_build(g["K"])
    nodes, w = eng.neighbours_get()
    assert G.digest(nodes) == g["lists_sha256"] and int(nodes.max()) >= 65536
    rows = np.arange(0, n, 997)
    assert np.array_equal(w[rows], G.euc(xy, rows[:, None], nodes[rows]).astype(np.float64))
    path = stripe_tour(xy)
    assert G.digest(path) == g["start_sha256"]
    cost, mv, dl = eng.two_opt_nl_once(path, g["start_cost"])
    assert len(mv) == g["moves"] and cost == g["cost"]
    assert G.digest(mv) == g["moves_sha256"] and float(dl.sum()) == g["delta_sum"] and G.digest(path) == g["path_sha256"]
    assert int(mv.max()) >= 65536
    eng.close()


def model_walk(start, nodes, c, **src):
    """the sweeps of the model's descent from `start`, one record per sweep (the last one accepts nothing)"""
    path = start.copy()
    cost = tour_cost(path, costs=c)
    out = []
    while True:
        r = model_sweep(path, cost, nodes, **src)
        cost = r["cost"]
        out.append((r["moves"], r["deltas"], path.copy(), cost))
        if len(r["moves"]) == 0:
            return out


def check_walk(eng, start, c, sweeps, what):
    """two_opt_nl_once repeated to the optimum against the model's sweeps: list, order, deltas, path, cost"""
    path = start.copy()
    cost = tour_cost(path, costs=c)
    for t, (moves, deltas, want_path, want_cost) in enumerate(sweeps):
        cost, mv, dl = eng.two_opt_nl_once(path, cost)
        assert np.array_equal(mv, moves), (what, t)
        assert np.array_equal(dl, deltas), (what, t)
        assert np.array_equal(path, want_path), (what, t)
        assert cost == want_cost, (what, t)
    info = eng.info()
    assert (info["nl_sweeps"], info["nl_moves"]) == (1, 0)
    return sum(len(s[0]) >= 2 for s in sweeps)


def run_walks(mode, n, Ks, starts=("nn0", "random")):
    xy, kind = points_for(mode, n, 0)
    c = weight_matrix(xy, kind)
    src = source_of(mode, xy, kind, c)
    eng = engine_for(mode, xy, kind)
    multi = 0
    for K in Ks:
        eng.neighbours_build(K)
        nodes, _ = model_lists(K, **src)
        for s in starts:
            st = nn0(c) if s == "nn0" else random_tour(n, np.random.default_rng(n))
            # (the hundreds of sweeps from a random start of a large instance go through the matrix model in every mode: the
            # same sweeps as the coordinate model's, test_model_coordinate_variant_equals_the_matrix_model)
            walk = model_walk(st, nodes, c, **(src if n < 500 else dict(costs=c)))
            multi += check_walk(eng, st, c, walk, (mode, n, K, s))
    return eng, multi


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 6, 7, 8, 9, 12, 17, 63, 64, 65, 200])
@pytest.mark.parametrize("mode", MODES)
def test_gpu_move_by_move(mode, n):
    eng, multi = run_walks(mode, n, (5, 16))
    assert n < 63 or multi >= 1
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_move_by_move_at_the_workgroup_boundaries(mode):
    """one below, at and one above a multiple of the sweep's nodes per workgroup, read from the library"""
    eng, _ = run_walks(mode, 40, (5,))
    R = eng.info()["nl_nodes"]
    eng.close()
    assert R >= 1
    for n in (9 * R - 1, 9 * R, 9 * R + 1):
        run_walks(mode, n, (5,))[0].close()


@pytest.mark.gpu
@pytest.mark.parametrize("start", ["nn0", "random"])
@pytest.mark.parametrize("n", [1000, 1100])
@pytest.mark.parametrize("mode", MODES)
def test_gpu_move_by_move_large(mode, n, start):
    eng, multi = run_walks(mode, n, (8,), (start,))
    assert multi >= 1
    eng.close()


CAP_N, CAP_K = 40, 8


def cap_case(mode, seed, sweep):
    """40 random points and a random start; `sweep` is a module's model of one sweep -> (xy, kind, nodes, start, the model's
    record of the first sweep, the path behind it)"""
    xy, kind = points_for(mode, CAP_N, seed)
    src = source_of(mode, xy, kind, weight_matrix(xy, kind))
    nodes, _ = model_lists(CAP_K, **src)
    start = random_tour(CAP_N, np.random.default_rng(seed))
    want = start.copy()
    r = sweep(want, 123.0, nodes, **src)
    return xy, kind, nodes, start, r, want


def check_cap_refusal(mode, seed, ints, sweep, raw_once, once):
    """the caller's arrays hold one move less than the sweep accepts: 8, nothing applied and nothing written; they hold exactly
    as many: the model's sweep.  raw_once(eng, path, cost, cnt, mv, dl, cap) is the C entry point, once(eng, path, cost, cap)
    the engine's method.  The seed is chosen on the CPU so that the model accepts k >= 2 moves"""
    xy, kind, _, start, r, want = cap_case(mode, seed, sweep)
    k = len(r["moves"])
    assert k >= 2, (mode, seed, k)
    eng = engine_for(mode, xy, kind)
    eng.neighbours_build(CAP_K)
    path = start.copy()
    mv, dl = np.full(ints * CAP_N, -7, np.int32), np.full(CAP_N, -7.0)
    cost, cnt = C.c_double(123.0), C.c_int(-7)
    assert raw_once(eng, path, C.byref(cost), C.byref(cnt), mv, dl, k - 1) == 8
    assert np.array_equal(path, start) and cost.value == 123.0 and cnt.value == -7 and np.all(mv == -7) and np.all(dl == -7.0)
    got, mv, dl = once(eng, path, 123.0, k)
    assert np.array_equal(mv, r["moves"]) and np.array_equal(dl, r["deltas"])
    assert np.array_equal(path, want) and got == r["cost"]
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode,seed", [("u16", 1), ("mf_euc", 1)])
def test_gpu_cap_below_the_accepted_count(mode, seed):
    check_cap_refusal(mode, seed, 2, model_sweep,
                      lambda eng, *a: eng.L.tspgpu_two_opt_nl_once(eng.ctx, *a), lambda eng, p, c, cap: eng.two_opt_nl_once(p, c, cap=cap))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["u16", "i32", "f64", "mf_euc", "mf_ceil_int"])
def test_gpu_full_lists_equal_the_parallel_move_sweep(mode):
    """n <= 17, K = 16: every sweep equals tspgpu_two_opt_multi_once on the same tour"""
    for n in range(5, 18):
        xy, kind = points_for(mode, n, 3)
        c = weight_matrix(xy, kind)
        eng = engine_for(mode, xy, kind)
        eng.neighbours_build(16)
        assert eng.info()["nl_k"] == n - 1
        path = random_tour(n, np.random.default_rng(n))
        cost = tour_cost(path, costs=c)
        for sweep in range(10 * n):
            p1, p2 = path.copy(), path.copy()
            c1, m1, d1 = eng.two_opt_multi_once(p1, cost)
            c2, m2, d2 = eng.two_opt_nl_once(p2, cost)
            assert np.array_equal(m1, m2) and np.array_equal(d1, d2) and np.array_equal(p1, p2) and c1 == c2, (mode, n, sweep)
            path, cost = p2, c2
            if not len(m2):
                break
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["u16", "f64", "mf_euc"])
def test_gpu_rotation_and_direction(mode):
    """the same tour in a slot that 2-opt moves left with dir = -1 and a rotated ord gives the sweep of the freshly loaded
    successor array: pred(x) is read from pos, ord and dir.  Direction and rotation are the mirror's (slot_after_two_opt)."""
    n, K = 300, 8
    xy, kind = points_for(mode, n, 4)
    c = weight_matrix(xy, kind)
    eng = engine_for(mode, xy, kind)
    eng.neighbours_build(K)
    nodes, _ = model_lists(K, costs=c)
    seen_multi, dirs, rotated = False, set(), False
    for sweeps in (1, 2, 3, 5, 8):
        d, cell0, mirror = slot_after_two_opt(c, random_tour(n, np.random.default_rng(9)), sweeps)
        dirs.add(d)
        rotated |= cell0 != 0
        eng.tour_load(1, random_tour(n, np.random.default_rng(9)))
        eng.tour_two_opt(1, max_sweeps=sweeps)          # the shorter arc is reversed: the other arc toggles dir
        tour, cost, _ = eng.tour_store(1)
        assert np.array_equal(tour, mirror)
        fresh = tour.copy()
        fcost, fmv, fdl = eng.two_opt_nl_once(fresh, cost)          # slot 0 reloaded: dir = +1, ord from node 0
        sw, mv, rc = eng.tour_two_opt_nl(1, max_sweeps=1)
        got, gcost, gdelta = eng.tour_store(1)
        want = tour.copy()
        r = model_sweep(want, cost, nodes, costs=c)
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
    n, K = 400, 6
    xy, kind = points_for(mode, n, 2)
    c = weight_matrix(xy, kind)
    start = nn0(c)
    eng = engine_for(mode, xy, kind)
    if mode.startswith("mf"):
        eng.set_option(T._lib.OPT_OR_MATRIX_FREE, 1)
    eng.neighbours_build(K)
    nodes, _ = model_lists(K, costs=c)
    for sweeps in (1, 2, 3):
        want = start.copy()
        cost = tour_cost(want, costs=c)
        for _ in range(sweeps):
            cost = model_sweep(want, cost, nodes, costs=c)["cost"]
        eng.tour_load(0, start)
        sw, mv, rc = eng.tour_two_opt_nl(0, max_sweeps=sweeps)
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
    # the descent with its polish, and tspgpu_two_opt on the result: one sweep, the same path
    path = start.copy()
    r = eng.two_opt_nl(path)
    want = start.copy()
    m = model_descent(want, nodes, True, costs=c)
    assert r["rc"] == 0 and np.array_equal(path, want)
    assert (r["cost"], r["sweeps"], r["moves"], r["polish_sweeps"], r["polish_moves"]) == \
        (m["cost"], m["sweeps"], m["moves"], m["polish_sweeps"], m["polish_moves"])
    again = path.copy()
    cost2, sweeps2, rc2 = eng.two_opt(again)
    assert (cost2, sweeps2, rc2) == (r["cost"], 1, 0) and np.array_equal(again, path)
    eng.close()


@functools.lru_cache(maxsize=None)
def golden():
    return json.load(open(GOLDEN))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 8])
@pytest.mark.parametrize("name", ["pr1002", "fnl4461"])
def test_gpu_descent_equals_the_golden(name, K):
    g = golden()[name]
    want = next(d for d in g["descents"] if d["K"] == K)
    xy = O.read_tsplib(os.path.join(DATA, name + ".tsp"))[0]
    eng = engine_for("u16", xy, EUC_2D)
    assert eng.info()["elem"] == 3
    eng.neighbours_build(K)
    start, _ = eng.nn_tour(0)
    assert G.digest(start) == g["start_sha256"]
    path = start.copy()
    r = eng.two_opt_nl(path, polish=False)
    assert (r["rc"], r["cost"], r["sweeps"], r["moves"], r["polish_sweeps"]) == (0, want["cost"], want["sweeps"], want["moves"], 0)
    assert G.digest(path) == want["path_sha256"]
    info = eng.info()
    assert (info["nl_k"], info["nl_sweeps"], info["nl_moves"], info["nl_polish_sweeps"]) == (K, want["sweeps"], want["moves"], 0)
    path = start.copy()
    r = eng.two_opt_nl(path)
    assert (r["rc"], r["sweeps"], r["moves"]) == (0, want["sweeps"], want["moves"])
    assert (r["cost"], r["polish_sweeps"], r["polish_moves"]) == (want["polished_cost"], want["polish_sweeps"], want["polish_moves"])
    assert G.digest(path) == want["polished_path_sha256"]
    info = eng.info()
    assert (info["nl_sweeps"], info["nl_moves"], info["nl_polish_sweeps"]) == (want["sweeps"], want["moves"], want["polish_sweeps"])
    if name == "pr1002":        # the polished tour passes the oracle's full sweep
        c = O.cost_matrix(xy)
        d, _, _ = O.two_opt_once(c, path.copy(), r["cost"])
        assert not d < EPS and r["cost"] == O.tour_cost(c, path)
    eng.close()


@pytest.mark.gpu
def test_gpu_descent_and_polish_with_real_costs():
    """pr1002 as a matrix of doubles with non-integer costs (Euclidean weights scaled by per-edge factors): paths, sweeps and
    moves of both phases are the model's (every delta is bit-exact); the cost is the sum of the accepted deltas on the
    recomputed start cost, in an order that is not specified: within 1e-9 relative of the tour's cost from the matrix"""
    rng = np.random.default_rng(1002)
    xy = O.read_tsplib(os.path.join(DATA, "pr1002.tsp"))[0]
    n = len(xy)
    c = O.cost_matrix(xy) * (1.0 + symmetric_noise(n, rng))
    np.fill_diagonal(c, -1.0)
    start = nn0(c)
    eng = engine_for("f64", costs=c)
    eng.neighbours_build(8)
    nodes, w = eng.neighbours_get()
    want_nodes, want_w = model_lists(8, costs=c)
    assert np.array_equal(nodes, want_nodes) and np.array_equal(w, want_w)
    want = start.copy()
    m = model_descent(want, nodes, True, costs=c)
    path = start.copy()
    r = eng.two_opt_nl(path, polish=False)
    assert r["rc"] == 0 and np.array_equal(path, m["nl_path"]) and (r["sweeps"], r["moves"]) == (m["sweeps"], m["moves"])
    path = start.copy()
    r = eng.two_opt_nl(path)
    assert r["rc"] == 0 and np.array_equal(path, want)
    assert (r["sweeps"], r["moves"], r["polish_sweeps"], r["polish_moves"]) == (m["sweeps"], m["moves"], m["polish_sweeps"], m["polish_moves"])
    exact = O.tour_cost(c, path)
    assert abs(r["cost"] - exact) <= 1e-9 * exact
    d, _, _ = O.two_opt_once(c, path.copy(), exact)
    assert not d < EPS
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
    # no lists yet: 9, the tour untouched
    for call in (lambda: eng.two_opt_nl(path), lambda: eng.two_opt_nl_once(path, 0.0), lambda: eng.neighbours_get()):
        with pytest.raises(TspGpuError) as e:
            call()
        assert e.value.code == 9 and "tspgpu_neighbours_build" in str(e.value) and np.array_equal(path, keep)
    # K = 17 and K = -1: 3, and no lists appear
    for K in (17, -1):
        with pytest.raises(TspGpuError) as e:
            eng.neighbours_build(K)
        assert e.value.code == 3 and eng.info()["nl_k"] == 0
    # lists of another cost source: 9, with the reason
    eng.neighbours_build(8)
    assert eng.info()["nl_k"] == 8
    c2 = sym_int_matrix(n, rng)
    eng.set_costs(c2)
    assert eng.info()["nl_k"] == 0
    with pytest.raises(TspGpuError) as e:
        eng.two_opt_nl(path)
    assert e.value.code == 9 and "invalidated" in str(e.value) and np.array_equal(path, keep)
    eng.tour_load(0, path)
    with pytest.raises(TspGpuError) as e:
        eng.tour_two_opt_nl(0)
    assert e.value.code == 9 and "invalidated" in str(e.value)
    eng.neighbours_build(8)
    want = path.copy()
    m = model_descent(want, model_lists(8, costs=c2)[0], True, costs=c2)
    got = path.copy()
    r = eng.two_opt_nl(got)
    assert r["rc"] == 0 and np.array_equal(got, want) and r["cost"] == m["cost"]
    # an asymmetric matrix: 9 from the build and from the descents, and the context works afterwards
    asym = c.copy()
    asym[3][7] += 5.0
    eng.set_costs(asym)
    for call in (lambda: eng.neighbours_build(8), lambda: eng.two_opt_nl(path), lambda: eng.two_opt_nl_once(path, 0.0)):
        with pytest.raises(TspGpuError) as e:
            call()
        assert e.value.code == 9 and np.array_equal(path, keep)
    # n = 4: 3
    eng.set_points(O.random_points(4, 3), EUC_2D)
    eng.build_costs()
    eng.neighbours_build(16)
    assert eng.info()["nl_k"] == 3
    with pytest.raises(TspGpuError) as e:
        eng.two_opt_nl(np.roll(np.arange(4, dtype=np.int32), -1))
    assert e.value.code == 3
    # cap below the accepted count: 8, the path and the cost as they were
    n = 300
    xy = O.random_points(n, 8)
    cc = O.cost_matrix(xy)
    eng.set_points(xy)
    eng.build_costs()
    eng.neighbours_build(8)
    nodes, _ = model_lists(8, costs=cc)
    path = nn0(cc)
    keep = path.copy()
    k = len(model_sweep(path.copy(), 0.0, nodes, costs=cc)["moves"])
    assert k >= 2
    with pytest.raises(TspGpuError) as e:
        eng.two_opt_nl_once(path, 123.0, cap=k - 1)
    assert e.value.code == 8 and np.array_equal(path, keep)
    cost, mv, dl = eng.two_opt_nl_once(path, 123.0, cap=k)
    assert len(mv) == k and cost == 123.0 + dl.sum()
    # a deadline of 0: 4, a valid tour and its cost
    path = nn0(cc)
    keep = path.copy()
    r = eng.two_opt_nl(path, time_left_s=0.0)
    assert r["rc"] == 4 and np.array_equal(path, keep) and r["cost"] == O.tour_cost(cc, path)
    eng.tour_load(0, path)
    sw, mv, rc = eng.tour_two_opt_nl(0, time_left_s=0.0)
    assert rc == 4
    assert eng.time_nl_sweep(0, 2) > 0.0
    got, gcost, _ = eng.tour_store(0)
    assert np.array_equal(got, path) and gcost == r["cost"]        # timing applies nothing
    eng.close()


# ----------------------------------------------------------------------------------------------------------------- host
def run_tsp(*args, env_set=None, timeout=300):
    import subprocess
    env = dict(os.environ)
    for k in ("TSP_2OPT_MULTI", "TSP_2OPT_NEIGHBOURS", "TSP_2OPT_NEIGHBOURS_POLISH"):
        env.pop(k, None)
    env.update(env_set or {})
    os.makedirs(os.path.join(ROOT, "results"), exist_ok=True)
    r = subprocess.run([os.path.join(ROOT, "travellingsalesmanoptimization_amd", "host", "tsp"), *args], capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=ROOT)
    return r.returncode, r.stdout.strip(), r.stderr


@pytest.mark.gpu
def test_host_binary_runs_the_neighbour_list_descent():
    """`-alg VNS -k 1` is the binary's way to one ref_2opt call on a single tour: the best nearest-neighbour tour, one local
    search, the incumbent.  With TSP_2OPT_NEIGHBOURS=8 that local search is the golden's descent from that tour: polished by
    default, unpolished with TSP_2OPT_NEIGHBOURS_POLISH=0; it goes before TSP_2OPT_MULTI=1"""
    want = golden()["pr1002_best_nn"]["descents"][0]
    assert want["K"] == 8 and want["polished_cost"] < want["cost"]
    args = ("-f", os.path.join(DATA, "pr1002.tsp"), "-alg", "VNS", "-k", "1", "-seed", "1")
    rc, out, err = run_tsp(*args, "-q", env_set={"TSP_2OPT_NEIGHBOURS": "8"})
    assert rc == 0 and out == "Cost: %.2f" % want["polished_cost"], err
    rc, out, err = run_tsp(*args, "-q", env_set={"TSP_2OPT_NEIGHBOURS": "8", "TSP_2OPT_MULTI": "1"})
    assert rc == 0 and out == "Cost: %.2f" % want["polished_cost"], err
    rc, out, err = run_tsp(*args, "-q", env_set={"TSP_2OPT_NEIGHBOURS": "8", "TSP_2OPT_NEIGHBOURS_POLISH": "0"})
    assert rc == 0 and out == "Cost: %.2f" % want["cost"], err
    rc, out, err = run_tsp(*args, env_set={"TSP_2OPT_NEIGHBOURS": "8"})
    assert rc == 0 and "TSP_2OPT_NEIGHBOURS=8" in out + err and "differ from the reference" in out + err


@pytest.mark.gpu
def test_host_switch_values():
    args = ("-f", os.path.join(DATA, "kroA100.tsp"), "-alg", "VNS", "-k", "20", "-q")
    for bad in ("17", "-1", "eight", ""):
        rc, out, err = run_tsp(*args, env_set={"TSP_2OPT_NEIGHBOURS": bad})
        assert rc != 0 and "TSP_2OPT_NEIGHBOURS" in err and "1 to 16" in err, bad
    rc, out, err = run_tsp(*args, env_set={"TSP_2OPT_NEIGHBOURS": "8", "TSP_2OPT_NEIGHBOURS_POLISH": "2"})
    assert rc != 0 and "TSP_2OPT_NEIGHBOURS_POLISH" in err and "expected 0 or 1" in err
    plain = run_tsp(*args)
    assert plain[0] == 0 and run_tsp(*args, env_set={"TSP_2OPT_NEIGHBOURS": "0"}) == plain
