"""The batched neighbour-list descent (include/tspgpu.h "Batched neighbour-list descent"): the descent over the
lists on every tour of a batch per launch, the multi-start built on it, the multi-device form and the host switch.

The model is the CPU model of the single-tour descent (tests/or_opt_nl_model.c through make_golden_or_opt_nl.model_ls_descent,
the lists from make_golden_two_opt_nl.model_lists): a batch is nothing but its tours.  The existing tests pin that model to a
brute-force restatement.  Per slot the device must give the model's tour, cost, counters and last delta -- and, bit for bit,
what tspgpu_tour_local_search_nl leaves on the same tour.
"""
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
import make_golden_nl_batch as GB  # noqa: E402
import make_golden_two_opt_nl as G2  # noqa: E402
from make_golden_or_opt_nl import model_ls_descent, model_or_sweep  # noqa: E402
from make_golden_two_opt_nl import digest, model_lists, model_sweep  # noqa: E402
from test_two_opt_multi import (EUC_2D, MODES, engine_for, points_for, random_tour, sym_int_matrix, symmetric_noise,  # noqa: E402
                                tour_cost, weight_matrix)
from test_two_opt_nl import source_of, stripe_tour  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_nl_batch.json")
NEW_SYMBOLS = ["tspgpu_tours_local_search_nl", "tspgpu_multistart_local_search_nl", "tspgpu_multi_neighbours_build",
               "tspgpu_multi_multistart_local_search_nl"]
COUNTERS = ("two_opt_sweeps", "two_opt_moves", "or_sweeps", "or_moves", "rounds")


@functools.lru_cache(maxsize=None)
def golden():
    return json.load(open(GOLDEN))


@functools.lru_cache(maxsize=None)
def pr1002():
    """-> (xy, the model's lists for K = 8)"""
    xy = G2.tsplib_points("pr1002")
    return xy, model_lists(8, xy=xy)[0]


# ------------------------------------------------------------------------------------------------------------ CPU tests
def test_libraries_export_the_entry_points():
    from travellingsalesmanoptimization_amd import _lib
    import travellingsalesmanoptimization_amd as T
    host = C.CDLL(os.path.join(ROOT, "travellingsalesmanoptimization_amd", "host", "libtsphost.so"))
    for s in NEW_SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(_lib.load(), s), s
        assert hasattr(host, s), s
    assert hasattr(host, "h_greedy_local_search_nl")
    for m in ("tours_local_search_nl", "multistart_local_search_nl"):
        assert hasattr(T.Engine, m)
    for m in ("neighbours_build", "multistart_local_search_nl"):
        assert hasattr(T.MultiEngine, m)


def test_header_carries_the_section_and_the_info_indices():
    text = open(os.path.join(ROOT, "include", "tspgpu.h")).read()
    assert "Batched neighbour-list descent" in text
    at = text.index("Batched neighbour-list descent")
    assert at > text.index("Neighbour-list Or-opt")
    section = text[at:]
    for s in NEW_SYMBOLS[:2]:
        assert ("int %s(tspgpu_ctx *ctx" % s) in section, s
    for s in NEW_SYMBOLS[2:]:
        assert ("int %s(tspgpu_multi *m" % s) in section, s
    for idx in ("52", "53", "54", "55"):
        assert idx in section[section.index("tspgpu_info:"):section.index("int tspgpu_tours_local_search_nl")], idx
    from travellingsalesmanoptimization_amd import _lib
    assert (_lib.INFO_NL_BATCH_TOURS, _lib.INFO_NL_BATCH_LAUNCHES, _lib.INFO_NL_BATCH_MAX_LIVE, _lib.INFO_NL_BATCH_WGS) == (52, 53, 54, 55)


def test_no_context_means_14():
    from travellingsalesmanoptimization_amd import _lib
    L = _lib.load()
    null = C.c_void_p()
    best = np.full(8, -7, np.int32)
    cost, start = C.c_double(8.0), C.c_int(-7)
    a, b, c, d = C.c_long(), C.c_long(), C.c_long(), C.c_long()
    assert L.tspgpu_tours_local_search_nl(null, 0, 1, -1.0, None, None, None, None, None) == _lib.UNAVAILABLE
    assert L.tspgpu_multistart_local_search_nl(null, None, 8, -1.0, best, C.byref(cost), C.byref(start), C.byref(a), C.byref(b), C.byref(c),
                                               C.byref(d), None) == _lib.UNAVAILABLE
    assert L.tspgpu_multi_neighbours_build(null, 8) == _lib.UNAVAILABLE
    assert L.tspgpu_multi_multistart_local_search_nl(null, None, 8, -1.0, best, C.byref(cost), C.byref(start), C.byref(a), C.byref(b),
                                                     C.byref(c), C.byref(d)) == _lib.UNAVAILABLE
    assert np.all(best == -7) and cost.value == 8.0 and start.value == -7        # and no CPU fallback ran


def test_golden_is_reproducible_from_the_model():
    """starts 0 (DESIGN 4.15's row), 4 and 5 (a cost tie), 14 (the best of the first sixteen); the figures of start 15"""
    g = golden()
    xy, nodes = pr1002()
    assert (g["instance"], g["n"], g["K"], len(g["starts"])) == ("pr1002", 1002, 8, 32) and digest(nodes) == g["lists_sha256"]
    for s in (0, 4, 5, 14):
        got, _ = GB.start_entry(xy, nodes, s)
        assert got == g["starts"][s], s
    rows = {s: tuple(g["starts"][s][k] for k in ("rounds", "two_opt_sweeps", "or_sweeps", "cost")) for s in (0, 4, 5, 14, 15)}
    assert rows == {0: (3, 57, 36, 276720.0), 4: (2, 31, 11, 273069.0), 5: (2, 31, 11, 273069.0), 14: (3, 56, 33, 270144.0),
                    15: (2, 40, 14, 278497.0)}
    costs = [e["cost"] for e in g["starts"]]
    assert min(costs[:16]) == costs[14] and g["winner"]["start"] == costs.index(min(costs)) and g["winner"]["cost"] == min(costs)
    assert g["winner"]["path_sha256"] == g["starts"][g["winner"]["start"]]["path_sha256"]
    assert g["totals"] == {k: sum(e[k] for e in g["starts"]) for k in COUNTERS[:4]}


# ------------------------------------------------------------------------------------------------------------ GPU tests
def model_batch(tours, nodes, **src):
    """the model's descent of every tour -> [(path, record)]"""
    out = []
    for t in tours:
        p = t.copy()
        out.append((p, model_ls_descent(p, nodes, **src)))
    return out


def load_batch(eng, tours, slot0=0):
    for i in reversed(range(len(tours))):           # (the highest slot first: the slot array grows once)
        eng.tour_load(slot0 + i, tours[i])


def check_slot(eng, slot, want, what):
    path, rec = want
    got, cost, delta = eng.tour_store(slot)
    assert np.array_equal(got, path), what
    assert cost == rec["cost"], what
    assert delta == 0.0, what                       # the last sweep of a descent accepts nothing
    return got, cost, delta


def check_batch(eng, tours, want, what, slot0=0, single=True):
    """tours_local_search_nl on the loaded slots against the model, then against tour_local_search_nl on the same tours"""
    n = len(tours)
    load_batch(eng, tours, slot0)
    r = eng.tours_local_search_nl(slot0, n)
    assert r["rc"] == 0, what
    stored = []
    for i in range(n):
        assert {k: int(r[k][i]) for k in COUNTERS} == {k: want[i][1][k] for k in COUNTERS}, (what, i)
        stored.append(check_slot(eng, slot0 + i, want[i], (what, i)))
    info = eng.info()
    assert info["nl_batch_tours"] == n and info["nl_batch_max_live"] == n and info["nl_batch_wgs"] == (eng.n + 3) // 4
    longest = max(w[1]["two_opt_sweeps"] + w[1]["or_sweeps"] for w in want)
    assert longest <= info["nl_batch_launches"] <= longest + 3, what       # four sweeps between two looks at the control blocks
    if not single:
        return
    load_batch(eng, tours, slot0)
    for i in range(n):
        r1 = eng.tour_local_search_nl(slot0 + i)
        assert r1["rc"] == 0 and {k: r1[k] for k in COUNTERS} == {k: int(r[k][i]) for k in COUNTERS}, (what, i)
        got, cost, delta = eng.tour_store(slot0 + i)
        assert np.array_equal(got, stored[i][0]) and (cost, delta) == stored[i][1:], (what, i)       # bit-equal, doubles too


def mixed_batch(n, nodes, **src):
    """13 random tours and one that is the result of a descent already; the tours must leave the live list at different times"""
    rng = np.random.default_rng(7)
    tours = [random_tour(n, rng) for _ in range(13)]
    done = tours[0].copy()
    model_ls_descent(done, nodes, **src)
    tours.append(done)
    want = model_batch(tours, nodes, **src)
    assert len({w[1]["rounds"] for w in want}) >= 2 and len({w[1]["two_opt_sweeps"] for w in want}) >= 5
    assert tuple(want[13][1][k] for k in COUNTERS) == (1, 0, 1, 0, 1) and np.array_equal(want[13][0], done)
    return tours, want


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_every_slot_equals_the_model(mode):
    n, K = 40, 8
    xy, kind = points_for(mode, n, 0)
    c = weight_matrix(xy, kind)
    src = source_of(mode, xy, kind, c)
    nodes, _ = model_lists(K, **src)
    tours, want = mixed_batch(n, nodes, **src)
    eng = engine_for(mode, xy, kind)
    eng.neighbours_build(K)
    check_batch(eng, tours, want, mode)
    eng.close()


@pytest.mark.gpu
def test_gpu_every_slot_equals_the_model_with_real_costs():
    """f64 cells that hold non-integer costs: tours, counters, last delta and cost are the model's, the cost to the bit.
    include/tspgpu.h leaves the order in which a sweep's accepted deltas are summed open (rule 6 of "Neighbour-list Or-opt"):
    the model adds them one after the other, the device in a tree of fixed shape.  On this batch the two agree in every sweep
    of every tour (measured on the device: all 14 differences are 0), and both are deterministic; against
    tspgpu_tour_local_search_nl the cost is bit-equal by construction."""
    n, K = 40, 8
    rng = np.random.default_rng(64)
    c = O.cost_matrix(O.random_points(n, 64 + n)) * (1.0 + symmetric_noise(n, rng))
    np.fill_diagonal(c, -1.0)
    nodes, _ = model_lists(K, costs=c)
    tours, want = mixed_batch(n, nodes, costs=c)
    eng = engine_for("f64", costs=c)
    eng.neighbours_build(K)
    check_batch(eng, tours, want, "real")
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 9, 17, 18, 33, 257, 300, 1025])
@pytest.mark.parametrize("mode", ["u16", "mf_euc"])
def test_gpu_geometry_boundaries(mode, n):
    """a batch of five tours (the stripe tour and four random ones) at the sizes where a kernel's geometry changes: the partial
    last workgroup of the candidate sweep in both phases (8 and 4 nodes per workgroup: 8 | 9, 17 | 18, 33), a second selection
    workgroup per tour (257; no stripe or random tour of 257 nodes has more than 256 candidates in a sweep -- the model counts
    at most 237 -- so the second tile with candidates in it is n = 300's, asserted below), two nodes per thread of the
    compaction (1025)"""
    K = 8
    xy, kind = points_for(mode, n, 0)
    c = weight_matrix(xy, kind)
    src = source_of(mode, xy, kind, c)
    nodes, _ = model_lists(K, **src)
    rng = np.random.default_rng(n)
    tours = [stripe_tour(xy)] + [random_tour(n, rng) for _ in range(4)]
    if n == 300:
        first = [len(model_sweep(t.copy(), tour_cost(t, costs=c), nodes, apply=False, **src)["cand"]) for t in tours]
        assert max(first) > 256, first
    want = model_batch(tours, nodes, **src)
    eng = engine_for(mode, xy, kind)
    eng.neighbours_build(K)
    check_batch(eng, tours, want, (mode, n), single=n <= 33)
    eng.close()


def planted_case(n, spec):
    """a tour that a long-arc 2-opt flip leaves (dir = -1, a rotated ord), and the matrix that plants the moves of `spec` on it
    (test_or_opt_nl.apply_cases, one case of it) -> (tour0, flip (a, b, delta), the tour after the flip, the matrix)"""
    import test_or_opt_geometry as OG
    from test_or_opt_nl import planted_matrix, planted_moves
    tour0 = random_tour(n, np.random.default_rng(40 + n))
    fl = OG.long_arc_flip(tour0)[0]
    lay, path = OG.Layout(tour0), tour0.copy()
    O.apply_move(path, None, fl[0], fl[1])
    lay.flip(*fl)
    assert lay.dir == -1 and int(np.nonzero(lay.ord == 0)[0][0]) != 0
    moves = planted_moves(n, spec)
    c = planted_matrix(path, OG.forward_order(path), moves)
    return tour0, (fl[0], fl[1], O.tour_cost(c, path) - O.tour_cost(c, tour0)), path, c


@pytest.mark.gpu
@pytest.mark.parametrize("long_block", ["behind", "front"])
def test_gpu_apply_in_a_batch(long_block):
    """n = 1100: planted moves, one of them with a shifted block of three chunks of the apply workgroup's 256 cells and more,
    inserted behind (one case) and in front (the other), on a freshly loaded slot and on a slot that a 2-opt move left with
    dir = -1 and a rotated ord, batched with three ordinary tours"""
    from test_or_opt_nl import APPLY_CHUNK, apply_specs
    n, K = 1100, 4
    spec = next(s for s in apply_specs(n) if s[0] == (long_block, 3 * APPLY_CHUNK + 5, 2 if long_block == "behind" else 0))
    assert {w for w, _, _ in spec} == {"behind", "front"}
    tour0, flip, path, c = planted_case(n, spec)
    assert flip[2] < -1.0e-7
    nodes, _ = model_lists(K, costs=c)
    # the model's 2-opt phase takes two short moves next to the small planted ones; its first Or-opt sweep then accepts several
    # planted moves at once, the one with the long block among them, in the direction asked for
    import test_or_opt_geometry as OG
    after = path.copy()
    G2.model_descent(after, nodes, False, costs=c)
    P = np.empty(n, np.int64)
    P[OG.forward_order(after)] = np.arange(n)
    first = model_or_sweep(after.copy(), 0.0, nodes, costs=c)
    blocks = [("behind", int(P[q] - (P[s] + L) + 1)) if P[q] > P[s] else ("front", int(P[s] - 1 - P[q])) for s, L, q, _ in first["moves"]]
    assert len(blocks) >= 2 and (long_block, 3 * APPLY_CHUNK + 5) in blocks and np.all(first["deltas"] == -297.0), blocks
    rng = np.random.default_rng(3)
    tours = [path, path] + [random_tour(n, rng) for _ in range(3)]
    want = model_batch(tours, nodes, costs=c)
    assert want[0][1]["or_moves"] >= 2
    eng = engine_for("u16", costs=c)
    eng.neighbours_build(K)
    load_batch(eng, tours)
    eng.tour_load(1, tour0)
    eng.tour_apply_move(1, *flip)
    got, cost, _ = eng.tour_store(1)
    assert np.array_equal(got, path) and cost == O.tour_cost(c, path)
    r = eng.tours_local_search_nl(0, 5)
    assert r["rc"] == 0
    for i in range(5):
        assert {k: int(r[k][i]) for k in COUNTERS} == {k: want[i][1][k] for k in COUNTERS}, i
        check_slot(eng, i, want[i], i)
    eng.close()


@pytest.mark.gpu
def test_gpu_more_rows_than_one_grid():
    """65 537 + 3 slots of n = 8: the live list spans two runs of grid rows; 16 distinct start tours repeated cyclically"""
    import travellingsalesmanoptimization_amd as T
    n, K, slots = 8, 5, 65537 + 3
    xy, kind = points_for("u16", n, 0)
    c = weight_matrix(xy, kind)
    nodes, _ = model_lists(K, costs=c)
    rng = np.random.default_rng(8)
    tours = [random_tour(n, rng) for _ in range(16)]
    assert len({digest(t) for t in tours}) == 16
    want = model_batch(tours, nodes, costs=c)
    eng = engine_for("u16", xy, kind)
    eng.set_option(T.OPT_MAX_TOURS, slots)
    eng.neighbours_build(K)
    eng.tour_load(slots - 1, tours[(slots - 1) % 16])
    for k in range(16):
        eng.tour_load(k, tours[k])
    for s in range(16, slots - 1):
        eng.tour_copy(s, s % 16)
    r = eng.tours_local_search_nl(0, slots)
    assert r["rc"] == 0 and eng.info()["nl_batch_max_live"] == slots
    for k in COUNTERS:
        assert np.array_equal(r[k], np.resize(np.array([w[1][k] for w in want]), slots)), k
    for s in range(slots):
        path, cost, _ = eng.tour_store(s)
        assert cost == want[s % 16][1]["cost"] and np.array_equal(path, want[s % 16][0]), s
    eng.close()


@pytest.mark.gpu
def test_gpu_slot_range_inside_the_slots():
    n, K = 40, 8
    xy, kind = points_for("u16", n, 1)
    c = weight_matrix(xy, kind)
    nodes, _ = model_lists(K, costs=c)
    rng = np.random.default_rng(5)
    tours = [random_tour(n, rng) for _ in range(10)]
    eng = engine_for("u16", xy, kind)
    eng.neighbours_build(K)
    load_batch(eng, tours)
    before = [eng.tour_store(s) for s in range(10)]
    want = model_batch(tours[3:7], nodes, costs=c)
    r = eng.tours_local_search_nl(3, 4)
    assert r["rc"] == 0
    for i in range(4):
        assert {k: int(r[k][i]) for k in COUNTERS} == {k: want[i][1][k] for k in COUNTERS}, i
        check_slot(eng, 3 + i, want[i], i)
    for s in (0, 1, 2, 7, 8, 9):
        path, cost, delta = eng.tour_store(s)
        assert np.array_equal(path, before[s][0]) and (cost, delta) == before[s][1:], s
        # ... and still a slot the other calls can use: its own descent is the model's
        p = tours[s].copy()
        m = model_ls_descent(p, nodes, costs=c)
        r1 = eng.tour_local_search_nl(s)
        assert {k: r1[k] for k in COUNTERS} == {k: m[k] for k in COUNTERS} and np.array_equal(eng.tour_store(s)[0], p), s
    eng.close()


def check_multistart(r, starts, g, path=True):
    rows = [g["starts"][s] for s in starts]
    costs = [e["cost"] for e in rows]
    win = costs.index(min(costs))
    assert r["rc"] == 0 and np.array_equal(r["costs"], costs)
    assert (r["start"], r["cost"]) == (starts[win], costs[win])
    assert {k: r[k] for k in COUNTERS[:4]} == {k: sum(e[k] for e in rows) for k in COUNTERS[:4]}
    if path:
        assert digest(r["path"]) == rows[win]["path_sha256"]


@pytest.mark.gpu
def test_gpu_multistart_pr1002():
    import travellingsalesmanoptimization_amd as T
    g = golden()
    xy = O.read_tsplib(os.path.join(DATA, "pr1002.tsp"))[0]
    eng = engine_for("u16", xy, EUC_2D)
    eng.neighbours_build(8)
    assert digest(eng.neighbours_get()[0]) == g["lists_sha256"]
    every = list(range(32))
    # (a) one chunk, and seven chunks with the last one partial
    eng.set_option(T.OPT_MAX_TOURS, 1024)
    r = eng.multistart_local_search_nl(every)
    check_multistart(r, every, g)
    assert (r["start"], r["cost"], digest(r["path"])) == (g["winner"]["start"], g["winner"]["cost"], g["winner"]["path_sha256"])
    assert {k: r[k] for k in COUNTERS[:4]} == g["totals"]
    info = eng.info()
    assert (info["nl_batch_tours"], info["nl_batch_max_live"], info["nl_batch_wgs"]) == (32, 32, 251)
    eng.set_option(T.OPT_MAX_TOURS, 5)
    r5 = eng.multistart_local_search_nl(every)
    check_multistart(r5, every, g)
    assert np.array_equal(r5["path"], r["path"]) and eng.info()["nl_batch_tours"] == 2
    eng.set_option(T.OPT_MAX_TOURS, 1024)
    # (b) the cost tie of the starts 4 and 5 goes to the earlier entry of the list
    assert g["starts"][4]["cost"] == g["starts"][5]["cost"]
    for starts in ([5, 4], [4, 5]):
        r = eng.multistart_local_search_nl(starts)
        check_multistart(r, starts, g)
        assert r["start"] == starts[0]
    # (c) a repeated entry, descending order
    starts = [15, 14, 14, 9, 5, 0]
    check_multistart(eng.multistart_local_search_nl(starts), starts, g)
    # a sweep cap is refused
    eng.set_option(T.OPT_SWEEP_CAP, 3)
    with pytest.raises(T.TspGpuError) as e:
        eng.multistart_local_search_nl([0, 1])
    assert e.value.code == 3 and "TSPGPU_OPT_SWEEP_CAP" in str(e.value)
    eng.close()
    # (d) matrix-free
    mf = engine_for("mf_euc", xy, EUC_2D)
    mf.neighbours_build(8)
    check_multistart(mf.multistart_local_search_nl(list(range(8))), list(range(8)), g)
    mf.close()


@pytest.mark.gpu
def test_gpu_two_contexts_behind_one_handle():
    import travellingsalesmanoptimization_amd as T
    g = golden()
    xy = O.read_tsplib(os.path.join(DATA, "pr1002.tsp"))[0]
    eng = engine_for("u16", xy, EUC_2D)
    eng.neighbours_build(8)
    one = eng.multistart_local_search_nl(list(range(16)))
    eng.close()
    check_multistart(one, list(range(16)), g)
    assert one["start"] == 14
    m = T.MultiEngine([0, 0])
    m.set_points(xy)
    m.build_costs()
    with pytest.raises(T.TspGpuError) as e:
        m.multistart_local_search_nl(list(range(16)))
    assert e.value.code == 9 and "no neighbour lists" in str(e.value)
    m.neighbours_build(8)
    two = m.multistart_local_search_nl(list(range(16)))
    m.close()
    for k in ("rc", "cost", "start") + COUNTERS[:4]:
        assert two[k] == one[k], k
    assert np.array_equal(two["path"], one["path"])


def is_tour(path):
    n, v = len(path), 0
    for _ in range(n):
        v = int(path[v])
        if not 0 <= v < n:
            return False
    return v == 0 and len(set(int(x) for x in path)) == n


@pytest.mark.gpu
@pytest.mark.parametrize("left", [0.0, 1.0e-6])
def test_gpu_deadline(left):
    g = golden()
    xy = O.read_tsplib(os.path.join(DATA, "pr1002.tsp"))[0]
    c = O.cost_matrix(xy)
    eng = engine_for("u16", xy, EUC_2D)
    eng.neighbours_build(8)
    for s in reversed(range(8)):
        eng.tour_nn(s, s)
    r = eng.tours_local_search_nl(0, 8, time_left_s=left)
    assert r["rc"] == 4
    for s in range(8):
        path, cost, _ = eng.tour_store(s)
        assert is_tour(path) and cost == O.tour_cost(c, path), s
        for k in COUNTERS:
            assert 0 <= int(r[k][s]) <= g["starts"][s][k], (s, k)
    # the descent goes on from what the deadline left, to a tour both list neighbourhoods cannot improve
    r = eng.tours_local_search_nl(0, 8)
    assert r["rc"] == 0
    xy2, nodes = pr1002()
    for s in range(8):
        path, cost, delta = eng.tour_store(s)
        assert is_tour(path) and cost == O.tour_cost(c, path) and delta == 0.0, s
        assert tuple(model_ls_descent(path.copy(), nodes, xy=xy2)[k] for k in COUNTERS) == (1, 0, 1, 0, 1), s
    ms = eng.multistart_local_search_nl(list(range(8)), time_left_s=0.0)
    assert ms["rc"] == 4
    eng.close()


@pytest.mark.gpu
def test_gpu_refusals():
    from travellingsalesmanoptimization_amd import TspGpuError
    import travellingsalesmanoptimization_amd as T
    rng = np.random.default_rng(1)
    n = 40
    c = sym_int_matrix(n, rng)
    tours = [random_tour(n, rng) for _ in range(4)]
    eng = engine_for("u16", costs=c)
    load_batch(eng, tours)
    keep = [eng.tour_store(s) for s in range(4)]
    calls = (lambda: eng.tours_local_search_nl(0, 4), lambda: eng.multistart_local_search_nl([0, 1]))

    def untouched():
        return all(np.array_equal(eng.tour_store(s)[0], keep[s][0]) and eng.tour_store(s)[1:] == keep[s][1:] for s in range(4))

    def refused(code, word, these=calls):
        for call in these:
            with pytest.raises(TspGpuError) as e:
                call()
            assert e.value.code == code and word in str(e.value), str(e.value)
    # no lists yet: 9 with the text of "Neighbour-list 2-opt"
    refused(9, "no neighbour lists: call tspgpu_neighbours_build first")
    assert untouched()
    eng.neighbours_build(8)
    # a bad slot range: 3
    tcap = 16
    for slot0, count in ((-1, 2), (0, 0), (0, -3), (2, tcap), (tcap, 1), (1, 2 ** 31 - 1)):
        with pytest.raises(TspGpuError) as e:
            eng.tours_local_search_nl(slot0, count)
        assert e.value.code == 3, (slot0, count)
    # a slot of the range without a tour: 9, nothing run
    with pytest.raises(TspGpuError) as e:
        eng.tours_local_search_nl(2, 4)
    assert e.value.code == 9 and "holds no tour" in str(e.value) and untouched()
    # lists of another cost source: 9, with the reason
    eng.set_costs(sym_int_matrix(n, rng))
    load_batch(eng, tours)
    refused(9, "invalidated by a new cost source")
    # ... the same after tspgpu_build_costs
    xy = O.random_points(n, 3)
    eng.set_points(xy, EUC_2D)
    eng.build_costs()
    eng.neighbours_build(8)
    eng.build_costs()
    load_batch(eng, tours)
    refused(9, "invalidated by a new cost source")
    # an asymmetric matrix: 9
    asym = c.copy()
    asym[3][7] += 5.0
    eng.set_costs(asym)
    load_batch(eng, tours)
    refused(9, "symmetric")
    # no costs: 9
    fresh = T.Engine(0)
    fresh.n = 8
    for call in (lambda: fresh.tours_local_search_nl(0, 1), lambda: fresh.multistart_local_search_nl([0])):
        with pytest.raises(TspGpuError) as e:
            call()
        assert e.value.code == 9
    fresh.close()
    # n = 7: 3, with lists in place
    eng.set_points(O.random_points(7, 3), EUC_2D)
    eng.build_costs()
    eng.neighbours_build(16)
    eng.tour_load(0, np.roll(np.arange(7, dtype=np.int32), -1))
    refused(3, "8 nodes", (lambda: eng.tours_local_search_nl(0, 1), lambda: eng.multistart_local_search_nl([0])))
    eng.close()


# ----------------------------------------------------------------------------------------------------------------- host
def run_tsp(*args, env_set=None, timeout=300):
    import subprocess
    env = dict(os.environ)
    for k in ("TSP_2OPT_MULTI", "TSP_2OPT_NEIGHBOURS", "TSP_2OPT_NEIGHBOURS_POLISH", "TSP_OR_OPT", "TSP_OR_OPT_NEIGHBOURS",
              "TSP_OR_OPT_MATRIX_FREE", "TSP_OR_OPT_EVERY_START", "TSP_EVERY_START_NEIGHBOURS", "TSP_GPU_DEVICES"):
        env.pop(k, None)
    env.update(env_set or {})
    os.makedirs(os.path.join(ROOT, "results"), exist_ok=True)
    r = subprocess.run([os.path.join(ROOT, "travellingsalesmanoptimization_amd", "host", "tsp"), *args], capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=ROOT)
    return r.returncode, r.stdout.strip(), r.stderr


@pytest.mark.gpu
def test_host_binary_runs_the_multistart_over_the_lists():
    """the binary has no switch that restricts the starts, so: berlin52 over all 52 starts against the model"""
    xy = G2.tsplib_points("berlin52")
    nodes, _ = model_lists(8, xy=xy)
    costs = [GB.start_entry(xy, nodes, s)[0]["cost"] for s in range(len(xy))]
    args = ("-f", os.path.join(DATA, "berlin52.tsp"), "-alg", "2OPT_GREEDY")
    rc, out, err = run_tsp(*args, "-q", env_set={"TSP_EVERY_START_NEIGHBOURS": "8"})
    assert rc == 0 and out == "Cost: %.2f" % min(costs), err
    # the same lists for the other switches; on two contexts of one device
    rc, out, err = run_tsp(*args, "-q", env_set={"TSP_EVERY_START_NEIGHBOURS": "8", "TSP_2OPT_NEIGHBOURS": "8", "TSP_GPU_DEVICES": "0,0"})
    assert rc == 0 and out == "Cost: %.2f" % min(costs), err
    rc, out, err = run_tsp(*args, env_set={"TSP_EVERY_START_NEIGHBOURS": "8"})
    assert rc == 0 and "results differ from the reference's trajectory" in out + err
    # off: what the binary does today
    plain = run_tsp(*args, "-q")
    assert plain[0] == 0 and run_tsp(*args, "-q", env_set={"TSP_EVERY_START_NEIGHBOURS": "0"}) == plain


@pytest.mark.gpu
def test_host_switch_values():
    args = ("-f", os.path.join(DATA, "berlin52.tsp"), "-alg", "2OPT_GREEDY", "-q")
    for bad in ("17", "-1", "eight", ""):
        rc, out, err = run_tsp(*args, env_set={"TSP_EVERY_START_NEIGHBOURS": bad})
        assert rc != 0 and "TSP_EVERY_START_NEIGHBOURS" in err and "1 to 16" in err, bad
    rc, out, err = run_tsp(*args, env_set={"TSP_EVERY_START_NEIGHBOURS": "8", "TSP_2OPT_NEIGHBOURS": "5"})
    assert rc != 0 and "TSP_EVERY_START_NEIGHBOURS=8" in err and "TSP_2OPT_NEIGHBOURS=5" in err
    rc, out, err = run_tsp(*args, env_set={"TSP_EVERY_START_NEIGHBOURS": "8", "TSP_OR_OPT": "1", "TSP_OR_OPT_NEIGHBOURS": "5"})
    assert rc != 0 and "TSP_EVERY_START_NEIGHBOURS=8" in err and "TSP_OR_OPT_NEIGHBOURS=5" in err
    rc, out, err = run_tsp(*args, env_set={"TSP_EVERY_START_NEIGHBOURS": "8", "TSP_OR_OPT_EVERY_START": "1"})
    assert rc != 0 and "TSP_EVERY_START_NEIGHBOURS=8" in err and "TSP_OR_OPT_EVERY_START=1" in err
