"""One context for many instances, slot-array growths and move families (DESIGN 4.17 "Context lifetime").

Every other GPU test builds a fresh Engine for one cost source; the host layer keeps ONE context for a whole run, and
include/tspgpu.h promises one per caller thread for the life of the thread.  A context carries state that has to be dropped,
rebuilt or resized at the right moment: the launch plan and its captured graphs, cell type and matrix / matrix-free mode, the
nearest-neighbour grid, the neighbour lists, the candidate buffers (by n, and by n x count), the gathered points, the tabu
arrays, slot validity, the per-capacity scratch and the "what the last call did" words of tspgpu_info.

1. a ladder of instances through one context (sizes up and down, cell types, modes, weight kinds, caller matrices), probed
   after every step exactly as a fresh context is;
2. the slot array growing under live tours in every state;
3. every move family in turn on one slot;
4. the "last call" words of tspgpu_info after calls of different kinds;
5. one multi-device handle through three instances, and a cost tie across its contexts.

Every expectation comes from the CPU models the family tests pin (the oracle, tests/two_opt_multi_model.c,
tests/two_opt_nl_model.c, tests/or_opt_nl_model.c, tests/or_opt_model.c); a fresh Engine in the same process is a second
witness for bit-equality and for the geometry words, never the only one -- with one exception, said where it is made (the
geometry word or_batch_r, which no model knows)."""
import functools
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
import make_golden_two_opt_nl as G2  # noqa: E402
import test_two_opt_multi as M2  # noqa: E402  (model_sweep, model_descent: the parallel-move C model)
from make_golden_nl_batch import start_entry  # noqa: E402
from make_golden_or_opt_nl import model_ls_descent, model_or_sweep  # noqa: E402
from make_golden_two_opt_nl import digest, model_lists  # noqa: E402
from test_or_opt import descent_model, or_opt_phase  # noqa: E402
from test_two_opt_multi import (ATT, CEIL_2D, EPS, EUC_2D, MODES, engine_for, points_for, random_tour, sym_int_matrix,  # noqa: E402
                                symmetric_noise, weight_matrix)
from test_two_opt_nl import source_of, stripe_tour  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")
COUNTERS = ("two_opt_sweeps", "two_opt_moves", "or_sweeps", "or_moves", "rounds")
F64, I32, U16 = 1, 2, 3

# tspgpu_info words that describe the instance and its plans: a long-lived context must show what a fresh one shows
GEOMETRY_KEYS = ("n", "ld", "elem", "kernel", "wgs_per_tour", "lds_bytes", "block", "symmetric", "depth", "matrix_free", "fused", "nn_grid",
                 "nn_grid_max_cell", "pipe2", "persist_wgs", "persist_edges", "persist_lds", "persist_window_cells", "otf_kernel", "ceil_int",
                 "or_single_r", "or_block", "or_nch", "multi_r", "multi_block", "multi_nch", "nl_k", "nl_batch_wgs")
# ... and the words about the last call of a family (persist, persist_handed, persist_window, persist_sweeps are left out:
# they say whether the grid came up co-resident on a chip that others share)
FAMILY_KEYS = {"two_opt": ("stream_persist",), "multi": ("multi_sweeps", "multi_moves", "multi_max_moves"),
               "nl": ("nl_sweeps", "nl_moves", "nl_polish_sweeps"), "or_nl": ("or_nl_sweeps", "or_nl_moves", "or_nl_max_moves", "or_nl_rounds"),
               "nl_batch": ("nl_batch_tours", "nl_batch_launches", "nl_batch_max_live"), "or": ("or_otf", "or_otf_R"), "or_batch": ("or_batch_r",)}


def T():
    import travellingsalesmanoptimization_amd
    return travellingsalesmanoptimization_amd


# ----------------------------------------------------------------------------------------------------------- small glue
def nl_entry(c, nodes, start, **src):
    """make_golden_nl_batch.start_entry for any cost source: the record of the descent over the lists from the oracle's
    nearest-neighbour tour of `start` -> (record, path)"""
    path = O.nn_tour(c, start)[0]
    r = model_ls_descent(path, nodes, **src)
    return dict({k: r[k] for k in COUNTERS}, start=start, cost=r["cost"], path_sha256=digest(path)), path


def model_or_nl_phase(path, cost, nodes, max_sweeps=-1, **src):
    """rule 7 of "Neighbour-list Or-opt" from the model's sweep; path in place -> (cost, sweeps, moves, most moves of a sweep, last
    sweep's smallest delta or 0)"""
    sweeps = moves = most = 0
    while max_sweeps < 0 or sweeps < max_sweeps:
        r = model_or_sweep(path, cost, nodes, **src)
        cost, k = r["cost"], len(r["moves"])
        sweeps, moves, most = sweeps + 1, moves + k, max(most, k)
        if not k:
            break
    return cost, sweeps, moves, most


def multistart_two_opt(c, starts, threads=16):
    """oracle.multistart_nn_2opt from oracle.nn_tour and oracle.two_opt, the starts spread over threads (the oracle's loop is
    sequential: 48 starts of 1100 nodes take it 19 s) -> (best path, cost, start, total sweeps), [(path, cost) of every start].
    The winner is the first strictly lowest cost, as h_greedy_2opt keeps it (src/algorithms/heuristics.c:74-116)."""
    from concurrent.futures import ThreadPoolExecutor

    def one(s):
        p = O.nn_tour(c, s)[0]
        sweeps, cost = O.two_opt(c, p)
        return p, cost, sweeps
    with ThreadPoolExecutor(threads) as pool:
        done = list(pool.map(one, starts))
    costs = [d[1] for d in done]
    win = costs.index(min(costs))
    return (done[win][0], costs[win], starts[win], sum(d[2] for d in done)), [d[:2] for d in done]


def refused(call, code, *words, without=()):
    with pytest.raises(T().TspGpuError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)
    for w in without:
        assert w not in str(e.value), str(e.value)


def cost_is(cost, c, path, integer, what):
    """integer-valued sources: the tour's cost exactly.  Real-valued ones: a descent adds at most a few thousand doubles no
    larger than the cost, each rounded to 2^-53 relative -- below 1e-12 relative in all --, and one wrong edge moves the cost
    by about 1e-3 relative: 1e-9 separates the two"""
    exact = O.tour_cost(c, np.ascontiguousarray(path, np.int32))
    if integer:
        assert cost == exact, (what, cost, exact)
    else:
        assert abs(cost - exact) <= 1e-9 * cost, (what, cost, exact)


# ================================================================================================ 1. the ladder
LADDER_SIZES = (200, 40, 1025, 8, 300, 64, 33, 257)     # the geometry boundaries of the family tests, up and down
LADDER_KS = (1, 5, 8, 16)
S_MULTI, S_NL, S_ORNL, S_LSNL, S_2OPT, S_OR, S_LS, S_BLS = 16, 17, 18, 19, 20, 21, 22, 23      # the single-tour slots of the probe


@functools.lru_cache(maxsize=None)
def ladder():
    """the stages: dicts of
         how     "points" (tspgpu_set_points + tspgpu_build_costs), "rebuild" (tspgpu_build_costs again), "costs" (tspgpu_set_costs)
         elem, mf, or_mf   TSPGPU_OPT_ELEM, matrix-free mode, TSPGPU_OPT_OR_MATRIX_FREE -- set before the stage's set-up
         xy, kind          the points the context holds at this stage (None: none, after a caller matrix of another n)
         c                 the weights the stage's cost source gives, as a matrix of doubles
         K, batch          the list length and (slot0, count) of the batched call"""
    out = []

    def add(name, how, elem, mf, or_mf, xy, kind, c, batch=(0, 3), integer=True, K=None):
        n = len(c)
        out.append(dict(name=name, how=how, elem=elem, mf=mf, or_mf=or_mf, xy=xy, kind=kind, c=np.ascontiguousarray(c), n=n,
                        K=LADDER_KS[len(out) % 4] if K is None else K, batch=batch, integer=integer, index=len(out)))

    # points, n up and down (uint16 cells)
    for i, n in enumerate(LADDER_SIZES):
        xy, kind = points_for("u16", n, 11)
        add("n%d" % n, "points", U16, 0, 0, xy, kind, weight_matrix(xy, kind), batch=(0, 5) if i == 3 else (0, 3))
    # the same points: cell types (the batched call grows its buffers, uses them with a smaller count, ...), then modes
    xy, kind = out[-1]["xy"], EUC_2D
    c = out[-1]["c"]
    add("f64", "rebuild", F64, 0, 0, xy, kind, c, batch=(0, 10))
    add("i32", "rebuild", I32, 0, 0, xy, kind, c, batch=(7, 2))
    add("matrix_free", "rebuild", I32, 1, 1, xy, kind, c)
    add("matrix_again", "rebuild", U16, 0, 0, xy, kind, c)
    # weight kinds: ATT, CEIL_2D over real coordinates, CEIL_2D over integer ones (ceil_int and its integer points come and go)
    xy, kind = points_for("mf_att", 100, 11)
    add("att", "points", 0, 1, 1, xy, kind, weight_matrix(xy, kind), batch=(0, 5))      # (... and are rebuilt for a new n)
    xy, kind = points_for("mf_ceil", 90, 11)
    add("ceil_real", "points", U16, 0, 0, xy, kind, weight_matrix(xy, kind))
    xy, kind = points_for("mf_ceil_int", 130, 11)
    cc = weight_matrix(xy, kind)
    add("ceil_int", "points", 0, 1, 0, xy, kind, cc)
    # caller matrices of the same n: integers in uint16 cells, real values in doubles; then the points again
    rng = np.random.default_rng(130)
    add("caller_u16", "costs", U16, 0, 0, xy, kind, sym_int_matrix(130, rng))
    real = O.cost_matrix(O.random_points(130, 64 + 130)) * (1.0 + symmetric_noise(130, rng))
    np.fill_diagonal(real, -1.0)
    add("caller_real", "costs", F64, 0, 0, xy, kind, real, integer=False)
    add("points_again", "rebuild", U16, 0, 0, xy, kind, cc)
    # a caller matrix of another n: the points are gone
    add("caller_other_n", "costs", U16, 0, 0, None, None, sym_int_matrix(50, rng))
    # ... and a last instance: K' = n - 1
    xy, kind = points_for("i32", 17, 11)
    add("n17", "points", I32, 0, 0, xy, kind, weight_matrix(xy, kind), K=16)
    return out


def stage_source(st):
    """the model's cost source: the coordinates in matrix-free mode (small sizes), else the matrix -- the same weights
    (test_two_opt_nl.test_model_coordinate_variant_equals_the_matrix_model)"""
    if st["mf"] and st["n"] < 500:
        return source_of("mf", st["xy"], st["kind"], st["c"])
    return dict(costs=st["c"])


@functools.lru_cache(maxsize=None)
def stage_models(index):
    """everything the probe expects at a stage, from the CPU models alone"""
    st = ladder()[index]
    n, K, c = st["n"], st["K"], st["c"]
    src = stage_source(st)
    rng = np.random.default_rng(9000 + index)
    w = {}
    w["nodes"], w["weights"] = model_lists(K, **src)
    nodes = w["nodes"]
    w["nn"] = [O.nn_tour(c, s) for s in range(4)]
    slot0, count = st["batch"]
    # (the stripe tour and random ones; nearest-neighbour tours in place of the random ones at the larger sizes, see single())
    tours = ([stripe_tour(st["xy"])] if st["xy"] is not None else []) + \
        [random_tour(n, rng) if n <= 300 else O.nn_tour(c, int(rng.integers(4, n)))[0] for _ in range(count)]
    w["tours"] = tours[:count]
    w["batch"] = []
    for t in w["tours"]:
        p = t.copy()
        w["batch"].append((p, model_ls_descent(p, nodes, **src)))

    def single(fn):
        # (random tours where the models' descents from them take no time, nearest-neighbour tours at the larger sizes)
        t = random_tour(n, rng) if n <= 300 else O.nn_tour(c, int(rng.integers(4, n)))[0]
        p = t.copy()
        return t, p, fn(p)
    w["multi"] = single(lambda p: M2.model_descent(p, **src))
    w["nl"] = single(lambda p: G2.model_descent(p, nodes, False, **src))
    w["or_nl"] = single(lambda p: model_or_nl_phase(p, O.tour_cost(c, p), nodes, **src))
    w["ls_nl"] = single(lambda p: model_ls_descent(p, nodes, **src))
    p = w["nn"][1][0].copy()
    w["two_opt"] = (w["nn"][1][0], p, O.two_opt(c, p))
    # Or-opt from a nearest-neighbour tour (to its end at the small sizes, 25 moves at the others), the 2-opt + Or-opt descent
    # from tours the descent over the lists has left (a few moves from a full local optimum)
    w["or_cap"] = -1 if n <= 100 else 25
    p = w["nn"][2][0].copy()
    w["or"] = (w["nn"][2][0], p, or_opt_phase(c, p, w["nn"][2][1], w["or_cap"])[:2])
    p = w["ls_nl"][1].copy()
    w["ls"] = (w["ls_nl"][1], p, descent_model(c, p))
    w["batch_ls"] = []
    for t, _ in w["batch"][:3]:
        p = t.copy()
        w["batch_ls"].append((t, p, descent_model(c, p)))
    w["ms2"] = O.multistart_nn_2opt(c, [0, 1, 2, 3])
    w["msnl"] = [nl_entry(c, nodes, s, **src) for s in range(4)]
    if st["how"] != "costs" and st["kind"] == EUC_2D:
        for s in range(4):          # (the golden's own record of a start, where it applies: EUC_2D from the coordinates)
            assert start_entry(st["xy"], nodes, s)[0] == w["msnl"][s][0], (st["name"], s)
    return w


def set_options(eng, st):
    eng.set_option(T().OPT_ELEM, st["elem"])
    eng.set_option(T().OPT_MATRIX_FREE, 1 if st["mf"] else 2)
    eng.set_option(T()._lib.OPT_OR_MATRIX_FREE, st["or_mf"])


def advance(eng, st):
    """the long-lived context's step to the stage"""
    set_options(eng, st)
    if st["how"] == "points":
        eng.set_points(st["xy"], st["kind"])
        eng.build_costs()
    elif st["how"] == "rebuild":
        eng.build_costs()
    else:
        eng.set_costs(st["c"])


def fresh_engine(st):
    """a new context with the stage's options and set-up calls"""
    eng = T().Engine(0)
    set_options(eng, st)
    if st["xy"] is not None:
        eng.set_points(st["xy"], st["kind"])
    if st["how"] == "costs":
        eng.set_costs(st["c"])
    else:
        eng.build_costs()
    return eng


def probe_slots(st):
    slot0, count = st["batch"]
    return [0] + list(range(slot0, slot0 + count)) + list(range(S_MULTI, S_BLS + 3))


def probe(eng, st, w):
    """every family once, each result against the model -> what was observed, for the comparison with the other context"""
    c, n, K, integer = st["c"], st["n"], st["K"], st["integer"]
    what = st["name"]
    obs, ran = [], ["two_opt", "multi", "nl", "or_nl", "nl_batch"]

    def stored(slot, path, tag, cost=None, delta=None):
        got, gcost, gdelta = eng.tour_store(slot)
        assert np.array_equal(got, path), (what, tag)
        cost_is(gcost, c, got, integer, (what, tag))
        if integer and cost is not None:
            assert gcost == cost, (what, tag)
        if delta is not None:
            assert gdelta == delta, (what, tag)
        obs.append((tag, got.tobytes(), gcost, gdelta))

    # nearest-neighbour tours: on a slot and through the host arrays
    eng.tour_nn(0, 0)
    stored(0, w["nn"][0][0], "tour_nn")
    path, cost = eng.nn_tour(0)
    assert np.array_equal(path, w["nn"][0][0]), what
    assert cost == w["nn"][0][1] if integer else abs(cost - w["nn"][0][1]) <= 1e-9 * cost, what
    obs.append(("nn_tour", path.tobytes(), cost))
    # the lists
    eng.neighbours_build(K)
    nodes, weights = eng.neighbours_get()
    assert eng.info()["nl_k"] == min(K, n - 1) == w["nodes"].shape[1], what
    assert np.array_equal(nodes, w["nodes"]) and np.array_equal(weights, w["weights"]), what
    # the batched descent over the lists, lowest slot first
    slot0, count = st["batch"]
    for i, t in enumerate(w["tours"]):
        eng.tour_load(slot0 + i, t)
    r = eng.tours_local_search_nl(slot0, count)
    assert r["rc"] == 0, what
    for i, (p, rec) in enumerate(w["batch"]):
        assert {k: int(r[k][i]) for k in COUNTERS} == {k: rec[k] for k in COUNTERS}, (what, i)
        stored(slot0 + i, p, ("batch", i), rec["cost"], 0.0)
    info = eng.info()
    longest = max(rec["two_opt_sweeps"] + rec["or_sweeps"] for _, rec in w["batch"])
    assert info["nl_batch_tours"] == count == info["nl_batch_max_live"] and longest <= info["nl_batch_launches"] <= longest + 3, what
    # the single-tour families on further slots
    t, p, m = w["multi"]
    eng.tour_load(S_MULTI, t)
    assert eng.tour_two_opt_multi(S_MULTI) == (m["sweeps"], m["moves"], 0), what
    stored(S_MULTI, p, "multi", m["cost"], 0.0)
    info = eng.info()
    assert (info["multi_sweeps"], info["multi_moves"], info["multi_max_moves"]) == (m["sweeps"], m["moves"], m["max_k"]), what
    t, p, m = w["nl"]
    eng.tour_load(S_NL, t)
    assert eng.tour_two_opt_nl(S_NL) == (m["sweeps"], m["moves"], 0), what
    stored(S_NL, p, "nl", m["cost"], 0.0)
    info = eng.info()
    assert (info["nl_sweeps"], info["nl_moves"]) == (m["sweeps"], m["moves"]), what
    t, p, (mcost, sweeps, moves, most) = w["or_nl"]
    eng.tour_load(S_ORNL, t)
    assert eng.tour_or_opt_nl(S_ORNL) == (sweeps, moves, 0), what
    stored(S_ORNL, p, "or_nl", mcost, 0.0)
    info = eng.info()
    assert (info["or_nl_sweeps"], info["or_nl_moves"], info["or_nl_max_moves"]) == (sweeps, moves, most), what
    t, p, m = w["ls_nl"]
    eng.tour_load(S_LSNL, t)
    r = eng.tour_local_search_nl(S_LSNL)
    assert r["rc"] == 0 and {k: r[k] for k in COUNTERS} == {k: m[k] for k in COUNTERS}, what
    stored(S_LSNL, p, "ls_nl", m["cost"], 0.0)
    info = eng.info()
    assert (info["or_nl_rounds"], info["or_nl_sweeps"], info["or_nl_moves"]) == (m["rounds"], m["or_sweeps"], m["or_moves"]), what
    t, p, (sweeps, mcost) = w["two_opt"]
    eng.tour_load(S_2OPT, t)
    assert eng.tour_two_opt(S_2OPT) == (sweeps, 0), what
    stored(S_2OPT, p, "two_opt", mcost)
    # Or-opt and the 2-opt + Or-opt descent: matrix mode, or single tours with TSPGPU_OPT_OR_MATRIX_FREE = 1; else 12
    eng.tour_load(S_OR, w["or"][0])
    eng.tour_load(S_LS, w["ls"][0])
    for i, (t, _, _) in enumerate(w["batch_ls"]):
        eng.tour_load(S_BLS + i, t)
    nb = len(w["batch_ls"])
    if not st["mf"] or st["or_mf"]:
        ran.append("or")
        t, p, (mcost, moves) = w["or"]
        assert eng.tour_or_opt(S_OR, max_moves=w["or_cap"]) == (moves, 0), what
        stored(S_OR, p, "or", mcost)
        t, p, m = w["ls"]
        r = eng.tour_local_search(S_LS)
        assert r["rc"] == 0 and {k: r[k] for k in m if k != "cost"} == {k: m[k] for k in m if k != "cost"}, what
        stored(S_LS, p, "ls", m["cost"])
    else:
        refused(lambda: eng.tour_or_opt(S_OR, max_moves=1), 12, "matrix-free")
        refused(lambda: eng.tour_local_search(S_LS), 12, "matrix-free")
    if not st["mf"]:
        ran.append("or_batch")
        r = eng.tours_local_search(S_BLS, nb)
        assert r["rc"] == 0, what
        for i, (t, p, m) in enumerate(w["batch_ls"]):
            assert (int(r["two_opt_sweeps"][i]), int(r["or_moves"][i]), int(r["rounds"][i])) == (m["two_opt_sweeps"], m["or_moves"], m["rounds"]), (what, i)
            stored(S_BLS + i, p, ("batch_ls", i), m["cost"])
    else:
        refused(lambda: eng.tours_local_search(S_BLS, nb), 12, "matrix-free")
        refused(lambda: eng.multistart_local_search([0, 1]), 12, "matrix-free")
    # the multi-starts (slots 0 .. 3 are their scratch)
    best, mcost, arg, sweeps = w["ms2"]
    r = eng.multistart_nn_2opt([0, 1, 2, 3])
    assert (r["rc"], r["start"], r["sweeps"]) == (0, arg, sweeps) and np.array_equal(r["path"], best), what
    cost_is(r["cost"], c, r["path"], integer, (what, "ms2"))
    obs.append(("ms2", r["path"].tobytes(), r["cost"]))
    rows = [e for e, _ in w["msnl"]]
    costs = [e["cost"] for e in rows]
    win = costs.index(min(costs))
    r = eng.multistart_local_search_nl([0, 1, 2, 3])
    assert (r["rc"], r["start"]) == (0, win) and np.array_equal(r["path"], w["msnl"][win][1]), what
    assert {k: r[k] for k in COUNTERS[:4]} == {k: sum(e[k] for e in rows) for k in COUNTERS[:4]}, what
    cost_is(r["cost"], c, r["path"], integer, (what, "msnl"))
    for s in range(4):
        cost_is(float(r["costs"][s]), c, w["msnl"][s][1], integer, (what, "msnl", s))
    obs.append(("msnl", r["path"].tobytes(), r["cost"], r["costs"].tobytes()))
    info = eng.info()
    keys = GEOMETRY_KEYS + tuple(k for f in ran for k in FAMILY_KEYS[f])
    obs.append(("info", {k: info[k] for k in keys}))
    return obs


def check_dropped(eng, slots, had_lists):
    """after a new cost source and before its first use: no slot holds a tour, the lists are gone and say why"""
    for s in slots:
        refused(lambda: eng.tour_store(s), 9, "slot %d holds no tour" % s)
    if had_lists:
        for call in (eng.neighbours_get, lambda: eng.tours_local_search_nl(0, 1), lambda: eng.multistart_local_search_nl([0]),
                     lambda: eng.tour_two_opt_nl(0, max_sweeps=1), lambda: eng.tour_or_opt_nl(0, max_sweeps=1)):
            refused(call, 9, "invalidated by a new cost source")
    eng.neighbours_build(0)
    assert eng.info()["nl_k"] == 0
    refused(eng.neighbours_get, 9, "no neighbour lists: call tspgpu_neighbours_build first", without=("invalidated",))
    refused(lambda: eng.tours_local_search_nl(0, 1), 9, "no neighbour lists: call tspgpu_neighbours_build first", without=("invalidated",))


def test_ladder_goes_up_and_down_and_through_every_switch():
    L = ladder()
    sizes = [st["n"] for st in L if st["how"] == "points"][:len(LADDER_SIZES)]
    assert tuple(sizes) == LADDER_SIZES and set(LADDER_SIZES) == {200, 40, 1025, 8, 300, 64, 33, 257}
    steps = [b - a for a, b in zip(sizes, sizes[1:])]
    assert sum(d > 0 for d in steps) >= 3 and sum(d < 0 for d in steps) >= 3
    assert {st["K"] for st in L} == set(LADDER_KS) and any(st["K"] == 16 and st["n"] == 8 for st in L)
    by = {st["name"]: st for st in L}
    names = [st["name"] for st in L]
    # cell types and modes change under the same points, with tspgpu_build_costs alone
    at = names.index("n257")
    assert [(st["elem"], st["mf"], st["how"]) for st in L[at:at + 5]] == \
        [(U16, 0, "points"), (F64, 0, "rebuild"), (I32, 0, "rebuild"), (I32, 1, "rebuild"), (U16, 0, "rebuild")]
    # the batched call: 3, 10 and 2 tours (from slot 7) on one instance, then 5 on a new n
    assert [st["batch"] for st in L[at:at + 3]] == [(0, 3), (0, 10), (7, 2)] and len({st["n"] for st in L[at:at + 5]}) == 1
    nxt = next(st for st in L[at + 3:] if st["how"] == "points")
    assert nxt["batch"] == (0, 5) and nxt["n"] != 257
    # weight kinds, and both CEIL_2D forms
    assert [st["kind"] for st in L[at + 4:at + 8]] == [EUC_2D, ATT, CEIL_2D, CEIL_2D]
    real, integer = by["ceil_real"]["xy"], by["ceil_int"]["xy"]
    assert np.any(real != np.floor(real)) and np.all(integer == np.floor(integer))
    # caller matrices: the same n as the points before them (integers, then real values), then the points again, then another n
    assert [by[k]["n"] for k in ("ceil_int", "caller_u16", "caller_real", "points_again")] == [130] * 4
    assert by["caller_u16"]["integer"] and np.all(by["caller_u16"]["c"] == np.floor(by["caller_u16"]["c"]))
    assert not by["caller_real"]["integer"] and np.any(by["caller_real"]["c"] != np.floor(by["caller_real"]["c"]))
    assert by["points_again"]["how"] == "rebuild" and np.array_equal(by["points_again"]["c"], by["ceil_int"]["c"])
    assert by["caller_other_n"]["n"] != 130 and by["caller_other_n"]["xy"] is None
    # Or-opt in matrix-free mode: allowed at one stage, refused at another
    assert {(st["mf"], st["or_mf"]) for st in L} == {(0, 0), (1, 1), (1, 0)}
    for st in L:
        slot0, count = st["batch"]
        assert st["n"] >= 8 and slot0 + count <= S_MULTI and (3 <= count <= 10 or (slot0, count) == (7, 2))      # three to five tours, but for the growth


def test_ladder_models_of_the_small_stages():
    """the probe's expectations exist and are what they should be where that is cheap to say: descents end in optima of their
    own neighbourhoods, and the real-valued stage is real-valued all the way"""
    L = ladder()
    for st in L:
        if st["n"] > 64:
            continue
        w = stage_models(st["index"])
        for p, rec in w["batch"]:
            assert O.valid_tour(p) and tuple(model_ls_descent(p.copy(), w["nodes"], **stage_source(st))[k] for k in COUNTERS) == (1, 0, 1, 0, 1)
        assert not O.two_opt_once(st["c"], w["two_opt"][1].copy(), 0.0)[0] < EPS
        assert not O.two_opt_once(st["c"], w["ls"][1].copy(), 0.0)[0] < EPS


_LONG = {"eng": None, "at": -1, "used": [], "lists": False}       # the long-lived context of the ladder and where it stands


def ladder_step(st, compare=True):
    """the long-lived context's step to `st`, the checks between two stages, the probe -- and the same probe on a fresh context"""
    eng = _LONG["eng"]
    advance(eng, st)
    check_dropped(eng, _LONG["used"], _LONG["lists"])
    w = stage_models(st["index"])
    long_lived = probe(eng, st, w)
    _LONG.update(at=st["index"], used=probe_slots(st), lists=True)
    if st["name"] == "caller_other_n":
        refused(eng.build_costs, 9, "no points")
        assert np.array_equal(eng.tour_store(S_2OPT)[0], w["two_opt"][1])       # (the refusal has not touched what is in place)
    if not compare:
        return
    other = fresh_engine(st)
    fresh = probe(other, st, w)
    other.close()
    assert len(long_lived) == len(fresh)
    for a, b in zip(long_lived, fresh):
        if a[0] == "info":
            assert a == b, (st["name"], "info: long-lived, fresh", {k: (a[1][k], b[1][k]) for k in a[1] if a[1][k] != b[1][k]})
        assert a == b, (st["name"], a[0])


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(ladder())), ids=[st["name"] for st in ladder()])
def test_gpu_ladder_of_instances_through_one_context(index):
    """ONE Engine through every stage of ladder(), a stage per case, in order: the context is kept between the cases (a case that
    does not find it at the stage before its own -- run alone, or out of order -- takes a new one through the earlier stages
    first, probes included).  After the stage's set-up the probe runs on it and on a fresh Engine with the same options and
    set-up calls.  Both must give the models' results; their costs must agree to the bit (the real-valued stage included) and
    so must the geometry words of tspgpu_info and the per-call words of the families the probe ran.  Between two stages,
    before the new cost source is used: no slot holds a tour (9), the lists are gone and say why (9)."""
    L = ladder()
    if _LONG["eng"] is None or _LONG["at"] != index - 1:
        if _LONG["eng"] is not None:
            _LONG["eng"].close()
        _LONG.update(eng=T().Engine(0), at=-1, used=[], lists=False)
        for st in L[:index]:
            ladder_step(st, compare=False)
    try:
        ladder_step(L[index])
    except BaseException:
        _LONG["eng"].close()
        _LONG.update(eng=None, at=-1)
        raise
    if index == len(L) - 1:
        _LONG["eng"].close()
        _LONG.update(eng=None, at=-1)


# ================================================================================= 2. the slot array grows under live tours
STATES = ("loaded", "flipped", "or_nl_sweep", "ls_nl_done", "two_opt_sweep")


@functools.lru_cache(maxsize=None)
def growth_case(n):
    """n nodes (the same integer points in the modes u16, f64 and mf_euc), K = 5, and for the slots 0 .. 15 a start tour, the
    state it is brought into and the model's tour and cost in that state; what every later call of the test must give"""
    import test_or_opt_geometry as OG
    K = 5
    xy, kind = points_for("u16", n, 2)
    for mode in ("f64", "mf_euc"):
        assert np.array_equal(points_for(mode, n, 2)[0], xy) and points_for(mode, n, 2)[1] == kind
    c = weight_matrix(xy, kind)
    nodes, _ = model_lists(K, costs=c)
    g = dict(xy=xy, kind=kind, c=c, K=K, nodes=nodes, slots=[])
    for s in range(16):
        state = STATES[s % 5]
        rec = dict(state=state)
        if state == "flipped":
            # a random tour and a long-arc 2-opt flip that improves it: the slot is left with dir = -1 and a rotated ord
            # (test_nl_batch.planted_case)
            for seed in range(100 * s, 100 * s + 100):
                t = random_tour(n, np.random.default_rng(seed))
                for fl in OG.long_arc_flip(t):
                    p = t.copy()
                    O.apply_move(p, None, fl[0], fl[1])
                    d = O.tour_cost(c, p) - O.tour_cost(c, t)
                    lay = OG.Layout(t)
                    lay.flip(*fl)
                    if d < EPS and lay.dir == -1 and int(np.nonzero(lay.ord == 0)[0][0]) != 0:
                        break
                else:
                    continue
                break
            else:
                raise AssertionError("no improving long-arc flip")
            rec.update(start=t, move=(fl[0], fl[1], d), path=p, cost=O.tour_cost(c, p))
        else:
            t = O.nn_tour(c, (3 * s + 1) % n)[0] if s % 2 else random_tour(n, np.random.default_rng(500 + s))
            p, cost = t.copy(), O.tour_cost(c, t)
            if state == "or_nl_sweep":
                cost = model_or_sweep(p, cost, nodes, costs=c)["cost"]
            elif state == "ls_nl_done":
                cost = model_ls_descent(p, nodes, costs=c)["cost"]
            elif state == "two_opt_sweep":
                cost = O.two_opt_once(c, p, cost)[1]
            rec.update(start=t, path=p, cost=cost)
        g["slots"].append(rec)
    assert {r["state"] for r in g["slots"][8:]} == set(STATES)
    paths = [r["path"] for r in g["slots"]]
    # how each family goes on from a slot (one family per slot 0 .. 7)
    p = paths[0].copy()
    d, cost, _ = O.two_opt_once(c, p, g["slots"][0]["cost"])
    g["next_two_opt"] = (p, cost)
    p = paths[1].copy()
    r = M2.model_sweep(p, g["slots"][1]["cost"], costs=c)
    g["next_multi"] = (p, r["cost"], len(r["moves"]))
    p = paths[2].copy()
    r = G2.model_sweep(p, g["slots"][2]["cost"], nodes, costs=c)
    g["next_nl"] = (p, r["cost"], len(r["moves"]))
    p = paths[3].copy()
    r = model_or_sweep(p, g["slots"][3]["cost"], nodes, costs=c)
    g["next_or_nl"] = (p, r["cost"], len(r["moves"]))
    p = paths[4].copy()
    g["next_ls_nl"] = (p, model_ls_descent(p, nodes, costs=c))
    p = paths[5].copy()
    cost, m, _ = or_opt_phase(c, p, g["slots"][5]["cost"], max_moves=1)
    g["next_or"] = (p, cost, m)
    p = paths[6].copy()
    cost = g["slots"][6]["cost"]
    for _ in range(3):
        cost = O.two_opt_once(c, p, cost)[1]
    g["next_two_opt3"] = (p, cost)
    p = paths[7].copy()
    d, cost, (a, b) = O.two_opt_once(c, p, g["slots"][7]["cost"])
    g["next_apply"] = (p, cost, (a, b, d))
    assert d < EPS
    # the batched descent over the lists from the slots 8 .. 15 as they stand
    g["batch"] = []
    for r in g["slots"][8:]:
        p = r["path"].copy()
        g["batch"].append((p, model_ls_descent(p, nodes, costs=c)))
    # the multi-start that grows the array a second time, and what it leaves in the slots 8 .. 15: the 2-opt optima of the
    # nearest-neighbour tours from 8 .. 15; the batched descent from those
    g["ms2"], every = multistart_two_opt(c, list(range(48)))
    g["left"], g["batch2"] = every[8:16], []
    for p, _ in g["left"]:
        q = p.copy()
        g["batch2"].append((q, model_ls_descent(q, nodes, costs=c)))
    g["nn7"] = O.nn_tour(c, 7)
    return g


def test_growth_case_covers_every_state():
    g = growth_case(65)
    assert [r["state"] for r in g["slots"]].count("flipped") == 3 and all(O.valid_tour(r["path"]) for r in g["slots"])
    for r in g["slots"]:
        assert r["cost"] == O.tour_cost(g["c"], r["path"])
        if r["state"] != "loaded":
            assert r["cost"] < O.tour_cost(g["c"], r["start"])            # every state is a state after at least one move
    assert g["next_multi"][2] >= 1 and g["next_nl"][2] >= 1 and g["next_or"][2] == 1
    # the multi-start's expectation is the oracle's own loop
    best, cost, arg, sweeps = O.multistart_nn_2opt(g["c"], list(range(48)))
    assert (cost, arg, sweeps) == g["ms2"][1:] and np.array_equal(best, g["ms2"][0])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 1100])
@pytest.mark.parametrize("mode", ["u16", "f64", "mf_euc"])
def test_gpu_slot_array_growth_with_live_tours(mode, n):
    """slots 0 .. 15 (the initial capacity) filled lowest first with tours in five states; tspgpu_tour_nn(40, 7) grows the array:
    every slot stores what it stored, bit for bit, and every family goes on from it as its model does.  A multi-start over 48
    starts (TSPGPU_OPT_MAX_TOURS = 64) grows it again: the oracle's result, and nothing beyond slot 47.  The multi-starts use
    the slots from 0 upwards as scratch (include/tspgpu.h), so the batched descent over the slots 8 .. 15 runs twice: after
    the first growth on the tours loaded before it, after the second on what the multi-start left there -- the model's 2-opt
    optima of the nearest-neighbour tours from 8 .. 15."""
    g = growth_case(n)
    c, nodes = g["c"], g["nodes"]
    eng = engine_for(mode, g["xy"], g["kind"])
    eng.set_option(T()._lib.OPT_OR_MATRIX_FREE, 1)
    eng.neighbours_build(g["K"])
    for s, r in enumerate(g["slots"]):
        eng.tour_load(s, r["start"])
        if r["state"] == "flipped":
            eng.tour_apply_move(s, *r["move"])
        elif r["state"] == "or_nl_sweep":
            assert eng.tour_or_opt_nl(s, max_sweeps=1)[0] == 1
        elif r["state"] == "ls_nl_done":
            assert eng.tour_local_search_nl(s)["rc"] == 0
        elif r["state"] == "two_opt_sweep":
            assert eng.tour_two_opt(s, max_sweeps=1) == (1, 0)
    before = [eng.tour_store(s) for s in range(16)]
    for s, r in enumerate(g["slots"]):
        assert np.array_equal(before[s][0], r["path"]) and before[s][1] == r["cost"], (s, r["state"])
    refused(lambda: eng.tour_store(16), 9, "holds no tour")
    eng.tour_nn(40, 7)                                                # the first growth
    for s in range(16):
        path, cost, delta = eng.tour_store(s)
        assert np.array_equal(path, before[s][0]) and (cost, delta) == before[s][1:], (s, g["slots"][s]["state"])
    path, cost, _ = eng.tour_store(40)
    assert np.array_equal(path, g["nn7"][0]) and cost == g["nn7"][1]
    for s in list(range(16, 40)) + [41]:
        refused(lambda: eng.tour_store(s), 9, "holds no tour")

    def stored(slot, path, cost, what):
        got, gcost, _ = eng.tour_store(slot)
        assert np.array_equal(got, path) and gcost == cost, what
    assert eng.tour_two_opt(0, max_sweeps=1) == (1, 0)
    stored(0, *g["next_two_opt"], "two_opt")
    assert eng.tour_two_opt_multi(1, max_sweeps=1) == (1, g["next_multi"][2], 0)
    stored(1, *g["next_multi"][:2], "multi")
    assert eng.tour_two_opt_nl(2, max_sweeps=1) == (1, g["next_nl"][2], 0)
    stored(2, *g["next_nl"][:2], "nl")
    assert eng.tour_or_opt_nl(3, max_sweeps=1) == (1, g["next_or_nl"][2], 0)
    stored(3, *g["next_or_nl"][:2], "or_nl")
    r = eng.tour_local_search_nl(4)
    assert r["rc"] == 0 and {k: r[k] for k in COUNTERS} == {k: g["next_ls_nl"][1][k] for k in COUNTERS}
    stored(4, g["next_ls_nl"][0], g["next_ls_nl"][1]["cost"], "ls_nl")
    assert eng.tour_or_opt(5, max_moves=1) == (g["next_or"][2], 0)
    stored(5, *g["next_or"][:2], "or")
    assert eng.tour_two_opt(6, max_sweeps=3) == (3, 0)
    stored(6, *g["next_two_opt3"], "two_opt3")
    eng.tour_apply_move(7, *g["next_apply"][2])
    stored(7, *g["next_apply"][:2], "apply")

    def batched(want, what):
        r = eng.tours_local_search_nl(8, 8)
        assert r["rc"] == 0
        for i, (p, rec) in enumerate(want):
            assert {k: int(r[k][i]) for k in COUNTERS} == {k: rec[k] for k in COUNTERS}, (what, i)
            got, cost, delta = eng.tour_store(8 + i)
            assert np.array_equal(got, p) and (cost, delta) == (rec["cost"], 0.0), (what, i)
    batched(g["batch"], "after the first growth")
    eng.set_option(T().OPT_MAX_TOURS, 64)
    best, cost, arg, sweeps = g["ms2"]
    r = eng.multistart_nn_2opt(list(range(48)))                       # the second growth
    assert (r["rc"], r["cost"], r["start"], r["sweeps"]) == (0, cost, arg, sweeps) and np.array_equal(r["path"], best)
    for s in (48, 49, 63, 64):
        refused(lambda: eng.tour_store(s), 9, "holds no tour")
    for i, (p, cost) in enumerate(g["left"]):
        stored(8 + i, p, cost, ("left", i))
    batched(g["batch2"], "after the second growth")
    eng.close()


# ====================================================================================== 3. every family in turn on one slot
FAMILIES = ("two_opt", "or_opt", "two_opt_multi", "two_opt_nl", "or_opt_nl", "apply_move")
FAMILY_SEED, FAMILY_STEPS = 264, 60


def family_sequence():
    return [FAMILIES[i] for i in np.random.default_rng(FAMILY_SEED).integers(0, len(FAMILIES), FAMILY_STEPS)]


@functools.lru_cache(maxsize=None)
def alternation_case(n):
    """the models' walk through family_sequence() from a random tour of n nodes (the same integer points in u16, f64 and mf_euc)
    -> dict(xy, kind, K, start, steps: [(family, path after, cost after, count, the move handed to apply_move or None)])"""
    K = 5
    xy, kind = points_for("u16", n, 3)
    for mode in ("f64", "mf_euc"):
        assert np.array_equal(points_for(mode, n, 3)[0], xy)
    c = weight_matrix(xy, kind)
    nodes, _ = model_lists(K, costs=c)
    start = random_tour(n, np.random.default_rng(n))
    path, cost = start.copy(), O.tour_cost(c, start)
    steps = []
    for fam in family_sequence():
        move = None
        if fam == "two_opt":
            d, cost, _ = O.two_opt_once(c, path, cost)
            count, moved = 1, d < EPS                          # (tspgpu_tour_two_opt counts its sweeps)
        elif fam == "or_opt":
            cost, count, _ = or_opt_phase(c, path, cost, max_moves=1)
            moved = count == 1
        elif fam == "apply_move":
            probe_ = path.copy()
            d, _, (a, b) = O.two_opt_once(c, probe_, cost)
            moved = d < EPS
            move, count = (a, b, d) if moved else (0, 0, 0.0), None       # (tspgpu_tour_sweep_part's "nothing improves")
            if moved:
                O.apply_move(path, None, a, b)
                cost += d
                assert np.array_equal(path, probe_)
        else:
            r = (M2.model_sweep(path, cost, costs=c) if fam == "two_opt_multi" else
                 G2.model_sweep(path, cost, nodes, costs=c) if fam == "two_opt_nl" else model_or_sweep(path, cost, nodes, costs=c))
            cost, count = r["cost"], len(r["moves"])
            moved = count > 0
        assert cost == O.tour_cost(c, path)
        steps.append((fam, path.copy(), cost, count, move, moved))
    return dict(xy=xy, kind=kind, K=K, c=c, start=start, steps=steps)


def test_family_sequence_lets_every_family_follow_every_other():
    seq = family_sequence()
    assert len(seq) == 60 and set(seq) == set(FAMILIES)
    pairs = set(zip(seq, seq[1:]))
    assert all((a, b) in pairs for a in FAMILIES for b in FAMILIES if a != b)


@pytest.mark.parametrize("n", [65, 1100])
def test_family_sequence_keeps_moving(n):
    """from a random tour the sixty steps do not reach a common optimum: at least 40 of them apply a move, by the models alone"""
    steps = alternation_case(n)["steps"]
    assert sum(1 for st in steps if st[5]) >= 40
    for fam in FAMILIES:
        assert any(st[5] for st in steps if st[0] == fam), fam


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 1100])
@pytest.mark.parametrize("mode", ["u16", "f64", "mf_euc"])
def test_gpu_every_family_in_turn_on_one_slot(mode, n):
    """test_or_opt.test_gpu_slot_invariants_under_alternation for all six ways to change a slot, in matrix-free mode too: after
    every step the slot stores the model's tour and its exact cost, and the call returns the model's count"""
    case = alternation_case(n)
    eng = engine_for(mode, case["xy"], case["kind"])
    eng.set_option(T()._lib.OPT_OR_MATRIX_FREE, 1)
    eng.neighbours_build(case["K"])
    eng.tour_load(0, case["start"])
    for k, (fam, path, cost, count, move, _) in enumerate(case["steps"]):
        if fam == "two_opt":
            assert eng.tour_two_opt(0, max_sweeps=1) == (count, 0), (k, fam)
        elif fam == "or_opt":
            assert eng.tour_or_opt(0, max_moves=1) == (count, 0), (k, fam)
        elif fam == "two_opt_multi":
            assert eng.tour_two_opt_multi(0, max_sweeps=1) == (1, count, 0), (k, fam)
        elif fam == "two_opt_nl":
            assert eng.tour_two_opt_nl(0, max_sweeps=1) == (1, count, 0), (k, fam)
        elif fam == "or_opt_nl":
            assert eng.tour_or_opt_nl(0, max_sweeps=1) == (1, count, 0), (k, fam)
        else:
            eng.tour_apply_move(0, *move)
        got, gcost, _ = eng.tour_store(0)
        assert np.array_equal(got, path) and gcost == cost, (k, fam)
    eng.close()


# ============================================================================ 4. the "last call" words describe the last call
@functools.lru_cache(maxsize=None)
def last_call_case():
    n, K = 1024, 8
    xy, kind = points_for("u16", n, 4)
    c = weight_matrix(xy, kind)
    nodes, _ = model_lists(K, costs=c)
    g = dict(xy=xy, kind=kind, c=c, K=K, nodes=nodes, n=n)
    g["start"] = O.nn_tour(c, 0)[0]
    p = g["start"].copy()
    g["two_opt"] = (p, O.two_opt(c, p))
    # two inputs per family, so that the second call's words cannot be the first's
    g["starts"] = [O.nn_tour(c, 0)[0], O.nn_tour(c, 5)[0], stripe_tour(xy)]
    g["multi"], g["nl"], g["or_nl"], g["ls_nl"] = [], [], [], []
    for t in g["starts"]:
        p = t.copy()
        g["multi"].append((p, M2.model_descent(p, costs=c)))
        p = t.copy()
        g["nl"].append((p, G2.model_descent(p, nodes, True, costs=c)))
        p = t.copy()
        g["or_nl"].append((p, model_or_nl_phase(p, O.tour_cost(c, t), nodes, costs=c)))
        p = t.copy()
        g["ls_nl"].append((p, model_ls_descent(p, nodes, costs=c)))
    return g


def test_last_call_inputs_differ():
    g = last_call_case()
    for key, words in (("multi", lambda m: (m["sweeps"], m["moves"], m["max_k"])),
                       ("nl", lambda m: (m["sweeps"], m["moves"], m["polish_sweeps"])),
                       ("or_nl", lambda m: m[1:]),
                       ("ls_nl", lambda m: (m["or_sweeps"], m["or_moves"], m["rounds"], m["two_opt_sweeps"]))):
        assert words(g[key][0][1]) != words(g[key][1][1]), key


@pytest.mark.gpu
def test_gpu_last_call_words_describe_the_last_call():
    """one context, uint16 cells, n = 1024 (the smallest size the streamed kernel takes).
    The descent three times from the same start: in the streamed kernel (TSPGPU_OPT_PERSIST = 0, _STREAM_PERSIST = 2), in the
    LDS-resident kernel (2, 1), one launch per sweep (0, 0); a forced kernel that does not run is code 8, so none of the three
    can pass without having run.  tspgpu_info 15 / 20 / 21 / 24 must say how THIS descent ran.  On the parent of the commit that
    added this test the second descent showed persist = 1 with stream_persist still 1: run_sweeps cleared the streamed
    kernel's word only behind the LDS-resident branch.
    Then every other family twice with different inputs: its words are the model's for the second call."""
    g = last_call_case()
    c, nodes = g["c"], g["nodes"]
    eng = engine_for("u16", g["xy"], g["kind"])
    want_path, (want_sweeps, want_cost) = g["two_opt"]

    def descend(persist, stream):
        eng.set_option(T().OPT_PERSIST, persist)
        eng.set_option(T().OPT_STREAM_PERSIST, stream)
        path = g["start"].copy()
        cost, sweeps, rc = eng.two_opt(path)
        assert (rc, cost, sweeps) == (0, want_cost, want_sweeps) and np.array_equal(path, want_path), (persist, stream)
        info = eng.info()
        print("descent with TSPGPU_OPT_PERSIST = %d, TSPGPU_OPT_STREAM_PERSIST = %d:" % (persist, stream),
              {k: info[k] for k in ("persist", "persist_window", "persist_handed", "stream_persist", "persist_sweeps")})
        return info
    info = descend(0, 2)
    assert (info["stream_persist"], info["persist"]) == (1, 0)
    info = descend(2, 1)
    assert info["persist"] == 1
    assert info["stream_persist"] == 0
    info = descend(0, 0)
    assert (info["persist"], info["persist_window"], info["persist_handed"], info["stream_persist"]) == (0, 0, 0, 0)
    eng.set_option(T().OPT_PERSIST, 1)
    eng.set_option(T().OPT_STREAM_PERSIST, 1)
    eng.neighbours_build(g["K"])
    for i in (0, 1):
        p, m = g["multi"][i]
        path = g["starts"][i].copy()
        assert eng.two_opt_multi(path) == (m["cost"], m["sweeps"], m["moves"], 0) and np.array_equal(path, p)
        info = eng.info()
        assert (info["multi_sweeps"], info["multi_moves"], info["multi_max_moves"]) == (m["sweeps"], m["moves"], m["max_k"]), i
    for i in (0, 1):
        p, m = g["nl"][i]
        path = g["starts"][i].copy()
        r = eng.two_opt_nl(path, polish=True)
        assert (r["rc"], r["cost"], r["sweeps"], r["moves"], r["polish_sweeps"], r["polish_moves"]) == \
            (0, m["cost"], m["sweeps"], m["moves"], m["polish_sweeps"], m["polish_moves"]) and np.array_equal(path, p)
        info = eng.info()
        assert (info["nl_sweeps"], info["nl_moves"], info["nl_polish_sweeps"]) == (m["sweeps"], m["moves"], m["polish_sweeps"]), i
    # (a neighbour-list phase without polish after one with: the polish word is this call's, 0)
    eng.tour_load(0, g["starts"][2])
    p, m = g["nl"][2]
    assert eng.tour_two_opt_nl(0) == (m["sweeps"], m["moves"], 0)
    info = eng.info()
    assert (info["nl_sweeps"], info["nl_moves"], info["nl_polish_sweeps"]) == (m["sweeps"], m["moves"], 0)
    for i in (0, 1):
        p, (mcost, sweeps, moves, most) = g["or_nl"][i]
        path = g["starts"][i].copy()
        assert eng.or_opt_nl(path, O.tour_cost(c, path)) == (mcost, sweeps, moves, 0) and np.array_equal(path, p)
        info = eng.info()
        assert (info["or_nl_sweeps"], info["or_nl_moves"], info["or_nl_max_moves"]) == (sweeps, moves, most), i
    for i in (0, 1):
        p, m = g["ls_nl"][i]
        path = g["starts"][i].copy()
        r = eng.local_search_nl(path)
        assert r["rc"] == 0 and {k: r[k] for k in COUNTERS} == {k: m[k] for k in COUNTERS} and r["cost"] == m["cost"] and np.array_equal(path, p)
        info = eng.info()
        assert (info["or_nl_sweeps"], info["or_nl_moves"], info["or_nl_rounds"]) == (m["or_sweeps"], m["or_moves"], m["rounds"]), i
    # the batched descent over the lists: three tours, then two
    for tours in ((0, 1, 2), (1, 0)):
        for s, i in enumerate(tours):
            eng.tour_load(s, g["starts"][i])
        r = eng.tours_local_search_nl(0, len(tours))
        assert r["rc"] == 0
        for s, i in enumerate(tours):
            assert {k: int(r[k][s]) for k in COUNTERS} == {k: g["ls_nl"][i][1][k] for k in COUNTERS}
        info = eng.info()
        longest = max(g["ls_nl"][i][1]["two_opt_sweeps"] + g["ls_nl"][i][1]["or_sweeps"] for i in tours)
        assert (info["nl_batch_tours"], info["nl_batch_max_live"]) == (len(tours), len(tours))
        assert longest <= info["nl_batch_launches"] <= longest + 3
    # the batched 2-opt + Or-opt descent, three tours and then one.  No model knows the sweep's R: a fresh context that
    # makes the second call alone is the witness here
    ends = [g["ls_nl"][i][0] for i in range(3)]
    for s in range(3):
        eng.tour_load(s, ends[s])
    assert eng.tours_local_search(0, 3)["rc"] == 0
    r3 = eng.info()["or_batch_r"]
    eng.tour_load(0, ends[1])
    assert eng.tours_local_search(0, 1)["rc"] == 0
    r1 = eng.info()["or_batch_r"]
    other = engine_for("u16", g["xy"], g["kind"])
    other.tour_load(0, ends[1])
    assert other.tours_local_search(0, 1)["rc"] == 0
    assert r1 == other.info()["or_batch_r"] and r1 > 0 and r3 > 0
    assert np.array_equal(other.tour_store(0)[0], eng.tour_store(0)[0])
    other.close()
    eng.close()


# ==================================================================================== 5. one multi-device handle, instances
@functools.lru_cache(maxsize=None)
def handle_case():
    g = {}
    for name in ("berlin52", "pr1002"):
        xy = G2.tsplib_points(name)
        nodes, _ = model_lists(8, xy=xy)
        g[name] = (xy, nodes)
    xy, kind = points_for("u16", 40, 5)
    assert kind == EUC_2D
    g["n40"] = (xy, model_lists(8, xy=xy)[0])
    return g


def check_handle_multistart(r, starts, entries):
    """entries: start_entry's (record, path) of every list entry"""
    costs = [e["cost"] for e, _ in entries]
    win = costs.index(min(costs))               # the earliest of equal costs
    assert (r["rc"], r["start"], r["cost"]) == (0, starts[win], costs[win])
    assert np.array_equal(r["path"], entries[win][1])
    assert {k: r[k] for k in COUNTERS[:4]} == {k: sum(e[k] for e, _ in entries) for k in COUNTERS[:4]}


def test_tie_pair_lands_on_two_contexts():
    """pr1002's starts 4 and 5 end at the same cost (tests/golden/golden_nl_batch.json): listed as [5, 4] and as [4, 5] behind a handle of two
    contexts (entry p on context p mod 2) the winner must be picked across the contexts, by the list position"""
    xy, nodes = handle_case()["pr1002"]
    (e4, p4), (e5, p5) = start_entry(xy, nodes, 4), start_entry(xy, nodes, 5)
    assert e4["cost"] == e5["cost"] == 273069.0
    for starts in ([5, 4], [4, 5]):
        assert [p % 2 for p in range(len(starts))] == [0, 1]


@pytest.mark.gpu
def test_gpu_one_handle_three_instances_and_a_tie_across_contexts():
    g = handle_case()
    m = T().MultiEngine([0, 0])
    # berlin52
    xy, nodes = g["berlin52"]
    m.set_points(xy)
    m.build_costs()
    m.neighbours_build(8)
    starts = list(range(8))
    check_handle_multistart(m.multistart_local_search_nl(starts), starts, [start_entry(xy, nodes, s) for s in starts])
    # 40 nodes on the same handle: the lists are berlin52's until they are built again
    xy, nodes = g["n40"]
    m.set_points(xy)
    m.build_costs()
    refused(lambda: m.multistart_local_search_nl(starts), 9, "invalidated by a new cost source")
    m.neighbours_build(8)
    check_handle_multistart(m.multistart_local_search_nl(starts), starts, [start_entry(xy, nodes, s) for s in starts])
    # pr1002: a cost tie between the two contexts goes to the earlier list entry
    xy, nodes = g["pr1002"]
    m.set_points(xy)
    m.build_costs()
    refused(lambda: m.multistart_local_search_nl([4, 5]), 9, "invalidated by a new cost source")
    m.neighbours_build(8)
    for starts in ([5, 4], [4, 5]):
        entries = [start_entry(xy, nodes, s) for s in starts]
        assert entries[0][0]["cost"] == entries[1][0]["cost"]
        r = m.multistart_local_search_nl(starts)
        check_handle_multistart(r, starts, entries)
        assert r["start"] == starts[0]
    m.close()
