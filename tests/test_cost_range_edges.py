"""The extension move families at the edges of the cost range: Or-opt (matrix and matrix-free), the parallel-move 2-opt, the
neighbour-list 2-opt / Or-opt / 3-opt, their descent, the batched and don't-look forms, the VNS walks over the lists, the
greedy-edge construction and Extra Mileage -- on weights at every threshold the engine changes representation at, on negative
costs, and with Extra Mileage's 64-bit keys filled to both ends of their fields.  Every other test of these families draws
weights below about 1.4e6.

- the table (CASES): test_gpu_edges._edge_instance on each side of 65 534 (uint16 -> int32 cells), 2^22 (CEIL_2D's integer
  ceil-sqrt and the int2 points of the matrix-free extension kernels -> the generic double form) and 2^27 (int32 -> f64 cells),
  and the f64 instance scaled by 8 (weights to 2^30, sums of three past 2^31).  Per case and cost source, on one engine: the
  lists and their stored weights, the first three sweeps of every family move by move, the descent with the 3-opt phase
  (host and slot form), greedy edge, Extra Mileage (both forms; refused with code 9 on f64 cells); on three cases the
  multi-start, the multi-start with looks and two VNS walks.  At the top of int32 the deltas of three edges pass 2^28 (the
  first 3-opt sweep of i32_top accepts -270 619 565), and T = Gmax + c[q][q'] - 1 of k_oropt_sweep_otf's early-out passes
  2^24, where (float)T rounds.
- signed costs (caller matrices, n = 9 .. 64): real values in (-50, 50); integers in -2 .. 2 with zeros of both signs (f64 cells,
  the sign branch of the order-preserving folds nl_ck(double) and ge_wkey); integers in [0, 60 000] with off-diagonal -1
  (the documented lower end of int32 cells).  The models are first pinned on these matrices to the brute-force restatements
  (CPU), then the device to the models.  Extra Mileage refuses all three with code 9.
- Extra Mileage's key fields: a constructed matrix whose insertion sequence holds a delta of exactly -(2^27 - 1) while
  another node's best delta stands at 2 (2^27 - 1) (both ends of the biased 29-bit field), one cell at 2^27 (refused), and the
  farthest pair at n = 131 072 with the answer in the last row (the largest i n + j of the 35-bit index field) and its tie
  rule across rows.

Every comparison is bit-exact (moves, deltas, paths, integer costs); for real-valued f64 cells the accumulated tour cost is
held within 1e-9 relative, as test_three_opt_nl.test_gpu_move_by_move_with_real_costs does and for its reason.  Every
expectation is computed at test time from the CPU models or holds by construction.  The conditions that keep a case from
passing vacuously (a family's first sweep accepts a move, a 3-opt delta below -2^28, descents that apply 3-opt moves, the
deltas of the constructed matrix) are assertions.

What each defect would trip, read from the code (no broken kernel was run):
- nl_ck(double) without its sign branch orders negative doubles by magnitude, so the lists of the matrices a and b come out
  with their negative entries reversed: check_lists in test_gpu_families_on_signed_costs[a-*] and [b-*];
- ge_wkey without its sign branch (every key folded as a positive double's) orders the negative costs among themselves by
  magnitude, so greedy edge takes -1 before -2 and -3.5 before -40: check_greedy in test_gpu_families_on_signed_costs[a-*] and
  [b-*], whose cheapest edges are the negative ones;
- a delta of k_nl3_sweep narrowed to 28 bits cannot hold -270 619 565 or -281 666 499, accepted by the first and the third
  3-opt sweep of test_gpu_families_at_the_width_edges[i32_top-CEIL_2D-rand_int-*] (and every first 3-opt delta of the three
  i32_top cases is past -2^27);
- Extra Mileage's bias at 2^26 makes -(2^27 - 1) + bias negative, at 2^28 makes 2 (2^27 - 1) + bias need 30 bits: either way
  test_gpu_extra_mileage_at_both_ends_of_the_delta_field gets another insertion order.

Device wall time of the GPU tests of this module on an MI355X: 7.3 s for its 35 GPU tests, the CPU models of the expectations
included (one pytest process; the slowest test 1.3 s, the two farthest-pair runs at n = 131 072 0.5 s together)."""
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
import make_golden_greedy_edge as GE  # noqa: E402
import make_golden_vns_nl as GV  # noqa: E402
import test_extra_mileage as TE  # noqa: E402
import test_greedy_edge as TG  # noqa: E402
import test_gpu_edges as E  # noqa: E402
import test_or_opt as TO  # noqa: E402
import test_or_opt_nl as TON  # noqa: E402
import test_three_opt_nl as T3  # noqa: E402
import test_two_opt_multi as M2  # noqa: E402
import test_two_opt_nl as T2  # noqa: E402
from make_golden_dont_look import all_awake, model_dl_descent  # noqa: E402
from make_golden_or_opt_nl import model_or_sweep  # noqa: E402
from make_golden_three_opt_nl import model_ls3_descent, model_three_sweep  # noqa: E402
from make_golden_two_opt_nl import model_lists, model_sweep  # noqa: E402
from test_two_opt_multi import random_tour, tour_cost  # noqa: E402

K, W = 8, 5
SWEEPS = 3
TOP = (1 << 27) - 1                     # the largest weight int32 cells, matrix-free mode and Extra Mileage take
COUNTERS = ("two_opt_sweeps", "two_opt_moves", "or_sweeps", "or_moves", "rounds", "three_sweeps", "three_moves", "three_phases")
TOTALS = tuple(k for k in COUNTERS if k not in ("rounds", "three_phases"))
OR_OTF = {2: 1, 1: 2}                   # hook 90 -> what tspgpu_info 34 reports (test_or_opt_matrix_free.OR_OTF)

# (regime, kind, instance, scale, elem of the cells, the cost sources)
CASES = [("u16_top", "EUC_2D", "dups", 1, 3, ("cells", "mf")),
         ("i32_bottom", "CEIL_2D", "rand_int", 1, 2, ("cells", "mf")),
         ("ceil_int_top", "CEIL_2D", "lattice", 1, 2, ("mf", "cells")),
         ("ceil_generic", "CEIL_2D", "lattice", 1, 2, ("mf", "cells")),
         ("i32_top", "EUC_2D", "lattice", 1, 2, ("cells", "mf")),
         ("i32_top", "CEIL_2D", "rand_int", 1, 2, ("cells", "mf")),
         ("i32_top", "ATT", "rand_frac", 1, 2, ("cells", "mf")),
         ("f64_bottom", "EUC_2D", "rand_int", 1, 1, ("cells",)),
         ("f64_bottom", "EUC_2D", "rand_int", 8, 1, ("cells",))]
# ceil_int (tspgpu_info 26): CEIL_2D on integer coordinates with cost_bound below 2^22
CEIL_INT = {("i32_bottom", "CEIL_2D"): 1, ("ceil_int_top", "CEIL_2D"): 1}
BATCHED = (0, 5, 8)                     # u16_top, i32_top CEIL_2D, f64_bottom x 8
PAIRS = [(i, s) for i, case in enumerate(CASES) for s in case[5]]


def case_id(i):
    regime, kind, inst, scale = CASES[i][:4]
    return "%s-%s-%s%s" % (regime, kind, inst, "-x%d" % scale if scale != 1 else "")


PAIR_IDS = ["%s-%s" % (case_id(i), s) for i, s in PAIRS]


# ------------------------------------------------------------------------------------------- the instances and the models
@functools.lru_cache(maxsize=None)
def instance(i):
    """-> dict(xy, kind, c: the oracle's matrix, n, nodes: the model's lists, start, cost0)"""
    regime, kind, inst, scale = CASES[i][:4]
    k = getattr(O, kind)
    xy = np.ascontiguousarray(E._edge_instance(inst, k, regime) * float(scale))
    c = O.cost_matrix(xy, k)
    n = len(xy)
    nodes, _ = model_lists(K, costs=c)
    start = random_tour(n, np.random.default_rng(n))
    return {"xy": xy, "kind": k, "c": c, "n": n, "nodes": nodes, "start": start, "cost0": tour_cost(start, costs=c)}


def model_sweeps(c, nodes, start, cost0, count=SWEEPS):
    """the first `count` sweeps of every family from `start` -> {family: [(moves, deltas, path, cost)]}; Or-opt: moves is the
    one (s, L, q, rev) (or the empty list), deltas the one delta"""
    fams = {"multi": lambda p, cost: M2.model_sweep(p, cost, costs=c),
            "nl2": lambda p, cost: model_sweep(p, cost, nodes, costs=c),
            "ornl": lambda p, cost: model_or_sweep(p, cost, nodes, costs=c),
            "nl3": lambda p, cost: model_three_sweep(p, cost, nodes, W, costs=c)}
    out = {}
    for name, sweep in fams.items():
        p, cost, rows = start.copy(), cost0, []
        for _ in range(count):
            r = sweep(p, cost)
            cost = r["cost"]
            rows.append((np.array(r["moves"]), np.array(r["deltas"], np.float64), p.copy(), cost))
        out[name] = rows
    p, cost, rows = start.copy(), cost0, []
    for _ in range(count):
        mv = TO.best_move(c, p)
        if mv[0] < TO.EPS:
            TO.apply_move(p, *mv[1:])
            cost += mv[0]
            rows.append((mv[1:], mv[0], p.copy(), cost))
        else:
            rows.append(((-1, -1, -1, -1), 0.0, p.copy(), cost))
    out["or"] = rows
    return out


@functools.lru_cache(maxsize=None)
def case_sweeps(i):
    I = instance(i)
    s = model_sweeps(I["c"], I["nodes"], I["start"], I["cost0"])
    for fam, rows in s.items():                     # each family's first sweep accepts a move, in every case
        assert (rows[0][1] < 0.0 if fam == "or" else len(rows[0][0]) >= 1), (case_id(i), fam)
    return s


@functools.lru_cache(maxsize=None)
def case_descent(i):
    I = instance(i)
    p = I["start"].copy()
    r = model_ls3_descent(p, I["nodes"], W, costs=I["c"], limit_sweeps=100 * I["n"])
    assert O.valid_tour(p) and r["cost"] == O.tour_cost(I["c"], p)
    return p, r


def greedy_of(nodes, c):
    """the sequential rule's tour and the parallel form's counters (test_greedy_edge: the two give the same tour)"""
    want = GE.model_rounds(nodes, costs=c)
    seq = GE.model_greedy(nodes, costs=c)
    assert np.array_equal(want["path"], seq["path"]) and want["cost"] == seq["cost"]
    assert (want["edges1"], want["free"]) == (seq["edges1"], seq["free"])
    return want


@functools.lru_cache(maxsize=None)
def case_greedy(i):
    I = instance(i)
    return greedy_of(I["nodes"], I["c"])


@functools.lru_cache(maxsize=None)
def case_em(i):
    I = instance(i)
    a, b = TE.farthest_pair(I["c"])
    succ, cost, _ = TE.em_model(I["c"], a, b)
    assert O.valid_tour(succ) and cost == O.tour_cost(I["c"], succ)
    return a, b, succ, cost


@functools.lru_cache(maxsize=None)
def case_batched(i):
    """-> dict(nn: the NN tours of the starts 0 .. 3, ls3 / dl: the model's descent of each, walks: two model walks)"""
    I = instance(i)
    c, nodes, n = I["c"], I["nodes"], I["n"]
    nn = [O.nn_tour(c, s) for s in range(4)]
    ls3, dl = [], []
    for path, cost in nn:
        p = path.copy()
        ls3.append((p, model_ls3_descent(p, nodes, W, costs=c)))
        p = path.copy()
        dl.append((p, model_dl_descent(p, cost, all_awake(n), nodes, W, 1, costs=c)))
    starts = [nn[0][0], nn[1][0]]
    cost0 = [nn[0][1], nn[1][1]]
    walks = [GV.model_walk(starts[w], cost0[w], nodes, 3, 1 + w, kick=O.vns_kick,
                           descent=lambda path, nodes, **src: model_ls3_descent(path, nodes, W, **src), costs=c) for w in range(2)]
    return {"nn": nn, "ls3": ls3, "dl": dl, "starts": starts, "cost0": cost0, "walks": walks}


# --------------------------------------------------------------------------------------------------- signed caller matrices
SIGNED_N = (9, 18, 40, 64)
SIGNED = [(v, n) for v in "abc" for n in SIGNED_N]


@functools.lru_cache(maxsize=None)
def signed_matrix(variant, n):
    """symmetric, diagonal -1.  a: real values uniform in (-50, 50); b: integers in -2 .. 2, every zero +0.0 or -0.0 at random;
    c: integers in [0, 60 000], about one off-diagonal cell in ten -1"""
    rng = np.random.default_rng(1000 * n + ord(variant))
    if variant == "a":
        a = rng.uniform(-50.0, 50.0, (n, n))
    elif variant == "b":
        a = rng.integers(-2, 3, (n, n)).astype(np.float64)
    else:
        a = rng.integers(0, 60001, (n, n)).astype(np.float64)
        a = np.where(rng.random((n, n)) < 0.1, -1.0, a)
    a = np.triu(a, 1)
    a = a + a.T
    if variant == "b":
        neg = np.triu(rng.random((n, n)) < 0.5, 1)
        a[(neg | neg.T) & (a == 0)] = -0.0
    np.fill_diagonal(a, -1.0)
    assert np.array_equal(a, a.T) and np.array_equal(np.signbit(a), np.signbit(a.T))
    return np.ascontiguousarray(a)


@functools.lru_cache(maxsize=None)
def signed_case(variant, n):
    c = signed_matrix(variant, n)
    nodes, w = model_lists(K, costs=c)
    start = random_tour(n, np.random.default_rng(n + ord(variant)))
    cost0 = tour_cost(start, costs=c)
    sweeps = model_sweeps(c, nodes, start, cost0)
    p = start.copy()
    r = model_ls3_descent(p, nodes, W, costs=c, limit_sweeps=100 * n)
    return {"c": c, "n": n, "nodes": nodes, "w": w, "start": start, "cost0": cost0, "sweeps": sweeps, "descent": (p, r),
            "greedy": greedy_of(nodes, c)}


def test_signed_matrices_have_the_signs_they_are_for():
    for n in SIGNED_N:
        a, b, c = (signed_matrix(v, n) for v in "abc")
        off = ~np.eye(n, dtype=bool)
        assert (a[off] < 0).any() and (a[off] > 0).any() and (a != np.trunc(a))[off].all()
        assert b[off].min() == -2.0 and b[off].max() == 2.0 and (b == np.trunc(b)).all()
        zeros = off & (b == 0)
        assert np.signbit(b[zeros]).any() and not np.signbit(b[zeros]).all()               # zeros of both signs
        assert c[off].min() == -1.0 and c[off].max() > 32767.0 and (c == np.trunc(c)).all() and (c[off] == -1.0).sum() >= 2


@pytest.mark.parametrize("variant", "abc")
def test_models_equal_the_restatements_on_signed_matrices(variant):
    """the C models on negative costs against the plain-Python restatements written from the rules: the lists and their weights,
    greedy edge (sequential rule and parallel rounds), every sweep of the first three of each family: parallel-move 2-opt,
    neighbour-list 2-opt, Or-opt and 3-opt, plain Or-opt"""
    accepted = {"multi": 0, "nl2": 0, "ornl": 0, "nl3": 0, "or": 0}
    for n in (9, 18, 40):
        S = signed_case(variant, n)
        c, nodes, start = S["c"], S["nodes"], S["start"]
        cl, lists = c.tolist(), nodes.tolist()
        assert lists == T2.brute_lists(cl, K), (variant, n)
        assert all(S["w"][v][j] == cl[v][u] for v in range(n) for j, u in enumerate(lists[v]))
        py = TG.py_greedy(cl, lists)
        assert np.array_equal(S["greedy"]["path"], py["path"]) and (S["greedy"]["edges1"], S["greedy"]["free"]) == (py["edges1"], py["free"])
        rounds = TG.py_rounds(cl, lists)
        assert (S["greedy"]["rounds1"], S["greedy"]["rounds2"]) == (rounds["rounds1"], rounds["rounds2"])
        brutes = {"multi": lambda p: M2.brute_sweep(cl, p), "nl2": lambda p: T2.brute_sweep(cl, p, lists),
                  "ornl": lambda p: TON.brute_sweep(cl, p, lists), "nl3": lambda p: T3.brute_sweep(cl, p, lists, W)}
        for fam, brute in brutes.items():
            p = start.copy()
            for t, (moves, deltas, path, _) in enumerate(S["sweeps"][fam]):
                want = brute(p)
                assert [tuple(int(v) for v in mv) for mv in moves] == [tuple(mv) for mv in want["moves"]], (variant, n, fam, t)
                assert [float(d) for d in deltas] == [float(d) for d in want["deltas"]], (variant, n, fam, t)
                assert [int(v) for v in path] == want["path"], (variant, n, fam, t)
                p = path.copy()
                accepted[fam] += len(moves)
        p = start.copy()
        for t, (mv, d, path, _) in enumerate(S["sweeps"]["or"]):
            want = TO.or_opt_best_move_plain(c, p)
            if want[0] < TO.EPS:
                assert (d, *mv) == tuple(want), (variant, n, t)
                accepted["or"] += 1
            else:
                assert d == 0.0 and mv == (-1, -1, -1, -1), (variant, n, t)
            p = path.copy()
    assert all(v >= 3 for v in accepted.values()), accepted


def test_models_accept_moves_at_every_edge_of_the_range():
    """the conditions the GPU cases rest on, on the CPU: every family's first model sweep accepts a move in every case of the
    table (asserted in case_sweeps); over the i32_top cases an accepted 3-opt delta lies below -2^28; at least four descents of
    the table apply a 3-opt move"""
    deepest = 0.0
    for i, case in enumerate(CASES):
        s = case_sweeps(i)
        if case[0] == "i32_top":
            assert instance(i)["c"].max() > 0.99 * TOP
            deepest = min([deepest] + [float(d) for _, deltas, _, _ in s["nl3"] for d in deltas])
    assert deepest < -float(1 << 28), deepest
    assert sum(case_descent(i)[1]["three_moves"] >= 1 for i in range(len(CASES))) >= 4
    top = instance(8)["c"].max()
    assert top > float(1 << 29) and 3.0 * top > float(1 << 31)          # f64_bottom x 8: sums of three past 2^31


# ------------------------------------------------------------------------------------------------------------ GPU helpers
def open_engine(i, source):
    """an engine on case i through `source`; asserts the storage, the mode and the CEIL_2D form before anything runs"""
    import travellingsalesmanoptimization_amd as T
    regime, kind, _, _, elem, _ = CASES[i]
    I = instance(i)
    eng = T.Engine(0)
    eng.set_option(T.OPT_ELEM, 0)
    eng.set_option(T.OPT_MATRIX_FREE, 1 if source == "mf" else 2)
    eng.set_points(I["xy"], I["kind"])
    eng.build_costs()
    info = eng.info()
    want = (2 if source == "mf" else elem, 1 if source == "mf" else 0, CEIL_INT.get((regime, kind), 0))
    assert (info["elem"], info["matrix_free"], info["ceil_int"]) == want, (case_id(i), source, info["elem"], info["matrix_free"], info["ceil_int"])
    return eng


def same_cost(got, want, exact):
    return got == want if exact else abs(got - want) <= 1e-9 * abs(want)


def check_lists(eng, c, nodes, what):
    eng.neighbours_build(K)
    got, w = eng.neighbours_get()
    assert eng.info()["nl_k"] == nodes.shape[1] == min(K, len(c) - 1), what
    assert np.array_equal(got, nodes), what
    want_w = c[np.arange(len(c))[:, None], nodes]
    assert np.array_equal(w, want_w), what
    return w


def check_sweeps(eng, start, cost0, sweeps, what, exact=True):
    """the first sweeps of the four parallel-move families against the model: the move lists in order, the deltas, the path,
    the cost"""
    calls = {"multi": lambda p, cost: eng.two_opt_multi_once(p, cost), "nl2": lambda p, cost: eng.two_opt_nl_once(p, cost),
             "ornl": lambda p, cost: eng.or_opt_nl_once(p, cost), "nl3": lambda p, cost: eng.three_opt_nl_once(p, cost, W)}
    for fam, once in calls.items():
        path, cost = start.copy(), cost0
        for t, (moves, deltas, want_path, want_cost) in enumerate(sweeps[fam]):
            cost, mv, dl = once(path, cost)
            assert len(mv) == len(moves) and np.array_equal(mv, np.asarray(moves).reshape(mv.shape)), (what, fam, t, mv[:4], moves[:4])
            assert np.array_equal(dl, deltas), (what, fam, t, dl[:4], deltas[:4])
            assert np.array_equal(path, want_path), (what, fam, t)
            assert same_cost(cost, want_cost, exact), (what, fam, t, cost, want_cost)


def check_or_opt(eng, start, cost0, rows, what, exact=True):
    path, cost = start.copy(), cost0
    for t, (mv, d, want_path, want_cost) in enumerate(rows):
        gd, cost, gmv = eng.or_opt_once(path, cost)
        assert (gd, gmv) == (d, tuple(mv)), (what, "or", t, gd, gmv, d, mv)
        assert np.array_equal(path, want_path) and same_cost(cost, want_cost, exact), (what, "or", t, cost, want_cost)


def check_descent(eng, start, want, what, exact=True):
    """local_search_nl3 on a host tour and on a slot: every counter, the cost, the path"""
    want_path, r = want
    path = start.copy()
    got = eng.local_search_nl3(path, W)
    assert got["rc"] == 0 and {k: got[k] for k in COUNTERS} == {k: r[k] for k in COUNTERS}, (what, got, r)
    assert np.array_equal(path, want_path) and same_cost(got["cost"], r["cost"], exact), (what, got["cost"], r["cost"])
    info = eng.info()
    assert (info["three_nl_sweeps"], info["three_nl_moves"], info["three_nl_phases"]) == (r["three_sweeps"], r["three_moves"], r["three_phases"]), what
    assert (info["or_nl_sweeps"], info["or_nl_moves"], info["or_nl_rounds"]) == (r["or_sweeps"], r["or_moves"], r["rounds"]), what
    eng.tour_load(1, start)
    got1 = eng.tour_local_search_nl3(1, W)
    spath, scost, _ = eng.tour_store(1)
    assert got1["rc"] == 0 and {k: got1[k] for k in COUNTERS} == {k: r[k] for k in COUNTERS}, (what, got1, r)
    assert np.array_equal(spath, want_path) and same_cost(scost, r["cost"], exact), (what, scost, r["cost"])


def check_greedy(eng, want, what):
    path, cost = eng.greedy_tour()
    assert np.array_equal(path, want["path"]) and cost == want["cost"], (what, cost, want["cost"])
    TG.check_counters(eng, want, what)


def refused_by_extra_mileage(eng, what):
    import travellingsalesmanoptimization_amd as T
    for call in (eng.farthest_pair, lambda: eng.extra_mileage(0, 1)):
        with pytest.raises(T.TspGpuError) as ei:
            call()
        assert ei.value.code == 9 and "2^27" in str(ei.value), (what, ei.value)


def check_extra_mileage(eng, want, n, what):
    """the default form, then form 1 (the one-launch form) as test_extra_mileage.test_gpu_pr1002_matrix_free_and_forms"""
    import travellingsalesmanoptimization_amd as T
    a, b, succ, cost = want
    for form in (0, 1):
        eng.set_option(T.OPT_EM_FORM, form)
        ga, gb, gc = eng.farthest_pair()
        assert (ga, gb) == (a, b), (what, form, ga, gb, a, b)
        got, gcost, rc = eng.extra_mileage()
        assert rc == 0 and gcost == cost and np.array_equal(got, succ), (what, form, gcost, cost)
        info = eng.info()
        assert (info["em_form"] == 1 if form else info["em_form"] in (1, 2)) and info["em_steps"] == n - 2, (what, form, info["em_form"])
    eng.set_option(T.OPT_EM_FORM, 0)


# -------------------------------------------------------------------------------------------------------------- GPU: the table
@pytest.mark.gpu
@pytest.mark.parametrize("i,source", PAIRS, ids=PAIR_IDS)
def test_gpu_families_at_the_width_edges(i, source):
    """one case of the table through one cost source, on one engine: lists, sweeps, descent, greedy edge, Extra Mileage"""
    import travellingsalesmanoptimization_amd as T
    I = instance(i)
    c, n, start, cost0 = I["c"], I["n"], I["start"], I["cost0"]
    sweeps = case_sweeps(i)
    what = (case_id(i), source)
    eng = open_engine(i, source)
    check_lists(eng, c, I["nodes"], what)
    check_sweeps(eng, start, cost0, sweeps, what)
    if source == "mf":
        eng.set_option(T._lib.OPT_OR_MATRIX_FREE, 1)
        for form in (2, 1):                         # every candidate evaluated; the exact early-out
            eng.set_option(90, form)
            check_or_opt(eng, start, cost0, sweeps["or"], what + (form,))
            info = eng.info()
            assert info["matrix_free"] == 1 and info["or_otf"] == OR_OTF[form], (what, form, info["or_otf"])
        eng.set_option(90, 0)
    else:
        check_or_opt(eng, start, cost0, sweeps["or"], what)
    check_descent(eng, start, case_descent(i), what)
    check_greedy(eng, case_greedy(i), what)
    if CASES[i][4] == 1:
        refused_by_extra_mileage(eng, what)
    else:
        check_extra_mileage(eng, case_em(i), n, what)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("i,source", [p for p in PAIRS if p[0] in BATCHED], ids=[d for p, d in zip(PAIRS, PAIR_IDS) if p[0] in BATCHED])
def test_gpu_batched_forms_at_the_width_edges(i, source):
    """the multi-start over the starts 0 .. 3 (the model's descent of each NN tour), the multi-start with looks (closing 1,
    every start all awake) and two VNS walks of three iterations on the glibc stream"""
    import test_nl3_batch as B3
    I = instance(i)
    c, n, nodes = I["c"], I["n"], I["nodes"]
    want = case_batched(i)
    what = (case_id(i), source)
    eng = open_engine(i, source)
    eng.neighbours_build(K)
    starts = [0, 1, 2, 3]
    for s, (path, cost) in enumerate(want["nn"]):
        got, gcost = eng.nn_tour(s)
        assert gcost == cost and np.array_equal(got, path), (what, s)
    for name, run, keys in (("ls3", lambda: eng.multistart_local_search_nl3(W, starts), TOTALS),
                            ("dl", lambda: eng.multistart_local_search_nl3_dl(W, 1, starts), TOTALS + ("looked", "full_sweeps"))):
        rows = want[name]
        costs = [r["cost"] for _, r in rows]
        win = costs.index(min(costs))
        r = run()
        assert r["rc"] == 0 and list(r["costs"]) == costs, (what, name, list(r["costs"]), costs)
        assert (r["start"], r["cost"]) == (starts[win], costs[win]) and np.array_equal(r["path"], rows[win][0]), (what, name)
        assert {k: r[k] for k in keys} == {k: sum(m[k] for _, m in rows) for k in keys}, (what, name)
    k = 3
    rvs = [GV.libc_draws(1 + w, GV.draws_for(k)) for w in range(2)]
    r, paths, bests = B3.run_walks3(eng, want["starts"], want["cost0"], rvs, k, W)
    assert r["rc"] == 0
    for w in range(2):
        B3.check_walk(r, paths, bests, w, want["walks"][w], tour_cost(want["walks"][w]["path"], costs=c), k, what + (w,))
    eng.close()


# ------------------------------------------------------------------------------------------------------- GPU: signed costs
@pytest.mark.gpu
@pytest.mark.parametrize("variant,n", SIGNED, ids=["%s-n%d" % s for s in SIGNED])
def test_gpu_families_on_signed_costs(variant, n):
    import travellingsalesmanoptimization_amd as T
    S = signed_case(variant, n)
    c, start, cost0 = S["c"], S["start"], S["cost0"]
    exact = variant != "a"
    what = (variant, n)
    eng = T.Engine(0)
    eng.set_option(T.OPT_ELEM, 0)
    eng.set_costs(c)
    info = eng.info()
    assert (info["elem"], info["matrix_free"], info["ceil_int"], info["symmetric"]) == (2 if variant == "c" else 1, 0, 0, 1), (what, info["elem"])
    w = check_lists(eng, c, S["nodes"], what)
    if variant == "b" and n <= 18:                  # (K' = 8 of at most 17: the lists reach the zeros; at n >= 40 they hold -2 and -1 alone)
        cells = c[np.arange(n)[:, None], S["nodes"]]
        zeros = cells == 0
        assert np.signbit(cells[zeros]).any() and not np.signbit(cells[zeros]).all()       # zeros of both signs, ordered by node
        assert (w[zeros] == 0).all()
    check_sweeps(eng, start, cost0, S["sweeps"], what, exact)
    check_or_opt(eng, start, cost0, S["sweeps"]["or"], what, exact)
    check_descent(eng, start, S["descent"], what, exact)
    check_greedy(eng, S["greedy"], what)
    refused_by_extra_mileage(eng, what)
    eng.close()


# ------------------------------------------------------------------------------------------ Extra Mileage: the key fields
def em_trace(c, a, b):
    """h_extramileage_util restated with full rescans (no incremental state): every step the first strict minimum of
    c[u][i] + c[i][v] - c[u][v] over the nodes outside ascending, then the edges in array order; the split edge becomes (u, i)
    in place and (i, v) is appended -> (succ, cost, the inserted deltas, per step the largest best delta among the nodes outside)"""
    n = len(c)
    ci = c.astype(np.int64)
    eu, ev = [a, b], [b, a]
    succ = np.full(n, -1, np.int32)
    succ[a], succ[b] = b, a
    outside = [v for v in range(n) if v not in (a, b)]
    deltas, waiting = [], []
    while outside:
        D = ci[np.array(eu)[None, :], np.array(outside)[:, None]] + ci[np.array(outside)[:, None], np.array(ev)[None, :]] \
            - ci[np.array(eu), np.array(ev)][None, :]
        best = D.min(axis=1)
        waiting.append(int(best.max()))
        r = int(np.argmin(best))                    # the first minimum: the lowest node
        j = int(np.argmin(D[r]))                    # the first minimum: the lowest edge index
        x, u, v = outside.pop(r), eu[j], ev[j]
        deltas.append(int(D[r, j]))
        ev[j] = x
        eu.append(x)
        ev.append(v)
        succ[u], succ[x] = x, v
    return succ, 2.0 * float(c[a, b]) + float(sum(deltas)), deltas, waiting


@functools.lru_cache(maxsize=None)
def em_field_matrix(n=56):
    """integers in [0, 2^27): the nodes 0 and 1 at 2^27 - 1 from each other (the farthest pair: ahead of every other pair of
    that cost in row-major order), the nodes 2 and 3 at 0 from both -- node 2 goes into the edge (0, 1) and node 3 into (1, 0),
    each with delta -(2^27 - 1), and leave a tour of four edges of cost 0 --, node n - 1 at 2^27 - 1 from everything -- its
    best delta is 2 (2^27 - 1) - the largest edge cost of the tour: 2 (2^27 - 1) on that tour, and never below 2^27 - 1, above
    every other node's, so it goes in last --, every other cell random in [1, 2^26)"""
    rng = np.random.default_rng(n)
    c = np.triu(rng.integers(1, 1 << 26, (n, n)).astype(np.float64), 1)
    c = c + c.T
    c[0, 1] = c[1, 0] = float(TOP)
    for v in (2, 3):
        c[0, v] = c[v, 0] = c[1, v] = c[v, 1] = 0.0
    c[n - 1, :] = c[:, n - 1] = float(TOP)
    np.fill_diagonal(c, -1.0)
    return np.ascontiguousarray(c)


def test_extra_mileage_field_matrix_reaches_both_ends_of_the_delta_field():
    """on the model, by replaying its insertion order with a restatement of the rule: the farthest pair is (0, 1), the sequence
    holds a delta of exactly -(2^27 - 1), and a node outside stands at a best delta of 2 (2^27 - 1) for at least one step --
    the two ends of the documented (-2^27, 2^28)"""
    c = em_field_matrix()
    n = len(c)
    assert 48 <= n <= 64 and c.max() == TOP and c[~np.eye(n, dtype=bool)].min() == 0.0
    assert TE.farthest_pair(c) == (0, 1)
    succ, cost, _ = TE.em_model(c, 0, 1)
    rsucc, rcost, deltas, waiting = em_trace(c, 0, 1)
    assert np.array_equal(succ, rsucc) and cost == rcost == O.tour_cost(c, succ) and O.valid_tour(succ)
    assert deltas[:2] == [-TOP, -TOP] and min(deltas) == -TOP > -(1 << 27)
    assert max(waiting) == waiting[2] == 2 * TOP < (1 << 28)
    assert int(succ[n - 1]) >= 0 and deltas[-1] >= TOP          # the node at 2^27 - 1 from everything went in last


@pytest.mark.gpu
def test_gpu_extra_mileage_at_both_ends_of_the_delta_field():
    import travellingsalesmanoptimization_amd as T
    c = em_field_matrix()
    n = len(c)
    succ, cost, _ = TE.em_model(c, 0, 1)
    eng = T.Engine(0)
    eng.set_costs(c)
    info = eng.info()
    assert (info["elem"], info["matrix_free"], info["ceil_int"]) == (2, 0, 0)
    check_extra_mileage(eng, (0, 1, succ, cost), n, "field")
    assert eng.farthest_pair() == (0, 1, float(TOP))
    over = c.copy()                                 # one cell at 2^27: refused, whatever cells hold it
    over[5, 6] = over[6, 5] = float(1 << 27)
    eng.set_costs(over)
    refused_by_extra_mileage(eng, "field + 2^27")
    eng.close()


def far_points(n, copy_at=None):
    """integer points in [0, 1000]^2, point n - 2 at (-10^6, -10^6) and point n - 1 at (10^6 + 1000, 10^6 + 1000): the two are
    farther from each other than any other pair by construction; copy_at: that point is a copy of point n - 1"""
    rng = np.random.default_rng(n)
    xy = rng.integers(0, 1001, (n, 2)).astype(np.float64)
    xy[n - 2] = (-1.0e6, -1.0e6)
    xy[n - 1] = (1.0e6 + 1000.0, 1.0e6 + 1000.0)
    if copy_at is not None:
        xy[copy_at] = xy[n - 1]
    return np.ascontiguousarray(xy)


@pytest.mark.gpu
def test_gpu_farthest_pair_at_the_top_of_the_index_field():
    """n = 131 072 in the automatic mode (matrix-free there): the answer (n - 2, n - 1) is the largest i n + j the key can
    hold; with a copy of point n - 1 at index 5 two pairs tie and the first in row-major order, (5, n - 2), wins"""
    import travellingsalesmanoptimization_amd as T
    n = 131072
    eng = T.Engine(0)
    for copy_at, want in ((None, (n - 2, n - 1)), (5, (5, n - 2))):
        xy = far_points(n, copy_at)
        eng.set_points(xy)
        eng.build_costs()
        info = eng.info()
        assert (info["n"], info["matrix_free"]) == (n, 1)
        a, b, cost = eng.farthest_pair()
        w = O.cost_matrix(np.ascontiguousarray(xy[[n - 2, n - 1]]))[0, 1]
        assert (a, b, cost) == (want[0], want[1], w), (copy_at, a, b, cost, w)
        assert (n - 2) * n + (n - 1) == (1 << 34) - n - 1 and w > 2.0e6
    eng.close()
