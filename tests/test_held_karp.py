"""Held-Karp lower bound: 1-trees in Boruvka rounds and the subgradient ascent (include/tspgpu.h "Held-Karp lower bound").

The model is tests/held_karp_model.c (wrappers in tools/make_golden_held_karp.py): Prim under the key order, and rule 3 literally.
CPU: the model's tree against a Python Kruskal written from rule 2 and against a Python statement of rule 4's rounds (random
matrices, all ties, the lattice, two clusters, with and without multipliers), rule 3 restated in Python against the model on
berlin52 and kroA100, the golden against the optima and against L(0), berlin52's tour, reason 5, the header, the symbols and
the null-handle code.
GPU: one_tree bit-equal with the model in every integral cell type and weight form at the sizes around a wave, a workgroup's
rows and a vector, the tie cases, the ascent against the golden, continuation, fnl4461 / pla85900 trees against the golden,
refusals, reasons 2 and 5, the deadline, memory across instances, the host binary's TSP_LOWER_BOUND.
tests/test_held_karp_limits.py goes on from here with the helpers of this file: the scans that read comp[] and pi[] through L2
(n > 5440), weights that need 64 bits, one hook chain of n - 3, reason 3, other batch sizes."""
import json
import math
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
import make_golden_held_karp as G  # noqa: E402
from make_golden_held_karp import S, bound_of, digest64, fixed_pi, model_ascent, model_one_tree, tsplib_instance  # noqa: E402
from make_golden_two_opt_nl import digest  # noqa: E402
from test_two_opt_multi import engine_for, points_for, sym_int_matrix  # noqa: E402
from test_or_opt_nl import rect_lattice, run_tsp  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_held_karp.json")
DATA = os.path.join(ROOT, "tests", "golden", "data")
NEW_SYMBOLS = ["tspgpu_one_tree", "tspgpu_lower_bound"]
OPTIMA = {"berlin52": 7542, "kroA100": 21282, "eil51": 426, "att48": 10628, "pr1002": 259045}
PI_MAX = 1 << 45


def golden():
    return json.load(open(GOLDEN))


# ---------------------------------------------------------------------------------------------- the rule, restated in Python
def ints(c):
    return [[int(x) for x in row] for row in np.asarray(c)]


def weight(c, pi, a, b):
    return S * c[a][b] + pi[a] + pi[b]


class Sets:
    def __init__(self, n):
        self.up = list(range(n))

    def root(self, v):
        while self.up[v] != v:
            self.up[v] = self.up[self.up[v]]
            v = self.up[v]
        return v


def zero_edges(c, pi):
    return sorted((weight(c, pi, 0, u), 0, u) for u in range(1, len(c)))[:2]


def finish(n, pi, keys):
    deg = [0] * n
    for _, a, b in keys:
        deg[a] += 1
        deg[b] += 1
    return {"L": sum(k[0] for k in keys) - 2 * sum(pi), "edges": sorted((a, b) for _, a, b in keys), "deg": deg}


def py_tree(c, pi=None):
    """rule 2 by Kruskal: all pairs of the nodes 1 .. n - 1 sorted by key, union-find; then node 0's two smallest keys"""
    n = len(c)
    pi = [0] * n if pi is None else [int(x) for x in pi]
    sets, keys = Sets(n), []
    for w, a, b in sorted((weight(c, pi, a, b), a, b) for a in range(1, n) for b in range(a + 1, n)):
        ra, rb = sets.root(a), sets.root(b)
        if ra != rb:
            sets.up[ra] = rb
            keys.append((w, a, b))
    assert len(keys) == n - 2
    return finish(n, pi, keys + zero_edges(c, pi))


def py_rounds(c, pi=None):
    """rule 4: every node's smallest key into another component, every component's smallest, accept, merge -> tree and rounds"""
    n = len(c)
    pi = [0] * n if pi is None else [int(x) for x in pi]
    comp, keys, rounds = list(range(n)), [], 0
    while len(keys) < n - 2:
        best = {}
        for v in range(1, n):
            cand = [(weight(c, pi, min(v, u), max(v, u)), min(v, u), max(v, u)) for u in range(1, n) if comp[u] != comp[v]]
            k = min(cand)
            if comp[v] not in best or k < best[comp[v]]:
                best[comp[v]] = k
        take = sorted(set(best.values()))
        sets = Sets(n)
        for _, a, b in take:
            ra, rb = sets.root(comp[a]), sets.root(comp[b])
            assert ra != rb, "an accepted edge closed a cycle"
            sets.up[ra] = rb
        comp = [sets.root(x) for x in comp]
        keys += take
        rounds += 1
    out = finish(n, pi, keys + zero_edges(c, pi))
    out["rounds"] = rounds
    return out


def py_ascent(c, upper, iters, patience, pi=None):
    """rule 3, literally"""
    n = len(c)
    pi = [0] * n if pi is None else [int(x) for x in pi]
    h = bad = it = reason = 0
    best, star, tree = None, None, None
    while it < iters:
        tree = py_tree(c, pi)
        L = tree["L"]
        if best is None or L > best:
            best, star, bad = L, list(pi), 0
        else:
            bad += 1
            if bad >= patience:
                h, bad = h + 1, 0
        it += 1
        g = [d - 2 for d in tree["deg"]]
        q = sum(x * x for x in g)
        if q == 0:
            reason = 1
            break
        gap = S * upper - L
        if gap <= 0:
            reason = 2
            break
        t = ((2 * gap) >> h) // q
        if t == 0:
            reason = 3
            break
        if any(abs(p + t * x) > PI_MAX for p, x in zip(pi, g)):
            reason = 5
            break
        pi = [p + t * x for p, x in zip(pi, g)]
    return {"bound": -((-best) // S), "best": best, "reason": reason, "iters": it, "h": h, "pi": np.array(star, np.int64), "tree": tree}


def clusters(n, seed):
    """two far-apart clusters of integer points"""
    rng = np.random.default_rng(seed)
    xy = rng.integers(0, 30, (n, 2)).astype(np.float64)
    xy[n // 2:] += 20000.0
    return xy


def tie_cases():
    ones = np.ones((12, 12))
    np.fill_diagonal(ones, -1.0)
    yield "ones12", ones
    yield "lattice15", O.cost_matrix(rect_lattice(5, 3))
    yield "lattice40", O.cost_matrix(rect_lattice(8, 5))
    yield "clusters14", O.cost_matrix(clusters(14, 3))


def small_cases():
    rng = np.random.default_rng(424)
    for n in (5, 6, 9, 33, 100):
        yield "matrix%d" % n, sym_int_matrix(n, rng)
    yield from tie_cases()


def random_pi(n, rng):
    return rng.integers(-(1 << 20), (1 << 20) + 1, n).astype(np.int64)


def same_tree(got, want, what):
    assert int(got["L"]) == want["L"], what
    assert [tuple(int(x) for x in e) for e in got["edges"]] == want["edges"], what
    assert [int(d) for d in got["deg"]] == want["deg"], what


def tour_of(path):
    assert O.valid_tour(path)
    return path


# ------------------------------------------------------------------------------------------------------------ CPU tests
def test_model_tree_equals_the_python_kruskal():
    """the model's Prim against Kruskal from rule 2: L, the edge list ascending by pair, the degrees; pi = 0 and random pi in
    +-2^20, which makes weights negative (128 c <= 128 000)"""
    rng = np.random.default_rng(7)
    for name, c in small_cases():
        n = len(c)
        for pi in (None, random_pi(n, rng), random_pi(n, rng)):
            got, want = model_one_tree(costs=c, pi=pi), py_tree(ints(c), pi)
            same_tree(got, want, name)
            assert want["deg"][0] == 2 and sum(want["deg"]) == 2 * n and len(set(want["edges"])) == n, name
        if pi is not None:
            assert min(weight(ints(c), [int(x) for x in pi], a, b) for a in range(n) for b in range(a + 1, n)) < 0, name


def test_rounds_give_the_tree_of_rule_2():
    """rule 4 stated in Python: the same edge set as the model, within ceil(log2(n - 1)) rounds"""
    rng = np.random.default_rng(8)
    for name, c in small_cases():
        n = len(c)
        for pi in (None, random_pi(n, rng)):
            want = py_rounds(ints(c), pi)
            same_tree(model_one_tree(costs=c, pi=pi), want, name)
            assert 1 <= want["rounds"] <= max(1, math.ceil(math.log2(n - 1))), name


@pytest.mark.parametrize("name", ["berlin52", "kroA100"])
def test_ascent_equals_the_python_restatement(name):
    g = golden()["ascent"][name]
    xy, kind = tsplib_instance(name)
    want = py_ascent(ints(O.cost_matrix(xy, kind)), g["upper"], g["iters_asked"], g["patience"])
    got = model_ascent(g["upper"], xy=xy, kind=kind)
    for k in ("bound", "best", "reason", "iters", "h"):
        assert got[k] == want[k] == g[k], k
    assert np.array_equal(got["pi"], want["pi"]) and digest64(got["pi"]) == g["pi_sha256"]


def test_golden_is_the_model_and_a_lower_bound():
    """every committed instance: the golden is what the model gives now (pr1002 included: 1.6 s), bound <= optimum, and the ascent
    does not end below where it starts, ceil(L(0) / S)"""
    g = golden()["ascent"]
    assert sorted(g) == sorted(OPTIMA)
    for name, e in g.items():
        assert e["optimum"] == OPTIMA[name] and e["bound"] <= OPTIMA[name], name
        assert e["bound"] >= bound_of(e["L0"]) and e["bound"] == bound_of(e["best"]), name
        xy, kind = tsplib_instance(name)
        got = model_ascent(e["upper"], e["iters_asked"], e["patience"], xy=xy, kind=kind)
        assert (got["bound"], got["best"], got["reason"], got["iters"], got["h"]) == (e["bound"], e["best"], e["reason"], e["iters"], e["h"]), name
        assert digest64(got["pi"]) == e["pi_sha256"], name
        assert model_one_tree(xy=xy, kind=kind)["L"] == e["L0"], name


def test_berlin52_ends_with_the_optimal_tour():
    g = golden()["ascent"]["berlin52"]
    xy, kind = tsplib_instance("berlin52")
    got = model_ascent(8980, xy=xy, kind=kind)
    assert got["reason"] == 1 and got["bound"] == 7542
    path = tour_of(got["path"])
    c = O.cost_matrix(xy, kind)
    assert sum(c[i][int(path[i])] for i in range(52)) == 7542.0 == g["tour_cost"]
    assert path[0] < int(np.flatnonzero(path == 0)[0]) and digest(path) == g["path_sha256"]


def test_reason_5_in_the_model():
    """multipliers all at 2^45 - 10 give the tree of pi = 0; its nodes of degree >= 3 would pass 2^45: reason 5 in the first
    iteration, nothing applied, and the Python restatement says the same"""
    rng = np.random.default_rng(55)
    c = sym_int_matrix(33, rng)
    pi = np.full(33, PI_MAX - 10, np.int64)
    got, want = model_ascent(30000, 20, 3, costs=c, pi=pi), py_ascent(ints(c), 30000, 20, 3, pi)
    assert got["reason"] == want["reason"] == 5 and got["iters"] == want["iters"] == 1
    assert np.array_equal(got["pi"], pi) and got["best"] == want["best"] == model_one_tree(costs=c)["L"]


def test_header_section_and_exported_symbols():
    from travellingsalesmanoptimization_amd import _lib
    text = open(os.path.join(ROOT, "include", "tspgpu.h")).read()
    assert "Held-Karp lower bound" in text and "S = 128" in text and "Boruvka rounds" in text
    L = _lib.load()
    for s in NEW_SYMBOLS:
        assert s in text and s in _lib.SIGNATURES and hasattr(L, s), s


@pytest.mark.parametrize("symbol", NEW_SYMBOLS)
def test_null_handle_is_14_with_outputs_untouched(symbol):
    from test_abi import test_null_handle_code_and_untouched_outputs as check
    check(symbol, 14)


# ------------------------------------------------------------------------------------------------------------ GPU tests
SIZES = (5, 6, 7, 8, 63, 64, 65, 127, 129, 255, 257, 1002)
HK_MODES = ["u16", "i32", "mf_euc", "mf_att", "mf_ceil", "mf_ceil_int"]


def check_tree(eng, pi, what, **src):
    L, edges, deg = eng.one_tree(pi)
    want = model_one_tree(pi=pi, **src)
    assert L == want["L"], what
    assert np.array_equal(edges, want["edges"]) and np.array_equal(deg, want["deg"]), what
    return L


@pytest.mark.gpu
@pytest.mark.parametrize("mode", HK_MODES)
def test_one_tree_equals_the_model(mode):
    """uint16 and int32 cells and the four weight forms from the points (matrix-free forced), at the wave, rows-per-workgroup
    and vector edges, pi = 0 and two fixed random pi"""
    for n in SIZES:
        xy, kind = points_for(mode, n, 1)
        eng = engine_for(mode, xy, kind)
        rng = np.random.default_rng(n)
        for pi in (None, random_pi(n, rng), random_pi(n, rng)):
            check_tree(eng, pi, (mode, n), xy=xy, kind=kind)
        info = eng.info()
        assert 1 <= info["hk_rounds"] <= max(1, math.ceil(math.log2(n - 1))) and info["hk_nodes"] == 8, (mode, n)
        eng.close()


@pytest.mark.gpu
def test_one_tree_on_a_caller_matrix():
    """tspgpu_set_costs without points: uint16 and int32 cells"""
    for n in SIZES:
        rng = np.random.default_rng(100 + n)
        c = sym_int_matrix(n, rng)
        for mode in ("u16", "i32"):
            eng = engine_for(mode, costs=c)
            for pi in (None, random_pi(n, rng)):
                check_tree(eng, pi, (mode, n), costs=c)
            eng.close()


@pytest.mark.gpu
def test_one_tree_where_every_choice_is_a_tie():
    for name, c in tie_cases():
        eng = engine_for("u16", costs=c)
        check_tree(eng, None, name, costs=c)
        check_tree(eng, np.zeros(len(c), np.int64), name, costs=c)
        eng.close()
    for name, xy in (("lattice40", rect_lattice(8, 5)), ("lattice1000", rect_lattice(40, 25)), ("clusters300", clusters(300, 5))):
        for mode in ("u16", "mf_euc"):
            eng = engine_for(mode, xy, 0)
            check_tree(eng, None, (name, mode), xy=xy, kind=0)
            eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["berlin52", "kroA100", "att48", "eil51", "pr1002"])
def test_ascent_equals_the_golden(name):
    """bound, reason, iterations, the digest of pi*, the final h, and on berlin52 the tour -- from the matrix and from the points"""
    g = golden()["ascent"][name]
    xy, kind = tsplib_instance(name)
    for mode in ("u16", "mf"):
        eng = engine_for(mode, xy, kind)
        r = eng.lower_bound(g["upper"], g["iters_asked"], g["patience"])
        assert (r.rc, r.bound, r.reason, r.iters) == (0, g["bound"], g["reason"], g["iters"]), (name, mode)
        assert digest64(r.pi) == g["pi_sha256"], (name, mode)
        info = eng.info()
        assert (info["hk_iterations"], info["hk_reason"], info["hk_h"]) == (g["iters"], g["reason"], g["h"]), (name, mode)
        if g["reason"] == 1:
            assert digest(tour_of(r.path)) == g["path_sha256"], (name, mode)
        else:
            assert r.path is None
        assert eng.one_tree(r.pi)[0] == g["best"], (name, mode)
        eng.close()


@pytest.mark.gpu
def test_ascent_continues_from_the_returned_multipliers():
    """100 iterations, then 200 from pi*: both valid bounds, the second no lower than the first, each equal to the model's"""
    xy, kind = tsplib_instance("kroA100")
    eng = engine_for("u16", xy, kind)
    a = eng.lower_bound(27807, 100, 10)
    b = eng.lower_bound(27807, 200, 10, pi=a.pi)
    ma = model_ascent(27807, 100, 10, xy=xy, kind=kind)
    mb = model_ascent(27807, 200, 10, xy=xy, kind=kind, pi=ma["pi"])
    assert (a.bound, a.reason, a.iters) == (ma["bound"], ma["reason"], ma["iters"]) and np.array_equal(a.pi, ma["pi"])
    assert (b.bound, b.reason, b.iters) == (mb["bound"], mb["reason"], mb["iters"]) and np.array_equal(b.pi, mb["pi"])
    assert bound_of(golden()["ascent"]["kroA100"]["L0"]) <= a.bound <= b.bound <= OPTIMA["kroA100"]
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", [("fnl4461", "u16"), ("pla85900", "mf")])
def test_large_trees_equal_the_golden(name, mode):
    """one 1-tree at pi = 0 and at the golden's fixed pi: L and the digest of the edge array (the model ran offline)"""
    g = golden()["tree"][name]
    xy, kind = tsplib_instance(name)
    eng = engine_for(mode, xy, kind)
    for tag, pi in (("zero", None), ("fixed", fixed_pi(len(xy), g["seed"]))):
        L, edges, deg = eng.one_tree(pi)
        assert L == g[tag]["L"] and digest(edges) == g[tag]["edges_sha256"], (name, tag)
        assert deg[0] == 2 and int(deg.sum()) == 2 * len(xy), (name, tag)
        assert eng.info()["hk_rounds"] <= math.ceil(math.log2(len(xy) - 1)), (name, tag)
    eng.close()


def refused(call):
    from travellingsalesmanoptimization_amd import TspGpuError
    with pytest.raises(TspGpuError) as e:
        call()
    return e.value.code


@pytest.mark.gpu
def test_refusals():
    import travellingsalesmanoptimization_amd as T
    rng = np.random.default_rng(9)
    c = sym_int_matrix(20, rng)
    eng = engine_for("f64", costs=c)
    assert refused(eng.one_tree) == 12 and refused(lambda: eng.lower_bound(20000)) == 12
    eng.close()
    a = c.copy()
    a[2][5] += 1.0
    eng = engine_for("u16", costs=a)
    assert refused(eng.one_tree) == 9 and refused(lambda: eng.lower_bound(20000)) == 9
    eng.close()
    eng = T.Engine(0)
    eng.set_points(points_for("u16", 20, 1)[0])
    eng.n = 20
    assert refused(eng.one_tree) == 9 and refused(lambda: eng.lower_bound(20000)) == 9       # no costs
    eng.close()
    eng = engine_for("u16", costs=sym_int_matrix(4, rng))
    assert refused(eng.one_tree) == 3 and refused(lambda: eng.lower_bound(2000)) == 3         # n = 4
    eng.close()
    eng = engine_for("u16", costs=c)
    for bad in (float(1 << 33), -1.0, 100.5, float("nan")):                                  # S UB >= 2^40, negative, fractional
        assert refused(lambda: eng.lower_bound(bad)) == 3, bad
    assert refused(lambda: eng.lower_bound(20000, iters=0)) == 3 and refused(lambda: eng.lower_bound(20000, patience=0)) == 3
    too_big = np.zeros(20, np.int64)
    too_big[3] = PI_MAX + 1
    assert refused(lambda: eng.one_tree(too_big)) == 3 and refused(lambda: eng.lower_bound(20000, pi=too_big)) == 3
    assert eng.lower_bound(float((1 << 33) - 1), iters=1).rc == 0
    eng.close()


@pytest.mark.gpu
def test_deadline_reasons_2_and_5():
    xy, kind = tsplib_instance("kroA100")
    eng = engine_for("u16", xy, kind)
    g = golden()["ascent"]["kroA100"]
    r = eng.lower_bound(27807, 300, 10, time_left_s=0.0)      # a passed deadline: one batch of TSPGPU_OPT_BATCH iterations ran
    m = model_ascent(27807, 32, 10, xy=xy, kind=kind)
    assert (r.rc, r.reason, r.iters) == (4, 4, 32) and r.bound == m["bound"] and np.array_equal(r.pi, m["pi"])
    assert bound_of(g["L0"]) <= r.bound <= OPTIMA["kroA100"]
    r = eng.lower_bound(20000, 300, 10)                         # an upper bound below the bound the ascent reaches
    m = model_ascent(20000, 300, 10, xy=xy, kind=kind)
    assert m["reason"] == 2 and m["best"] >= S * 20000
    assert (r.rc, r.bound, r.reason, r.iters) == (0, m["bound"], 2, m["iters"]) and np.array_equal(r.pi, m["pi"])
    pi = np.full(100, PI_MAX - 10, np.int64)                    # every node of degree >= 3 would pass 2^45
    r = eng.lower_bound(27807, 20, 3, pi=pi)
    m = model_ascent(27807, 20, 3, xy=xy, kind=kind, pi=pi)
    assert m["reason"] == 5 and (r.rc, r.bound, r.reason, r.iters) == (0, m["bound"], 5, 1) and np.array_equal(r.pi, pi)
    eng.close()


@pytest.mark.gpu
def test_two_instances_on_one_context():
    """the state is dropped with the instance: a larger n, then a smaller one, then tspgpu_destroy"""
    import travellingsalesmanoptimization_amd as T
    eng = T.Engine(0)
    for n in (300, 77, 513):
        xy, kind = points_for("u16", n, 2)
        eng.set_points(xy, kind)
        eng.build_costs()
        check_tree(eng, None, n, xy=xy, kind=kind)
        r = eng.lower_bound(iters=20)
        m = model_ascent(r.upper, 20, 10, xy=xy, kind=kind)
        assert r.upper == O.nn_tour(O.cost_matrix(xy, kind), 0)[1]
        assert (r.bound, r.reason, r.iters) == (m["bound"], m["reason"], m["iters"]) and np.array_equal(r.pi, m["pi"]), n
    eng.close()


@pytest.mark.gpu
def test_host_binary_reports_the_bound():
    """TSP_LOWER_BOUND=50 with -alg GREEDY: the bound line on stderr is the model's from the reported cost, the solution and the
    exit code are those of the run without the variable; a malformed value is refused"""
    args = ("-f", os.path.join(DATA, "berlin52.tsp"), "-alg", "GREEDY", "-q")
    os.environ.pop("TSP_LOWER_BOUND", None)
    plain = run_tsp(*args)
    assert plain[0] == 0 and plain[1].startswith("Cost: ") and "lower bound" not in plain[2]
    cost = float(plain[1].split()[1])
    xy, kind = tsplib_instance("berlin52")
    m = model_ascent(int(cost), 50, 10, xy=xy, kind=kind)
    code, out, err = run_tsp(*args, env_set={"TSP_LOWER_BOUND": "50", "TSP_GPU_STATS": "1"})
    assert (code, out) == plain[:2], err
    assert "tsp: lower bound %d after %d iterations (reason %d), gap %.4f %%" % (m["bound"], m["iters"], m["reason"],
                                                                                  100.0 * ((cost - m["bound"]) / m["bound"])) in err
    stats = [json.loads(line.split("tspgpu-stats: ", 1)[1]) for line in err.splitlines() if line.startswith("tspgpu-stats: ") and "lower_bound" in line]
    assert len(stats) == 1 and (stats[0]["bound"], stats[0]["iterations"], stats[0]["reason"]) == (m["bound"], m["iters"], m["reason"])
    assert run_tsp(*args, env_set={"TSP_LOWER_BOUND": "0"})[:2] == plain[:2]
    for bad in ("x", "-1", "100001", "", "5x"):
        code, out, err = run_tsp(*args, env_set={"TSP_LOWER_BOUND": bad})
        assert code != 0 and "TSP_LOWER_BOUND" in err and "expected an iteration count" in err, bad
