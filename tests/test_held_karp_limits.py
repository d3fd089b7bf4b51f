"""Held-Karp lower bound at its limits (include/tspgpu.h "Held-Karp lower bound"): what tests/test_held_karp.py leaves
comfortable.  Every comparison is bit for bit; the reference is tests/held_karp_model.c, and where noted the arbitrary-precision
Python restatement of test_held_karp.py is the reference for the model.

CPU: the model against the Python Kruskal with weights that need 64 bits (costs below 2^27, four families of multipliers up to
2^45), on coordinates whose costs reach 2^27, on the line with growing gaps (one round, one hook chain of n - 3), and rule 3 to
its reason 3.
GPU: one_tree on both sides of the staging threshold (tspgpu_info 91 says which scan ran) in every cell type and weight form,
the 64-bit weights in every cost source, the chains, reason 3, the ascent under other batch sizes, the ascent and a context
beyond the threshold.

The multiplier families (pi_family): a uniform in +-2^45; b uniform in +-2^33, the size of 128 c; c +-2^44 per node plus noise
in +-2^20; d an integer in +-2^13 shifted left by 32, nothing in the low word.  Every case asserts that its weights leave 32
bits: below -2^40 and above 2^40 for a, c and d.  Family b cannot reach that (|pi[a] + pi[b]| <= 2^34 and 128 c < 2^34 bound
every weight by 2^35), so there the assertion is below -2^32 and above 2^32: what no 32-bit word holds, signed or not."""
import functools
import hashlib
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import oracle as O  # noqa: E402
from make_golden_held_karp import S, model_ascent, model_one_tree, tsplib_instance  # noqa: E402
from make_golden_two_opt_nl import digest  # noqa: E402
from test_held_karp import (HK_MODES, OPTIMA, PI_MAX, check_tree, golden, ints, py_ascent, py_rounds, py_tree, random_pi,  # noqa: E402
                            same_tree, tour_of)
from test_two_opt_multi import ATT, CEIL_2D, EUC_2D, engine_for, points_for, sym_int_matrix  # noqa: E402

FAMILIES = ("a", "b", "c", "d")
LEAVES_32_BITS = {"a": 1 << 40, "b": 1 << 32, "c": 1 << 40, "d": 1 << 40}
COST_MAX = 1 << 27
BIG_FORMS = ("euc", "ceil_int", "ceil_real", "att")
REASON_3 = (("kroA100", 27807), ("eil51", 450))         # patience 1, 3000 iterations asked: the step reaches 0 long before


def pi_family(fam, n, rng):
    if fam == "a":
        return rng.integers(-PI_MAX, PI_MAX + 1, n).astype(np.int64)
    if fam == "b":
        return rng.integers(-(1 << 33), (1 << 33) + 1, n).astype(np.int64)
    if fam == "c":
        level = np.where(rng.integers(0, 2, n) == 1, 1 << 44, -(1 << 44)).astype(np.int64)
        return level + rng.integers(-(1 << 20), (1 << 20) + 1, n).astype(np.int64)
    assert fam == "d"
    return rng.integers(-(1 << 13), (1 << 13) + 1, n).astype(np.int64) << 32


def weight_range(c, pi):
    """the smallest and the largest w(a, b), a != b, exactly (|w| < 2^47)"""
    w = S * np.asarray(c).astype(np.int64) + pi[:, None] + pi[None, :]
    off = ~np.eye(len(pi), dtype=bool)
    return int(w[off].min()), int(w[off].max())


def leaves_32_bits(c, pi, fam, what):
    lo, hi = weight_range(c, pi)
    assert lo < -LEAVES_32_BITS[fam] and hi > LEAVES_32_BITS[fam], (what, lo, hi)


def big_points(form, n, seed):
    """-> (xy, kind): coordinates whose costs come close to 2^27 without reaching it"""
    rng = np.random.default_rng(77000 + 10 * n + seed)
    if form == "att":
        return rng.integers(0, 280000001, (n, 2)).astype(np.float64), ATT
    if form == "ceil_real":
        return rng.uniform(0.0, 9.0e7, (n, 2)), CEIL_2D
    return rng.integers(0, 90000001, (n, 2)).astype(np.float64), (EUC_2D if form == "euc" else CEIL_2D)


def line_points(n, backwards):
    """node i at x = (i + 1)(i + 2) / 2: the gap behind node i is i + 2, strictly growing; backwards: numbered from the far end"""
    x = np.array([(i + 1) * (i + 2) // 2 for i in range(n)], np.float64)
    xy = np.stack([x[::-1] if backwards else x, np.zeros(n)], axis=1)
    return np.ascontiguousarray(xy), EUC_2D


def line_tree(n):
    """the 1-tree of the line in either numbering: the path over the nodes 1 .. n - 1, and node 0 with its two nearest"""
    return sorted([(0, 1), (0, 2)] + [(v, v + 1) for v in range(1, n - 1)])


def edges_of(tree_edges):
    return [tuple(int(x) for x in e) for e in np.asarray(tree_edges)]


# the model's answers are computed once per input and only compared afterwards
_trees = {}


def model_tree(xy, kind, pi):
    key = (kind, hashlib.sha256(np.ascontiguousarray(xy).tobytes()).digest(), None if pi is None else hashlib.sha256(pi.tobytes()).digest())
    if key not in _trees:
        _trees[key] = model_one_tree(xy=xy, kind=kind, pi=pi)
    return _trees[key]


def check_points_tree(eng, xy, kind, pi, what):
    L, edges, deg = eng.one_tree(pi)
    want = model_tree(xy, kind, pi)
    assert L == want["L"], what
    assert np.array_equal(edges, want["edges"]) and np.array_equal(deg, want["deg"]), what
    return want


@functools.lru_cache(maxsize=None)
def reason_3_case(name, upper):
    xy, kind = tsplib_instance(name)
    return xy, kind, model_ascent(upper, 3000, 1, xy=xy, kind=kind)


@functools.lru_cache(maxsize=None)
def beyond_case(n):
    """the points of the uint16 / EUC_2D modes at n, the oracle's NN(0) cost, and the model's ascent from it (10 iterations, patience 3)"""
    xy, kind = points_for("u16", n, 1)
    upper = O.nn_tour_xy(xy, kind, 0)[1]
    return xy, kind, upper, model_ascent(upper, 10, 3, xy=xy, kind=kind)


# ------------------------------------------------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("n", [9, 33, 100])
def test_model_tree_equals_the_python_kruskal_at_64_bit_weights(n):
    """B1.  costs below 2^27 (128 c up to 2^34) with every multiplier family: the model's 64-bit Prim against Kruskal in Python's
    integers"""
    rng = np.random.default_rng(6400 + n)
    c = sym_int_matrix(n, rng, hi=COST_MAX)
    assert c.max() >= COST_MAX // 2
    for fam in FAMILIES:
        pi = pi_family(fam, n, rng)
        leaves_32_bits(c, pi, fam, (n, fam))
        same_tree(model_one_tree(costs=c, pi=pi), py_tree(ints(c), pi), (n, fam))


@pytest.mark.parametrize("form", BIG_FORMS)
def test_model_on_large_coordinates(form):
    """B2.  integer points in [0, 9e7]^2 (EUC_2D, CEIL_2D), real ones (CEIL_2D), integer points in [0, 2.8e8]^2 (ATT): costs
    stay below 2^27, and the model from the points, the model from the oracle's matrix and the Python Kruskal agree"""
    n = 60
    xy, kind = big_points(form, n, 0)
    c = O.cost_matrix(xy, kind)
    assert COST_MAX // 2 < c.max() < COST_MAX
    pi = pi_family("b", n, np.random.default_rng(60))
    leaves_32_bits(c, pi, "b", form)
    want = py_tree(ints(c), pi)
    same_tree(model_one_tree(xy=xy, kind=kind, pi=pi), want, form)
    same_tree(model_one_tree(costs=c, pi=pi), want, form)


@pytest.mark.parametrize("backwards", [False, True])
def test_the_line_is_one_round_and_one_chain(backwards):
    """B3.  every node's nearest node is the one towards the small gaps, so all n - 2 tree edges are accepted in the first round and
    n - 3 components hook onto one another in one chain"""
    for n in (40, 300):
        xy, kind = line_points(n, backwards)
        c = O.cost_matrix(xy, kind)
        want = py_rounds(ints(c))
        assert want["rounds"] == 1 and want["edges"] == line_tree(n), n
        same_tree(model_one_tree(xy=xy, kind=kind), want, n)
        same_tree(model_one_tree(costs=c), want, n)
    xy, kind = line_points(5441, backwards)
    assert edges_of(model_tree(xy, kind, None)["edges"]) == line_tree(5441)


@pytest.mark.parametrize("name,upper", REASON_3)
def test_reason_3_in_the_model(name, upper):
    """B4.  patience 1 doubles the divisor at every iteration that is no new best: the step reaches 0 (17 iterations, h = 16,
    bound 19 094 on kroA100; 25 iterations, h = 10, bound 422 on eil51 when this test was written -- compared live, not pinned)"""
    xy, kind, got = reason_3_case(name, upper)
    want = py_ascent(ints(O.cost_matrix(xy, kind)), upper, 3000, 1)
    for k in ("bound", "best", "reason", "iters", "h"):
        assert got[k] == want[k], k
    assert np.array_equal(got["pi"], want["pi"])
    assert got["reason"] == 3 and got["h"] >= 1 and got["iters"] < 3000 and got["bound"] <= OPTIMA[name]


def test_info_91_is_documented_and_named():
    import inspect
    import travellingsalesmanoptimization_amd as T
    text = open(os.path.join(ROOT, "include", "tspgpu.h")).read()
    section = text[text.index("---- Held-Karp lower bound"):]
    assert "91 the LDS bytes per workgroup" in section and "86 .. 91" in text
    names = re.findall(r'"(\w+)"', inspect.getsource(T.Engine.info))
    assert names.index("hk_nodes") == 90 and names.index("hk_lds") == 91


# ------------------------------------------------------------------------------------------------------------ GPU tests
def rounds_ok(eng, n):
    return 1 <= eng.info()["hk_rounds"] <= math.ceil(math.log2(n - 1))


@pytest.mark.gpu
@pytest.mark.parametrize("n,ld,lds", [(5440, 5440, 65280), (5441, 5472, 0), (6001, 6016, 0)])
@pytest.mark.parametrize("mode", HK_MODES)
def test_staging_boundary(mode, n, ld, lds):
    """C1.  n = 5440 is the last size whose comp[] and pi[] are staged in LDS (12 ld = 65 280 bytes), 5441 the first that reads them
    through L2 (ld = 5472: 31 padding cells behind every row), 6001 well beyond: pi = 0, pi in +-2^20 and family b"""
    xy, kind = points_for(mode, n, 1)
    eng = engine_for(mode, xy, kind)
    info = eng.info()
    assert info["ld"] == ld and info["hk_lds"] == 0                 # (no 1-tree yet)
    rng = np.random.default_rng(n)
    for tag, pi in (("zero", None), ("2^20", random_pi(n, rng)), ("b", pi_family("b", n, rng))):
        check_points_tree(eng, xy, kind, pi, (mode, n, tag))
        assert eng.info()["hk_lds"] == lds and rounds_ok(eng, n), (mode, n, tag)
    eng.close()


def hub(want, n, what):
    """family a: the node of the smallest multiplier is every node's nearest -- a star of n - 2 edges, and node 0's edge"""
    assert int(np.max(want["deg"])) in (n - 2, n - 1), what


@pytest.mark.gpu
@pytest.mark.parametrize("mode,hi", [("i32", COST_MAX), ("u16", 65535)])
def test_weights_past_32_bits_on_a_caller_matrix(mode, hi):
    """C2.  int32 cells up to 2^27 - 1 and uint16 cells up to 65 534 under every multiplier family"""
    for n in (65, 257, 1002):
        rng = np.random.default_rng(3201 + n)           # (a seed whose two smallest multipliers of family a lie more than 2^34 apart)
        c = sym_int_matrix(n, rng, hi=hi)
        assert c.max() >= hi - 1 - hi // 64
        eng = engine_for(mode, costs=c)
        for fam in FAMILIES:
            pi = pi_family(fam, n, rng)
            leaves_32_bits(c, pi, fam, (mode, n, fam))
            L, edges, deg = eng.one_tree(pi)
            want = model_one_tree(costs=c, pi=pi)
            assert L == want["L"] and np.array_equal(edges, want["edges"]) and np.array_equal(deg, want["deg"]), (mode, n, fam)
            if fam == "a":
                hub(want, n, (mode, n))
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", BIG_FORMS)
def test_weights_past_32_bits_matrix_free(form):
    """C2.  the weight forms from the points, costs up to 2^27 (the engine's cost bound, from the bounding box, is between 2^26 and
    2^27, so tspgpu_build_costs accepts the box as it is); with coordinates this large CEIL_2D runs its generic form"""
    for n in (65, 257, 1002):
        xy, kind = big_points(form, n, 1)
        eng = engine_for({"euc": "mf_euc", "att": "mf_att"}.get(form, "mf_ceil"), xy, kind)
        info = eng.info()
        assert info["matrix_free"] == 1 and info["ceil_int"] == 0, (form, n)
        c = O.cost_matrix(xy, kind)
        assert COST_MAX // 2 < c.max() < COST_MAX
        rng = np.random.default_rng(3300 + n)
        for fam in FAMILIES:
            pi = pi_family(fam, n, rng)
            leaves_32_bits(c, pi, fam, (form, n, fam))
            want = check_points_tree(eng, xy, kind, pi, (form, n, fam))
            if fam == "a":
                hub(want, n, (form, n))
        eng.close()


@pytest.mark.gpu
def test_weights_past_32_bits_unstaged():
    """C2.  n = 5441, int32 cells built from the large EUC_2D points: k_hk_scan<int, false> with weights up to 2^46"""
    n = 5441
    xy, kind = big_points("euc", n, 1)
    eng = engine_for("i32", xy, kind)
    assert eng.info()["elem"] == 2
    rng = np.random.default_rng(3400 + n)
    for fam in FAMILIES:
        pi = pi_family(fam, n, rng)
        want = check_points_tree(eng, xy, kind, pi, fam)
        assert eng.info()["hk_lds"] == 0 and rounds_ok(eng, n), fam
        if fam == "a":
            hub(want, n, fam)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("backwards", [False, True])
@pytest.mark.parametrize("mode,n", [("u16", 300), ("i32", 1002), ("mf_euc", 1002), ("mf_euc", 5441)])
def test_one_chain_of_hooks(mode, n, backwards):
    """C3.  the line: n - 3 components hook in the one round, and k_hk_flat walks a chain of that length; the tree is the path and
    node 0's two nearest, as written out, and the model's"""
    xy, kind = line_points(n, backwards)
    eng = engine_for(mode, xy, kind)
    want = check_points_tree(eng, xy, kind, None, (mode, n, backwards))        # (an INTERNAL error would raise here)
    assert edges_of(want["edges"]) == line_tree(n) and edges_of(eng.one_tree()[1]) == line_tree(n)
    assert eng.info()["hk_rounds"] == 1
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,upper", REASON_3)
def test_reason_3_on_the_device(name, upper):
    """C4.  the two ascents of test_reason_3_in_the_model, from the matrix and from the points"""
    xy, kind, m = reason_3_case(name, upper)
    assert m["reason"] == 3
    for mode in ("u16", "mf"):
        eng = engine_for(mode, xy, kind)
        r = eng.lower_bound(upper, 3000, 1)
        assert (r.rc, r.bound, r.reason, r.iters) == (0, m["bound"], 3, m["iters"]) and np.array_equal(r.pi, m["pi"]), (name, mode)
        info = eng.info()
        assert (info["hk_reason"], info["hk_iterations"], info["hk_h"]) == (3, m["iters"], m["h"]), (name, mode)
        assert r.path is None and eng.one_tree(r.pi)[0] == m["best"], (name, mode)
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 7, 1000])
def test_ascent_does_not_depend_on_the_batch(batch):
    """C5.  kroA100, 100 iterations: one, seven and all iterations enqueued per look at the control block"""
    import travellingsalesmanoptimization_amd as T
    xy, kind = tsplib_instance("kroA100")
    m = model_ascent(27807, 100, 10, xy=xy, kind=kind)
    eng = engine_for("u16", xy, kind)
    eng.set_option(T.OPT_BATCH, batch)
    r = eng.lower_bound(27807, 100, 10)
    assert (r.rc, r.bound, r.reason, r.iters) == (0, m["bound"], m["reason"], m["iters"]) and np.array_equal(r.pi, m["pi"])
    info = eng.info()
    assert (info["hk_reason"], info["hk_iterations"], info["hk_h"]) == (m["reason"], m["iters"], m["h"])
    assert eng.one_tree(r.pi)[0] == m["best"]
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 1000])
def test_the_tour_of_reason_1_under_other_batches(batch):
    """C5.  berlin52 stops with reason 1 after 163 iterations: a look per iteration, and with all 300 enqueued at once -- the
    stop then happens with the launches of 137 iterations queued behind it, which must leave the tree in hand alone"""
    import travellingsalesmanoptimization_amd as T
    g = golden()["ascent"]["berlin52"]
    assert g["reason"] == 1 and g["iters"] < g["iters_asked"]
    xy, kind = tsplib_instance("berlin52")
    eng = engine_for("u16", xy, kind)
    eng.set_option(T.OPT_BATCH, batch)
    r = eng.lower_bound(g["upper"], g["iters_asked"], g["patience"])
    assert (r.rc, r.bound, r.reason, r.iters) == (0, g["bound"], 1, g["iters"])
    assert digest(tour_of(r.path)) == g["path_sha256"]
    eng.close()


@pytest.mark.gpu
def test_a_passed_deadline_runs_one_batch_of_five():
    """C5.  the clock is read every TSPGPU_OPT_BATCH iterations and at least that many run: code 4, reason 4, 5 iterations"""
    import travellingsalesmanoptimization_amd as T
    xy, kind = tsplib_instance("kroA100")
    m = model_ascent(27807, 5, 10, xy=xy, kind=kind)
    eng = engine_for("u16", xy, kind)
    eng.set_option(T.OPT_BATCH, 5)
    r = eng.lower_bound(27807, 300, 10, time_left_s=0.0)
    assert (r.rc, r.reason, r.iters) == (4, 4, 5) and r.bound == m["bound"] and np.array_equal(r.pi, m["pi"])
    info = eng.info()
    assert (info["hk_reason"], info["hk_iterations"], info["hk_h"]) == (4, 5, m["h"])
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["u16", "mf_euc"])
def test_ascent_beyond_the_threshold(mode):
    """C6.  n = 5441: ten iterations of the ascent with comp[] and pi[] through L2, from the NN tour's cost"""
    n = 5441
    xy, kind, upper, m = beyond_case(n)
    eng = engine_for(mode, xy, kind)
    r = eng.lower_bound(iters=10, patience=3)
    assert r.upper == upper
    assert (r.rc, r.bound, r.reason, r.iters) == (0, m["bound"], m["reason"], m["iters"]) and np.array_equal(r.pi, m["pi"]), mode
    info = eng.info()
    assert (info["hk_reason"], info["hk_iterations"], info["hk_h"], info["hk_lds"]) == (m["reason"], m["iters"], m["h"], 0), mode
    eng.close()


@pytest.mark.gpu
def test_one_context_across_the_threshold():
    """C6.  5441 nodes, then 300, then 5441 again on one context: the scan follows the instance"""
    import travellingsalesmanoptimization_amd as T
    eng = T.Engine(0)
    assert eng.info()["hk_lds"] == 0
    for n, seed, lds in ((5441, 1, 0), (300, 2, 3840), (5441, 3, 0)):
        xy, kind = points_for("u16", n, seed)
        eng.set_points(xy, kind)
        eng.build_costs()
        rng = np.random.default_rng(n + seed)
        for pi in (None, pi_family("b", n, rng)):
            check_points_tree(eng, xy, kind, pi, (n, seed))
            assert eng.info()["hk_lds"] == lds, (n, seed)
    eng.close()
