"""Don't-look bits for the neighbour-list families and the kick on a slot (include/tspgpu.h "Don't-look bits").

The model is tests/dont_look_model.c (wrappers in tools/make_golden_dont_look.py): the plain models' candidates, masked to the
looked units, with compaction, selection, apply, carry and ends restated behind them.
CPU: the model's first all-awake sweep against the plain models' sweeps, a closing phase against the plain models' sweeps on the
result, the golden, the header and the exported symbols, the host's part of a phase (tests/dont_look_main.cpp) under ASan/UBSan.
GPU: the first all-awake sweep against the plain slot calls in every cell type and weight form and both slot directions,
stepping through phases and descents against the model with the three awake sets, closing phases against the plain _once calls,
windows, the kick, the state rules, refusals, memory across instances, the host binary's TSP_DONT_LOOK."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import oracle as O  # noqa: E402
import make_golden_dont_look as G  # noqa: E402
import make_golden_two_opt_nl as G2  # noqa: E402
from make_golden_dont_look import all_awake, model_dl_descent, model_dl_phase, model_dl_sweep, model_kick  # noqa: E402
from make_golden_or_opt_nl import model_or_sweep  # noqa: E402
from make_golden_three_opt_nl import model_three_sweep  # noqa: E402
from make_golden_two_opt_nl import digest, model_lists, model_sweep  # noqa: E402
from test_mem_owner import CSRC, SAN, asan_links  # noqa: E402
from test_two_opt_multi import MODES, engine_for, points_for, random_tour, symmetric_noise, weight_matrix  # noqa: E402
from test_or_opt_nl import run_tsp, tour_from_zero  # noqa: E402
from test_or_opt_geometry import Layout  # noqa: E402
from test_vns_nl import f64_cost_bound  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_dont_look.json")
NEW_SYMBOLS = ["tspgpu_tour_wake", "tspgpu_tour_sleep", "tspgpu_tour_awake", "tspgpu_tour_kick", "tspgpu_tour_two_opt_nl_dl",
               "tspgpu_tour_or_opt_nl_dl", "tspgpu_tour_three_opt_nl_dl", "tspgpu_tour_local_search_nl3_dl", "tspgpu_local_search_nl3_dl"]
SIZES = (8, 9, 13, 64, 65, 257)
K, W = 5, 4
PLAIN = (lambda p, c, nodes, **s: model_sweep(p, c, nodes, **s), lambda p, c, nodes, **s: model_or_sweep(p, c, nodes, **s),
         lambda p, c, nodes, **s: model_three_sweep(p, c, nodes, W, **s))


def tour_cost(path, c):
    return float(sum(c[i][int(path[i])] for i in range(len(path))))


def int_case(n, seed=0):
    rng = np.random.default_rng(77 * n + seed)
    xy = rng.integers(0, 60 if n < 20 else 900, (n, 2)).astype(np.float64)
    return O.cost_matrix(xy), random_tour(n, rng)


# ------------------------------------------------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("n", SIZES)
def test_model_first_all_awake_sweep_is_the_plain_sweep(n):
    """consequence (a), in the model: tour, cost and moves of the plain models' sweeps; Q is every node; the new set is carry +
    ends, a subset that holds the end nodes of every accepted move"""
    c, start = int_case(n)
    nodes, _ = model_lists(K, costs=c)
    for f in range(3):
        want, cost0 = start.copy(), tour_cost(start, c)
        r = PLAIN[f](want, cost0, nodes, costs=c)
        got, awake = start.copy(), all_awake(n)
        d = model_dl_sweep(f, got, cost0, awake, nodes, W, costs=c)
        assert np.array_equal(got, want) and d["cost"] == r["cost"] and d["moves"] == len(r["moves"]) and d["looked"] == n, f
        A = awake.reshape(3, n)
        changed = {v for v in range(n) if start[v] != got[v]}
        assert changed <= set(np.flatnonzero(A[f])), f
        for g in range(3):
            if g != f:
                assert changed <= set(np.flatnonzero(A[g])) and A[g].all()      # the others were all awake and stay so


@pytest.mark.parametrize("n", SIZES)
def test_model_closing_phase_ends_where_the_plain_phase_does(n):
    """consequence (b), in the model: after a closing phase the plain models' sweep accepts nothing and the set is empty;
    without closing the set is empty too and the phase never looks at more units than sweeps x n"""
    c, start = int_case(n, 1)
    nodes, _ = model_lists(K, costs=c)
    for f in range(3):
        for closing in (1, 0):
            path, awake = start.copy(), all_awake(n)
            r = model_dl_phase(f, path, tour_cost(start, c), awake, nodes, W, closing, costs=c)
            assert O.valid_tour(path) and r["cost"] == tour_cost(path, c)
            assert not awake.reshape(3, n)[f].any() and r["looked"] <= r["sweeps"] * n and r["full_sweeps"] >= 1
            if closing:
                assert len(PLAIN[f](path.copy(), r["cost"], nodes, costs=c, apply=False)["moves"]) == 0, f
    path, awake = start.copy(), all_awake(n)
    r = model_dl_descent(path, tour_cost(start, c), awake, nodes, W, 1, costs=c)
    for f in range(3):
        assert len(PLAIN[f](path.copy(), r["cost"], nodes, costs=c, apply=False)["moves"]) == 0
    assert not awake.any()


def test_golden_is_the_model_and_the_kicks_look_at_less():
    want = json.load(open(GOLDEN))
    got = json.loads(json.dumps({"pr1002": G.loop(), "rejected_inside_reversal": G.rejected_inside_reversal()}))
    assert got == want
    p = want["pr1002"]
    assert p["kicks_looked"] == sum(it["looked"] for it in p["iterations"]) < p["kicks_plain_units"]
    assert len(p["iterations"]) == len(p["plain_iterations"]) == len(p["kicks"]) == 20


def test_header_states_the_rule_and_the_library_exports_the_symbols():
    text = open(os.path.join(ROOT, "include", "tspgpu.h")).read()
    for phrase in ("Don't-look bits", "A_f' = carry + ends", "fwd = 0 for the 2-opt, 2 for Or-opt", "Phase with looks", "closing != 0",
                   "((c[a][b'] + c[c][a']) + c[b][c']) - ((c[a][a'] + c[b][b']) + c[c][c'])", "the classic approximation",
                   "70 `looked` of the last call with looks"):
        assert phrase in text, phrase
    from travellingsalesmanoptimization_amd import _lib
    L = _lib.load()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in _lib.SIGNATURES and s in text
    for s in NEW_SYMBOLS:       # a null handle: UNAVAILABLE before anything is touched
        args = [np.zeros(16, np.int32) if t is _lib._ip else 1 if t in (_lib.C.c_int, _lib.C.c_long, _lib.C.c_double) else None
                for t in _lib.SIGNATURES[s][1][1:]]
        assert getattr(L, s)(None, *args) == 14, s


def test_host_part_of_a_phase_under_sanitizers(tmp_path):
    if not asan_links(tmp_path):
        pytest.skip("linking an empty program with g++ -fsanitize=address -static-libasan fails here (no sanitizer runtime)")
    exe = str(tmp_path / "dont_look")
    r = subprocess.run(["g++", *SAN, "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "dont_look_main.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "dont_look ok"


# ------------------------------------------------------------------------------------------------------------ GPU tests
def dl_call(eng, f, slot, closing, max_sweeps=-1):
    if f == 0:
        return eng.tour_two_opt_nl_dl(slot, closing, max_sweeps)
    if f == 1:
        return eng.tour_or_opt_nl_dl(slot, closing, max_sweeps)
    return eng.tour_three_opt_nl_dl(slot, W, closing, max_sweeps)


def plain_call(eng, f, slot, max_sweeps=-1):
    if f == 0:
        return eng.tour_two_opt_nl(slot, max_sweeps)
    if f == 1:
        return eng.tour_or_opt_nl(slot, max_sweeps)
    return eng.tour_three_opt_nl(slot, W, max_sweeps)


def sets_of(eng, slot):
    return np.concatenate([eng.tour_awake(slot, f) for f in range(3)])


def same_store(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2]


def turn_slot_backward(eng, slot, c):
    """dir = -1 and a rotated order, reached as tests/test_three_opt_nl.py reaches them: one improving 2-opt move (a, b), a < b,
    whose arc succ a .. b holds more than half of the nodes -- the apply reverses the OTHER arc and toggles dir.  The slot's
    layout is mirrored by test_or_opt_geometry.Layout, which asserts the arc; the stored tour must be the moved one.
    -> (dir, the cell of node 0)"""
    path, cost, _ = eng.tour_store(slot)
    n = len(path)
    _, f = tour_from_zero(path)
    for i in range(n):
        for span in range(2, n - 1):
            u, v = f[i], f[(i + span) % n]
            a, b, arc = (u, v, span) if u < v else (v, u, n - span)
            sa, sb = int(path[a]), int(path[b])
            d = (c[a][b] + c[sa][sb]) - (c[a][sa] + c[b][sb])
            if 2 * arc > n and n - arc >= 2 and d < -1.0e-7:
                lay = Layout(path)
                want = path.copy()
                assert O.apply_move(want, None, a, b) == arc
                lay.flip(a, b, arc)
                eng.tour_apply_move(slot, a, b, float(d))
                got, gcost, _ = eng.tour_store(slot)
                assert np.array_equal(got, want) and abs(gcost - (cost + d)) <= 1e-9 * abs(cost)
                return lay.dir, int(np.nonzero(lay.ord == 0)[0][0])
    raise AssertionError("no improving long-arc 2-opt move on this tour")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_first_all_awake_sweep_is_the_plain_sweep(mode):
    """consequence (a) on the device: tour, cost and last delta bit-equal to the plain slot call on a copy, at every size, on a
    freshly loaded slot and on one that a long-arc 2-opt move left with dir = -1 and a rotated order"""
    dirs, rotated = set(), False
    for n in SIZES + (1002,):
        if n == 1002:       # pr1002's points under the mode's weight kind (integer coordinates: the generic CEIL_2D form has no pr1002)
            if mode == "mf_ceil":
                continue
            xy, kind = G2.tsplib_points("pr1002"), points_for(mode, 8, 0)[1]
        else:
            xy, kind = points_for(mode, n, 3)
        c = weight_matrix(xy, kind)
        if mode == "f64":
            c = c + symmetric_noise(n, np.random.default_rng(n))
            eng = engine_for(mode, costs=c)
        else:
            eng = engine_for(mode, xy, kind)
        eng.neighbours_build(K)
        for flipped in (False, True):
            eng.tour_load(0, random_tour(n, np.random.default_rng(n + 5)))
            if flipped:
                d, cell0 = turn_slot_backward(eng, 0, c)
                assert d == -1
                dirs.add(d)
                rotated |= cell0 != 0
            else:
                dirs.add(1)
            for f in range(3):
                eng.tour_copy(1, 0)
                eng.tour_copy(2, 0)
                s, m, rc = plain_call(eng, f, 1, 1)
                assert dl_call(eng, f, 2, 0, 1) == (s, m, n, rc), (n, f, flipped)
                assert same_store(eng.tour_store(1), eng.tour_store(2)), (n, f, flipped)
                info = eng.info()
                assert (info["dl_looked"], info["dl_full_sweeps"], info["dl_max_queue"]) == (n, 1, 0)
        eng.close()
    assert dirs == {1, -1} and rotated


def stepping_case(mode, n):
    xy, kind = points_for(mode, n, 4)
    c = weight_matrix(xy, kind)
    if mode == "f64":
        c = c + symmetric_noise(n, np.random.default_rng(n))
        return engine_for(mode, costs=c), c, dict(costs=c)
    return engine_for(mode, xy, kind), c, dict(costs=c)


def close_enough(mode, got, want, c, sweeps, moves):
    """integer cells: exact.  Real cells: the device sums a sweep's deltas in a tree, the model in key order -- test_vns_nl's
    f64_cost_bound, 2 (moves + sweeps) 2^-53 n max(c), with the sweeps and moves of what is compared: model and device start
    from the same cost, so only these additions can differ"""
    if mode != "f64":
        return got == want
    return abs(got - want) <= f64_cost_bound(c, {"two_opt_sweeps": sweeps, "two_opt_moves": moves, "or_sweeps": 0, "or_moves": 0})


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["u16", "i32", "f64", "mf_att"])
def test_gpu_stepping_through_phases_and_descents(mode):
    """max_sweeps = 1 through phases of every family, closing and not, and whole descents, against the model after every sweep:
    tour, cost, moves, looked and the three awake sets"""
    for n in SIZES:
        eng, c, src = stepping_case(mode, n)
        eng.neighbours_build(K)
        nodes, _ = model_lists(K, **src)
        for closing in (0, 1):
            path = random_tour(n, np.random.default_rng(n + closing))
            eng.tour_load(0, path)
            _, cost, _ = eng.tour_store(0)
            awake = all_awake(n)
            for rnd in range(3):
                for f in range(3):
                    for step in range(1000):
                        r = model_dl_phase(f, path, cost, awake, nodes, W, closing, 1, **src)
                        got = dl_call(eng, f, 0, closing, 1)
                        assert got == (r["sweeps"], r["moves"], r["looked"], 0), (n, closing, rnd, f, step)
                        gpath, gcost, _ = eng.tour_store(0)
                        assert np.array_equal(gpath, path) and close_enough(mode, gcost, r["cost"], c, r["sweeps"], r["moves"]), \
                            (n, closing, rnd, f, step)
                        assert np.array_equal(sets_of(eng, 0), awake), (n, closing, rnd, f, step)
                        cost = gcost
                        if r["sweeps"] == 0 or (r["moves"] == 0 and (r["full_sweeps"] or not closing)):
                            break
                    else:
                        raise AssertionError("a phase of 1000 sweeps at n = %d" % n)
            # the whole descent, from a fresh tour and from the state the steps left (a descent with nothing awake)
            for fresh in (True, False):
                if fresh:
                    path = random_tour(n, np.random.default_rng(n + 9))
                    eng.tour_load(0, path)
                    awake, cost = all_awake(n), eng.tour_store(0)[1]
                r = model_dl_descent(path, cost, awake, nodes, W, closing, **src)
                got = eng.tour_local_search_nl3_dl(0, W, closing)
                for key in ("two_opt_sweeps", "two_opt_moves", "or_sweeps", "or_moves", "rounds", "three_sweeps", "three_moves", "three_phases",
                            "looked", "full_sweeps"):
                    assert got[key] == r[key], (n, closing, fresh, key)
                gpath, gcost, _ = eng.tour_store(0)
                assert np.array_equal(gpath, path) and close_enough(
                    mode, gcost, r["cost"], c, r["two_opt_sweeps"] + r["or_sweeps"] + r["three_sweeps"],
                    r["two_opt_moves"] + r["or_moves"] + r["three_moves"]), (n, closing, fresh)
                assert np.array_equal(sets_of(eng, 0), awake) and not awake.any()
                info = eng.info()
                assert (info["dl_looked"], info["dl_full_sweeps"]) == (r["looked"], r["full_sweeps"])
                # the plain families' words as tspgpu_tour_local_search_nl3 leaves them
                assert (info["or_nl_sweeps"], info["or_nl_moves"], info["or_nl_rounds"]) == (r["or_sweeps"], r["or_moves"], r["rounds"])
                assert (info["three_nl_sweeps"], info["three_nl_moves"], info["three_nl_phases"]) == \
                    (r["three_sweeps"], r["three_moves"], r["three_phases"])
                cost = gcost
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["u16", "mf_euc"])
def test_gpu_closing_phase_ends_where_the_plain_phase_does(mode):
    """consequence (b) on the device, with existing code as the oracle: after every closing phase and descent the plain _once
    entry point of the family (of all three behind a descent) accepts nothing on the stored tour"""
    for n in SIZES + (1002,):
        xy, kind = (G2.tsplib_points("pr1002"), 0) if n == 1002 else points_for(mode, n, 6)
        eng = engine_for(mode, xy, kind)
        eng.neighbours_build(K)
        once = (lambda p, c: eng.two_opt_nl_once(p, c), lambda p, c: eng.or_opt_nl_once(p, c), lambda p, c: eng.three_opt_nl_once(p, c, W))
        start = random_tour(n, np.random.default_rng(n)) if n != 1002 else O.nn_tour(O.cost_matrix(xy), 0)[0]
        for f in range(3):
            eng.tour_load(1, start)
            s, m, looked, rc = dl_call(eng, f, 1, 1)
            path, cost, _ = eng.tour_store(1)
            assert rc == 0 and s >= 1 and not eng.tour_awake(1, f).any()
            assert len(once[f](path.copy(), cost)[1]) == 0, (n, f)
        eng.tour_load(1, start)
        r = eng.tour_local_search_nl3_dl(1, W, 1)
        path, cost, _ = eng.tour_store(1)
        for f in range(3):
            assert len(once[f](path.copy(), cost)[1]) == 0, (n, f)
        assert r["full_sweeps"] >= 3 and not sets_of(eng, 1).any()
        eng.close()


@pytest.mark.gpu
def test_gpu_windows():
    """everything asleep but one node: at position 0, at position n - 1, and node 0 -- the 2-opt and the 3-opt look at one unit,
    Or-opt at the three whose window holds it (fewer where windows coincide cannot happen at n >= 8: three distinct
    units); the result is the model's.  And the stored case: a rejected candidate inside an accepted reversal stays looked at"""
    for n in (8, 9, 64, 257):
        c, start = int_case(n, 2)
        eng = engine_for("u16", costs=c)
        eng.neighbours_build(K)
        nodes, _ = model_lists(K, costs=c)
        _, order = tour_from_zero(start)
        for node in (order[0], order[n - 1], 0):
            for f in range(3):
                eng.tour_load(0, start)
                eng.tour_sleep(0)
                eng.tour_wake(0, [node])
                awake = np.zeros(3 * n, np.uint8)
                awake[[node, n + node, 2 * n + node]] = 1
                assert np.array_equal(sets_of(eng, 0), awake)
                path, cost = start.copy(), tour_cost(start, c)
                r = model_dl_sweep(f, path, cost, awake, nodes, W, costs=c)
                assert r["looked"] == (3 if f == 1 else 1)
                assert dl_call(eng, f, 0, 0, 1) == (1, r["moves"], r["looked"], 0), (n, node, f)
                got, gcost, _ = eng.tour_store(0)
                assert np.array_equal(got, path) and gcost == r["cost"] and np.array_equal(sets_of(eng, 0), awake), (n, node, f)
        eng.close()
    case = json.load(open(GOLDEN))["rejected_inside_reversal"]
    n = case["n"]
    rng = np.random.default_rng(case["seed"])
    xy = rng.integers(0, 1000, (n, 2)).astype(np.float64)
    start = random_tour_from(rng, n)
    assert digest(start) == case["start_sha256"]
    eng = engine_for("mf_euc", xy, 0)
    eng.neighbours_build(case["K"])
    nodes, _ = model_lists(case["K"], xy=xy)
    eng.tour_load(0, start)
    path, awake, cost = start.copy(), all_awake(n), eng.tour_store(0)[1]
    r = model_dl_sweep(0, path, cost, awake, nodes, W, xy=xy)
    assert eng.tour_two_opt_nl_dl(0, 0, 1) == (1, r["moves"], n, 0)
    a, b = case["rejected"]
    assert awake[a] and awake[start[a]] and np.array_equal(sets_of(eng, 0), awake)
    r = model_dl_sweep(0, path, r["cost"], awake, nodes, W, xy=xy)
    assert r["Q"][a]                                                # rejected, inside a reversal that was applied: looked at again
    assert eng.tour_two_opt_nl_dl(0, 0, 1) == (1, r["moves"], r["looked"], 0)
    assert np.array_equal(eng.tour_store(0)[0], path) and np.array_equal(sets_of(eng, 0), awake)
    eng.close()


def random_tour_from(rng, n):
    perm = rng.permutation(n)
    path = np.empty(n, np.int32)
    path[perm] = np.roll(perm, -1)
    return path


def check_slot_serves_the_other_calls(eng, slot, path, cost, c, nodes):
    """the slot's invariants as tests/test_three_opt_nl.py checks them: a reference 2-opt sweep (edge costs by position) and the
    plain neighbour-list 2-opt and Or-opt sweeps (successors and edge costs by node) equal their models on the stored tour"""
    eng.tour_copy(slot + 1, slot)
    w = path.copy()
    d, wc, _ = O.two_opt_once(c, w, cost)
    assert eng.tour_two_opt(slot + 1, max_sweeps=1) == (1, 0)
    got, gcost, gdelta = eng.tour_store(slot + 1)
    assert np.array_equal(got, w) and (gcost, gdelta) == (wc, d)
    for call, model in ((eng.tour_two_opt_nl, model_sweep), (eng.tour_or_opt_nl, model_or_sweep)):
        eng.tour_copy(slot + 1, slot)
        w = path.copy()
        m = model(w, cost, nodes, costs=c)
        assert call(slot + 1, max_sweeps=1) == (1, len(m["moves"]), 0)
        got, gcost, _ = eng.tour_store(slot + 1)
        assert np.array_equal(got, w) and gcost == m["cost"]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["u16", "f64", "mf_euc"])
def test_gpu_kick(mode):
    """tspgpu_tour_kick against the slice restatement order[:i+1] + B + A + order[k+1:], at the ends of the tour and with
    segments of one node, in both slot directions; the cost by the stated formula; the six nodes awake in all three sets;
    the slot still serves the other slot calls"""
    rotated = False
    for n in (8, 9, 65, 300):
        xy, kind = points_for(mode, n, 8)
        c = weight_matrix(xy, kind)
        eng = engine_for(mode, xy, kind)
        eng.neighbours_build(K)
        nodes, _ = model_lists(K, costs=c)
        cases = [(0, 2, 5), (1, 3, n - 1), (0, 3, n - 1), (2, 3, 4), (0, 1, 2), (n - 3, n - 2, n - 1), (1, n // 2, n - 2)]
        for flipped in (False, True):
            for i, j, k in cases:
                eng.tour_load(0, random_tour(n, np.random.default_rng(n + i + k)))
                if flipped:
                    d, cell0 = turn_slot_backward(eng, 0, c)
                    assert d == -1
                    rotated |= cell0 != 0
                before, cost, _ = eng.tour_store(0)
                eng.tour_sleep(0)
                eng.tour_kick(0, i, j, k)
                _, o = tour_from_zero(before)
                new = o[:i + 1] + o[j + 1:k + 1] + o[i + 1:j + 1] + o[k + 1:]
                want = np.empty(n, np.int32)
                want[new] = np.roll(new, -1)
                a, a1, b, b1, cc, c1 = o[i], o[i + 1], o[j], o[j + 1], o[k], o[(k + 1) % n]
                delta = ((c[a][b1] + c[cc][a1]) + c[b][c1]) - ((c[a][a1] + c[b][b1]) + c[cc][c1])
                got, gcost, gdelta = eng.tour_store(0)
                assert np.array_equal(got, want) and (gcost, gdelta) == (cost + delta, delta), (n, flipped, i, j, k)
                awake = np.zeros(3 * n, np.uint8)
                for v in (a, a1, b, b1, cc, c1):
                    awake[[v, n + v, 2 * n + v]] = 1
                assert np.array_equal(sets_of(eng, 0), awake)
                mpath, mawake = before.copy(), np.zeros(3 * n, np.uint8)
                assert model_kick(mpath, cost, i, j, k, mawake, costs=c) == (gcost, gdelta)
                assert np.array_equal(mpath, want) and np.array_equal(mawake, awake)
                check_slot_serves_the_other_calls(eng, 0, got, gcost, c, nodes)
        for bad in ((-1, 2, 3), (2, 2, 3), (3, 2, 5), (1, 2, n), (1, 3, 3)):
            assert eng.L.tspgpu_tour_kick(eng.ctx, 0, *bad) == 3
        assert eng.L.tspgpu_tour_kick(eng.ctx, 7, 1, 2, 3) == 9 and eng.L.tspgpu_tour_kick(None, 0, 1, 2, 3) == 14
        eng.close()
    assert rotated


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["u16", "mf_euc"])
def test_gpu_golden_loop(mode):
    """the golden loop on the device: the descent with looks from NN(0) on pr1002 (closing 1 and 0), then 20 kicks on the slot,
    each followed by the descent with closing = 0 -- per iteration cost, tour, sweeps, moves, looked and full sweeps"""
    g = json.load(open(GOLDEN))["pr1002"]
    xy = G2.tsplib_points("pr1002")
    eng = engine_for(mode, xy, 0)
    eng.neighbours_build(g["K"])
    start = G2.nn_from(xy, 0)[0]
    assert digest(start) == g["start_sha256"]

    def check(r, want, what):
        path, cost, _ = eng.tour_store(0)
        for key in ("two_opt_sweeps", "two_opt_moves", "or_sweeps", "or_moves", "rounds", "three_sweeps", "three_moves", "three_phases",
                    "looked", "full_sweeps"):
            assert r[key] == want[key], (what, key)
        assert cost == want["cost"] and digest(path) == want["path_sha256"], what

    for closing in (1, 0):
        eng.tour_load(0, start)
        check(eng.tour_local_search_nl3_dl(0, g["W"], closing), g["descent_closing%d" % closing], closing)
    path = start.copy()
    r = eng.local_search_nl3_dl(path, g["W"], 1)        # the host-tour form recomputes the cost and ends at the same tour
    assert r["cost"] == g["descent_closing1"]["cost"] and digest(path) == g["descent_closing1"]["path_sha256"]
    eng.tour_load(0, start)
    eng.tour_local_search_nl3_dl(0, g["W"], 0)
    for it, (i, j, k) in zip(g["iterations"], g["kicks"]):
        eng.tour_kick(0, i, j, k)
        assert eng.tour_store(0)[2] == it["kick_delta"]
        check(eng.tour_local_search_nl3_dl(0, g["W"], 0), it, (i, j, k))
    eng.close()


@pytest.mark.gpu
def test_gpu_state_rules():
    """a plain slot call between two _dl calls leaves all awake; tour_copy copies the sets; tour_load resets them; an empty set
    runs no sweep without closing and exactly one full sweep with it; wake with a bad node changes nothing"""
    n = 200
    c, start = int_case(n, 3)
    eng = engine_for("u16", costs=c)
    eng.neighbours_build(K)
    eng.tour_load(0, start)
    assert sets_of(eng, 0).all()                                    # loaded: all awake
    eng.tour_sleep(0)
    eng.tour_wake(0, [3, 10, 77])
    assert eng.tour_two_opt_nl_dl(0, 0, 1)[2] == 3                  # three units looked at
    eng.tour_wake(0, [5, 150])
    sets = sets_of(eng, 0)
    assert not sets.all() and sets.any()
    eng.tour_copy(3, 0)
    assert np.array_equal(sets_of(eng, 3), sets)                    # copied with the tour
    bad = np.array([1, n], np.int32)
    assert eng.L.tspgpu_tour_wake(eng.ctx, 0, bad.ctypes.data, 2) == 3
    assert np.array_equal(sets_of(eng, 0), sets)
    eng.tour_store(0)                                               # (reading changes nothing)
    assert np.array_equal(sets_of(eng, 0), sets)
    assert eng.tour_or_opt_nl(0, max_sweeps=1)[0] == 1              # a plain slot call: every node wakes
    assert sets_of(eng, 0).all() and np.array_equal(sets_of(eng, 3), sets)
    assert eng.tour_two_opt_nl_dl(0, 0, 1)[2] == n                  # ... so the next sweep with looks is full
    eng.tour_load(3, start)
    assert sets_of(eng, 3).all()                                    # loaded again: reset
    for f in range(3):
        eng.tour_load(0, start)
        eng.tour_sleep(0)
        assert not sets_of(eng, 0).any()
        before = eng.tour_store(0)
        assert dl_call(eng, f, 0, 0) == (0, 0, 0, 0) and same_store(before, eng.tour_store(0))
        eng.tour_copy(1, 0)
        s, m, rc = plain_call(eng, f, 1, 1)
        assert dl_call(eng, f, 0, 1, 1) == (1, m, n, 0) and same_store(eng.tour_store(0), eng.tour_store(1))
        assert (eng.info()["dl_looked"], eng.info()["dl_full_sweeps"]) == (n, 1)
    eng.tour_sleep(0)
    eng.tour_wake(0)
    assert sets_of(eng, 0).all()
    eng.close()


@pytest.mark.gpu
def test_gpu_queue_above_the_sweep_grid():
    """more looked units than one pass of the fixed sweep grid holds: the grid-stride loop takes a second pass.  Uniform-random
    points, matrix-free, two sweeps per family against the plain slot calls (the first) and the model (the second)"""
    import travellingsalesmanoptimization_amd as T
    eng = T.Engine(0)
    wgs = 0
    eng.set_option(T.OPT_MATRIX_FREE, 1)
    xy = np.random.default_rng(99).integers(0, 30000, (16, 2)).astype(np.float64)
    eng.set_points(xy)
    eng.build_costs()
    wgs = eng.info()["dl_max_wgs"]
    assert wgs > 0
    n = 8 * wgs + 77                                                # above a pass of every family (8, 4 and 4 units per workgroup)
    assert n <= 20000, "the sweep grid of this chip asks for a larger instance than this test was sized for"
    xy = np.random.default_rng(99).integers(0, 30000, (n, 2)).astype(np.float64)
    eng.set_points(xy)
    eng.build_costs()
    eng.neighbours_build(K)
    nodes, _ = model_lists(K, xy=xy)
    start = G2.stripe_tour(xy)
    for f in range(3):
        eng.tour_load(0, start)
        eng.tour_copy(1, 0)
        s, m, rc = plain_call(eng, f, 1, 1)
        assert dl_call(eng, f, 0, 0, 1) == (1, m, n, 0) and same_store(eng.tour_store(0), eng.tour_store(1))
        path, cost, _ = eng.tour_store(0)
        awake = sets_of(eng, 0)
        want = path.copy()
        r = model_dl_sweep(f, want, cost, awake, nodes, W, xy=xy)
        assert dl_call(eng, f, 0, 0, 1) == (1, r["moves"], r["looked"], 0), f
        got, gcost, _ = eng.tour_store(0)
        assert np.array_equal(got, want) and gcost == r["cost"] and np.array_equal(sets_of(eng, 0), awake), f
    eng.close()


@pytest.mark.gpu
def test_gpu_refusals_deadline_and_memory_across_instances():
    """the codes of the section; a _dl call after tspgpu_set_points answers 9 with the invalidation text; the look memory
    follows the instance and the slots: a new instance drops it, more slots grow it with the sets kept"""
    import travellingsalesmanoptimization_amd as T
    n = 120
    xy, kind = points_for("u16", n, 1)
    eng = engine_for("u16", xy, kind)
    L, ctx = eng.L, eng.ctx
    eng.tour_load(0, random_tour(n, np.random.default_rng(1)))
    assert L.tspgpu_tour_two_opt_nl_dl(ctx, 0, 1, -1, -1.0, None, None, None) == 9 and b"tspgpu_neighbours_build" in L.tspgpu_last_error(ctx)
    eng.neighbours_build(K)
    assert L.tspgpu_tour_three_opt_nl_dl(ctx, 0, 0, 1, -1, -1.0, None, None, None) == 3
    assert L.tspgpu_tour_three_opt_nl_dl(ctx, 0, 17, 1, -1, -1.0, None, None, None) == 3
    assert L.tspgpu_tour_local_search_nl3_dl(ctx, 0, 17, 1, -1.0, *[None] * 10) == 3
    assert L.tspgpu_tour_local_search_nl3_dl(ctx, 0, -1, 1, -1.0, *[None] * 10) == 3
    assert L.tspgpu_tour_two_opt_nl_dl(ctx, 5, 1, -1, -1.0, None, None, None) == 9
    assert L.tspgpu_tour_awake(ctx, 0, 3, None, None) == 3 and L.tspgpu_tour_awake(ctx, 9, 0, None, None) == 9
    assert L.tspgpu_tour_sleep(ctx, 9) == 9 and L.tspgpu_tour_wake(ctx, 9, None, -1) == 9
    # a deadline that has passed: 4, nothing ran, the tour is valid
    before = eng.tour_store(0)
    assert eng.tour_local_search_nl3_dl(0, W, 1, time_left_s=0.0)["rc"] == 4 and same_store(before, eng.tour_store(0))
    # the descent without a 3-opt phase is rule 8
    r = eng.tour_local_search_nl3_dl(0, 0, 1)
    assert r["three_phases"] == 0 and r["three_sweeps"] == 0 and r["rc"] == 0 and not sets_of(eng, 0)[:2 * n].any()
    # more slots: the sets of slot 0 survive the growth, the new slots are all awake
    eng.tour_sleep(0)
    eng.tour_wake(0, [3])
    eng.tour_nn(40, 0)
    assert sets_of(eng, 0).sum() == 3 and sets_of(eng, 40).all()
    assert eng.tour_two_opt_nl_dl(40, 0, 1)[2] == n
    # a new cost source: the lists are invalidated, the slots emptied
    eng.set_points(xy, kind)
    eng.build_costs()
    assert L.tspgpu_tour_two_opt_nl_dl(ctx, 0, 1, -1, -1.0, None, None, None) == 9 and b"invalidated" in L.tspgpu_last_error(ctx)
    eng.neighbours_build(K)
    assert L.tspgpu_tour_two_opt_nl_dl(ctx, 0, 1, -1, -1.0, None, None, None) == 9      # no tour in the slot
    # a smaller instance through the same context, then the first again: the look memory is the new instance's
    for m in (9, n):
        xy2, kind2 = points_for("u16", m, 2)
        eng.set_points(xy2, kind2)
        eng.build_costs()
        eng.neighbours_build(K)
        c2 = weight_matrix(xy2, kind2)
        nodes, _ = model_lists(K, costs=c2)
        path = random_tour(m, np.random.default_rng(m))
        eng.tour_load(0, path)
        assert sets_of(eng, 0).all()
        r = model_dl_descent(path, tour_cost(path, c2), all_awake(m), nodes, W, 1, costs=c2)
        got = eng.tour_local_search_nl3_dl(0, W, 1)
        assert (got["looked"], got["full_sweeps"]) == (r["looked"], r["full_sweeps"])
        gpath, gcost, _ = eng.tour_store(0)
        assert np.array_equal(gpath, path) and gcost == r["cost"]
    eng.close()


@pytest.mark.gpu
def test_host_binary_runs_the_descent_with_looks():
    """TSP_DONT_LOOK=1 with the three switches ends at the golden's closing = 1 cost for pr1002; bad values are refused; alone
    it only warns"""
    g = json.load(open(GOLDEN))["pr1002"]
    data = os.path.join(ROOT, "tests", "golden", "data", "pr1002.tsp")
    env = {"TSP_OR_OPT": "1", "TSP_OR_OPT_NEIGHBOURS": str(g["K"]), "TSP_3OPT_WIDTH": str(g["W"]), "TSP_DONT_LOOK": "1"}
    args = ("-f", data, "-alg", "GREEDY", "-q")
    for k in ("TSP_3OPT_WIDTH", "TSP_DONT_LOOK"):
        os.environ.pop(k, None)
    code, out, err = run_tsp(*args, env_set=env)
    assert code == 0 and out == "Cost: %.2f" % g["descent_closing1"]["cost"], (out, err)
    assert run_tsp(*args, env_set=dict(env, TSP_DONT_LOOK="0"))[1] == "Cost: %.2f" % g["plain_descent"]["cost"]
    for bad in ("2", "x", "-1", ""):
        code, out, err = run_tsp(*args, env_set=dict(env, TSP_DONT_LOOK=bad))
        assert code != 0 and "TSP_DONT_LOOK" in err and "expected 0 or 1" in err, bad
    plain = run_tsp(*args)
    code, out, err = run_tsp(*args[:-1], env_set={"TSP_DONT_LOOK": "1"})
    assert code == 0 and "TSP_DONT_LOOK=1 has no effect" in out + err
    assert run_tsp(*args, env_set={"TSP_DONT_LOOK": "1"})[:2] == plain[:2]
