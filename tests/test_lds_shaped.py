"""The shaped instantiations of k_lds2opt (csrc/tspgpu_lds2opt.inc: the plain packed descent compiled for
(n, edges per workgroup) = (4096, 16) and (1024, 4)) against the generic kernel of the same build (option 89), the
one-launch-per-sweep path and the golden vectors: same moves, same sweep count, same tour.  And the dispatch: every other
shape, the 32-bit form, the tabu and the VNS walk keep the generic code and their results."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPT_LP_GENERIC = 89         # undocumented: 1 = the generic k_lds2opt where a shaped instantiation exists
HIST = 4096


def fx(O, v):
    return f"{O.fnv1a(v):016x}"


@pytest.fixture(scope="module")
def points(O):
    """every point set of this file, drawn before its first GPU call (the HIP runtime draws from rand() while it comes up)"""
    return {(n, s): O.random_points(n, s) for n, s in ((1024, 1), (1024, 123), (4096, 123), (1000, 123), (2048, 123))}


@pytest.fixture(scope="module")
def T():
    import travellingsalesmanoptimization_amd as T
    return T


@pytest.fixture(scope="module")
def eng(points, T):
    e = T.Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def defaults(eng, T):
    yield
    eng.set_option(OPT_LP_GENERIC, 0); eng.set_option(T.OPT_PERSIST, 1); eng.set_option(T.OPT_PERSIST_EDGES, 0)
    eng.set_option(T.OPT_HISTORY, 0)


def load(eng, T, xy):
    eng.set_option(T.OPT_ELEM, 3); eng.set_option(T.OPT_KERNEL, 0)
    eng.set_points(xy); eng.build_costs()


def path_mode(eng, T, path):
    """shaped: the default where the shape is instantiated; generic: the hook; sweep: one launch per sweep"""
    eng.set_option(OPT_LP_GENERIC, 1 if path == "generic" else 0)
    eng.set_option(T.OPT_PERSIST, 0 if path == "sweep" else 2)


def descend(eng, T, path):
    """NN(0) -> 2-opt local optimum; (sweeps, cost, tour, a, b, delta, info)"""
    path_mode(eng, T, path)
    succ, nn_cost = eng.nn_tour(0)
    eng.set_option(T.OPT_HISTORY, HIST)
    cost, sweeps, rc = eng.two_opt(succ)
    assert rc == 0
    a, b, d = eng.history(HIST)
    return sweeps, cost, succ, a.copy(), b.copy(), d.copy(), eng.info(), nn_cost


@pytest.mark.parametrize("n,seed", [(1024, 1), (1024, 123), (4096, 123)])
def test_three_paths_move_by_move(eng, T, O, points, golden, n, seed):
    """shaped, generic and one launch per sweep: identical sweep count, cost, successor array and (a, b, delta) of every
    sweep; the golden result where the reference recorded one; persist_shaped reports the shaped run only"""
    load(eng, T, points[(n, seed)])
    runs = {p: descend(eng, T, p) for p in ("shaped", "generic", "sweep")}
    sh = runs["shaped"]
    assert sh[6]["persist"] == 1 and sh[6]["persist_shaped"] == 1 and sh[6]["persist_edges"] == (16 if n == 4096 else 4)
    assert runs["generic"][6]["persist"] == 1 and runs["generic"][6]["persist_shaped"] == 0
    assert runs["sweep"][6]["persist"] == 0 and runs["sweep"][6]["persist_shaped"] == 0
    assert len(sh[3]) == sh[0] and sh[3][-1] == -1 and O.valid_tour(sh[2])
    for p in ("generic", "sweep"):
        r = runs[p]
        assert (r[0], r[1]) == (sh[0], sh[1]), p
        assert np.array_equal(r[2], sh[2]), p
        for i in (3, 4, 5):
            bad = np.nonzero(r[i] != sh[i])[0] if len(r[i]) == len(sh[i]) else [-1]
            assert len(bad) == 0, (p, i, bad[:4])
    g = golden["random"].get(f"n{n}_s{seed}")
    if (n, seed) != (1024, 123):
        assert g is not None
    if g is not None:
        g = g["two_opt"]
        assert sh[7] == g["nn_cost"]
        assert (sh[0], sh[1], fx(O, sh[2])) == (g["sweeps"], g["final_cost"], g["final_fnv"])
        run = sh[7]
        for i, want in enumerate(g["trace"]):
            run += sh[5][i]
            assert run == want


def test_flagship_shape_other_trajectories(eng, T, O, points):
    """8 other descents at n = 4096 (the starts with the most and the fewest sweeps among the golden's first 64: both arc
    choices, ranges across workgroup boundaries, long reversals): sweeps, cost and tour hash of the compiled reference"""
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden_n4096_multistart.json")))
    assert (g["n"], g["seed"]) == (4096, 123)
    first = sorted(g["starts"], key=lambda e: e["start"])[:64]
    by_sweeps = sorted(first, key=lambda e: (e["sweeps"], e["start"]))
    picks = by_sweeps[:4] + by_sweeps[-4:]
    load(eng, T, points[(4096, 123)])
    path_mode(eng, T, "shaped")
    for e in picks:
        eng.tour_nn(0, e["start"])
        sweeps, rc = eng.tour_two_opt(0)
        info = eng.info()
        assert rc == 0 and info["persist"] == 1 and info["persist_shaped"] == 1
        p, cost, _ = eng.tour_store(0)
        assert (sweeps, cost, fx(O, p)) == (e["sweeps"], e["cost"], e["fnv"]), e["start"]


def test_state_write_back(eng, T, O, points, golden):
    """a capped launch leaves the tour state the next one continues from: 50 sweeps, then on to the optimum = one go; the
    shaped and the generic kernel agree on the state behind the cap"""
    load(eng, T, points[(1024, 1)])
    g = golden["random"]["n1024_s1"]["two_opt"]
    mid, end = {}, {}
    for p in ("shaped", "generic"):
        path_mode(eng, T, p)
        eng.tour_nn(0, 0)
        sw, rc = eng.tour_two_opt(0, max_sweeps=50)
        assert (sw, rc) == (50, 0) and eng.info()["persist_shaped"] == (1 if p == "shaped" else 0)
        mid[p] = eng.tour_store(0)
        sw2, rc = eng.tour_two_opt(0)
        assert rc == 0 and eng.info()["persist_shaped"] == (1 if p == "shaped" else 0)
        end[p] = (sw2,) + tuple(eng.tour_store(0))
    assert np.array_equal(mid["shaped"][0], mid["generic"][0]) and mid["shaped"][1:] == mid["generic"][1:]
    assert O.valid_tour(mid["shaped"][0])
    assert end["shaped"][0] == end["generic"][0] and np.array_equal(end["shaped"][1], end["generic"][1])
    assert end["shaped"][2:] == end["generic"][2:]
    assert (end["shaped"][2], fx(O, end["shaped"][1])) == (g["final_cost"], g["final_fnv"])
    assert end["shaped"][0] == g["sweeps"] - 50                     # (a call counts its own sweeps)


def test_dispatch_keeps_the_generic_kernel(eng, T, O, points, golden):
    """not shaped: n = 1000, n = 2048 (no instantiation), costs past 16 383 at n = 1024 (the 32-bit form), the tabu and the
    VNS walk at n = 1024 -- with the results they had"""
    # n = 1000: the golden descent
    load(eng, T, points[(1000, 123)])
    r = descend(eng, T, "shaped")
    g = golden["random"]["n1000_s123"]["two_opt"]
    assert r[6]["persist"] == 1 and r[6]["persist_shaped"] == 0
    assert (r[0], r[1], fx(O, r[2])) == (g["sweeps"], g["final_cost"], g["final_fnv"])
    # n = 2048: against one launch per sweep
    load(eng, T, points[(2048, 123)])
    r, s = descend(eng, T, "shaped"), descend(eng, T, "sweep")
    assert r[6]["persist"] == 1 and r[6]["persist_shaped"] == 0 and s[6]["persist"] == 0
    assert (r[0], r[1]) == (s[0], s[1]) and np.array_equal(r[2], s[2])
    assert np.array_equal(r[3], s[3]) and np.array_equal(r[4], s[4]) and np.array_equal(r[5], s[5])
    # n = 1024, the points scaled until the largest cost passes 16 383: unpacked 32-bit deltas
    xy = points[(1024, 1)] * 1.5
    c = O.cost_matrix(xy)
    assert c.max() > 16383
    load(eng, T, xy)
    r = descend(eng, T, "shaped")
    osucc, _ = O.nn_tour(c, 0)
    osweeps, ocost = O.two_opt(c, osucc)
    assert r[6]["persist"] == 1 and r[6]["persist_shaped"] == 0 and r[6]["persist_edges"] == 4
    assert (r[0], r[1]) == (osweeps, ocost) and np.array_equal(r[2], osucc)
    # n = 1024: tabu walk and VNS walk from the local optimum / from NN(7)
    xy = points[(1024, 1)]
    c = O.cost_matrix(xy)
    load(eng, T, xy)
    path_mode(eng, T, "shaped")
    seed0, _ = O.nn_tour(c, 0)
    O.two_opt(c, seed0)
    cost = O.tour_cost(c, seed0)
    oseed = seed0.copy()
    k = 40
    best, best_cost, final, trace = eng.tabu_search(seed0, cost, k, want_trace=True)
    assert eng.info()["persist"] == 1 and eng.info()["persist_shaped"] == 0
    obest, obc, ofinal, otrace = O.tabu_search(c, oseed, cost, k)
    assert np.array_equal(trace, otrace) and final == ofinal and np.array_equal(seed0, oseed)
    assert best_cost == obc and np.array_equal(best, obest)
    import ctypes
    libc = ctypes.CDLL(None)
    k = 6
    O.libc_srand(5)
    rv = np.array([libc.rand() for _ in range(64 * k + 4096)], dtype=np.int32)
    start, cost0 = O.nn_tour(c, 7)
    O.libc_srand(5)
    os_ = start.copy()
    obest, obc = O.vns(c, os_, cost0, k)
    path, best = start.copy(), start.copy()
    res = eng.vns_search(path, k, rv, best, cost0)
    assert eng.info()["persist"] == 1 and eng.info()["persist_shaped"] == 0
    assert (res["rc"], res["iterations"], res["kick_pending"]) == (0, k, 0)
    assert res["best_cost"] == obc and np.array_equal(best, obest) and np.array_equal(path, os_)
