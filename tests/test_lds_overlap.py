"""The shaped k_lds2opt with its packed deltas carried under a bias of 0x8000 a half (csrc/tspgpu_lds2opt.inc, the row loop:
one three-operand add a register, unsigned packed minimum; csrc/tspgpu_lds_tmat.h: pk_bias, pk_biased), with rows from the
tour-ordered copy (TM) and with rows reloaded from the matrix (option 88), against the one-launch-per-sweep path, the CPU
oracle and the golden vectors: the same moves, sweep counts and tours, bit for bit.  n = 1024 with 4 edges a workgroup is
the smallest shaped form and the one in which short moves touch a workgroup boundary most often; the tour-ordered copy is
checked whole behind capped launches from a permutation start.  (tests/test_packed_limits.py pins the same kernels at the
cost limit 16383, where the bias argument is tight.)"""
import json
import os

import numpy as np
import pytest

from test_lds_tmat import HIST, OPT_LP_NO_TMAT, check_tmat, fx, perm_tour

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def points(O):
    """every point set of this file, drawn before its first GPU call (the HIP runtime draws from rand() while it comes up)"""
    return {(n, s): O.random_points(n, s) for n, s in ((1024, 1), (1024, 123), (4096, 123))}


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
    eng.set_option(OPT_LP_NO_TMAT, 0); eng.set_option(T.OPT_PERSIST, 1); eng.set_option(T.OPT_HISTORY, 0)


@pytest.fixture(scope="module")
def perm_descents(O, points):
    """the CPU oracle's descent from the permutation start at n = 1024, once a seed: (start, sweeps, cost, local optimum)"""
    out = {}
    for seed in (1, 123):
        c = O.cost_matrix(points[(1024, seed)])
        start = perm_tour(1024, 7)
        succ = start.copy()
        sweeps, cost = O.two_opt(c, succ)
        out[seed] = (start, sweeps, cost, succ)
    return out


def load(eng, T, xy):
    eng.set_option(T.OPT_ELEM, 3); eng.set_option(T.OPT_KERNEL, 0)
    eng.set_points(xy); eng.build_costs()


PATHS = ("tmat", "mat", "sweep")


def path_mode(eng, T, path):
    """tmat: the default; mat: rows reloaded from the matrix (option 88); sweep: one launch per sweep"""
    eng.set_option(OPT_LP_NO_TMAT, 1 if path == "mat" else 0)
    eng.set_option(T.OPT_PERSIST, 0 if path == "sweep" else 2)


def descend(eng, T, path, start):
    """start (None: NN(0)) -> 2-opt local optimum; (sweeps, cost, tour, a, b, delta, info)"""
    path_mode(eng, T, path)
    succ = eng.nn_tour(0)[0] if start is None else start.copy()
    eng.set_option(T.OPT_HISTORY, HIST)
    cost, sweeps, rc = eng.two_opt(succ)
    assert rc == 0
    a, b, d = eng.history(HIST)
    return sweeps, cost, succ, a.copy(), b.copy(), d.copy(), eng.info()


@pytest.mark.parametrize("start", ["nn", "perm"])
@pytest.mark.parametrize("seed", [1, 123])
def test_every_path_move_by_move(eng, T, O, points, perm_descents, seed, start):
    """identical sweep count, cost, successor array and (a, b, delta) of every sweep on every path; from the permutation start
    (long reversals, both arcs, ranges across the array end) also the CPU oracle's descent"""
    load(eng, T, points[(1024, seed)])
    st = None if start == "nn" else perm_descents[seed][0]
    runs = {p: descend(eng, T, p, st) for p in PATHS}
    ref = runs["tmat"]
    assert [(runs[p][6]["persist"], runs[p][6]["persist_shaped"], runs[p][6]["persist_tmat"]) for p in PATHS] == [(1, 1, 1), (1, 1, 0), (0, 0, 0)]
    assert len(ref[3]) == min(ref[0], HIST) and O.valid_tour(ref[2])
    for p in PATHS[1:]:
        r = runs[p]
        assert (r[0], r[1]) == (ref[0], ref[1]), p
        assert np.array_equal(r[2], ref[2]), p
        for i in (3, 4, 5):
            bad = np.nonzero(r[i] != ref[i])[0] if len(r[i]) == len(ref[i]) else [-1]
            assert len(bad) == 0, (p, i, bad[:4])
    if start == "perm":
        _, osweeps, ocost, osucc = perm_descents[seed]
        assert (ref[0], ref[1]) == (osweeps, ocost) and np.array_equal(ref[2], osucc)


def test_the_copy_itself(eng, T, O, points, perm_descents):
    """launches capped at 1, 2, 3, 17 and 50 sweeps and run to the optimum, from the permutation start: the whole copy behind
    each (a row of it is what the row loop read: a wrong minimum would have moved other rows)"""
    xy = points[(1024, 123)]
    c = O.cost_matrix(xy)
    assert c.max() < 16383
    load(eng, T, xy)
    path_mode(eng, T, "tmat")
    for cap in (1, 2, 3, 17, 50, -1):
        eng.tour_load(0, perm_descents[123][0])
        sweeps, rc = eng.tour_two_opt(0, max_sweeps=cap)
        assert rc == 0 and eng.info()["persist_tmat"] == 1 and (cap < 0 or sweeps == cap)
        check_tmat(eng, c, 1024)
    assert sweeps == perm_descents[123][1]


def test_continuation(eng, T, O, points, golden):
    """50 capped sweeps, then on to the optimum = one go = the golden, with rows from the copy and from the matrix"""
    load(eng, T, points[(1024, 1)])
    g = golden["random"]["n1024_s1"]["two_opt"]
    for path in ("tmat", "mat"):
        path_mode(eng, T, path)
        eng.tour_nn(0, 0)
        sw, rc = eng.tour_two_opt(0, max_sweeps=50)
        assert (sw, rc) == (50, 0) and eng.info()["persist_shaped"] == 1
        sw2, rc = eng.tour_two_opt(0)
        assert rc == 0
        two = eng.tour_store(0)
        eng.tour_nn(0, 0)
        sw1, rc = eng.tour_two_opt(0)
        one = eng.tour_store(0)
        assert rc == 0 and sw1 == 50 + sw2 and np.array_equal(one[0], two[0]) and one[1:] == two[1:]
        assert (sw1, one[1], fx(O, one[0])) == (g["sweeps"], g["final_cost"], g["final_fnv"]), path


def test_flagship_shape(eng, T, O, points):
    """n = 4096 (16 edges a workgroup, 8 rows a thread in the row loop): the golden start with the fewest sweeps among the first
    64, with rows from the copy and from the matrix, and start 0, the headline descent -- sweeps, cost and tour hash of the
    compiled reference"""
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden_n4096_multistart.json")))
    assert (g["n"], g["seed"]) == (4096, 123)
    first = sorted(g["starts"], key=lambda e: e["start"])[:64]
    e = sorted(first, key=lambda e: (e["sweeps"], e["start"]))[0]
    load(eng, T, points[(4096, 123)])
    for path in ("tmat", "mat"):
        path_mode(eng, T, path)
        eng.tour_nn(0, e["start"])
        sweeps, rc = eng.tour_two_opt(0)
        info = eng.info()
        assert rc == 0 and (info["persist"], info["persist_shaped"], info["persist_tmat"]) == (1, 1, 1 if path == "tmat" else 0)
        p, cost, _ = eng.tour_store(0)
        assert (sweeps, cost, fx(O, p)) == (e["sweeps"], e["cost"], e["fnv"]), (path, e["start"])
    path_mode(eng, T, "tmat")
    eng.tour_nn(0, 0)
    sweeps, rc = eng.tour_two_opt(0)
    p, cost, _ = eng.tour_store(0)
    assert rc == 0 and eng.info()["persist_tmat"] == 1
    assert (sweeps, cost, fx(O, p)) == (609, 488522.0, "891c70ef880aa369")
