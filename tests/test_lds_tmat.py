"""The TM instantiations of k_lds2opt (csrc/tspgpu_lds2opt.inc: the shaped descent that fetches the rows a move brings to a
workgroup from a tour-ordered copy of the matrix in device memory, kept up to date by the workgroups that hold the rows)
against the shaped kernel that reloads from the matrix (option 88), the one-launch-per-sweep path, the CPU oracle and the
golden vectors: the same moves, sweep counts and tours, bit for bit.  And the copy itself (tspgpu_debug_tmat) behind
launches capped at a few sweeps and at the optimum: tmat[x][q] == c[x][node at cell q], the cell of x poisoned."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPT_LP_NO_TMAT = 88         # undocumented: 1 = the shaped k_lds2opt that reloads moved rows from the matrix
HIST = 4096
POISON = 16383


def fx(O, v):
    return f"{O.fnv1a(v):016x}"


def perm_tour(n, seed):
    """a seeded random permutation tour as a successor array: long reversals, both arc choices, ranges across the array end"""
    perm = np.random.RandomState(seed).permutation(n)
    succ = np.empty(n, dtype=np.int32)
    succ[perm] = np.roll(perm, -1)
    return succ


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
def perm_descent(O, points):
    """the CPU oracle's descent from the permutation start at n = 1024, once: (start, sweeps, cost, local optimum)"""
    c = O.cost_matrix(points[(1024, 1)])
    start = perm_tour(1024, 7)
    succ = start.copy()
    sweeps, cost = O.two_opt(c, succ)
    return start, sweeps, cost, succ


def load(eng, T, xy):
    eng.set_option(T.OPT_ELEM, 3); eng.set_option(T.OPT_KERNEL, 0)
    eng.set_points(xy); eng.build_costs()


def path_mode(eng, T, path):
    """tmat: the default where a shape is instantiated; mat: the hook; sweep: one launch per sweep"""
    eng.set_option(OPT_LP_NO_TMAT, 1 if path == "mat" else 0)
    eng.set_option(T.OPT_PERSIST, 0 if path == "sweep" else 2)


def descend(eng, T, path):
    """NN(0) -> 2-opt local optimum; (sweeps, cost, tour, a, b, delta, info)"""
    path_mode(eng, T, path)
    succ, _ = eng.nn_tour(0)
    eng.set_option(T.OPT_HISTORY, HIST)
    cost, sweeps, rc = eng.two_opt(succ)
    assert rc == 0
    a, b, d = eng.history(HIST)
    return sweeps, cost, succ, a.copy(), b.copy(), d.copy(), eng.info()


@pytest.mark.parametrize("seed", [1, 123])
def test_three_paths_move_by_move(eng, T, O, points, seed):
    """rows from the tour-ordered copy, rows from the matrix, one launch per sweep: identical sweep count, cost, successor
    array and (a, b, delta) of every sweep; persist_tmat reports the first only"""
    load(eng, T, points[(1024, seed)])
    runs = {p: descend(eng, T, p) for p in ("tmat", "mat", "sweep")}
    tm = runs["tmat"]
    assert [(runs[p][6]["persist"], runs[p][6]["persist_shaped"], runs[p][6]["persist_tmat"]) for p in ("tmat", "mat", "sweep")] == \
        [(1, 1, 1), (1, 1, 0), (0, 0, 0)]
    assert len(tm[3]) == tm[0] and tm[3][-1] == -1 and O.valid_tour(tm[2])
    for p in ("mat", "sweep"):
        r = runs[p]
        assert (r[0], r[1]) == (tm[0], tm[1]), p
        assert np.array_equal(r[2], tm[2]), p
        for i in (3, 4, 5):
            bad = np.nonzero(r[i] != tm[i])[0] if len(r[i]) == len(tm[i]) else [-1]
            assert len(bad) == 0, (p, i, bad[:4])


def test_long_reversals_against_the_oracle(eng, T, O, points, perm_descent):
    """from a random permutation tour (M up to n/2, both arcs, wraps, mirrored chunks): the CPU oracle's descent"""
    start, osweeps, ocost, osucc = perm_descent
    load(eng, T, points[(1024, 1)])
    path_mode(eng, T, "tmat")
    succ = start.copy()
    cost, sweeps, rc = eng.two_opt(succ)
    assert rc == 0 and eng.info()["persist_tmat"] == 1
    assert osweeps > 500
    assert (sweeps, cost) == (osweeps, ocost) and np.array_equal(succ, osucc)


def check_tmat(eng, c, n):
    """the copy behind the last launch against c[x][node at cell q]; the cells come from the poisoned cell of every row (the
    cell of the row's own node) and must be the tour that tour_store returns, in one of its two directions"""
    tm = np.empty((n, n), dtype=np.uint16)
    eng._ck(eng.L.tspgpu_debug_tmat(eng.ctx, tm.ctypes.data, tm.size))
    succ, _, _ = eng.tour_store(0)
    rows, cells = np.nonzero(tm == POISON)
    assert np.array_equal(rows, np.arange(n)), "one poisoned cell a row"
    ord_ = np.empty(n, dtype=np.int64)
    ord_[cells] = rows
    assert np.array_equal(np.sort(cells), np.arange(n)), "every cell holds one node"
    nxt, prv = np.roll(ord_, -1), np.roll(ord_, 1)
    assert np.array_equal(succ[ord_], nxt) or np.array_equal(succ[ord_], prv), "the cells are not the slot's tour"
    want = c[:, ord_].astype(np.uint16)
    want[rows, cells] = POISON
    bad = np.argwhere(tm != want)
    assert len(bad) == 0, (len(bad), bad[:4])


@pytest.mark.parametrize("start", ["nn", "perm"])
def test_the_copy_itself(eng, T, O, points, perm_descent, start):
    """launches capped at 1, 2, 3, 17 and 50 sweeps and run to the optimum: the whole copy behind each"""
    xy = points[(1024, 1)]
    c = O.cost_matrix(xy)
    assert c.max() < POISON
    load(eng, T, xy)
    path_mode(eng, T, "tmat")
    for cap in (1, 2, 3, 17, 50, -1):
        if start == "nn":
            eng.tour_nn(0, 0)
        else:
            eng.tour_load(0, perm_descent[0])
        sweeps, rc = eng.tour_two_opt(0, max_sweeps=cap)
        assert rc == 0 and eng.info()["persist_tmat"] == 1 and (cap < 0 or sweeps == cap)
        check_tmat(eng, c, 1024)
    if start == "perm":
        assert sweeps == perm_descent[1]


def test_continuation(eng, T, O, points, golden):
    """50 capped sweeps, then on to the optimum (the second launch fills the copy again) = one go"""
    load(eng, T, points[(1024, 1)])
    g = golden["random"]["n1024_s1"]["two_opt"]
    path_mode(eng, T, "tmat")
    eng.tour_nn(0, 0)
    sw, rc = eng.tour_two_opt(0, max_sweeps=50)
    assert (sw, rc) == (50, 0) and eng.info()["persist_tmat"] == 1
    sw2, rc = eng.tour_two_opt(0)
    assert rc == 0 and eng.info()["persist_tmat"] == 1
    two = eng.tour_store(0)
    eng.tour_nn(0, 0)
    sw1, rc = eng.tour_two_opt(0)
    one = eng.tour_store(0)
    assert rc == 0 and sw1 == 50 + sw2 and np.array_equal(one[0], two[0]) and one[1:] == two[1:]
    assert (sw1, one[1], fx(O, one[0])) == (g["sweeps"], g["final_cost"], g["final_fnv"])


def test_flagship_shape(eng, T, O, points):
    """n = 4096 (16 edges a workgroup): the two starts with the fewest and the two with the most sweeps among the golden's
    first 64 -- sweeps, cost and tour hash of the compiled reference"""
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden_n4096_multistart.json")))
    assert (g["n"], g["seed"]) == (4096, 123)
    first = sorted(g["starts"], key=lambda e: e["start"])[:64]
    by_sweeps = sorted(first, key=lambda e: (e["sweeps"], e["start"]))
    load(eng, T, points[(4096, 123)])
    path_mode(eng, T, "tmat")
    for e in by_sweeps[:2] + by_sweeps[-2:]:
        eng.tour_nn(0, e["start"])
        sweeps, rc = eng.tour_two_opt(0)
        info = eng.info()
        assert rc == 0 and (info["persist"], info["persist_shaped"], info["persist_tmat"]) == (1, 1, 1)
        p, cost, _ = eng.tour_store(0)
        assert (sweeps, cost, fx(O, p)) == (e["sweeps"], e["cost"], e["fnv"]), e["start"]
