"""The one-launch 2-opt kernels (k_lds2opt generic, shaped and TM, k_lds2opt_w, k_str2opt) at the limits of their narrow
arithmetic, and the shaped / TM instantiations on ties -- move by move against the CPU oracle (oracle/).

- packed 16-bit deltas: chosen when every off-diagonal cost is <= 16383; a delta then spans +-32766 in an s16;
- the packed tabu form: chosen when every cost is <= 8190; a valid delta (<= 16380) and a poisoned pair (>= 16386) are told
  apart by 16383;
- the exchange record of k_lds2opt and k_str2opt: the delta in 18 bits biased by 131072; uint16 cells up to 65534 give
  +-131068.
The caller matrices below are built so that those extremes occur: symmetric, integers, diagonal -1, the largest cell
exactly the limit M under test (`above`: M + 1, the other side of the threshold).  The CPU tests state on the oracle alone
that the extremes are reached; the device tests (-m gpu) compare every path that admits the instance with the oracle
and read from info() which kernel and which form (persist_packed) ran."""
import ctypes

import numpy as np
import pytest

N = 1024
HIST = 8192
PK16, PK8, U16 = 16383, 8190, 65534
OPT_LP_NO_TMAT, OPT_LP_GENERIC = 88, 89     # undocumented: see tests/test_lds_tmat.py, tests/test_lds_shaped.py

gpu = pytest.mark.gpu


# ------------------------------------------------------------------ the fixtures
def perm_tour(n, seed=7):
    """a seeded random permutation tour as a successor array: long reversals, both arc choices, ranges across the array end"""
    perm = np.random.RandomState(seed).permutation(n)
    succ = np.empty(n, dtype=np.int32)
    succ[perm] = np.roll(perm, -1)
    return succ


def _symmetric(cells):
    c = np.triu(cells.astype(np.float64), 1)
    c = c + c.T
    np.fill_diagonal(c, -1.0)
    return np.ascontiguousarray(c)


def two(n, M, seed=1):
    """cells drawn from {0, M}: ties everywhere, deltas in {0, +-M, +-2M}"""
    rng = np.random.default_rng(seed)
    return _symmetric(rng.integers(0, 2, size=(n, n)) * M)


def top(n, M, seed=1):
    """cells uniform in [M-3, M], about one in 16 set to 0: deltas within a few units of +-2M, mostly distinct"""
    rng = np.random.default_rng(seed)
    cells = rng.integers(M - 3, M + 1, size=(n, n))
    cells[rng.random((n, n)) < 1.0 / 16.0] = 0
    return _symmetric(cells)


def planted(n, M, flat, seed=1):
    """one zero-cost Hamiltonian cycle, every other cell exactly M (flat) or uniform in [M-3, M] -> (matrix, the cycle);
    the cycle is a local optimum of cost 0 from which every valid pair has delta 2M (flat) or >= 2(M-3)"""
    rng = np.random.default_rng(seed)
    cells = np.full((n, n), M) if flat else rng.integers(M - 3, M + 1, size=(n, n))
    c = _symmetric(cells)
    perm = rng.permutation(n)
    succ = np.empty(n, dtype=np.int32)
    succ[perm] = np.roll(perm, -1)
    idx = np.arange(n)
    c[idx, succ] = 0.0
    c[succ, idx] = 0.0
    return c, succ


def above(c, tour):
    """a copy with one pair that is no edge of `tour` raised from the maximum M to M + 1: the same instance on the other side
    of the threshold"""
    M = c.max()
    on_tour = np.zeros(c.shape, dtype=bool)
    idx = np.arange(len(tour))
    on_tour[idx, tour] = on_tour[tour, idx] = True
    i, j = np.argwhere((c == M) & ~on_tour)[0]
    out = c.copy()
    out[i, j] = out[j, i] = M + 1
    return out


def lattice(side, spacing=10.0):
    g = np.arange(side, dtype=np.float64) * spacing
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g), -1).reshape(-1, 2))


def doubled_points(half, seed=9):
    """`half` random integer points in [0, 50)^2, each taken twice: zero-length edges and many ties"""
    base = np.random.RandomState(seed).randint(0, 50, size=(half, 2)).astype(np.float64)
    return np.ascontiguousarray(np.concatenate([base, base]))


def small_matrix(n, seed=3):
    """entries in 1..9 (tests/test_gpu_parity.py::test_symmetric_caller_matrices' tie case)"""
    return _symmetric(np.random.default_rng(seed).integers(1, 10, size=(n, n)))


class Descent:
    """the oracle's descent from `start`: (a, b, delta) of every sweep (a = -1: the sweep that found nothing), the tour and
    its cost behind the last sweep"""

    def __init__(self, O, c, start, cap=-1):
        succ = start.copy()
        cost = O.tour_cost(c, succ)
        self.start, self.cost0 = start, cost
        a, b, d = [], [], []
        while cap < 0 or len(a) < cap:
            dd, cost, mv = O.two_opt_once(c, succ, cost)
            if dd >= -1e-7:
                a.append(-1); b.append(-1); d.append(0.0)
                break
            a.append(min(mv)); b.append(max(mv)); d.append(dd)
        self.a, self.b, self.d = np.array(a), np.array(b), np.array(d)
        self.sweeps, self.succ, self.cost = len(a), succ, cost


_cache = {}


def cached(key, make):
    """every matrix and every oracle run of this file is made once and left unchanged"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def descent_fixture(O, kind, M, over=False):
    """(matrix, oracle descent from the permutation start) of two / top at n = 1024"""
    def make():
        start = perm_tour(N)
        c = {"two": two, "top": top}[kind](N, M)
        if over:
            c = above(c, start)
        return c, Descent(O, c, start)
    return cached((kind, M, over), make)


def planted_fixture(O, M, flat, over=False, k=150):
    """(matrix, the planted cycle, the oracle's tabu walk of k iterations from it)"""
    def make():
        c, cyc = planted(N, M, flat)
        if over:
            c = above(c, cyc)
        s = cyc.copy()
        best, best_cost, final, trace = O.tabu_search(c, s, 0.0, k)
        return c, cyc, (best, best_cost, final, trace, s)
    return cached(("planted", M, flat, over, k), make)


# ------------------------------------------------------------------ on the CPU: what the fixtures are for
DESCENTS = [("two", PK16), ("top", PK16), ("two", U16), ("top", U16), ("top", PK16 - 1)]


@pytest.mark.parametrize("kind,M", DESCENTS)
def test_descent_fixtures_reach_the_extreme_deltas(O, kind, M):
    """the largest cell is exactly M (M + 1 above the threshold), the matrix is symmetric; from the permutation start the
    oracle runs at least 100 sweeps and at least 20 of its moves have delta == -2M"""
    c, run = descent_fixture(O, kind, M)
    assert c.max() == M and np.array_equal(c, c.T) and (np.diag(c) == -1).all() and c.min() == -1
    assert (c[~np.eye(N, dtype=bool)] >= 0).all() and np.array_equal(c, np.floor(c))
    assert run.sweeps >= 100 and int((run.d == -2.0 * M).sum()) >= 20, (run.sweeps, int((run.d == -2.0 * M).sum()))
    assert O.valid_tour(run.succ) and run.cost == O.tour_cost(c, run.succ)
    if M == PK16 and kind == "top":
        over, orun = descent_fixture(O, kind, M, over=True)
        assert over.max() == M + 1 and np.array_equal(over, over.T) and int((over != c).sum()) == 2
        assert orun.sweeps >= 100 and int((orun.d == -2.0 * M).sum()) >= 20


@pytest.mark.parametrize("M,flat", [(PK8, True), (PK8, False), (U16, True)])
def test_planted_fixtures_take_the_largest_positive_deltas(O, M, flat):
    """the planted cycle costs 0 and is a local optimum; the first tabu step from it is +2M (flat) / >= 2(M-3).  So are the
    first 128 (the smallest tenure, n / 8): until then every node that a move touched is tabu, so every pair the walk may
    take removes two edges of the cycle (cost 0) and adds two cells that are none"""
    c, cyc, walk = planted_fixture(O, M, flat)
    assert c.max() == M and np.array_equal(c, c.T) and (np.diag(c) == -1).all()
    assert O.valid_tour(cyc) and O.tour_cost(c, cyc) == 0.0
    d, _, _ = O.two_opt_once(c, cyc.copy(), 0.0)
    assert d >= -1e-7
    steps = np.diff(np.concatenate([[0.0], walk[3]]))
    if flat:
        assert (steps[:128] == 2.0 * M).all()
    else:
        assert (steps[:128] >= 2.0 * (M - 3)).all()
    assert steps.max() <= 2.0 * M
    if M == PK8:
        over, _, _ = planted_fixture(O, M, flat, over=True)
        assert over.max() == M + 1 and np.array_equal(over, over.T) and O.tour_cost(over, cyc) == 0.0 and int((over != c).sum()) == 2


# ------------------------------------------------------------------ on the device
@pytest.fixture(scope="module")
def T():
    import travellingsalesmanoptimization_amd as T
    return T


@pytest.fixture(scope="module")
def eng(T):
    e = T.Engine(0)
    yield e
    e.close()


def _defaults(T):
    return {T.OPT_ELEM: 0, T.OPT_KERNEL: 0, T.OPT_MATRIX_FREE: 0, T.OPT_PERSIST: 1, T.OPT_PERSIST_EDGES: 0, T.OPT_PERSIST_WINDOW: 0,
            T.OPT_STREAM_PERSIST: 1, T.OPT_FUSED: 1, T.OPT_HISTORY: 0, OPT_LP_NO_TMAT: 0, OPT_LP_GENERIC: 0}


@pytest.fixture
def clean(eng, T):
    """every test starts and ends on the engine's defaults"""
    def reset():
        for o, v in _defaults(T).items():
            eng.set_option(o, v)
    reset()
    yield eng
    reset()


class mode:
    """the options of one path, the defaults again behind it"""

    def __init__(self, eng, T, opts):
        self.eng, self.T, self.opts = eng, T, opts

    def __enter__(self):
        for o, v in self.opts.items():
            self.eng.set_option(o, v)

    def __exit__(self, *exc):
        d = _defaults(self.T)
        for o in self.opts:
            self.eng.set_option(o, d[o])


def paths(T):
    """path -> (options, the info() words that say this path ran on a packed instance at n = 1024; the callers add
    persist_packed, and overwrite the words of the shaped forms where the instance admits the 32-bit form only)"""
    lds = {"persist": 1, "stream_persist": 0}
    return {
        "tm": ({T.OPT_PERSIST: 2}, dict(lds, persist_shaped=1, persist_tmat=1, persist_window=0, persist_edges=4)),
        "shaped_no_copy": ({T.OPT_PERSIST: 2, OPT_LP_NO_TMAT: 1}, dict(lds, persist_shaped=1, persist_tmat=0, persist_window=0)),
        "generic": ({T.OPT_PERSIST: 2, OPT_LP_GENERIC: 1}, dict(lds, persist_shaped=0, persist_tmat=0, persist_window=0, persist_edges=4)),
        "generic_e7": ({T.OPT_PERSIST: 2, T.OPT_PERSIST_EDGES: 7}, dict(lds, persist_shaped=0, persist_tmat=0, persist_window=0, persist_edges=7)),
        "window": ({T.OPT_PERSIST: 2, T.OPT_PERSIST_WINDOW: 1}, dict(lds, persist_shaped=0, persist_window=1)),
        "stream": ({T.OPT_PERSIST: 0, T.OPT_STREAM_PERSIST: 2}, {"persist": 0, "stream_persist": 1}),
        "sweep": ({T.OPT_PERSIST: 0}, {"persist": 0, "stream_persist": 0, "fused": 1}),
        "sweep_split": ({T.OPT_PERSIST: 0, T.OPT_FUSED: 0}, {"persist": 0, "stream_persist": 0, "fused": 0}),
    }


LDS_PATHS = ("tm", "shaped_no_copy", "generic", "generic_e7", "window")


def engine_descent(eng, T, start, cap=-1):
    eng.set_option(T.OPT_HISTORY, HIST)
    eng.tour_load(0, start)
    sweeps, rc = eng.tour_two_opt(0, max_sweeps=cap)
    a, b, d = (np.array(v) for v in eng.history(HIST))
    succ, cost, _ = eng.tour_store(0)
    info = eng.info()
    eng.set_option(T.OPT_HISTORY, 0)
    return rc, sweeps, np.minimum(a, b), np.maximum(a, b), d, succ, cost, info


def same_descent(got, want, tag):
    """the sweep count, (a, b, delta) of every sweep, the successor array and the cost, all bit-exact"""
    rc, sweeps, a, b, d, succ, cost, _ = got
    assert rc == 0 and sweeps == want.sweeps and len(a) == want.sweeps, (tag, rc, sweeps, len(a), want.sweeps)
    moved = want.a >= 0
    bad = np.nonzero((a != want.a) | (moved & ((b != want.b) | (d != want.d))))[0]
    assert len(bad) == 0, (tag, "sweep", int(bad[0]), "engine", (int(a[bad[0]]), int(b[bad[0]]), float(d[bad[0]])),
                           "oracle", (int(want.a[bad[0]]), int(want.b[bad[0]]), float(want.d[bad[0]])))
    assert cost == want.cost and np.array_equal(succ, want.succ), (tag, cost, want.cost)


def expect_info(info, words, tag):
    got = {k: info[k] for k in words}
    assert got == words, (tag, got, words)


def run_descent_paths(eng, T, want, names, words_of, cap=-1):
    """`want` on every named path; words_of(name, words) completes the info() words the path must show"""
    P = paths(T)
    ran = []
    for name in names:
        opts, words = P[name]
        with mode(eng, T, opts):
            got = engine_descent(eng, T, want.start, cap)
        same_descent(got, want, name)
        expect_info(got[7], words_of(name, dict(words)), name)
        ran.append(name)
    return ran


@gpu
@pytest.mark.parametrize("kind", ["two", "top"])
def test_descent_at_the_packed_16_bit_limit(clean, T, O, kind):
    """costs up to exactly 16383 at n = 1024, from the permutation start to the optimum (moves of -32766 in the packed
    s16 deltas): the TM, the shaped, the generic (two geometries) and the half-window kernel in the packed form, k_str2opt
    and both one-launch-per-sweep paths"""
    eng = clean
    c, want = descent_fixture(O, kind, PK16)
    eng.set_costs(c)
    assert eng.info()["elem"] == 3 and eng.info()["symmetric"] == 1

    def words(name, w):
        if name in LDS_PATHS:
            w["persist_packed"] = 1
        return w
    ran = run_descent_paths(eng, T, want, list(paths(T)), words)
    assert len(ran) == 8


@gpu
def test_descent_just_above_the_packed_16_bit_limit(clean, T, O):
    """the same instance with one pair at 16384: every LDS-resident path runs the generic kernel's 32-bit form, no shaped
    instantiation; the moves are the oracle's"""
    eng = clean
    c, want = descent_fixture(O, "top", PK16, over=True)
    eng.set_costs(c)
    assert eng.info()["elem"] == 3

    def words(name, w):
        if name in LDS_PATHS:
            w.update(persist=1, persist_shaped=0, persist_tmat=0, persist_packed=0)
        return w
    ran = run_descent_paths(eng, T, want, list(paths(T)), words)
    assert len(ran) == 8


@gpu
@pytest.mark.parametrize("kind", ["two", "top"])
def test_descent_at_the_top_of_uint16(clean, T, O, kind):
    """uint16 cells up to exactly 65534 in the 32-bit form: moves of -131068 through the 18-bit fields of the exchange
    records of k_lds2opt, k_lds2opt_w and k_str2opt, and through both one-launch-per-sweep paths"""
    eng = clean
    c, want = descent_fixture(O, kind, U16)
    assert int((want.d == -131068.0).sum()) >= 20
    eng.set_costs(c)
    assert eng.info()["elem"] == 3

    def words(name, w):
        if name in LDS_PATHS:
            w.update(persist_shaped=0, persist_tmat=0, persist_packed=0)
        return w
    # ("tm": OPT_PERSIST = 2 and nothing else -- on this instance the generic kernel)
    ran = run_descent_paths(eng, T, want, ["tm", "window", "stream", "sweep", "sweep_split"], words)
    assert len(ran) == 5


@gpu
def test_storage_at_65534_and_65535(clean, T, O):
    """one pair raised from 65534 to 65535: the cells become int32 (65535 is the uint16 image of the -1 diagonal), the
    one-launch kernels refuse with code 8 where they are demanded, the descent still matches the oracle"""
    eng = clean
    c, _ = descent_fixture(O, "top", U16)
    eng.set_costs(c)
    assert eng.info()["elem"] == 3 and np.array_equal(eng.get_costs(), c)
    start = perm_tour(N)
    over = cached(("top", U16, "65535"), lambda: above(c, start))
    assert over.max() == 65535.0
    want = cached(("top", U16, "65535", "descent"), lambda: Descent(O, over, start, cap=120))
    eng.set_costs(over)
    assert eng.info()["elem"] == 2 and np.array_equal(eng.get_costs(), over)
    P = paths(T)
    ran = []
    for name in ("default", "sweep", "sweep_split", "tm", "stream"):
        opts = {} if name == "default" else P[name][0]
        with mode(eng, T, opts):
            if name in ("tm", "stream"):        # OPT_PERSIST = 2 / OPT_STREAM_PERSIST = 2: uint16 cells or code 8
                eng.tour_load(0, start)
                with pytest.raises(T.TspGpuError) as ei:
                    eng.tour_two_opt(0, max_sweeps=120)
                assert ei.value.code == 8, name
            else:
                got = engine_descent(eng, T, start, cap=120)
                same_descent(got, want, name)
                expect_info(got[7], dict({"elem": 2, "persist": 0, "stream_persist": 0, "persist_packed": 0},
                                         **({"fused": 0} if name == "sweep_split" else {})), name)
        ran.append(name)
    assert len(ran) == 5
    with pytest.raises(T.TspGpuError) as ei:    # uint16 cells demanded: not representable
        with mode(eng, T, {T.OPT_ELEM: 3}):
            eng.set_costs(over)
    assert ei.value.code == 3


TABU_PATHS = {"lds": ({16: 2}, {"persist": 1, "persist_window": 0}), "window": ({16: 2, 18: 1}, {"persist": 1, "persist_window": 1}),
              "sweep": ({16: 0}, {"persist": 0})}


def run_tabu_paths(eng, T, c, cyc, walk, packed, k=150):
    obest, obest_cost, ofinal, otrace, opath = walk
    ran = []
    for name, (opts, words) in TABU_PATHS.items():
        with mode(eng, T, opts):
            path = cyc.copy()
            best, best_cost, final, trace = eng.tabu_search(path, 0.0, k, want_trace=True)
            info = eng.info()
        bad = np.nonzero(trace != otrace)[0]
        assert len(bad) == 0, (name, "iteration", int(bad[0]), float(trace[bad[0]]), float(otrace[bad[0]]))
        assert final == ofinal and np.array_equal(path, opath), name
        assert best_cost == obest_cost and np.array_equal(best, obest), name
        words = dict(words)
        if words["persist"]:
            words["persist_packed"] = packed
            words["persist_shaped"] = 0
        expect_info(info, words, name)
        ran.append(name)
    return ran


@gpu
@pytest.mark.parametrize("flat", [True, False])
def test_tabu_walk_at_the_packed_limit(clean, T, O, flat):
    """150 iterations from the planted cycle at cost 0, costs up to exactly 8190: steps of +16380 (flat) / >= +16374 next
    to the poisoned pairs (>= 16386) of the packed tabu form -- LDS-resident, half window, one launch per sweep"""
    eng = clean
    c, cyc, walk = planted_fixture(O, PK8, flat)
    eng.set_costs(c)
    assert eng.info()["elem"] == 3
    assert len(run_tabu_paths(eng, T, c, cyc, walk, packed=1)) == 3


@gpu
@pytest.mark.parametrize("flat", [True, False])
def test_tabu_walk_just_above_the_packed_limit(clean, T, O, flat):
    """one pair at 8191: the tabu walk runs the 32-bit form; the plain descent on the same matrix (limit 16383) still
    runs the shaped packed kernel, 64 sweeps from the permutation start against the oracle"""
    eng = clean
    c, cyc, walk = planted_fixture(O, PK8, flat, over=True)
    eng.set_costs(c)
    assert eng.info()["elem"] == 3
    assert len(run_tabu_paths(eng, T, c, cyc, walk, packed=0)) == 3
    want = cached(("planted", PK8, flat, "descent"), lambda: Descent(O, c, perm_tour(N), cap=64))
    ran = run_descent_paths(eng, T, want, ["tm", "sweep"], lambda name, w: dict(w, persist_packed=1) if name == "tm" else w, cap=64)
    assert len(ran) == 2


@gpu
def test_tabu_walk_at_the_top_of_uint16(clean, T, O):
    """costs of exactly 65534: steps of +131068 through the exchange record, the 32-bit tabu form"""
    eng = clean
    c, cyc, walk = planted_fixture(O, U16, True)
    eng.set_costs(c)
    assert eng.info()["elem"] == 3
    assert len(run_tabu_paths(eng, T, c, cyc, walk, packed=0)) == 3


@gpu
def test_vns_walk_in_the_packed_form(clean, T, O):
    """one VNS walk (k = 4, glibc's rand stream) on the planted matrix with costs up to 8190, from the permutation start:
    the VNS instantiation's packed loop (persist_packed), against the oracle's walk"""
    eng = clean
    c, cyc, _ = planted_fixture(O, PK8, False)
    k = 4
    libc = ctypes.CDLL(None)
    start = cyc.copy()
    O.libc_srand(4)
    for _ in range(3):                          # a start three kicks away from the cycle: the first descent repairs them
        O.vns_kick(start)
    cost0 = O.tour_cost(c, start)
    assert O.valid_tour(start) and cost0 >= 3.0 * (PK8 - 3)
    O.libc_srand(5)
    rv = np.array([libc.rand() for _ in range(64 * k + 4096)], dtype=np.int32)
    O.libc_srand(5)
    opath = start.copy()
    obest, obest_cost = O.vns(c, opath, cost0, k)
    eng.set_costs(c)
    with mode(eng, T, {T.OPT_PERSIST: 2}):
        path, best = start.copy(), start.copy()
        res = eng.vns_search(path, k, rv, best, cost0)
        info = eng.info()
    assert (res["rc"], res["iterations"], res["kick_pending"]) == (0, k, 0)
    assert res["best_cost"] == obest_cost and np.array_equal(best, obest) and np.array_equal(path, opath)
    expect_info(info, {"persist": 1, "persist_packed": 1, "persist_shaped": 0, "vns_mode": 1}, "vns")


# ------------------------------------------------------------------ the shaped and TM instantiations on ties
def tie_instance(O, name):
    """name -> (points or None, matrix)"""
    def make():
        if name == "lattice":
            xy = lattice(32)
        elif name == "doubled":
            xy = doubled_points(N // 2)
        else:
            return None, small_matrix(N)
        return xy, O.cost_matrix(xy)
    return cached(("ties", name), make)


def load_instance(eng, xy, c):
    if xy is None:
        eng.set_costs(c)
    else:
        eng.set_points(xy); eng.build_costs()


@gpu
@pytest.mark.parametrize("start", ["nn", "perm"])
@pytest.mark.parametrize("name", ["lattice", "doubled", "matrix_1_9"])
def test_shaped_and_tm_on_ties(clean, T, O, name, start):
    """a 32 x 32 lattice, 512 integer points each taken twice (zero-length edges), a caller matrix with entries in 1..9, all
    at n = 1024: where the (delta, a, b) order itself decides the move -- to the optimum on the TM, the shaped, the generic
    kernel and one launch per sweep, every move the oracle's"""
    eng = clean
    xy, c = tie_instance(O, name)
    assert len(c) == N and c.max() <= PK8
    want = cached(("ties", name, start), lambda: Descent(O, c, O.nn_tour(c, 0)[0] if start == "nn" else perm_tour(N)))
    load_instance(eng, xy, c)
    assert eng.info()["elem"] == 3
    if start == "nn":
        g, gcost = eng.nn_tour(0)
        assert gcost == want.cost0 and np.array_equal(g, want.start)
    ran = run_descent_paths(eng, T, want, ["tm", "shaped_no_copy", "generic", "sweep"],
                            lambda p, w: dict(w, persist_packed=1) if p in LDS_PATHS else w)
    assert len(ran) == 4


@gpu
@pytest.mark.parametrize("name", ["lattice", "top16382"])
def test_the_copy_on_ties_and_at_the_limit(clean, T, O, name):
    """the tour-ordered copy behind launches capped at 1, 2, 3 and 17 sweeps and at the optimum, on the lattice and on costs
    up to 16382 (16383 is the copy's poison value: the matrices with that cost are checked through their moves only)"""
    from test_lds_tmat import check_tmat
    eng = clean
    if name == "lattice":
        xy, c = tie_instance(O, "lattice")
    else:
        xy, (c, _) = None, descent_fixture(O, "top", PK16 - 1)
    assert c.max() < PK16
    load_instance(eng, xy, c)
    start = perm_tour(N)
    with mode(eng, T, {T.OPT_PERSIST: 2}):
        for cap in (1, 2, 3, 17, -1):
            eng.tour_load(0, start)
            sweeps, rc = eng.tour_two_opt(0, max_sweeps=cap)
            expect_info(eng.info(), {"persist": 1, "persist_shaped": 1, "persist_tmat": 1, "persist_packed": 1}, cap)
            assert rc == 0 and (sweeps == cap if cap > 0 else sweeps > 100), (cap, sweeps)
            check_tmat(eng, c, N)


# ------------------------------------------------------------------ the flagship shape
@gpu
@pytest.mark.parametrize("name", ["two", "lattice"])
def test_flagship_shape_on_ties(clean, T, O, name):
    """n = 4096 (16 edges a workgroup), costs in {0, 16383} and a 64 x 64 lattice: 40 sweeps from the permutation start on
    the TM kernel and one launch per sweep, every move the oracle's; the copy behind the cap for the lattice"""
    from test_lds_tmat import check_tmat
    eng = clean
    n, cap = 4096, 40
    start = perm_tour(n)
    if name == "two":
        xy, c = None, two(n, PK16)
        assert c.max() == PK16 and np.array_equal(c, c.T)
    else:
        xy = lattice(64)
        c = O.cost_matrix(xy)
    want = Descent(O, c, start, cap=cap)
    assert want.sweeps == cap and (want.a >= 0).all()
    assert name != "two" or int((want.d == -2.0 * PK16).sum()) >= 20
    load_instance(eng, xy, c)
    assert eng.info()["elem"] == 3
    P = paths(T)
    ran = []
    for p in ("tm", "sweep"):
        with mode(eng, T, P[p][0]):
            got = engine_descent(eng, T, start, cap)
            same_descent(got, want, p)
            expect_info(got[7], dict(P[p][1], persist_edges=16, **({"persist_packed": 1} if p == "tm" else {})), p)
            if p == "tm" and name == "lattice":
                check_tmat(eng, c, n)
        ran.append(p)
    assert len(ran) == 2
