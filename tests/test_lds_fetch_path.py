"""The shaped instantiations of k_lds2opt without their phase clocks (csrc/tspgpu_lds2opt.inc: the clocks are a template
parameter, option 98 picks the clocked instantiation) and the fetching workgroup's path of the TM form, class by class.  Every
descent is compared move by move with the shaped kernel that reloads from the matrix (option 88) and with the
one-launch-per-sweep path, and its recorded moves are replayed through the array model of tests/lds_overlap_step0.py to make
sure that the descent held a sweep of every class the path distinguishes: only the copy row fetched, the copy row with the
range across the array end, a partial fetch of one row and of several, a workgroup that fetches all its rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPT_LP_NO_TMAT = 88         # undocumented: 1 = the shaped k_lds2opt that reloads moved rows from the matrix
OPT_STAMPS = 98             # undocumented: 1 = the clocked instantiation, phase stamps per workgroup
HIST = 4096
POISON = 16383


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
    e.set_option(T.OPT_ELEM, 3); e.set_option(T.OPT_KERNEL, 0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def defaults(eng, T):
    yield
    eng.set_option(OPT_LP_NO_TMAT, 0); eng.set_option(OPT_STAMPS, 0); eng.set_option(T.OPT_PERSIST, 1); eng.set_option(T.OPT_HISTORY, 0)


def load(eng, xy):
    eng.set_points(xy); eng.build_costs()


def path_mode(eng, T, path):
    """tmat: the default where a shape is instantiated; mat: the hook; sweep: one launch per sweep"""
    eng.set_option(OPT_LP_NO_TMAT, 1 if path == "mat" else 0)
    eng.set_option(T.OPT_PERSIST, 0 if path == "sweep" else 2)


def run(eng, T, path, start, cap=-1):
    """the descent of slot 0 from the successor array `start`, at most `cap` sweeps: (sweeps, cost, tour, a, b, delta, info)"""
    path_mode(eng, T, path)
    eng.tour_load(0, start)
    eng.set_option(T.OPT_HISTORY, HIST)
    sweeps, rc = eng.tour_two_opt(0, max_sweeps=cap)
    assert rc == 0
    a, b, d = eng.history(HIST)
    succ, cost, _ = eng.tour_store(0)
    return sweeps, cost, succ, a.copy(), b.copy(), d.copy(), eng.info()


def same_moves(x, y, what):
    assert (x[0], x[1]) == (y[0], y[1]), what
    assert np.array_equal(x[2], y[2]), what
    for i in (3, 4, 5):
        bad = np.nonzero(x[i] != y[i])[0] if len(x[i]) == len(y[i]) else [-1]
        assert len(bad) == 0, (what, i, bad[:4])


def replay(start, a, b, E):
    """The recorded moves through the kernel's array (tests/lds_overlap_step0.py): the array is the visiting order from node 0,
    the shorter arc [lo, lo + M) is reversed, k0 = E * wg, an own cell whose mirror cell lies more than E cells behind k0 needs
    a fetched row.  Per moving sweep (lo, M, need[W][E + 1]); and the array and direction at the end."""
    n = len(start)
    W = n // E
    ord_ = np.empty(n, dtype=np.int64)
    v = 0
    for p in range(n):
        ord_[p] = v; v = start[v]
    pos = np.empty(n, dtype=np.int64); pos[ord_] = np.arange(n)
    dirn = 1
    k0 = np.arange(W)[:, None] * E
    r = np.arange(E + 1)[None, :]
    out = []
    for la, lb in zip(a, b):
        if la < 0:
            break
        ea = pos[la] if dirn > 0 else (pos[la] - 1) % n
        eb = pos[lb] if dirn > 0 else (pos[lb] - 1) % n
        s1, s2 = (ea, eb) if dirn > 0 else (eb, ea)
        L = (s2 - s1) % n
        other = n - L < L
        M = n - L if other else L
        lo = ((s2 if other else s1) + 1) % n
        if other:
            dirn = -dirn
        rel = (k0 - lo + r) % n
        rm = ((lo + M - 1 - rel) % n - k0) % n
        out.append((int(lo), int(M), (rel < M) & (rm > E)))
        idx = (lo + np.arange(M)) % n
        ord_[idx] = ord_[idx][::-1]
        pos[ord_[idx]] = idx
    return out, ord_, dirn


def classes(moves, n, E):
    """how many sweeps of each class of the fetching workgroup's path the moves hold"""
    c = dict(copy_only=0, copy_wrapped=0, partial_1=0, partial_2plus=0, all_rows=0)
    for lo, M, need in moves:
        cnt = need.sum(axis=1)
        copy = need[:, E]
        c["copy_only"] += bool((copy & (cnt == 1)).any())
        c["copy_wrapped"] += bool(copy.any() and lo + M > n)
        c["partial_1"] += bool((cnt == 1).any())
        c["partial_2plus"] += bool(((cnt >= 2) & (cnt <= E)).any())
        c["all_rows"] += bool((cnt == E + 1).any())
    return c


def succ_of(ord_, dirn):
    succ = np.empty(len(ord_), dtype=np.int32)
    succ[ord_] = np.roll(ord_, -1) if dirn > 0 else np.roll(ord_, 1)
    return succ


def check_tmat(eng, c, ord_):
    """the copy behind the last launch: tmat[x][q] == c[x][node at cell q], the cell of x poisoned, the cells the replay's"""
    n = len(ord_)
    tm = np.empty((n, n), dtype=np.uint16)
    eng._ck(eng.L.tspgpu_debug_tmat(eng.ctx, tm.ctypes.data, tm.size))
    want = c[:, ord_].astype(np.uint16)
    want[ord_, np.arange(n)] = POISON
    bad = np.argwhere(tm != want)
    assert len(bad) == 0, (len(bad), bad[:4])


@pytest.fixture(scope="module")
def nn_runs(eng, T, O, points):
    """NN(0) to the optimum at n = 1024 (shaped (1024, 4)) on the three paths, once per seed"""
    cache = {}

    def get(seed):
        if seed not in cache:
            load(eng, points[(1024, seed)])
            start, _ = eng.nn_tour(0)
            cache[seed] = (start, {p: run(eng, T, p, start) for p in ("tmat", "mat", "sweep")})
        return cache[seed]
    return get


@pytest.mark.parametrize("seed", [1, 123])
def test_descents_hold_every_class(eng, T, O, nn_runs, seed):
    """NN(0) at n = 1024: the tmat path against option 88 and the per-sweep path, move by move; the recorded moves hold a sweep
    with only the copy row fetched, one with the copy row and the range across the array end, partial fetches of 1 and of 2 or
    more rows and a workgroup that fetches all its rows"""
    start, runs = nn_runs(seed)
    tm = runs["tmat"]
    assert [(runs[p][6]["persist"], runs[p][6]["persist_shaped"], runs[p][6]["persist_tmat"]) for p in ("tmat", "mat", "sweep")] == \
        [(1, 1, 1), (1, 1, 0), (0, 0, 0)]
    assert len(tm[3]) == tm[0] and tm[3][-1] == -1 and O.valid_tour(tm[2])
    moves, ord_, dirn = replay(start, tm[3], tm[4], 4)
    assert len(moves) == tm[0] - 1 and np.array_equal(succ_of(ord_, dirn), tm[2]), "the array model lost the kernel's tour"
    cl = classes(moves, 1024, 4)
    print(seed, cl)
    assert all(v > 0 for v in cl.values()), cl
    for p in ("mat", "sweep"):
        same_moves(runs[p], tm, p)


def test_long_reversals_capped(eng, T, O, points):
    """from a random permutation tour at n = 1024, 300 sweeps: M up to n/2, every class again, the three paths move by move, and
    the whole copy behind the launch"""
    xy = points[(1024, 1)]
    load(eng, xy)
    start = perm_tour(1024, 7)
    runs = {p: run(eng, T, p, start, cap=300) for p in ("mat", "sweep", "tmat")}
    tm = runs["tmat"]
    assert tm[0] == 300 and tm[6]["persist_tmat"] == 1
    moves, ord_, dirn = replay(start, tm[3], tm[4], 4)
    assert len(moves) == 300 and np.array_equal(succ_of(ord_, dirn), tm[2]), "the array model lost the kernel's tour"
    Ms = np.array([m[1] for m in moves])
    cl = classes(moves, 1024, 4)
    print(Ms.max(), (Ms > 64).sum(), cl)
    assert Ms.max() > 480 and (Ms > 64).sum() >= 30          # (long ranges, up to n/2)
    assert all(v > 0 for v in cl.values()), cl
    for p in ("mat", "sweep"):
        same_moves(runs[p], tm, p)
    check_tmat(eng, O.cost_matrix(xy), ord_)                  # (the tmat run was the last launch)


def test_capped_launches(eng, T, O, points, nn_runs):
    """launches capped behind a move that left a workgroup with a partial fetch (and behind the first sweep): tour, cost and
    sweep count are the per-sweep path's at the same cap, and the continuation reaches the uncapped descent's optimum"""
    start, runs = nn_runs(1)
    load(eng, points[(1024, 1)])
    full = runs["tmat"]
    moves, _, _ = replay(start, full[3], full[4], 4)
    partial = [s + 1 for s, (lo, M, need) in enumerate(moves) if ((need.sum(axis=1) >= 1) & (need.sum(axis=1) <= 4)).any()]
    assert len(partial) >= 3
    caps = sorted({1, partial[len(partial) // 4], partial[len(partial) // 2], partial[-1]})
    assert len(caps) == 4
    for cap in caps:
        got = run(eng, T, "tmat", start, cap=cap)
        want = run(eng, T, "sweep", start, cap=cap)
        assert got[0] == cap and got[6]["persist_tmat"] == 1
        same_moves(want, got, cap)
        path_mode(eng, T, "tmat")
        eng.tour_load(0, got[2])
        more, rc = eng.tour_two_opt(0)
        succ, cost, _ = eng.tour_store(0)
        assert rc == 0 and cap + more == full[0] and cost == full[1] and np.array_equal(succ, full[2]), cap


def test_clocked_against_production(eng, T, points, nn_runs):
    """option 98 picks the instantiation with the phase clocks: the same moves, stamps only from it, both shaped and on tmat"""
    start, runs = nn_runs(123)
    load(eng, points[(1024, 123)])
    buf = np.zeros(1024 * 64, dtype=np.uint64)
    eng.set_option(OPT_STAMPS, 1)                             # (allocates and zeroes the stamps)
    eng.set_option(OPT_STAMPS, 0)
    off = run(eng, T, "tmat", start)
    eng._ck(eng.L.tspgpu_debug_stamps(eng.ctx, buf.ctypes.data, buf.size))
    assert not buf.any(), "the production instantiation wrote stamps"
    eng.set_option(OPT_STAMPS, 1)
    on = run(eng, T, "tmat", start)
    eng._ck(eng.L.tspgpu_debug_stamps(eng.ctx, buf.ctypes.data, buf.size))
    eng.set_option(OPT_STAMPS, 0)
    for r in (off, on):
        assert (r[6]["persist"], r[6]["persist_shaped"], r[6]["persist_tmat"]) == (1, 1, 1)
    same_moves(on, off, "clocked")
    same_moves(off, runs["tmat"], "production")
    st = buf.reshape(-1, 16)[:256]
    assert (st[:, 8] == on[0]).all(), "every workgroup counts the descent's sweeps"
    assert (st[:, :6] > 0).all() and (st[:, 12] > 0).all(), "a phase clock (or the write-back's) stayed at zero"
    assert st[:, 6].max() > 0 and st[:, 7].sum() >= st[:, 6].sum()


def test_flagship_shape_long_reversals(eng, T, O, points):
    """(4096, 16) from a permutation tour, 200 sweeps, tmat path against the per-sweep path move by move: ranges longer than 512
    cells and a workgroup that fetches all 17 rows"""
    load(eng, points[(4096, 123)])
    start = perm_tour(4096, 11)
    tm = run(eng, T, "tmat", start, cap=200)
    assert tm[0] == 200 and (tm[6]["persist"], tm[6]["persist_shaped"], tm[6]["persist_tmat"]) == (1, 1, 1)
    sw = run(eng, T, "sweep", start, cap=200)
    same_moves(sw, tm, "sweep")
    moves, ord_, dirn = replay(start, tm[3], tm[4], 16)
    assert np.array_equal(succ_of(ord_, dirn), tm[2]), "the array model lost the kernel's tour"
    Ms = np.array([m[1] for m in moves])
    cl = classes(moves, 4096, 16)
    print(Ms.max(), (Ms > 512).sum(), cl)
    assert (Ms > 512).any() and cl["all_rows"] > 0 and cl["copy_wrapped"] > 0
