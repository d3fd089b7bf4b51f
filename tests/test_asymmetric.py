"""Caller matrices that are not symmetric (tspgpu_set_costs, tspgpu_info 7 == 0), at every edge of the masks of the forms that
run on them: sweep_step_as<T, NCH, TABU, BLOCKS = false> (the cyclic index range [a+1, n-1] per wave: skipped, clean, or masked
per lane), k_sweep_simple's kmax = n - 1 - a, k_apply's reference arc with its edge costs re-read in tour direction, the
launch path that is always batches of sweep + apply launches, the matrix NN kernels, the farthest pair and Extra Mileage.

Everything is bit-exact against the CPU oracle (oracle/cpu_ref.c indexes c[a][b] orientation-faithfully) or the numpy model of
tests/test_extra_mileage.py; there are no tolerances.  The CPU tests state on the oracle alone that each fixture reaches the
edge it is meant to; the device tests (-m gpu) compare with the oracle and read from info() which kernel and geometry ran.

A wave holds S = 64 V consecutive node indices per chunk: 128 (f64), 256 (int32), 512 (uint16).  The sizes below put one, two
and three to four such waves on a row, the last one almost all pad or with one real lane.

2-opt with the reference's delta need not terminate on such a matrix: every descent here is capped."""
import itertools
import os

import numpy as np
import pytest

from test_packed_limits import Descent, perm_tour

gpu = pytest.mark.gpu

HIST = 64
VEC = {1: 2, 2: 4, 3: 8}                    # cells per 16-byte vector: f64, int32, uint16
SPAN = {e: 64 * v for e, v in VEC.items()}  # node indices one wave holds per chunk
ROWS = [(1, 130), (1, 300), (2, 517), (3, 1100), (3, 1537)]      # (cell type, n) of the planted sweeps
KERNELS, BLOCKS, WGS = (1, 2, 3), (0, 64, 128), (0, 1)
CAP = 40

_cache = {}


def cached(key, make):
    """every matrix and every oracle run of this file is made once and left unchanged"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def inverse(succ):
    pred = np.empty_like(succ)
    pred[succ] = np.arange(len(succ), dtype=succ.dtype)
    return pred


# ------------------------------------------------------------------ 1. planted single sweeps: the fixture
def best_pair(c, succ, both=False, pred_mask=True, own_row=True, tabu=False):
    """one sweep's pick by evaluating all pairs -> ((lo, hi), delta), ((-1, -1), 0.0) when nothing improves (tabu: the least
    delta whatever its sign).  The defaults are the reference's rule (refinment.c:49-69): b > a, b != succ a, succ b != a,
    delta = c[a][b] + c[sa][sb] - (c[a][sa] + c[b][sb]), the first strict minimum in (a, b) order.  Each flag switches one
    mistake on: both -- the orientation b < a is evaluated too; pred_mask = False -- b == pred a is not excluded;
    own_row = False -- c[a][succ a] is read as c[succ a][a]."""
    n = len(c)
    idx = np.arange(n)
    d_b = c[idx, succ]
    d_a = d_b if own_row else c[succ, idx]
    D = (c + c[succ][:, succ]) - (d_a[:, None] + d_b[None, :])
    A, B = idx[:, None], idx[None, :]
    ok = (A != B) & (B != succ[A])
    if pred_mask:
        ok &= succ[B] != A
    if not both:
        ok &= B > A
    D = np.where(ok, D, np.inf)
    a, b = divmod(int(np.argmin(D)), n)       # first minimum in row-major order
    if not tabu and not D[a, b] < 0:
        return (-1, -1), 0.0
    return (min(a, b), max(a, b)), float(D[a, b])


class Planted:
    """every off-diagonal cell an integer in [1000, 1050], the diagonal -1, and on the permutation tour `tour`:
    - c[a][b] = c[succ a][succ b] = 30 (plant): the pair (a, b) is the unique minimum, about -1940;
    - the transposed decoy c[y][x] = c[succ y][succ x] = 0 for some x < y away from the planted nodes: better than the planted
      pair, and seen only if the orientation b < a is evaluated;
    - the excluded-pair decoy c[a][pred a] = c[succ a][a] = 0: the pair (a, pred a) would have delta about -2050; where
      pred a > a it wins as soon as b == pred a is not masked, and the second cell makes c[a][succ a] read from the wrong row
      lose the planted pair;
    - (the pad cells of a device row are zero: with every real cell >= 1000 an unmasked pad lane wins.)
    plant = False: the tour's own edges cost 400 .. 450 instead, so every admissible delta is positive (the tabu move takes
    the least of them) and both decoys are negative."""

    def __init__(self, O, base, tour, a, b, plant=True):
        n = len(tour)
        pred = inverse(tour)
        c = base.copy()
        rng = np.random.default_rng(10000 * a + b + 1)
        if not plant:
            c[np.arange(n), tour] = rng.integers(400, 451, size=n)
        sa, pa = int(tour[a]), int(pred[a])
        c[a, pa] = c[sa, a] = 0.0
        used = {a, sa, pa, int(pred[pa])}
        want = 0.0
        if plant:
            sb = int(tour[b])
            assert a < b and b not in (sa, pa)
            c[a, b] = c[sa, sb] = 30.0
            used |= {b, sb, int(pred[b])}
            want = 60.0 - (c[a, sa] + c[b, sb])
        for _ in range(100000):
            x, y = sorted(int(v) for v in rng.choice(n, 2, replace=False))
            sx, sy = int(tour[x]), int(tour[y])
            if not ({x, y, sx, sy} & used) and sx != y and sy != x and -(c[x, sx] + c[y, sy]) < want:
                break
        else:
            raise AssertionError("no transposed decoy")
        c[y, x] = c[sy, sx] = 0.0
        self.n, self.c, self.tour, self.a, self.b, self.pa, self.decoy, self.plant = n, np.ascontiguousarray(c), tour, a, b, pa, (x, y), plant
        self.cost0 = O.tour_cost(self.c, tour)
        self.succ = tour.copy()                 # the oracle's sweep
        self.delta, self.cost, self.move = O.two_opt_once(self.c, self.succ, self.cost0)


def planted_cases(n, S):
    """-> (tour, [(a, b)]): a in {0, S-1, S, n-3, the largest a whose predecessor has the higher index} x b in {a+2, the last
    index of a's wave, the first of the next wave, the first and last index of the first wave wholly inside [a+1, n-1], n-1},
    and for a = 0 also b = pred pred a (the flipped arc succ a .. b then has n - 2 cells, the most there can be) and both ends of pred a's wave, without the
    pairs refinment.c:55 excludes.  The tour is the first seeded permutation tour (seed 7 upwards) on which n-1 is
    no tour neighbour of any a -- the case b = n-1 stays for every a -- and pred a > a holds for at least three of the a's
    (n = 130 has only three a's: for two), and on which pred 0 lies in a wave wholly inside the range of a = 0 where there is
    one, and succ 0 in another: but for the lane of b == pred a that wave would take the path without masks; and on which the wave
    behind a = S-1, wholly inside its range, holds neither succ a nor pred a: it takes the path without masks, and both its
    ends are planted b's."""
    for seed in range(7, 2000):
        tour = perm_tour(n, seed)
        pred = inverse(tour)
        amax = max(a for a in range(n - 2) if pred[a] > a and n - 1 not in (tour[a], pred[a]))
        As = sorted({a for a in (0, S - 1, S, n - 3, amax) if a <= n - 3})
        if any(n - 1 in (tour[a], pred[a]) for a in As) or sum(pred[a] > a for a in As) < min(3, len(As) - 1):
            continue
        if n >= 2 * S and not (1 <= pred[0] // S < n // S and tour[0] // S != pred[0] // S):
            continue
        if n >= 2 * S and 1 in (tour[S - 1] // S, pred[S - 1] // S):
            continue
        cases = []
        for a in As:
            w = a // S
            bs = {a + 2, min((w + 1) * S - 1, n - 1), (w + 1) * S, n - 1}
            if a == 0:
                bs.add(int(pred[pred[0]]))      # the longest arc there is: n - 2 cells
                if n >= 2 * S:
                    bs |= {pred[0] // S * S, pred[0] // S * S + S - 1}      # both ends of pred a's wave
            wi = (a + S) // S                   # the first wave that begins at or behind a + 1
            if (wi + 1) * S - 1 <= n - 1:
                bs |= {wi * S, (wi + 1) * S - 1}
            bs = sorted(b for b in bs if a < b < n and b not in (tour[a], pred[a]))
            assert n - 1 in bs
            cases += [(a, b) for b in bs]
        return tour, cases
    raise AssertionError("no tour")


def wave_inside(p, S):
    """b's wave lies wholly inside the range [a+1, n-1]"""
    w = p.b // S
    return w * S >= p.a + 1 and (w + 1) * S <= p.n


def mask_free_wave(p, S):
    """... and holds none of a, pred a, succ a: sweep_step_as evaluates it without the per-lane valid()"""
    return wave_inside(p, S) and p.b // S not in (p.a // S, p.pa // S, int(p.tour[p.a]) // S)


def planted_fixture(O, n, S):
    """the planted cases of (n, S), and one case without a planted pair (a = 0)"""
    def make():
        rng = np.random.default_rng(n)
        base = rng.integers(1000, 1051, size=(n, n)).astype(np.float64)
        np.fill_diagonal(base, -1.0)
        tour, cases = planted_cases(n, S)
        return [Planted(O, base, tour, a, b) for a, b in cases] + [Planted(O, base, tour, 0, -1, plant=False)]
    return cached(("planted", n, S), make)


def tabu_lists(n, S, a):
    """(list, tenure, iteration): nothing tabu; every third node of a's wave stamped within the tenure"""
    free = np.full(n, -1, dtype=np.int32)
    part = free.copy()
    part[(a // S) * S:min(n, (a // S + 1) * S):3] = 6
    return [(free, 5, 9), (part, 5, 9)]


def oracle_tabu(O, p, tl, tenure, it):
    def make():
        succ, stamps = p.tour.copy(), tl.copy()
        cost, mv = O.tabu_move(p.c, succ, p.cost0, stamps, tenure, it)
        return succ, stamps, cost, mv
    return cached(("tabu", p.n, p.a, p.b, p.plant, int((tl >= 0).sum())), make)


@pytest.mark.parametrize("elem,n", ROWS)
def test_planted_cases_are_picked_by_the_oracle_and_missed_by_each_wrong_rule(O, elem, n):
    """every planted pair is the oracle's move, with delta 60 - c[a][succ a] - c[b][succ b]; evaluating both orientations
    picks the transposed decoy, leaving b == pred a unmasked picks (a, pred a) where pred a > a, and c[a][succ a] read from
    the row of succ a picks another pair or gives the planted one a delta about 1000 too high; the case without a planted pair has a positive best admissible delta"""
    S = SPAN[elem]
    fx = planted_fixture(O, n, S)
    assert len(fx) >= 8 and sum(p.pa > p.a for p in fx) >= len(fx) // 2
    for p in fx:
        c, tour = p.c, p.tour
        off = ~np.eye(n, dtype=bool)
        assert (np.diag(c) == -1).all() and (c[off] >= 0).all() and c.max() <= 1050 and not np.array_equal(c, c.T)
        right = best_pair(c, tour, tabu=not p.plant)
        if p.plant:
            assert p.move == (p.a, p.b) and -2040.0 <= p.delta <= -1940.0, (p.a, p.b, p.move, p.delta)
            assert p.delta == 60.0 - (c[p.a, tour[p.a]] + c[p.b, tour[p.b]]) and p.cost == p.cost0 + p.delta
            assert right == (p.move, p.delta)
        else:
            assert p.move == (-1, -1) and p.delta == 0.0 and np.array_equal(p.succ, tour) and right[1] > 0.0
            free, tenure, it = tabu_lists(n, S, p.a)[0]
            _, _, cost, mv = oracle_tabu(O, p, free, tenure, it)
            assert (mv, cost - p.cost0) == right
        assert best_pair(c, tour, both=True, tabu=not p.plant)[0] == p.decoy
        if p.pa > p.a:
            assert best_pair(c, tour, pred_mask=False, tabu=not p.plant)[0] == (p.a, p.pa)
        if p.plant:
            wrong = best_pair(c, tour, own_row=False)
            assert wrong != right and (wrong[0] != right[0] or wrong[1] > -1000.0), wrong
    # the waves: a in the first, a middle and the last wave; b in a's wave, in the next and in the last one
    planted = [p for p in fx if p.plant]
    assert {p.a // S for p in planted} >= {0, (n - 3) // S} and all((a, n - 1) in {(p.a, p.b) for p in planted} for a in {p.a for p in planted})
    assert any(p.b // S == p.a // S for p in planted) and any(p.b // S == p.a // S + 1 for p in planted)
    if n >= 2 * S:
        assert any(p.b % S == 0 and p.b // S > p.a // S for p in planted) and any(p.b % S == S - 1 for p in planted)
        # the path without masks: b in a wave wholly inside [a+1, n-1] that holds none of a, pred a, succ a -- its first and
        # its last lane; and the same wave made to take the masked path by pred a alone (a = 0)
        free = [p for p in planted if mask_free_wave(p, S)]
        assert {p.b % S for p in free} >= {0, S - 1}, [(p.a, p.b) for p in free]
        assert any(p.a == 0 and p.pa // S == p.b // S and wave_inside(p, S) and p.tour[0] // S != p.b // S for p in planted)


# ------------------------------------------------------------------ 2. capped descents: the fixtures
DESCENTS = [(130, 999), (300, 9), (517, 60000), (1100, 65534), (1100, 100000), (1537, 16383)]
CROSS = [(300, 9), (1100, 65534), (1100, 100000), (1537, 16383)]      # the descents that must cross waves


def asym_matrix(n, hi):
    def make():
        c = np.random.default_rng(n + hi).integers(1, hi + 1, size=(n, n)).astype(np.float64)
        np.fill_diagonal(c, -1.0)
        return np.ascontiguousarray(c)
    return cached(("matrix", n, hi), make)


def start_tour(O, c, start):
    return O.nn_tour(c, 0)[0] if start == "nn" else perm_tour(len(c))


def descent_fixture(O, n, hi, start, cap=CAP):
    """(matrix, the oracle's `cap` sweeps from NN(0) / the permutation tour, the cost carried from sweep to sweep)"""
    c = asym_matrix(n, hi)
    return c, cached(("descent", n, hi, start, cap), lambda: Descent(O, c, start_tour(O, c, start), cap=cap))


def elems_of(hi):
    """the cell types that admit integer costs up to hi, and what AUTO picks"""
    return ([1, 2, 3], 3) if hi <= 65534 else ([1, 2], 2)


@pytest.mark.parametrize("start", ["nn", "perm"])
@pytest.mark.parametrize("n,hi", DESCENTS)
def test_capped_descents_use_their_whole_cap(O, n, hi, start):
    """the oracle moves in every one of the 40 sweeps (none of these instances reaches an optimum earlier); the carried
    cost is the start's cost plus the deltas, which on such a matrix is not the tour's cost; at n = 300 and n >= 1100 at
    least 10 of the 40 moves join two different waves, at the wave span of every cell type that admits the matrix and has
    at least two whole waves on the row"""
    c, run = descent_fixture(O, n, hi, start)
    assert c.max() == hi and c.min() == -1 and not np.array_equal(c, c.T)
    assert run.sweeps == CAP and (run.a >= 0).all() and (run.d < 0).all()
    assert O.valid_tour(run.succ) and run.cost == run.cost0 + run.d.sum()
    if (n, hi) in CROSS:
        for elem in elems_of(hi)[0]:
            S = SPAN[elem]
            if 2 * S <= n:                  # (n = 300: one wave of uint16 cells, and the second of int32 cells is mostly pad)
                assert int((run.a // S != run.b // S).sum()) >= 10, (S, int((run.a // S != run.b // S).sum()))


def test_carried_cost_is_not_the_tour_cost(O):
    """why a continued slot is compared with the carried cost: the reference's delta assumes symmetry"""
    c, run = descent_fixture(O, 517, 60000, "perm")
    assert run.cost != O.tour_cost(c, run.succ)


# ------------------------------------------------------------------ 3. Extra Mileage: the model against the reference's loop
def em_transcription(c, a, b):
    """h_extramileage_util (heuristics.c:290-367) from (a, b) with the cost 2 c[a][b] of :196, loop for loop"""
    n = len(c)
    cl = c.tolist()
    visited = [False] * n
    visited[a] = visited[b] = True
    edges = [(a, b), (b, a)]
    succ = np.full(n, -1, dtype=np.int32)
    succ[a], succ[b] = b, a
    cost = 2 * cl[a][b]
    while len(edges) < n:
        mileage, best_j, best_i = float("inf"), -1, -1
        for i in range(n):
            if visited[i]:
                continue
            ci = cl[i]
            for j, (u, v) in enumerate(edges):
                delta = cl[u][i] + ci[v] - cl[u][v]
                if delta < mileage:
                    mileage, best_j, best_i = delta, j, i
        if best_j == -1:
            break
        u, v = edges[best_j]
        succ[u] = best_i
        edges[best_j] = (u, best_i)
        succ[best_i] = v
        edges.append((best_i, v))
        visited[best_i] = True
        cost += mileage
    return succ, cost


@pytest.mark.parametrize("hi", [9, 1000, 60000])
@pytest.mark.parametrize("n", [40, 70, 90])
def test_em_model_equals_the_reference_loop_on_asymmetric_matrices(n, hi):
    from test_extra_mileage import em_model, farthest_pair
    c = asym_matrix(n, hi)
    a, b = farthest_pair(c)
    assert c[a, b] == np.triu(c, 1).max() and a < b
    for pair in ((a, b), (b, a), (3, n - 1)):
        msucc, mcost, _ = em_model(c, *pair)
        tsucc, tcost = em_transcription(c, *pair)
        assert mcost == tcost and np.array_equal(msucc, tsucc), (n, hi, pair)


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
    return {T.OPT_ELEM: 0, T.OPT_KERNEL: 0, T.OPT_BATCH: 32, T.OPT_WGS_PER_TOUR: 0, T.OPT_GRAPH: 1, T.OPT_BLOCK: 0, T.OPT_FUSED: 1,
            T.OPT_SWEEP_CAP: -1, T.OPT_NN_KERNEL: 0, T.OPT_PERSIST: 1, T.OPT_STREAM_PERSIST: 1, T.OPT_EM_FORM: 0, T.OPT_HISTORY: 0}


@pytest.fixture
def clean(eng, T):
    """every test starts and ends on the engine's defaults"""
    def reset():
        for o, v in _defaults(T).items():
            eng.set_option(o, v)
    reset()
    yield eng
    reset()


def options(eng, opts):
    for o, v in opts.items():
        eng.set_option(o, v)


def expect_info(info, words, tag):
    got = {k: info[k] for k in words}
    assert got == words, (tag, got, words)


ASYM = {"symmetric": 0, "fused": 0, "persist": 0, "stream_persist": 0, "matrix_free": 0}


def check_geometry(info, elem, kernel, block, wgs, tag):
    """what info() says ran: the cell type and the kernel asked for, never a fused or one-launch form.  The simple and the
    pipelined kernel take the block and the workgroup count as given.  The resident kernel takes the block where it needs no
    more chunks than the kernel has (one for uint16 cells, two otherwise) and else its own, one vector per thread; it keeps
    runs of P = 2 .. 8 tour edges, P + 1 rows in LDS, whatever the workgroup count asked for, so it always runs several
    workgroups per tour.  -> chunks per thread, from the row length and the block (0: k_sweep_simple strides)"""
    expect_info(info, dict(ASYM, elem=elem, kernel=kernel), tag)
    nvec = info["ld"] // VEC[elem]
    if kernel in (1, 2):
        assert block == 0 or info["block"] == block, (tag, info["block"])
        assert (info["wgs_per_tour"] == 1) if wgs == 1 else (info["wgs_per_tour"] > 1), (tag, info["wgs_per_tour"])
    else:
        own = min(1024, max(64, (nvec + 63) // 64 * 64))
        fits = block > 0 and (nvec + block - 1) // block <= (1 if elem == 3 else 2)
        assert info["block"] == (block if fits else own), (tag, info["block"], own)
        P = info["lds_bytes"] // (info["ld"] * 16 // VEC[elem]) - 1       # whole rows in the dynamic LDS, less the one of succ
        assert 2 <= P <= 8 and info["wgs_per_tour"] == (info["n"] + P - 1) // P > 1, (tag, P, info["wgs_per_tour"], info["lds_bytes"])
    if kernel == 1:
        return 0
    return (nvec + info["block"] - 1) // info["block"]


def refusal_allowed(e, kernel, info):
    """the one refusal a sweep geometry may meet: the resident sweep with uint16 cells on a row of more than one chunk of
    1024 threads (no instance of this file is that long, so every combination has to run)"""
    return e.code == 8 and kernel == 3 and info["elem"] == 3 and info["ld"] // VEC[3] > 1024


def geometries():
    return list(itertools.product(KERNELS, BLOCKS, WGS))


def set_geometry(eng, T, kernel, block, wgs):
    options(eng, {T.OPT_KERNEL: kernel, T.OPT_BLOCK: block, T.OPT_WGS_PER_TOUR: wgs})


@gpu
@pytest.mark.parametrize("elem,n", ROWS)
def test_planted_single_sweeps(clean, T, O, elem, n):
    """every planted case on every geometry (kernel 1, 2, 3 x block auto, 64, 128 x workgroups auto, 1), through
    two_opt_once on a host tour and through a slot with tour_two_opt(max_sweeps = 1) and the history: (min, max, delta),
    the cost start + delta and the whole successor array -- the reference's arc succ a .. b flipped, up to n - 1 cells long
    and across the array end -- are the oracle's"""
    eng = clean
    fx = planted_fixture(O, n, SPAN[elem])
    options(eng, {T.OPT_ELEM: elem, T.OPT_HISTORY: HIST})
    chunks, ran, wgs_seen = set(), 0, set()
    for p in fx:
        eng.set_costs(p.c)
        for kernel, block, wgs in geometries():
            tag = (n, elem, p.a, p.b, kernel, block, wgs)
            set_geometry(eng, T, kernel, block, wgs)
            path = p.tour.copy()
            try:
                d, cost = eng.two_opt_once(path, p.cost0)
            except T.TspGpuError as e:
                assert refusal_allowed(e, kernel, eng.info()), (tag, e)
                continue
            assert (d, cost) == (p.delta, p.cost) and np.array_equal(path, p.succ), (tag, d, cost, p.delta, p.cost)
            info = eng.info()
            chunks.add((kernel, check_geometry(info, elem, kernel, block, wgs, tag)))
            wgs_seen.add(info["wgs_per_tour"] > 1)
            eng.tour_load(0, p.tour)
            sweeps, rc = eng.tour_two_opt(0, max_sweeps=1)
            ha, hb, hd = eng.history(HIST)
            succ, cost, last = eng.tour_store(0)
            assert (rc, sweeps, len(ha)) == (0, 1, 1), tag
            assert (min(ha[0], hb[0]), max(ha[0], hb[0]), hd[0]) == (p.move[0], p.move[1], p.delta), (tag, ha, hb, hd)
            assert (cost, last) == (p.cost, p.delta) and np.array_equal(succ, p.succ), tag
            assert check_geometry(eng.info(), elem, kernel, block, wgs, tag) == check_geometry(info, elem, kernel, block, wgs, tag)
            ran += 1
    assert ran == len(fx) * len(geometries()) and wgs_seen == {False, True}
    per_kernel2 = {c for k, c in chunks if k == 2}
    assert (1, 0) in chunks and {c for k, c in chunks if k == 3} >= ({1} if elem == 3 else {1, 2}), chunks
    assert per_kernel2 >= ({1, 2} if n == 130 else {1, 2, 3} if n < 1537 else {1, 2, 4}), chunks


@gpu
@pytest.mark.parametrize("elem,n", ROWS)
def test_planted_tabu_moves(clean, T, O, elem, n):
    """the same cases through tabu_move against the oracle's, on every geometry: with nothing tabu (a zero delta can win now,
    and in the case without a planted pair the best admissible delta is positive), and with every third node of a's wave
    stamped within the tenure (the bit mask of the packed state and the verdict bytes in LDS)"""
    eng = clean
    S = SPAN[elem]
    fx = planted_fixture(O, n, S)
    options(eng, {T.OPT_ELEM: elem})
    ran, positive = 0, 0
    for p in fx:
        eng.set_costs(p.c)
        for tl, tenure, it in tabu_lists(n, S, p.a):
            osucc, ostamps, ocost, omv = oracle_tabu(O, p, tl, tenure, it)
            assert omv[0] >= 0
            positive += ocost > p.cost0
            for kernel, block, wgs in geometries():
                tag = (n, elem, p.a, p.b, int((tl >= 0).sum()), kernel, block, wgs)
                set_geometry(eng, T, kernel, block, wgs)
                path, stamps = p.tour.copy(), tl.copy()
                try:
                    cost = eng.tabu_move(path, p.cost0, stamps, tenure, it)
                except T.TspGpuError as e:
                    assert refusal_allowed(e, kernel, eng.info()), (tag, e)
                    continue
                assert cost == ocost and np.array_equal(path, osucc) and np.array_equal(stamps, ostamps), (tag, cost, ocost, omv)
                check_geometry(eng.info(), elem, kernel, block, wgs, tag)
                ran += 1
    assert ran == len(fx) * 2 * len(geometries()) and positive >= 1


# ------------------------------------------------------------------ 2. capped descents
def engine_descent(eng, start, cap, load=True):
    if load:
        eng.tour_load(0, start)
    sweeps, rc = eng.tour_two_opt(0, max_sweeps=cap)
    a, b, d = (np.array(v) for v in eng.history(HIST))
    succ, cost, _ = eng.tour_store(0)
    return rc, sweeps, np.minimum(a, b), np.maximum(a, b), d, succ, cost, eng.info()


def same_moves(got, want, lo, hi, tag):
    """the sweeps lo .. hi-1 of the oracle's run: the count and (a, b, delta) of each"""
    rc, sweeps, a, b, d = got[:5]
    assert rc == 0 and sweeps == hi - lo and len(a) == hi - lo, (tag, rc, sweeps, len(a))
    bad = np.nonzero((a != want.a[lo:hi]) | (b != want.b[lo:hi]) | (d != want.d[lo:hi]))[0]
    assert len(bad) == 0, (tag, "sweep", lo + int(bad[0]), "engine", (int(a[bad[0]]), int(b[bad[0]]), float(d[bad[0]])),
                           "oracle", (int(want.a[lo + bad[0]]), int(want.b[lo + bad[0]]), float(want.d[lo + bad[0]])))


def same_descent(got, want, tag):
    """a whole run: every move, the carried cost and the successor array, all bit-exact"""
    same_moves(got, want, 0, want.sweeps, tag)
    assert got[6] == want.cost and np.array_equal(got[5], want.succ), (tag, got[6], want.cost)


@gpu
@pytest.mark.parametrize("start", ["nn", "perm"])
@pytest.mark.parametrize("n,hi", DESCENTS)
def test_capped_descents_every_move(clean, T, O, n, hi, start):
    """40 sweeps from NN(0) / the permutation tour on every cell type that admits the matrix and AUTO (uint16 where the
    costs allow), kernels 1, 2, 3, graph replay and eager launches, batches of 32 and of 7 (the cap crosses batch boundaries
    unevenly): every (a, b, delta), the sweep count, the carried cost and the final successor array are the oracle's"""
    eng = clean
    c, want = descent_fixture(O, n, hi, start)
    elems, auto = elems_of(hi)
    eng.set_option(T.OPT_HISTORY, HIST)
    ran = 0
    for elem in [0] + elems:
        eng.set_option(T.OPT_ELEM, elem)
        eng.set_costs(c)
        assert eng.info()["elem"] == (elem or auto) and eng.info()["symmetric"] == 0
        if start == "nn":
            g, gcost = eng.nn_tour(0)
            assert gcost == want.cost0 and np.array_equal(g, want.start)
        for kernel, graph, batch in itertools.product(KERNELS, (1, 0), (32, 7)):
            tag = (n, hi, start, elem, kernel, graph, batch)
            options(eng, {T.OPT_KERNEL: kernel, T.OPT_GRAPH: graph, T.OPT_BATCH: batch})
            try:
                got = engine_descent(eng, want.start, CAP)
            except T.TspGpuError as e:
                assert refusal_allowed(e, kernel, eng.info()), (tag, e)
                continue
            same_descent(got, want, tag)
            expect_info(got[7], dict(ASYM, elem=elem or auto, kernel=kernel), tag)
            ran += 1
    assert ran == (len(elems) + 1) * 12


@gpu
@pytest.mark.parametrize("elem,n,hi", [(1, 300, 9), (3, 1100, 65534)])
def test_a_continued_slot_carries_its_cost(clean, T, O, elem, n, hi):
    """20 + 20 sweeps on one slot without a load in between.  tour_two_opt re-arms the slot's sweep counter and its done
    flag and leaves its cost alone, so the cost is carried across the calls: the two calls together are ONE oracle run of
    40 sweeps with the carried cost (not two runs that each begin at the cost of their tour), move for move"""
    eng = clean
    c, want = descent_fixture(O, n, hi, "perm")
    options(eng, {T.OPT_ELEM: elem, T.OPT_HISTORY: HIST})
    eng.set_costs(c)
    first = engine_descent(eng, want.start, 20)
    same_moves(first, want, 0, 20, "first")
    assert first[6] == want.cost0 + want.d[:20].sum()
    second = engine_descent(eng, None, 20, load=False)
    same_moves(second, want, 20, 40, "second")
    assert second[6] == want.cost and np.array_equal(second[5], want.succ)
    expect_info(second[7], dict(ASYM, elem=elem), "second")


@gpu
@pytest.mark.parametrize("elem,n,hi", [(1, 300, 9), (2, 300, 9), (3, 600, 999)])
def test_multistart_batch(clean, T, O, elem, n, hi):
    """starts 0 .. 7 in one batch (blockIdx.y slots) with 12 sweeps each, against a loop over the oracle: NN, 12 sweeps, the
    best by carried cost with a strict <; the best start, its cost and tour, and the total sweep count"""
    eng = clean
    c = asym_matrix(n, hi)

    def make():
        best, total = None, 0
        for s in range(8):
            succ, _ = O.nn_tour(c, s)
            sw, cost = O.two_opt(c, succ, 12)
            total += sw
            if best is None or cost < best[1]:
                best = (s, cost, succ)
        return best, total
    (ostart, ocost, osucc), ototal = cached(("multi", n, hi), make)
    assert ototal == 8 * 12
    options(eng, {T.OPT_ELEM: elem, T.OPT_SWEEP_CAP: 12})
    eng.set_costs(c)
    for kernel in (0, 1, 2, 3):
        eng.set_option(T.OPT_KERNEL, kernel)
        res = eng.multistart_nn_2opt(starts=np.arange(8))
        assert (res["rc"], res["start"], res["cost"], res["sweeps"]) == (0, ostart, ocost, ototal), (kernel, res["start"], res["cost"], res["sweeps"])
        assert np.array_equal(res["path"], osucc), kernel
        expect_info(eng.info(), dict(ASYM, elem=elem, **({"kernel": kernel} if kernel else {})), kernel)


@gpu
@pytest.mark.parametrize("elem,n,hi", [(1, 130, 999), (2, 517, 60000), (3, 1100, 65534)])
def test_tabu_walk(clean, T, O, elem, n, hi):
    """tabu_search with k = 80 from NN(0): the trace, the final tour and cost and the incumbent tour and cost are the
    oracle's; the LDS-resident walk never takes such a matrix (info 15 reads 0)"""
    eng = clean
    c = asym_matrix(n, hi)
    k = 80

    def make():
        s, cost0 = O.nn_tour(c, 0)
        start = s.copy()
        best, best_cost, final, trace = O.tabu_search(c, s, cost0, k)
        return start, cost0, best, best_cost, final, trace, s
    start, cost0, obest, obest_cost, ofinal, otrace, opath = cached(("walk", n, hi), make)
    eng.set_option(T.OPT_ELEM, elem)
    eng.set_costs(c)
    for kernel in (0, 1, 2, 3):
        eng.set_option(T.OPT_KERNEL, kernel)
        path = start.copy()
        best, best_cost, final, trace = eng.tabu_search(path, cost0, k, want_trace=True)
        bad = np.nonzero(trace != otrace)[0]
        assert len(bad) == 0, (kernel, "iteration", int(bad[0]), float(trace[bad[0]]), float(otrace[bad[0]]))
        assert final == ofinal and np.array_equal(path, opath), kernel
        assert best_cost == obest_cost and np.array_equal(best, obest), kernel
        assert eng.L.tspgpu_info(eng.ctx, 15) == 0
        expect_info(eng.info(), dict(ASYM, elem=elem, **({"kernel": kernel} if kernel else {})), kernel)


# ------------------------------------------------------------------ 3. the constructions
@gpu
@pytest.mark.parametrize("n,hi", [(130, 999), (517, 60000)])
def test_nearest_neighbour(clean, T, O, n, hi):
    """nn_tour from 0, n // 2 and n - 1 and nn_all over every start, every cell type, the automatic and the matrix NN kernel:
    c[cur][i] is read from the row of cur"""
    eng = clean
    c = asym_matrix(n, hi)
    want = cached(("nn", n, hi), lambda: ([O.nn_tour(c, s) for s in (0, n // 2, n - 1)], O.nn_all(c)))
    for elem, nnk in itertools.product((1, 2, 3), (0, 1)):
        options(eng, {T.OPT_ELEM: elem, T.OPT_NN_KERNEL: nnk})
        eng.set_costs(c)
        for s, (osucc, ocost) in zip((0, n // 2, n - 1), want[0]):
            g, gcost = eng.nn_tour(s)
            assert gcost == ocost and np.array_equal(g, osucc), (elem, nnk, s)
        best, cost, arg = eng.nn_all()
        assert (cost, arg) == want[1][1:] and np.array_equal(best, want[1][0]), (elem, nnk)
        expect_info(eng.info(), {"symmetric": 0, "elem": elem, "nn_grid": 0}, (elem, nnk))


@gpu
@pytest.mark.parametrize("hi", [9, 1000, 60000])
@pytest.mark.parametrize("n", [70, 300])
def test_farthest_pair_and_extra_mileage(clean, T, O, n, hi):
    """farthest_pair (the pairs i < j of the upper triangle only) and extra_mileage in both forms on every cell type,
    against the model: the tour, the cost and the stale-rescan count; c[i][v] is read from the row of i"""
    from test_extra_mileage import em_model, farthest_pair
    eng = clean
    c = asym_matrix(n, hi)
    a, b = farthest_pair(c)
    msucc, mcost, mstale = cached(("em", n, hi), lambda: em_model(c, a, b))
    assert O.valid_tour(msucc)
    for elem, form in itertools.product((1, 2, 3), (1, 2)):
        options(eng, {T.OPT_ELEM: elem, T.OPT_EM_FORM: form})
        eng.set_costs(c)
        assert eng.farthest_pair() == (a, b, c[a, b]), (elem, form)
        succ, cost, rc = eng.extra_mileage()
        assert rc == 0 and cost == mcost and np.array_equal(succ, msucc), (elem, form, cost, mcost)
        expect_info(eng.info(), {"symmetric": 0, "elem": elem, "em_form": form, "em_stale": mstale, "em_steps": n - 2}, (elem, form))


# ------------------------------------------------------------------ 4. refusals and lifetime
@gpu
def test_refusals_leave_the_context_working(clean, T, O):
    """on one context holding a non-symmetric matrix: the LDS-resident and the streamed one-launch descent, where demanded,
    fail with 8, a sharded sweep with 9; OPT_FUSED = 2 is no error and runs the same moves; after each of them the context
    still computes the capped descent"""
    eng = clean
    c, want = descent_fixture(O, 1100, 65534, "perm")
    eng.set_option(T.OPT_HISTORY, HIST)
    eng.set_costs(c)
    assert eng.info()["elem"] == 3 and eng.info()["symmetric"] == 0

    def still_works(tag):
        got = engine_descent(eng, want.start, CAP)
        same_descent(got, want, tag)
        expect_info(got[7], dict(ASYM, elem=3), tag)
    still_works("before")
    for tag, opts in (("persist", {T.OPT_PERSIST: 2}), ("stream", {T.OPT_PERSIST: 0, T.OPT_STREAM_PERSIST: 2})):
        options(eng, opts)
        eng.tour_load(0, want.start)
        with pytest.raises(T.TspGpuError) as ei:
            eng.tour_two_opt(0, max_sweeps=CAP)
        assert ei.value.code == 8, tag
        options(eng, {T.OPT_PERSIST: 1, T.OPT_STREAM_PERSIST: 1})
        still_works(tag)
    eng.tour_load(0, want.start)
    with pytest.raises(T.TspGpuError) as ei:
        eng.tour_sweep_part(0, 0, 1)
    assert ei.value.code == 9
    still_works("sweep_part")
    eng.set_option(T.OPT_FUSED, 2)
    still_works("fused")


@gpu
def test_one_context_symmetric_asymmetric_symmetric(clean, T, O):
    """one context at n = 517 with int32 cells, graphs on and slot 0 loaded throughout: a symmetric matrix, a non-symmetric
    one, the first again.  Each segment reproduces its own oracle run of 30 sweeps; info()'s symmetric and fused follow the
    matrix; the slot of the previous matrix is refused (9) until it is loaded again"""
    eng = clean
    n, cap = 517, 30
    asym = asym_matrix(n, 60000)
    sym = cached(("sym", n), lambda: np.ascontiguousarray(np.triu(asym, 1) + np.triu(asym, 1).T - np.eye(n)))
    assert np.array_equal(sym, sym.T) and (np.diag(sym) == -1).all()
    start = perm_tour(n)
    runs = {"sym": cached(("life", "sym"), lambda: Descent(O, sym, start, cap=cap)),
            "asym": cached(("life", "asym"), lambda: Descent(O, asym, start, cap=cap))}
    assert all(r.sweeps == cap and (r.a >= 0).all() for r in runs.values())
    options(eng, {T.OPT_ELEM: 2, T.OPT_HISTORY: HIST, T.OPT_GRAPH: 1})
    for seg, name in enumerate(("sym", "asym", "sym")):
        eng.set_costs(sym if name == "sym" else asym)
        if seg:
            with pytest.raises(T.TspGpuError) as ei:
                eng.tour_two_opt(0, max_sweeps=cap)
            assert ei.value.code == 9, seg
            with pytest.raises(T.TspGpuError) as ei:
                eng.tour_store(0)
            assert ei.value.code == 9, seg
        got = engine_descent(eng, start, cap)
        same_descent(got, runs[name], (seg, name))
        expect_info(got[7], {"elem": 2, "symmetric": int(name == "sym"), "fused": int(name == "sym"), "persist": 0}, (seg, name))


# ------------------------------------------------------------------ 5. a small fuzz of its own
_TALLY = {"ran": 0, "refused": 0, "sweeps": 0}
SEEDS = int(os.environ.get("TSP_ASYM_FUZZ_SEEDS", "30"))


@gpu
@pytest.mark.parametrize("seed", range(SEEDS))
def test_random_asymmetric_configurations_against_the_oracle(clean, T, O, seed):
    """a random non-symmetric matrix -- every cell drawn, or a symmetric one with exactly one cell pair made unequal, the
    smallest thing that flips `symmetric` --, a random cell type, kernel, block, workgroup count, graph or eager, NN or
    permutation start: up to 30 sweeps against the oracle, move by move.  A refusal is 8 or 3 with a reason"""
    eng = clean
    r = np.random.RandomState(5000 + seed)
    n = int(r.choice([r.randint(8, 65), r.randint(64, 301), r.randint(300, 1301)]))
    hi = int(r.choice([9, 999, 60000]))
    c = r.randint(1, hi + 1, size=(n, n)).astype(np.float64)
    one_cell = bool(r.randint(2))
    if one_cell:
        c = np.triu(c, 1)
        c = c + c.T
        i, j = (int(v) for v in r.choice(n, 2, replace=False))
        c[i, j] += 1.0
    np.fill_diagonal(c, -1.0)
    c = np.ascontiguousarray(c)
    assert (int((c != c.T).sum()) == 2) if one_cell else (not np.array_equal(c, c.T))
    opts = dict(elem=int(r.choice([0, 1, 2, 3])), kernel=int(r.choice([0, 1, 2, 3])), block=int(r.choice([0, 64, 128, 256])),
                wgs=int(r.choice([0, 1, 3])), graph=int(r.randint(2)))
    if r.randint(2):
        start = O.nn_tour(c, int(r.randint(n)))[0]
    else:
        perm = r.permutation(n).astype(np.int32)
        start = np.empty(n, dtype=np.int32)
        start[perm] = np.roll(perm, -1)
    tag = dict(opts, seed=seed, n=n, hi=hi, one_cell=one_cell)
    want = Descent(O, c, start, cap=30)
    options(eng, {T.OPT_ELEM: opts["elem"], T.OPT_KERNEL: opts["kernel"], T.OPT_BLOCK: opts["block"], T.OPT_WGS_PER_TOUR: opts["wgs"],
                  T.OPT_GRAPH: opts["graph"], T.OPT_HISTORY: HIST})
    try:
        eng.set_costs(c)
        got = engine_descent(eng, start, 30)
    except T.TspGpuError as e:
        assert e.code in (8, 3) and len(str(e).split(": ", 1)[1]) > 0, (tag, e)
        _TALLY["refused"] += 1
        return
    rc, sweeps, a, b, d, succ, cost, info = got
    moved = want.a >= 0
    assert rc == 0 and sweeps == want.sweeps and len(a) == want.sweeps, (tag, rc, sweeps, want.sweeps)
    bad = np.nonzero((a != want.a) | (moved & ((b != want.b) | (d != want.d))))[0]
    assert len(bad) == 0, (tag, "sweep", int(bad[0]), (int(a[bad[0]]), int(b[bad[0]]), float(d[bad[0]])),
                           (int(want.a[bad[0]]), int(want.b[bad[0]]), float(want.d[bad[0]])))
    assert cost == want.cost and np.array_equal(succ, want.succ), (tag, cost, want.cost)
    expect_info(info, dict(ASYM, **({"elem": opts["elem"]} if opts["elem"] else {}), **({"kernel": opts["kernel"]} if opts["kernel"] else {})), tag)
    _TALLY["ran"] += 1
    _TALLY["sweeps"] += sweeps


@gpu
def test_random_asymmetric_configurations_mostly_ran(capsys):
    """(runs after the seeds above) at least two thirds of the configurations exist and ran"""
    with capsys.disabled():
        print(f"\n[asymmetric fuzz] {_TALLY}")
    assert 3 * _TALLY["ran"] >= 2 * SEEDS, _TALLY
