"""Or-opt at every sweep launch geometry and every apply rotation (include/tspgpu.h "Or-opt", DESIGN 4.12 "Geometry classes").

The model is tests/test_or_opt.py's (the C restatement of the sweep, apply_move, descent_model), imported from there.  Every
comparison is exact: the costs are integers held in doubles.

1. Sweep classes.  The plan picks threads per workgroup (BT) and 16-byte vectors per thread and row (NCH) from the row
   stride; every (cell type, BT, NCH) class and the largest accepted size of each type run K = 6 moves from the identity
   tour on random points, move by move (or_opt_once reloads the path) and then in a slot (tour_or_opt keeps it).  The class is
   read from info()["or_block"] / ["or_nch"].  One node past the limit is refused.
2. Batched sweep at NCH = 2 and 3.  A planted matrix -- 1000 + noise everywhere, the edges of a random base tour at
   100 + (position mod 97), the new edges of a handful of planted moves at 1 -- and start tours that are the base tour with
   some of the planted moves already made (batch_instance lists them): five Or-opt moves of four (L, rev) kinds, one 2-opt
   move that an Or-opt move opens and that opens another, so the tours take 3, 2, 3, 2 and 1 rounds and leave the batch at
   different times.  Every slot but the extra fifth makes an Or-opt move.
3. Apply.  A planted matrix makes one chosen move the best one (tour edges 100, the move's three new edges 1); the tests
   ask the MODEL which move that is and derive the rotation class from it: forward / backward, one / several chunks of the
   apply workgroup, across cell n-1 -> 0 or not, slot direction +1 / -1 (-1: a 2-opt move over the longer arc first).  A 2-opt
   sweep and another Or-opt sweep follow, which read the cached edge costs the apply has patched.

Model cost.  A case whose model side takes more than about 5 s on the CPU is read from tests/golden/golden_or_opt_geometry.json
(oracle/make_golden_or_opt_geometry.py, which runs the functions of this module and prints the seconds of each case); the
others are computed here.  Measured on 8 CPU cores, seconds for the whole model side of a case (matrix included):
    walks (K = 6):     n = 300, 600, 1100: 0.1 | 2100: 0.8 | 4100: 3.1 | 5024: 6.3 (golden) | 8200: 22 (golden)
                       | 10048: 34 (golden) | 16400: 124 (golden) | 20096: 188 (golden)
    batches (5 tours, one thread each): n = 1100: 0.5 | 2100: 1.5 | 4100: 8.8 (golden) | 8200: 38 (golden) | 16400: 182 (golden)
A GPU test of a golden walk rebuilds the paths from the trace with apply_move and never forms the host matrix; a batch test
still builds the host matrix for set_costs: batch_instance takes 1.1 s at n = 8200 (0.5 GB) and 4.7 s at n = 16400 (2.2 GB),
measured on the CPU host, set_costs not included.

Not here: the batch descents the issue describes, on a "hidden cycle" matrix (cycle edges 10, the rest 1000 + noise) from
the cycle with a few segments displaced.  On the model 2-opt alone repairs 2942 of 3000 such starts (n = 200) and none takes
a third round, so no batch of them has an Or-opt move in every tour and tours that differ in rounds.  Section 2 keeps
those two requirements and the noise matrix, and plants the moves instead."""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import oracle as O  # noqa: E402
import test_or_opt as M  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_or_opt_geometry.json")
F64, I32, U16 = 1, 2, 3
K = 6
COUNTS = ("two_opt_sweeps", "or_moves", "rounds")
RESOURCE_EXHAUSTED = 8

# (cell type, n, BT, NCH): the smallest convenient n of every class, no multiple of 32, and the largest accepted n of each type
SWEEP_CASES = [
    (F64, 300, 256, 1), (F64, 600, 512, 1), (F64, 1100, 512, 2), (F64, 2100, 1024, 2), (F64, 4100, 1024, 3), (F64, 5024, 1024, 3),
    (I32, 600, 256, 1), (I32, 1100, 512, 1), (I32, 2100, 512, 2), (I32, 4100, 1024, 2), (I32, 8200, 1024, 3), (I32, 10048, 1024, 3),
    (U16, 1100, 256, 1), (U16, 2100, 512, 1), (U16, 4100, 512, 2), (U16, 8200, 1024, 2), (U16, 16400, 1024, 3), (U16, 20096, 1024, 3),
]
LIMITS = {F64: 5024, I32: 10048, U16: 20096}
GOLDEN_WALKS = (5024, 8200, 10048, 16400, 20096)          # the 5 s rule (module docstring)
# (cell type, n, BT, NCH) of the batch cases
BATCH_CASES = [
    (F64, 1100, 512, 2), (F64, 2100, 1024, 2), (F64, 4100, 1024, 3),
    (I32, 4100, 1024, 2), (I32, 8200, 1024, 3),
    (U16, 4100, 512, 2), (U16, 8200, 1024, 2), (U16, 16400, 1024, 3),
]
GOLDEN_BATCHES = (4100, 8200, 16400)


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def identity_tour(n):
    return np.roll(np.arange(n, dtype=np.int32), -1)


def path_of(seq):
    """successor array of the cyclic node sequence"""
    seq = np.asarray(seq, np.int64)
    path = np.empty(len(seq), np.int32)
    path[seq] = np.roll(seq, -1)
    return path


def forward_order(path, first=0):
    n = len(path)
    out = np.empty(n, np.int64)
    v = first
    for i in range(n):
        out[i] = v
        v = int(path[v])
    assert v == first
    return out


def sha(path):
    return hashlib.sha256(np.ascontiguousarray(path, "<i4").tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------------ 1. sweep walks
def model_sweep_walk(n):
    """the model's first K moves from the identity tour on random_points(n) -> (start cost, trace); forms the n^2 matrix"""
    c = O.cost_matrix(M.instance_xy("n%d" % n))
    start = identity_tour(n)
    cost = O.tour_cost(c, start)
    trace, _ = M.walk(c, start.copy(), cost, K)
    return cost, trace


@functools.lru_cache(maxsize=None)
def sweep_walk(n):
    """-> (start, cost, trace, paths); from the golden file where the model is slow, the paths rebuilt with apply_move"""
    if n in GOLDEN_WALKS:
        g = golden()["walks"][str(n)]
        cost, trace = float(g["cost"]), [(float(m[0]), int(m[1]), int(m[2]), int(m[3]), int(m[4])) for m in g["trace"]]
    else:
        cost, trace = model_sweep_walk(n)
    start = identity_tour(n)
    path, paths = start.copy(), []
    for mv in trace:
        M.apply_move(path, *mv[1:])
        paths.append(path.copy())
    return start, cost, trace, paths


def move_delta_xy(xy, path, prev, s, L, q, rev):
    """delta of a legal Or-opt move from the coordinates: the weights of the six edges involved, in the definition's order"""
    n = len(path)
    assert L in (1, 2, 3) and rev in (0, 1) and (L > 1 or rev == 0) and 0 <= s < n and 0 <= q < n
    seg = [s]
    for _ in range(L - 1):
        seg.append(int(path[seg[-1]]))
    t = seg[-1]
    p, x, qn = int(prev[s]), int(path[t]), int(path[q])
    assert q != p and q not in seg and len({p, x, *seg}) == L + 2
    h, e = (t, s) if rev else (s, t)
    w = O.cost_rows(xy, [p, t, q, e])
    return ((w[0][x] + w[2][h]) + w[3][qn]) - ((w[0][s] + w[1][x]) + w[2][qn])


def test_golden_walks_replay():
    """every golden trace from its start tour: legal moves, a valid tour after each, each delta the change in tour length"""
    assert set(golden()["walks"]) == {str(n) for n in GOLDEN_WALKS}
    for n in GOLDEN_WALKS:
        xy = M.instance_xy("n%d" % n)
        start, cost, trace, paths = sweep_walk(n)
        assert len(trace) == K and cost == O.tour_cost_xy(xy, O.EUC_2D, start)
        path = start.copy()
        for k, mv in enumerate(trace):
            prev = np.empty(n, np.int64)
            prev[path] = np.arange(n)
            d = move_delta_xy(xy, path, prev, *mv[1:])
            assert d == mv[0] and d < M.EPS, (n, k, d, mv)
            M.apply_move(path, *mv[1:])
            assert O.valid_tour(path) and np.array_equal(path, paths[k]), (n, k)
            cost += d
            assert cost == O.tour_cost_xy(xy, O.EUC_2D, path), (n, k)


def test_sweep_cases_cover_the_table():
    """every class of every type once below the limit, the limit itself, and the small walks reach K moves"""
    for elem in (F64, I32, U16):
        mine = [c for c in SWEEP_CASES if c[0] == elem]
        assert {(bt, nch) for _, _, bt, nch in mine} == {(256, 1), (512, 1), (512, 2), (1024, 2), (1024, 3)}
        assert mine[-1][1] == LIMITS[elem] and all(n % 32 for _, n, _, _ in mine[:-1])
    for n in (300, 600, 1100):
        assert len(sweep_walk(n)[2]) == K


@pytest.mark.gpu
@pytest.mark.parametrize("elem,n,bt,nch", SWEEP_CASES)
def test_gpu_sweep_class(elem, n, bt, nch):
    eng = M.engine_for("n%d" % n, elem)
    info = eng.info()
    assert (info["elem"], info["or_block"], info["or_nch"]) == (elem, bt, nch), info
    start, cost, trace, paths = sweep_walk(n)
    assert len(trace) == K
    M.check_walk(eng, start, cost, trace, paths, limit=K)
    eng.tour_load(0, start)                             # the slot form: no reload between the moves
    assert eng.tour_or_opt(0, max_moves=K) == (K, 0)
    path, gcost, _ = eng.tour_store(0)
    assert np.array_equal(path, paths[-1]) and gcost == cost + sum(mv[0] for mv in trace)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("elem", [F64, I32, U16])
def test_gpu_one_past_the_limit_is_refused(elem):
    """n = limit + 1 rounds the row stride up one step: code 8, and the text names the limit"""
    n = LIMITS[elem] + 1
    eng = M.engine_for("n%d" % n, elem)
    assert eng.info()["elem"] == elem
    M.refused(eng, RESOURCE_EXHAUSTED, n, word=str(LIMITS[elem]))
    eng.close()


# ---------------------------------------------------------------------------------------------------- 2. batch descents
def batch_instance(n):
    """-> (matrix, start tours).  1000 + symmetric integer noise in [0, 400); the edges of a random base tour f at 100 + (k mod 97),
    k the position of the edge, so that no two neighbouring cached edge costs are equal; planted edges at 1.  Planted on f:
      A  Or-opt (L = 3, rev = 0): f[11..13] to between f[200] and f[201]
      T  2-opt, possible only after A (f[10] then precedes f[14]): new edges {f[10], f[40]} and {f[14], f[41]}
      C  Or-opt (L = 3, reversed), possible only after T (f[14] and f[41] are then neighbours): f[300..302] to between them
      B  Or-opt (L = 2, rev = 1): f[500..501] to between f[700] and f[701]
      E  Or-opt (L = 1), possible only after B: f[600] to between f[499] and f[502]
      D  Or-opt (L = 3, rev = 0): f[800..802] to between f[900] and f[901]
    (L, rev) = (2, 0) and L = 1 on the untouched tour are left out: one 2-opt move then adds two of the three planted edges,
    and the 2-opt phase, which comes first, takes it.  The start tours: f; f with A, B, E, D made; f with B, E; f with A, D;
    and, as an extra, f with everything made (no move at all).  The descents need
        slot 0: Or-opt A B E D | 2-opt T, Or-opt C | nothing           3 rounds, 5 Or-opt moves
        slot 1: 2-opt T, Or-opt C | nothing                             2 rounds, 1
        slot 2: Or-opt A D | 2-opt T, Or-opt C | nothing                3 rounds, 3
        slot 3: 2-opt T, Or-opt C B E | nothing                         2 rounds, 3
        slot 4: nothing                                                 1 round,  0"""
    rng = np.random.default_rng(7000 + n)
    a = np.triu(rng.integers(0, 400, (n, n), dtype=np.int16), 1)
    a += a.T
    c = a.astype(np.float64)
    del a
    c += 1000.0
    f = rng.permutation(n)
    base = path_of(f)
    w = 100.0 + np.arange(n) % 97
    c[f, base[f]] = w
    c[base[f], f] = w
    f = [int(v) for v in f]
    for u, v in ((10, 14), (200, 11), (13, 201),            # A
                 (10, 40), (14, 41),                        # T
                 (299, 303), (14, 302), (300, 41),          # C
                 (499, 502), (700, 501), (500, 701),        # B
                 (599, 601), (499, 600), (600, 502),        # E
                 (799, 803), (900, 800), (802, 901)):       # D
        c[f[u], f[v]] = c[f[v], f[u]] = 1.0
    np.fill_diagonal(c, -1.0)
    A, B, E, D = (f[11], 3, f[200], 0), (f[500], 2, f[700], 1), (f[600], 1, f[499], 0), (f[800], 3, f[900], 0)

    def made(*moves):
        path = base.copy()
        for mv in moves:
            M.apply_move(path, *mv)
        return path
    done = made(A, B, E, D)
    O.apply_move(done, None, min(f[10], f[40]), max(f[10], f[40]))              # T, as the 2-opt sweep orders its pair
    s = f[300] if done[f[300]] == f[301] else f[302]                            # C in the orientation T has left
    q, h = (f[14], f[302]) if done[f[14]] == f[41] else (f[41], f[300])
    assert done[q] in (f[14], f[41])
    M.apply_move(done, s, 3, q, int(h != s))
    return c, [base, made(A, B, E, D), made(B, E), made(A, D), done]


def batch_model(c, starts):
    """descent_model per start, one thread each (the C model runs without the interpreter lock) ->
    [dict(cost, two_opt_sweeps, or_moves, rounds, sha256, path)]"""
    from concurrent.futures import ThreadPoolExecutor

    def one(s):
        path = s.copy()
        res = M.descent_model(c, path)
        res.update(path=path, sha256=sha(path))
        return res
    M.c_model(), O.lib()
    with ThreadPoolExecutor(max_workers=len(starts)) as ex:
        return list(ex.map(one, starts))


@functools.lru_cache(maxsize=None)
def batch_want(n):
    """the model's results of the batch case of size n (the golden's where the model is slow: no paths then)"""
    if n in GOLDEN_BATCHES:
        return tuple(golden()["batches"][str(n)])
    return tuple(batch_model(*batch_instance(n)))


def check_batch_shape(n, want):
    """the model does what batch_instance plants: every tour but the extra one makes an Or-opt move, the rounds differ, a
    2-opt sweep more than rounds where T is made, and every descent ends at the cost of the tour with everything made"""
    assert [w["or_moves"] for w in want] == [5, 1, 3, 3, 0] and [w["rounds"] for w in want] == [3, 2, 3, 2, 1], want
    assert [w["two_opt_sweeps"] for w in want] == [4, 3, 4, 3, 1], want
    assert len({w["cost"] for w in want}) == 1, want


def test_planted_batches_behave():
    """n = 1100 from the model, the golden cases from the file"""
    assert set(golden()["batches"]) == {str(n) for n in GOLDEN_BATCHES}
    c, starts = batch_instance(1100)
    assert all(O.valid_tour(s) for s in starts) and batch_want(1100)[0]["cost"] == O.tour_cost(c, starts[4])
    assert len({int(v) for v in c[np.arange(1100), starts[0]]}) == 97
    for n in (1100,) + GOLDEN_BATCHES:
        check_batch_shape(n, batch_want(n))


@pytest.mark.gpu
@pytest.mark.parametrize("elem,n,bt,nch", BATCH_CASES)
def test_gpu_batch_sweep_class(elem, n, bt, nch):
    c, starts = batch_instance(n)
    want = batch_want(n)
    check_batch_shape(n, want)
    eng = M.engine_for(costs=c, elem=elem)
    del c
    info = eng.info()
    assert (info["elem"], info["or_block"], info["or_nch"], info["symmetric"]) == (elem, bt, nch, 1), info
    for s, path in enumerate(starts):
        eng.tour_load(s, path)
    got = eng.tours_local_search(0, len(starts))
    assert got["rc"] == 0
    for i, w in enumerate(want):
        path, cost, _ = eng.tour_store(i)
        assert tuple(int(got[k][i]) for k in COUNTS) == tuple(w[k] for k in COUNTS), (i, [got[k][i] for k in COUNTS], w)
        assert cost == w["cost"] and sha(path) == w["sha256"], (i, cost, w["cost"])
        if "path" in w:
            assert np.array_equal(path, w["path"]), i
    eng.close()


# ------------------------------------------------------------------------------------------------------------ 3. apply
def apply_block(n):
    """threads of the apply workgroup = cells per rotation chunk (include/tspgpu.h "Or-opt")"""
    return min(1024, max(64, 1 << max(0, (n // 8 - 1).bit_length())))


@functools.lru_cache(maxsize=None)
def noise_matrix(n):
    rng = np.random.default_rng(300 + n)
    a = np.triu(rng.integers(0, 400, (n, n)), 1)
    c = (a + a.T + 1000).astype(np.float64)
    np.fill_diagonal(c, -1.0)
    return c


def planted_move_matrix(path, s, L, q, rev):
    """1000 + noise, the tour's edges 100, the three edges the move (s, L, q, rev) adds 1"""
    n = len(path)
    c = noise_matrix(n).copy()
    idx = np.arange(n)
    c[idx, path] = 100.0
    c[path, idx] = 100.0
    prev = np.empty(n, np.int64)
    prev[path] = idx
    t = s
    for _ in range(L - 1):
        t = int(path[t])
    p, x, qn = int(prev[s]), int(path[t]), int(path[q])
    h, e = (t, s) if rev else (s, t)
    for u, v in ((p, x), (q, h), (e, qn)):
        c[u, v] = c[v, u] = 1.0
    return c


class Layout:
    """the slot's position array as tour_load and a 2-opt apply leave it (DESIGN 4.12 / the Tours comment): after a load
    cell k holds the k-th node from node 0 and dir = +1; a 2-opt move (a, b), a < b, whose arc succ a .. b holds more than
    n / 2 nodes reverses the cells of the OTHER arc and toggles dir.  Only used to name the rotation class of a move: the
    applied results are compared with the model whatever this says, but the classes (and the dir = -1 half of the coverage) are
    this mirror's, not read from the device -- if the 2-opt apply stops toggling dir, this class must follow it."""

    def __init__(self, path):
        self.ord = forward_order(path)
        self.dir = 1

    def flip(self, a, b, arc):
        n = len(self.ord)
        assert self.dir == 1 and a < b and 2 * arc > n
        pos = np.empty(n, np.int64)
        pos[self.ord] = np.arange(n)
        i, j = int(pos[a]), int(pos[b])
        assert (j - i) % n == arc
        cells = (j + 1 + np.arange(n - arc)) % n
        self.ord[cells] = self.ord[cells][::-1].copy()
        self.dir = -1

    def forward(self):
        """node at forward position k"""
        return self.ord if self.dir > 0 else self.ord[::-1]

    def klass(self, s, L, q):
        """-> (rotation 'fwd' / 'back', cells of the rotated block, several chunks, crosses cell n-1 -> 0, dir)"""
        f = self.forward()
        n = len(f)
        a, b = int(np.nonzero(f == s)[0][0]), int(np.nonzero(f == q)[0][0])
        m1 = (b - (a + L)) % n + 1
        m2 = n - L - m1
        fwd = m2 < m1
        m = m2 if fwd else m1
        lo = (a - m if fwd else a) % n                  # the forward positions the rotation reads or writes: lo .. lo + m + L - 1
        return ("fwd" if fwd else "back", m, m > apply_block(n), lo + m + L - 1 >= n, self.dir)


def long_arc_flip(path):
    """2-opt moves (a, b), a < b, whose arc succ a .. b holds more than n / 2 nodes (and leaves two outside) -> [(a, b, arc)]"""
    f = forward_order(path)
    n = len(f)
    out = []
    for i in (1, 2, 0):
        for span in (3 * n // 4, n - 3 * n // 4):
            u, v = int(f[i]), int(f[(i + span) % n])
            arc = span if u < v else n - span
            if 2 * arc > n and n - arc >= 2:
                out.append((min(u, v), max(u, v), arc))
    assert out
    return out


def apply_case(tour0, flipped, plant):
    """the model's side of one case.  plant(path, layout) -> (s, L, q, rev) to plant on the tour the Or-opt move starts
    from.  -> dict: matrix, tour0, the planted move and the cells of its shorter block, flip (a, b, delta) or None, and
    (path, cost) after the flip, the Or-opt move (and the move), the 2-opt sweep, the second Or-opt sweep; klass of the
    model's move"""
    flips = long_arc_flip(tour0) if flipped else [None]
    for fl in flips:
        lay, path = Layout(tour0), tour0.copy()
        if fl:
            assert O.apply_move(path, None, fl[0], fl[1]) == fl[2]
            lay.flip(*fl)
            f = lay.forward()
            assert np.array_equal(path[f], np.roll(f, -1))
        planted = plant(path, lay)
        c = planted_move_matrix(path, *planted)
        cost0, cost = O.tour_cost(c, tour0), O.tour_cost(c, path)
        if fl is None or cost - cost0 < M.EPS:
            break
    else:
        raise AssertionError("no long-arc 2-opt move improves under the planted matrix")
    out = {"c": c, "tour0": tour0, "planted": planted, "planted_m": lay.klass(*planted[:3])[1], "flip": (fl[0], fl[1], cost - cost0) if fl else None, "cost0": cost0, "start": (path.copy(), cost)}
    cost, m, trace = M.or_opt_phase(c, path, cost, max_moves=1)
    assert m == 1, "the planted matrix left the model without an improving Or-opt move"
    out["move"], out["klass"] = trace[0], lay.klass(*trace[0][1:4])
    out["or1"] = (path.copy(), cost)
    _, cost, _ = O.two_opt_once(c, path, cost)
    out["two"] = (path.copy(), cost)
    cost, m, _ = M.or_opt_phase(c, path, cost, max_moves=1)
    out["or2"] = (path.copy(), cost, m)
    return out


def exhaustive_cases(n, tour0):
    """every (s, L, q, rev) on the tour the Or-opt move starts from, in both slot directions (by forward position: s at a, q
    from x round to the node before p)"""
    for flipped in (False, True):
        for a in range(n):
            for L, rev in ((1, 0), (2, 0), (2, 1), (3, 0), (3, 1)):
                for j in range(n - L - 1):
                    def plant(path, lay, a=a, L=L, rev=rev, j=j):
                        f = lay.forward()
                        return int(f[a]), L, int(f[(a + L + j) % n]), rev
                    yield apply_case(tour0, flipped, plant)


def chunk_lengths(n):
    bt = apply_block(n)
    return [1, 2, 3, 4, bt - 1, bt, bt + 1] + ([2 * bt] if 2 * bt < (n - 3) // 2 else []) + ["max"]


def chunk_cases(n, tour0):
    """rotations of m cells around the chunk size of the apply workgroup: forward and backward, across cell n-1 -> 0 and
    not, both slot directions; (L, rev) cycles through its five values, shifted so that each rotation meets all of them"""
    LR = ((1, 0), (2, 0), (2, 1), (3, 0), (3, 1))
    k = 0
    for flipped in (False, True):
        for rot in ("back", "fwd"):
            for wraps in (False, True):
                for mi, m in enumerate(chunk_lengths(n)):
                    L, rev = LR[(k + mi) % 5]
                    if m == "max":
                        m = (n - L) // 2 if rot == "back" else (n - L - 1) // 2
                    if rot == "back":                   # the block x .. q has m cells
                        a = n - 1 - (m + L - 1) // 2 if wraps else 2
                        b = a + L + m - 1
                    else:                               # the block q' .. p has m cells
                        a = m // 2 if wraps else m + 2
                        b = a - m - 1

                    def plant(path, lay, a=a, b=b, L=L, rev=rev):
                        f = lay.forward()
                        return int(f[a % n]), L, int(f[b % n]), rev
                    yield apply_case(tour0, flipped, plant)
                k += 1


ALL_CLASSES = {(r, ch, w, d) for r in ("fwd", "back") for ch in (False, True) for w in (False, True) for d in (1, -1)}


def classes_of(cases):
    return {(c["klass"][0],) + c["klass"][2:] for c in cases}


def apply_tours(n):
    return [identity_tour(n), M.random_tour(n, np.random.default_rng(40 + n))]


@functools.lru_cache(maxsize=None)
def chunk_case_list(n):
    """the chunk cases of size n without their matrices (rebuilt per cell type from the planted move: see run_apply_case)"""
    out = []
    for c in chunk_cases(n, apply_tours(n)[1]):
        c.pop("c")
        out.append(c)
    return out


def test_planted_moves_behave():
    """exhaustive at n = 8 and 12: the model takes a move in every case (apply_case asserts it), the planted one whenever
    both blocks exceed 3 nodes; the chunk cases at n = 150 and 1100 meet every rotation class and every (L, rev)"""
    for n in (8, 12):
        for tour0 in apply_tours(n):
            seen = both = 0
            for c in exhaustive_cases(n, tour0):
                seen += 1
                if c["planted_m"] > 3:
                    assert c["move"] == (-297.0,) + c["planted"], (c["move"], c["planted"])
                    both += 1
            assert seen == 2 * n * (n - 2 + 2 * (n - 3) + 2 * (n - 4)) and (both > 0) == (n == 12)
    for n in (150, 1100):
        cases = chunk_case_list(n)
        assert classes_of(cases) == ALL_CLASSES, ALL_CLASSES - classes_of(cases)
        for rot in ("fwd", "back"):
            for d in (1, -1):
                mine = [c for c in cases if c["klass"][0] == rot and c["klass"][4] == d]
                assert {(c["move"][2], c["move"][4]) for c in mine} == {(1, 0), (2, 0), (2, 1), (3, 0), (3, 1)}, (n, rot, d)
                bt = apply_block(n)
                assert {bt - 1, bt, bt + 1} <= {c["klass"][1] for c in mine}, (n, rot, d)


def run_apply_case(eng, case, c):
    eng.set_costs(c)
    eng.tour_load(0, case["tour0"])
    if case["flip"]:
        eng.tour_apply_move(0, *case["flip"])
    path, cost, _ = eng.tour_store(0)
    assert np.array_equal(path, case["start"][0]) and cost == case["start"][1], case["flip"]
    assert eng.tour_or_opt(0, max_moves=1) == (1, 0), case["move"]
    path, cost, delta = eng.tour_store(0)
    assert np.array_equal(path, case["or1"][0]) and (cost, delta) == (case["or1"][1], case["move"][0]), (case["move"], case["klass"])
    assert eng.tour_two_opt(0, max_sweeps=1) == (1, 0)              # reads the edge costs by position
    path, cost, _ = eng.tour_store(0)
    assert np.array_equal(path, case["two"][0]) and cost == case["two"][1], (case["move"], case["klass"])
    assert eng.tour_or_opt(0, max_moves=1) == (case["or2"][2], 0)   # reads the successors and the edge costs by node
    path, cost, _ = eng.tour_store(0)
    assert np.array_equal(path, case["or2"][0]) and cost == case["or2"][1], (case["move"], case["klass"])


def apply_engine(elem):
    import travellingsalesmanoptimization_amd as T
    eng = T.Engine(0)
    eng.set_option(T.OPT_ELEM, elem)
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 9, 12])
@pytest.mark.parametrize("elem", [F64, I32, U16])
def test_gpu_apply_exhaustive(elem, n):
    eng = apply_engine(elem)
    dirs = set()
    for tour0 in apply_tours(n):
        for case in exhaustive_cases(n, tour0):
            run_apply_case(eng, case, case["c"])
            dirs.add(case["klass"][4])
    assert eng.info()["elem"] == elem and dirs == {1, -1}
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [150, 1100])
@pytest.mark.parametrize("elem", [F64, I32, U16])
def test_gpu_apply_chunk_boundaries(elem, n):
    eng = apply_engine(elem)
    cases = chunk_case_list(n)
    for case in cases:
        run_apply_case(eng, case, planted_move_matrix(case["start"][0], *case["planted"]))
    assert eng.info()["elem"] == elem and classes_of(cases) == ALL_CLASSES
    eng.close()
