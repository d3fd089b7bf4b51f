"""Extra Mileage (h_ExtraMileage, src/algorithms/heuristics.c:156-210; h_extramileage_util :290-367).

CPU: an incremental numpy model of the insertion loop (per unvisited node the best (delta, edge) over the current
edges; only the nodes whose best edge was the one split rescan) against the compiled reference and the golden file.
GPU: tspgpu_farthest_pair / tspgpu_extra_mileage (both forms, every cell type, matrix-free) against the golden file
and the model, and the host binary's -alg EXTRA_MILEAGE."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import oracle as O  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_extra_mileage.json")
TSP_BIN = os.path.join(ROOT, "travellingsalesmanoptimization_amd", "host", "tsp")


# ---------------------------------------------------------------------------------------------------------------- model
def farthest_pair(c):
    """heuristics.c:165-177: the first pair i < j (row-major) whose cost is strictly the largest; all 0 -> (0, 1)."""
    n = len(c)
    m = np.where(np.triu(np.ones((n, n), dtype=bool), 1), c, -1.0)
    lin = int(np.argmax(m))                # first maximum in row-major order
    a, b = divmod(lin, n)
    if m[a, b] <= 0.0:
        return 0, 1
    return a, b


def em_model(c, a, b):
    """h_extramileage_util from (a, b), incremental -> (succ, cost, stale rescans)."""
    c = np.asarray(c)
    n = len(c)
    ci = c.astype(np.int64)
    eu = np.zeros(n, np.int64); ev = np.zeros(n, np.int64); ec = np.zeros(n, np.int64)
    eu[0], ev[0], ec[0] = a, b, ci[a, b]
    eu[1], ev[1], ec[1] = b, a, ci[b, a]
    k = 2
    succ = np.full(n, -1, np.int32)
    succ[a], succ[b] = b, a
    cost = 2.0 * float(c[a, b])
    unv = np.ones(n, dtype=bool)
    unv[[a, b]] = False
    bd = np.zeros(n, np.int64); bj = np.zeros(n, np.int64)
    idx = np.nonzero(unv)[0]
    d0 = ci[a, idx] + ci[idx, b] - ci[a, b]
    d1 = ci[b, idx] + ci[idx, a] - ci[b, a]
    one = d1 < d0
    bd[idx] = np.where(one, d1, d0); bj[idx] = np.where(one, 1, 0)
    stale = 0
    for _ in range(n - 2):
        cand = np.nonzero(unv)[0]
        kb = bd[cand]
        x = int(cand[int(np.argmax(kb == kb.min()))])          # min (bd, i)
        d = int(bd[x]); e = int(bj[x]); u, v = int(eu[e]), int(ev[e])
        ev[e], ec[e] = x, ci[u, x]
        eu[k], ev[k], ec[k] = x, v, ci[x, v]
        m = k; k += 1
        succ[u], succ[x] = x, v
        cost += d
        unv[x] = False
        rest = np.nonzero(unv)[0]
        if not len(rest):
            break
        st = rest[bj[rest] == e]
        ok = rest[bj[rest] != e]
        b0, j0 = bd[ok], bj[ok]
        de = ci[u, ok] + ci[ok, x] - ci[u, x]
        t = (de < b0) | ((de == b0) & (e < j0))
        b0 = np.where(t, de, b0); j0 = np.where(t, e, j0)
        dm = ci[x, ok] + ci[ok, v] - ci[x, v]
        t = dm < b0
        bd[ok] = np.where(t, dm, b0); bj[ok] = np.where(t, m, j0)
        if len(st):
            stale += len(st)
            D = ci[eu[:k][None, :], st[:, None]] + ci[st[:, None], ev[:k][None, :]] - ec[:k][None, :]
            j = np.argmin(D, axis=1)                         # first minimum: the lowest edge index
            bd[st] = D[np.arange(len(st)), j]; bj[st] = j
    return succ, cost, stale


# --------------------------------------------------------------------------------------------------------------- inputs
def lattice(side=24):
    g = np.arange(side, dtype=np.float64) * 10.0
    return np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)


def tripled(n=300, seed=5):
    return np.repeat(O.random_points(n, seed), 3, axis=0)


def collinear(n=200):
    return np.stack([np.arange(n, dtype=np.float64) * 7.0, np.zeros(n)], -1)


TIE_SETS = {"lattice24": lattice, "tripled300": tripled, "collinear200": collinear}


def instance_xy(name):
    return O.read_tsplib(os.path.join(DATA, name + ".tsp"))[0]


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def have_ref():
    return os.path.exists(O.REF_SO)


def ref_em(R, xy, a, b):
    """the reference's own h_extramileage_util from (a, b) on xy (EUC_2D) -> (succ, cost)"""
    import ctypes as C

    class Sol(C.Structure):
        _fields_ = [("cost", C.c_double), ("path", C.POINTER(C.c_int)), ("ncomp", C.c_int), ("comp", C.POINTER(C.c_int))]

    R.set_points(xy)
    c = R.costs()
    n = len(xy)
    path = np.zeros(n, dtype=np.int32)
    path[a], path[b] = b, a
    s = Sol(2.0 * c[a, b], path.ctypes.data_as(C.POINTER(C.c_int)), 0, None)
    fn = R.L.h_extramileage_util
    fn.argtypes = [C.POINTER(Sol), C.c_int, C.c_int]
    fn.restype = C.c_int
    assert fn(C.byref(s), a, b) == 0
    return path, s.cost


# ------------------------------------------------------------------------------------------------------------ CPU tests
def test_farthest_pair_tie_rule():
    c = np.zeros((5, 5))
    assert farthest_pair(c) == (0, 1)                               # all points identical
    c = np.array([[0, 3, 5, 5], [3, 0, 5, 1], [5, 5, 0, 2], [5, 1, 2, 0]], dtype=np.float64)
    assert farthest_pair(c) == (0, 2)                               # first of the four 5s in row-major order
    xy = np.array([[0, 0], [10, 0], [0, 10], [10, 10]], dtype=np.float64)
    assert farthest_pair(O.cost_matrix(xy)) == (0, 3)               # (0, 3) and (1, 2) tie: the first


def test_model_small_by_hand():
    # square + centre: start (0, 2), the centre is never first (its delta exceeds the corners')
    xy = np.array([[0, 0], [10, 0], [10, 10], [0, 10], [5, 5]], dtype=np.float64)
    c = O.cost_matrix(xy)
    succ, cost, _ = em_model(c, *farthest_pair(c))
    assert O.valid_tour(succ) and cost == O.tour_cost(c, succ)


@pytest.mark.skipif(not have_ref(), reason="oracle/_ref (the compiled reference) is not built")
@pytest.mark.parametrize("which", ["rand60", "rand257", "rand500", "lattice24", "tripled300", "collinear200"])
def test_model_equals_reference(which):
    R = O.Reference()
    if which.startswith("rand"):
        n = int(which[4:])
        xy = O.random_points(n, 1000 + n)
    else:
        xy = TIE_SETS[which]()
    c = O.cost_matrix(xy)
    a, b = farthest_pair(c)
    rsucc, rcost = ref_em(R, xy, a, b)
    msucc, mcost, _ = em_model(c, a, b)
    assert mcost == rcost and np.array_equal(msucc, rsucc)
    # also from a pair that is not the farthest (the EM_RANDOM case)
    rsucc, rcost = ref_em(R, xy, 3, len(xy) - 2)
    msucc, mcost, _ = em_model(c, 3, len(xy) - 2)
    assert mcost == rcost and np.array_equal(msucc, rsucc)


def test_golden_reproduces_published_column():
    G = golden()
    pub = G["published"]
    assert len(pub) == 14
    for name, rec in pub.items():
        assert rec["cost"] == rec["published"], name


@pytest.mark.parametrize("name", sorted(json.load(open(GOLDEN))["published"]) if os.path.exists(GOLDEN) else [])
def test_model_equals_golden(name):
    rec = golden()["published"][name]
    c = O.cost_matrix(instance_xy(name))
    a, b = farthest_pair(c)
    assert (a, b) == (rec["a"], rec["b"])
    succ, cost, _ = em_model(c, a, b)
    assert cost == rec["cost"] and O.fnv1a(succ) == int(rec["fnv"], 16)


# ------------------------------------------------------------------------------------------------------------ GPU tests
def engine_for(xy, kind=O.EUC_2D, elem=0, matrix_free=0, form=0):
    import travellingsalesmanoptimization_amd as T
    eng = T.Engine(0)
    eng.set_option(T.OPT_ELEM, elem)
    eng.set_option(T.OPT_MATRIX_FREE, matrix_free)
    eng.set_option(T.OPT_EM_FORM, form)
    eng.set_points(xy, kind)
    eng.build_costs()
    return eng


def check_tour(succ, cost, c=None):
    assert O.valid_tour(succ)
    if c is not None:
        assert cost == O.tour_cost(c, succ)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(json.load(open(GOLDEN))["published"]) if os.path.exists(GOLDEN) else [])
def test_gpu_published(name):
    rec = golden()["published"][name]
    eng = engine_for(instance_xy(name))
    a, b, _ = eng.farthest_pair()
    assert (a, b) == (rec["a"], rec["b"])
    succ, cost, rc = eng.extra_mileage()
    assert rc == 0 and cost == rec["cost"] == rec["published"] and O.fnv1a(succ) == int(rec["fnv"], 16)
    assert eng.info()["em_form"] in (1, 2)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", [1, 2])
def test_gpu_pr1002_matrix_free_and_forms(form):
    rec = golden()["published"]["pr1002"]
    eng = engine_for(instance_xy("pr1002"), matrix_free=1, form=form)
    assert eng.info()["matrix_free"] == 1
    succ, cost, rc = eng.extra_mileage()
    assert rc == 0 and cost == 302240.0 and O.fnv1a(succ) == int(rec["fnv"], 16)
    assert eng.info()["em_form"] == form
    eng.close()


SIZES = [4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 5000]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_gpu_sizes_equal_model(n):
    xy = O.random_points(n, 77 + n)
    c = O.cost_matrix(xy)
    a, b = farthest_pair(c)
    msucc, mcost, _ = em_model(c, a, b)
    for form in (1, 2):
        eng = engine_for(xy, form=form)
        assert eng.farthest_pair()[:2] == (a, b)
        succ, cost, rc = eng.extra_mileage()
        assert rc == 0 and cost == mcost and np.array_equal(succ, msucc), (n, form)
        assert eng.info()["em_form"] == form and eng.info()["em_steps"] == n - 2
        eng.close()
    check_tour(msucc, mcost, c)


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(TIE_SETS))
@pytest.mark.parametrize("elem", [1, 2, 3])
def test_gpu_tie_sets_every_cell_type(which, elem):
    xy = TIE_SETS[which]()
    c = O.cost_matrix(xy)
    a, b = farthest_pair(c)
    msucc, mcost, _ = em_model(c, a, b)
    eng = engine_for(xy, elem=elem)
    assert eng.info()["elem"] == elem
    succ, cost, rc = eng.extra_mileage()
    assert rc == 0 and cost == mcost and np.array_equal(succ, msucc)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [O.ATT, O.CEIL_2D])
@pytest.mark.parametrize("matrix_free", [2, 1])
def test_gpu_att_ceil(kind, matrix_free):
    xy = O.random_points(700, 31 + kind)
    c = O.cost_matrix(xy, kind)
    a, b = farthest_pair(c)
    msucc, mcost, _ = em_model(c, a, b)
    eng = engine_for(xy, kind=kind, matrix_free=matrix_free)
    assert eng.farthest_pair()[:2] == (a, b)
    succ, cost, rc = eng.extra_mileage()
    assert rc == 0 and cost == mcost and np.array_equal(succ, msucc)
    eng.close()


@pytest.mark.gpu
def test_gpu_caller_matrix_and_pair():
    import travellingsalesmanoptimization_amd as T
    xy = O.random_points(300, 9)
    c = O.cost_matrix(xy)
    eng = T.Engine(0)
    eng.set_costs(c)
    msucc, mcost, _ = em_model(c, 17, 4)
    succ, cost, rc = eng.extra_mileage(17, 4)
    assert rc == 0 and cost == mcost and np.array_equal(succ, msucc)
    with pytest.raises(T.TspGpuError) as ei:
        eng.extra_mileage(5, 5)
    assert ei.value.code == T._lib.INVALID_ARGUMENT
    bad = c.copy(); bad[3, 4] = 0.5
    eng.set_costs(bad)
    with pytest.raises(T.TspGpuError) as ei:
        eng.extra_mileage(0, 1)
    assert ei.value.code == T._lib.FAILED_PRECONDITION
    eng.close()


@pytest.mark.gpu
def test_gpu_fnl4461_golden():
    rec = golden()["extra"]["fnl4461"]
    for form in (1, 2):
        eng = engine_for(instance_xy("fnl4461"), form=form)
        succ, cost, rc = eng.extra_mileage()
        assert rc == 0 and cost == rec["cost"] == 212547.0 and O.fnv1a(succ) == int(rec["fnv"], 16)
        check_tour(succ, cost)
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", [1, 2])
def test_gpu_deadline_leaves_no_tour(form):
    """the in-kernel deadline (wall clock, checked before every insertion) in both forms: code 4, no tour, and the
    construction stopped part way"""
    import travellingsalesmanoptimization_amd as T
    eng = engine_for(instance_xy("fnl4461"), form=form)
    succ, cost, rc = eng.extra_mileage(time_left_s=2e-3)
    info = eng.info()
    assert rc == T._lib.DEADLINE_EXCEEDED and succ is None and cost is None
    assert info["em_form"] == form and 0 < info["em_steps"] < 4461 - 2, info
    eng.close()


def large_xy(name):
    xy, ewt = O.read_tsplib(os.path.join(DATA, name + ".tsp"))
    return xy, {"EUC_2D": O.EUC_2D, "ATT": O.ATT, "CEIL_2D": O.CEIL_2D}[ewt]


@pytest.mark.gpu
def test_gpu_d18512_matrix_golden():
    """n = 18 512, matrix mode, the default (per-step) form: the C restatement's golden (tools/em_model.c)"""
    rec = golden()["extra"]["d18512"]
    xy, kind = large_xy("d18512")
    eng = engine_for(xy, kind=kind, matrix_free=2)
    assert eng.info()["matrix_free"] == 0
    assert eng.farthest_pair()[:2] == (rec["a"], rec["b"])
    succ, cost, rc = eng.extra_mileage()
    assert rc == 0 and cost == rec["cost"] and "%016x" % O.fnv1a(succ) == rec["fnv"]
    assert eng.info()["em_stale"] == rec["stale"]
    assert O.valid_tour(succ) and cost == O.tour_cost_xy(xy, kind, succ)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", [2, 1])
def test_gpu_pla85900_matrix_free_golden(form):
    """n = 85 900 (node and edge labels past 2^16 in the 17-bit key fields), CEIL_2D, matrix-free, both forms"""
    rec = golden()["extra"]["pla85900"]
    xy, kind = large_xy("pla85900")
    assert kind == O.CEIL_2D
    eng = engine_for(xy, kind=kind, form=form)
    assert eng.info()["matrix_free"] == 1
    assert eng.farthest_pair()[:2] == (rec["a"], rec["b"])
    succ, cost, rc = eng.extra_mileage()
    assert rc == 0 and cost == rec["cost"] and "%016x" % O.fnv1a(succ) == rec["fnv"]
    assert eng.info()["em_form"] == form and eng.info()["em_stale"] == rec["stale"]
    assert O.valid_tour(succ) and cost == O.tour_cost_xy(xy, kind, succ)
    eng.close()


@pytest.mark.skipif(not have_ref(), reason="oracle/_ref (the compiled reference) is not built")
def test_c_model_equals_reference(tmp_path):
    """tools/em_model.c (the restatement behind the d18512 / pla85900 goldens) against the reference's own loop"""
    exe = str(tmp_path / "em_model")
    subprocess.run(["gcc", "-O3", "-fopenmp", "-ffp-contract=off", "-fno-math-errno", "-o", exe,
                    os.path.join(ROOT, "tools", "em_model.c"), "-lm"], check=True)
    R = O.Reference()
    for xy in [O.random_points(300, 4), lattice(), tripled(), collinear()]:
        c = O.cost_matrix(xy)
        a, b = farthest_pair(c)
        rsucc, rcost = ref_em(R, xy, a, b)
        path = str(tmp_path / "xy.bin")
        np.ascontiguousarray(xy, np.float64).tofile(path)
        ga, gb, gcost, gfnv, _ = subprocess.run([exe, path, str(len(xy)), "0"], check=True, capture_output=True,
                                                text=True).stdout.split()
        assert (int(ga), int(gb), float(gcost), gfnv) == (a, b, rcost, "%016x" % O.fnv1a(rsucc))


# ------------------------------------------------------------------------------------------------------- host binary
def run_tsp(*args, timeout=300):
    env = dict(os.environ)
    return subprocess.run([TSP_BIN, *args], capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)


@pytest.mark.gpu
def test_host_binary_pr1002():
    r = run_tsp("-f", os.path.join(DATA, "pr1002.tsp"), "-alg", "EXTRA_MILEAGE", "-q")
    assert r.returncode == 0 and r.stdout.strip() == "Cost: 302240.00", r.stdout + r.stderr


def libc_draws(seed, n, skip=0):
    """EM_RANDOM's (A, B) (heuristics.c:179-181) from glibc's stream after srand(seed) and `skip` draws:
    A = rand() % (n+1), B = rand() % (n-A+1) + A.  An instance read from a file leaves the stream unseeded (= seed 1);
    -n N -seed s seeds it and draws 2N coordinates first (tsp.c:468-481)."""
    import ctypes as C
    libc = C.CDLL(None)
    libc.srand(C.c_uint(seed))
    for _ in range(skip):
        libc.rand()
    a = libc.rand() % (n + 1)
    return a, libc.rand() % (n - a + 1) + a


@pytest.mark.gpu
def test_host_binary_random_pair():
    xy = instance_xy("kroA100")
    a, b = libc_draws(1, len(xy))
    assert a < b < len(xy)                                   # a valid draw (32, 78)
    _, mcost, _ = em_model(O.cost_matrix(xy), a, b)
    r = run_tsp("-f", os.path.join(DATA, "kroA100.tsp"), "-alg", "EXTRA_MILEAGE", "-em", "RANDOM", "-q")
    assert r.returncode == 0 and r.stdout.strip() == "Cost: %.2f" % mcost, r.stdout + r.stderr


def test_host_binary_degenerate_draw():
    """a draw with A == B or an index == n: INVALID_ARGUMENT (logged), exit status 1, no tour -- before any device call"""
    n = 60
    bad = next(s for s in range(1, 5000) if (lambda p: p[0] == p[1] or p[1] >= n)(libc_draws(s, n, 2 * n)))
    r = run_tsp("-n", str(n), "-seed", str(bad), "-alg", "EXTRA_MILEAGE", "-em", "RANDOM")
    assert r.returncode != 0 and "cost:" not in r.stdout.lower(), r.stdout
    assert "not two distinct nodes" in (r.stdout + r.stderr)


@pytest.mark.gpu
def test_host_binary_deadline_keeps_incumbent():
    # d18512: the matrix is built before the clock starts (main.c's order), the construction takes far longer than
    # 0.1 s, so the limit passes INSIDE the device loop, which says how far it got
    r = run_tsp("-f", os.path.join(DATA, "d18512.tsp"), "-alg", "EXTRA_MILEAGE", "-t", "0.1", "-v")
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "time limit exceeded after" in out, out
    # DEADLINE_EXCEEDED is a success for the reference (errors.c:31-37): the untouched incumbent is printed
    cost = [ln for ln in r.stdout.splitlines() if ln.strip().lower().startswith("cost:")]
    assert cost and float(cost[-1].split()[-1]) > 1e300, out
