"""Or-opt and the 2-opt + Or-opt descent in matrix-free mode (TSPGPU_OPT_OR_MATRIX_FREE = 22; include/tspgpu.h "Or-opt",
DESIGN 4.12): k_oropt_sweep_otf / k_oropt_apply_otf against the model of tests/test_or_opt.py, whose costs are the
oracle's matrix of the same points and kind.  Every comparison is exact (delta, (s, L, q, rev), path, cost), every GPU
case runs under both forms of the sweep (hook 90 = 2: every candidate evaluated; 1: the exact early-out) and asserts
that the context is matrix-free and that the form asked for is the one that ran (tspgpu_info 34).

Past the sizes a matrix can be held at (n = 66 000, and one sweep at the size limit n = 131 072) the expected moves are
read from tests/golden/golden_or_opt_matrix_free.json, written by tools/make_golden_or_opt_matrix_free.py with the
threaded C restatement over coordinates tests/or_opt_model_xy.c, which a CPU test here pins to the plain model at
n = 200.  The n = 131 072 model sweep takes well under the ten minutes the size was conditional on, so it is kept.

Device wall time of this module: not measured -- no device run of it is recorded yet."""
import ctypes as C
import functools
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import oracle as O  # noqa: E402
import test_or_opt as M  # noqa: E402
from test_or_opt import apply_move, best_move, descent_model, instance_xy, walk  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_or_opt_matrix_free.json")
EUC_2D, ATT, CEIL_2D = 0, 1, 2
EPS = M.EPS
FORMS = [2, 1]                      # hook 90: 2 = the full form, 1 = the early-out form
OR_OTF = {2: 1, 1: 2}               # ... -> what tspgpu_info 34 reports
RUN = 16                            # tour positions per workgroup of k_oropt_sweep_otf (tspgpu_info 35)
ENTRY_POINTS = ["tspgpu_or_opt_once", "tspgpu_or_opt", "tspgpu_local_search", "tspgpu_tour_or_opt", "tspgpu_tour_local_search",
                "tspgpu_time_or_sweep"]


# ---------------------------------------------------------------------------------------------------------------- model
@functools.lru_cache(maxsize=None)
def xy_model():
    """tests/or_opt_model_xy.c compiled into a scratch directory (kept for the process)"""
    d = tempfile.mkdtemp(prefix="or_opt_model_xy_")
    so = os.path.join(d, "or_opt_model_xy.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", "-o", so,
                    os.path.join(ROOT, "tests", "or_opt_model_xy.c"), "-lm"], check=True)
    lib = C.CDLL(so)
    lib.orx_best_move.restype = C.c_int
    lib.orx_best_move.argtypes = [np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS"), C.c_int, C.c_int,
                                  np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS"), C.c_int, C.POINTER(C.c_double),
                                  np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")]
    return lib


def best_move_xy(xy, kind, path, threads=16):
    """the restatement over coordinates -> (delta, s, L, q, rev)"""
    d = C.c_double()
    mv = np.empty(4, np.int32)
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1)
    assert xy_model().orx_best_move(xy, len(path), kind, np.ascontiguousarray(path, np.int32), threads, C.byref(d), mv) == 0
    return (d.value, *[int(v) for v in mv])


def big_points(n):
    """n uniform-random integer points in [0, 10^6)^2"""
    return np.random.default_rng(n).integers(0, 1000000, (n, 2)).astype(np.float64)


def boustrophedon(xy, columns=256):
    """successor array of the tour that visits the points column by column over a `columns`-column grid, up the even
    columns and down the odd ones (ties by index)"""
    n = len(xy)
    x, y = xy[:, 0], xy[:, 1]
    col = np.minimum((x - x.min()) * columns // (x.max() - x.min() + 1), columns - 1).astype(np.int64)
    key = np.where(col % 2 == 0, y, -y)
    order = np.lexsort((np.arange(n), key, col)).astype(np.int32)
    path = np.empty(n, np.int32)
    path[order] = np.roll(order, -1)
    return path


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def costs_of(name, kind=EUC_2D):
    return O.cost_matrix(instance_xy(name), kind)


def ceil_points(shift):
    return np.random.default_rng(600).integers(0, 5000, (600, 2)).astype(np.float64) + shift


WALKS = {   # name -> (points, kind, tspgpu_info 26 or None)
    "n64": (lambda: instance_xy("n64"), EUC_2D, None),
    "n1000": (lambda: instance_xy("n1000"), EUC_2D, None),
    "pr1002": (lambda: instance_xy("pr1002"), EUC_2D, None),
    "att48": (lambda: instance_xy("att48"), ATT, None),
    "ceil600_int": (lambda: ceil_points(0.0), CEIL_2D, 1),
    "ceil600_quarter": (lambda: ceil_points(0.25), CEIL_2D, 0),
}


@functools.lru_cache(maxsize=None)
def walk_model(name, from_2opt, limit=200):
    """the model's first `limit` Or-opt moves from NN(0) or its 2-opt optimum -> (start, cost, trace, paths)"""
    get, kind, _ = WALKS[name]
    c = O.cost_matrix(get(), kind)
    path, cost = O.nn_tour(c, 0)
    if from_2opt:
        _, cost = O.two_opt(c, path)
    return (path.copy(), cost) + walk(c, path.copy(), cost, limit)


# ------------------------------------------------------------------------------------------------------------ CPU tests
def test_option_and_info_constants():
    import travellingsalesmanoptimization_amd as T
    assert T._lib.OPT_OR_MATRIX_FREE == 22 and (T._lib.INFO_OR_OTF, T._lib.INFO_OR_OTF_R) == (34, 35)

    class Lib:
        @staticmethod
        def tspgpu_info(ctx, i):
            return i
    eng = object.__new__(T.Engine)
    eng.L, eng.ctx = Lib, None
    info = eng.info()
    assert (info["or_otf"], info["or_otf_R"]) == (34, 35) and info["or_nch"] == 33 and info["matrix_free"] == 10


def test_header_names_the_option():
    text = open(os.path.join(ROOT, "include", "tspgpu.h")).read()
    assert "TSPGPU_OPT_OR_MATRIX_FREE = 22" in text
    section = text[text.index("---- Or-opt and the 2-opt + Or-opt descent"):text.index("/* one Or-opt sweep on a host tour")]
    assert "TSPGPU_OPT_OR_MATRIX_FREE = 1" in section and "tspgpu_tours_local_search" in section
    for name in ENTRY_POINTS:
        assert name in section, name


def test_symbols_still_export():
    from travellingsalesmanoptimization_amd import _lib
    L = _lib.load()
    for s in ENTRY_POINTS + ["tspgpu_set_option", "tspgpu_info", "tspgpu_tours_local_search", "tspgpu_multistart_local_search"]:
        assert s in _lib.SIGNATURES and hasattr(L, s), s
    host = C.CDLL(os.path.join(M.PKG, "host", "libtsphost.so"))
    assert hasattr(host, "tsp_or_opt_polish")


def test_xy_model_equals_the_plain_model():
    """tests/or_opt_model_xy.c against best_move over the oracle's matrix: n = 200 in every kind, random and NN tours, one
    thread, stripes that do not divide n, more stripes than make sense; and the smallest sizes"""
    rng = np.random.default_rng(200)
    for n in (200, 8, 9, 17):
        for kind in (EUC_2D, ATT, CEIL_2D):
            xy = rng.integers(0, 3000, (n, 2)).astype(np.float64) + (0.5 if kind == CEIL_2D else 0.0)
            c = O.cost_matrix(xy, kind)
            tours = [M.random_tour(n, rng), O.nn_tour(c, 0)[0]]
            opt = tours[1].copy()
            O.two_opt(c, opt)
            for path in tours + [opt]:
                want = best_move(c, path)
                for threads in (1, 3, 16, 64):
                    assert best_move_xy(xy, kind, path, threads) == want, (n, kind, threads)
    side = np.arange(8, dtype=np.float64) * 10.0                # ties in large groups
    xy = np.stack(np.meshgrid(side, side, indexing="ij"), -1).reshape(-1, 2)
    c = O.cost_matrix(xy)
    for path in (O.nn_tour(c, 0)[0], M.random_tour(64, rng)):
        assert best_move_xy(xy, EUC_2D, path, 5) == best_move(c, path)


def test_golden_inputs_are_the_ones_the_test_rebuilds():
    """the points and start tours the golden was made from are what big_points / boustrophedon give here"""
    g = golden()
    for key in ("n66000", "n131072"):
        n = g[key]["n"]
        xy = big_points(n)
        path = boustrophedon(xy)
        assert O.valid_tour(path)
        assert (sha(xy), sha(path)) == (g[key]["points_sha"], g[key]["start_sha"]), key
    assert len(g["n66000"]["moves"]) == 3 and len(g["n66000"]["costs"]) == 4 and len(g["n131072"]["moves"]) == 1
    assert all(m[0] < EPS for m in g["n66000"]["moves"] + g["n131072"]["moves"])
    assert max(m[1] for m in g["n131072"]["moves"]) < 131072


# ------------------------------------------------------------------------------------------------------------ GPU tests
def mf_engine(xy, kind=EUC_2D, form=2, option=1, auto=False):
    """a matrix-free context with TSPGPU_OPT_OR_MATRIX_FREE = option and the sweep form of hook 90"""
    import travellingsalesmanoptimization_amd as T
    eng = T.Engine(0)
    eng.set_option(T.OPT_MATRIX_FREE, 0 if auto else 1)
    if option is not None:
        eng.set_option(T._lib.OPT_OR_MATRIX_FREE, option)
    eng.set_option(90, form)
    eng.set_points(xy, kind)
    eng.build_costs()
    assert eng.info()["matrix_free"] == 1
    return eng


def ran_as(eng, form):
    info = eng.info()
    assert info["matrix_free"] == 1 and (info["or_otf"], info["or_otf_R"]) == (OR_OTF[form], RUN), info
    assert (info["or_batch_r"], info["or_single_r"], info["or_block"], info["or_nch"]) == (0, 0, 0, 0), info


def refused_everywhere(eng, n, code):
    import travellingsalesmanoptimization_amd as T
    path = np.roll(np.arange(n, dtype=np.int32), -1)
    eng.tour_load(0, path)
    for call in (lambda: eng.or_opt_once(path, 0.0), lambda: eng.or_opt(path, 0.0), lambda: eng.local_search(path),
                 lambda: eng.tour_or_opt(0), lambda: eng.tour_local_search(0), lambda: eng.time_or_sweep(0, 1)):
        with pytest.raises(T.TspGpuError) as ei:
            call()
        assert ei.value.code == code, ei.value
        assert "matrix-free" in str(ei.value), ei.value
    assert np.array_equal(path, np.roll(np.arange(n), -1))
    got, _, _ = eng.tour_store(0)
    assert np.array_equal(got, path)
    assert eng.info()["or_otf"] == 0 and eng.info()["or_otf_R"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_gpu_switch(form):
    import travellingsalesmanoptimization_amd as T
    xy, c = instance_xy("n64"), costs_of("n64")
    eng = mf_engine(xy, form=form, option=None)             # the default
    refused_everywhere(eng, 64, T._lib.UNIMPLEMENTED)
    eng.set_option(T._lib.OPT_OR_MATRIX_FREE, 0)
    refused_everywhere(eng, 64, T._lib.UNIMPLEMENTED)
    for bad in (2, -1):
        with pytest.raises(T.TspGpuError) as ei:
            eng.set_option(T._lib.OPT_OR_MATRIX_FREE, bad)
        assert ei.value.code == T._lib.INVALID_ARGUMENT
    refused_everywhere(eng, 64, T._lib.UNIMPLEMENTED)       # a refused value changes nothing
    eng.set_option(T._lib.OPT_OR_MATRIX_FREE, 1)
    path, cost = O.nn_tour(c, 0)
    want = best_move(c, path)
    assert want[0] < EPS
    d, cost2, mv = eng.or_opt_once(path, cost)
    assert (d, *mv) == want and cost2 == cost + d == O.tour_cost(c, path)
    ran_as(eng, form)
    assert eng.time_or_sweep(0, 2) > 0.0
    # the batch stays refused, and the context goes on working
    eng.tour_load(0, path)
    eng.tour_load(1, path)
    with pytest.raises(T.TspGpuError) as ei:
        eng.tours_local_search(0, 2)
    assert ei.value.code == T._lib.UNIMPLEMENTED
    with pytest.raises(T.TspGpuError) as ei:
        eng.multistart_local_search(starts=[0, 1])
    assert ei.value.code == T._lib.UNIMPLEMENTED
    M.still_works(eng, c)
    eng.set_points(O.random_points(7, 3))                   # n = 7 with the option on: 3
    eng.build_costs()
    with pytest.raises(T.TspGpuError) as ei:
        eng.or_opt_once(np.roll(np.arange(7, dtype=np.int32), -1), 0.0)
    assert ei.value.code == T._lib.INVALID_ARGUMENT
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(WALKS))
def test_gpu_move_by_move(name, form):
    get, kind, ceil_int = WALKS[name]
    eng = mf_engine(get(), kind, form)
    if ceil_int is not None:
        assert eng.info()["ceil_int"] == ceil_int
    for from_2opt in (False, True):
        start, cost, trace, paths = walk_model(name, from_2opt)
        assert len(trace) <= 200 and (from_2opt or len(trace) > 0)
        M.check_walk(eng, start, cost, trace, paths)
    ran_as(eng, form)
    eng.close()


SIZES = [8, 9, 12, RUN - 1, RUN, RUN + 1, 2 * RUN + 1, 255, 256, 257, 1023, 1025, 2049]


@functools.lru_cache(maxsize=None)
def size_case(n):
    """random points, two random tours and the model's first six moves from each"""
    rng = np.random.default_rng(7000 + n)
    xy = O.random_points(n, 7000 + n)
    c = O.cost_matrix(xy)
    out = []
    for _ in range(2):
        path = M.random_tour(n, rng)
        cost = O.tour_cost(c, path)
        out.append((path, cost) + walk(c, path.copy(), cost, 6))
    return xy, out


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", SIZES)
def test_gpu_smallest_sizes_and_run_boundaries(n, form):
    xy, cases = size_case(n)
    eng = mf_engine(xy, form=form)
    for path, cost, trace, paths in cases:
        assert len(trace) >= 1
        M.check_walk(eng, path, cost, trace, paths, limit=6)
    ran_as(eng, form)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [8, 9])
def test_gpu_every_rotation_and_direction(n, form):
    """one tour seen from every rotation (the node the slot's position 0 holds: labels 0 and ord[r] swapped) and in both
    directions, as loaded and after one 2-opt move on the slot (which may flip the slot's direction): segments that
    straddle cell n - 1 -> 0 in either direction"""
    rng = np.random.default_rng(90 + n)
    xy0 = O.random_points(n, 90 + n)
    base = M.random_tour(n, rng)
    ord0 = M.tour_order(base)
    eng = mf_engine(xy0, form=form)
    compared = moved = 0
    for r in range(n):
        relabel = np.arange(n)
        relabel[[0, ord0[r]]] = relabel[[ord0[r], 0]]          # old label -> new label (an involution)
        xy = xy0[relabel]
        fwd = np.empty(n, np.int32)
        fwd[relabel] = relabel[base]
        back = np.empty(n, np.int32)
        back[fwd] = np.arange(n, dtype=np.int32)
        c = O.cost_matrix(xy)
        eng.set_points(xy)
        eng.build_costs()
        assert eng.info()["matrix_free"] == 1
        for start in (fwd, back):
            for two_opt_first in (False, True):
                path, cost = start.copy(), O.tour_cost(c, start)
                eng.tour_load(0, path)
                if two_opt_first:
                    sweeps, rc = eng.tour_two_opt(0, max_sweeps=1)
                    d2, cost, _ = O.two_opt_once(c, path, cost)
                    assert (sweeps, rc) == (1, 0)
                    moved += d2 < EPS
                want = best_move(c, path)
                moves, rc = eng.tour_or_opt(0, max_moves=1)
                applied = want[0] < EPS
                if applied:
                    apply_move(path, *want[1:])
                    cost += want[0]
                gpath, gcost, gdelta = eng.tour_store(0)
                assert (moves, rc) == (int(applied), 0) and np.array_equal(gpath, path), (r, two_opt_first, want)
                assert (gcost, gdelta) == (cost, want[0] if applied else 0.0), (r, two_opt_first, want)
                compared += 1
    assert compared == 4 * n and moved > 0
    ran_as(eng, form)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_gpu_ties_lattice(form):
    side = np.arange(12, dtype=np.float64) * 10.0
    xy = np.stack(np.meshgrid(side, side, indexing="ij"), -1).reshape(-1, 2)
    c = O.cost_matrix(xy)
    eng = mf_engine(xy, form=form)
    rng = np.random.default_rng(12)
    for start in (O.nn_tour(c, 0)[0], M.random_tour(144, rng)):
        cost = O.tour_cost(c, start)
        trace, paths = walk(c, start.copy(), cost, 60)
        M.check_walk(eng, start, cost, trace, paths, limit=60)
    ran_as(eng, form)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_gpu_ties_collinear(form):
    """64 equidistant points on a line, the identity tour: nothing improves -> delta 0, move -1, no move applied"""
    n = 64
    xy = np.stack([np.arange(n, dtype=np.float64) * 10.0, np.zeros(n)], -1)
    c = O.cost_matrix(xy)
    path = np.roll(np.arange(n, dtype=np.int32), -1)
    cost = O.tour_cost(c, path)
    assert not best_move(c, path)[0] < EPS
    eng = mf_engine(xy, form=form)
    d, cost2, mv = eng.or_opt_once(path, cost)
    assert (d, cost2, mv) == (0.0, cost, (-1, -1, -1, -1)) and np.array_equal(path, np.roll(np.arange(n), -1))
    eng.tour_load(0, path)
    assert eng.tour_or_opt(0) == (0, 0)                   # the first sweep raises `stop`
    gpath, gcost, gdelta = eng.tour_store(0)
    assert np.array_equal(gpath, path) and (gcost, gdelta) == (cost, 0.0)
    ran_as(eng, form)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_gpu_slot_invariants_under_alternation(form):
    """tour_or_opt(max_moves=1) and tour_two_opt(max_sweeps=1) in turn: the matrix-free 2-opt sweep reads what the new apply
    wrote, and the other way round"""
    xy, c = instance_xy("n1000"), costs_of("n1000")
    eng = mf_engine(xy, form=form)
    path, cost = O.nn_tour(c, 0)
    eng.tour_load(0, path)
    for step in range(60):
        if step % 2 == 0:
            moves, rc = eng.tour_or_opt(0, max_moves=1)
            cost, m, trace = M.or_opt_phase(c, path, cost, max_moves=1)
            delta = trace[0][0] if m else 0.0
            assert (moves, rc) == (m, 0), step
        else:
            sweeps, rc = eng.tour_two_opt(0, max_sweeps=1)
            delta, cost, _ = O.two_opt_once(c, path, cost)
            assert (sweeps, rc) == (1, 0), step
        gpath, gcost, gdelta = eng.tour_store(0)
        assert np.array_equal(gpath, path) and (gcost, gdelta) == (cost, delta), step
    ran_as(eng, form)
    eng.close()


@functools.lru_cache(maxsize=None)
def pr1002_descent():
    c = costs_of("pr1002")
    start, _ = O.nn_tour(c, 0)
    path = start.copy()
    return start, path, descent_model(c, path)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_gpu_descent_equals_model_and_matrix_mode(form):
    c = costs_of("pr1002")
    start, mpath, want = pr1002_descent()
    assert want["or_moves"] > 0 and want["rounds"] >= 2
    eng = mf_engine(instance_xy("pr1002"), form=form)
    path = start.copy()
    got = eng.local_search(path)
    assert got.pop("rc") == 0 and got == want, (got, want)
    assert np.array_equal(path, mpath) and O.tour_cost(c, path) == got["cost"]
    eng.tour_load(1, start)                                 # the slot form
    slot = eng.tour_local_search(1)
    spath, scost, _ = eng.tour_store(1)
    assert slot.pop("rc") == 0 and slot == {k: want[k] for k in slot}
    assert np.array_equal(spath, mpath) and scost == want["cost"]
    ran_as(eng, form)
    eng.close()
    meng = M.engine_for("pr1002")                           # the same call on a matrix-mode context
    assert meng.info()["matrix_free"] == 0
    path2 = start.copy()
    got2 = meng.local_search(path2)
    assert got2.pop("rc") == 0 and got2 == got and np.array_equal(path2, path)
    meng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_gpu_past_every_matrix_mode_limit(form):
    """n = 66 000 in automatic mode: the first three Or-opt moves from the boustrophedon tour, and the cost after each"""
    g = golden()["n66000"]
    n = g["n"]
    xy = big_points(n)
    eng = mf_engine(xy, form=form, auto=True)
    path = boustrophedon(xy)
    want = path.copy()
    cost = g["costs"][0]
    assert O.tour_cost_xy(xy, EUC_2D, path) == cost
    for k, mv in enumerate(g["moves"]):
        d, cost2, got = eng.or_opt_once(path, cost)
        assert (d, *got) == tuple(mv), (k, d, got, mv)
        apply_move(want, *mv[1:])
        assert cost2 == g["costs"][k + 1] == cost + d and np.array_equal(path, want), k
        cost = cost2
    assert O.tour_cost_xy(xy, EUC_2D, path) == cost
    ran_as(eng, form)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_gpu_one_sweep_at_the_size_limit(form):
    """n = 131 072: the largest n, every bit of the key's 17-bit fields in use"""
    g = golden()["n131072"]
    n = g["n"]
    assert n == 131072
    xy = big_points(n)
    eng = mf_engine(xy, form=form, auto=True)
    path = boustrophedon(xy)
    want = path.copy()
    mv = g["moves"][0]
    d, cost2, got = eng.or_opt_once(path, g["costs"][0])
    assert (d, *got) == tuple(mv), (d, got, mv)
    apply_move(want, *mv[1:])
    assert cost2 == g["costs"][1] and np.array_equal(path, want)
    ran_as(eng, form)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_gpu_deadline_returns_a_tour(form):
    import travellingsalesmanoptimization_amd as T
    c = costs_of("pr1002")
    eng = mf_engine(instance_xy("pr1002"), form=form)
    path, _ = O.nn_tour(c, 0)
    got = eng.local_search(path, time_left_s=0.0)
    assert got["rc"] == T._lib.DEADLINE_EXCEEDED
    assert O.valid_tour(path) and O.tour_cost(c, path) == got["cost"]
    eng.close()


# ------------------------------------------------------------------------------------------------------- host binary
def run_tsp(*args, env_extra, timeout=300):
    env = dict(os.environ)
    for k in ("TSP_OR_OPT", "TSP_OR_OPT_MATRIX_FREE", "TSP_OR_OPT_EVERY_START", "TSP_MATRIX_FREE"):
        env.pop(k, None)
    env.update(env_extra)
    return subprocess.run([M.TSP_BIN, *args], capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)


@pytest.mark.gpu
def test_host_binary_switch():
    c = costs_of("pr1002")
    eng = M.engine_for("pr1002")
    res = eng.multistart_nn_2opt()
    eng.close()
    winner, wcost = res["path"], res["cost"]
    assert O.tour_cost(c, winner) == wcost == 266290.0
    want = descent_model(c, winner.copy())["cost"]
    assert want < wcost
    args = ("-f", os.path.join(M.DATA, "pr1002.tsp"), "-alg", "2OPT_GREEDY", "-q")
    r = run_tsp(*args, env_extra={"TSP_MATRIX_FREE": "1", "TSP_OR_OPT": "1", "TSP_OR_OPT_MATRIX_FREE": "1"})
    assert r.returncode == 0 and r.stdout.strip() == "Cost: %.2f" % want, r.stdout + r.stderr
    for off in ({}, {"TSP_OR_OPT_MATRIX_FREE": "0"}):
        r = run_tsp(*args, env_extra={"TSP_MATRIX_FREE": "1", "TSP_OR_OPT": "1", **off})
        assert r.returncode == 0 and r.stdout.strip() == "Cost: 266290.00", r.stdout + r.stderr
    r = run_tsp(*args, env_extra={"TSP_MATRIX_FREE": "1", "TSP_OR_OPT": "1", "TSP_OR_OPT_MATRIX_FREE": "2"})
    assert r.returncode != 0 and "TSP_OR_OPT_MATRIX_FREE" in r.stderr and "Cost:" not in r.stdout, r.stdout + r.stderr
