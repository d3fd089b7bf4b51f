"""The 2-opt + Or-opt descent over a batch of tours (include/tspgpu.h: tspgpu_tours_local_search,
tspgpu_multistart_local_search, tspgpu_multi_multistart_local_search; DESIGN 4.12 "Batches").

The yardstick is the model of tests/test_or_opt.py (descent_model: the oracle's 2-opt, the C restatement of the Or-opt sweep),
imported from there -- not the engine's single-tour path.  Every comparison is exact: the costs are integers or bit-exact
doubles.
CPU: exported symbols, loud failure without a device.
GPU: every slot against the model (tours that finish in different rounds), ranges that do not start at slot 0, chunking and
the start list, a size at which the batch plan differs from the single-tour plan, ties, preconditions, the deadline, two
contexts behind one multi-device handle, and the host binary's TSP_OR_OPT_EVERY_START switch."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import oracle as O  # noqa: E402
import test_or_opt as M  # noqa: E402

NEW_SYMBOLS = ["tspgpu_tours_local_search", "tspgpu_multistart_local_search", "tspgpu_multi_multistart_local_search"]
COUNTS = ("two_opt_sweeps", "or_moves", "rounds")


# ---------------------------------------------------------------------------------------------------------------- model
def model_from(c, start_path):
    """descent_model from a tour -> dict(path, cost, two_opt_sweeps, or_moves, rounds)"""
    path = np.array(start_path, np.int32)
    res = M.descent_model(c, path)
    res["path"] = path
    return res


@functools.lru_cache(maxsize=None)
def nn_models(name, nstarts):
    """the model's descent from NN(s), s = 0 .. nstarts - 1 (computed once per instance, never modified)"""
    c = M.instance_costs(name)
    return tuple(model_from(c, O.nn_tour(c, s)[0]) for s in range(nstarts))


@functools.lru_cache(maxsize=None)
def tie_case(which):
    """the matrices of test_or_opt.test_gpu_tie_order, eight tours (NN from four starts, four random tours) and their models"""
    c = M.lattice_matrix(20) if which == "lattice" else M.equal_matrix(400)
    rng = np.random.default_rng(23)
    starts = [O.nn_tour(c, s)[0] for s in (0, 7, 199, 399)] + [M.random_tour(len(c), rng) for _ in range(4)]
    return c, starts, [model_from(c, s) for s in starts]


def check_slots(eng, slot0, got, want):
    """slots slot0 .. hold exactly what the model leaves, and the per-slot counters are the model's"""
    assert got["rc"] == 0
    for i, w in enumerate(want):
        path, cost, _ = eng.tour_store(slot0 + i)
        assert np.array_equal(path, w["path"]) and cost == w["cost"], (i, cost, w["cost"])
        assert tuple(int(got[k][i]) for k in COUNTS) == tuple(w[k] for k in COUNTS), (i, [got[k][i] for k in COUNTS], w)


# ------------------------------------------------------------------------------------------------------------ CPU tests
def test_libraries_export_the_batch_entry_points():
    from travellingsalesmanoptimization_amd import _lib
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "tspgpu.h")).read()
    for s in NEW_SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(L, s) and s + "(" in header, s
    host = C.CDLL(os.path.join(M.PKG, "host", "libtsphost.so"))
    assert hasattr(host, "h_greedy_local_search")


def test_no_device_means_loud_failure():
    """a null context / handle: 14 (or 13) and an error text, the output arrays untouched, no CPU fallback"""
    from travellingsalesmanoptimization_amd import _lib
    L = _lib.load()
    null = C.c_void_p()
    sw, om = np.full(4, -7, np.int64), np.full(4, -7, np.int64)
    nr = np.full(4, -7, np.int32)
    best = np.full(8, -7, np.int32)
    costs = np.full(8, -7.0)
    cost, start, tsw, tom = C.c_double(-7.0), C.c_int(-7), C.c_long(-7), C.c_long(-7)
    rc = L.tspgpu_tours_local_search(null, 0, 4, -1.0, sw.ctypes.data, om.ctypes.data, nr.ctypes.data)
    assert rc in (_lib.UNAVAILABLE, _lib.INTERNAL) and L.tspgpu_last_error(null)
    rc = L.tspgpu_multistart_local_search(null, None, 8, -1.0, best, C.byref(cost), C.byref(start), C.byref(tsw), C.byref(tom),
                                          costs.ctypes.data)
    assert rc in (_lib.UNAVAILABLE, _lib.INTERNAL) and L.tspgpu_last_error(null)
    rc = L.tspgpu_multi_multistart_local_search(null, None, 8, -1.0, best, C.byref(cost), C.byref(start), C.byref(tsw), C.byref(tom))
    assert rc in (_lib.UNAVAILABLE, _lib.INTERNAL) and L.tspgpu_multi_last_error(null)
    assert (sw == -7).all() and (om == -7).all() and (nr == -7).all() and (best == -7).all() and (costs == -7.0).all()
    assert (cost.value, start.value, tsw.value, tom.value) == (-7.0, -7, -7, -7)


# ------------------------------------------------------------------------------------------------------------ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("elem", [3, 2, 1])
def test_gpu_every_slot_equals_the_model(elem):
    """berlin52, all 52 NN starts in slots 0 .. 51: some tours take one round and some two, so they leave the batch at
    different times"""
    want = nn_models("berlin52", 52)
    assert len({w["rounds"] for w in want}) >= 2
    eng = M.engine_for("berlin52", elem)
    assert eng.info()["elem"] == elem
    for s in range(52):
        eng.tour_nn(s, s)
    got = eng.tours_local_search(0, 52)
    check_slots(eng, 0, got, want)
    eng.close()


@pytest.mark.gpu
def test_gpu_range_inside_the_slots_leaves_the_neighbours_alone():
    want = nn_models("berlin52", 52)
    eng = M.engine_for("berlin52")
    for s in range(12):
        eng.tour_nn(s, s)
    outside = (0, 1, 2, 10, 11)
    before = {s: eng.tour_store(s) for s in outside}
    got = eng.tours_local_search(3, 7)
    check_slots(eng, 3, got, want[3:10])
    for s in outside:
        path, cost, delta = eng.tour_store(s)
        assert np.array_equal(path, before[s][0]) and (cost, delta) == before[s][1:], s
    got = eng.tours_local_search(11, 1)                 # a batch of one tour, the last slot
    check_slots(eng, 11, got, want[11:12])
    eng.close()


@pytest.mark.gpu
def test_gpu_chunks_and_the_start_list():
    """kroA100 in chunks of 7 tours: a permuted list with one start twice"""
    import travellingsalesmanoptimization_amd as T
    want = nn_models("kroA100", 100)
    rng = np.random.default_rng(31)
    starts = rng.permutation(100).astype(np.int32)
    starts = np.insert(starts, 60, starts[5])
    costs = np.array([want[s]["cost"] for s in starts])
    first = int(np.argmin(costs))                       # the first list entry of lowest cost
    eng = M.engine_for("kroA100")
    res = {}
    for cap in (7, 1024):
        eng.set_option(T.OPT_MAX_TOURS, cap)
        r = res[cap] = eng.multistart_local_search(starts)
        assert r["rc"] == 0 and np.array_equal(r["costs"], costs)
        assert (r["start"], r["cost"]) == (int(starts[first]), costs[first]) and np.array_equal(r["path"], want[starts[first]]["path"])
        assert r["two_opt_sweeps"] == sum(want[s]["two_opt_sweeps"] for s in starts)
        assert r["or_moves"] == sum(want[s]["or_moves"] for s in starts)
    assert all(np.array_equal(res[7][k], res[1024][k]) for k in res[7])
    r = eng.multistart_local_search()                   # starts == NULL: 0 .. n - 1
    assert r["rc"] == 0 and np.array_equal(r["costs"], [w["cost"] for w in want])
    eng.close()


@pytest.mark.gpu
def test_gpu_batch_plan_differs_at_pr1002():
    """six tours of pr1002: a sweep workgroup takes more positions than in the single-tour plan; results against the C model"""
    want = nn_models("pr1002", 6)
    eng = M.engine_for("pr1002")
    for s in range(6):
        eng.tour_nn(s, s)
    assert eng.info()["or_batch_r"] == 0
    got = eng.tours_local_search(0, 6)
    check_slots(eng, 0, got, want)
    info = eng.info()
    assert 2 <= info["or_single_r"] < info["or_batch_r"] <= 64, info
    eng.tour_nn(6, 0)
    got = eng.tours_local_search(6, 1)                  # one tour in the batch: the single-tour plan
    check_slots(eng, 6, got, want[:1])
    assert eng.info()["or_batch_r"] == info["or_single_r"]
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["lattice", "equal"])
@pytest.mark.parametrize("elem", [3, 2, 1])
def test_gpu_ties(which, elem):
    c, starts, want = tie_case(which)
    eng = M.engine_for(costs=c, elem=elem)
    assert eng.info()["elem"] == elem
    for s, path in enumerate(starts):
        eng.tour_load(s, path)
    got = eng.tours_local_search(0, 8)
    check_slots(eng, 0, got, want)
    eng.close()


def refused(eng, code, n):
    import travellingsalesmanoptimization_amd as T
    for call in (lambda: eng.tours_local_search(0, 2), lambda: eng.multistart_local_search(np.arange(4))):
        with pytest.raises(T.TspGpuError) as ei:
            call()
        assert ei.value.code == code and str(ei.value), ei.value


@pytest.mark.gpu
def test_gpu_precondition_matrix_mode():
    import travellingsalesmanoptimization_amd as T
    eng = M.engine_for("n1000", matrix_free=1)
    assert eng.info()["matrix_free"] == 1
    refused(eng, T._lib.UNIMPLEMENTED, 1000)
    M.still_works(eng, M.instance_costs("n1000"))
    eng.close()


@pytest.mark.gpu
def test_gpu_precondition_size():
    import travellingsalesmanoptimization_amd as T
    eng = T.Engine(0)
    eng.set_points(O.random_points(7, 3))
    eng.build_costs()
    refused(eng, T._lib.INVALID_ARGUMENT, 7)
    eng.set_points(M.instance_xy("n64"))
    eng.build_costs()
    M.still_works(eng, M.instance_costs("n64"))
    eng.close()


@pytest.mark.gpu
def test_gpu_precondition_symmetry():
    import travellingsalesmanoptimization_amd as T
    rng = np.random.default_rng(5)
    asym = rng.integers(1, 100, (64, 64)).astype(np.float64)
    np.fill_diagonal(asym, -1.0)
    eng = M.engine_for(costs=asym)
    assert eng.info()["symmetric"] == 0
    refused(eng, T._lib.FAILED_PRECONDITION, 64)
    c = M.instance_costs("n64")
    eng.set_costs(c)
    M.still_works(eng, c)
    eng.close()


@pytest.mark.gpu
def test_gpu_precondition_lds_limit():
    """doubles: four rows of 5120 cells do not fit a workgroup's LDS"""
    import travellingsalesmanoptimization_amd as T
    eng = M.engine_for("n5100", elem=1)
    assert eng.info()["elem"] == 1
    refused(eng, T._lib.RESOURCE_EXHAUSTED, 5100)
    # (the oracle's 2-opt descent at n = 5100 takes a minute: the normal two_opt after the refusal runs on a 64-node
    # instance given to the same context)
    eng.set_points(M.instance_xy("n64"))
    eng.build_costs()
    M.still_works(eng, M.instance_costs("n64"))
    eng.close()


@pytest.mark.gpu
def test_gpu_precondition_hole_and_sweep_cap():
    """a slot of the range that holds no tour: 9 and nothing runs; a capped 2-opt phase is not this descent: 3"""
    import travellingsalesmanoptimization_amd as T
    c = M.instance_costs("kroA100")
    eng = M.engine_for("kroA100")
    for s in (0, 1, 3):
        eng.tour_nn(s, s)
    before = [eng.tour_store(s) for s in (0, 1, 3)]
    with pytest.raises(T.TspGpuError) as ei:
        eng.tours_local_search(0, 4)
    assert ei.value.code == T._lib.FAILED_PRECONDITION and "slot 2" in str(ei.value)
    for s, b in zip((0, 1, 3), before):
        path, cost, _ = eng.tour_store(s)
        assert np.array_equal(path, b[0]) and cost == b[1]
    with pytest.raises(T.TspGpuError) as ei:
        eng.tours_local_search(0, 0)
    assert ei.value.code == T._lib.INVALID_ARGUMENT
    eng.set_option(T.OPT_SWEEP_CAP, 5)
    with pytest.raises(T.TspGpuError) as ei:
        eng.multistart_local_search()
    assert ei.value.code == T._lib.INVALID_ARGUMENT and "SWEEP_CAP" in str(ei.value)
    eng.set_option(T.OPT_SWEEP_CAP, -1)
    M.still_works(eng, c)
    eng.close()


@pytest.mark.gpu
def test_gpu_deadline_leaves_tours():
    import travellingsalesmanoptimization_amd as T
    c = M.instance_costs("kroA100")
    eng = M.engine_for("kroA100")
    for s in range(10):
        eng.tour_nn(s, 3 * s)
    got = eng.tours_local_search(0, 10, time_left_s=0.0)
    assert got["rc"] == T._lib.DEADLINE_EXCEEDED
    for s in range(10):
        path, cost, _ = eng.tour_store(s)
        assert O.valid_tour(path) and O.tour_cost(c, path) == cost, s
    r = eng.multistart_local_search(time_left_s=0.0)
    assert r["rc"] == T._lib.DEADLINE_EXCEEDED
    assert O.valid_tour(r["path"]) and O.tour_cost(c, r["path"]) == r["cost"] and 0 <= r["start"] < 100
    eng.close()


@pytest.mark.gpu
def test_gpu_two_contexts_behind_one_handle():
    import travellingsalesmanoptimization_amd as T
    want = nn_models("kroA100", 100)
    eng = M.engine_for("kroA100")
    one = eng.multistart_local_search()
    eng.close()
    first = int(np.argmin([w["cost"] for w in want]))
    assert (one["rc"], one["start"], one["cost"]) == (0, first, want[first]["cost"])
    m = T.MultiEngine([0, 0])
    m.set_points(M.instance_xy("kroA100"))
    m.build_costs()
    two = m.multistart_local_search()
    m.close()
    for k in ("rc", "cost", "start", "two_opt_sweeps", "or_moves"):
        assert two[k] == one[k], k
    assert np.array_equal(two["path"], one["path"]) and np.array_equal(one["path"], want[first]["path"])


# ------------------------------------------------------------------------------------------------------- host binary
def run_tsp(*args, every_start=None, timeout=300):
    env = dict(os.environ)
    for k in ("TSP_OR_OPT", "TSP_OR_OPT_EVERY_START", "TSP_GPU_DEVICES"):
        env.pop(k, None)
    if every_start is not None:
        env["TSP_OR_OPT_EVERY_START"] = every_start
    return subprocess.run([M.TSP_BIN, *args], capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)


@pytest.mark.gpu
def test_host_binary_switch():
    want = min(w["cost"] for w in nn_models("kroA100", 100))
    eng = M.engine_for("kroA100")
    plain = eng.multistart_nn_2opt()["cost"]
    eng.close()
    assert want <= plain
    args = ("-f", os.path.join(M.DATA, "kroA100.tsp"), "-alg", "2OPT_GREEDY", "-q")
    r = run_tsp(*args, every_start="1")
    assert r.returncode == 0 and r.stdout.strip() == "Cost: %.2f" % want, r.stdout + r.stderr
    for off in (None, "0"):
        r = run_tsp(*args, every_start=off)
        assert r.returncode == 0 and r.stdout.strip() == "Cost: %.2f" % plain, r.stdout + r.stderr
    r = run_tsp(*args, every_start="x")
    assert r.returncode != 0 and "TSP_OR_OPT_EVERY_START" in r.stderr and "Cost:" not in r.stdout, r.stdout + r.stderr
