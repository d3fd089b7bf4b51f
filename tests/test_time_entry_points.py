"""The timing entry points (include/tspgpu.h: tspgpu_time_sweep, tspgpu_time_build, tspgpu_time_or_sweep,
tspgpu_time_multi_sweep, tspgpu_time_nl_sweep), which the tools under tools/ measure with: each returns a mean, the three
candidate sweeps leave the slot as it was loaded, and none of them wears anything out when it is called again and again
(they share one warm-up-and-time helper, which destroys its events on every way out).
n = 64 random integer points, once with a u16 matrix and once matrix-free (EUC_2D), neighbour lists of K = 5."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from test_two_opt_multi import EUC_2D, engine_for, points_for, random_tour  # noqa: E402

N, K, REPS, CALLS = 64, 5, 2, 50


@pytest.fixture(scope="module", params=["u16", "mf_euc"])
def loaded(request):
    """-> (engine, mode, path, cost): a random tour in slot 0 and the lists built"""
    import travellingsalesmanoptimization_amd as T
    mode = request.param
    xy, kind = points_for(mode, N, 7)
    assert kind == EUC_2D
    eng = engine_for(mode, xy, kind)
    if mode == "mf_euc":
        eng.set_option(T._lib.OPT_OR_MATRIX_FREE, 1)
    eng.neighbours_build(K)
    path = random_tour(N, np.random.default_rng(11))
    eng.tour_load(0, path)
    _, cost, _ = eng.tour_store(0)
    yield eng, mode, path, cost
    eng.close()


def slot_is(eng, path, cost):
    got, c, _ = eng.tour_store(0)
    return np.array_equal(got, path) and c == cost


@pytest.mark.gpu
def test_gpu_candidate_sweeps_return_a_mean_and_leave_the_slot(loaded):
    eng, mode, path, cost = loaded
    for timer in (eng.time_or_sweep, eng.time_multi_sweep, eng.time_nl_sweep):
        ms = timer(0, REPS)
        print(mode, timer.__name__, ms)
        assert ms > 0, (mode, timer.__name__, ms)
        assert slot_is(eng, path, cost), (mode, timer.__name__)


@pytest.mark.gpu
def test_gpu_sweep_and_build_return_a_mean(loaded):
    eng, mode, path, cost = loaded
    ms = eng.time_sweep(0, REPS)
    print(mode, "time_sweep", ms)
    assert ms > 0, (mode, ms)
    ms = eng.time_build(REPS)
    print(mode, "time_build", ms)
    assert ms > 0 if mode == "u16" else ms == 0, (mode, ms)


@pytest.mark.gpu
def test_gpu_fifty_calls_in_a_row(loaded):
    eng, mode, path, cost = loaded
    for timer in (eng.time_or_sweep, eng.time_multi_sweep, eng.time_nl_sweep):
        for _ in range(CALLS):
            assert timer(0, REPS) > 0, (mode, timer.__name__)
    assert slot_is(eng, path, cost), mode
    for _ in range(CALLS):
        assert eng.time_sweep(0, REPS) > 0, mode
    for _ in range(CALLS):
        ms = eng.time_build(REPS)
        assert ms > 0 if mode == "u16" else ms == 0, (mode, ms)
