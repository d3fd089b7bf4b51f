"""The per-sweep 2-opt launch plan end to end on the device, the runtime's own occupancy answers included: what
tspgpu_info reports after a plan was made equals what the engine reported before the plan moved into csrc/tspgpu_plan.h.

The expected values are the "device" key of tests/golden/golden_plan.json, recorded on an MI355X at the commit that the
file's header names, next to the compute units and LDS bytes they were recorded with.  The engine takes its compute units
from the device (info "cus") and its LDS bytes per workgroup from the architecture (gfx950: 160 KiB, the only architecture
a context comes up on), so the test asserts both and does not skip on another chip: a plan is a function of the two.

Single tours are planned by tspgpu_time_sweep with one repetition, batches by the smallest multi-start call that plans for
that many tours (NN + 2-opt from 8 starts at n = 512).  Every case runs on a fresh context over random integer points
(coordinates below 2000: uint16 cells unless the case asks for wider ones), so that nothing of an earlier plan is left.
"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_plan.json")

GFX950_LDS_MAX = 160 * 1024
FIELDS = ["kernel", "wgs_per_tour", "lds_bytes", "block", "depth", "fused", "pipe2", "otf_kernel",
          "persist_wgs", "persist_edges", "persist_lds", "persist_window_cells"]       # the last four: tspgpu_info 16-19

# option numbers of include/tspgpu.h
ELEM, KERNEL, WGS, BLOCK, DEPTH, MATRIX_FREE, PIPE2 = 1, 2, 4, 8, 10, 11, 15
U16, I32, F64 = 3, 2, 1

# (name, n, options, tours, points): points "int" / "real" (real: matrix-free CEIL_2D without the integer form)
CASES = (
    [(f"u16-n{n}", n, {ELEM: U16}, 1, "int") for n in (8, 200, 1024, 2048, 4461, 6144, 8192)]
    + [(f"{nm}-n{n}", n, {ELEM: e}, 1, "int") for nm, e in (("i32", I32), ("f64", F64)) for n in (1024, 4096)]
    + [(f"{nm}-n512-batch8", 512, {ELEM: e}, 8, "int") for nm, e in (("u16", U16), ("f64", F64))]
    + [(f"matrix-free-n1000-{p}", 1000, {MATRIX_FREE: 1}, 1, p) for p in ("int", "real")]
    + [(f"u16-n2048-{nm}{v}", 2048, {ELEM: U16, o: v}, 1, "int")
       for nm, o, v in (("kernel", KERNEL, 1), ("kernel", KERNEL, 2), ("kernel", KERNEL, 3), ("block", BLOCK, 320), ("wgs", WGS, 7),
                        ("depth", DEPTH, 4), ("pipe2-", PIPE2, 0))])


def planned(name, n, options, tours, points):
    """-> (cus, {field: value}) of a fresh context after the plan for `tours` tours was made"""
    import travellingsalesmanoptimization_amd as T
    rng = np.random.default_rng(n)
    xy = rng.integers(0, 2000, (n, 2)).astype(np.float64)
    if points == "real":
        xy += 0.25
    eng = T.Engine(0)
    try:
        for opt, value in options.items():
            eng.set_option(opt, value)
        eng.set_points(xy, T.CEIL_2D if options.get(MATRIX_FREE) else T.EUC_2D)
        eng.build_costs()
        if tours == 1:
            eng.tour_load(0, np.roll(np.arange(n, dtype=np.int32), -1))
            eng.time_sweep(0, 1)
        else:
            eng.multistart_nn_2opt(starts=list(range(tours)))
        info = eng.info()
        return info["cus"], {k: info[k] for k in FIELDS}
    finally:
        eng.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["device"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gpu_plan_is_the_recorded_one(golden, case):
    cus, got = planned(*case)
    print(case[0], cus, got)
    assert cus == golden["cus"] and GFX950_LDS_MAX == golden["lds_max"], (cus, golden["cus"], golden["lds_max"])
    assert golden["fields"] == FIELDS
    assert [got[k] for k in FIELDS] == golden["plans"][case[0]], case[0]
