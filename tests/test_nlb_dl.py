"""Don't-look bits for the batched list descent, the multi-start and the VNS walks (include/tspgpu.h "Batched don't-look bits",
DESIGN 4.23).

CPU: the extended phase machine (csrc/tspgpu_nlphase.h, tests/nlphase_dl_main.cpp under ASan/UBSan) against the sweep, phase
and "wake all" sequences of the C model; the model of a walk with looks against a from-scratch difference set; the golden; the
header, the exported symbols, null handles.
GPU: the batch against the single-slot descent with looks, slot by slot and bit for bit, in every cell type and weight form;
slots that enter with different sets; the queue's stride; the C model; a range inside the slots; the multi-start; the walks
against the golden and against their restatement one iteration at a time; deadline, refusals, memory.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import make_golden_nlb_dl as GD  # noqa: E402
import make_golden_two_opt_nl as G2  # noqa: E402
import make_golden_vns_nl as GV  # noqa: E402
from make_golden_dont_look import all_awake, model_dl_descent, model_dl_sweep  # noqa: E402
from make_golden_two_opt_nl import digest, model_lists  # noqa: E402
from test_dont_look import sets_of, turn_slot_backward  # noqa: E402
from test_mem_owner import CSRC, SAN, asan_links  # noqa: E402
from test_nl_batch import is_tour  # noqa: E402
from test_two_opt_multi import EUC_2D, MODES, engine_for, points_for, random_tour, symmetric_noise, weight_matrix  # noqa: E402
from test_vns_nl import f64_cost_bound  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_nlb_dl.json")
NEW_SYMBOLS = ["tspgpu_tours_local_search_nl3_dl", "tspgpu_multistart_local_search_nl3_dl", "tspgpu_vns_walks_nl3_dl"]
COUNTERS = ("two_opt_sweeps", "two_opt_moves", "or_sweeps", "or_moves", "rounds", "three_sweeps", "three_moves", "three_phases", "looked",
            "full_sweeps")
SIZES = (8, 9, 13, 64, 65, 257)
K = W = 8         # the issue's lists and width (at n = 8 the lists hold 7 nodes and the width in effect is 7)


def tour_cost(path, c):
    return float(sum(c[i][int(path[i])] for i in range(len(path))))


# ------------------------------------------------------------------------------------------------------------ CPU tests
def dl_trace(start, cost, awake, nodes, width, closing, **src):
    """rule 8 of "Don't-look bits", phase by phase on the model's sweeps (dlm_sweep) -> the events (phase, K or -1 for an empty
    set that ends a phase with no sweep, |Q|, 1: every node wakes behind it), the path and the sets"""
    n = len(start)
    path, awake = start.copy(), awake.copy()
    ev, state = [], {"cost": cost}

    def phase(f):
        A = awake.reshape(3, n)[f]
        applied = 0
        if not A.any():
            if not closing:
                ev.append((f, -1, 0, 0))
                return 0
            A[:] = 1
        while True:
            d = model_dl_sweep(f, path, state["cost"], awake, nodes, width, **src)
            state["cost"] = d["cost"]
            k, q = d["moves"], d["looked"]
            applied += k
            wake = int(k == 0 and q < n and bool(closing))
            ev.append((f, k, q, wake))
            if k == 0:
                if not wake:
                    return applied
                A[:] = 1
    while True:
        while True:
            phase(0)
            if not phase(1):
                break
        if not width or not phase(2):
            return ev, path, awake


def phase_cases():
    xy = G2.tsplib_points("kroA100")
    yield "kroA100", G2.nn_from(xy, 0)[0], None, model_lists(8, xy=xy)[0], dict(xy=xy)
    xy = G2.tsplib_points("pr1002")
    nodes = model_lists(8, xy=xy)[0]
    for s in (0, 14, 4):
        yield "pr1002/%d" % s, G2.nn_from(xy, s)[0], None, nodes, dict(xy=xy)
    yield "pr1002/asleep", G2.nn_from(xy, 0)[0], np.zeros(3 * len(xy), np.uint8), nodes, dict(xy=xy)


def test_phase_machine_with_looks_stand_alone(tmp_path):
    """nlphase_close(NlbDlCtl) and nlphase_empty, stepped as the queue pass and the apply's close step them, fed the model's
    events: the machine is in the model's phase in front of every event, leaves "wake all" exactly where the model wakes every
    node, ends at the last event and holds dlm_descent's counters"""
    if not asan_links(tmp_path):
        pytest.skip("linking an empty program with g++ -fsanitize=address -static-libasan fails here (no sanitizer runtime)")
    exe = str(tmp_path / "nlphase_dl")
    r = subprocess.run(["g++", *SAN, "-g", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "nlphase_dl_main.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines, want = [], []
    woke = cascades = 0
    for name, start, sets, nodes, src in phase_cases():
        n = len(start)
        cost0 = GD.load_cost(start, **src)
        for closing in (0, 1):
            for width in (8, 0):
                awake = all_awake(n) if sets is None else sets
                ev, path, left = dl_trace(start, cost0, awake, nodes, width, closing, **src)
                p, a = start.copy(), awake.copy()
                m = model_dl_descent(p, cost0, a, nodes, width, closing, **src)
                assert np.array_equal(p, path) and np.array_equal(a, left), (name, closing, width)
                lines.append("%d %d %d %d %s\n" % (1 if width else 0, closing, n, len(ev), " ".join("%d %d" % (k, q) for _, k, q, _ in ev)))
                partial = [q for _, k, q, _ in ev if k >= 0 and q < n]
                want.append(((name, closing, width), len(ev) - 1, [m[k] for k in COUNTERS] + [max(partial, default=0)],
                             [f for f, _, _, _ in ev], [w for _, _, _, w in ev]))
                woke += sum(w for _, _, _, w in ev)
                cascades += sets is not None and not closing and all(k < 0 for _, k, _, _ in ev)
    assert woke > 0 and cascades == 2       # both new decisions are exercised
    cases = tmp_path / "cases.txt"
    cases.write_text("".join(lines))
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = [[int(v) for v in ln.split()] for ln in r.stdout.split("\n")[:3 * len(want)]]
    for i, (what, at, counters, phases, wakes) in enumerate(want):
        head, ph, wk = out[3 * i:3 * i + 3]
        assert head[0] == at, (what, head)
        assert head[1:] == counters, (what, head, counters)
        assert ph == phases and wk == wakes, what
    # a tour with nothing awake and no closing: three empty phases, the counters of a descent that ran no sweep
    asleep = [w for w in want if w[0][0] == "pr1002/asleep" and w[0][1] == 0]
    assert [w[3] for w in asleep] == [[0, 1, 2], [0, 1]] and all(w[2] == [0, 0, 0, 0, 1, 0, 0, 1 if w[0][2] else 0, 0, 0, 0] for w in asleep)


def test_difference_rule_and_the_model_of_a_walk():
    """one proper segment swap wakes exactly its six end nodes; behind every kick phase of the model's walk the set the descent
    enters with is the from-scratch difference of the two tours, and it is a multiple of 6 at most 6 x kicks"""
    n = 40
    rng = np.random.default_rng(3)
    path = random_tour(n, rng)
    order = [0]
    while len(order) < n:
        order.append(int(path[order[-1]]))
    i, j, k = 5, 17, 30
    new = order[:i + 1] + order[j + 1:k + 1] + order[i + 1:j + 1] + order[k + 1:]
    after = np.empty(n, np.int32)
    for p in range(n):
        after[new[p]] = new[(p + 1) % n]
    ends = {order[i], order[i + 1], order[j], order[j + 1], order[k], order[(k + 1) % n]}
    assert set(np.flatnonzero(GD.difference_set(path, after))) == ends and len(ends) == 6
    assert not GD.difference_set(path, path).any()
    rev = np.empty(n, np.int32)
    rev[path] = np.arange(n)                    # the same cycle walked backwards: no node's neighbours differ
    assert not GD.difference_set(path, rev).any()

    def brute(before, now):
        nb = lambda s: [{int(np.flatnonzero(s == v)[0]), int(s[v])} for v in range(len(s))]     # noqa: E731
        return np.array([x != y for x, y in zip(nb(before), nb(now))], np.uint8)
    xy, kind = points_for("u16", n, 0)
    c = weight_matrix(xy, kind)
    nodes, _ = model_lists(8, costs=c)
    log, tours = [], []

    def kick(p):
        GV.kick_port(p, GV.libc_rand)
    m = GD.model_walk_dl(path, tour_cost(path, c), nodes, 5, 7, 8, 0, kick=kick, log=log, costs=c)
    assert len(log) == 5 and log[0][0].all() and m["looked"] == sum(q for _, q, _ in log)
    # replay: the sets behind every kick phase from scratch
    GV.libc_srand(7)
    p = path.copy()
    for it in range(5):
        if it:
            assert np.array_equal(log[it][0], brute(tours[-1], p)), it
            assert int(log[it][0].sum()) % 6 == 0 or int(log[it][0].sum()) < 6 * 7
        aw = all_awake(n) if not it else np.tile(log[it][0], 3)
        model_dl_descent(p, tour_cost(p, c), aw, nodes, 8, 0, costs=c)
        tours.append(p.copy())
        for _ in range(GV.libc_rand() % 9 - 2):
            GV.kick_port(p, GV.libc_rand)
    assert np.array_equal(p, m["path"])


def test_golden_is_the_model():
    g = json.load(open(GOLDEN))
    assert (g["instance"], g["n"], g["K"], g["W"], g["walks"], g["k"]) == ("pr1002", 1002, 8, 8, 8, 6)
    xy = G2.tsplib_points("pr1002")
    nodes, _ = model_lists(8, xy=xy)
    start, cost0 = G2.nn_from(xy, 0)
    assert digest(start) == g["start_sha256"]
    for closing in (0, 1):
        for w in (0, 5):
            assert json.loads(json.dumps(GD.walk_entry(xy, nodes, start, float(cost0), 6, w, closing))) == g["closing%d" % closing][w]
    for e in g["closing0"]:     # what the looks are for: behind the kicks the descents look at a fraction of n x sweeps
        assert e["awake_at_entry"][0] == 1002 and all(a <= 6 * 6 for a in e["awake_at_entry"][1:])
        assert sum(e["looked_by_iteration"][1:]) < 1002 * sum(e["sweeps_by_iteration"][1:]) // 20


def test_header_symbols_and_null_handles():
    text = open(os.path.join(ROOT, "include", "tspgpu.h")).read()
    for phrase in ("Batched don't-look bits", "whose unordered pair {pred v, succ v} differs", "its six end nodes",
                   "82 `looked` of the last batched descent with looks", "[walks][11]", "all or none"):
        assert phrase in text, phrase
    from travellingsalesmanoptimization_amd import _lib
    L = _lib.load()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in _lib.SIGNATURES and s in text
        args = [np.zeros(16, np.int32) if t is _lib._ip else np.zeros(4) if t is _lib._dp else 1 if t in (_lib.C.c_int, _lib.C.c_long, _lib.C.c_double)
                else None for t in _lib.SIGNATURES[s][1][1:]]
        assert getattr(L, s)(None, *args) == 14, s


# ------------------------------------------------------------------------------------------------------------ GPU tests
def case_for(mode, n, seed=3):
    """-> (engine with lists, cost matrix, the model's source)"""
    if n == 1002:
        xy, kind = G2.tsplib_points("pr1002"), points_for(mode, 8, 0)[1]
    else:
        xy, kind = points_for(mode, n, seed)
    c = weight_matrix(xy, kind)
    if mode == "f64":
        c = c + symmetric_noise(n, np.random.default_rng(n))
        eng = engine_for(mode, costs=c)
    else:
        eng = engine_for(mode, xy, kind)
    eng.neighbours_build(K)
    return eng, c


def prepare_slot(eng, slot, kind, tour, c, width):
    """the five ways a slot enters: 0 all awake, 1 all asleep, 2 one awake node, 3 a local optimum kicked, 4 dir = -1 and a
    rotated order (all awake)"""
    n = len(tour)
    eng.tour_load(slot, tour)
    if kind == 1:
        eng.tour_sleep(slot)
    elif kind == 2:
        eng.tour_sleep(slot)
        eng.tour_wake(slot, [n // 2])
    elif kind == 3:
        eng.tour_local_search_nl3_dl(slot, width, 0)
        eng.tour_kick(slot, 1, n // 2, n - 2)
    elif kind == 4:
        turn_slot_backward(eng, slot, c)


def state_of(eng, slot):
    path, cost, delta = eng.tour_store(slot)
    return path, cost, delta, sets_of(eng, slot)


def same_state(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and np.array_equal(a[3], b[3])


def batch_against_single(eng, c, n, count, width, closing, seed, what, kinds=(0, 1, 2, 3, 4)):
    """slots 0 .. count - 1 and copies of them behind: the batch on the first, the single-slot descent on each copy"""
    rng = np.random.default_rng(seed)
    eng.tour_load(2 * count - 1, random_tour(n, rng))       # (the slot array grows once)
    entered = []
    for i in range(count):
        prepare_slot(eng, i, kinds[i % len(kinds)], random_tour(n, rng), c, width)
        eng.tour_copy(count + i, i)
        entered.append(state_of(eng, i))
    r = eng.tours_local_search_nl3_dl(0, count, width, closing)
    assert r["rc"] == 0, what
    info = eng.info()
    assert info["nlb_dl_looked"] == int(r["looked"].sum()) and info["nlb_dl_full_sweeps"] == int(r["full_sweeps"].sum()), what
    for i in range(count):
        s = eng.tour_local_search_nl3_dl(count + i, width, closing)
        assert {k: int(r[k][i]) for k in COUNTERS} == {k: s[k] for k in COUNTERS}, (what, i, kinds[i % len(kinds)])
        assert same_state(state_of(eng, i), state_of(eng, count + i)), (what, i, kinds[i % len(kinds)])
        assert is_tour(eng.tour_store(i)[0])
    return r, entered


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_batch_equals_the_single_slot_descent(mode):
    """(a), (b): tour, cost, last delta, the ten counters and the three sets, at every size, count = 1, 3 and 17, both closing
    values, width 0 and 8, with slots that enter all awake, all asleep, with one awake node, kicked, and turned backwards.
    Every count x width x closing runs at three of the six sizes; pr1002 (integer coordinates: not in the generic CEIL_2D form)
    runs three tours at width 8 with both closing values"""
    combos = [(count, width, closing) for count in (1, 3, 17) for width in (W, 0) for closing in (0, 1)]
    sizes = SIZES + ((1002,) if mode != "mf_ceil" else ())
    for at, n in enumerate(sizes):
        eng, c = case_for(mode, n)
        for count, width, closing in (combos[at % 2::2] if n != 1002 else [(3, W, 0), (3, W, 1)]):
            kinds = (0, 1, 2, 3, 4) if n >= 13 else (0, 1, 2, 3)
            if count == 1:
                kinds = (3,)
            batch_against_single(eng, c, n, count, width, closing, 10 * n + count, (mode, n, count, width, closing), kinds)
        eng.close()


@pytest.mark.gpu
def test_gpu_slots_in_different_phases_and_the_cascade():
    """(b): the five entries side by side, checked against the single slot and the C model; an all-asleep slot of a descent that
    does not close costs one launch and counts its empty phases as the single-slot descent does"""
    n = 64
    eng, c = case_for("u16", n)
    nodes, _ = model_lists(K, costs=c)
    for closing in (0, 1):
        r, entered = batch_against_single(eng, c, n, 5, W, closing, 77 + closing, ("mixed", closing))
        for i, (path, cost, _, sets) in enumerate(entered):         # (d): the C model from the state the slot entered with
            p, a = path.copy(), sets.copy()
            m = model_dl_descent(p, cost, a, nodes, W, closing, costs=c)
            got = state_of(eng, i)
            assert np.array_equal(got[0], p) and got[1] == m["cost"] and np.array_equal(got[3], a), (closing, i)
            assert {k: int(r[k][i]) for k in COUNTERS} == {k: m[k] for k in COUNTERS}, (closing, i)
        if not closing:
            assert [int(r[k][1]) for k in COUNTERS] == [0, 0, 0, 0, 1, 0, 0, 1, 0, 0]
    for i in range(3):
        eng.tour_load(i, random_tour(n, np.random.default_rng(i)))
        eng.tour_sleep(i)
    before = [state_of(eng, i) for i in range(3)]
    r = eng.tours_local_search_nl3_dl(0, 3, W, 0)
    info = eng.info()
    assert r["rc"] == 0 and info["nl_batch_launches"] <= 4 and info["nlb_dl_looked"] == 0      # (the host looks every fourth round)
    assert all(same_state(before[i], state_of(eng, i)) for i in range(3))
    r = eng.tours_local_search_nl3_dl(0, 3, 0, 0)
    assert list(r["rounds"]) == [1, 1, 1] and not r["three_phases"].any() and not r["or_sweeps"].any()
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["u16", "f64", "mf_att"])
def test_gpu_all_awake_first_sweep_through_the_stride(mode):
    """(c), (d): n = 257, every slot all awake: the first queue is longer than one pass of the queued sweep's grid in every
    phase; the batch equals the single slot and the C model (f64 with real costs: within test_vns_nl.f64_cost_bound)"""
    n, count = 257, 3
    eng, c = case_for(mode, n, seed=9)
    nodes, _ = model_lists(K, costs=c)
    for closing in (0, 1):
        r, entered = batch_against_single(eng, c, n, count, W, closing, 5 + closing, (mode, closing), kinds=(0,))
        info = eng.info()
        assert info["nlb_dl_qsweep_wgs"] * max(info["nl_nodes"], info["or_nl_starts"], info["three_nl_nodes"]) < n
        assert (r["full_sweeps"] >= 1).all() and info["nlb_dl_max_queue"] < n
        for i, (path, cost, _, sets) in enumerate(entered):
            p, a = path.copy(), sets.copy()
            m = model_dl_descent(p, cost, a, nodes, W, closing, costs=c)
            got = state_of(eng, i)
            assert np.array_equal(got[0], p) and np.array_equal(got[3], a), (mode, closing, i)
            assert {k: int(r[k][i]) for k in COUNTERS} == {k: m[k] for k in COUNTERS}, (mode, closing, i)
            if mode == "f64":
                tot = {"two_opt_sweeps": m["two_opt_sweeps"] + m["three_sweeps"], "two_opt_moves": m["two_opt_moves"] + m["three_moves"],
                       "or_sweeps": m["or_sweeps"], "or_moves": m["or_moves"]}
                assert abs(got[1] - m["cost"]) <= f64_cost_bound(c, tot), (closing, i, got[1], m["cost"])
            else:
                assert got[1] == m["cost"], (mode, closing, i)
    eng.close()


@pytest.mark.gpu
def test_gpu_slot_range_inside_the_slots_and_flagged_slots():
    """(e): the batch on slots 3 .. 6 of 10 leaves the others as they were; a plain batched call flags its slots "all awake",
    and the batch with looks fills them before it starts"""
    n = 65
    eng, c = case_for("i32", n)
    rng = np.random.default_rng(4)
    tours = [random_tour(n, rng) for _ in range(10)]
    for i in reversed(range(10)):
        eng.tour_load(i, tours[i])
    for i in (0, 4, 9):
        eng.tour_sleep(i)
        eng.tour_wake(i, [i, i + 7])
    eng.tour_load(20, tours[0])
    for i in range(3, 7):
        eng.tour_copy(11 + i, i)
    before = {i: state_of(eng, i) for i in (0, 1, 2, 7, 8, 9)}
    r = eng.tours_local_search_nl3_dl(3, 4, W, 0)
    assert r["rc"] == 0
    for i in range(3, 7):
        s = eng.tour_local_search_nl3_dl(11 + i, W, 0)
        assert {k: int(r[k][i - 3]) for k in COUNTERS} == {k: s[k] for k in COUNTERS}, i
        assert same_state(state_of(eng, i), state_of(eng, 11 + i)), i
    assert all(same_state(before[i], state_of(eng, i)) for i in before)
    assert not sets_of(eng, 3).any()
    assert eng.tours_local_search_nl3(3, 4, W)["rc"] == 0      # the plain batch: its slots count as all awake afterwards
    assert sets_of(eng, 3).all() and sets_of(eng, 6).all() and not sets_of(eng, 0).all()
    r = eng.tours_local_search_nl3_dl(3, 4, W, 0)
    assert r["rc"] == 0 and (r["full_sweeps"] >= 1).all() and (r["looked"] >= n).all() and not sets_of(eng, 3).any()
    with pytest.raises(Exception) as e:
        eng.tours_local_search_nl3_dl(8, 30, W, 0)
    assert e.value.code == 3
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["u16", "mf_euc"])
def test_gpu_multistart_pr1002(mode):
    """(f): starts 0 .. 15 in chunks of 5 against tour_nn + tour_local_search_nl3_dl per start"""
    import travellingsalesmanoptimization_amd as T
    xy = G2.tsplib_points("pr1002")
    eng = engine_for(mode, xy, EUC_2D)
    eng.neighbours_build(8)
    starts = list(range(16))
    want, tot = [], {k: 0 for k in COUNTERS}
    for s in starts:
        eng.tour_nn(30, s)
        d = eng.tour_local_search_nl3_dl(30, 8, 0)
        want.append(eng.tour_store(30))
        for k in COUNTERS:
            tot[k] += d[k]
    eng.set_option(T.OPT_MAX_TOURS, 5)
    r = eng.multistart_local_search_nl3_dl(8, 0, starts)
    assert r["rc"] == 0 and list(r["costs"]) == [w[1] for w in want]
    best = int(np.argmin([w[1] for w in want]))
    assert (r["start"], r["cost"]) == (best, want[best][1]) and np.array_equal(r["path"], want[best][0])
    assert {k: r[k] for k in COUNTERS if k not in ("rounds", "three_phases")} == {k: tot[k] for k in COUNTERS if k not in ("rounds", "three_phases")}
    assert r["looked"] < 1002 * (r["two_opt_sweeps"] + r["or_sweeps"] + r["three_sweeps"]) and r["full_sweeps"] >= 16
    eng.set_option(T.OPT_SWEEP_CAP, 3)
    with pytest.raises(T.TspGpuError) as e:
        eng.multistart_local_search_nl3_dl(8, 0, [0, 1])
    assert e.value.code == 3
    eng.close()


def walk_args(starts, cost0):
    paths = np.ascontiguousarray(np.stack(starts), np.int32)
    return paths, paths.copy(), np.array(cost0, np.float64)


def restated_walk(eng, slot, start, best_cost, rv, k, width, closing):
    """one iteration at a time on a slot: tour_load, tour_sleep, tour_wake(D), tour_local_search_nl3_dl, tour_store, and the
    Python port of vns_kick_host -> dict as the walks answer"""
    path, best, opt = start.copy(), start.copy(), None
    tot = {t: 0 for t in GD.TOTALS}
    trace, cur = [], 0
    for _ in range(k):
        eng.tour_load(slot, path)
        if opt is not None:
            eng.tour_sleep(slot)
            eng.tour_wake(slot, np.flatnonzero(GD.difference_set(opt, path)))
        d = eng.tour_local_search_nl3_dl(slot, width, closing)
        path, cost, _ = eng.tour_store(slot)
        for t in COUNTERS:
            tot[t] += d[t]
        trace.append(cost)
        if cost < best_cost:
            best_cost, best = cost, path.copy()
        opt = path.copy()
        cur, kicks = GV.kick_phase_port(path, rv, cur)
        tot["kicks"] += kicks
    eng.tour_load(slot, path)
    return dict(tot, path=path, cost=eng.tour_store(slot)[1], best_path=best, best_cost=best_cost, trace=trace, consumed=cur)


def check_walk(r, paths, bests, w, m, k, what):
    assert (int(r["iterations"][w]), int(r["kick_pending"][w])) == (k, 0), what
    assert np.array_equal(paths[w], m["path"]) and np.array_equal(bests[w], m["best_path"]), what
    assert r["costs"][w] == m["cost"] and r["best_costs"][w] == m["best_cost"], what
    assert list(r["trace"][w]) == list(m["trace"]), what
    assert int(r["consumed"][w]) == m["consumed"], what
    assert {t: int(r["totals"][t][w]) for t in GD.TOTALS} == {t: m[t] for t in GD.TOTALS}, what


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["u16", "i32", "f64"])
def test_gpu_walks_equal_their_restatement(mode):
    """(g): n = 8, 10, 13, 64: three walks bit-equal with the restatement one iteration at a time; the same walks fed their
    numbers in pieces, both closing values -- a first call with exactly the numbers the walk that needs the fewest uses, so that
    it finishes while the others run dry in the same call, then calls of 3, 5, 1 and 40 numbers, the dry walks resumed in front
    of their kick phases; a walk alone"""
    for n in (8, 10, 13, 64):
        walks, k = 3, 4
        eng, c = case_for(mode, n, seed=6)
        rng = np.random.default_rng(n)
        starts = [random_tour(n, rng) for _ in range(walks)]
        cost0 = [tour_cost(s, c) for s in starts]
        rvs = [GV.libc_draws(11 + w, GV.draws_for(k)) for w in range(walks)]
        for closing in (0, 1):
            want = [restated_walk(eng, 8, starts[w], cost0[w], rvs[w], k, W, closing) for w in range(walks)]
            paths, bests, bc = walk_args(starts, cost0)
            r = eng.vns_walks_nl3_dl(paths, k, np.stack(rvs), bests, bc, W, closing, want_trace=True)
            assert r["rc"] == 0
            for w in range(walks):
                check_walk(r, paths, bests, w, want[w], k, (mode, n, closing, w))
            if n >= 13:
                assert any(want[w]["looked"] < n * (want[w]["two_opt_sweeps"] + want[w]["or_sweeps"] + want[w]["three_sweeps"]) for w in range(walks))
            # a walk alone is the walk in company
            p1, b1, c1 = walk_args(starts[1:2], cost0[1:2])
            r1 = eng.vns_walks_nl3_dl(p1, k, rvs[1][None, :], b1, c1, W, closing)
            assert r1["rc"] == 0 and np.array_equal(p1[0], paths[1]) and np.array_equal(b1[0], bests[1]) and c1[0] == bc[1]
            assert all(int(r1["totals"][t][0]) == int(r["totals"][t][1]) for t in GD.TOTALS)
            # refills; a dry walk waits in front of its kick phase
            used = [int(v) for v in r["consumed"]]
            assert min(used) < max(used)
            p2, b2, c2 = walk_args(starts, cost0)
            it, kp = np.zeros(walks, np.int32), np.zeros(walks, np.int32)
            at, tot = [0] * walks, {t: np.zeros(walks, np.int64) for t in GD.TOTALS}
            entered_pending = dry_beside_finishing = False
            for calls, size in enumerate([min(used)] + [3, 5, 1, 40] * 40):
                rv = np.stack([np.resize(rvs[w][at[w]:at[w] + size], size) for w in range(walks)])
                entered_pending |= bool(kp.any())
                q = eng.vns_walks_nl3_dl(p2, k, rv, b2, c2, W, closing, iterations=it, kick_pending=kp)
                assert q["rc"] in (0, 8)
                dry_beside_finishing |= q["rc"] == 8 and bool(((q["iterations"] == k) & (it < k)).any())
                it, kp = q["iterations"], q["kick_pending"]
                for w in range(walks):
                    at[w] += int(q["consumed"][w])
                for t in GD.TOTALS:
                    tot[t] += q["totals"][t]
                if q["rc"] == 0:
                    break
            assert q["rc"] == 0 and calls < 160 and entered_pending and dry_beside_finishing
            assert np.array_equal(p2, paths) and np.array_equal(b2, bests) and np.array_equal(c2, bc)
            assert at == [int(v) for v in r["consumed"]]
            for t in GD.TOTALS:
                assert np.array_equal(tot[t], r["totals"][t]), t
        eng.close()


@pytest.mark.gpu
def test_gpu_walks_pr1002_golden_and_the_looks_are_on():
    """(g), (h): pr1002, K = W = 8, 8 walks of 6 iterations against the model's golden, closing 0 and 1.  With closing 0 the
    `looked` of the iterations 2 .. k is strictly below n x their sweeps -- a walk that silently stayed all awake would look at
    n units in every sweep.  The plain walks on the same numbers answer the same in front of and behind the calls with looks in
    this session; that their answer is the one of earlier commits is pinned by the goldens of test_nl3_batch and test_vns_nl"""
    g = json.load(open(GOLDEN))
    walks, k, n = g["walks"], g["k"], g["n"]
    xy = G2.tsplib_points("pr1002")
    start, cost0 = G2.nn_from(xy, 0)
    rvs = np.stack([GV.libc_draws(1 + w, GV.draws_for(k)) for w in range(walks)])
    eng = engine_for("u16", xy, EUC_2D)
    eng.neighbours_build(8)

    def plain():
        paths, bests, bc = walk_args([start] * 2, [float(cost0)] * 2)
        r = eng.vns_walks_nl3(paths, 3, rvs[:2], bests, bc, 8, want_trace=True)
        return r["rc"], paths.tobytes(), bests.tobytes(), bc.tobytes(), r["trace"].tobytes(), {t: v.tolist() for t, v in r["totals"].items()}
    plain_before = plain()
    for closing in (0, 1):
        paths, bests, bc = walk_args([start] * walks, [float(cost0)] * walks)
        r = eng.vns_walks_nl3_dl(paths, k, rvs, bests, bc, 8, closing, want_trace=True)
        assert r["rc"] == 0
        for w, e in enumerate(g["closing%d" % closing]):
            assert digest(paths[w]) == e["path_sha256"] and digest(bests[w]) == e["best_path_sha256"], (closing, w)
            assert r["costs"][w] == e["cost"] and r["best_costs"][w] == e["best_cost"] and list(r["trace"][w]) == e["trace"], (closing, w)
            assert int(r["consumed"][w]) == e["consumed"]
            assert {t: int(r["totals"][t][w]) for t in GD.TOTALS} == {t: e[t] for t in GD.TOTALS}, (closing, w)
        if closing == 0:
            p1, b1, c1 = walk_args([start] * walks, [float(cost0)] * walks)
            first = eng.vns_walks_nl3_dl(p1, 1, rvs, b1, c1, 8, 0)
            sweeps = lambda t: t["two_opt_sweeps"] + t["or_sweeps"] + t["three_sweeps"]        # noqa: E731
            later_looked = r["totals"]["looked"] - first["totals"]["looked"]
            later_sweeps = sweeps(r["totals"]) - sweeps(first["totals"])
            print("looked in iterations 2 .. k:", later_looked.tolist(), "n x sweeps:", (n * later_sweeps).tolist())
            assert (later_sweeps > 0).all() and (later_looked < n * later_sweeps).all()
            assert int(later_looked.sum()) == sum(sum(e["looked_by_iteration"][1:]) for e in g["closing0"])
    assert plain() == plain_before
    eng.close()


@pytest.mark.gpu
def test_gpu_deadline_refusals_and_memory():
    """(i): a deadline that has passed answers 4 with valid tours whose stored cost is their cost; refusals; the batch's memory
    goes with the instance and comes back; the slots grow under the sets"""
    import travellingsalesmanoptimization_amd as T
    n = 64
    eng, c = case_for("u16", n)
    rng = np.random.default_rng(8)
    tours = [random_tour(n, rng) for _ in range(4)]
    for left in (0.0, 1.0e-6):
        for i in reversed(range(4)):
            eng.tour_load(i, tours[i])
        r = eng.tours_local_search_nl3_dl(0, 4, W, 1, time_left_s=left)
        assert r["rc"] == 4
        for i in range(4):
            path, cost, _ = eng.tour_store(i)
            assert is_tour(path) and cost == tour_cost(path, c)
        paths, bests, bc = walk_args(tours[:2], [tour_cost(t, c) for t in tours[:2]])
        q = eng.vns_walks_nl3_dl(paths, 3, np.stack([GV.libc_draws(1 + w, 500) for w in range(2)]), bests, bc, W, 0, time_left_s=left)
        assert q["rc"] == 4 and all(is_tour(p) for p in paths) and [tour_cost(p, c) for p in paths] == list(q["costs"])
        m = eng.multistart_local_search_nl3_dl(W, 0, [0, 1, 2], time_left_s=left)
        assert m["rc"] == 4 and is_tour(m["path"]) and m["cost"] == tour_cost(m["path"], c)
    for bad in (-1, 17):
        with pytest.raises(T.TspGpuError) as e:
            eng.tours_local_search_nl3_dl(0, 2, bad, 0)
        assert e.value.code == 3
    with pytest.raises(T.TspGpuError) as e:
        eng.tours_local_search_nl3_dl(0, 0, W, 0)
    assert e.value.code == 3
    with pytest.raises(T.TspGpuError) as e:
        eng.tours_local_search_nl3_dl(2, 40, W, 0)      # slots past the end
    assert e.value.code in (3, 9)
    # slot growth: sets that exist grow with the slots and keep their contents
    eng.tour_load(0, tours[0])
    eng.tour_sleep(0)
    eng.tour_wake(0, [5, 6])
    kept = sets_of(eng, 0)
    eng.tour_load(70, tours[1])
    assert np.array_equal(sets_of(eng, 0), kept)
    for i in range(1, 70):
        eng.tour_copy(i, 70)
    r = eng.tours_local_search_nl3_dl(0, 71, W, 0)
    assert r["rc"] == 0 and r["looked"][0] < r["looked"][1] == r["looked"][70]
    # a new instance drops everything; the next call allocates again
    eng.neighbours_build(0)
    with pytest.raises(T.TspGpuError) as e:
        eng.tours_local_search_nl3_dl(0, 2, W, 0)
    assert e.value.code == 9
    xy, kind = points_for("u16", 13, 1)
    eng.set_points(xy, kind)
    eng.build_costs()
    eng.neighbours_build(K)
    c13 = weight_matrix(xy, kind)
    with pytest.raises(T.TspGpuError) as e:
        eng.tours_local_search_nl3_dl(0, 2, W, 0)       # no tours yet
    assert e.value.code in (3, 9)
    batch_against_single(eng, c13, 13, 3, W, 1, 2, "after a new instance")
    eng.close()


# ----------------------------------------------------------------------------------------------------------------- host
DATA = os.path.join(ROOT, "tests", "golden", "data")
SWITCHES = ("TSP_VNS_DONT_LOOK", "TSP_EVERY_START_DONT_LOOK", "TSP_DONT_LOOK_CLOSING")


TSP_BIN = os.path.join(ROOT, "travellingsalesmanoptimization_amd", "host", "tsp")


def run_tsp(*args, env_set=None, timeout=300):
    """the binary in a child environment of its own: the caller's TSP_ switches are left out (its choice of device stays),
    env_set is put in"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("TSP_") or k == "TSP_GPU_DEVICE"}
    env.update(env_set or {})
    os.makedirs(os.path.join(ROOT, "results"), exist_ok=True)
    r = subprocess.run([TSP_BIN, *args], capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    return r.returncode, r.stdout.strip(), r.stderr


@pytest.mark.gpu
def test_host_binary_switches():
    """(j): TSP_EVERY_START_DONT_LOOK=1 and TSP_VNS_DONT_LOOK=1 give the costs of the engine's entry points on the same input,
    with and without TSP_DONT_LOOK_CLOSING=1; wrong values are refused, switches without their companions are warned about"""
    k = 4
    xy = G2.tsplib_points("pr1002")
    eng = engine_for("u16", xy, EUC_2D)
    eng.neighbours_build(8)
    ms = [eng.multistart_local_search_nl3_dl(8, closing) for closing in (0, 1)]
    start, cost0, _ = eng.nn_all()
    rv = GV.libc_draws(1, 32 * k + 1024)
    walk = []
    for closing in (0, 1):
        paths, bests, bc = walk_args([start], [cost0])
        r = eng.vns_walks_nl3_dl(paths, k, rv[None, :], bests, bc, 8, closing)
        assert r["rc"] == 0
        walk.append(float(bc[0]))
    eng.close()
    every = ("-f", os.path.join(DATA, "pr1002.tsp"), "-alg", "2OPT_GREEDY")
    env = {"TSP_EVERY_START_NEIGHBOURS": "8", "TSP_EVERY_START_3OPT_WIDTH": "8", "TSP_EVERY_START_DONT_LOOK": "1"}
    for closing in (0, 1):
        rc, out, err = run_tsp(*every, "-q", env_set=dict(env, TSP_DONT_LOOK_CLOSING=str(closing)))
        assert ms[closing]["rc"] == 0 and rc == 0 and out == "Cost: %.2f" % ms[closing]["cost"], (closing, err)
    vns = ("-f", os.path.join(DATA, "pr1002.tsp"), "-alg", "VNS", "-k", str(k), "-seed", "1")
    venv = {"TSP_VNS_NEIGHBOURS": "8", "TSP_VNS_3OPT_WIDTH": "8", "TSP_VNS_DONT_LOOK": "1"}
    for closing in (0, 1):
        rc, out, err = run_tsp(*vns, "-q", env_set=dict(venv, TSP_DONT_LOOK_CLOSING=str(closing)))
        assert rc == 0 and out == "Cost: %.2f" % walk[closing], (closing, err)
    small = ("-f", os.path.join(DATA, "berlin52.tsp"), "-alg", "2OPT_GREEDY")
    for name in SWITCHES:
        for bad in ("2", "yes", ""):
            rc, out, err = run_tsp(*small, "-q", env_set={name: bad})
            assert rc != 0 and name in err and "expected 0 or 1" in err, (name, bad)
        rc, out, err = run_tsp(*small, env_set={name: "1"})
        assert rc == 0 and name + "=1 has no effect without" in out + err, name
    plain = run_tsp(*small, "-q")
    assert plain[0] == 0 and run_tsp(*small, "-q", env_set={"TSP_EVERY_START_DONT_LOOK": "1"})[:2] == plain[:2]
