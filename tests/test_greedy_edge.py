"""Greedy-edge tour construction over the neighbour lists (include/tspgpu.h "Greedy-edge construction").

The model is tests/greedy_edge_model.c (wrappers in tools/make_golden_greedy_edge.py): the sequential rule, sorting E1 and then
E2, and the parallel form in rounds of locally dominant edges.
CPU: the model's sequential form against a Python restatement written from the rule (sort, validity by union-find), a Python
statement of the parallel rounds against the model, K' = n - 1 against greedy over all pairs, the golden, the header and the
exported symbols.
GPU: the tour bit-equal with the model in every cell type and weight form at sizes around a wave and a workgroup, real-valued
f64 cells, the lattice, pr1002 / fnl4461 / pla85900 against the golden with the info counters, the slot form with a descent
behind it, refusals, memory across instances, the host binary's TSP_GREEDY_EDGE_NEIGHBOURS."""
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
import oracle as O  # noqa: E402
import make_golden_greedy_edge as G  # noqa: E402
from make_golden_greedy_edge import model_greedy, model_lists, model_rounds  # noqa: E402
from make_golden_two_opt_nl import digest  # noqa: E402
from test_two_opt_multi import MODES, engine_for, points_for, sym_int_matrix, symmetric_noise, weight_matrix  # noqa: E402
from test_or_opt_nl import rect_lattice, run_tsp  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_greedy_edge.json")
NEW_SYMBOLS = ["tspgpu_tour_greedy", "tspgpu_greedy_tour"]
W = 8


# ---------------------------------------------------------------------------------------------- the rule, restated in Python
def list_edges(nodes):
    return {(min(v, int(u)), max(v, int(u))) for v in range(len(nodes)) for u in nodes[v]}


class Forest:
    """rule 2 with union-find: degrees, and a cycle iff both ends are in one component"""

    def __init__(self, n):
        self.deg, self.up, self.edges = [0] * n, list(range(n)), []

    def root(self, v):
        while self.up[v] != v:
            self.up[v] = self.up[self.up[v]]
            v = self.up[v]
        return v

    def valid(self, a, b):
        return self.deg[a] < 2 and self.deg[b] < 2 and self.root(a) != self.root(b)

    def link(self, a, b):
        self.deg[a] += 1
        self.deg[b] += 1
        self.up[self.root(a)] = self.root(b)
        self.edges.append((a, b))


def tour_of(n, edges):
    """rule 4's closing edge and rule 5's orientation -> successor array"""
    adj = [[] for _ in range(n)]
    for a, b in edges:
        adj[a].append(b)
        adj[b].append(a)
    ends = [v for v in range(n) if len(adj[v]) == 1]
    assert len(edges) == n - 1 and len(ends) == 2
    adj[ends[0]].append(ends[1])
    adj[ends[1]].append(ends[0])
    path = np.empty(n, np.int32)
    prev, v = 0, min(adj[0])
    path[0] = v
    for _ in range(n - 1):
        nxt = adj[v][1] if adj[v][0] == prev else adj[v][0]
        path[v], prev, v = nxt, v, nxt
    assert v == 0
    return path


def py_greedy(c, nodes, all_pairs=False):
    """rules 3 and 4: sort E1, take in order; sort E2, take in order -> dict(path, edges, edges1, free)"""
    n = len(c)
    F = Forest(n)
    e1 = {(a, b) for a in range(n) for b in range(a + 1, n)} if all_pairs else list_edges(nodes)
    for a, b in sorted(e1, key=lambda e: (c[e[0]][e[1]], e[0], e[1])):
        if F.valid(a, b):
            F.link(a, b)
    edges1 = len(F.edges)
    free = [v for v in range(n) if F.deg[v] < 2]
    for a, b in sorted(((a, b) for i, a in enumerate(free) for b in free[i + 1:]), key=lambda e: (c[e[0]][e[1]], e[0], e[1])):
        if len(F.edges) == n - 1:
            break
        if F.valid(a, b):
            F.link(a, b)
    return {"path": tour_of(n, F.edges), "edges": set(F.edges), "edges1": edges1, "free": len(free)}


def py_rounds(c, nodes):
    """rule 7: rounds of locally dominant edges, fragments by their node sets -> dict(edges, edges1, free, rounds1, rounds2)"""
    n = len(c)
    deg, frag = [0] * n, {v: v for v in range(n)}       # frag[v]: the fragment's label
    members = {v: [v] for v in range(n)}
    accepted, rounds = [], [0, 0]

    def valid(a, b):
        return deg[a] < 2 and deg[b] < 2 and frag[a] != frag[b]

    def one_round(candidates):
        best = {}
        for a, b in candidates:
            if valid(a, b):
                k = (c[a][b], a, b)
                for v in (a, b):
                    if v not in best or k < best[v]:
                        best[v] = k
        fbest = {}
        for v, k in best.items():
            if frag[v] not in fbest or k < fbest[frag[v]]:
                fbest[frag[v]] = k
        take = sorted({k for k in fbest.values() if fbest[frag[k[1]]] == k and fbest[frag[k[2]]] == k})
        for _, a, b in take:
            deg[a] += 1
            deg[b] += 1
            fa, fb = frag[a], frag[b]
            for v in members[fb]:
                frag[v] = fa
            members[fa] += members.pop(fb)
            accepted.append((a, b))
        return len(take)

    e1 = sorted(list_edges(nodes))
    while one_round(e1):
        rounds[0] += 1
    edges1 = len(accepted)
    free0 = [v for v in range(n) if deg[v] < 2]
    while len(accepted) < n - 1:
        free = [v for v in range(n) if deg[v] < 2]
        assert one_round([(a, b) for i, a in enumerate(free) for b in free[i + 1:]]) > 0
        rounds[1] += 1
    return {"edges": set(accepted), "edges1": edges1, "free": len(free0), "rounds1": rounds[0], "rounds2": rounds[1]}


def model_edges(r):
    return {(v, int(u)) for v in range(len(r["adj"])) for u in r["adj"][v] if u > v}


def tour_cost(path, c):
    total = 0.0
    for i in range(len(path)):
        total += c[i][int(path[i])]
    return float(total)


def small_cases():
    rng = np.random.default_rng(4021)
    for n in list(range(5, 14)) + [17, 18, 25, 33, 40]:
        yield "matrix%d" % n, sym_int_matrix(n, rng).astype(np.float64)
        yield "points%d" % n, O.cost_matrix(rng.integers(0, 40, (n, 2)).astype(np.float64))
    yield "fewvalues12", sym_int_matrix(12, rng, hi=3).astype(np.float64)
    yield "real14", sym_int_matrix(14, rng) + symmetric_noise(14, rng)


def pr1002_matrix():
    return O.cost_matrix(G.tsplib_instance("pr1002")[0])


# ------------------------------------------------------------------------------------------------------------ CPU tests
def test_model_equals_the_python_restatement():
    """the C model's sequential form: the edge set, the tour from node 0, the counts and the cost in node order"""
    for name, c in small_cases():
        for K in (1, 2, 5, 16):
            nodes = model_lists(K, costs=c)
            want, got = py_greedy(c, nodes), model_greedy(nodes, costs=c)
            assert model_edges(got) == want["edges"], (name, K)
            assert np.array_equal(got["path"], want["path"]) and O.valid_tour(got["path"]), (name, K)
            assert (got["edges1"], got["free"]) == (want["edges1"], want["free"]), (name, K)
            assert got["cost"] == tour_cost(got["path"], c), (name, K)
            assert got["path"][0] == min(int(got["path"][0]), int(np.flatnonzero(got["path"] == 0)[0])), (name, K)


def parallel_case(c, K, what):
    nodes = model_lists(K, costs=c)
    seq, par, py = model_greedy(nodes, costs=c), model_rounds(nodes, costs=c), py_rounds(c, nodes)
    assert py["edges"] == model_edges(seq) == model_edges(par), what
    assert np.array_equal(seq["path"], par["path"]) and seq["cost"] == par["cost"], what
    assert (py["edges1"], py["free"]) == (seq["edges1"], seq["free"]) == (par["edges1"], par["free"]), what
    assert (py["rounds1"], py["rounds2"]) == (par["rounds1"], par["rounds2"]), what
    assert 1 <= par["rounds1"] <= len(c) - 1 and par["rounds2"] <= len(c) - 1, what
    return par


def test_parallel_rounds_give_the_sequential_edge_set():
    """rule 7 in Python and in the C model against the sequential form: the small instances, and a lattice, where nearly all keys
    tie on cost and the index tie-break decides"""
    for name, c in small_cases():
        for K in (1, 2, 5, 16):
            parallel_case(c, K, (name, K))
    lattice = O.cost_matrix(rect_lattice(12, 7))
    for K in (2, 4, 8):
        r = parallel_case(lattice, K, ("lattice", K))
        assert r["rounds1"] > 2


def test_parallel_rounds_give_the_sequential_edge_set_pr1002():
    g = json.load(open(GOLDEN))["pr1002_K8"]
    r = parallel_case(pr1002_matrix(), 8, "pr1002")
    assert (r["cost"], r["edges1"], r["free"], r["rounds1"], r["rounds2"]) == (g["cost"], g["edges1"], g["free"], g["rounds1"], g["rounds2"])


def test_full_lists_give_plain_greedy_edge():
    """rule 6: with K' = n - 1 E1 is every pair, and phase 2 has nothing left to join"""
    for name, c in small_cases():
        if len(c) > 17:
            continue
        nodes = model_lists(16, costs=c)
        assert nodes.shape[1] == len(c) - 1
        want, got = py_greedy(c, None, all_pairs=True), model_greedy(nodes, costs=c)
        assert model_edges(got) == want["edges"] and np.array_equal(got["path"], want["path"]), name
        assert got["edges1"] == len(c) - 1 and got["free"] == 2, name


def test_golden_is_the_model():
    """every entry below pla85900's, whose lists alone take the model an n^2 scan (tools/make_golden_greedy_edge.py writes it, the
    GPU test reads it); the golden's pr1002 and fnl4461 costs are the ones the issue's prototype gave"""
    want = json.load(open(GOLDEN))
    cases = [cs for cs in G.CASES if cs[0] != "pla85900"]
    got = json.loads(json.dumps(G.build(cases)))
    assert got == {k: v for k, v in want.items() if v["instance"] != "pla85900"} and len(want) == len(G.CASES)
    assert want["pr1002_K8"]["cost"] == 310535 and want["fnl4461_K8"]["cost"] == 211572
    p = want["pla85900_K8"]
    assert (p["n"], p["free"], p["rounds1"], p["rounds2"]) == (85900, 3106, 1675, 29)
    for e in want.values():
        assert e["rounds1"] > 1 and e["rounds2"] > 1 and e["edges1"] < e["n"] - 1


def test_header_states_the_rule_and_the_library_exports_the_symbols():
    text = open(os.path.join(ROOT, "include", "tspgpu.h")).read()
    for phrase in ("Greedy-edge construction", "its key is (c[a][b], a, b)", "Phase 1 (list edges)", "Phase 2 (joining)",
                   "the smaller-numbered of its two tour", "Equality with plain greedy edge", "locally dominant edges",
                   "74 / 75 the rounds of phase 1 / phase 2"):
        assert phrase in text, phrase
    from travellingsalesmanoptimization_amd import _lib
    L = _lib.load()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in _lib.SIGNATURES and s in text
    assert L.tspgpu_tour_greedy(None, 0) == 14
    assert L.tspgpu_greedy_tour(None, np.zeros(8, np.int32), None) == 14


# ------------------------------------------------------------------------------------------------------------ GPU tests
def check_slot(eng, slot, want, what):
    path, cost, last = eng.tour_store(slot)
    assert np.array_equal(path, want["path"]), what
    assert cost == want["cost"] and last == 0.0, (what, cost, want["cost"], last)


def check_counters(eng, want, what):
    info = eng.info()
    assert (info["greedy_edges1"], info["greedy_free"]) == (want["edges1"], want["free"]), what
    assert (info["greedy_rounds1"], info["greedy_rounds2"]) == (want["rounds1"], want["rounds2"]), what


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_tour_is_the_models(mode):
    """successor array, slot cost and last delta 0, bit-equal with the model: n = 5 .. 17 at K = 16 (K' = n - 1; n = 17 is the edge
    of rule 6), n = 64, 65, 257 at K = 1, 5, 8 (K = 1 leaves the most fragments: phase 2 carries the work; the sizes straddle a
    wave and a 256-thread workgroup).  The counters are the parallel form's"""
    eng = None
    for n, Ks in [(m, (16,)) for m in (5, 8, 9, 13, 17)] + [(m, (1, 5, 8)) for m in (64, 65, 257)]:
        xy, kind = points_for(mode, n, 7)
        if eng is None:
            eng = engine_for(mode, xy, kind)
        else:
            eng.set_points(xy, kind)
            eng.build_costs()
        c = weight_matrix(xy, kind)
        for K in Ks:
            eng.neighbours_build(K)
            nodes = model_lists(K, costs=c)
            want = model_rounds(nodes, costs=c)
            eng.tour_greedy(0)
            check_slot(eng, 0, want, (mode, n, K))
            check_counters(eng, want, (mode, n, K))
            if K == 16:
                assert want["edges1"] == n - 1 and want["rounds2"] == 0
            path, cost = eng.greedy_tour()
            assert np.array_equal(path, want["path"]) and cost == want["cost"], (mode, n, K)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", (9, 65, 257))
def test_gpu_real_valued_cells(n):
    """f64 cells that are no integers: the rule compares doubles exactly and adds nothing, so the tour is the model's and the cost
    is its sum in node order, bit for bit"""
    rng = np.random.default_rng(n)
    c = sym_int_matrix(n, rng, hi=50) + symmetric_noise(n, rng)
    eng = engine_for("f64", costs=c)
    for K in (2, 8):
        eng.neighbours_build(K)
        want = model_rounds(model_lists(K, costs=c), costs=c)
        eng.tour_greedy(0)
        check_slot(eng, 0, want, (n, K))
        check_counters(eng, want, (n, K))
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("u16", "mf_euc"))
def test_gpu_lattice(mode):
    """ties everywhere, many rounds: the index tie-break makes accepted chains advance link by link"""
    xy = rect_lattice(31, 9)
    eng = engine_for(mode, xy, 0)
    c = weight_matrix(xy, 0)
    for K in (4, 8):
        eng.neighbours_build(K)
        want = model_rounds(model_lists(K, costs=c), costs=c)
        assert want["rounds1"] > 8
        eng.tour_greedy(0)
        check_slot(eng, 0, want, (mode, K))
        check_counters(eng, want, (mode, K))
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ("pr1002_K8", "pr1002_K5", "pr1002_K16", "fnl4461_K8"))
def test_gpu_golden_instances(case):
    g = json.load(open(GOLDEN))[case]
    xy, kind = G.tsplib_instance(g["instance"])
    eng = engine_for("u16", xy, kind)
    eng.neighbours_build(g["K"])
    path, cost = eng.greedy_tour()
    assert cost == g["cost"] and digest(path) == g["path_sha256"]
    check_counters(eng, g, case)
    info = eng.info()
    assert info["greedy_rounds1"] > 1 and info["greedy_rounds2"] > 1       # no degenerate path
    eng.close()


# the child of test_gpu_golden_pla85900: first measured on one MI355X at 0.7 s of wall time for the whole process (imports, the
# points, the lists, NN(0) and the construction twice each); the limit leaves room for a cold start of the runtime on a busy
# machine and still ends a stuck round loop
PLA_TIMEOUT_S = 60


@pytest.mark.gpu
def test_gpu_golden_pla85900():
    """the ~1 700-round case, matrix-free, through tools/greedy_rate.py in a child with a time limit"""
    g = json.load(open(GOLDEN))["pla85900_K8"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "greedy_rate.py"), "--instance", "pla85900", "--reps", "1", "--construct-only"],
                       capture_output=True, text=True, timeout=PLA_TIMEOUT_S, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["matrix_free"] == 1 and out["n"] == 85900
    assert out["greedy_cost"] == g["cost"] and out["greedy_path_sha256"] == g["path_sha256"]
    assert (out["rounds1"], out["rounds2"], out["edges1"], out["free"]) == (g["rounds1"], g["rounds2"], g["edges1"], g["free"])


@pytest.mark.gpu
def test_gpu_slot_form_and_the_descent_behind_it():
    """tour_greedy(3) on a context whose slot array has not grown that far; every node awake; the descent with looks on it equals
    the same descent on the model's tour loaded with tour_load; the other slots keep what they held"""
    n = 257
    xy, kind = points_for("u16", n, 11)
    eng = engine_for("u16", xy, kind)
    c = weight_matrix(xy, kind)
    eng.neighbours_build(W)
    want = model_rounds(model_lists(W, costs=c), costs=c)
    eng.tour_greedy(3)
    check_slot(eng, 3, want, "slot 3")
    for f in range(3):
        assert eng.tour_awake(3, f).all()
    assert eng.L.tspgpu_tour_two_opt_nl(eng.ctx, 0, -1, -1.0, None, None) == 9       # slot 0 holds no tour: untouched
    eng.tour_nn(0, 0)
    eng.tour_nn(1, 5)
    keep = [eng.tour_store(s) for s in (0, 1)]
    eng.tour_sleep(3)
    eng.tour_greedy(3)                                                               # built again: awake again
    for f in range(3):
        assert eng.tour_awake(3, f).all()
    for s in (0, 1):
        got = eng.tour_store(s)
        assert np.array_equal(got[0], keep[s][0]) and got[1:] == keep[s][1:]
    a = eng.tour_local_search_nl3_dl(3, W, 1)
    eng.tour_load(4, want["path"])
    b = eng.tour_local_search_nl3_dl(4, W, 1)
    assert a == b and a["rc"] == 0
    pa, pb = eng.tour_store(3), eng.tour_store(4)
    assert np.array_equal(pa[0], pb[0]) and pa[1:] == pb[1:] and pa[1] <= want["cost"]
    eng.close()


@pytest.mark.gpu
def test_gpu_refusals_and_memory_across_instances():
    """the codes of the section; lists dropped by neighbours_build(0) and by a later set_points; the scratch memory follows the
    instance: a larger n through the same context builds the larger model's tour"""
    import travellingsalesmanoptimization_amd as T
    n = 40
    xy, kind = points_for("u16", n, 1)
    eng = T.Engine(0)
    L, ctx = eng.L, eng.ctx
    buf = np.zeros(512, np.int32)
    cost = T._lib.C.c_double()
    ref = T._lib.C.byref(cost)
    assert L.tspgpu_tour_greedy(ctx, 0) == 9 and L.tspgpu_greedy_tour(ctx, buf, ref) == 9           # no costs
    eng.close()
    eng = engine_for("u16", xy, kind)
    L, ctx = eng.L, eng.ctx
    assert L.tspgpu_tour_greedy(ctx, 0) == 9 and b"tspgpu_neighbours_build" in L.tspgpu_last_error(ctx)
    assert L.tspgpu_greedy_tour(ctx, buf, ref) == 9
    eng.neighbours_build(5)
    assert L.tspgpu_tour_greedy(ctx, -1) == 3
    assert L.tspgpu_greedy_tour(ctx, buf, None) == 3
    eng.tour_greedy(0)
    eng.neighbours_build(0)                                                         # dropped on purpose
    assert L.tspgpu_tour_greedy(ctx, 0) == 9 and b"no neighbour lists" in L.tspgpu_last_error(ctx)
    eng.neighbours_build(5)
    eng.tour_greedy(0)
    eng.set_points(xy, kind)                                                        # a new cost source
    eng.build_costs()
    assert L.tspgpu_tour_greedy(ctx, 0) == 9 and b"invalidated" in L.tspgpu_last_error(ctx)
    # an asymmetric matrix, and fewer than 5 nodes
    a = sym_int_matrix(12, np.random.default_rng(3)).astype(np.float64)
    a[2, 7] += 1
    eng.set_costs(a)
    assert L.tspgpu_tour_greedy(ctx, 0) == 9 and b"symmetric" in L.tspgpu_last_error(ctx)
    eng.set_costs(sym_int_matrix(4, np.random.default_rng(3)).astype(np.float64))
    assert L.tspgpu_tour_greedy(ctx, 0) == 3 and L.tspgpu_greedy_tour(ctx, buf, ref) == 3
    # the same context through a small, a larger and the small instance again
    for m in (9, 300, 9):
        xy2, kind2 = points_for("u16", m, 2)
        eng.set_points(xy2, kind2)
        eng.build_costs()
        eng.neighbours_build(5)
        c2 = weight_matrix(xy2, kind2)
        want = model_rounds(model_lists(5, costs=c2), costs=c2)
        eng.tour_greedy(2)
        check_slot(eng, 2, want, m)
        check_counters(eng, want, m)
    eng.close()


@pytest.mark.gpu
def test_host_binary_builds_the_greedy_edge_tour():
    """TSP_GREEDY_EDGE_NEIGHBOURS=8 with -alg GREEDY reports the golden cost; unset or 0 it reports the nearest-neighbour cost as
    before; a malformed value and a list length that differs from another switch's are refused"""
    g = json.load(open(GOLDEN))["pr1002_K8"]
    args = ("-f", os.path.join(ROOT, "tests", "golden", "data", "pr1002.tsp"), "-alg", "GREEDY", "-q")
    os.environ.pop("TSP_GREEDY_EDGE_NEIGHBOURS", None)
    plain = run_tsp(*args)
    nn_cost = O.nn_tour(pr1002_matrix(), 0)[1]
    assert plain[0] == 0 and plain[1] == "Cost: %.2f" % nn_cost
    code, out, err = run_tsp(*args, env_set={"TSP_GREEDY_EDGE_NEIGHBOURS": "8"})
    assert code == 0 and out == "Cost: %.2f" % g["cost"], (out, err)
    assert run_tsp(*args, env_set={"TSP_GREEDY_EDGE_NEIGHBOURS": "0"})[:2] == plain[:2]
    for bad in ("17", "x", "-1", ""):
        code, out, err = run_tsp(*args, env_set={"TSP_GREEDY_EDGE_NEIGHBOURS": bad})
        assert code != 0 and "TSP_GREEDY_EDGE_NEIGHBOURS" in err and "expected a list length" in err, bad
    code, out, err = run_tsp(*args, env_set={"TSP_GREEDY_EDGE_NEIGHBOURS": "8", "TSP_OR_OPT": "1", "TSP_OR_OPT_NEIGHBOURS": "5"})
    assert code != 0 and "the list lengths must be equal" in err
    # the polish follows unchanged: the descent over the same lists ends no higher than the construction
    code, out, err = run_tsp(*args, env_set={"TSP_GREEDY_EDGE_NEIGHBOURS": "8", "TSP_OR_OPT": "1", "TSP_OR_OPT_NEIGHBOURS": "8"})
    assert code == 0 and out.startswith("Cost: ") and float(out.split()[1]) <= g["cost"], (out, err)
