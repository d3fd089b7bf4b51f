"""Alpha-nearness of the Held-Karp 1-tree ("Held-Karp"): the rule and its model, on the CPU.  Every comparison is bit for bit.

alpha(a, b) = max(0, w(a, b) - beta(a, b)) under the 1-tree T(pi) of include/tspgpu.h "Held-Karp lower bound": beta is the largest
weight on the tree path between a and b (both >= 1), and w(0, u2) of node 0's larger edge for a pair with node 0.  The model is
tests/alpha_model.c (wrappers in tools/make_golden_alpha.py): the Prim tree of tests/held_karp_model.c and one depth-first walk per
source node that carries the path's maximum.
Here: the model against a Python brute force written from that rule; against a Python statement of the level rule -- beta(a, b) =
max(M_{r*-1}(a), M_{r*-1}(b)) from the labels and chosen weights of the Boruvka rounds, the form a device build would use --; the
properties alpha >= 0, symmetric, 0 on tree edges, w >= beta; the model's lists and rows against each other; the golden."""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import oracle as O  # noqa: E402
import make_golden_alpha as GA  # noqa: E402
from make_golden_alpha import model_alpha, model_alpha_lists, model_alpha_row, row_list  # noqa: E402
from make_golden_held_karp import model_one_tree  # noqa: E402
from test_held_karp import Sets, ints, py_tree, random_pi, tie_cases, weight, zero_edges  # noqa: E402
from test_held_karp_limits import line_points, pi_family  # noqa: E402
from test_two_opt_multi import sym_int_matrix  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_alpha.json")


def golden():
    return json.load(open(GOLDEN))


# ---------------------------------------------------------------------------------------------- the rule, restated in Python
def py_alpha(c, pi=None):
    """the rule by brute force: Kruskal's tree (test_held_karp.py), then for every source a walk over the tree's adjacency that
    carries the largest weight of the path -> alpha [n][n] (the diagonal 0); asserts w >= beta among the nodes >= 1"""
    n = len(c)
    pi = [0] * n if pi is None else [int(x) for x in pi]
    tree = py_tree(c, pi)
    adj = [[] for _ in range(n)]
    for a, b in tree["edges"]:
        if a != 0:
            adj[a].append(b)
            adj[b].append(a)
    b0 = zero_edges(c, pi)[1][0]
    out = [[0] * n for _ in range(n)]
    for a in range(1, n):
        beta, todo = {a: None}, [a]
        while todo:
            v = todo.pop()
            for u in adj[v]:
                if u not in beta:
                    w = weight(c, pi, min(u, v), max(u, v))
                    beta[u] = w if beta[v] is None else max(w, beta[v])
                    todo.append(u)
        assert len(beta) == n - 1
        for b in range(1, n):
            if b != a:
                w = weight(c, pi, min(a, b), max(a, b))
                assert w >= beta[b], (a, b)
                out[a][b] = w - beta[b]
    for u in range(1, n):
        out[0][u] = out[u][0] = max(0, weight(c, pi, 0, u) - b0)
    return out, tree


def py_levels(c, pi=None):
    """the level rule: the rounds of test_held_karp.py's py_rounds, recording per round every node's label and the weight its component chose
    -> (C [rounds][n], M [rounds][n] running maxima); node 0 takes no part"""
    n = len(c)
    pi = [0] * n if pi is None else [int(x) for x in pi]
    comp, nkeys, C, M = list(range(n)), 0, [], []
    while nkeys < n - 2:
        best = {}
        for v in range(1, n):
            k = min((weight(c, pi, min(v, u), max(v, u)), min(v, u), max(v, u)) for u in range(1, n) if comp[u] != comp[v])
            if comp[v] not in best or k < best[comp[v]]:
                best[comp[v]] = k
        C.append(list(comp))
        m = [best[comp[v]][0] if v else None for v in range(n)]
        M.append(m if not M else [None if v == 0 else max(M[-1][v], m[v]) for v in range(n)])
        take = sorted(set(best.values()))
        sets = Sets(n)
        for _, a, b in take:
            sets.up[sets.root(comp[a])] = sets.root(comp[b])
        comp = [sets.root(x) for x in comp]
        nkeys += len(take)
    return C, M


def py_alpha_by_levels(c, pi=None):
    n = len(c)
    p = [0] * n if pi is None else [int(x) for x in pi]
    C, M = py_levels(c, p)
    b0 = zero_edges(c, p)[1][0]
    out = [[0] * n for _ in range(n)]
    for a in range(n):
        for b in range(n):
            if a == b:
                continue
            w = weight(c, p, min(a, b), max(a, b))
            if a == 0 or b == 0:
                beta = b0
            else:
                r = next((r for r in range(1, len(C)) if C[r][a] == C[r][b]), len(C))
                beta = max(M[r - 1][a], M[r - 1][b])
            out[a][b] = max(0, w - beta)
    return out, len(C)


def growing_line(n, backwards):
    return O.cost_matrix(*line_points(n, backwards))


def cpu_cases():
    rng = np.random.default_rng(4250)
    for n in (5, 6, 9, 33, 100):
        yield "matrix%d" % n, sym_int_matrix(n, rng)
    yield from tie_cases()
    yield "line40", growing_line(40, False)
    yield "line40_backwards", growing_line(40, True)


def cpu_multipliers(n, rng):
    yield "zero", None
    yield "2^20", random_pi(n, rng)
    yield "2^45", pi_family("a", n, rng)
    yield "2^44", pi_family("c", n, rng)


# ------------------------------------------------------------------------------------------------------------ CPU tests
def test_model_equals_the_python_brute_force():
    """all pairs, and the properties: alpha >= 0, symmetric, 0 on the edges of T(pi) (w >= beta is asserted in py_alpha and
    in the model, which answers 3 otherwise)"""
    rng = np.random.default_rng(71)
    for name, c in cpu_cases():
        n = len(c)
        for tag, pi in cpu_multipliers(n, rng):
            want, tree = py_alpha(ints(c), pi)
            got = model_alpha(costs=c, pi=pi)
            assert got.tolist() == want, (name, tag)
            assert (got >= 0).all() and np.array_equal(got, got.T), (name, tag)
            assert all(got[a][b] == 0 for a, b in tree["edges"]), (name, tag)


def test_levels_give_beta():
    """the level rule stated in Python against the model; the line of growing gaps is one level in both numberings"""
    rng = np.random.default_rng(72)
    for name, c in cpu_cases():
        n = len(c)
        for tag, pi in cpu_multipliers(n, rng):
            want, levels = py_alpha_by_levels(ints(c), pi)
            assert model_alpha(costs=c, pi=pi).tolist() == want, (name, tag)
            assert 1 <= levels <= max(1, math.ceil(math.log2(n - 1))), (name, tag)
            if name.startswith("line") and pi is None:
                assert levels == 1, name


def test_model_lists_and_rows_agree():
    """the lists by a plain sort equal the rows' first K' under the key, and the row model on the model's own tree equals all pairs"""
    rng = np.random.default_rng(73)
    for name, c in cpu_cases():
        n = len(c)
        pi = random_pi(n, rng)
        al = model_alpha(costs=c, pi=pi)
        edges = model_one_tree(costs=c, pi=pi)["edges"]
        for K in (1, 5, 16):
            nodes, co = model_alpha_lists(K, costs=c, pi=pi)
            for v in range(n):
                row, cost = model_alpha_row(edges, v, costs=c, pi=pi)
                assert np.array_equal(row, al[v]), (name, v)
                assert np.array_equal(nodes[v], row_list(row, cost, v, K)) and np.array_equal(co[v], cost[nodes[v]]), (name, K, v)
                assert all(int(cost[u]) == int(c[v][u]) for u in range(n) if u != v)


def test_golden_is_the_model():
    g = golden()
    assert sorted(g) == sorted(GA.INSTANCES)
    for name, e in g.items():
        assert GA.entry(name) == e, name
