"""The oracle's move-level helpers and the history replay the GPU edge tests rely on (CPU only): move_delta_xy and
apply_move are the scan's arithmetic and the sweep's move, and replay accepts the oracle's own descent and rejects a
history that is wrong in any one of the ways it checks."""
import numpy as np
import pytest


def _instance(O, name):
    if name == "grid20":          # lattice: almost every delta is shared by many pairs
        g = np.arange(20, dtype=np.float64)
        return np.ascontiguousarray(np.stack(np.meshgrid(g * 10, g * 10), -1).reshape(-1, 2))
    if name == "dups":            # every point twice plus a collinear run: zero-length edges
        base = np.random.RandomState(9).randint(0, 50, size=(150, 2)).astype(np.float64)
        return np.ascontiguousarray(np.concatenate([base, base, np.stack([np.arange(60.0), np.zeros(60)], -1)]))
    if name == "frac":
        return np.random.RandomState(4).uniform(-500, 500, size=(157, 2))
    return O.random_points(int(name[1:]), 7)


def _oracle_history(O, xy, kind, succ0, cost0):
    """two_opt_once_xy to the local optimum, recorded as an engine records it (the final sweep: (-1, -1, delta))"""
    succ, cost = succ0.copy(), cost0
    a, b, d = [], [], []
    while True:
        dd, cost, mv = O.two_opt_once_xy(xy, kind, succ, cost)
        if dd >= -1e-7:
            a.append(-1); b.append(-1); d.append(dd)
            return (np.array(a, np.int32), np.array(b, np.int32), np.array(d)), succ, cost
        a.append(mv[0]); b.append(mv[1]); d.append(dd)


@pytest.mark.parametrize("kind", ["EUC_2D", "ATT", "CEIL_2D"])
@pytest.mark.parametrize("name", ["n120", "grid20", "dups", "frac"])
def test_move_delta_and_apply_match_two_opt_once(O, name, kind):
    k = getattr(O, kind)
    xy = _instance(O, name)
    succ, cost = O.nn_tour_xy(xy, k, 0)
    for _ in range(40):
        before = succ.copy()
        d, cost, (a, b) = O.two_opt_once_xy(xy, k, succ, cost)
        if d >= -1e-7:
            break
        assert a < b and O.move_delta_xy(xy, k, before, a, b) == d
        prev = np.empty_like(before)
        prev[before] = np.arange(len(before), dtype=np.int32)
        O.apply_move(before, prev, a, b)
        assert np.array_equal(before, succ)
        assert np.array_equal(prev[succ], np.arange(len(succ)))      # the inverse is kept


@pytest.mark.parametrize("kind", ["EUC_2D", "CEIL_2D"])
@pytest.mark.parametrize("name", ["n200", "grid20", "dups"])
def test_replay_accepts_the_oracle_descent(O, name, kind):
    k = getattr(O, kind)
    xy = _instance(O, name)
    succ0, cost0 = O.nn_tour_xy(xy, k, 3)
    hist, want, want_cost = _oracle_history(O, xy, k, succ0, cost0)
    m = len(hist[0])
    assert m > 5
    got, cost, kept, lens = O.replay(xy, k, succ0, cost0, hist, checkpoints=range(m), final=want, threads=4, keep=(0, m - 1))
    assert cost == want_cost and np.array_equal(got, want)
    assert np.array_equal(kept[0], succ0) and len(lens) == m - 1 and min(lens) >= 2
    # the same history with its arguments swapped (an engine may record (b, a)) replays the same way
    a, b, d = hist
    got, _, _, _ = O.replay(xy, k, succ0, cost0, (b, a, d), checkpoints=(0, m // 2, m - 1), final=want, threads=4)


@pytest.mark.parametrize("name", ["n200", "grid20", "dups"])
def test_replay_rejects_wrong_histories(O, name):
    k = O.EUC_2D
    xy = _instance(O, name)
    succ0, cost0 = O.nn_tour_xy(xy, k, 3)
    (a, b, d), want, _ = _oracle_history(O, xy, k, succ0, cost0)
    m = len(a)
    j = m // 2
    # a delta off by one
    dd = d.copy(); dd[j] += 1.0
    with pytest.raises(AssertionError):
        O.replay(xy, k, succ0, cost0, (a, b, dd), threads=4)
    # another improving pair of the same tour in place of the best: every delta right, only the checkpoint sees it
    succ = succ0.copy()
    for i in range(j):
        O.apply_move(succ, None, a[i], b[i])
    n = len(succ)
    alt = None
    for x in range(n - 1):
        for y in range(x + 1, n):
            if (x, y) == (a[j], b[j]) or succ[x] == succ[y] or x == succ[y] or y == succ[x]:
                continue
            if O.move_delta_xy(xy, k, succ, x, y) < -1e-7:
                alt = (x, y)
                break
        if alt:
            break
    assert alt is not None
    aa, bb, d2 = a[:j + 1].copy(), b[:j + 1].copy(), d[:j + 1].copy()
    aa[j], bb[j] = alt
    d2[j] = O.move_delta_xy(xy, k, succ, *alt)
    O.replay(xy, k, succ0, cost0, (aa, bb, d2), threads=4)                   # deltas alone cannot tell
    with pytest.raises(AssertionError):
        O.replay(xy, k, succ0, cost0, (aa, bb, d2), checkpoints=(j,), threads=4)
    # degenerate pairs (a == b, b the successor of a) are named as such, before any move is applied
    for x, y in ((a[0], a[0]), (a[0], succ0[a[0]])):
        with pytest.raises(AssertionError, match="degenerate pair"):
            O.replay(xy, k, succ0, cost0, (np.array([x]), np.array([y]), np.array([-1.0])), threads=4)
    # a history cut short: the final tour differs from the engine's
    with pytest.raises(AssertionError):
        O.replay(xy, k, succ0, cost0, (a[:m - 2], b[:m - 2], d[:m - 2]), final=want, threads=4)
    # a no-move entry in the middle of the descent
    with pytest.raises(AssertionError):
        O.replay(xy, k, succ0, cost0, (np.r_[a[:j], -1, a[j:]], np.r_[b[:j], -1, b[j:]], np.r_[d[:j], 0.0, d[j:]]), threads=4)
    # stopped early: the engine's "nothing found" where the oracle still improves
    cut = (np.r_[a[:j], -1], np.r_[b[:j], -1], np.r_[d[:j], 0.0])
    O.replay(xy, k, succ0, cost0, cut, threads=4)
    with pytest.raises(AssertionError):
        O.replay(xy, k, succ0, cost0, cut, checkpoints=(j,), threads=4)
