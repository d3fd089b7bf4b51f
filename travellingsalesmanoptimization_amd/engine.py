"""Engine: Python handle on one tspgpu context (one MI355X).

Thin: every method is one call through the C ABI of include/tspgpu.h.  Tours
are successor arrays (int32), matrices row-major float64, as in the reference.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (DEADLINE_EXCEEDED, ELEM_AUTO, ELEM_F64, ELEM_I32, EUC_2D, T_OK)


class TspGpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"tspgpu error {code}: {msg}")
        self.code = code


class LowerBound:
    """what Engine.lower_bound returns: the bound (ceil(best L / 128)), pi* [n] int64 in units of 1/128, the iterations evaluated,
    the stop reason (0 iterations ran out, 1 the 1-tree is a tour -- `path` holds it --, 2 the bound met `upper`, 3 the step
    reached 0, 4 deadline, 5 a multiplier would pass 2^45), the upper bound used and the return code (0, or 4 on a deadline)."""

    def __init__(self, bound, pi, iters, reason, path, upper, rc):
        self.bound, self.pi, self.iters, self.reason, self.path, self.upper, self.rc = bound, pi, iters, reason, path, upper, rc

    def gap(self, cost):
        """(cost - bound) / bound"""
        return (cost - self.bound) / self.bound

    def __repr__(self):
        return f"LowerBound(bound={self.bound:.0f}, iters={self.iters}, reason={self.reason})"


class Engine:
    def __init__(self, device=0):
        self.L = _lib.load()
        self.ctx = C.c_void_p()
        rc = self.L.tspgpu_create(device, C.byref(self.ctx))
        if rc != T_OK:
            raise TspGpuError(rc, "tspgpu_create failed (no gfx950 device visible?)")
        self.n = 0

    def close(self):
        if self.ctx:
            self.L.tspgpu_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, ok=(T_OK,)):
        if rc not in ok:
            raise TspGpuError(rc, self.L.tspgpu_last_error(self.ctx).decode())
        return rc

    # ---- options / info
    def set_option(self, opt, value):
        self._ck(self.L.tspgpu_set_option(self.ctx, opt, int(value)))

    def info(self):
        names = ["n", "ld", "elem", "kernel", "wgs_per_tour", "lds_bytes", "block", "symmetric", "cus", "depth", "matrix_free", "fused",
                 "nn_grid", "nn_grid_max_cell", "pipe2", "persist", "persist_wgs", "persist_edges", "persist_lds", "persist_window_cells",
                 "persist_window", "persist_handed", "persist_sweeps", "vns_mode", "stream_persist",
                 "otf_kernel", "ceil_int", "em_form", "em_stale", "em_steps", "or_batch_r", "or_single_r",
                 "or_block", "or_nch", "or_otf", "or_otf_R",
                 "multi_sweeps", "multi_moves", "multi_max_moves", "multi_r", "multi_block", "multi_nch",
                 "nl_k", "nl_sweeps", "nl_moves", "nl_polish_sweeps", "nl_nodes",
                 "or_nl_sweeps", "or_nl_moves", "or_nl_max_moves", "or_nl_rounds", "or_nl_starts",
                 "nl_batch_tours", "nl_batch_launches", "nl_batch_max_live", "nl_batch_wgs",
                 "vns_nl_walks", "vns_nl_iterations", "vns_nl_rounds", "vns_nl_max_live", "vns_nl_dry",
                 "persist_shaped",
                 "three_nl_w", "three_nl_sweeps", "three_nl_moves", "three_nl_max_moves", "three_nl_phases", "three_nl_nodes",
                 "persist_tmat", "persist_packed",
                 "dl_looked", "dl_full_sweeps", "dl_max_queue", "dl_max_wgs",
                 "greedy_rounds1", "greedy_rounds2", "greedy_edges1", "greedy_free",
                 "nl3_batch_w", "nl3_batch_sweeps", "nl3_batch_moves", "nl3_batch_max_moves",
                 "nlb_dl_looked", "nlb_dl_full_sweeps", "nlb_dl_max_queue", "nlb_dl_qsweep_wgs",
                 "hk_rounds", "hk_iterations", "hk_reason", "hk_h", "hk_nodes", "hk_lds"]
        return {k: int(self.L.tspgpu_info(self.ctx, i)) for i, k in enumerate(names)}

    # ---- instance
    def set_points(self, xy, kind=EUC_2D):
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1)
        self.n = len(xy) // 2
        self._ck(self.L.tspgpu_set_points(self.ctx, xy, self.n, kind))

    def build_costs(self, fetch=False):
        """tsp_compute_costs (src/tsp.c:608-636) on the device."""
        if fetch:
            out = np.empty((self.n, self.n), dtype=np.float64)
            self._ck(self.L.tspgpu_build_costs(self.ctx, out.ctypes.data))
            return out
        self._ck(self.L.tspgpu_build_costs(self.ctx, None))
        return None

    def set_costs(self, costs):
        costs = np.ascontiguousarray(costs, dtype=np.float64)
        assert costs.ndim == 2 and costs.shape[0] == costs.shape[1]
        self.n = costs.shape[0]
        self._ck(self.L.tspgpu_set_costs(self.ctx, costs.reshape(-1), self.n))

    def get_costs(self):
        out = np.empty((self.n, self.n), dtype=np.float64)
        self._ck(self.L.tspgpu_get_costs(self.ctx, out.reshape(-1)))
        return out

    # ---- single tour, host arrays
    def nn_tour(self, start):
        """h_greedyutil (heuristics.c:216-288) -> (succ, cost)."""
        path = np.empty(self.n, dtype=np.int32)
        cost = C.c_double()
        self._ck(self.L.tspgpu_nn_tour(self.ctx, int(start), path, C.byref(cost)))
        return path, cost.value

    def farthest_pair(self):
        """The EM_MAX start of h_ExtraMileage (heuristics.c:165-177) -> (a, b, cost)."""
        a, b, c = C.c_int(), C.c_int(), C.c_double()
        self._ck(self.L.tspgpu_farthest_pair(self.ctx, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def extra_mileage(self, a=None, b=None, time_left_s=-1.0):
        """h_extramileage_util (heuristics.c:290-367) from (a, b), by default the farthest pair -> (succ, cost, rc).
        rc is DEADLINE_EXCEEDED when the time ran out; succ is then None and cost None."""
        if a is None or b is None:
            a, b, _ = self.farthest_pair()
        path = np.empty(self.n, dtype=np.int32)
        cost = C.c_double()
        rc = self._ck(self.L.tspgpu_extra_mileage(self.ctx, int(a), int(b), float(time_left_s), path, C.byref(cost)),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        if rc != T_OK:
            return None, None, rc
        return path, cost.value, rc

    def two_opt_once(self, path, cost):
        """ref_2opt_once (refinment.c:39-93); path modified in place -> (delta, cost)."""
        c, d = C.c_double(cost), C.c_double()
        self._ck(self.L.tspgpu_two_opt_once(self.ctx, path, C.byref(c), C.byref(d)))
        return d.value, c.value

    def two_opt(self, path, time_left_s=-1.0):
        """ref_2opt (refinment.c:3-37); path in place -> (cost, sweeps, rc)."""
        c, s = C.c_double(), C.c_long()
        rc = self._ck(self.L.tspgpu_two_opt(self.ctx, path, C.byref(c), float(time_left_s), C.byref(s)),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return c.value, s.value, rc

    def or_opt_once(self, path, cost):
        """one Or-opt sweep (include/tspgpu.h "Or-opt"); path in place -> (delta, cost, (s, L, q, rev));
        delta 0 and (-1, -1, -1, -1) when nothing improves."""
        c, d = C.c_double(cost), C.c_double()
        mv = np.empty(4, dtype=np.int32)
        self._ck(self.L.tspgpu_or_opt_once(self.ctx, path, C.byref(c), C.byref(d), mv))
        return d.value, c.value, tuple(int(v) for v in mv)

    def or_opt(self, path, cost, time_left_s=-1.0):
        """Or-opt sweeps until none improves; path in place -> (cost, moves, rc)."""
        c, m = C.c_double(cost), C.c_long()
        rc = self._ck(self.L.tspgpu_or_opt(self.ctx, path, C.byref(c), float(time_left_s), C.byref(m)),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return c.value, m.value, rc

    def two_opt_multi_once(self, path, cost, cap=None):
        """one parallel-move 2-opt sweep (include/tspgpu.h "Parallel-move 2-opt"); path in place ->
        (cost, moves, deltas): moves an array [k][2] of a, b with P(a) < P(b) in ascending key order, deltas [k]
        (k = 0: nothing improves).  More than `cap` (default n) accepted moves: RESOURCE_EXHAUSTED, nothing applied."""
        cap = self.n if cap is None else int(cap)
        c, k = C.c_double(cost), C.c_int()
        mv = np.empty(2 * max(cap, 1), dtype=np.int32)
        dl = np.empty(max(cap, 1), dtype=np.float64)
        self._ck(self.L.tspgpu_two_opt_multi_once(self.ctx, path, C.byref(c), C.byref(k), mv, dl, cap))
        return c.value, mv[:2 * k.value].reshape(-1, 2).copy(), dl[:k.value].copy()

    def two_opt_multi(self, path, time_left_s=-1.0):
        """parallel-move 2-opt sweeps until one accepts nothing; path in place -> (cost, sweeps, moves, rc)."""
        c, s, m = C.c_double(), C.c_long(), C.c_long()
        rc = self._ck(self.L.tspgpu_two_opt_multi(self.ctx, path, C.byref(c), float(time_left_s), C.byref(s), C.byref(m)),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return c.value, s.value, m.value, rc

    def neighbours_build(self, K):
        """neighbour lists of K nodes (1..16; 0 drops them) for the cost source in place (include/tspgpu.h "Neighbour-list 2-opt")."""
        self._ck(self.L.tspgpu_neighbours_build(self.ctx, int(K)))

    def neighbours_get(self):
        """-> (nodes [n][K'], weights [n][K']) of the lists in place."""
        k = int(self.L.tspgpu_info(self.ctx, 42))
        nodes = np.empty((self.n, max(k, 1)), dtype=np.int32)
        w = np.empty((self.n, max(k, 1)), dtype=np.float64)
        self._ck(self.L.tspgpu_neighbours_get(self.ctx, nodes, w.ctypes.data))
        return nodes, w

    def two_opt_nl_once(self, path, cost, cap=None):
        """one neighbour-list 2-opt sweep; arguments and results as two_opt_multi_once."""
        cap = self.n if cap is None else int(cap)
        c, k = C.c_double(cost), C.c_int()
        mv = np.empty(2 * max(cap, 1), dtype=np.int32)
        dl = np.empty(max(cap, 1), dtype=np.float64)
        self._ck(self.L.tspgpu_two_opt_nl_once(self.ctx, path, C.byref(c), C.byref(k), mv, dl, cap))
        return c.value, mv[:2 * k.value].reshape(-1, 2).copy(), dl[:k.value].copy()

    def two_opt_nl(self, path, time_left_s=-1.0, polish=True):
        """neighbour-list 2-opt sweeps until one accepts nothing, then (polish) the parallel-move descent on the result;
        path in place -> dict(cost, sweeps, moves, polish_sweeps, polish_moves, rc)."""
        c, s, m, ps, pm = C.c_double(), C.c_long(), C.c_long(), C.c_long(), C.c_long()
        rc = self._ck(self.L.tspgpu_two_opt_nl(self.ctx, path, C.byref(c), float(time_left_s), 1 if polish else 0, C.byref(s), C.byref(m),
                                               C.byref(ps), C.byref(pm)), ok=(T_OK, DEADLINE_EXCEEDED))
        return {"cost": c.value, "sweeps": s.value, "moves": m.value, "polish_sweeps": ps.value, "polish_moves": pm.value, "rc": rc}

    def or_opt_nl_once(self, path, cost, cap=None):
        """one neighbour-list Or-opt sweep (include/tspgpu.h "Neighbour-list Or-opt"); path in place ->
        (cost, moves, deltas): moves an array [k][4] of s, L, q, rev in ascending key order, deltas [k] (k = 0: nothing
        improves).  More than `cap` (default n) accepted moves: RESOURCE_EXHAUSTED, nothing applied."""
        cap = self.n if cap is None else int(cap)
        c, k = C.c_double(cost), C.c_int()
        mv = np.empty(4 * max(cap, 1), dtype=np.int32)
        dl = np.empty(max(cap, 1), dtype=np.float64)
        self._ck(self.L.tspgpu_or_opt_nl_once(self.ctx, path, C.byref(c), C.byref(k), mv, dl, cap))
        return c.value, mv[:4 * k.value].reshape(-1, 4).copy(), dl[:k.value].copy()

    def or_opt_nl(self, path, cost, time_left_s=-1.0):
        """neighbour-list Or-opt sweeps until one accepts nothing; path in place -> (cost, sweeps, moves, rc)."""
        c, s, m = C.c_double(cost), C.c_long(), C.c_long()
        rc = self._ck(self.L.tspgpu_or_opt_nl(self.ctx, path, C.byref(c), float(time_left_s), C.byref(s), C.byref(m)),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return c.value, s.value, m.value, rc

    def local_search_nl(self, path, time_left_s=-1.0):
        """neighbour-list 2-opt and neighbour-list Or-opt in turn until an Or-opt phase applies nothing; path in place ->
        dict(cost, two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, rounds, rc)."""
        c, tw, tm, os_, om, nr = C.c_double(), C.c_long(), C.c_long(), C.c_long(), C.c_long(), C.c_int()
        rc = self._ck(self.L.tspgpu_local_search_nl(self.ctx, path, C.byref(c), float(time_left_s), C.byref(tw), C.byref(tm), C.byref(os_),
                                                    C.byref(om), C.byref(nr)), ok=(T_OK, DEADLINE_EXCEEDED))
        return {"cost": c.value, "two_opt_sweeps": tw.value, "two_opt_moves": tm.value, "or_sweeps": os_.value, "or_moves": om.value,
                "rounds": nr.value, "rc": rc}

    def three_opt_nl_once(self, path, cost, width, cap=None):
        """one neighbour-list 3-opt sweep over the first `width` list entries (include/tspgpu.h "Neighbour-list 3-opt"); path in
        place -> (cost, moves, deltas): moves an array [k][4] of i, j, k, kind in ascending key order, deltas [k] (k = 0: nothing
        improves).  More than `cap` (default n) accepted moves: RESOURCE_EXHAUSTED, nothing applied."""
        cap = self.n if cap is None else int(cap)
        c, k = C.c_double(cost), C.c_int()
        mv = np.empty(4 * max(cap, 1), dtype=np.int32)
        dl = np.empty(max(cap, 1), dtype=np.float64)
        self._ck(self.L.tspgpu_three_opt_nl_once(self.ctx, int(width), path, C.byref(c), C.byref(k), mv, dl, cap))
        return c.value, mv[:4 * k.value].reshape(-1, 4).copy(), dl[:k.value].copy()

    def three_opt_nl(self, path, cost, width, time_left_s=-1.0):
        """neighbour-list 3-opt sweeps until one accepts nothing; path in place -> (cost, sweeps, moves, rc)."""
        c, s, m = C.c_double(cost), C.c_long(), C.c_long()
        rc = self._ck(self.L.tspgpu_three_opt_nl(self.ctx, int(width), path, C.byref(c), float(time_left_s), C.byref(s), C.byref(m)),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return c.value, s.value, m.value, rc

    def local_search_nl3(self, path, width, time_left_s=-1.0):
        """the descent of local_search_nl and a neighbour-list 3-opt phase in turn until a 3-opt phase applies nothing; path in
        place -> dict(cost, two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, rounds, three_sweeps, three_moves, three_phases, rc)."""
        c, tw, tm, os_, om, nr = C.c_double(), C.c_long(), C.c_long(), C.c_long(), C.c_long(), C.c_int()
        ts, tv, tp = C.c_long(), C.c_long(), C.c_int()
        rc = self._ck(self.L.tspgpu_local_search_nl3(self.ctx, int(width), path, C.byref(c), float(time_left_s), C.byref(tw), C.byref(tm),
                                                     C.byref(os_), C.byref(om), C.byref(nr), C.byref(ts), C.byref(tv), C.byref(tp)),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return {"cost": c.value, "two_opt_sweeps": tw.value, "two_opt_moves": tm.value, "or_sweeps": os_.value, "or_moves": om.value,
                "rounds": nr.value, "three_sweeps": ts.value, "three_moves": tv.value, "three_phases": tp.value, "rc": rc}

    def local_search(self, path, time_left_s=-1.0):
        """2-opt and Or-opt in turn until neither improves; path in place ->
        dict(cost, two_opt_sweeps, or_moves, rounds, rc)."""
        c, sw, om, nr = C.c_double(), C.c_long(), C.c_long(), C.c_int()
        rc = self._ck(self.L.tspgpu_local_search(self.ctx, path, C.byref(c), float(time_left_s), C.byref(sw), C.byref(om), C.byref(nr)),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return {"cost": c.value, "two_opt_sweeps": sw.value, "or_moves": om.value, "rounds": nr.value, "rc": rc}

    def tabu_move(self, path, cost, tabu_list, tenure, it):
        """tabu_best_move (metaheuristic.c:188-245); path and tabu_list in place -> cost."""
        c = C.c_double(cost)
        self._ck(self.L.tspgpu_tabu_move(self.ctx, path, C.byref(c), tabu_list, int(tenure), int(it)))
        return c.value

    def tabu_search(self, path, cost, k, want_trace=False):
        """mh_TabuSearch's loop (metaheuristic.c:115-166) -> (best_path, best_cost, final_cost, trace)."""
        c, bc = C.c_double(cost), C.c_double()
        best = np.empty(self.n, dtype=np.int32)
        trace = np.empty(max(k, 1), dtype=np.float64) if want_trace else None
        self._ck(self.L.tspgpu_tabu_search(self.ctx, path, C.byref(c), int(k), best, C.byref(bc),
                                           trace.ctypes.data if want_trace else None))
        return best, bc.value, c.value, (trace[:k] if want_trace else None)

    def vns_search(self, path, k, rand_values, best_path, best_cost, iterations=0, kick_pending=0, time_left_s=-1.0, want_trace=False):
        """mh_VNS's loop (metaheuristic.c:279-318); path and best_path in place ->
        dict(rc, cost, best_cost, iterations, kick_pending, consumed, trace)."""
        rv = np.ascontiguousarray(rand_values, dtype=np.int32)
        c, bc = C.c_double(), C.c_double(best_cost)
        used, it, kp = C.c_long(), C.c_int(iterations), C.c_int(kick_pending)
        trace = np.full(max(k - iterations, 1), np.nan, dtype=np.float64) if want_trace else None
        rc = self._ck(self.L.tspgpu_vns_search(self.ctx, path, C.byref(c), int(k), float(time_left_s), rv, len(rv), C.byref(used),
                                               C.byref(it), C.byref(kp), best_path, C.byref(bc), trace.ctypes.data if want_trace else None),
                      ok=(T_OK, DEADLINE_EXCEEDED, 8))
        return {"rc": rc, "cost": c.value, "best_cost": bc.value, "iterations": it.value, "kick_pending": kp.value,
                "consumed": used.value, "trace": trace}

    def _vns_walks(self, fn, head, names, paths, k, rand_values, best_paths, best_costs, iterations, kick_pending, time_left_s, want_trace):
        W = paths.shape[0]
        assert paths.dtype == np.int32 and best_paths.dtype == np.int32 and best_costs.dtype == np.float64
        assert paths.flags.c_contiguous and best_paths.flags.c_contiguous and best_costs.flags.c_contiguous
        assert paths.shape == best_paths.shape == (W, self.n) and best_costs.shape == (W,)
        rv = np.ascontiguousarray(rand_values, dtype=np.int32).reshape(W, -1)
        it = np.zeros(W, dtype=np.int32) if iterations is None else np.array(iterations, dtype=np.int32)
        kp = np.zeros(W, dtype=np.int32) if kick_pending is None else np.array(kick_pending, dtype=np.int32)
        costs = np.zeros(W, dtype=np.float64)
        used = np.zeros(W, dtype=np.int64)
        totals = np.zeros((W, len(names)), dtype=np.int64)
        trace = np.full((W, max(int(k), 1)), np.nan, dtype=np.float64) if want_trace else None
        rc = self._ck(fn(self.ctx, *head, W, int(k), float(time_left_s), paths.reshape(-1), costs, rv.ctypes.data, rv.shape[1],
                         used.ctypes.data, it, kp, best_paths.reshape(-1), best_costs,
                         trace.ctypes.data if want_trace else None, totals.ctypes.data),
                      ok=(T_OK, DEADLINE_EXCEEDED, 8))
        return {"rc": rc, "costs": costs, "best_costs": best_costs, "iterations": it, "kick_pending": kp, "consumed": used,
                "trace": trace[:, :int(k)] if want_trace else None, "totals": {nm: totals[:, i].copy() for i, nm in enumerate(names)}}

    def vns_walks_nl(self, paths, k, rand_values, best_paths, best_costs, iterations=None, kick_pending=None, time_left_s=-1.0,
                     want_trace=False):
        """W walks of the neighbour-list VNS (include/tspgpu.h "Neighbour-list VNS").  paths, best_paths [W][n] int32 and
        best_costs [W] float64 in place; rand_values [W][nrand]; iterations, kick_pending [W] (default: zeros) are copied ->
        dict(rc, costs, best_costs, iterations, kick_pending, consumed, trace [W][k] (NaN: not written by this call) or None,
        totals: dict of [W] arrays two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, rounds, kicks)."""
        names = ("two_opt_sweeps", "two_opt_moves", "or_sweeps", "or_moves", "rounds", "kicks")
        return self._vns_walks(self.L.tspgpu_vns_walks_nl, (), names, paths, k, rand_values, best_paths, best_costs, iterations, kick_pending,
                               time_left_s, want_trace)

    def vns_walks_nl3(self, paths, k, rand_values, best_paths, best_costs, width, iterations=None, kick_pending=None, time_left_s=-1.0,
                      want_trace=False):
        """vns_walks_nl with the descent of local_search_nl3 at `width` (include/tspgpu.h "Batched neighbour-list 3-opt"); totals
        gains three_sweeps, three_moves, three_phases."""
        names = ("two_opt_sweeps", "two_opt_moves", "or_sweeps", "or_moves", "rounds", "kicks", "three_sweeps", "three_moves", "three_phases")
        return self._vns_walks(self.L.tspgpu_vns_walks_nl3, (int(width),), names, paths, k, rand_values, best_paths, best_costs, iterations,
                               kick_pending, time_left_s, want_trace)

    # ---- multi-start
    @staticmethod
    def _starts(starts, n):
        if starts is None:
            return None, n, None
        a = np.ascontiguousarray(starts, dtype=np.int32)
        return a.ctypes.data, len(a), a

    def nn_all(self, starts=None):
        """h_Greedy_iterative (heuristics.c:34-72) -> (best_path, best_cost, best_start)."""
        p, m, keep = self._starts(starts, self.n)
        best = np.empty(self.n, dtype=np.int32)
        c, s = C.c_double(), C.c_int()
        self._ck(self.L.tspgpu_nn_all(self.ctx, p, m, best, C.byref(c), C.byref(s)))
        return best, c.value, s.value

    def nn_all_timed(self, starts=None, time_left_s=-1.0):
        """h_Greedy_iterative under its deadline -> (best_path, best_cost, best_start, done_starts, rc)."""
        p, m, keep = self._starts(starts, self.n)
        best = np.empty(self.n, dtype=np.int32)
        c, s, d = C.c_double(), C.c_int(), C.c_int()
        rc = self._ck(self.L.tspgpu_nn_all_timed(self.ctx, p, m, float(time_left_s), best, C.byref(c), C.byref(s), C.byref(d)),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return best, c.value, s.value, d.value, rc

    def multistart_nn_2opt(self, starts=None, time_left_s=-1.0, want_last=False):
        """h_greedy_2opt (heuristics.c:74-116) -> dict."""
        p, m, keep = self._starts(starts, self.n)
        best = np.empty(self.n, dtype=np.int32)
        c, s, sw = C.c_double(), C.c_int(), C.c_long()
        last = np.empty(self.n, dtype=np.int32) if want_last else None
        lc = C.c_double()
        rc = self._ck(self.L.tspgpu_multistart_nn_2opt(
            self.ctx, p, m, float(time_left_s), best, C.byref(c), C.byref(s), C.byref(sw),
            last.ctypes.data if want_last else None, C.addressof(lc) if want_last else None),
            ok=(T_OK, DEADLINE_EXCEEDED))
        return {"path": best, "cost": c.value, "start": s.value, "sweeps": sw.value, "rc": rc,
                "last_path": last, "last_cost": lc.value if want_last else None}

    def multistart_local_search(self, starts=None, time_left_s=-1.0):
        """NN + the 2-opt + Or-opt descent from every start, batched ->
        dict(path, cost, start, two_opt_sweeps, or_moves, costs, rc); costs[i] is the final cost of list entry i."""
        p, m, keep = self._starts(starts, self.n)
        best = np.empty(self.n, dtype=np.int32)
        c, s, sw, om = C.c_double(), C.c_int(), C.c_long(), C.c_long()
        costs = np.full(m, np.nan, dtype=np.float64)
        rc = self._ck(self.L.tspgpu_multistart_local_search(self.ctx, p, m, float(time_left_s), best, C.byref(c), C.byref(s),
                                                            C.byref(sw), C.byref(om), costs.ctypes.data),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return {"path": best, "cost": c.value, "start": s.value, "two_opt_sweeps": sw.value, "or_moves": om.value,
                "costs": costs, "rc": rc}

    def multistart_local_search_nl(self, starts=None, time_left_s=-1.0):
        """NN + the descent over the neighbour lists from every start, batched (neighbours_build first) ->
        dict(path, cost, start, two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, costs, rc); costs[i] is the final cost of list entry i."""
        p, m, keep = self._starts(starts, self.n)
        best = np.empty(self.n, dtype=np.int32)
        c, s = C.c_double(), C.c_int()
        tw, tm, os_, om = C.c_long(), C.c_long(), C.c_long(), C.c_long()
        costs = np.full(m, np.nan, dtype=np.float64)
        rc = self._ck(self.L.tspgpu_multistart_local_search_nl(self.ctx, p, m, float(time_left_s), best, C.byref(c), C.byref(s),
                                                               C.byref(tw), C.byref(tm), C.byref(os_), C.byref(om), costs.ctypes.data),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return {"path": best, "cost": c.value, "start": s.value, "two_opt_sweeps": tw.value, "two_opt_moves": tm.value,
                "or_sweeps": os_.value, "or_moves": om.value, "costs": costs, "rc": rc}

    def multistart_local_search_nl3(self, width, starts=None, time_left_s=-1.0):
        """multistart_local_search_nl with the 3-opt phase at `width` -> its dict with three_sweeps, three_moves added."""
        p, m, keep = self._starts(starts, self.n)
        best = np.empty(self.n, dtype=np.int32)
        c, s = C.c_double(), C.c_int()
        tw, tm, os_, om, ts, tv = (C.c_long() for _ in range(6))
        costs = np.full(m, np.nan, dtype=np.float64)
        rc = self._ck(self.L.tspgpu_multistart_local_search_nl3(self.ctx, int(width), p, m, float(time_left_s), best, C.byref(c), C.byref(s),
                                                                C.byref(tw), C.byref(tm), C.byref(os_), C.byref(om), C.byref(ts), C.byref(tv),
                                                                costs.ctypes.data),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return {"path": best, "cost": c.value, "start": s.value, "two_opt_sweeps": tw.value, "two_opt_moves": tm.value,
                "or_sweeps": os_.value, "or_moves": om.value, "three_sweeps": ts.value, "three_moves": tv.value, "costs": costs, "rc": rc}

    # ---- device-resident
    def tour_load(self, slot, path):
        self._ck(self.L.tspgpu_tour_load(self.ctx, slot, np.ascontiguousarray(path, np.int32)))

    def tour_nn(self, slot, start):
        self._ck(self.L.tspgpu_tour_nn(self.ctx, slot, int(start)))

    def tour_copy(self, dst, src):
        self._ck(self.L.tspgpu_tour_copy(self.ctx, dst, src))

    def tour_two_opt(self, slot, max_sweeps=-1, time_left_s=-1.0):
        s = C.c_long()
        rc = self._ck(self.L.tspgpu_tour_two_opt(self.ctx, slot, int(max_sweeps), float(time_left_s), C.byref(s)),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return s.value, rc

    def tour_or_opt(self, slot, max_moves=-1, time_left_s=-1.0):
        """Or-opt moves on a slot -> (moves, rc)."""
        m = C.c_long()
        rc = self._ck(self.L.tspgpu_tour_or_opt(self.ctx, int(slot), int(max_moves), float(time_left_s), C.byref(m)),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return m.value, rc

    def tour_local_search(self, slot, time_left_s=-1.0):
        """the descent of local_search on a slot -> dict(two_opt_sweeps, or_moves, rounds, rc)."""
        sw, om, nr = C.c_long(), C.c_long(), C.c_int()
        rc = self._ck(self.L.tspgpu_tour_local_search(self.ctx, int(slot), float(time_left_s), C.byref(sw), C.byref(om), C.byref(nr)),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return {"two_opt_sweeps": sw.value, "or_moves": om.value, "rounds": nr.value, "rc": rc}

    def tours_local_search(self, slot0, count, time_left_s=-1.0):
        """the descent of tour_local_search on slots slot0 .. slot0+count-1 at once ->
        dict(two_opt_sweeps, or_moves, rounds: arrays of count entries, rc)."""
        count = int(count)
        sw, om = np.zeros(max(count, 0), dtype=np.int64), np.zeros(max(count, 0), dtype=np.int64)
        nr = np.zeros(max(count, 0), dtype=np.int32)
        rc = self._ck(self.L.tspgpu_tours_local_search(self.ctx, int(slot0), count, float(time_left_s),
                                                       sw.ctypes.data, om.ctypes.data, nr.ctypes.data),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return {"two_opt_sweeps": sw, "or_moves": om, "rounds": nr, "rc": rc}

    def tour_two_opt_multi(self, slot, max_sweeps=-1, time_left_s=-1.0):
        """parallel-move 2-opt sweeps on a slot -> (sweeps, moves, rc)."""
        s, m = C.c_long(), C.c_long()
        rc = self._ck(self.L.tspgpu_tour_two_opt_multi(self.ctx, int(slot), int(max_sweeps), float(time_left_s), C.byref(s), C.byref(m)),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return s.value, m.value, rc

    def tour_two_opt_nl(self, slot, max_sweeps=-1, time_left_s=-1.0):
        """neighbour-list 2-opt sweeps on a slot -> (sweeps, moves, rc)."""
        s, m = C.c_long(), C.c_long()
        rc = self._ck(self.L.tspgpu_tour_two_opt_nl(self.ctx, int(slot), int(max_sweeps), float(time_left_s), C.byref(s), C.byref(m)),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return s.value, m.value, rc

    def tour_or_opt_nl(self, slot, max_sweeps=-1, time_left_s=-1.0):
        """neighbour-list Or-opt sweeps on a slot -> (sweeps, moves, rc)."""
        s, m = C.c_long(), C.c_long()
        rc = self._ck(self.L.tspgpu_tour_or_opt_nl(self.ctx, int(slot), int(max_sweeps), float(time_left_s), C.byref(s), C.byref(m)),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return s.value, m.value, rc

    def tour_local_search_nl(self, slot, time_left_s=-1.0):
        """the descent of local_search_nl on a slot -> dict(two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, rounds, rc)."""
        tw, tm, os_, om, nr = C.c_long(), C.c_long(), C.c_long(), C.c_long(), C.c_int()
        rc = self._ck(self.L.tspgpu_tour_local_search_nl(self.ctx, int(slot), float(time_left_s), C.byref(tw), C.byref(tm), C.byref(os_),
                                                         C.byref(om), C.byref(nr)), ok=(T_OK, DEADLINE_EXCEEDED))
        return {"two_opt_sweeps": tw.value, "two_opt_moves": tm.value, "or_sweeps": os_.value, "or_moves": om.value, "rounds": nr.value,
                "rc": rc}

    def tours_local_search_nl(self, slot0, count, time_left_s=-1.0):
        """the descent of tour_local_search_nl on slots slot0 .. slot0+count-1 at once ->
        dict(two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, rounds: arrays of count entries, rc)."""
        count = int(count)
        tw, tm, os_, om = (np.zeros(max(count, 0), dtype=np.int64) for _ in range(4))
        nr = np.zeros(max(count, 0), dtype=np.int32)
        rc = self._ck(self.L.tspgpu_tours_local_search_nl(self.ctx, int(slot0), count, float(time_left_s), tw.ctypes.data, tm.ctypes.data,
                                                          os_.ctypes.data, om.ctypes.data, nr.ctypes.data),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return {"two_opt_sweeps": tw, "two_opt_moves": tm, "or_sweeps": os_, "or_moves": om, "rounds": nr, "rc": rc}

    def tours_local_search_nl3(self, slot0, count, width, time_left_s=-1.0):
        """the descent of tour_local_search_nl3 on slots slot0 .. slot0+count-1 at once ->
        dict(two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, rounds, three_sweeps, three_moves, three_phases: arrays of count
        entries, rc)."""
        count = int(count)
        tw, tm, os_, om, ts, tv = (np.zeros(max(count, 0), dtype=np.int64) for _ in range(6))
        nr, tp = (np.zeros(max(count, 0), dtype=np.int32) for _ in range(2))
        rc = self._ck(self.L.tspgpu_tours_local_search_nl3(self.ctx, int(slot0), count, int(width), float(time_left_s), tw.ctypes.data,
                                                           tm.ctypes.data, os_.ctypes.data, om.ctypes.data, nr.ctypes.data, ts.ctypes.data,
                                                           tv.ctypes.data, tp.ctypes.data),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return {"two_opt_sweeps": tw, "two_opt_moves": tm, "or_sweeps": os_, "or_moves": om, "rounds": nr,
                "three_sweeps": ts, "three_moves": tv, "three_phases": tp, "rc": rc}

    def tour_three_opt_nl(self, slot, width, max_sweeps=-1, time_left_s=-1.0):
        """neighbour-list 3-opt sweeps on a slot -> (sweeps, moves, rc)."""
        s, m = C.c_long(), C.c_long()
        rc = self._ck(self.L.tspgpu_tour_three_opt_nl(self.ctx, int(slot), int(width), int(max_sweeps), float(time_left_s), C.byref(s),
                                                      C.byref(m)), ok=(T_OK, DEADLINE_EXCEEDED))
        return s.value, m.value, rc

    def tour_local_search_nl3(self, slot, width, time_left_s=-1.0):
        """the descent of local_search_nl3 on a slot -> dict(two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, rounds,
        three_sweeps, three_moves, three_phases, rc)."""
        tw, tm, os_, om, nr = C.c_long(), C.c_long(), C.c_long(), C.c_long(), C.c_int()
        ts, tv, tp = C.c_long(), C.c_long(), C.c_int()
        rc = self._ck(self.L.tspgpu_tour_local_search_nl3(self.ctx, int(slot), int(width), float(time_left_s), C.byref(tw), C.byref(tm),
                                                          C.byref(os_), C.byref(om), C.byref(nr), C.byref(ts), C.byref(tv), C.byref(tp)),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return {"two_opt_sweeps": tw.value, "two_opt_moves": tm.value, "or_sweeps": os_.value, "or_moves": om.value, "rounds": nr.value,
                "three_sweeps": ts.value, "three_moves": tv.value, "three_phases": tp.value, "rc": rc}

    # ---- don't-look bits (include/tspgpu.h "Don't-look bits")
    def tour_wake(self, slot, nodes=None):
        """nodes join the slot's three awake sets; None: every node wakes."""
        if nodes is None:
            self._ck(self.L.tspgpu_tour_wake(self.ctx, int(slot), None, -1))
            return
        a = np.ascontiguousarray(nodes, dtype=np.int32)
        self._ck(self.L.tspgpu_tour_wake(self.ctx, int(slot), a.ctypes.data, len(a)))

    def tour_sleep(self, slot):
        self._ck(self.L.tspgpu_tour_sleep(self.ctx, int(slot)))

    def tour_awake(self, slot, family):
        """the awake set of family 0 (2-opt), 1 (Or-opt) or 2 (3-opt) -> uint8 [n]."""
        out, cnt = np.empty(self.n, dtype=np.uint8), C.c_int()
        self._ck(self.L.tspgpu_tour_awake(self.ctx, int(slot), int(family), out.ctypes.data, C.byref(cnt)))
        assert cnt.value == int(out.sum())
        return out

    def tour_kick(self, slot, i, j, k):
        """the segment swap at the edge positions i < j < k, whatever its delta."""
        self._ck(self.L.tspgpu_tour_kick(self.ctx, int(slot), int(i), int(j), int(k)))

    def _tour_dl(self, fn, slot, head, closing, max_sweeps, time_left_s):
        s, m, q = C.c_long(), C.c_long(), C.c_long()
        rc = self._ck(fn(self.ctx, int(slot), *head, int(closing), int(max_sweeps), float(time_left_s), C.byref(s), C.byref(m), C.byref(q)),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return s.value, m.value, q.value, rc

    def tour_two_opt_nl_dl(self, slot, closing=1, max_sweeps=-1, time_left_s=-1.0):
        """the neighbour-list 2-opt phase with looks on a slot -> (sweeps, moves, looked, rc)."""
        return self._tour_dl(self.L.tspgpu_tour_two_opt_nl_dl, slot, (), closing, max_sweeps, time_left_s)

    def tour_or_opt_nl_dl(self, slot, closing=1, max_sweeps=-1, time_left_s=-1.0):
        return self._tour_dl(self.L.tspgpu_tour_or_opt_nl_dl, slot, (), closing, max_sweeps, time_left_s)

    def tour_three_opt_nl_dl(self, slot, width, closing=1, max_sweeps=-1, time_left_s=-1.0):
        return self._tour_dl(self.L.tspgpu_tour_three_opt_nl_dl, slot, (int(width),), closing, max_sweeps, time_left_s)

    def _descent_dl(self, call):
        tw, tm, os_, om, nr = C.c_long(), C.c_long(), C.c_long(), C.c_long(), C.c_int()
        ts, tv, tp, lk, fs = C.c_long(), C.c_long(), C.c_int(), C.c_long(), C.c_long()
        rc = self._ck(call(C.byref(tw), C.byref(tm), C.byref(os_), C.byref(om), C.byref(nr), C.byref(ts), C.byref(tv), C.byref(tp),
                           C.byref(lk), C.byref(fs)), ok=(T_OK, DEADLINE_EXCEEDED))
        return {"two_opt_sweeps": tw.value, "two_opt_moves": tm.value, "or_sweeps": os_.value, "or_moves": om.value, "rounds": nr.value,
                "three_sweeps": ts.value, "three_moves": tv.value, "three_phases": tp.value, "looked": lk.value, "full_sweeps": fs.value,
                "rc": rc}

    def tour_local_search_nl3_dl(self, slot, width, closing=1, time_left_s=-1.0):
        """the descent over the lists with looks on a slot (width 0: no 3-opt phase) -> dict(the counters of
        tour_local_search_nl3, looked, full_sweeps, rc)."""
        return self._descent_dl(lambda *out: self.L.tspgpu_tour_local_search_nl3_dl(self.ctx, int(slot), int(width), int(closing),
                                                                                    float(time_left_s), *out))

    def local_search_nl3_dl(self, path, width, closing=1, time_left_s=-1.0):
        """the same on a host tour, path in place -> the dict with cost."""
        c = C.c_double()
        r = self._descent_dl(lambda *out: self.L.tspgpu_local_search_nl3_dl(self.ctx, int(width), int(closing), path, C.byref(c),
                                                                            float(time_left_s), *out))
        r["cost"] = c.value
        return r

    # ---- batched don't-look bits (include/tspgpu.h "Batched don't-look bits")
    def tours_local_search_nl3_dl(self, slot0, count, width, closing=0, time_left_s=-1.0):
        """tour_local_search_nl3_dl on slots slot0 .. slot0+count-1 at once, from their sets as they stand ->
        dict(the counters of tours_local_search_nl3, looked, full_sweeps: arrays of count entries, rc)."""
        count = int(count)
        tw, tm, os_, om, ts, tv, lk, fs = (np.zeros(max(count, 0), dtype=np.int64) for _ in range(8))
        nr, tp = (np.zeros(max(count, 0), dtype=np.int32) for _ in range(2))
        rc = self._ck(self.L.tspgpu_tours_local_search_nl3_dl(self.ctx, int(slot0), count, int(width), int(closing), float(time_left_s),
                                                              tw.ctypes.data, tm.ctypes.data, os_.ctypes.data, om.ctypes.data, nr.ctypes.data,
                                                              ts.ctypes.data, tv.ctypes.data, tp.ctypes.data, lk.ctypes.data, fs.ctypes.data),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return {"two_opt_sweeps": tw, "two_opt_moves": tm, "or_sweeps": os_, "or_moves": om, "rounds": nr,
                "three_sweeps": ts, "three_moves": tv, "three_phases": tp, "looked": lk, "full_sweeps": fs, "rc": rc}

    def multistart_local_search_nl3_dl(self, width, closing=0, starts=None, time_left_s=-1.0):
        """multistart_local_search_nl3 with the descent with looks (every start all awake) -> its dict with looked, full_sweeps added."""
        p, m, keep = self._starts(starts, self.n)
        best = np.empty(self.n, dtype=np.int32)
        c, s = C.c_double(), C.c_int()
        tw, tm, os_, om, ts, tv, lk, fs = (C.c_long() for _ in range(8))
        costs = np.full(m, np.nan, dtype=np.float64)
        rc = self._ck(self.L.tspgpu_multistart_local_search_nl3_dl(self.ctx, int(width), int(closing), p, m, float(time_left_s), best,
                                                                   C.byref(c), C.byref(s), C.byref(tw), C.byref(tm), C.byref(os_), C.byref(om),
                                                                   C.byref(ts), C.byref(tv), C.byref(lk), C.byref(fs), costs.ctypes.data),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return {"path": best, "cost": c.value, "start": s.value, "two_opt_sweeps": tw.value, "two_opt_moves": tm.value,
                "or_sweeps": os_.value, "or_moves": om.value, "three_sweeps": ts.value, "three_moves": tv.value,
                "looked": lk.value, "full_sweeps": fs.value, "costs": costs, "rc": rc}

    def vns_walks_nl3_dl(self, paths, k, rand_values, best_paths, best_costs, width, closing=0, iterations=None, kick_pending=None,
                         time_left_s=-1.0, want_trace=False):
        """vns_walks_nl3 with the descent with looks: behind a kick phase only the nodes whose tour neighbours changed are awake;
        totals gains looked, full_sweeps."""
        names = ("two_opt_sweeps", "two_opt_moves", "or_sweeps", "or_moves", "rounds", "kicks", "three_sweeps", "three_moves", "three_phases",
                 "looked", "full_sweeps")
        return self._vns_walks(self.L.tspgpu_vns_walks_nl3_dl, (int(width), int(closing)), names, paths, k, rand_values, best_paths,
                               best_costs, iterations, kick_pending, time_left_s, want_trace)

    # ---- greedy-edge construction (include/tspgpu.h "Greedy-edge construction")
    def tour_greedy(self, slot):
        """the greedy-edge tour over the neighbour lists into a slot, as tour_nn."""
        self._ck(self.L.tspgpu_tour_greedy(self.ctx, int(slot)))

    def greedy_tour(self):
        """the same into host arrays -> (path, cost)."""
        path, c = np.empty(self.n, dtype=np.int32), C.c_double()
        self._ck(self.L.tspgpu_greedy_tour(self.ctx, path, C.byref(c)))
        return path, c.value

    # ---- Held-Karp lower bound (include/tspgpu.h "Held-Karp lower bound")
    def _pi_arg(self, pi):
        if pi is None:
            return None, None
        pi = np.ascontiguousarray(pi, dtype=np.int64)
        if pi.shape != (self.n,):
            raise ValueError("pi must hold n multipliers")
        return pi, pi.ctypes.data

    def one_tree(self, pi=None):
        """the 1-tree T(pi) -> (L in units of 1/128, edges [n][2] ascending by pair, degree [n])."""
        keep, pp = self._pi_arg(pi)
        edges, deg, w = np.empty((self.n, 2), dtype=np.int32), np.empty(self.n, dtype=np.int32), C.c_long()
        self._ck(self.L.tspgpu_one_tree(self.ctx, pp, edges.ctypes.data, deg.ctypes.data, C.byref(w)))
        return w.value, edges, deg

    def lower_bound(self, upper=None, iters=300, patience=10, pi=None, time_left_s=-1.0):
        """the subgradient ascent over 1-trees -> LowerBound; upper=None takes the cost of nn_tour(0)."""
        if upper is None:
            upper = self.nn_tour(0)[1]
        keep, pp = self._pi_arg(pi)
        out, path = np.zeros(self.n, dtype=np.int64), np.full(self.n, -1, dtype=np.int32)
        bound, it, why = C.c_double(), C.c_int(), C.c_int()
        rc = self._ck(self.L.tspgpu_lower_bound(self.ctx, float(upper), int(iters), int(patience), float(time_left_s), pp, C.byref(bound),
                                                out.ctypes.data, path.ctypes.data, C.byref(it), C.byref(why)), ok=(T_OK, DEADLINE_EXCEEDED))
        return LowerBound(bound.value, out, it.value, why.value, path if why.value == 1 else None, float(upper), rc)

    def time_three_nl_sweep(self, slot, width, reps):
        ms = C.c_float()
        self._ck(self.L.tspgpu_time_three_nl_sweep(self.ctx, int(slot), int(width), int(reps), C.byref(ms)))
        return ms.value

    def time_or_nl_sweep(self, slot, reps):
        ms = C.c_float()
        self._ck(self.L.tspgpu_time_or_nl_sweep(self.ctx, slot, reps, C.byref(ms)))
        return ms.value

    def time_nl_sweep(self, slot, reps):
        ms = C.c_float()
        self._ck(self.L.tspgpu_time_nl_sweep(self.ctx, slot, reps, C.byref(ms)))
        return ms.value

    def time_multi_sweep(self, slot, reps):
        ms = C.c_float()
        self._ck(self.L.tspgpu_time_multi_sweep(self.ctx, slot, reps, C.byref(ms)))
        return ms.value

    def time_or_sweep(self, slot, reps):
        ms = C.c_float()
        self._ck(self.L.tspgpu_time_or_sweep(self.ctx, slot, reps, C.byref(ms)))
        return ms.value

    def tour_sweep_part(self, slot, part, nparts):
        """one sweep's runs [part*G/nparts, (part+1)*G/nparts) -> (delta, a, b); (0, 0, 0): nothing improving there"""
        d, a, b = C.c_double(), C.c_int(), C.c_int()
        self._ck(self.L.tspgpu_tour_sweep_part(self.ctx, int(slot), int(part), int(nparts), C.byref(d), C.byref(a), C.byref(b)))
        return d.value, a.value, b.value

    def tour_apply_move(self, slot, a, b, delta):
        """apply the agreed move (delta >= 0: none -- the slot is locally optimal)"""
        self._ck(self.L.tspgpu_tour_apply_move(self.ctx, int(slot), int(a), int(b), float(delta)))

    def tour_store(self, slot, want_path=True):
        path = np.empty(self.n, dtype=np.int32) if want_path else None
        c, d = C.c_double(), C.c_double()
        self._ck(self.L.tspgpu_tour_store(self.ctx, slot, path.ctypes.data if want_path else None,
                                          C.byref(c), C.byref(d)))
        return path, c.value, d.value

    def time_sweep(self, slot, reps):
        ms = C.c_float()
        self._ck(self.L.tspgpu_time_sweep(self.ctx, slot, reps, C.byref(ms)))
        return ms.value

    def time_build(self, reps):
        ms = C.c_float()
        self._ck(self.L.tspgpu_time_build(self.ctx, reps, C.byref(ms)))
        return ms.value

    def timing_read(self, reset=True):
        ms, cnt = C.c_double(), C.c_long()
        self._ck(self.L.tspgpu_timing_read(self.ctx, C.byref(ms), C.byref(cnt), 1 if reset else 0))
        return ms.value, cnt.value

    def history(self, capacity):
        a = np.empty(capacity, dtype=np.int32)
        b = np.empty(capacity, dtype=np.int32)
        d = np.empty(capacity, dtype=np.float64)
        m = C.c_int()
        self._ck(self.L.tspgpu_history(self.ctx, a, b, d, capacity, C.byref(m)))
        return a[:m.value], b[:m.value], d[:m.value]


class MultiEngine:
    """Python handle on one tspgpu_multi (several MI355X driven by one process, include/tspgpu.h
    "multi-device"): start list sharded over the devices, ONE RCCL MIN all-reduce + ONE broadcast per call."""

    def __init__(self, devices):
        self.L = _lib.load()
        self.m = C.c_void_p()
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        rc = self.L.tspgpu_multi_create(dev, len(dev), C.byref(self.m))
        if rc != T_OK:
            raise TspGpuError(rc, f"tspgpu_multi_create{tuple(int(d) for d in dev)} failed")
        self.n = 0

    def close(self):
        if self.m:
            self.L.tspgpu_multi_destroy(self.m)
            self.m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, ok=(T_OK,)):
        if rc not in ok:
            raise TspGpuError(rc, self.L.tspgpu_multi_last_error(self.m).decode())
        return rc

    def set_option(self, opt, value):
        self._ck(self.L.tspgpu_multi_set_option(self.m, opt, int(value)))

    def info(self):
        names = ["devices", "exchange_next", "exchange_last", "rccl_init_s", "exchange_s", "solve_s", "exchanges", "distinct"]
        return {k: self.L.tspgpu_multi_info(self.m, i) for i, k in enumerate(names)}

    def device_info(self, i):
        ctx = self.L.tspgpu_multi_ctx(self.m, i)
        names = ["n", "ld", "elem", "kernel", "wgs_per_tour", "lds_bytes", "block", "symmetric", "cus", "depth", "matrix_free", "fused"]
        return {k: int(self.L.tspgpu_info(ctx, j)) for j, k in enumerate(names)}

    def set_points(self, xy, kind=EUC_2D):
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1)
        self.n = len(xy) // 2
        self._ck(self.L.tspgpu_multi_set_points(self.m, xy, self.n, kind))

    def build_costs(self):
        self._ck(self.L.tspgpu_multi_build_costs(self.m))

    def prepare(self):
        """create the RCCL communicator ahead of the first exchange (outside any timed region)"""
        self._ck(self.L.tspgpu_multi_prepare(self.m))

    def multistart_nn_2opt(self, starts=None, time_left_s=-1.0):
        """h_greedy_2opt (heuristics.c:74-116) over every device -> dict."""
        p, m, keep = Engine._starts(starts, self.n)
        best = np.empty(self.n, dtype=np.int32)
        c, s, sw = C.c_double(), C.c_int(), C.c_long()
        rc = self._ck(self.L.tspgpu_multi_multistart_nn_2opt(self.m, p, m, float(time_left_s), best, C.byref(c), C.byref(s), C.byref(sw)),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return {"path": best, "cost": c.value, "start": s.value, "sweeps": sw.value, "rc": rc}

    def multistart_local_search(self, starts=None, time_left_s=-1.0):
        """Engine.multistart_local_search over every device -> dict(path, cost, start, two_opt_sweeps, or_moves, rc)."""
        p, m, keep = Engine._starts(starts, self.n)
        best = np.empty(self.n, dtype=np.int32)
        c, s, sw, om = C.c_double(), C.c_int(), C.c_long(), C.c_long()
        rc = self._ck(self.L.tspgpu_multi_multistart_local_search(self.m, p, m, float(time_left_s), best, C.byref(c), C.byref(s),
                                                                  C.byref(sw), C.byref(om)),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return {"path": best, "cost": c.value, "start": s.value, "two_opt_sweeps": sw.value, "or_moves": om.value, "rc": rc}

    def neighbours_build(self, K):
        """Engine.neighbours_build on every device's context"""
        self._ck(self.L.tspgpu_multi_neighbours_build(self.m, int(K)))

    def multistart_local_search_nl(self, starts=None, time_left_s=-1.0):
        """Engine.multistart_local_search_nl over every device ->
        dict(path, cost, start, two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, rc)."""
        p, m, keep = Engine._starts(starts, self.n)
        best = np.empty(self.n, dtype=np.int32)
        c, s = C.c_double(), C.c_int()
        tw, tm, os_, om = C.c_long(), C.c_long(), C.c_long(), C.c_long()
        rc = self._ck(self.L.tspgpu_multi_multistart_local_search_nl(self.m, p, m, float(time_left_s), best, C.byref(c), C.byref(s),
                                                                     C.byref(tw), C.byref(tm), C.byref(os_), C.byref(om)),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return {"path": best, "cost": c.value, "start": s.value, "two_opt_sweeps": tw.value, "two_opt_moves": tm.value,
                "or_sweeps": os_.value, "or_moves": om.value, "rc": rc}

    def multistart_local_search_nl3(self, width, starts=None, time_left_s=-1.0):
        """Engine.multistart_local_search_nl3 over every device ->
        dict(path, cost, start, two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, three_sweeps, three_moves, rc)."""
        p, m, keep = Engine._starts(starts, self.n)
        best = np.empty(self.n, dtype=np.int32)
        c, s = C.c_double(), C.c_int()
        tw, tm, os_, om, ts, tv = (C.c_long() for _ in range(6))
        rc = self._ck(self.L.tspgpu_multi_multistart_local_search_nl3(self.m, int(width), p, m, float(time_left_s), best, C.byref(c),
                                                                      C.byref(s), C.byref(tw), C.byref(tm), C.byref(os_), C.byref(om),
                                                                      C.byref(ts), C.byref(tv)),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return {"path": best, "cost": c.value, "start": s.value, "two_opt_sweeps": tw.value, "two_opt_moves": tm.value,
                "or_sweeps": os_.value, "or_moves": om.value, "three_sweeps": ts.value, "three_moves": tv.value, "rc": rc}

    def nn_all(self, starts=None, time_left_s=-1.0):
        """h_Greedy_iterative (heuristics.c:34-72) over every device -> (best_path, best_cost, best_start, done, rc)."""
        p, m, keep = Engine._starts(starts, self.n)
        best = np.empty(self.n, dtype=np.int32)
        c, s, d = C.c_double(), C.c_int(), C.c_int()
        rc = self._ck(self.L.tspgpu_multi_nn_all(self.m, p, m, float(time_left_s), best, C.byref(c), C.byref(s), C.byref(d)),
                      ok=(T_OK, DEADLINE_EXCEEDED))
        return best, c.value, s.value, d.value, rc


def evals_per_sweep(n):
    """valid pairs per sweep = n(n-3)/2 (adjacent pairs are skipped, refinment.c:55)."""
    return n * (n - 3) // 2
