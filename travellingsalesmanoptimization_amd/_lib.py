"""ctypes binding of the C ABI in include/tspgpu.h (csrc/libtspgpu.so).

The library is hand-written HIP for gfx950 and has no CPU fallback: if the
shared object is missing this module raises, and every call fails with
UNAVAILABLE (14) when no MI355X is visible.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libtspgpu.so")

# the reference's ERROR_CODE numbering, src/utils/errors.h:33-51
T_OK, CANCELLED, UNKNOWN, INVALID_ARGUMENT, DEADLINE_EXCEEDED = 0, 1, 2, 3, 4
RESOURCE_EXHAUSTED, FAILED_PRECONDITION, UNIMPLEMENTED, INTERNAL, UNAVAILABLE = 8, 9, 12, 13, 14

EUC_2D, ATT, CEIL_2D = 0, 1, 2
ELEM_AUTO, ELEM_F64, ELEM_I32, ELEM_U16 = 0, 1, 2, 3
OPT_ELEM, OPT_KERNEL, OPT_BATCH, OPT_WGS_PER_TOUR, OPT_HISTORY = 1, 2, 3, 4, 5
OPT_GRAPH, OPT_TIMING, OPT_BLOCK, OPT_MAX_TOURS, OPT_DEPTH, OPT_MATRIX_FREE, OPT_FUSED, OPT_SWEEP_CAP, OPT_NN_KERNEL, OPT_PIPE2 = 6, 7, 8, 9, 10, 11, 12, 13, 14, 15
OPT_PERSIST, OPT_PERSIST_EDGES, OPT_PERSIST_WINDOW, OPT_BUILD_KERNEL, OPT_STREAM_PERSIST = 16, 17, 18, 19, 20
OPT_EM_FORM = 21
OPT_OR_MATRIX_FREE = 22
INFO_OR_OTF, INFO_OR_OTF_R = 34, 35     # tspgpu_info: form (0 none, 1 full, 2 early-out) and R of the last matrix-free Or-opt sweep
# ... sweeps, moves and the largest move count of one sweep of the last parallel-move 2-opt descent; R and threads of its candidate sweep
INFO_MULTI_SWEEPS, INFO_MULTI_MOVES, INFO_MULTI_MAX_MOVES, INFO_MULTI_R, INFO_MULTI_THREADS, INFO_MULTI_NCH = 36, 37, 38, 39, 40, 41
# ... K' of the neighbour lists in place, sweeps / moves of the last neighbour-list 2-opt phase, sweeps of its polish, nodes per workgroup
INFO_NL_K, INFO_NL_SWEEPS, INFO_NL_MOVES, INFO_NL_POLISH_SWEEPS, INFO_NL_NODES = 42, 43, 44, 45, 46
# ... Or-opt sweeps / moves / largest sweep of the last neighbour-list Or-opt call, rounds of the last local_search_nl, starts per workgroup
INFO_OR_NL_SWEEPS, INFO_OR_NL_MOVES, INFO_OR_NL_MAX_MOVES, INFO_OR_NL_ROUNDS, INFO_OR_NL_STARTS = 47, 48, 49, 50, 51
# ... tours, sweep launches and most live tours of the last batched neighbour-list descent, workgroups per tour of its candidate sweep
INFO_NL_BATCH_TOURS, INFO_NL_BATCH_LAUNCHES, INFO_NL_BATCH_MAX_LIVE, INFO_NL_BATCH_WGS = 52, 53, 54, 55
# ... walks, iterations completed, sweep rounds, most live walks and dry walks of the last neighbour-list VNS call
INFO_VNS_NL_WALKS, INFO_VNS_NL_ITERATIONS, INFO_VNS_NL_ROUNDS, INFO_VNS_NL_MAX_LIVE, INFO_VNS_NL_DRY = 56, 57, 58, 59, 60
# ... W in effect, sweeps / moves / largest sweep of the last neighbour-list 3-opt call, 3-opt phases of the last local_search_nl3,
# nodes per workgroup of its candidate sweep (61 is the shape-specialised LDS-resident descent's flag)
INFO_THREE_NL_W, INFO_THREE_NL_SWEEPS, INFO_THREE_NL_MOVES, INFO_THREE_NL_MAX_MOVES, INFO_THREE_NL_PHASES, INFO_THREE_NL_NODES = 62, 63, 64, 65, 66, 67
INFO_PERSIST_TMAT = 68                  # the last LDS-resident descent fetched moved rows from the tour-ordered matrix copy
INFO_PERSIST_PACKED = 69                # the last LDS-resident descent / tabu walk / VNS walk ran the packed 16-bit loop
# ... units looked at, full sweeps and the largest sweep that was not full of the last call with don't-look bits; the most
# workgroups of a queued sweep
INFO_DL_LOOKED, INFO_DL_FULL_SWEEPS, INFO_DL_MAX_QUEUE, INFO_DL_MAX_WGS = 70, 71, 72, 73
# ... the last greedy-edge construction: rounds of phase 1 and of phase 2, edges phase 1 accepted, free nodes entering phase 2
INFO_GREEDY_ROUNDS1, INFO_GREEDY_ROUNDS2, INFO_GREEDY_EDGES1, INFO_GREEDY_FREE = 74, 75, 76, 77
# ... the last batched neighbour-list descent: its 3-opt width in effect (0: two phases), 3-opt sweeps / moves over the tours, and the
# most moves one tour's 3-opt sweep accepted
INFO_NL3_BATCH_W, INFO_NL3_BATCH_SWEEPS, INFO_NL3_BATCH_MOVES, INFO_NL3_BATCH_MAX_MOVES = 78, 79, 80, 81
# ... Boruvka rounds of the last 1-tree, iterations / reason / final h of the last Held-Karp ascent, nodes per workgroup of its scan
INFO_HK_ROUNDS, INFO_HK_ITERATIONS, INFO_HK_REASON, INFO_HK_H, INFO_HK_NODES = 86, 87, 88, 89, 90
EM_FORM_AUTO, EM_FORM_RESIDENT, EM_FORM_PER_STEP = 0, 1, 2
MOPT_EXCHANGE = 1000
EXCHANGE_AUTO, EXCHANGE_HOST, EXCHANGE_RCCL = 0, 1, 2

_dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_ip = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_pd = C.POINTER(C.c_double)
_pi = C.POINTER(C.c_int)
_pl = C.POINTER(C.c_long)
_ctx = C.c_void_p

# symbol -> (restype, argtypes): every entry point include/tspgpu.h declares
SIGNATURES = {
    "tspgpu_device_count": (C.c_int, []),
    "tspgpu_create": (C.c_int, [C.c_int, C.POINTER(_ctx)]),
    "tspgpu_destroy": (None, [_ctx]),
    "tspgpu_last_error": (C.c_char_p, [_ctx]),
    "tspgpu_set_option": (C.c_int, [_ctx, C.c_int, C.c_long]),
    "tspgpu_info": (C.c_long, [_ctx, C.c_int]),
    "tspgpu_set_points": (C.c_int, [_ctx, _dp, C.c_int, C.c_int]),
    "tspgpu_build_costs": (C.c_int, [_ctx, C.c_void_p]),
    "tspgpu_set_costs": (C.c_int, [_ctx, _dp, C.c_int]),
    "tspgpu_get_costs": (C.c_int, [_ctx, _dp]),
    "tspgpu_nn_tour": (C.c_int, [_ctx, C.c_int, _ip, _pd]),
    "tspgpu_two_opt_once": (C.c_int, [_ctx, _ip, _pd, _pd]),
    "tspgpu_two_opt": (C.c_int, [_ctx, _ip, _pd, C.c_double, _pl]),
    "tspgpu_tabu_move": (C.c_int, [_ctx, _ip, _pd, _ip, C.c_int, C.c_int]),
    "tspgpu_tabu_search": (C.c_int, [_ctx, _ip, _pd, C.c_int, _ip, _pd, C.c_void_p]),
    "tspgpu_vns_search": (C.c_int, [_ctx, _ip, _pd, C.c_int, C.c_double, _ip, C.c_long, _pl, _pi, _pi, _ip, _pd, C.c_void_p]),
    "tspgpu_farthest_pair": (C.c_int, [_ctx, _pi, _pi, _pd]),
    "tspgpu_extra_mileage": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_double, _ip, _pd]),
    "tspgpu_or_opt_once": (C.c_int, [_ctx, _ip, _pd, _pd, _ip]),
    "tspgpu_or_opt": (C.c_int, [_ctx, _ip, _pd, C.c_double, _pl]),
    "tspgpu_local_search": (C.c_int, [_ctx, _ip, _pd, C.c_double, _pl, _pl, _pi]),
    "tspgpu_tour_or_opt": (C.c_int, [_ctx, C.c_int, C.c_long, C.c_double, _pl]),
    "tspgpu_tour_local_search": (C.c_int, [_ctx, C.c_int, C.c_double, _pl, _pl, _pi]),
    "tspgpu_tours_local_search": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tspgpu_multistart_local_search": (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_double, _ip, _pd, _pi, _pl, _pl, C.c_void_p]),
    "tspgpu_time_or_sweep": (C.c_int, [_ctx, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "tspgpu_nn_all": (C.c_int, [_ctx, C.c_void_p, C.c_int, _ip, _pd, _pi]),
    "tspgpu_tour_sweep_part": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, _pd, _pi, _pi]),
    "tspgpu_tour_apply_move": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_double]),
    "tspgpu_nn_all_timed": (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_double, _ip, _pd, _pi, _pi]),
    "tspgpu_multistart_nn_2opt": (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_double, _ip, _pd, _pi, _pl,
                                            C.c_void_p, C.c_void_p]),
    "tspgpu_multi_select": (C.c_int, [_dp, np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS"), C.c_int, C.c_int]),
    "tspgpu_multi_create": (C.c_int, [_ip, C.c_int, C.POINTER(_ctx)]),
    "tspgpu_multi_destroy": (None, [_ctx]),
    "tspgpu_multi_last_error": (C.c_char_p, [_ctx]),
    "tspgpu_multi_devices": (C.c_int, [_ctx]),
    "tspgpu_multi_ctx": (_ctx, [_ctx, C.c_int]),
    "tspgpu_multi_info": (C.c_double, [_ctx, C.c_int]),
    "tspgpu_multi_set_option": (C.c_int, [_ctx, C.c_int, C.c_long]),
    "tspgpu_multi_prepare": (C.c_int, [_ctx]),
    "tspgpu_multi_set_points": (C.c_int, [_ctx, _dp, C.c_int, C.c_int]),
    "tspgpu_multi_build_costs": (C.c_int, [_ctx]),
    "tspgpu_multi_multistart_nn_2opt": (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_double, _ip, _pd, _pi, _pl]),
    "tspgpu_multi_multistart_local_search": (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_double, _ip, _pd, _pi, _pl, _pl]),
    "tspgpu_multi_nn_all": (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_double, _ip, _pd, _pi, _pi]),
    "tspgpu_tour_load": (C.c_int, [_ctx, C.c_int, _ip]),
    "tspgpu_tour_nn": (C.c_int, [_ctx, C.c_int, C.c_int]),
    "tspgpu_tour_copy": (C.c_int, [_ctx, C.c_int, C.c_int]),
    "tspgpu_tour_two_opt": (C.c_int, [_ctx, C.c_int, C.c_long, C.c_double, _pl]),
    "tspgpu_tour_store": (C.c_int, [_ctx, C.c_int, C.c_void_p, _pd, _pd]),
    "tspgpu_time_sweep": (C.c_int, [_ctx, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "tspgpu_time_build": (C.c_int, [_ctx, C.c_int, C.POINTER(C.c_float)]),
    "tspgpu_timing_read": (C.c_int, [_ctx, _pd, _pl, C.c_int]),
    "tspgpu_debug_stamps": (C.c_int, [_ctx, C.c_void_p, C.c_int]),
    "tspgpu_debug_tmat": (C.c_int, [_ctx, C.c_void_p, C.c_size_t]),
    "tspgpu_history": (C.c_int, [_ctx, _ip, _ip, _dp, C.c_int, _pi]),
    "tspgpu_two_opt_multi_once": (C.c_int, [_ctx, _ip, _pd, _pi, _ip, _dp, C.c_int]),
    "tspgpu_two_opt_multi": (C.c_int, [_ctx, _ip, _pd, C.c_double, _pl, _pl]),
    "tspgpu_tour_two_opt_multi": (C.c_int, [_ctx, C.c_int, C.c_long, C.c_double, _pl, _pl]),
    "tspgpu_time_multi_sweep": (C.c_int, [_ctx, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "tspgpu_neighbours_build": (C.c_int, [_ctx, C.c_int]),
    "tspgpu_neighbours_get": (C.c_int, [_ctx, _ip, C.c_void_p]),
    "tspgpu_two_opt_nl_once": (C.c_int, [_ctx, _ip, _pd, _pi, _ip, _dp, C.c_int]),
    "tspgpu_two_opt_nl": (C.c_int, [_ctx, _ip, _pd, C.c_double, C.c_int, _pl, _pl, _pl, _pl]),
    "tspgpu_tour_two_opt_nl": (C.c_int, [_ctx, C.c_int, C.c_long, C.c_double, _pl, _pl]),
    "tspgpu_time_nl_sweep": (C.c_int, [_ctx, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "tspgpu_or_opt_nl_once": (C.c_int, [_ctx, _ip, _pd, _pi, _ip, _dp, C.c_int]),
    "tspgpu_or_opt_nl": (C.c_int, [_ctx, _ip, _pd, C.c_double, _pl, _pl]),
    "tspgpu_tour_or_opt_nl": (C.c_int, [_ctx, C.c_int, C.c_long, C.c_double, _pl, _pl]),
    "tspgpu_local_search_nl": (C.c_int, [_ctx, _ip, _pd, C.c_double, _pl, _pl, _pl, _pl, _pi]),
    "tspgpu_tour_local_search_nl": (C.c_int, [_ctx, C.c_int, C.c_double, _pl, _pl, _pl, _pl, _pi]),
    "tspgpu_time_or_nl_sweep": (C.c_int, [_ctx, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "tspgpu_three_opt_nl_once": (C.c_int, [_ctx, C.c_int, _ip, _pd, _pi, _ip, _dp, C.c_int]),
    "tspgpu_three_opt_nl": (C.c_int, [_ctx, C.c_int, _ip, _pd, C.c_double, _pl, _pl]),
    "tspgpu_tour_three_opt_nl": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_long, C.c_double, _pl, _pl]),
    "tspgpu_local_search_nl3": (C.c_int, [_ctx, C.c_int, _ip, _pd, C.c_double, _pl, _pl, _pl, _pl, _pi, _pl, _pl, _pi]),
    "tspgpu_tour_local_search_nl3": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_double, _pl, _pl, _pl, _pl, _pi, _pl, _pl, _pi]),
    "tspgpu_time_three_nl_sweep": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "tspgpu_tours_local_search_nl": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tspgpu_multistart_local_search_nl": (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_double, _ip, _pd, _pi, _pl, _pl, _pl, _pl, C.c_void_p]),
    "tspgpu_vns_walks_nl": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_double, _ip, _dp, C.c_void_p, C.c_long, C.c_void_p, _ip, _ip, _ip, _dp,
                                      C.c_void_p, C.c_void_p]),
    "tspgpu_tour_wake": (C.c_int, [_ctx, C.c_int, C.c_void_p, C.c_int]),
    "tspgpu_tour_sleep": (C.c_int, [_ctx, C.c_int]),
    "tspgpu_tour_awake": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_void_p, _pi]),
    "tspgpu_tour_kick": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_int]),
    "tspgpu_tour_two_opt_nl_dl": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_long, C.c_double, _pl, _pl, _pl]),
    "tspgpu_tour_or_opt_nl_dl": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_long, C.c_double, _pl, _pl, _pl]),
    "tspgpu_tour_three_opt_nl_dl": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_long, C.c_double, _pl, _pl, _pl]),
    "tspgpu_tour_local_search_nl3_dl": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_double, _pl, _pl, _pl, _pl, _pi, _pl, _pl, _pi, _pl, _pl]),
    "tspgpu_local_search_nl3_dl": (C.c_int, [_ctx, C.c_int, C.c_int, _ip, _pd, C.c_double, _pl, _pl, _pl, _pl, _pi, _pl, _pl, _pi, _pl, _pl]),
    "tspgpu_tour_greedy": (C.c_int, [_ctx, C.c_int]),
    "tspgpu_greedy_tour": (C.c_int, [_ctx, _ip, _pd]),
    "tspgpu_one_tree": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_void_p, _pl]),
    "tspgpu_lower_bound": (C.c_int, [_ctx, C.c_double, C.c_int, C.c_int, C.c_double, C.c_void_p, _pd, C.c_void_p, C.c_void_p, _pi, _pi]),
    "tspgpu_multi_neighbours_build": (C.c_int, [_ctx, C.c_int]),
    "tspgpu_multi_multistart_local_search_nl": (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_double, _ip, _pd, _pi, _pl, _pl, _pl, _pl]),
    "tspgpu_tours_local_search_nl3": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tspgpu_multistart_local_search_nl3": (C.c_int, [_ctx, C.c_int, C.c_void_p, C.c_int, C.c_double, _ip, _pd, _pi, _pl, _pl, _pl, _pl, _pl, _pl,
                                                     C.c_void_p]),
    "tspgpu_multi_multistart_local_search_nl3": (C.c_int, [_ctx, C.c_int, C.c_void_p, C.c_int, C.c_double, _ip, _pd, _pi, _pl, _pl, _pl, _pl,
                                                           _pl, _pl]),
    "tspgpu_vns_walks_nl3": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_double, _ip, _dp, C.c_void_p, C.c_long, C.c_void_p, _ip, _ip, _ip, _dp,
                                       C.c_void_p, C.c_void_p]),
    "tspgpu_tours_local_search_nl3_dl": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double] + [C.c_void_p] * 10),
    "tspgpu_multistart_local_search_nl3_dl": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_double, _ip, _pd, _pi, _pl, _pl, _pl, _pl,
                                                        _pl, _pl, _pl, _pl, C.c_void_p]),
    "tspgpu_vns_walks_nl3_dl": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _ip, _dp, C.c_void_p, C.c_long, C.c_void_p, _ip, _ip,
                                          _ip, _dp, C.c_void_p, C.c_void_p]),
}

_lib = None


def load():
    """dlopen the engine and bind every symbol; raises if the .so is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C travellingsalesmanoptimization_amd/csrc` (hipcc, gfx950). There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the ABI drifted from the header
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib
