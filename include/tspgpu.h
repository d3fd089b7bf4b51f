/*
 * include/tspgpu.h -- C ABI of the MI355X (gfx950) 2-opt local-search engine.
 *
 * This is the drop-in boundary for the heuristic path of
 * enricobolzonello/TravellingSalesmanOptimization.  The reference has no
 * plugin/FFI layer: its boundary is a set of plain C functions over two
 * process-wide globals (src/tsp.h:235-236).  Each entry point below names the
 * reference function (file:line under the reference checkout) whose work it
 * takes over; the host-side C layer in travellingsalesmanoptimization_amd/host/
 * keeps the reference's own signatures on top of these.
 *
 * Conventions
 *   - plain pointers and sizes only; no global state; one opaque context per
 *     caller thread (contexts are independent, so the CPLEX callback threads
 *     of src/algorithms/cplex_model.c:1176-1258 can each own one).
 *   - return value: the reference's ERROR_CODE numbering
 *     (src/utils/errors.h:33-51): 0 T_OK, 3 INVALID_ARGUMENT,
 *     4 DEADLINE_EXCEEDED (a success, src/utils/errors.c:31-37),
 *     8 RESOURCE_EXHAUSTED, 9 FAILED_PRECONDITION, 12 UNIMPLEMENTED,
 *     13 INTERNAL (HIP runtime failure), 14 UNAVAILABLE (no device).
 *   - tours are SUCCESSOR arrays, path[i] = node visited after node i
 *     (src/algorithms/refinment.c:51-52), exactly as tsp_solution.path.
 *   - cost matrices are row-major n x n doubles, as tsp_inst.costs.
 *   - there is NO CPU fallback: without a HIP device every call fails.
 */
#ifndef TSPGPU_H
#define TSPGPU_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tspgpu_ctx tspgpu_ctx;

/* edge-weight kinds for tspgpu_set_points.  EUC_2D reproduces src/tsp.c:629
 * bit for bit (float sqrt of a double sum).  ATT / CEIL_2D are TSPLIB 95
 * definitions in double; the reference rejects them (src/tsp.c:576-584). */
enum { TSPGPU_EUC_2D = 0, TSPGPU_ATT = 1, TSPGPU_CEIL_2D = 2 };

/* storage of the device-resident cost matrix.  AUTO keeps the narrowest EXACT copy:
 * uint16 when every entry is an integer in [0, 65534] (diagonal -1), int32 when every
 * entry is an integer in [-1, 2^27) (true for every EUC_2D / ATT / CEIL_2D matrix),
 * else doubles, the reference's own format.  The lower end is for every cell, not the diagonal alone: a caller matrix
 * (tspgpu_set_costs) with an off-diagonal -1 is admitted in int32 cells and taken as the cost -1 by the sweeps, the
 * neighbour lists and the greedy-edge construction; a matrix with a value below -1 or a non-integer is held in doubles,
 * negative values and -0.0 (which compares equal to +0.0) included.  Extra Mileage alone refuses a negative
 * off-diagonal cost, with FAILED_PRECONDITION (9): its packed keys hold costs in [0, 2^27). */
enum { TSPGPU_ELEM_AUTO = 0, TSPGPU_ELEM_F64 = 1, TSPGPU_ELEM_I32 = 2, TSPGPU_ELEM_U16 = 3 };

/* tunables (tspgpu_set_option) */
enum {
    TSPGPU_OPT_ELEM = 1,        /* TSPGPU_ELEM_*; takes effect at the next build/set_costs */
    TSPGPU_OPT_KERNEL = 2,      /* 0 auto, 1 "simple", 2 "pipelined", 3 "resident" sweep kernel (info reports 4 = matrix-free) */
    TSPGPU_OPT_BATCH = 3,       /* sweeps enqueued between host polls (default 32) */
    TSPGPU_OPT_WGS_PER_TOUR = 4,/* workgroups per tour in the sweep (0 = auto) */
    TSPGPU_OPT_HISTORY = 5,     /* record (a,b,delta) of the first N sweeps of slot 0 */
    TSPGPU_OPT_GRAPH = 6,       /* 1 = replay sweep batches as a hipGraph (default 1) */
    TSPGPU_OPT_TIMING = 7,      /* 1 = bracket every sweep kernel with HIP events */
    TSPGPU_OPT_BLOCK = 8,       /* threads per sweep workgroup (0 = auto) */
    TSPGPU_OPT_MAX_TOURS = 9,   /* tours kept in flight by the multi-start driver */
    TSPGPU_OPT_DEPTH = 10,      /* matrix rows in flight per workgroup in the pipelined sweep (0 = auto) */
    TSPGPU_OPT_FUSED = 12,      /* one launch per sweep (resident kernel): 1 (default) when <= 4 tours are in flight,
                                   2 always, 0 never (separate sweep + apply launches) */
    TSPGPU_OPT_MATRIX_FREE = 11,/* 0 auto (matrix-free when a matrix row cannot sit in LDS or n exceeds the matrix-mode
                                   limit of 65 536 nodes), 1 always, 2 never (tspgpu_build_costs then fails with code 8
                                   past either limit, before any matrix is allocated); takes effect at the next
                                   tspgpu_build_costs.  Matrix-free mode needs costs below 2^27 (else code 8) and n <= 131 072 */
    TSPGPU_OPT_PIPE2 = 15,      /* one-launch-per-sweep kernel over streamed rows: 1 (default) two tour edges per barrier
                                   interval where four rows fit LDS, 0 one edge per barrier over three row buffers */
    TSPGPU_OPT_NN_KERNEL = 14,  /* nearest-neighbour construction: 0 auto (the grid kernel whenever the weights come from
                                   the uploaded points -- with every point's 3 nearest neighbours in LDS where they fit --,
                                   else the matrix kernel), 1 matrix / strided kernels always, 3 the grid kernel without
                                   the neighbour lists */
    TSPGPU_OPT_SWEEP_CAP = 13,  /* sweeps per start in tspgpu_multistart_nn_2opt (-1 = to the local optimum, the
                                   reference's behaviour; >= 0 caps every local search: tests and bounded runs) */
    TSPGPU_OPT_PERSIST = 16,    /* single-tour descent with the uint16 matrix resident in LDS, one launch per descent
                                   (whole rows for n <= 4096, half-window rows up to n of about 5400, one workgroup per CU),
                                   and tspgpu_tabu_search's walk the same way (n up to about 3800): 0 never, 1 (default)
                                   where it applies -- falls back to one launch per sweep when the grid cannot be
                                   co-resident --, 2 or fail with code 8 */
    TSPGPU_OPT_PERSIST_EDGES = 17, /* tour edges per workgroup of that kernel (0 = auto: ceil(n / CUs); at most 16 with whole
                                   rows, 24 with half-window rows) */
    TSPGPU_OPT_BUILD_KERNEL = 19,  /* tspgpu_build_costs with uint16 cells: 0 (default) the upper triangle computed once, every
                                   64 x 64 tile stored twice (as it is and transposed through LDS), 1 every cell computed
                                   (what int32 / f64 cells always do) */
    TSPGPU_OPT_STREAM_PERSIST = 20,/* single-tour descent past the LDS-resident sizes (uint16 cells, n from about 5400 to 16383)
                                   in ONE launch with the rows streamed and the tour state kept on the chip (k_str2opt, one
                                   workgroup per CU, one grid-wide exchange per sweep): 0 never, 1 (default) where it applies
                                   -- falls back to one launch per sweep when the grid cannot be co-resident --, 2 or fail with
                                   code 8 (and used from n = 1024 up).  The LDS-resident descent is tried first: 2 forces this
                                   kernel only together with TSPGPU_OPT_PERSIST = 0; with TSPGPU_OPT_PERSIST = 1 or 2 an instance
                                   the LDS-resident kernel takes runs there, and tspgpu_info 24 then reads 0 */
    TSPGPU_OPT_PERSIST_WINDOW = 18 /* rows of that kernel: 0 auto (whole rows where they fit the chip's LDS, else the half
                                   window of n/2 cells ahead of the workgroup's own edges), 1 half-window rows wherever they
                                   apply, 2 whole rows only */,
    TSPGPU_OPT_EM_FORM = 21,    /* Extra Mileage insertion loop (tspgpu_extra_mileage): 0 (default) and 2 one launch pair per
                                   step, enqueued back to back (measured faster); 1 ONE launch for the whole construction
                                   (one workgroup per CU, a grid barrier between phases), or fail with code 8 when the grid
                                   does not come up co-resident */
    TSPGPU_OPT_OR_MATRIX_FREE = 22 /* Or-opt in matrix-free mode (the section "Or-opt" below): 0 (default) refused with code 12,
                                   1 the single-tour entry points run from the uploaded coordinates; any other value: 3 */
};

int  tspgpu_device_count(void);
int  tspgpu_create(int device, tspgpu_ctx **out);
void tspgpu_destroy(tspgpu_ctx *ctx);
const char *tspgpu_last_error(const tspgpu_ctx *ctx);
int  tspgpu_set_option(tspgpu_ctx *ctx, int option, long value);
/* info: 0 n, 1 row stride, 2 element kind in use, 3 sweep kernel in use,
 * 4 workgroups per tour, 5 LDS bytes per workgroup, 6 threads per workgroup,
 * 7 matrix is symmetric, 8 compute units, 9 rows in flight per workgroup,
 * 10 matrix-free mode in use, 11 one-launch-per-sweep path in use, 12 cells per side of the NN grid (0: the
 * grid kernel is not in use), 13 most points in one grid cell, 14 the fused streaming kernel takes two edges per
 * barrier interval, 15 the last single-tour descent ran LDS-resident (TSPGPU_OPT_PERSIST), 16 / 17 / 18 workgroups, tour
 * edges per workgroup and LDS bytes per workgroup of that kernel on this instance (0: it does not apply), 19 window cells per
 * row of its half-window form (0: whole rows), 20 the last single-tour descent ran in the half-window form, 21 the last
 * single-tour descent began LDS-resident and was finished one launch per sweep (the grid lost its co-residency), 22 sweeps run by the last
 * LDS-resident descent / tabu walk / VNS walk, 23 how the last tspgpu_vns_search ran (1 resident throughout, 2 one device local
 * search per iteration with the kicks on the host, 3 resident launches first, then -- the grid lost its co-residency -- host kicks),
 * 24 the last single-tour descent ran in the streamed persistent kernel (TSPGPU_OPT_STREAM_PERSIST), 25 the matrix-free sweep
 * kernel of the current plan (0 not matrix-free / no plan yet, 1 k_sweep_otf: costs from 2^25 or n = 131 072, 2 k_sweep_otf8,
 * 3 k_sweep_otf8 with the exact early-out), 26 CEIL_2D weights come from the exact integer ceil-sqrt of integer coordinates
 * (cost bound below 2^22; 0: the generic double form, or another kind), 27 how the last tspgpu_extra_mileage ran (1 one launch,
 * 2 one launch pair per step), 28 / 29 its stale-node rescans / insertions, 30 tour positions per Or-opt sweep workgroup (R) in
 * the first Or-opt round of the last batched descent (tspgpu_tours_local_search and the calls built on it; 0: none ran), 31 the R of a single-tour Or-opt sweep on this instance (0: no matrix),
 * 32 / 33 threads per workgroup (256, 512 or 1024) and 16-byte vectors per thread and matrix row (1, 2 or 3) of an Or-opt sweep,
 * single-tour or batched, on this instance (0 where 31 is 0), 34 how the last matrix-free Or-opt sweep ran (0 none, 1 every candidate
 * evaluated, 2 with the exact early-out), 35 tour positions per workgroup of that sweep (0 where 34 is 0); 36 .. 60 in the
 * sections below; 61 the last LDS-resident descent ran in an instantiation of k_lds2opt compiled for its shape (plain 2-opt,
 * packed 16-bit costs, (n, edges per workgroup) = (4096, 16) or (1024, 4); 0: the generic kernel); 62 .. 67 in
 * "Neighbour-list 3-opt" below; 68 with tspgpu_debug_tmat below; 69 the last LDS-resident descent, tabu walk or VNS walk (whole rows or
 * half-window rows) ran the loop over packed 16-bit deltas (every cost <= 16383; the tabu walk: <= 8190), 0: 32-bit deltas; 70 .. 77 in
 * the sections below; 78 .. 81 in "Batched neighbour-list 3-opt" below; 86 .. 91 in "Held-Karp lower bound" below */
long tspgpu_info(const tspgpu_ctx *ctx, int what);

/* ---- instance / cost matrix ------------------------------------------- */

/* Upload n points ({x,y} doubles = the reference's `point`, src/utils/utils.h:37-40). */
int tspgpu_set_points(tspgpu_ctx *ctx, const double *xy, int n, int edge_weight_type);

/* Replaces tsp_compute_costs (src/tsp.c:608-636): builds the n x n matrix on
 * the device from the uploaded points.  host_out may be NULL; otherwise it
 * receives the row-major n x n doubles (what tsp_inst.costs holds). */
int tspgpu_build_costs(tspgpu_ctx *ctx, double *host_out);

/* Caller-supplied matrix, the h_Greedy_2opt_mod_costs case
 * (src/algorithms/heuristics.c:118-149): row-major n x n doubles.
 * A matrix that is not symmetric is recorded (tspgpu_info 7 reads 0) and taken by the NN constructions, the plain 2-opt
 * sweeps, the tabu move and walk, tspgpu_vns_search, tspgpu_multistart_nn_2opt, the farthest pair and Extra Mileage, which then
 * evaluate only the reference's orientation b > a and read every cost from the row the reference reads it from.  The fused
 * sweep and the one-launch descents and walks never run on it (TSPGPU_OPT_PERSIST = 2 and TSPGPU_OPT_STREAM_PERSIST = 2
 * answer 8; both Extra Mileage forms do run) and the extensions refuse it with 9;
 * tests/test_asymmetric.py pins all of it against the CPU oracle. */
int tspgpu_set_costs(tspgpu_ctx *ctx, const double *host_costs, int n);

/* Read the device matrix back (row-major n x n doubles). */
int tspgpu_get_costs(tspgpu_ctx *ctx, double *host_out);

/* ---- single-tour entry points (host arrays in/out) --------------------- */

/* h_greedyutil (src/algorithms/heuristics.c:216-288): nearest-neighbour tour
 * from `start`, ties to the lowest index.  14 if start is out of range. */
int tspgpu_nn_tour(tspgpu_ctx *ctx, int start, int *path, double *cost);

/* ref_2opt_once (src/algorithms/refinment.c:39-93): one best-improvement sweep
 * over all pairs; applies the move when delta < -1e-7 and adds delta to *cost.
 * *delta receives the best delta (0 when no improving pair exists). */
int tspgpu_two_opt_once(tspgpu_ctx *ctx, int *path, double *cost, double *delta);

/* ref_2opt (src/algorithms/refinment.c:3-37): recomputes *cost from the
 * matrix, then sweeps to the local optimum.  time_left_s < 0 = no deadline
 * (tsp_env.timelimit == -1); otherwise 4 is returned once it is exceeded,
 * polled once per batch of sweeps.  *sweeps (may be NULL) counts sweeps, the
 * final non-improving one included. */
int tspgpu_two_opt(tspgpu_ctx *ctx, int *path, double *cost, double time_left_s, long *sweeps);

/* tabu_best_move (src/algorithms/metaheuristic.c:188-245): best non-tabu move,
 * always applied; stamps tabu_list[a,b,succ a,succ b] = iter. */
int tspgpu_tabu_move(tspgpu_ctx *ctx, int *path, double *cost, int *tabu_list, int tenure, int iter);

/* the k-iteration loop of mh_TabuSearch (src/algorithms/metaheuristic.c:115-166)
 * with tabu_init (:65-84) and the linear tenure policy (:40-59), resident on
 * the device.  In: path/cost = the seed.  Out: path/cost = the walk's final
 * tour, best_path/best_cost = the incumbent (strict <, src/tsp.c:669-676).
 * trace (may be NULL) receives the k per-iteration costs that the reference
 * prints to results/TabuResults.dat. */
int tspgpu_tabu_search(tspgpu_ctx *ctx, int *path, double *cost, int k,
                       int *best_path, double *best_cost, double *trace);

/* the loop of mh_VNS (src/algorithms/metaheuristic.c:279-318): k iterations of { ref_2opt (:290), incumbent (:298-302),
 * r = rand() % 9 - 2 kicks (:308-318; vns_kick :344-409 = three tour positions under the reference's rejection rule, then
 * tabu_make_move case 7, :490-500) }, resident on the device where the instance allows it (uint16 cells, n up to about
 * 5400, an idle chip: the whole loop inside the LDS-resident kernel -- every workgroup applies the same kicks to its own
 * copy of the tour, no exchange --, else one device local search per iteration with the kicks on the host).
 * The random numbers are the CALLER's: rand_values[0 .. nrand) are rand() outputs drawn from the program's stream in
 * order; *consumed says how many the call used, so that the caller's stream can continue exactly where the reference's
 * would (host/tsp_algos.c keeps the rest queued).  In / out: path (the current tour; *cost is recomputed, refinment.c:6-9),
 * *iterations (completed so far), *kick_pending (1: the local search of iteration *iterations is done, its kicks are not),
 * best_path / *best_cost (the incumbent, strict <).  trace (may be NULL, else room for k - *iterations doubles): the cost
 * of every local optimum reached by this call, trace[0] = iteration *iterations at entry (what the reference prints to
 * results/VNSResults.dat).  Returns 0 when *iterations == k, 4 when the deadline passed,
 * 8 when the numbers ran out in front of a kick phase -- state consistent, call again with more. */
int tspgpu_vns_search(tspgpu_ctx *ctx, int *path, double *cost, int k, double time_left_s,
                      const int *rand_values, long nrand, long *consumed, int *iterations, int *kick_pending,
                      int *best_path, double *best_cost, double *trace);

/* ---- Extra Mileage (h_ExtraMileage, src/algorithms/heuristics.c:156-210) --------
 * Both need every off-diagonal cost an integer in [0, 2^27) -- true for every matrix tspgpu_build_costs makes, in
 * matrix and matrix-free mode; a caller matrix (tspgpu_set_costs) that breaks it fails with FAILED_PRECONDITION (9). */

/* The EM_MAX start of h_ExtraMileage (src/algorithms/heuristics.c:165-177): the first pair i < j in row-major order
 * whose cost is strictly the largest (all costs 0: (0, 1)).  *cost = c[a][b]. */
int tspgpu_farthest_pair(tspgpu_ctx *ctx, int *a, int *b, double *cost);

/* h_extramileage_util (src/algorithms/heuristics.c:290-367) from the pair (a, b) as h_ExtraMileage starts it
 * (:180-186: path[a] = b, path[b] = a, cost 2 c[a][b]): cheapest insertion, the first strict minimum of
 * c[u][i] + c[i][v] - c[u][v] over unvisited i ascending, then edges in the reference's array order, until every
 * node is in.  path receives the successor array, *cost = 2 c[a][b] + the inserted deltas.  3 when a, b are not two
 * distinct nodes; time_left_s < 0 = no deadline, else checked before every insertion: 4 when it passes, and then path
 * and *cost are left untouched (the reference's partial tour is rejected by tsp_update_best_solution).
 * TSPGPU_OPT_EM_FORM chooses between the one-launch and the per-step form; tspgpu_info 27 says which ran. */
int tspgpu_extra_mileage(tspgpu_ctx *ctx, int a, int b, double time_left_s, int *path, double *cost);

/* ---- Or-opt and the 2-opt + Or-opt descent (an extension: the reference has no Or-opt) ----------------------------
 * A candidate (s, L, q, rev) moves the L in {1, 2, 3} consecutive tour nodes s .. t (t = L - 1 steps after s) between
 * q and q' = path[q]; q is any node outside the segment other than p = pred(s) (q = x = path[t] is allowed), rev = 1
 * (L >= 2 only) inserts the segment the other way round: (h, e) = (s, t), or (t, s) when rev.
 *     delta = ((c[p][x] + c[q][h]) + c[e][q']) - ((c[p][s] + c[t][x]) + c[q][q'])
 * evaluated in this order (bit-exact for double cells).  A sweep finds the first strict minimum over s ascending, then
 * L = 1, 2, 3, then q ascending, then rev = 0 before 1 -- the lexicographic minimum of (delta, s, L, q, rev) -- and applies
 * it iff delta < -1e-7 (TWO_OPT_EPS, src/algorithms/refinment.c): path[p] = x, path[q] = h, the segment's inner links
 * reversed when rev, path[e] = q', *cost += delta.
 * Preconditions: n >= 8 (else 3), a symmetric matrix (tspgpu_info 7, else 9), MATRIX MODE ONLY -- in matrix-free mode
 * every entry point of this section returns UNIMPLEMENTED (12) --, and four matrix rows of ld = n rounded up to 32 cells
 * plus 3072 bytes in one workgroup's 160 KiB of LDS: n <= 20 096 with uint16 cells, 10 048 with int32, 5 024 with
 * doubles, else RESOURCE_EXHAUSTED (8) with the limit in the error text.  Without a context (no device): 14.
 * With TSPGPU_OPT_OR_MATRIX_FREE = 1 the single-tour entry points -- tspgpu_or_opt_once, tspgpu_or_opt,
 * tspgpu_local_search, tspgpu_tour_or_opt, tspgpu_tour_local_search, tspgpu_time_or_sweep -- also run in matrix-free mode,
 * with the costs matrix mode would hold for the same points and kind recomputed from the coordinates: the same move, tie
 * order, outputs and deadline behaviour, so the whole descent equals the matrix-mode descent of the instance move for move.
 * There the preconditions are n >= 8 (else 3) and what matrix-free mode itself guarantees (integer costs below 2^27,
 * n <= 131 072, symmetry): there is no row-in-LDS limit.  The batch entry points (tspgpu_tours_local_search,
 * tspgpu_multistart_local_search, tspgpu_multi_multistart_local_search) stay refused with 12 in matrix-free mode whatever
 * the option says. */

/* one Or-opt sweep on a host tour; applies the move when delta < -1e-7.  *cost is the caller's running cost (as
 * tspgpu_two_opt_once).  move[4] = {s, L, q, rev} of the applied move (all -1 and *delta = 0 when nothing improves) */
int tspgpu_or_opt_once(tspgpu_ctx *ctx, int *path, double *cost, double *delta, int move[4]);
/* Or-opt sweeps until none improves; *cost is the caller's running cost plus the applied deltas in order; *moves (may be
 * NULL) counts applied moves.  time_left_s < 0 = no deadline, else polled before every sweep: 4 once it has passed */
int tspgpu_or_opt(tspgpu_ctx *ctx, int *path, double *cost, double time_left_s, long *moves);
/* Variable-neighbourhood descent: *cost recomputed as ref_2opt does (src/algorithms/refinment.c:6-9), then
 * { the 2-opt descent of tspgpu_two_opt to its local optimum; Or-opt sweeps until none improves } until the Or-opt
 * phase applies no move: the result is locally optimal for both neighbourhoods.  *two_opt_sweeps counts every round's
 * final non-improving sweep too, *rounds the 2-opt descents run (each may be NULL).  The deadline is polled between
 * Or-opt sweeps and handed on to the 2-opt descent; once it passes: 4, with a valid tour and its cost. */
int tspgpu_local_search(tspgpu_ctx *ctx, int *path, double *cost, double time_left_s,
                        long *two_opt_sweeps, long *or_moves, int *rounds);

/* ---- multi-start entry points ------------------------------------------ */

/* h_Greedy_iterative (src/algorithms/heuristics.c:34-72): NN from every listed
 * start (starts == NULL: 0..nstarts-1), first strictly-best kept. */
int tspgpu_nn_all(tspgpu_ctx *ctx, const int *starts, int nstarts,
                  int *best_path, double *best_cost, int *best_start);
/* The same under the reference's cooperative deadline (heuristics.c:43-49: checked before every
 * start): starts are processed in ascending batches sized to the time left (time_left_s < 0:
 * no limit); returns DEADLINE_EXCEEDED (4) with the best of the *done_starts processed so far
 * (best_start = -1 if none). */
int tspgpu_nn_all_timed(tspgpu_ctx *ctx, const int *starts, int nstarts, double time_left_s,
                        int *best_path, double *best_cost, int *best_start, int *done_starts);

/* h_greedy_2opt (src/algorithms/heuristics.c:74-116): NN + 2-opt from every
 * listed start, all on the device; the winner is the lowest cost, ties to the
 * earliest entry of `starts`.  last_path/last_cost (may be NULL) receive the
 * tour of the LAST start, which is what h_Greedy_2opt_mod_costs leaves in
 * *solution (src/algorithms/heuristics.c:118-149). */
int tspgpu_multistart_nn_2opt(tspgpu_ctx *ctx, const int *starts, int nstarts,
                              double time_left_s, int *best_path, double *best_cost,
                              int *best_start, long *total_sweeps,
                              int *last_path, double *last_cost);

/* NN + the 2-opt + Or-opt descent of tspgpu_local_search (the section "Or-opt" above, its preconditions and codes) from every
 * listed start (starts == NULL: 0..nstarts-1), the tours of a chunk of TSPGPU_OPT_MAX_TOURS starts descending together
 * (tspgpu_tours_local_search).  The winner is the lowest cost, ties to the earliest entry of `starts` (strict <); it is in
 * general NOT the tour tspgpu_multistart_nn_2opt + tspgpu_local_search on its winner gives.  costs_out (may be NULL) receives
 * every start's final cost in list order, the totals (each may be NULL) the sums over the starts.  A TSPGPU_OPT_SWEEP_CAP
 * other than -1 is refused with 3: a capped 2-opt phase is not this descent.  Once the deadline passes: 4, with the best of
 * the chunks begun so far (the entries of costs_out behind them are left as they were). */
int tspgpu_multistart_local_search(tspgpu_ctx *ctx, const int *starts, int nstarts, double time_left_s,
                                   int *best_path, double *best_cost, int *best_start,
                                   long *total_two_opt_sweeps, long *total_or_moves, double *costs_out);

/* ---- multi-device multi-start (csrc/tspgpu_multi.cpp) ------------------------
 * The reference's multi-start loops (h_greedy_2opt, src/algorithms/heuristics.c:82-111; h_Greedy_iterative, :43-66)
 * are sequential C; their iterations are independent except for the incumbent minimum (src/tsp.c:669-676, strict <).
 * Here one process drives several MI355X: one engine context and one host thread per device, entry p of the start
 * list on device p mod G, every device building its own matrix from the coordinates, and ONE exchange per call:
 * ncclAllReduce(ncclMin) over xGMI of one packed int64 per device (cost:31 | list position:24 | device rank:8: lowest
 * cost, ties to the earliest start -- the sequential strict-< result -- and the low byte names the owner), then
 * ncclBroadcast of the owner's successor array (4n bytes).  RCCL is dlopen'ed at the first exchange that needs it.
 * A device id may be listed more than once (several contexts on one GPU, how the sharding is exercised on a
 * one-GPU box); an RCCL communicator needs distinct devices, so that list exchanges on the host. */
typedef struct tspgpu_multi tspgpu_multi;
enum { TSPGPU_MOPT_EXCHANGE = 1000 };   /* tspgpu_multi_set_option: 0 auto (RCCL when G > 1 distinct devices, none for
                                           G = 1, host for a repeated device), 1 host, 2 RCCL (also with G = 1: a
                                           one-rank communicator; refused for a repeated device).  Every other option
                                           is a TSPGPU_OPT_* applied to each device's context. */
/* the winner among G per-device results by the host exchange's order (by_keys = 0) or by the keys the RCCL exchange reduces
 * (by_keys = 1); pos[i] < 0 = device i found nothing; returns the device rank, -1 if nobody, -2 on a bad argument.  Pure
 * host arithmetic (no device needed): what pins both selection orders in the CPU tests. */
int  tspgpu_multi_select(const double *cost, const long *pos, int ndev, int by_keys);
int  tspgpu_multi_create(const int *device_ids, int ndev, tspgpu_multi **out);
void tspgpu_multi_destroy(tspgpu_multi *m);
const char *tspgpu_multi_last_error(const tspgpu_multi *m);
int  tspgpu_multi_devices(const tspgpu_multi *m);
tspgpu_ctx *tspgpu_multi_ctx(tspgpu_multi *m, int i);          /* the i-th device's context (owned by m) */
/* info: 0 devices, 1 exchange the next call will use (0 none, 1 host, 2 RCCL), 2 exchange used by the last call,
 * 3 seconds spent in ncclCommInitAll, 4 seconds of the last exchange, 5 seconds of the last per-device solve,
 * 6 exchanges so far, 7 the device ids are distinct */
double tspgpu_multi_info(const tspgpu_multi *m, int what);
int  tspgpu_multi_set_option(tspgpu_multi *m, int option, long value);
/* create the RCCL communicator now if the next exchange will use one (ncclCommInitAll takes seconds on 8 devices;
 * the reference starts its clock after tsp_compute_costs, src/main.c:177 -- the host layer calls this there) */
int  tspgpu_multi_prepare(tspgpu_multi *m);
int  tspgpu_multi_set_points(tspgpu_multi *m, const double *xy, int n, int edge_weight_type);
int  tspgpu_multi_build_costs(tspgpu_multi *m);                 /* tsp_compute_costs on every device */
/* h_greedy_2opt (src/algorithms/heuristics.c:74-116) sharded over the devices; same results as
 * tspgpu_multistart_nn_2opt over the whole list when no deadline is set */
int  tspgpu_multi_multistart_nn_2opt(tspgpu_multi *m, const int *starts, int nstarts, double time_left_s,
                                     int *best_path, double *best_cost, int *best_start, long *total_sweeps);
/* tspgpu_multistart_local_search sharded the same way (entry p of the list on device p mod G, the same exchange);
 * without a handle: 14 */
int  tspgpu_multi_multistart_local_search(tspgpu_multi *m, const int *starts, int nstarts, double time_left_s,
                                          int *best_path, double *best_cost, int *best_start,
                                          long *total_two_opt_sweeps, long *total_or_moves);
/* h_Greedy_iterative (src/algorithms/heuristics.c:34-72) sharded the same way */
int  tspgpu_multi_nn_all(tspgpu_multi *m, const int *starts, int nstarts, double time_left_s,
                         int *best_path, double *best_cost, int *best_start, int *done_starts);

/* ---- device-resident variants (inputs already in HBM; used by bench.py) --- */

/* Tour slots: the slot array grows on demand and keeps what the existing slots hold; a slot holds a tour once
 * something was loaded / built / copied into it, and until the next tspgpu_build_costs / tspgpu_set_costs (its edge
 * costs belong to the matrix).  Slot entry points answer FAILED_PRECONDITION (9) for a slot that holds none -- a slot the
 * array has not grown to yet included (tspgpu_set_points and a tspgpu_set_costs of another n start the array empty) --
 * and INVALID_ARGUMENT (3) for a negative slot.
 * The host-array entry points above and the multi-start entry points use slots from 0 upwards as scratch. */
/* upload a successor array into tour slot `slot` */
int tspgpu_tour_load(tspgpu_ctx *ctx, int slot, const int *path);
/* NN tour built on the device straight into a slot */
int tspgpu_tour_nn(tspgpu_ctx *ctx, int slot, int start);
/* copy slot src to slot dst on the device */
int tspgpu_tour_copy(tspgpu_ctx *ctx, int dst, int src);
/* sweep slot to its local optimum (max_sweeps < 0: no cap) */
int tspgpu_tour_two_opt(tspgpu_ctx *ctx, int slot, long max_sweeps, double time_left_s, long *sweeps);
/* Or-opt on a slot (the section "Or-opt" above): at most max_moves moves (< 0: until no sweep improves); the slot's
 * cost and last delta follow, and every later slot call (2-opt sweeps included) sees the rewritten tour */
int tspgpu_tour_or_opt(tspgpu_ctx *ctx, int slot, long max_moves, double time_left_s, long *moves);
/* the descent of tspgpu_local_search on a slot (its cost is taken as it stands) */
int tspgpu_tour_local_search(tspgpu_ctx *ctx, int slot, double time_left_s,
                             long *two_opt_sweeps, long *or_moves, int *rounds);
/* the descent of tspgpu_tour_local_search on slots slot0 .. slot0+count-1 at once: one Or-opt sweep launch and one apply
 * launch per round serve every tour still descending, and each slot ends exactly as tspgpu_tour_local_search would leave
 * it.  Per-slot outputs, [count] each (each may be NULL).  A slot of the range that holds no tour: 9, nothing is run.
 * Once the deadline passes: 4, every slot holding a valid tour and its cost. */
int tspgpu_tours_local_search(tspgpu_ctx *ctx, int slot0, int count, double time_left_s,
                              long *two_opt_sweeps, long *or_moves, int *rounds);
/* a measurement aid (tools/oropt_rate.py), the Or-opt counterpart of tspgpu_time_sweep: launch the Or-opt sweep kernel
 * alone `reps` times on slot (no move applied) and return its mean duration in ms from HIP events on the engine's stream */
int tspgpu_time_or_sweep(tspgpu_ctx *ctx, int slot, int reps, float *ms_mean);
/* Intra-sweep sharding ("optional, config 5": one sweep of a large instance split over
 * the GPUs of a node).  Every rank holds the same tour in `slot`; tspgpu_tour_sweep_part evaluates
 * the runs [part*G/nparts, (part+1)*G/nparts) of ONE sweep (refinment.c:49-69) and returns the best
 * pair found there (delta 0, a = b = 0: nothing improving in this part); after the ranks have
 * agreed on the minimum of (delta, a, b) -- one MIN all-reduce -- each applies it with
 * tspgpu_tour_apply_move (refinment.c:74-86,95-114), which also counts the sweep; a delta >= 0
 * marks the slot as locally optimal.  Both take the slot as it stands, whatever ran on it before: a sweep cap that an
 * earlier call reached (tspgpu_tour_two_opt with max_sweeps, ...) or a local optimum it found does not hold them back.
 * Symmetric matrices only. */
int tspgpu_tour_sweep_part(tspgpu_ctx *ctx, int slot, int part, int nparts, double *delta, int *a, int *b);
int tspgpu_tour_apply_move(tspgpu_ctx *ctx, int slot, int a, int b, double delta);
/* fetch slot's successor array / cost / last delta */
int tspgpu_tour_store(tspgpu_ctx *ctx, int slot, int *path, double *cost, double *last_delta);
/* launch the sweep kernel alone `reps` times on slot (no move applied) and
 * return its mean duration in ms from HIP events on the engine's stream */
int tspgpu_time_sweep(tspgpu_ctx *ctx, int slot, int reps, float *ms_mean);
/* same for the matrix build kernel */
int tspgpu_time_build(tspgpu_ctx *ctx, int reps, float *ms_mean);
/* with TSPGPU_OPT_TIMING: sum of sweep-kernel ms and launch count since reset */
int tspgpu_timing_read(tspgpu_ctx *ctx, double *sweep_ms_total, long *sweep_launches, int reset);
/* diagnostics: 64 wall-clock stamps (10 ns ticks) per sweep workgroup of the last launch
 * made while stamping was enabled (tools/stamps.py); not part of the reference's surface */
int tspgpu_debug_stamps(tspgpu_ctx *ctx, unsigned long long *out, int capacity_words);
/* diagnostics: the first `cells` cells of the tour-ordered matrix copy that the last LDS-resident
 * descent kept (row of node x, n cells: c[x][node at array cell q], the cell of x itself 16383);
 * tspgpu_info 68 tells whether the last LDS-resident descent kept it up to date; error 9
 * (failed precondition) when no descent has kept one yet */
int tspgpu_debug_tmat(tspgpu_ctx *ctx, unsigned short *out, size_t cells);
/* with TSPGPU_OPT_HISTORY: the recorded moves of slot 0; returns count in *count */
int tspgpu_history(tspgpu_ctx *ctx, int *a, int *b, double *delta, int capacity, int *count);

/* ---- Parallel-move 2-opt (an extension: the reference applies one move per sweep) ---------------------------------
 * A sweep keeps one candidate per tour edge and applies every candidate that beats all candidates it conflicts with.
 * Preconditions: `path` a successor array, a symmetric cost matrix (or matrix-free mode), n >= 5.
 *   1. Candidates.  For every node a, sa = path[a], every b, sb = path[b], the reference does not skip
 *      (src/algorithms/refinment.c:55: sa == sb || a == sb || b == sa):
 *          delta(a, b) = (c[a][b] + c[sa][sb]) - (c[a][sa] + c[b][sb])        (refinment.c:60-62, in this order)
 *      cand(a) = the first strict minimum over b ascending, a candidate only if delta < -1e-7 (TWO_OPT_EPS).  A candidate
 *      is the unordered pair {a, b} with the key (delta, lo, hi), lo < hi its labels; two nodes that choose each other
 *      give one candidate.  The smallest key is the move ref_2opt_once makes.
 *   2. Interval.  P(0) = 0, P(path[v]) = P(v) + 1; i = min(P(a), P(b)), j = max(P(a), P(b)): the candidate removes the
 *      edges at positions i and j and reverses the nodes at positions i + 1 .. j.  Position 0 never moves.
 *   3. Conflict.  Two different candidates conflict iff their closed ranges [i, j] intersect (shared edge, crossing, nesting).
 *   4. Selection.  ONE round: a candidate is accepted iff its key is below the key of every candidate it conflicts with.
 *      The smallest key is always accepted, so a sweep that finds an improving pair makes progress.
 *   5. Apply.  Every accepted {a, b}, P(a) < P(b): path[a] = b, the links of sa .. b reversed, path[sa] = sb.  *cost grows
 *      by the sum of the accepted deltas (exact for integer-valued costs; for other double cells the order of the sum is
 *      not specified).
 *   6. Descent.  *cost is recomputed from the matrix as ref_2opt does (refinment.c:6-9); sweeps run until one accepts
 *      nothing, and that last sweep is counted as in tspgpu_two_opt.  The result is a local optimum of the full 2-opt
 *      neighbourhood -- in general not the one tspgpu_two_opt reaches.
 * Taken: every instance tspgpu_two_opt takes with a symmetric matrix (one matrix row in LDS: no tighter limit) and
 * everything matrix-free mode takes.  Codes: no context 14, n < 5 3, no costs 9, an asymmetric matrix 9, a deadline that
 * passed 4 (with a valid tour and its cost; it is polled between sweeps).  The candidate arrays (40 bytes per node) are
 * allocated at the first call.
 * tspgpu_info: 36 / 37 sweeps / moves of the last parallel-move descent (or single sweep), 38 the most moves one of its
 * sweeps accepted, 39 / 40 tour positions / threads per workgroup of the candidate sweep on this instance (0: no
 * symmetric costs of at least 5 nodes), 41 the 16-byte vectors of a matrix row one of its threads holds (1, 2, 4 or 10; 0 in
 * matrix-free mode). */
/* one sweep on a host tour.  *cost is the caller's running cost (as ref_2opt_once, refinment.c:83).  The accepted moves
 * come back in ascending key order: moves_ab[2k], moves_ab[2k + 1] = a, b with P(a) < P(b), deltas[k]; *nmoves their
 * number (0: nothing improves).  More accepted moves than `cap`: 8, nothing is applied and nothing written. */
int tspgpu_two_opt_multi_once(tspgpu_ctx *ctx, int *path, double *cost, int *nmoves,
                              int *moves_ab /* [2*cap] */, double *deltas /* [cap] */, int cap);
/* the descent (rule 6); *sweeps and *moves (each may be NULL) the sweeps run and the moves applied */
int tspgpu_two_opt_multi(tspgpu_ctx *ctx, int *path, double *cost, double time_left_s, long *sweeps, long *moves);
/* the same on a slot, whose cost is taken as it stands: at most max_sweeps sweeps (< 0: until one accepts nothing).  The
 * slot's cost, last delta (the smallest accepted delta of the last sweep, 0: none) and sweep count follow, and every later
 * slot call sees the rewritten tour */
int tspgpu_tour_two_opt_multi(tspgpu_ctx *ctx, int slot, long max_sweeps, double time_left_s, long *sweeps, long *moves);
/* a measurement aid (tools/multi2opt_rate.py), the counterpart of tspgpu_time_or_sweep: the candidate sweep and the
 * selection `reps` times on slot, nothing applied; mean duration in ms from HIP events on the engine's stream */
int tspgpu_time_multi_sweep(tspgpu_ctx *ctx, int slot, int reps, float *ms_mean);

/* ---- Neighbour-list 2-opt (an extension: the candidates of a parallel-move sweep from K-nearest-neighbour lists) ------
 * A sweep evaluates at most 2 K pairs per node instead of all n, and then selects and applies as the section above does.
 * Preconditions: those of "Parallel-move 2-opt", and lists built for the cost source in place.
 *   Lists.  For 1 <= K <= 16, K' = min(K, n - 1): N(v) = the K' nodes u != v with the smallest key (c[v][u], u), in
 *      ascending key order.  Costs are compared exactly: as integers for uint16 / int32 cells and in matrix-free mode
 *      (whose weights are the ones matrix mode would hold), as doubles for f64 cells.
 *   Candidates (in place of rule 1 above; rules 2-5 -- interval, conflict, one selection round, apply -- are taken over
 *      unchanged).  For node a, sa = path[a]:
 *          B(a) = N(a) + { pred(x) : x in N(sa) }, minus every b the reference skips
 *                 (src/algorithms/refinment.c:55: sa == sb || a == sb || b == sa)
 *      delta(a, b) as in rule 1 (refinment.c:60-62, in this order: bit-exact for doubles); cand(a) = the lexicographic
 *      minimum of (delta(a, b), b) over B(a), a candidate only if delta < -1e-7.  Two nodes that choose each other give
 *      the pair once.
 *   Membership.  A pair {a, b} is in B(a) or B(b) iff one of its two new edges (a, b), (sa, sb) joins a node to a member of
 *      its own list, in either direction.
 *   Local optimum.  The descent ends in a tour with no improving 2-opt move of that kind: a local optimum of the
 *      neighbour-list neighbourhood, not of full 2-opt.
 *   Equality with the full rule.  With K' = n - 1 (n <= 17 at K = 16) B(a) is everything rule 1 looks at: a sweep equals a
 *      sweep of tspgpu_two_opt_multi_once move for move.
 *   Descent (rule 6 with these candidates).  *cost is recomputed as ref_2opt does (refinment.c:6-9); sweeps run until one
 *      accepts nothing, and that sweep is counted.  polish != 0: the parallel-move descent above then continues on the same
 *      slot, without recomputing the cost, until it accepts nothing -- the result is a local optimum of full 2-opt.
 * Codes: no context 14, n < 5 3, no costs 9, an asymmetric matrix 9, lists not built -- or invalidated by a later
 * tspgpu_build_costs, tspgpu_set_costs or tspgpu_set_points -- 9 with the reason in tspgpu_last_error, a deadline that
 * passed 4 (with a valid tour and its cost), more accepted moves than `cap` in _once 8 (nothing applied).
 * The lists (12 bytes per entry: node and weight) stay on the device and are allocated all or none.
 * tspgpu_info: 42 K' in effect (0: no lists), 43 / 44 sweeps / moves of the last neighbour-list phase (or single sweep),
 * 45 sweeps of the polish behind that phase (0: it had none -- only tspgpu_two_opt_nl polishes), 46 nodes per workgroup of the
 * candidate sweep. */
/* K in 1..16 builds the lists of the cost source in place; 0 drops them; any other K: 3 */
int tspgpu_neighbours_build(tspgpu_ctx *ctx, int K);
/* the lists, row v at nodes[v * K'] .. ; weights (may be NULL) the costs c[v][nodes[..]] */
int tspgpu_neighbours_get(tspgpu_ctx *ctx, int *nodes /* [n*K'] */, double *weights /* [n*K'] or NULL */);
/* one sweep on a host tour: arguments and results as tspgpu_two_opt_multi_once */
int tspgpu_two_opt_nl_once(tspgpu_ctx *ctx, int *path, double *cost, int *nmoves,
                           int *moves_ab /* [2*cap] */, double *deltas /* [cap] */, int cap);
/* the descent; *sweeps / *moves of the neighbour-list phase, *polish_sweeps / *polish_moves of the polish (0 without);
 * each may be NULL */
int tspgpu_two_opt_nl(tspgpu_ctx *ctx, int *path, double *cost, double time_left_s, int polish,
                      long *sweeps, long *moves, long *polish_sweeps, long *polish_moves);
/* neighbour-list sweeps on a slot, as tspgpu_tour_two_opt_multi (no polish) */
int tspgpu_tour_two_opt_nl(tspgpu_ctx *ctx, int slot, long max_sweeps, double time_left_s, long *sweeps, long *moves);
/* a measurement aid (tools/nl2opt_rate.py): the candidate sweep and the selection `reps` times on slot, nothing applied */
int tspgpu_time_nl_sweep(tspgpu_ctx *ctx, int slot, int reps, float *ms_mean);

/* ---- Neighbour-list Or-opt (an extension: Or-opt candidates from the neighbour lists, every independent move of a sweep) --
 * A sweep evaluates at most 10 K' segment moves per node instead of 5 n - 16, and applies every accepted one at once.
 * Preconditions: `path` a successor array, symmetric costs (a symmetric matrix, or matrix-free mode), n >= 8, lists built by
 * tspgpu_neighbours_build for the cost source in place (N(v), K' as in "Neighbour-list 2-opt").  No row-in-LDS limit beyond
 * that section's: every instance tspgpu_two_opt_nl takes with n >= 8 is taken.  These entry points run in matrix-free mode
 * without TSPGPU_OPT_OR_MATRIX_FREE (that option guards the entry points of "Or-opt", whose code 12 stays).
 *   1. Move and delta: exactly those of "Or-opt".  A candidate (s, L, q, rev), L in {1, 2, 3}; t is L - 1 steps after s,
 *      p = pred(s), x = path[t], q' = path[q]; q outside the segment and q != p (q = x is allowed); rev only for L >= 2;
 *      (h, e) = (s, t), or (t, s) when rev;
 *          delta = ((c[p][x] + c[q][h]) + c[e][q']) - ((c[p][s] + c[t][x]) + c[q][q'])      in this order: bit-exact for doubles
 *   2. Candidates of a segment start.  P(0) = 0, P(path[v]) = P(v) + 1.  A segment that contains node 0 is no candidate:
 *      node 0 is never moved by this rule (as position 0 never moves in "Parallel-move 2-opt").  For s, each L, each
 *      segment end w ({s} for L = 1, {s, t} otherwise) and each u in N(w), two forms:
 *          (A) q = u, h = w:                rev = [w == t], 0 for L = 1
 *          (B) q' = u, q = pred(u), e = w:  rev = [w == s], 0 for L = 1
 *      kept iff q is outside the segment and q != p; duplicates are harmless: at most 10 K' evaluations per node.
 *      cand(s) = the lexicographic minimum of (delta, L, q, rev) over these, a candidate only if delta < -1e-7.  Its key is
 *      (delta, s, L, q, rev), labels as node ids.
 *   3. Membership.  (s, L, q, rev) is looked at iff one of its two new edges (q, h), (e, q') joins a segment end to a member
 *      of that end's own list.  The closing edge (p, x) plays no part.
 *   4. Range.  The edge leaving the node at position k has position k (the edge into node 0: n - 1).  With i = P(s),
 *      j = P(q) the move removes the edges at positions i - 1, i + L - 1 and j; its range is
 *      [lo, hi] = [min(i - 1, j), max(i + L - 1, j)], and 0 <= lo < hi <= n - 1: no range wraps.  Only the nodes at
 *      positions lo + 1 .. hi change position: insertion behind the segment (j > i) shifts the nodes i + L .. j down by L,
 *      insertion in front (j < i - 1) shifts the nodes j + 1 .. i - 1 up by L.
 *   5. Conflict and selection.  Two candidates conflict iff their closed ranges intersect.  ONE round: a candidate is accepted
 *      iff its key is below the key of every candidate it conflicts with.  The smallest key is always accepted.
 *   6. Apply.  Every accepted move: path[p] = x, path[q] = h, the inner links of the segment reversed when rev,
 *      path[e] = q'.  *cost grows by the sum of the accepted deltas (exact for integer-valued costs; otherwise the order of
 *      the sum is not specified).  Disjoint ranges touch disjoint edges; two accepted moves may share one end node (the
 *      hi + 1 node of one, the lo node of the other).
 *   7. Or-opt phase.  Sweeps run until one accepts nothing; that sweep is counted.  The result has no improving move with
 *      the membership property whose segment avoids node 0.
 *   8. Descent (tspgpu_local_search_nl).  *cost is recomputed as ref_2opt does (src/algorithms/refinment.c:6-9); then the
 *      neighbour-list 2-opt phase (tspgpu_tour_two_opt_nl to its end, no polish) alternates with the Or-opt phase of rule 7
 *      until an Or-opt phase applies nothing.  *rounds counts the 2-opt phases.  The result is locally optimal for both
 *      list neighbourhoods; tspgpu_local_search on it reaches the full ones (there is no polish flag).
 *   9. Equality with the full rule.  With K' = n - 1 (n <= 17 at K = 16) the candidates of s are every (L, q, rev) rule 1
 *      allows: the smallest key of a sweep is the move tspgpu_or_opt_once makes, whenever that move's segment does not
 *      contain node 0.
 * Codes: no context 14, n < 8 3, no costs 9, an asymmetric matrix 9, lists not built or invalidated 9 (the text of
 * "Neighbour-list 2-opt"), more accepted moves than `cap` in _once 8 (nothing applied, nothing written), a deadline that
 * passed 4 (with a valid tour and its cost).  No new device memory: the candidate arrays of "Parallel-move 2-opt" serve.
 * tspgpu_info: 47 / 48 Or-opt sweeps / moves of the last call of this section (a descent: totals over its rounds), 49 the
 * most moves one of its sweeps accepted, 50 rounds of the last tspgpu_local_search_nl, 51 segment starts per workgroup of the
 * candidate sweep. */
/* one sweep on a host tour.  *cost is the caller's running cost.  The accepted moves come back in ascending key order:
 * moves[4k .. 4k + 3] = s, L, q, rev, deltas[k]; *nmoves their number (0: nothing improves) */
int tspgpu_or_opt_nl_once(tspgpu_ctx *ctx, int *path, double *cost, int *nmoves,
                          int *moves /* [4*cap] */, double *deltas /* [cap] */, int cap);
/* the Or-opt phase (rule 7) on a host tour; *cost is the caller's running cost, as tspgpu_or_opt takes it */
int tspgpu_or_opt_nl(tspgpu_ctx *ctx, int *path, double *cost, double time_left_s, long *sweeps, long *moves);
/* the same on a slot: at most max_sweeps sweeps (< 0: until one accepts nothing); the slot is left as tspgpu_tour_two_opt_nl
 * leaves one: cost, last delta (the smallest accepted delta of the last sweep, 0: none), and every later slot call sees the tour */
int tspgpu_tour_or_opt_nl(tspgpu_ctx *ctx, int slot, long max_sweeps, double time_left_s, long *sweeps, long *moves);
/* the descent (rule 8); the counters (each may be NULL) are totals over the rounds */
int tspgpu_local_search_nl(tspgpu_ctx *ctx, int *path, double *cost, double time_left_s,
                           long *two_opt_sweeps, long *two_opt_moves, long *or_sweeps, long *or_moves, int *rounds);
/* the same on a slot, whose cost is taken as it stands */
int tspgpu_tour_local_search_nl(tspgpu_ctx *ctx, int slot, double time_left_s,
                                long *two_opt_sweeps, long *two_opt_moves, long *or_sweeps, long *or_moves, int *rounds);
/* a measurement aid (tools/ornl_rate.py): the candidate sweep, the compaction and the selection `reps` times on slot,
 * nothing applied */
int tspgpu_time_or_nl_sweep(tspgpu_ctx *ctx, int slot, int reps, float *ms_mean);

/* ---- Neighbour-list 3-opt (an extension: pure 3-opt moves from the neighbour lists, every independent move of a sweep) ----
 * The moves "Or-opt" cannot reach: segment insertion of any length, the double reversal and the two mixed forms.  A sweep
 * evaluates 8 W^2 chains per node instead of all triples of edges, and applies every accepted move at once.
 * Preconditions: those of "Neighbour-list Or-opt" -- `path` a successor array, symmetric costs (a symmetric matrix, or
 * matrix-free mode), n >= 8, lists built by tspgpu_neighbours_build for the cost source in place.  Every entry point takes a
 * `width` in 1 .. 16 (any other value: 3); W = min(width, K'), and only the first W entries of a list are used.
 *   1. Positions.  P(0) = 0, P(path[v]) = P(v) + 1; o[p] is the node at position p.  The tour edge at position p joins o[p]
 *      and o[(p + 1) mod n].
 *   2. Move.  Three edge positions i < j < k; a = o[i], a' = o[i+1], b = o[j], b' = o[j+1], c = o[k], c' = o[(k+1) mod n];
 *      A = the nodes at i+1 .. j, B = the nodes at j+1 .. k.  The three edges are removed and the positions i+1 .. k refilled:
 *          kind 0:  A reversed, B reversed    adds (a,b)  (a',c)  (b',c')
 *          kind 1:  B, A                      adds (a,b') (c,a')  (b,c')
 *          kind 2:  B reversed, A             adds (a,c)  (b',a') (b,c')
 *          kind 3:  B, A reversed             adds (a,b') (c,b)   (a',c')
 *      The three reconnections that are single 2-opt moves are not moves of this rule.
 *   3. Chain and delta.  A candidate is written as a chain t1 .. t6: removed {t1,t2}, {t3,t4}, {t5,t6}, added {t2,t3},
 *      {t4,t5}, {t6,t1};
 *          delta = ((c[t2][t3] + c[t4][t5]) + c[t6][t1]) - ((c[t1][t2] + c[t3][t4]) + c[t5][t6])      in this order: bit-exact for doubles
 *   4. Candidates of t1.  For s2 in {0: t2 = succ(t1), 1: t2 = pred(t1)}, j3 < W with t3 = N(t2)[j3], s4 in {0, 1} with t4 =
 *      succ or pred of t3, j5 < W with t5 = N(t4)[j5], s6 in {0, 1} with t6 = succ or pred of t5 -- no gain pruning: 8 W^2
 *      evaluations per node.  A chain is kept iff (i) its three removed edges sit at three different positions, (ii) its
 *      added set is that of one of the four kinds for those positions taken in ascending order, compared by role (edge rank,
 *      tail or head) and not by label, and (iii) no added edge has two equal ends or is one of the removed edges as a node pair.
 *          code = 1 << 30 | s2 << 10 | j3 << 6 | s4 << 5 | j5 << 1 | s6
 *      cand(t1) = the lexicographic minimum of (delta, code), a candidate only if delta < -1e-7.  Its key is (delta, t1, code).
 *   5. Membership.  The move (i, j, k, kind) is looked at iff one of the writings of its alternating cycle as a chain (a start
 *      node and a direction whose first edge is a removed one) has t3 among the first W of N(t2) and t5 among the first W
 *      of N(t4).  Several writings may survive as candidates of different t1; they have the same range, conflict with each
 *      other, and exactly one of them is accepted.
 *   6. Range.  [i, k] with 0 <= i < k <= n - 1.  Only the nodes at the positions i+1 .. k change position; position 0 never
 *      moves and no range wraps.  Node 0 may be a (i = 0) and may be c' (k = n - 1).
 *   7. Conflict and selection.  Exactly rules 3-4 of "Parallel-move 2-opt": closed ranges that intersect conflict, ONE round,
 *      a candidate is accepted iff its key is below the key of every candidate it conflicts with.  The smallest key is
 *      always accepted.
 *   8. Apply.  Every accepted move at once: the order of i+1 .. k is that of the move's kind.  *cost grows by the sum of the
 *      accepted deltas (exact for integer-valued costs; summed by the fixed-shape tree of "Parallel-move 2-opt").  Two
 *      accepted moves may share one end node (the k + 1 node of one, the i node of the other).
 *   9. Phase.  Sweeps run until one accepts nothing; that sweep is counted.
 *  10. Descent (tspgpu_local_search_nl3).  *cost is recomputed as ref_2opt does (src/algorithms/refinment.c:6-9); the
 *      alternation of rule 8 of "Neighbour-list Or-opt" runs to its end (without a further recompute); the 3-opt phase runs;
 *      both repeat until a 3-opt phase applies nothing.  The tour, the cost and the five counters at the end of the first
 *      rule-8 part are exactly those of tspgpu_local_search_nl on the same input: the final cost is never above that one, and
 *      strictly below iff a 3-opt move was applied.
 *  11. Full lists.  With W = K' = n - 1 every move of rule 2 that passes rule 4's test (iii) is looked at.
 * Codes: no context 14, a width outside 1 .. 16 3, n < 8 3, no costs 9, an asymmetric matrix 9, lists not built or
 * invalidated 9 (the text of "Neighbour-list 2-opt"), more accepted moves than `cap` in _once 8 (nothing applied, nothing
 * written), a deadline that passed 4 (with a valid tour and its cost).  No new device memory: the candidate arrays of
 * "Parallel-move 2-opt" serve.
 * tspgpu_info: 62 the W in effect, 63 / 64 3-opt sweeps / moves of the last call of this section (a descent: totals over its
 * phases), 65 the most moves one of its sweeps accepted, 66 3-opt phases of the last tspgpu_local_search_nl3, 67 nodes per
 * workgroup of the candidate sweep.  (A descent also leaves 43-45 and 47-50 as "Neighbour-list Or-opt" describes them,
 * with totals over all its rule-8 parts.) */
/* one sweep on a host tour.  *cost is the caller's running cost.  The accepted moves come back in ascending key order:
 * moves[4m .. 4m + 3] = i, j, k, kind, deltas[m]; *nmoves their number (0: nothing improves) */
int tspgpu_three_opt_nl_once(tspgpu_ctx *ctx, int width, int *path, double *cost, int *nmoves,
                             int *moves /* [4*cap] */, double *deltas /* [cap] */, int cap);
/* the 3-opt phase (rule 9) on a host tour; *cost is the caller's running cost */
int tspgpu_three_opt_nl(tspgpu_ctx *ctx, int width, int *path, double *cost, double time_left_s, long *sweeps, long *moves);
/* the same on a slot: at most max_sweeps sweeps (< 0: until one accepts nothing); the slot is left as tspgpu_tour_or_opt_nl
 * leaves one */
int tspgpu_tour_three_opt_nl(tspgpu_ctx *ctx, int slot, int width, long max_sweeps, double time_left_s, long *sweeps, long *moves);
/* the descent (rule 10); the counters (each may be NULL) are totals over the whole descent, *rounds the list 2-opt phases,
 * *three_phases the 3-opt phases */
int tspgpu_local_search_nl3(tspgpu_ctx *ctx, int width, int *path, double *cost, double time_left_s,
                            long *two_opt_sweeps, long *two_opt_moves, long *or_sweeps, long *or_moves, int *rounds,
                            long *three_sweeps, long *three_moves, int *three_phases);
/* the same on a slot, whose cost is taken as it stands */
int tspgpu_tour_local_search_nl3(tspgpu_ctx *ctx, int slot, int width, double time_left_s,
                                 long *two_opt_sweeps, long *two_opt_moves, long *or_sweeps, long *or_moves, int *rounds,
                                 long *three_sweeps, long *three_moves, int *three_phases);
/* a measurement aid (tools/three_opt_nl_rate.py): the candidate sweep, the compaction and the selection `reps` times on slot,
 * nothing applied */
int tspgpu_time_three_nl_sweep(tspgpu_ctx *ctx, int slot, int width, int reps, float *ms_mean);

/* ---- Don't-look bits (an extension: the neighbour-list sweeps evaluate only the nodes near a changed edge; a kick on a slot) ----
 * A sweep of "Neighbour-list 2-opt", "Neighbour-list Or-opt" and "Neighbour-list 3-opt" evaluates every node.  With looks it
 * evaluates the nodes near an edge that changed since they were last evaluated without result.  Opt-in: no other entry point
 * changes.  "Unit v" is what a family's sweep evaluates for node v: cand(a) of "Neighbour-list 2-opt", cand(s) of rule 2 of
 * "Neighbour-list Or-opt", cand(t1) of rule 4 of "Neighbour-list 3-opt".  P is the position function of those sections.
 * Preconditions and codes of every _dl entry point: those of its plain counterpart.
 *   1. State.  Per slot three sets of awake nodes, A2, AO and A3, one per family (family 0, 1, 2).  A slot that has just been
 *      loaded (tspgpu_tour_load, tspgpu_tour_nn, every host-tour entry point) has every node awake in all three;
 *      tspgpu_tour_copy copies the sets; every slot call outside this section that can rewrite a tour leaves every node awake
 *      in all three.  A slot for which nothing was ever allocated counts as all awake.
 *   2. Looked units of a sweep of family f.  Q = { v : one of the nodes at the positions P(v), .., P(v) + fwd (mod n) is in
 *      A_f }, fwd = 0 for the 2-opt, 2 for Or-opt (a changed edge (t, x) reaches the units s whose segments end in t), 0 for
 *      the 3-opt.
 *   3. Candidates.  cand(v) is the family's own for v in Q and "none" for every other node.  Range, conflict, the one
 *      selection round, apply and the cost sum are the family's rules on those candidates, unchanged.
 *   4. The new set.  A_f' = carry + ends.  carry: for every unit with a candidate (delta < -1e-7), accepted or not, read on
 *      the tour as it stood before the apply -- 2-opt: a and succ(a) (after a reversal the same tour edge is keyed on its
 *      other end); Or-opt: the nodes s .. t of the candidate's segment; 3-opt: t1.  ends: for every accepted move the end
 *      nodes of its removed edges (4, 6 and 6 nodes: a, succ a, b, succ b; p, s, t, x, q, q'; t1 .. t6).  The other two
 *      families g: A_g' = A_g + ends.
 *   5. Count.  `looked` grows by |Q|.  A sweep with |Q| = n is a full sweep.
 *   6. Phase with looks, with a flag `closing`.  A_f empty on entry: closing == 0 runs no sweep and every counter stays 0;
 *      closing != 0 wakes every node of A_f, so one full sweep runs.  Otherwise sweeps run until one accepts nothing; that
 *      sweep is counted.  If it was full the phase ends.  If not: closing != 0 wakes every node of A_f and the phase goes on
 *      (a phase cut by max_sweeps at that sweep still wakes them); closing == 0 ends the phase.  At the end of a phase that
 *      neither max_sweeps nor the deadline cut, A_f is empty: a sweep that accepts nothing had no candidate, because the
 *      smallest key is always accepted.
 *   7. Consequences.  (a) A first sweep with every node awake is the plain sweep move for move.  (b) With closing != 0 a
 *      phase ends exactly where the plain phase's end condition holds: the family's plain _once call on the result accepts
 *      nothing.  (c) With closing == 0 the result is the classic approximation: a sleeping unit whose far side (the q, q' or
 *      t3 .. t6 part) changed is not looked at again.  (d) The trajectory is in general not the plain one, and the final cost
 *      may be higher or lower.
 *   8. Descent.  Rule 10 of "Neighbour-list 3-opt" with every phase a phase with looks and one `closing` for all of them;
 *      width == 0 means no 3-opt phase, which is rule 8 of "Neighbour-list Or-opt".  The host-tour form recomputes the cost
 *      first, as the plain one does; the slot form takes the cost as it stands.
 *   9. Kick.  tspgpu_tour_kick applies the move (i, j, k, kind 1) of rule 2 of "Neighbour-list 3-opt" -- B, A: the segment
 *      swap of mh_VNS's kick -- whatever its delta, 0 <= i < j < k <= n - 1.  The slot's cost grows by
 *          ((c[a][b'] + c[c][a']) + c[b][c']) - ((c[a][a'] + c[b][b']) + c[c][c'])                 in this order
 *      which is also the slot's last delta, and a, a', b, b', c, c' join A2, AO and A3.  It needs n >= 8 and symmetric costs
 *      (or matrix-free mode), and no lists.
 * Codes: no context 14; lists not built or invalidated 9 (the text of "Neighbour-list 2-opt"); n < 5 (2-opt) / n < 8 3; a
 * width outside 1 .. 16 (the descents: 0 .. 16) 3; a slot that holds no tour 9; bad kick positions 3; a node outside
 * 0 .. n - 1 in tspgpu_tour_wake 3 (nothing changed); a family outside 0 .. 2 3; a deadline that passed 4 (with a valid tour).
 * Memory: at the first call of this section 3 n bytes per slot (the sets; they grow with the slots) and 4 n bytes per
 * context (the queue of looked units), all of it or none.
 * tspgpu_info: 70 `looked` of the last call with looks (a descent: the total), 71 its full sweeps, 72 the largest |Q| of one
 * of its sweeps that was not full, 73 the most workgroups a queued sweep runs (each takes the units of tspgpu_info 46 / 51 /
 * 67 per pass and strides over Q).  The plain families' counters (43-45, 47-50, 63-66) are left by a _dl call as its plain
 * counterpart leaves them, with the _dl call's own sweeps and moves. */
/* count < 0: every node of the slot wakes in all three sets; else nodes[0 .. count) join them */
int tspgpu_tour_wake(tspgpu_ctx *ctx, int slot, const int *nodes, int count);
/* all three sets empty */
int tspgpu_tour_sleep(tspgpu_ctx *ctx, int slot);
/* the set of `family` (0 2-opt, 1 Or-opt, 2 3-opt): out[v] = 1 iff v is awake (may be NULL), *count their number (may be NULL) */
int tspgpu_tour_awake(tspgpu_ctx *ctx, int slot, int family, unsigned char *out /* [n] */, int *count);
/* rule 9 */
int tspgpu_tour_kick(tspgpu_ctx *ctx, int slot, int i, int j, int k);
/* the phase with looks (rule 6) of each family on a slot: at most max_sweeps sweeps (< 0: no cap); *sweeps, *moves and
 * *looked (each may be NULL) are totals over the phase */
int tspgpu_tour_two_opt_nl_dl(tspgpu_ctx *ctx, int slot, int closing, long max_sweeps, double time_left_s,
                              long *sweeps, long *moves, long *looked);
int tspgpu_tour_or_opt_nl_dl(tspgpu_ctx *ctx, int slot, int closing, long max_sweeps, double time_left_s,
                             long *sweeps, long *moves, long *looked);
int tspgpu_tour_three_opt_nl_dl(tspgpu_ctx *ctx, int slot, int width, int closing, long max_sweeps, double time_left_s,
                                long *sweeps, long *moves, long *looked);
/* the descent (rule 8) on a slot and on a host tour; the nine counters of tspgpu_tour_local_search_nl3, then the units
 * looked at and the full sweeps over the whole descent (each may be NULL) */
int tspgpu_tour_local_search_nl3_dl(tspgpu_ctx *ctx, int slot, int width, int closing, double time_left_s,
                                    long *two_opt_sweeps, long *two_opt_moves, long *or_sweeps, long *or_moves, int *rounds,
                                    long *three_sweeps, long *three_moves, int *three_phases, long *looked, long *full_sweeps);
int tspgpu_local_search_nl3_dl(tspgpu_ctx *ctx, int width, int closing, int *path, double *cost, double time_left_s,
                               long *two_opt_sweeps, long *two_opt_moves, long *or_sweeps, long *or_moves, int *rounds,
                               long *three_sweeps, long *three_moves, int *three_phases, long *looked, long *full_sweeps);

/* ---- Greedy-edge construction (an extension: the greedy-edge tour over the neighbour lists, built on the device) ----------
 * A second single-tour construction next to tspgpu_tour_nn: the usual start of list-based 2-opt / 3-opt with don't-look bits.
 * Opt-in: no other entry point changes.
 * Preconditions: those of "Neighbour-list 2-opt" -- costs or points in place, a symmetric matrix, lists built for the cost
 * source in place with K' = min(K, n - 1), n >= 5 -- without that section's row-in-LDS limit.
 *   1. Edges and keys.  An edge is an unordered pair {a, b}, a < b; its key is (c[a][b], a, b), compared lexicographically, the
 *      cost exactly as the lists compare it (integers for uint16 / int32 cells and in matrix-free mode, doubles for f64 cells).
 *      Keys are distinct, so the order is total.
 *   2. State.  A set S of accepted edges in which every node has degree <= 2 and which has no cycle: a set of paths
 *      ("fragments"); a node of degree 0 is a fragment of its own.  An edge {a, b} is valid if both ends have degree < 2 and a
 *      and b are not the two ends of the same fragment.
 *   3. Phase 1 (list edges).  E1 = { {v, u} : u in N(v) }, membership in either direction.  S is the result of the sequential
 *      greedy over E1: the edges in ascending key order, each accepted iff it is valid when it is reached.
 *   4. Phase 2 (joining).  E2 = all pairs of nodes that have degree < 2 after phase 1.  The same sequential greedy goes on over
 *      E2 in ascending key order until a single fragment covers all n nodes; the edge between its two ends closes the tour.
 *   5. Orientation.  The slot's order starts at node 0, and the successor of node 0 is the smaller-numbered of its two tour
 *      neighbours.  The slot is then initialised as a loaded tour is: dir = +1, the cost recomputed in node order as ref_2opt
 *      does (refinment.c:6-9), last delta 0, every node awake in all three sets of "Don't-look bits".
 *   6. Equality with plain greedy edge.  With K' = n - 1 (n <= 17 at K = 16) E1 is every pair, and the result is the textbook
 *      greedy-edge tour under the key order.
 *   7. Rounds.  The device computes S without sorting, in rounds of locally dominant edges: best(v) is the smallest key among the
 *      valid edges of the phase's edge set at v, a fragment's best the smaller of its two ends' bests, and an edge is accepted
 *      iff it is the best of both fragments it joins.  This is the sequential result: an accepted edge is smaller than every
 *      valid edge at the four ends of its two fragments, and whatever could block it in the sequential order would be such an
 *      edge.  The globally smallest valid edge is always accepted, so a phase has at most n - 1 rounds; the counters below count
 *      the rounds that accepted an edge.
 * Codes: no context 14; a null argument or a negative slot 3; n < 5 3; no costs 9; an asymmetric matrix 9; lists not built or
 * invalidated 9 (the text of "Neighbour-list 2-opt").
 * Memory: 80 n bytes per context at the first construction, all of it or none; dropped with the lists and with the instance.
 * tspgpu_info: 74 / 75 the rounds of phase 1 / phase 2 of the last construction, 76 the edges phase 1 accepted, 77 the free
 * nodes (degree < 2) entering phase 2. */
/* the greedy-edge tour straight into a slot, as tspgpu_tour_nn (the slot array grows on demand) */
int tspgpu_tour_greedy(tspgpu_ctx *ctx, int slot);
/* the same into host arrays (successor array and cost), slot 0 as scratch */
int tspgpu_greedy_tour(tspgpu_ctx *ctx, int *path /* [n] */, double *cost);

/* ---- Batched neighbour-list descent (an extension: the descent over the lists on a batch of tours, and the multi-start) ----
 * The descent of "Neighbour-list Or-opt" (rule 8) on many tours at once: every launch serves every tour of the batch that
 * is still descending.  For each tour of the batch the descent is exactly rule 8, run on that tour alone:
 *   1. the neighbour-list 2-opt phase runs until a sweep accepts nothing; that sweep is counted;
 *   2. the neighbour-list Or-opt phase runs until a sweep accepts nothing; that sweep is counted;
 *   3. 1 and 2 repeat until an Or-opt phase applies nothing.
 * Tours do not interact, and a tour's phases advance on the device without a host read in between, so the tours of a batch
 * need not be in the same phase.  Each slot ends exactly as tspgpu_tour_local_search_nl would leave it: the successor array,
 * the cost and the last delta as tspgpu_tour_store shows them, the five counters, and a slot that every later slot call can
 * use.  The cost is bit-equal for double cells as well: the accepted deltas of a sweep are summed by the same tree of fixed
 * shape.  Matrix mode (uint16, int32, f64 cells) and matrix-free mode; no TSPGPU_OPT_OR_MATRIX_FREE and no row-in-LDS limit
 * beyond that of "Neighbour-list 2-opt".
 * Preconditions: those of "Neighbour-list Or-opt" (symmetric costs, n >= 8, lists built for the cost source in place).
 * Memory: the candidate arrays of "Parallel-move 2-opt" (40 bytes per node) and a control block once per slot of the range,
 * and the list of live slots, allocated at the first batched call, all or none; a failure is 8 with the byte count in the text.
 * Codes: no context or handle 14, n < 8 3, no costs 9, an asymmetric matrix 9, lists not built or invalidated 9 (the text
 * of "Neighbour-list 2-opt"), a bad slot range 3, a slot of the range that holds no tour 9 (nothing is run), a deadline
 * that passed 4 (every slot a valid tour whose stored cost is that tour's cost).
 * tspgpu_info: 52 tours of the last batched list descent, 53 its sweep launches (a sweep of every live tour: four kernels),
 * 54 the most tours live in one launch, 55 workgroups per tour of the batched candidate sweep on this instance (0: none). */
/* the descent on slots slot0 .. slot0+count-1 at once; per-slot outputs, [count] each (each may be NULL) */
int tspgpu_tours_local_search_nl(tspgpu_ctx *ctx, int slot0, int count, double time_left_s,
                                 long *two_opt_sweeps, long *two_opt_moves, long *or_sweeps, long *or_moves, int *rounds);
/* tspgpu_multistart_local_search with this descent: the NN tour from every listed start (starts NULL: 0 .. nstarts-1), the
 * batched descent in chunks of TSPGPU_OPT_MAX_TOURS, the lowest final cost wins, ties to the earliest entry of `starts`
 * (strict <).  costs_out [nstarts] (may be NULL): every start's final cost in list order; the totals (each may be NULL) are
 * sums over the starts.  A TSPGPU_OPT_SWEEP_CAP other than -1 is refused with 3.  Once the deadline passes: 4, with the best
 * of the chunks begun so far (the entries of costs_out behind them are left as they were). */
int tspgpu_multistart_local_search_nl(tspgpu_ctx *ctx, const int *starts, int nstarts, double time_left_s,
                                      int *best_path, double *best_cost, int *best_start,
                                      long *total_two_opt_sweeps, long *total_two_opt_moves,
                                      long *total_or_sweeps, long *total_or_moves, double *costs_out);
/* tspgpu_neighbours_build on every device's context of a multi-device handle */
int tspgpu_multi_neighbours_build(tspgpu_multi *m, int K);
/* tspgpu_multistart_local_search_nl sharded as tspgpu_multi_multistart_local_search is (entry p of the list on device
 * p mod G, the same exchange) */
int tspgpu_multi_multistart_local_search_nl(tspgpu_multi *m, const int *starts, int nstarts, double time_left_s,
                                            int *best_path, double *best_cost, int *best_start,
                                            long *total_two_opt_sweeps, long *total_two_opt_moves,
                                            long *total_or_sweeps, long *total_or_moves);

/* ---- Neighbour-list VNS (an extension: W independent walks of "descent over the lists, incumbent, kicks" on the device) ----
 * mh_VNS's loop (metaheuristic.c:279-318) with the descent of "Neighbour-list Or-opt" (rule 8) in the place of ref_2opt, on
 * `walks` tours at once: every launch serves every walk that is still walking, and the incumbents, the kicks, the cost
 * recompute and the re-arming stay on the device -- no host read stands between two iterations of a walk.
 * For each walk w, alone and independent of the others, k iterations of the steps 1 to 3:
 *   1. Descent: rule 8 of "Neighbour-list Or-opt", exactly as tspgpu_local_search_nl runs it on that tour: the cost is
 *      recomputed first (refinment.c:6-9), then the list 2-opt phase and the list Or-opt phase alternate until an Or-opt
 *      phase applies nothing; the empty sweeps are counted.
 *   2. Incumbent: a local optimum whose cost is strictly below best_costs[w] becomes the incumbent, cost and successor
 *      array (src/tsp.c:669-676); trace[w][it] receives the local optimum's cost.
 *   3. Kicks: r = rand % 9 - 2 kicks (r <= 0: none), behind the last iteration too, as in mh_VNS and tspgpu_vns_search.
 *      A kick is the kick of tspgpu_vns_search (vns_kick, metaheuristic.c:344-409, :490-500).
 *   4. The numbers are the caller's, one stream per walk: walk w reads rand_values[w * nrand .. (w + 1) * nrand) in order and
 *      consumed[w] says how many it used.  A walk whose numbers run out inside a kick phase is left in front of that kick
 *      phase, exactly as tspgpu_vns_search leaves its single walk: its tour is the local optimum, kick_pending[w] = 1,
 *      iterations[w] is not advanced and consumed[w] counts up to the end of the previous kick phase.  The other walks run
 *      to their own end; the call returns 8 once every walk is finished or dry.  Calling again with fresh numbers for the
 *      dry walks continues each walk so that the result equals an uninterrupted run on the concatenated streams.
 *   5. The state between calls is per walk and in host arrays, like tspgpu_vns_search's: paths, iterations, kick_pending,
 *      best_paths and best_costs, all in and out.  A walk with iterations[w] == k at entry is left alone.
 *   6. The deadline is polled between groups of launches.  Once it has passed the call returns 4; every walk then holds a
 *      valid tour and that tour's cost, a consistent iterations[w], and kick_pending[w] = 1 only if the walk's descent has
 *      ended and its kicks have not run (0 otherwise).  A walk caught inside a descent is NOT promised to continue on the
 *      same trajectory when called again: the next call begins a new descent on the tour the deadline left.
 *   7. The state after a kick phase is that of a freshly loaded tour: exactly what tspgpu_tour_load of the kicked successor
 *      array would leave in the slot (the order array from node 0, direction +1, positions, successors, edge weights, cost
 *      and sweep counters of the load, its summation order for double cells included).  So every iteration equals
 *      tspgpu_tour_load + tspgpu_tour_local_search_nl on the kicked tour, bit for bit, for f64 cells too.
 * Matrix mode (uint16, int32, f64 cells) and matrix-free mode; no TSPGPU_OPT_OR_MATRIX_FREE.  The slots 0 .. walks-1 are
 * scratch, like slot 0 of the other host-array entry points; they hold the walks' tours afterwards.
 * Preconditions and codes: those of "Batched neighbour-list descent" -- no context 14, n < 8 3, no costs 9, an asymmetric
 * matrix 9, lists not built or invalidated 9 --, and walks <= 0, k < 0, nrand < 0, a NULL where an array is required or an
 * iterations[w] outside [0, k] 3, a paths[w] that is no n-cycle 3 (nothing is run).
 * Memory: beyond that of "Batched neighbour-list descent", per walk two int arrays of n (the second order array, the
 * incumbent), nrand ints, k doubles and a control block; all or none, a failure is 8 with the byte count in the text.
 * trace is indexed by the iteration, [walks][k]: a cell is written by the call in which that iteration's descent ends.
 * tspgpu_info: 56 walks of the last call, 57 iterations it completed (summed over the walks), 58 its sweep rounds launched
 * (a round: the four kernels of the batched descent and the step kernel), 59 the most walks live in one round, 60 walks
 * that ended dry. */
int tspgpu_vns_walks_nl(tspgpu_ctx *ctx, int walks, int k, double time_left_s,
                        int *paths /* [walks][n] in/out */, double *costs /* [walks] out: cost of paths[w] */,
                        const int *rand_values /* [walks][nrand] */, long nrand, long *consumed /* [walks] out */,
                        int *iterations /* [walks] in/out */, int *kick_pending /* [walks] in/out */,
                        int *best_paths /* [walks][n] in/out */, double *best_costs /* [walks] in/out */,
                        double *trace /* [walks][k] or NULL; only the iterations this call completes are written */,
                        long *totals /* [walks][6] or NULL: two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, rounds, kicks of this call */);

/* ---- Batched neighbour-list 3-opt (an extension: the descent with a 3-opt phase on a batch of tours, the multi-start, the walks) ----
 * The descent of "Neighbour-list 3-opt" (rule 10) on many tours at once, in the way of "Batched neighbour-list descent": every
 * launch serves every tour of the batch that is still descending.  For each tour of the batch the descent is exactly rule 10,
 * run on that tour alone with the slot's cost taken as it stands:
 *   1. the neighbour-list 2-opt phase runs until a sweep accepts nothing; that sweep is counted;
 *   2. the neighbour-list Or-opt phase runs until a sweep accepts nothing; that sweep is counted;
 *   3. 1 and 2 repeat until an Or-opt phase applies nothing: a part of rule 8 has ended;
 *   4. the neighbour-list 3-opt phase (rule 9, W = min(width, K')) runs until a sweep accepts nothing; that sweep is counted;
 *   5. 1 to 4 repeat until a 3-opt phase applies nothing.
 * Tours do not interact, and a tour's phases advance on the device without a host read in between.  At the close of a sweep
 * that accepted nothing (phase 0 = 2-opt, 1 = Or-opt, 2 = 3-opt): 0 -> 1;  1 -> 0 with rounds += 1 if the Or-opt phase applied
 * something, 1 -> 2 with three_phases += 1 if it applied nothing;  2 -> 0 with rounds += 1 if the 3-opt phase applied something
 * (a new part of rule 8 begins at its round 1, and `rounds` sums the rounds of the parts), and the descent ends behind a 3-opt
 * phase that applied nothing.  Each slot ends exactly as tspgpu_tour_local_search_nl3 would leave it: the successor array, the
 * cost (bit-equal for double cells as well: the same tree of fixed shape sums a sweep's accepted deltas) and the last delta as
 * tspgpu_tour_store shows them, the eight counters, and a slot that every later slot call can use.
 * Matrix mode (uint16, int32, f64 cells) and matrix-free mode.
 * Preconditions, memory and codes: those of "Batched neighbour-list descent" (the walks: of "Neighbour-list VNS"), and a width
 * outside 1 .. 16 is 3.
 * tspgpu_info: 52 .. 55 describe the last batched list descent of either kind; 78 the W in effect of the last batched list
 * descent (0: it had no 3-opt phase), 79 / 80 its 3-opt sweeps / moves summed over the tours, 81 the most moves one tour's
 * 3-opt sweep accepted. */
/* the descent on slots slot0 .. slot0+count-1 at once; per-slot outputs, [count] each (each may be NULL) */
int tspgpu_tours_local_search_nl3(tspgpu_ctx *ctx, int slot0, int count, int width, double time_left_s,
                                  long *two_opt_sweeps, long *two_opt_moves, long *or_sweeps, long *or_moves, int *rounds,
                                  long *three_sweeps, long *three_moves, int *three_phases);
/* tspgpu_multistart_local_search_nl with this descent: its chunks, its winner (strict <, ties to the earliest entry), its
 * refusal of a sweep cap and its deadline behaviour */
int tspgpu_multistart_local_search_nl3(tspgpu_ctx *ctx, int width, const int *starts, int nstarts, double time_left_s,
                                       int *best_path, double *best_cost, int *best_start,
                                       long *total_two_opt_sweeps, long *total_two_opt_moves,
                                       long *total_or_sweeps, long *total_or_moves,
                                       long *total_three_sweeps, long *total_three_moves, double *costs_out);
/* ... sharded as tspgpu_multi_multistart_local_search_nl is (entry p of the list on device p mod G, the same exchange) */
int tspgpu_multi_multistart_local_search_nl3(tspgpu_multi *m, int width, const int *starts, int nstarts, double time_left_s,
                                             int *best_path, double *best_cost, int *best_start,
                                             long *total_two_opt_sweeps, long *total_two_opt_moves,
                                             long *total_or_sweeps, long *total_or_moves,
                                             long *total_three_sweeps, long *total_three_moves);
/* tspgpu_vns_walks_nl with this descent in step 1: every rule of "Neighbour-list VNS" holds with rule 10 of "Neighbour-list
 * 3-opt" in the place of rule 8, so every iteration equals tspgpu_tour_load + tspgpu_tour_local_search_nl3 on the kicked tour,
 * bit for bit */
int tspgpu_vns_walks_nl3(tspgpu_ctx *ctx, int width, int walks, int k, double time_left_s,
                         int *paths /* [walks][n] in/out */, double *costs /* [walks] out: cost of paths[w] */,
                         const int *rand_values /* [walks][nrand] */, long nrand, long *consumed /* [walks] out */,
                         int *iterations /* [walks] in/out */, int *kick_pending /* [walks] in/out */,
                         int *best_paths /* [walks][n] in/out */, double *best_costs /* [walks] in/out */,
                         double *trace /* [walks][k] or NULL; only the iterations this call completes are written */,
                         long *totals /* [walks][9] or NULL: two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, rounds, kicks,
                                         three_sweeps, three_moves, three_phases of this call */);

/* ---- Batched don't-look bits (an extension: the descent with looks on a batch of tours, the multi-start, the walks) ----
 * Rule 8 of "Don't-look bits" on many tours at once, in the way of "Batched neighbour-list 3-opt": every launch serves every
 * tour of the batch that is still descending, and a tour's phases and its `closing` decisions advance on the device without a
 * host read in between.  Everything here is opt-in: no other entry point changes.
 *
 * Batch.  For each slot of the range, alone, tspgpu_tours_local_search_nl3_dl runs rule 8 of "Don't-look bits" from the slot's
 * three sets as they stand; width == 0: no 3-opt phase.  Each slot ends exactly as tspgpu_tour_local_search_nl3_dl with the same
 * width and closing leaves it: the successor array, the cost (bit-equal for double cells as well: the same tree of fixed
 * shape sums a sweep's accepted deltas), the last delta, the ten counters, the three sets as tspgpu_tour_awake shows them, and
 * a finished slot.  A phase whose set is empty and that does not close ends with no sweep counted and counts as a phase that
 * applied nothing, so `rounds` and `three_phases` are what the single-slot descent reports; a tour whose three sets are empty
 * ends within one sweep launch.  In a closing phase a sweep that accepted nothing and was not full wakes every node of the
 * phase's set, and the phase goes on with one full sweep.
 * A slot of the range whose host flag says "every node is awake" (a loaded, built or copied tour, and any slot another kind
 * of call has rewritten) has its sets filled first.  This entry point does not set that flag; the plain batched entry points
 * still do.
 *
 * Multi-start.  tspgpu_multistart_local_search_nl3_dl is tspgpu_multistart_local_search_nl3 with this descent: every start is
 * loaded all awake; the chunks, the winner (strict <, ties to the earliest entry), the refusal of a sweep cap and the deadline
 * behaviour are its; two more totals, `looked` and `full_sweeps`.  There is no sharded form.
 *
 * Walks.  tspgpu_vns_walks_nl3_dl takes the arguments of tspgpu_vns_walks_nl3 and `closing`.  Every rule of "Neighbour-list
 * VNS" holds, with two changes.  Step 1 is rule 8 of "Don't-look bits".  Rule 7 becomes: after a kick phase the slot is what
 * tspgpu_tour_load of the kicked successor array leaves (order from node 0, direction +1, cost recomputed in the load's
 * summation order), the three sets are equal, and they hold exactly the nodes v whose unordered pair {pred v, succ v} differs
 * between the local optimum in front of the kick phase and the tour behind it (one proper segment swap: its six end nodes).
 * A walk that enters in front of a descent (kick_pending == 0, or left there by a deadline) starts all awake.  A walk that
 * enters in front of a kick phase, and a dry walk resumed, takes its paths[w] as the local optimum.  So every iteration equals
 * tspgpu_tour_load + tspgpu_tour_sleep + tspgpu_tour_wake(D) + tspgpu_tour_local_search_nl3_dl on the kicked tour, bit for
 * bit, and a resumed dry walk equals the uninterrupted one.
 *
 * Codes: those of the plain counterparts and of "Don't-look bits" (a width outside 0 .. 16 is 3).
 * Memory beyond theirs: 4 n bytes of queue and one look-control block per slot of the range (and the sets of "Don't-look
 * bits"), all or none; 8 carries the byte count.  It is dropped where the batch's candidate arrays are dropped.
 * tspgpu_info: 82 `looked` of the last batched descent with looks, summed over its tours, 83 its full sweeps (summed), 84 the
 * largest |Q| of one of its sweeps that was not full (over the tours), 85 the workgroups per tour its queued sweep launches
 * on the instance in place, min(16, ceil(n / 4)) (each takes the units of tspgpu_info 46 / 51 / 67 per pass; 0: no instance
 * the descent takes). */
/* the descent on slots slot0 .. slot0+count-1 at once; per-slot outputs, [count] each (each may be NULL) */
int tspgpu_tours_local_search_nl3_dl(tspgpu_ctx *ctx, int slot0, int count, int width, int closing, double time_left_s,
                                     long *two_opt_sweeps, long *two_opt_moves, long *or_sweeps, long *or_moves, int *rounds,
                                     long *three_sweeps, long *three_moves, int *three_phases,
                                     long *looked, long *full_sweeps);
int tspgpu_multistart_local_search_nl3_dl(tspgpu_ctx *ctx, int width, int closing, const int *starts, int nstarts,
                                          double time_left_s, int *best_path, double *best_cost, int *best_start,
                                          long *total_two_opt_sweeps, long *total_two_opt_moves,
                                          long *total_or_sweeps, long *total_or_moves,
                                          long *total_three_sweeps, long *total_three_moves,
                                          long *total_looked, long *total_full_sweeps, double *costs_out);
int tspgpu_vns_walks_nl3_dl(tspgpu_ctx *ctx, int width, int closing, int walks, int k, double time_left_s,
                            int *paths /* [walks][n] in/out */, double *costs /* [walks] out: cost of paths[w] */,
                            const int *rand_values /* [walks][nrand] */, long nrand, long *consumed /* [walks] out */,
                            int *iterations /* [walks] in/out */, int *kick_pending /* [walks] in/out */,
                            int *best_paths /* [walks][n] in/out */, double *best_costs /* [walks] in/out */,
                            double *trace /* [walks][k] or NULL; only the iterations this call completes are written */,
                            long *totals /* [walks][11] or NULL: the nine of tspgpu_vns_walks_nl3, then looked, full sweeps */);

/* ---- Held-Karp lower bound (an extension: 1-trees in Boruvka rounds and the subgradient ascent over them, on the device) ----
 * What none of the sections above gives: a distance to a bound instead of tour against tour.  Opt-in: no other entry point
 * changes.
 * Preconditions: costs or points in place; an integral cost source (uint16 or int32 cells, or matrix-free mode; f64 cells
 * answer 12); a symmetric matrix; n >= 5.  No row-in-LDS limit, and the neighbour lists play no part.
 * Scale: S = 128.  The multipliers pi[v] are 64-bit integers in units of 1/S of a cost unit, at most 2^45 in magnitude.  All
 * arithmetic is exact, in 64-bit integers.
 *   1. Weights and keys.  w(a, b) = S c[a][b] + pi[a] + pi[b].  An edge is an unordered pair {a, b}, a < b; its key is
 *      (w(a, b), a, b), compared lexicographically.  Keys are distinct, so the order is total and every minimum below is unique.
 *   2. 1-tree T(pi).  The minimum spanning tree, under the key order, of the complete graph on the nodes 1 .. n - 1, and the two
 *      edges {0, u} with the smallest keys.  deg[v] is v's degree in T (deg[0] = 2), and
 *      L(pi) = sum of w(e) over T - 2 sum of pi[v].  ceil(L(pi) / S) is a lower bound on every tour of an integer instance, for
 *      any pi: a tour is a 1-tree, and its w-weight is S times its cost plus 2 sum pi.
 *   3. Ascent.  Inputs: an upper bound UB, integral, 0 <= UB, S UB < 2^40; iters >= 1; patience >= 1; starting multipliers
 *      (default all 0).  State h = 0, bad = 0, best = -infinity.  For it = 0 .. iters - 1:
 *        compute L and deg of T(pi);
 *        if L > best: best = L, pi* = pi, bad = 0; else bad += 1, and if bad >= patience: h += 1, bad = 0;
 *        g[v] = deg[v] - 2, q = sum g[v]^2; if q = 0 stop with reason 1 (T is a tour, and it is optimal);
 *        gap = S UB - L; if gap <= 0 stop with reason 2 (the bound has met the caller's upper bound);
 *        t = floor(((2 gap) >> h) / q); if t = 0 stop with reason 3;
 *        if some |pi[v] + t g[v]| > 2^45 stop with reason 5, nothing applied;
 *        pi[v] += t g[v].
 *      When the iterations run out the reason is 0.  A passed deadline is reason 4 and code 4, with the bound so far -- a
 *      success, as everywhere in this ABI; the clock is read every TSPGPU_OPT_BATCH iterations, and at least that many run.
 *      Results: bound = ceil(best / S); pi*; the iterations evaluated (the one that stopped included); the reason; on reason 1
 *      the tour T is, as a successor array: it starts at node 0 and the successor of 0 is the smaller-numbered of its two
 *      neighbours (rule 5 of "Greedy-edge construction").
 *   4. Rounds.  The device computes the tree of rule 2 without sorting, in Boruvka rounds: every node v >= 1 finds the smallest
 *      key among its edges to nodes u >= 1 of another component; every component takes the smallest of its nodes' keys; those
 *      edges are accepted; the components are merged and relabelled.  This is the tree of rule 2: the smallest key leaving a
 *      component is the smallest key of a cut, and under a total order the minimum spanning tree is unique and holds the
 *      smallest edge of every cut.  No cycle can form: along a chain of components that hook onto one another the keys strictly
 *      decrease unless two components chose the same edge, so the only cycle is such a mutual pair, which is one edge.  Every
 *      round at least halves the components: at most ceil(log2(n - 1)) rounds, all of them enqueued; the rounds after the last
 *      merge return at once.  The ascent has no read-back per iteration and none per round.
 * Codes: no context 14, every output untouched; a null required argument (weight; bound, iters_done, reason) 3; n < 5 3; no
 * costs 9; an asymmetric matrix 9; f64 cells 12; UB, iters, patience or a multiplier out of range 3; the state cannot be
 * allocated 8, all of it or none.
 * Memory: 68 n bytes per context (and 1.3 KB of slack) at the first 1-tree; dropped with the instance.
 * tspgpu_info: 86 the Boruvka rounds (those that accepted an edge) of the last 1-tree, 87 / 88 the iterations and the reason
 * of the last ascent, 89 its final h, 90 the nodes per workgroup of the scan, 91 the LDS bytes per workgroup of the scan of the
 * last 1-tree (of one_tree or of an ascent): 12 ld where the labels and the multipliers of all nodes are staged there (12 ld <=
 * 65536: n <= 5440), 0 where the scan reads them through L2, and 0 before any 1-tree. */
/* one 1-tree: pi NULL = all zero; edges [2n] (n pairs a < b, ascending by pair), degree [n], each may be NULL */
int tspgpu_one_tree(tspgpu_ctx *ctx, const long *pi, int *edges, int *degree, long *weight /* L(pi), units of 1/128 */);
/* the ascent of rule 3 */
int tspgpu_lower_bound(tspgpu_ctx *ctx, double upper, int iters, int patience, double time_left_s,
                       const long *pi_in /* NULL = zeros */, double *bound, long *pi_out /* [n] or NULL */,
                       int *path /* [n] or NULL: the tour on reason 1 */, int *iters_done, int *reason);

#ifdef __cplusplus
}
#endif
#endif /* TSPGPU_H */
