/*
 * tsp_algos.c -- the heuristic path of the reference (src/algorithms/refinment.c,
 * heuristics.c, metaheuristic.c) with its own signatures, running on the MI355X through
 * include/tspgpu.h.  Control flow, incumbent rules, error codes and deadline semantics follow
 * the reference (cited per function); the O(n^2) loops are device kernels.
 *
 * Which matrix a call runs on: `costs == tsp_inst.costs` selects the matrix that
 * tsp_compute_costs left resident on the device; any other pointer (the xstar-weighted
 * matrix of cplex_model.c:1176-1258) is uploaded into a context private to the calling
 * thread, so concurrent CPLEX callback threads never share device state.
 */
#include "tsp_model.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tspgpu.h"

/* Per-thread contexts for caller-supplied matrices.  A context holds a stream, an n x n matrix and tour slots
 * on the device, so its lifetime is managed: a pthread key destructor destroys it when its thread exits (CPLEX
 * tears its worker threads down after the solve), and whatever is still alive when the instance is freed goes in
 * tsp_gpu_release_threads().  The registry (mutex-protected list) is what makes the second path possible. */
#include <pthread.h>

typedef struct thread_ctx {
    tspgpu_ctx *gpu;
    struct thread_ctx *next;
    pthread_mutex_t use;        /* held by the owning thread for the duration of a device call, and by whoever destroys
                                   the context: tsp_gpu_release_threads() waits for a call in flight instead of freeing
                                   the context under it */
} thread_ctx;

static pthread_mutex_t reg_lock = PTHREAD_MUTEX_INITIALIZER;
static thread_ctx *reg_head = NULL;
static int reg_live = 0;
static pthread_key_t reg_key;
static pthread_once_t reg_once = PTHREAD_ONCE_INIT;

static void reg_unlink(thread_ctx *t)
{
    for (thread_ctx **pp = &reg_head; *pp; pp = &(*pp)->next)
        if (*pp == t) { *pp = t->next; reg_live--; break; }
}

static void thread_ctx_exit(void *arg)          /* runs in the exiting thread */
{
    thread_ctx *t = (thread_ctx *)arg;
    pthread_mutex_lock(&reg_lock);              /* (tsp_gpu_release_threads walks the list under this lock) */
    reg_unlink(t);
    pthread_mutex_unlock(&reg_lock);
    pthread_mutex_lock(&t->use);
    tspgpu_destroy(t->gpu);
    t->gpu = NULL;
    pthread_mutex_unlock(&t->use);
    pthread_mutex_destroy(&t->use);
    free(t);
}

static void reg_make_key(void) { pthread_key_create(&reg_key, thread_ctx_exit); }

int tsp_gpu_thread_contexts(void)
{
    pthread_mutex_lock(&reg_lock);
    const int live = reg_live;
    pthread_mutex_unlock(&reg_lock);
    return live;
}

/* destroys the contexts of threads that are still alive (waiting for a device call that one of them may be in); they
 * re-create theirs on the next call */
void tsp_gpu_release_threads(void)
{
    pthread_mutex_lock(&reg_lock);
    for (thread_ctx *t = reg_head; t; t = t->next) {
        pthread_mutex_lock(&t->use);
        if (t->gpu) tspgpu_destroy(t->gpu);
        t->gpu = NULL;
        pthread_mutex_unlock(&t->use);
    }
    pthread_mutex_unlock(&reg_lock);
}

/* the calling thread's context, LOCKED (thread_done() when the device call is over); NULL without a device */
static thread_ctx *thread_lease(void)
{
    pthread_once(&reg_once, reg_make_key);
    thread_ctx *t = (thread_ctx *)pthread_getspecific(reg_key);
    if (!t) {
        t = (thread_ctx *)calloc(1, sizeof *t);
        if (!t) return NULL;
        pthread_mutex_init(&t->use, NULL);
        pthread_setspecific(reg_key, t);
        pthread_mutex_lock(&reg_lock);
        t->next = reg_head; reg_head = t; reg_live++;
        pthread_mutex_unlock(&reg_lock);
    }
    pthread_mutex_lock(&t->use);
    if (!t->gpu) {
        const char *dev = getenv("TSP_GPU_DEVICE");
        if (tspgpu_create(dev ? atoi(dev) : 0, &t->gpu) != 0) { t->gpu = NULL; pthread_mutex_unlock(&t->use); return NULL; }
    }
    return t;
}

static void thread_done(thread_ctx *t) { if (t) pthread_mutex_unlock(&t->use); }

static double time_left(void)
{
    if (tsp_env.timelimit == -1.0) return -1.0;
    const double left = tsp_env.timelimit - utils_timeelapsed(&tsp_inst.c);
    return left > 0 ? left : 0.0;
}

static bool past_deadline(void)
{
    return tsp_env.timelimit != -1.0 && utils_timeelapsed(&tsp_inst.c) > tsp_env.timelimit;
}

/* Context holding `costs`.  The instance's own matrix lives in the process-wide context; any other pointer is a
 * caller matrix and is uploaded into the calling thread's context on EVERY call: the pointer says nothing about
 * the contents (cplex_model.c:1176-1258 refills one buffer per callback), so nothing is cached across calls. */
static tspgpu_ctx *ctx_for(double *costs, thread_ctx **lease)
{
    *lease = NULL;
    if (costs == tsp_inst.costs || (!costs && tsp_lazy_costs)) return tsp_gpu();
    thread_ctx *t = thread_lease();
    if (!t) return NULL;
    if (tspgpu_set_costs(t->gpu, costs, tsp_inst.nnodes) != 0) {
        log_error("tspgpu_set_costs: %s", tspgpu_last_error(t->gpu));
        thread_done(t);
        return NULL;
    }
    *lease = t;                                 /* held until thread_done(): the context cannot be destroyed under the call */
    return t->gpu;
}

static ERROR_CODE from_rc(int rc) { return (ERROR_CODE)rc; }

/* TSP_GPU_STATS=1: one JSON line per multi-start call on stderr (what bench.py's C-path leg parses) */
static void multi_stats(const char *what, struct tspgpu_multi *m, int starts, long sweeps, double seconds, double cost)
{
    const char *on = getenv("TSP_GPU_STATS");
    if (!on || !atoi(on)) return;
    static const char *kinds[] = {"none", "host", "rccl"};
    const int kind = m ? (int)tspgpu_multi_info(m, 2) : 0;
    fprintf(stderr, "tspgpu-stats: {\"call\": \"%s\", \"devices\": %d, \"exchange\": \"%s\", \"starts\": %d, \"sweeps\": %ld, "
                    "\"seconds\": %.6f, \"solve_s\": %.6f, \"exchange_s\": %.6f, \"rccl_init_s\": %.6f, \"best_cost\": %.2f}\n",
            what, m ? tspgpu_multi_devices(m) : 1, kinds[kind < 0 || kind > 2 ? 0 : kind], starts, sweeps, seconds,
            m ? tspgpu_multi_info(m, 5) : seconds, m ? tspgpu_multi_info(m, 4) : 0.0, m ? tspgpu_multi_info(m, 3) : 0.0, cost);
}

/* ===================================================================== refinment.c */

/* TSP_2OPT_MULTI=1 (tsp_run_algorithm): ref_2opt runs the parallel-move descent (tspgpu_two_opt_multi, an extension: a 2-opt
 * local optimum by another trajectory than the reference's) */
static int two_opt_multi_on = 0;
/* TSP_2OPT_NEIGHBOURS=K, K in 1..16 (tsp_run_algorithm): ref_2opt runs the neighbour-list descent over lists of K nodes
 * (tspgpu_two_opt_nl), followed by the parallel-move descent as a polish unless TSP_2OPT_NEIGHBOURS_POLISH=0.  It goes
 * before TSP_2OPT_MULTI. */
static int two_opt_nl_k = 0, two_opt_nl_polish = 1;

/* refinment.c:3-37.  Cost recompute, sweep loop and stop rule run on the device
 * (tspgpu_two_opt); the deadline is polled once per batch of sweeps instead of per sweep. */
ERROR_CODE ref_2opt(tsp_solution *solution, double *costs, bool update_incumbent)
{
    thread_ctx *lease;
    tspgpu_ctx *g = ctx_for(costs, &lease);
    if (!g) return UNAVAILABLE;
    ERROR_CODE e = T_OK;
    if (past_deadline()) {
        /* the reference recomputes the cost and leaves at the first poll */
        double c = 0;
        for (int i = 0; i < tsp_inst.nnodes; i++)
            c += costs ? costs[(size_t)i * tsp_inst.nnodes + solution->path[i]] : tsp_get_cost(i, solution->path[i]);   /* (a lazy host copy: tsp_get_cost) */
        solution->cost = c;
        log_debug("time limit exceeded in 2opt");
        e = DEADLINE_EXCEEDED;
    } else {
        int rc = -1;
        if (two_opt_nl_k) {
            /* the lists belong to the costs in place: built at the first call, and again behind every new matrix (ctx_for) */
            const int kp = two_opt_nl_k < tsp_inst.nnodes - 1 ? two_opt_nl_k : tsp_inst.nnodes - 1;
            rc = tspgpu_info(g, 42) == kp ? 0 : tspgpu_neighbours_build(g, two_opt_nl_k);
            if (rc == 0)
                rc = tspgpu_two_opt_nl(g, solution->path, &solution->cost, time_left(), two_opt_nl_polish, NULL, NULL, NULL, NULL);
            if (rc == FAILED_PRECONDITION || rc == RESOURCE_EXHAUSTED) {   /* an asymmetric matrix, a size limit: the tour is untouched */
                log_warn("TSP_2OPT_NEIGHBOURS=%d: %s; running tspgpu_two_opt", two_opt_nl_k, tspgpu_last_error(g));
                rc = -1;
            }
        } else if (two_opt_multi_on) {
            rc = tspgpu_two_opt_multi(g, solution->path, &solution->cost, time_left(), NULL, NULL);
            if (rc == FAILED_PRECONDITION || rc == RESOURCE_EXHAUSTED) {   /* an asymmetric matrix, a size limit: the tour is untouched */
                log_warn("TSP_2OPT_MULTI=1: %s; running tspgpu_two_opt", tspgpu_last_error(g));
                rc = -1;
            }
        }
        if (rc < 0) rc = tspgpu_two_opt(g, solution->path, &solution->cost, time_left(), NULL);
        if (rc != 0 && rc != DEADLINE_EXCEEDED) {
            log_error("tspgpu_two_opt: %s", tspgpu_last_error(g));
            thread_done(lease);
            return from_rc(rc);
        }
        e = from_rc(rc);
    }
    thread_done(lease);
    if (update_incumbent) {
        ERROR_CODE u = tsp_update_best_solution(solution);
        if (!err_ok(u)) log_error("code %d : Error in 2opt solution update", u);
    }
    return e;
}

/* refinment.c:39-93.  The return value is the best delta and has no room for an error: a device failure here is fatal
 * (log_fatal + tsp_handlefatal, what the reference does with errors it cannot return, tsp.c:738-742) -- returning 0
 * would make a caller that loops on the delta stop as if it had reached a local optimum. */
double ref_2opt_once(tsp_solution *solution, double *costs)
{
    thread_ctx *lease;
    tspgpu_ctx *g = ctx_for(costs, &lease);
    double delta = 0;
    if (!g || tspgpu_two_opt_once(g, solution->path, &solution->cost, &delta) != 0) {
        log_fatal("tspgpu_two_opt_once failed: %s", g ? tspgpu_last_error(g) : "no device");
        thread_done(lease);
        tsp_handlefatal();
    }
    thread_done(lease);
    return delta;
}

/* refinment.c:95-114: host utility kept for callers that own a prev[] array (vns / 3-opt moves) */
void ref_reverse_path(int a, int succ_a, int b, int succ_b, int *prev, int *path)
{
    path[a] = b;
    path[succ_a] = succ_b;
    for (int v = b; ; ) {
        const int back = prev[v];
        path[v] = back;
        if (back == succ_a) break;
        v = back;
    }
    for (int k = 0; k < tsp_inst.nnodes; k++) prev[path[k]] = k;
}

/* ===================================================================== heuristics.c */

/* heuristics.c:216-288 */
ERROR_CODE h_greedyutil(int starting_node, tsp_solution *solution, double *costs)
{
    if (!costs && !tsp_matrix_free && !tsp_lazy_costs) { log_error("matrix of costs not found"); return INTERNAL; }
    if (starting_node >= tsp_inst.nnodes || starting_node < 0) { log_error("starting node not correct"); return UNAVAILABLE; }
    if (past_deadline()) { log_warn("time limit exceeded in greedy util"); return DEADLINE_EXCEEDED; }
    thread_ctx *lease;
    tspgpu_ctx *g = ctx_for(costs, &lease);
    if (!g) return UNAVAILABLE;
    int rc = tspgpu_nn_tour(g, starting_node, solution->path, &solution->cost);
    if (rc) log_error("tspgpu_nn_tour: %s", tspgpu_last_error(g));
    thread_done(lease);
    return from_rc(rc);
}

/* TSP_GREEDY_EDGE_NEIGHBOURS=K (tsp_run_algorithm): h_Greedy builds the greedy-edge tour over neighbour lists of K nodes
 * (tspgpu_greedy_tour) instead of the nearest-neighbour tour; an extension, the reference has no such construction */
static int greedy_edge_k = 0;

static ERROR_CODE greedy_edge_tour(tsp_solution *solution)
{
    if (past_deadline()) { log_warn("time limit exceeded in the greedy-edge construction"); return DEADLINE_EXCEEDED; }
    thread_ctx *lease;
    tspgpu_ctx *g = ctx_for(tsp_inst.costs, &lease);
    if (!g) return UNAVAILABLE;
    /* the lists belong to the costs in place: built when the context holds none of that length */
    const int kp = greedy_edge_k < tsp_inst.nnodes - 1 ? greedy_edge_k : tsp_inst.nnodes - 1;
    int rc = tspgpu_info(g, 42) == kp ? 0 : tspgpu_neighbours_build(g, greedy_edge_k);
    if (rc == 0) rc = tspgpu_greedy_tour(g, solution->path, &solution->cost);
    if (rc) log_error("tspgpu_greedy_tour: %s", tspgpu_last_error(g));
    else log_debug("greedy-edge tour over lists of %d: %ld + %ld rounds, %ld list edges, %ld free nodes joined, cost %f", greedy_edge_k,
                   tspgpu_info(g, 74), tspgpu_info(g, 75), tspgpu_info(g, 76), tspgpu_info(g, 77), solution->cost);
    thread_done(lease);
    return from_rc(rc);
}

/* heuristics.c:12-32 */
ERROR_CODE h_Greedy(void)
{
    log_info(greedy_edge_k ? "running Greedy Edge" : "running Nearest Neighbour");
    tsp_solution s;
    tsp_init_solution(tsp_inst.nnodes, &s);
    ERROR_CODE e = greedy_edge_k ? greedy_edge_tour(&s) : h_greedyutil(tsp_inst.starting_node, &s, tsp_inst.costs);
    if (!err_ok(e)) log_error("code %d : greedy did not finish correctly", e);
    else {
        e = tsp_update_best_solution(&s);
        if (!err_ok(e)) log_error("code %d : error in updating solution for greedy", e);
    }
    free(s.path); free(s.comp);
    return e;
}

/* heuristics.c:34-72: every start on the device in one batch; the first strictly best wins */
ERROR_CODE h_Greedy_iterative(void)
{
    log_info("running All Nearest Neighbour");
    if (past_deadline()) return DEADLINE_EXCEEDED;
    tspgpu_ctx *g = tsp_gpu();
    if (!g) return UNAVAILABLE;
    struct tspgpu_multi *m = tsp_gpu_multi();
    tsp_solution s;
    tsp_init_solution(tsp_inst.nnodes, &s);
    int start = -1, done = 0;
    const double t0 = utils_timeelapsed(&tsp_inst.c);
    int rc = m ? tspgpu_multi_nn_all(m, NULL, tsp_inst.nnodes, time_left(), s.path, &s.cost, &start, &done)
               : tspgpu_nn_all_timed(g, NULL, tsp_inst.nnodes, time_left(), s.path, &s.cost, &start, &done);
    multi_stats("h_Greedy_iterative", m, tsp_inst.nnodes, 0, utils_timeelapsed(&tsp_inst.c) - t0, s.cost);
    ERROR_CODE e = from_rc(rc);
    if (rc && rc != DEADLINE_EXCEEDED) log_error("tspgpu_nn_all: %s", m ? tspgpu_multi_last_error(m) : tspgpu_last_error(g));
    else if (start >= 0 && s.cost < tsp_inst.best_solution.cost) {
        log_info("found new best, node %d", start);
        tsp_inst.starting_node = start;
        ERROR_CODE u = tsp_update_best_solution(&s);
        if (!err_ok(u)) log_error("code %d : error in updating best solution of greedy iterative", u);
    }
    free(s.path); free(s.comp);
    return e;
}

/* heuristics.c:74-116: NN + 2-opt from every start, batched on the device.  Without a time
 * limit the result equals the sequential loop exactly (minimum over the same set, ties to the
 * lowest start) and starting_node ends as the LAST start processed (:105-109). */
ERROR_CODE h_greedy_2opt(void)
{
    log_info("running All Nearest Neighbour + 2OPT");
    if (past_deadline()) { log_warn("time limit exceeded in greedy 2opt"); return DEADLINE_EXCEEDED; }
    tspgpu_ctx *g = tsp_gpu();
    if (!g) return UNAVAILABLE;
    tsp_solution s;
    tsp_init_solution(tsp_inst.nnodes, &s);
    int start = -1;
    long sweeps = 0;
    /* several devices (TSP_GPU_DEVICES): start i on device i mod G, one RCCL MIN all-reduce + one broadcast */
    struct tspgpu_multi *m = tsp_gpu_multi();
    const double t0 = utils_timeelapsed(&tsp_inst.c);
    int rc = m ? tspgpu_multi_multistart_nn_2opt(m, NULL, tsp_inst.nnodes, time_left(), s.path, &s.cost, &start, &sweeps)
               : tspgpu_multistart_nn_2opt(g, NULL, tsp_inst.nnodes, time_left(), s.path, &s.cost, &start, &sweeps, NULL, NULL);
    multi_stats("h_greedy_2opt", m, tsp_inst.nnodes, sweeps, utils_timeelapsed(&tsp_inst.c) - t0, s.cost);
    ERROR_CODE e = from_rc(rc);
    if (rc != 0 && rc != DEADLINE_EXCEEDED) {
        log_error("tspgpu_multistart_nn_2opt: %s", m ? tspgpu_multi_last_error(m) : tspgpu_last_error(g));
    } else {
        ERROR_CODE u = tsp_update_best_solution(&s);
        if (!err_ok(u)) log_error("code %d : Error in 2opt solution update", u);
        if (rc == 0) tsp_inst.starting_node = tsp_inst.nnodes - 1;
        else log_warn("time limit exceeded in greedy 2opt");
        log_debug("best start %d, cost %f, %ld sweeps", start, s.cost, sweeps);
    }
    free(s.path); free(s.comp);
    return e;
}

/* heuristics.c:118-149: caller's matrix and solution, no incumbent update; what is left in
 * *solution is the tour of the LAST start, as in the reference's loop */
ERROR_CODE h_Greedy_2opt_mod_costs(tsp_solution *solution, double *costs)
{
    if (past_deadline()) return DEADLINE_EXCEEDED;
    thread_ctx *lease;
    tspgpu_ctx *g = ctx_for(costs, &lease);
    if (!g) return UNAVAILABLE;
    const int n = tsp_inst.nnodes;
    int *best = (int *)malloc((size_t)n * sizeof(int));
    double best_cost = 0;
    int start = -1;
    int rc = tspgpu_multistart_nn_2opt(g, NULL, n, time_left(), best, &best_cost, &start, NULL, solution->path, &solution->cost);
    free(best);
    if (rc != 0 && rc != DEADLINE_EXCEEDED) log_error("tspgpu_multistart_nn_2opt: %s", tspgpu_last_error(g));
    thread_done(lease);
    return from_rc(rc);
}

/* heuristics.c:156-210.  The farthest pair (EM_MAX) and the insertion loop run on the device.  EM_RANDOM draws the pair
 * from the program's rand() stream exactly as the reference does; the draws with which the reference would read outside
 * its arrays or build a broken tour (A == n, B == n, A == B) -- and instances of fewer than 2 nodes -- return
 * INVALID_ARGUMENT with the incumbent untouched.  A deadline that passes before the last insertion returns
 * DEADLINE_EXCEEDED, also with the incumbent untouched (the reference's partial tour fails tsp_update_best_solution). */
ERROR_CODE h_ExtraMileage(void)
{
    log_info("running Extra Mileage");
    const int n = tsp_inst.nnodes;
    double max_distance = 0.0;
    int nodeA = 0, nodeB = 1;
    switch (tsp_env.mileage_init) {
    case EM_MAX:
        if (n >= 2) {
            tspgpu_ctx *g = tsp_gpu();
            if (!g) return UNAVAILABLE;
            const int rc = tspgpu_farthest_pair(g, &nodeA, &nodeB, &max_distance);
            if (rc != 0) { log_error("tspgpu_farthest_pair: %s", tspgpu_last_error(g)); return from_rc(rc); }
        }
        break;
    case EM_RANDOM:
        nodeA = tsp_rand() % (n + 1);
        nodeB = tsp_rand() % (n - nodeA + 1) + nodeA;
        break;
    default:
        log_warn("aborted");
        return ABORTED;
    }
    log_debug("max edge : (%d, %d) with distance %f", nodeA, nodeB, max_distance);
    if (n < 2 || nodeA >= n || nodeB >= n || nodeA == nodeB) {
        log_error("extra mileage: starting pair (%d, %d) is not two distinct nodes of the %d", nodeA, nodeB, n);
        return INVALID_ARGUMENT;
    }
    tsp_solution solution;
    tsp_init_solution(n, &solution);
    solution.cost = 2 * tsp_get_cost(nodeA, nodeB);
    solution.path[nodeA] = nodeB;
    solution.path[nodeB] = nodeA;
    log_debug("initial cost: %f", solution.cost);
    ERROR_CODE error = h_extramileage_util(&solution, nodeA, nodeB);
    if (error == T_OK) {
        ERROR_CODE u = tsp_update_best_solution(&solution);
        if (!err_ok(u)) log_error("code %d : error in updating solution for extra mileage", u);
    } else if (error == DEADLINE_EXCEEDED) {
        log_warn("time limit exceeded in extra mileage");
    }
    free(solution.path); free(solution.comp);
    return error;
}

/* heuristics.c:290-367: cheapest insertion from the pair (nodeA, nodeB) on the device.  As in the reference, the
 * deltas are ADDED to the caller's solution->cost (h_ExtraMileage starts it at 2 c(A, B)) and the successor array is
 * written into solution->path.  DEADLINE_EXCEEDED (checked before every insertion) leaves *solution untouched. */
ERROR_CODE h_extramileage_util(tsp_solution *solution, int nodeA, int nodeB)
{
    const int n = tsp_inst.nnodes;
    if (n < 2 || nodeA < 0 || nodeA >= n || nodeB < 0 || nodeB >= n || nodeA == nodeB) {
        log_error("extra mileage: starting pair (%d, %d) is not two distinct nodes of the %d", nodeA, nodeB, n);
        return INVALID_ARGUMENT;
    }
    if (past_deadline()) return DEADLINE_EXCEEDED;
    tspgpu_ctx *g = tsp_gpu();
    if (!g) return UNAVAILABLE;
    int *path = (int *)malloc((size_t)n * sizeof(int));
    if (!path) return RESOURCE_EXHAUSTED;
    double cost = 0;
    const int rc = tspgpu_extra_mileage(g, nodeA, nodeB, time_left(), path, &cost);
    if (rc == 0) {
        memcpy(solution->path, path, (size_t)n * sizeof(int));
        solution->cost += cost - 2 * tsp_get_cost(nodeA, nodeB);     /* the inserted deltas: integers, exact */
        log_debug("current cost: %f", solution->cost);
    } else if (rc == DEADLINE_EXCEEDED) {
        log_info("extra mileage: %s", tspgpu_last_error(g));      /* the device's count of the insertions made */
    } else {
        log_error("tspgpu_extra_mileage: %s", tspgpu_last_error(g));
    }
    free(path);
    return from_rc(rc);
}

/* ===================================================================== metaheuristic.c */

ERROR_CODE tabu_fixed_policy(tabu_search *t, int value)
{
    if (tsp_env.policy != POL_FIXED) { log_warn("policy has already been set"); return ALREADY_EXISTS; }
    t->tenure = value;
    return T_OK;
}

ERROR_CODE tabu_dependent_policy(tabu_search *t)
{
    if (tsp_env.policy != POL_SIZE) { log_warn("policy has already been set"); return ALREADY_EXISTS; }
    t->tenure = (int)ceil((t->max_tenure + t->min_tenure) / 2);
    return T_OK;
}

ERROR_CODE tabu_random_policy(tabu_search *t)
{
    if (tsp_env.policy != POL_RANDOM) { log_warn("policy has already been set"); return ALREADY_EXISTS; }
    t->tenure = (int)(tsp_rand() / RAND_MAX) * (t->max_tenure - t->min_tenure) + t->min_tenure;
    return T_OK;
}

ERROR_CODE tabu_linear_policy(tabu_search *ts)
{
    if (tsp_env.policy != POL_LINEAR) { log_warn("policy has already been set"); return ALREADY_EXISTS; }
    if (ts->tenure == ts->max_tenure || ts->tenure == ts->min_tenure) ts->increment = !ts->increment;
    ts->tenure += ts->increment ? 1 : -1;
    return T_OK;
}

ERROR_CODE tabu_init(tabu_search *ts, int nnodes)
{
    log_info("running Tabu Search");
    ts->tabu_list = (int *)malloc((size_t)nnodes * sizeof(int));
    for (int i = 0; i < nnodes; i++) ts->tabu_list[i] = -1;
    ts->increment = true;
    ts->tenure = MIN_FRACTION * nnodes + 1;
    ts->max_tenure = MAX_FRACTION * nnodes;
    ts->min_tenure = MIN_FRACTION * nnodes;
    return T_OK;
}

bool is_in_tabu_list(tabu_search *ts, int node, int it)
{
    return it - ts->tabu_list[node] < ts->tenure && ts->tabu_list[node] != -1;
}

void tabu_free(tabu_search *ts) { utils_safe_free(ts->tabu_list); }

/* metaheuristic.c:188-245: one tabu move on the device, host arrays in and out */
ERROR_CODE tabu_best_move(int *path, double *cost, tabu_search *ts, int it)
{
    tspgpu_ctx *g = tsp_gpu();
    if (!g) return UNAVAILABLE;
    int rc = tspgpu_tabu_move(g, path, cost, ts->tabu_list, ts->tenure, it);
    if (rc) log_error("tspgpu_tabu_move: %s", tspgpu_last_error(g));
    return from_rc(rc);
}

/* metaheuristic.c:86-186.  With the only reachable policy (linear: tsp.c:15, no flag selects
 * another) the whole k-iteration walk runs resident on the device; other policies step
 * through tabu_best_move.  As in the reference the loop does not stop at the deadline
 * (:118-123): it needs an explicit -k. */
ERROR_CODE mh_TabuSearch(void)
{
    tabu_search ts;
    if (!err_ok(tabu_init(&ts, tsp_inst.nnodes))) { log_fatal("Error in init tabu search"); tsp_handlefatal(); }
    ERROR_CODE e = h_greedy_2opt();
    if (!err_ok(e)) { log_fatal("code %d : Error in greedy solution computation", e); tsp_handlefatal(); }

    const int n = tsp_inst.nnodes;
    tsp_solution s;
    tsp_init_solution(n, &s);
    s.cost = tsp_inst.best_solution.cost;
    memcpy(s.path, tsp_inst.best_solution.path, (size_t)n * sizeof(int));

    const int k = tsp_env.k;
    if (k > 50000000) { log_error("Tabu Search needs an explicit -k (at most 5e7 iterations)"); free(s.path); free(s.comp); tabu_free(&ts); return INVALID_ARGUMENT; }
    FILE *f = fopen("results/TabuResults.dat", "w+");
    e = past_deadline() ? DEADLINE_EXCEEDED : T_OK;

    if (tsp_env.policy == POL_LINEAR) {
        tspgpu_ctx *g = tsp_gpu();
        tsp_solution best;
        tsp_init_solution(n, &best);
        double *trace = (double *)malloc((size_t)(k > 0 ? k : 1) * sizeof(double));
        int rc = tspgpu_tabu_search(g, s.path, &s.cost, k, best.path, &best.cost, trace);
        if (rc) { log_fatal("code %d : Error in tabu best move: %s", rc, tspgpu_last_error(g)); tsp_handlefatal(); }
        if (f) for (int i = 0; i < k; i++) fprintf(f, "%d,%f\n", i, trace[i]);
        ERROR_CODE u = tsp_update_best_solution(&best);
        if (!err_ok(u)) { log_fatal("code %d : Error in updating best solution", u); tsp_handlefatal(); }
        free(trace); free(best.path); free(best.comp);
    } else {
        for (int it = 0; it < k; it++) {
            ERROR_CODE p = tsp_env.policy == POL_FIXED ? tabu_fixed_policy(&ts, 30)
                         : tsp_env.policy == POL_RANDOM ? tabu_random_policy(&ts) : tabu_dependent_policy(&ts);
            if (!err_ok(p)) log_warn("using already set policy %d", tsp_env.policy);
            ERROR_CODE m = tabu_best_move(s.path, &s.cost, &ts, it);
            if (!err_ok(m)) { log_fatal("code %d : Error in tabu best move", m); tsp_handlefatal(); }
            ERROR_CODE u = tsp_update_best_solution(&s);
            if (!err_ok(u)) { log_fatal("code %d : Error in updating best solution", u); tsp_handlefatal(); }
            if (f) fprintf(f, "%d,%f\n", it, s.cost);
        }
    }
    if (f) fclose(f);
    free(s.path); free(s.comp);
    tabu_free(&ts);
    return e;
}

/* metaheuristic.c:344-409 + :490-500 (case 7).  Three tour positions from rand(); the
 * reference compares candidates with tour[idx-1] / tour[idx+1] without wrapping (:372).  On
 * glibc those out-of-range ints read 0 (chunk-size high word / calloc padding) except the
 * upper one when 4n+8 is a multiple of 16; the guards below hold those values so that the
 * rand() stream is consumed exactly as by the reference binary. */
ERROR_CODE vns_kick(tsp_solution *solution)
{
    log_debug("KICK");
    const int n = tsp_inst.nnodes;
    int *store = (int *)malloc((size_t)(n + 2) * sizeof(int));
    int *tour = store + 1;
    tour[-1] = 0;
    tour[n] = (n % 4 == 2) ? -2 : 0;
    for (int p = 0, v = 0; p < n; p++, v = solution->path[v]) tour[p] = v;

    int pick[3];
    for (int i = 0; i < 3; i++) {
        int r;
        do {
            r = tsp_rand() % n;
            for (int j = 0; j < i; j++)
                if (r == pick[j] || r == tour[pick[j] - 1] || r == tour[pick[j] + 1]) { r = -1; break; }
        } while (r == -1);
        pick[i] = r;
        for (int j = i; j > 0 && pick[j] < pick[j - 1]; j--) swap(&pick[j], &pick[j - 1]);
    }
    const int A = tour[pick[0]], sA = tour[(pick[0] + 1) % n];
    const int B = tour[pick[1]], sB = tour[(pick[1] + 1) % n];
    const int C = tour[pick[2]], sC = tour[(pick[2] + 1) % n];
    free(store);
    return tabu_make_move(NULL, solution, 7, A, sA, B, sB, C, sC);
}

/* metaheuristic.c:425-507.  Case 7 is the one the VNS kick uses; 1-3 are single reversals;
 * 4-6 reproduce the reference's two-step sequences (including their variable shuffles). */
ERROR_CODE tabu_make_move(int *prev, tsp_solution *solution, int bestCase, int i, int succ_i, int j, int succ_j,
                          int k, int succ_k)
{
    int *own = NULL;
    if (!prev && bestCase != 7) {
        own = (int *)malloc((size_t)tsp_inst.nnodes * sizeof(int));
        for (int v = 0; v < tsp_inst.nnodes; v++) own[solution->path[v]] = v;
        prev = own;
    }
    int t;
    switch (bestCase) {
    case 1: ref_reverse_path(k, succ_k, i, succ_i, prev, solution->path); break;
    case 2: ref_reverse_path(j, succ_j, k, succ_k, prev, solution->path); break;
    case 3: ref_reverse_path(i, succ_i, j, succ_j, prev, solution->path); break;
    case 4:
        ref_reverse_path(i, succ_i, j, succ_j, prev, solution->path);
        j = succ_i; succ_i = j;
        ref_reverse_path(j, succ_j, k, succ_k, prev, solution->path);
        break;
    case 5:
        ref_reverse_path(k, succ_k, i, succ_i, prev, solution->path);
        t = i; i = succ_k; succ_k = t;
        ref_reverse_path(i, succ_i, j, succ_j, prev, solution->path);
        break;
    case 6:
        ref_reverse_path(j, succ_j, k, succ_k, prev, solution->path);
        t = k; k = succ_j; succ_j = t;
        ref_reverse_path(k, succ_k, i, succ_i, prev, solution->path);
        break;
    case 7:
        solution->path[i] = succ_j;
        solution->path[k] = succ_i;
        solution->path[j] = succ_k;
        break;
    default: break;
    }
    free(own);
    return T_OK;
}

/* TSP_VNS_NEIGHBOURS=K, K in 1..16 (tsp_run_algorithm): mh_VNS runs TSP_VNS_WALKS walks of the neighbour-list VNS
 * (tspgpu_vns_walks_nl) over lists of K nodes instead of its own loop.
 * TSP_VNS_3OPT_WIDTH=W, W in 1..16, with it: the walks' descent gets the 3-opt phase over the first W entries (tspgpu_vns_walks_nl3).
 * TSP_VNS_DONT_LOOK=1, with TSP_VNS_NEIGHBOURS=K [and TSP_VNS_3OPT_WIDTH=W]: the walks run with don't-look bits
 * (tspgpu_vns_walks_nl3_dl; W = 0: no 3-opt phase), closing = 0 unless TSP_DONT_LOOK_CLOSING=1 */
static int vns_nl_k = 0, vns_nl_walks = 1, vns_nl_width3 = 0, vns_nl_dont_look = 0, batch_dl_closing = 0;
enum { VNS_NL_NUMBERS = 1 << 22 };              /* random numbers drawn ahead per call, over all walks */

/* mh_VNS over the neighbour lists.  Every walk starts from the tour in *best (the All-NN tour).  Per call at most C
 * iterations (W (32 C + 1024) <= 2^22) and 32 c + 1024 numbers per walk for the c <= C iterations it covers: block w of the numbers peeked from the program's glibc stream goes to walk w.
 * One walk consumes the stream as used, exactly like the loop below; more walks consume the whole peeked block, so a run is
 * deterministic for a seed, a walk count and k.  The calls are rebased (iterations counted from the slowest walk), so the
 * trace rows stay C cells long.  The winner is the lowest incumbent, ties to the lowest walk; f gets walk 0's trace. */
static ERROR_CODE vns_nl_loop(tsp_solution *best, FILE *f)
{
    tspgpu_ctx *g = tsp_gpu();
    if (!g) return UNAVAILABLE;
    const int n = tsp_inst.nnodes, W = vns_nl_walks, k = tsp_env.k;
    const int kp = vns_nl_k < n - 1 ? vns_nl_k : n - 1;
    int rc = tspgpu_info(g, 42) == kp ? 0 : tspgpu_neighbours_build(g, vns_nl_k);
    if (rc) { log_fatal("code %d : TSP_VNS_NEIGHBOURS=%d: %s", rc, vns_nl_k, tspgpu_last_error(g)); tsp_handlefatal(); }
    long C = W == 1 ? 16384 : (VNS_NL_NUMBERS / W - 1024) / 32;
    if (C < 1) C = 1;
    if (C > 16384) C = 16384;
    int *paths = (int *)malloc((size_t)W * n * sizeof(int)), *bests = (int *)malloc((size_t)W * n * sizeof(int));
    int *it = (int *)calloc((size_t)W, sizeof(int)), *itl = (int *)calloc((size_t)W, sizeof(int)), *pending = (int *)calloc((size_t)W, sizeof(int));
    double *costs = (double *)calloc((size_t)W, sizeof(double)), *bcosts = (double *)malloc((size_t)W * sizeof(double));
    long *used = (long *)calloc((size_t)W, sizeof(long));
    double *trace = f ? (double *)malloc((size_t)W * C * sizeof(double)) : NULL;
    if (!paths || !bests || !it || !itl || !pending || !costs || !bcosts || !used || (f && !trace)) {
        log_fatal("out of memory for %d walks", W); tsp_handlefatal();
    }
    for (int w = 0; w < W; w++) {
        memcpy(paths + (size_t)w * n, best->path, (size_t)n * sizeof(int));
        memcpy(bests + (size_t)w * n, best->path, (size_t)n * sizeof(int));
        bcosts[w] = best->cost;
    }
    ERROR_CODE e = T_OK;
    double shown = best->cost;
    for (;;) {
        int lo = it[0];
        for (int w = 1; w < W; w++) if (it[w] < lo) lo = it[w];
        if (lo >= k) break;
        if (past_deadline()) { e = DEADLINE_EXCEEDED; break; }
        const int kk = k - lo > C ? (int)C : k - lo;
        const long per = 32L * kk + 1024;
        for (int w = 0; w < W; w++) itl[w] = it[w] - lo;
        const int *rv = tsp_rand_peek(per * W);
        if (!rv) { log_fatal("out of memory for %ld random numbers", per * W); tsp_handlefatal(); }
        if (trace) for (long i = 0; i < (long)W * kk; i++) trace[i] = NAN;
        rc = vns_nl_dont_look
                 ? tspgpu_vns_walks_nl3_dl(g, vns_nl_width3, batch_dl_closing, W, kk, time_left(), paths, costs, rv, per, used, itl, pending, bests,
                                           bcosts, trace, NULL)
             : vns_nl_width3
                 ? tspgpu_vns_walks_nl3(g, vns_nl_width3, W, kk, time_left(), paths, costs, rv, per, used, itl, pending, bests, bcosts, trace, NULL)
                 : tspgpu_vns_walks_nl(g, W, kk, time_left(), paths, costs, rv, per, used, itl, pending, bests, bcosts, trace, NULL);
        tsp_rand_consume(W == 1 ? used[0] : per * W);
        /* RESOURCE_EXHAUSTED with progress: walks ran dry in front of a kick phase, come back with more (see mh_VNS) */
        int progress = 0;
        for (int w = 0; w < W; w++) { if (lo + itl[w] > it[w] || used[w] > 0) progress = 1; it[w] = lo + itl[w]; }
        const int refill = rc == RESOURCE_EXHAUSTED && progress;
        if (rc != 0 && rc != DEADLINE_EXCEEDED && !refill) {
            log_fatal("code %d : Error in the neighbour-list VNS: %s", rc, tspgpu_last_error(g));
            tsp_handlefatal();
        }
        for (int w = 0; w < W; w++) if (bcosts[w] < shown) shown = bcosts[w];
        if (shown < best->cost) { log_info("found new best: %f ", shown); best->cost = shown; }
        if (trace) for (int i = 0; i < kk; i++) if (!isnan(trace[i])) fprintf(f, "%d,%f\n", lo + i, trace[i]);
        if (rc == DEADLINE_EXCEEDED) { e = DEADLINE_EXCEEDED; break; }
    }
    int win = 0;
    for (int w = 1; w < W; w++) if (bcosts[w] < bcosts[win]) win = w;
    best->cost = bcosts[win];
    memcpy(best->path, bests + (size_t)win * n, (size_t)n * sizeof(int));
    free(paths); free(bests); free(it); free(itl); free(pending); free(costs); free(bcosts); free(used); free(trace);
    return e;
}

/* metaheuristic.c:251-341.  The loop -- local search, incumbent, r = rand() % 9 - 2 kicks -- runs on the device
 * (tspgpu_vns_search: inside the LDS-resident kernel where the instance allows it).  The random numbers stay the
 * program's: they are drawn here from the glibc stream (tsp_rand_peek), handed over in order, and what the device did
 * not use stays queued for the next draw, so the stream is consumed exactly as by the reference binary.  TSP_VNS_HOST=1
 * keeps the loop on the host (one ref_2opt call per iteration, vns_kick above). */
ERROR_CODE mh_VNS(void)
{
    log_info("running Variable Neighborhood Search");
    const int n = tsp_inst.nnodes;
    tsp_solution s, best;
    tsp_init_solution(n, &s);
    ERROR_CODE e = h_Greedy_iterative();
    if (!err_ok(e)) { log_fatal("code %d : Error in greedy", e); tsp_handlefatal(); }
    memcpy(s.path, tsp_inst.best_solution.path, (size_t)n * sizeof(int));
    s.cost = tsp_inst.best_solution.cost;
    tsp_init_solution(n, &best);
    best.cost = s.cost;
    memcpy(best.path, s.path, (size_t)n * sizeof(int));

    FILE *f = fopen("results/VNSResults.dat", "w+");
    e = T_OK;
    const char *on_host = getenv("TSP_VNS_HOST");
    if (vns_nl_k) e = vns_nl_loop(&best, f);
    else if ((on_host && atoi(on_host)) || two_opt_multi_on || two_opt_nl_k) {      /* (the resident loop's local search is the reference's descent) */
        for (int it = 0; it < tsp_env.k; it++) {
            if (past_deadline()) { e = DEADLINE_EXCEEDED; break; }
            e = ref_2opt(&s, tsp_inst.costs, true);
            if (!err_ok(e)) { log_fatal("code %d : Error in local search", e); tsp_handlefatal(); }
            if (s.cost < best.cost) {
                log_info("found new best: %f ", s.cost);
                best.cost = s.cost;
                memcpy(best.path, s.path, (size_t)n * sizeof(int));
            }
            if (f) fprintf(f, "%d,%f\n", it, s.cost);
            const int kicks = tsp_rand() % (UPPER - LOWER + 1) - LOWER;
            for (int j = 0; j < kicks; j++) vns_kick(&s);
        }
    } else {
        tspgpu_ctx *g = tsp_gpu();
        if (!g) return UNAVAILABLE;
        enum { CHUNK = 16384 };                     /* iterations per call: bounds the trace buffer and the numbers drawn ahead */
        double *trace = f ? (double *)malloc(CHUNK * sizeof(double)) : NULL;
        int it = 0, pending = 0;
        while (it < tsp_env.k) {
            if (past_deadline()) { e = DEADLINE_EXCEEDED; break; }
            const int upto = tsp_env.k - it > CHUNK ? it + CHUNK : tsp_env.k;
            const long want = 32L * (upto - it) + 1024;
            const int *rv = tsp_rand_peek(want);
            if (!rv) { log_fatal("out of memory for %ld random numbers", want); tsp_handlefatal(); }
            long used = 0;
            const int it0 = it;
            const double best0 = best.cost;
            const int rc = tspgpu_vns_search(g, s.path, &s.cost, upto, time_left(), rv, want, &used, &it, &pending, best.path, &best.cost, trace);
            tsp_rand_consume(used);
            /* RESOURCE_EXHAUSTED means "the numbers ran out in front of a kick phase: come back with more" only when the call
             * got somewhere (iterations done or numbers consumed: `want` covers far more than one kick phase).  The same code
             * with no progress is a real failure (the resident loop forced where it does not apply, a plan that does not
             * fit) and calling again would spin for ever */
            const int refill = rc == RESOURCE_EXHAUSTED && (it > it0 || used > 0);
            if (rc != 0 && rc != DEADLINE_EXCEEDED && !refill) {
                log_fatal("code %d : Error in local search: %s", rc, tspgpu_last_error(g));
                tsp_handlefatal();
            }
            if (best.cost < best0) log_info("found new best: %f ", best.cost);
            if (f && trace) for (int i = it0; i < it; i++) fprintf(f, "%d,%f\n", i, trace[i - it0]);
            if (rc == DEADLINE_EXCEEDED) { e = DEADLINE_EXCEEDED; break; }
        }
        free(trace);
    }
    if (f) fclose(f);
    ERROR_CODE u = tsp_update_best_solution(&best);
    if (!err_ok(u)) log_error("code %d : error in updating best solution of VNS", u);
    free(best.path); free(best.comp); free(s.path); free(s.comp);
    return e;
}

/* ===================================================================== Or-opt polish (an extension: no reference counterpart) */

/* 2-opt and Or-opt in turn until neither improves (tspgpu_local_search), on the instance's own matrix, under
 * tsp_env.timelimit.  DEADLINE_EXCEEDED leaves a valid tour and its cost in *solution, like ref_2opt. */
/* the codes with which tspgpu_local_search refuses an instance it is not built for (fewer than 8 nodes, rows past the LDS
 * limit, an asymmetric matrix, matrix-free mode): the tour is untouched */
static int or_opt_refusal(ERROR_CODE e)
{
    return e == INVALID_ARGUMENT || e == RESOURCE_EXHAUSTED || e == FAILED_PRECONDITION || e == UNIMPLEMENTED;
}

/* TSP_OR_OPT_NEIGHBOURS=K, K in 1..16 (tsp_run_algorithm): the polish runs the descent over neighbour lists of K nodes
 * (tspgpu_local_search_nl) instead of tspgpu_local_search; it takes a matrix-free instance as it is */
static int or_opt_nl_k = 0;
/* TSP_3OPT_WIDTH=W, W in 1..16 (tsp_run_algorithm), with the two switches above: that descent gets a neighbour-list 3-opt phase
 * over the first W list entries (tspgpu_local_search_nl3) */
static int three_opt_width = 0;
/* TSP_DONT_LOOK=1 (tsp_run_algorithm), with TSP_OR_OPT=1 and TSP_OR_OPT_NEIGHBOURS=K [and TSP_3OPT_WIDTH=W]: that descent runs
 * with don't-look bits and a closing full sweep per phase (tspgpu_local_search_nl3_dl, closing = 1; W = 0: no 3-opt phase) */
static int dont_look_on = 0;

ERROR_CODE tsp_or_opt_polish(tsp_solution *solution)
{
    if (!solution || !solution->path) return INVALID_ARGUMENT;
    thread_ctx *lease;
    tspgpu_ctx *g = ctx_for(tsp_inst.costs, &lease);
    if (!g) return UNAVAILABLE;
    long sweeps = 0, moves = 0;
    int rounds = 0;
    if (or_opt_nl_k) {
        /* the lists belong to the costs in place: built when the context holds none of that length */
        const int kp = or_opt_nl_k < tsp_inst.nnodes - 1 ? or_opt_nl_k : tsp_inst.nnodes - 1;
        long or_sweeps = 0, two_opt_moves = 0, three_sweeps = 0, three_moves = 0;
        int three_phases = 0;
        long looked = 0, full_sweeps = 0;
        const char *call = dont_look_on ? "tspgpu_local_search_nl3_dl" : three_opt_width ? "tspgpu_local_search_nl3" : "tspgpu_local_search_nl";
        int rc = tspgpu_info(g, 42) == kp ? 0 : tspgpu_neighbours_build(g, or_opt_nl_k);
        if (rc == 0 && dont_look_on)
            rc = tspgpu_local_search_nl3_dl(g, three_opt_width, 1, solution->path, &solution->cost, time_left(), &sweeps, &two_opt_moves,
                                            &or_sweeps, &moves, &rounds, &three_sweeps, &three_moves, &three_phases, &looked, &full_sweeps);
        else if (rc == 0 && three_opt_width)
            rc = tspgpu_local_search_nl3(g, three_opt_width, solution->path, &solution->cost, time_left(), &sweeps, &two_opt_moves, &or_sweeps,
                                         &moves, &rounds, &three_sweeps, &three_moves, &three_phases);
        else if (rc == 0)
            rc = tspgpu_local_search_nl(g, solution->path, &solution->cost, time_left(), &sweeps, &two_opt_moves, &or_sweeps, &moves, &rounds);
        if (or_opt_refusal(from_rc(rc))) log_warn("%s: %s", call, tspgpu_last_error(g));
        else if (rc != 0 && rc != DEADLINE_EXCEEDED) log_error("%s: %s", call, tspgpu_last_error(g));
        else if (dont_look_on && !three_opt_width)
            log_debug("Or-opt polish over lists of %d with don't-look bits: %d rounds, %ld 2-opt sweeps (%ld moves), %ld Or-opt sweeps (%ld moves), "
                      "%ld units looked at, %ld full sweeps, cost %f", or_opt_nl_k, rounds, sweeps, two_opt_moves, or_sweeps, moves, looked,
                      full_sweeps, solution->cost);
        else if (dont_look_on)
            log_debug("Or-opt polish over lists of %d with 3-opt over %d and don't-look bits: %d rounds, %ld 2-opt sweeps (%ld moves), %ld Or-opt "
                      "sweeps (%ld moves), %d 3-opt phases, %ld sweeps (%ld moves), %ld units looked at, %ld full sweeps, cost %f", or_opt_nl_k,
                      three_opt_width, rounds, sweeps, two_opt_moves, or_sweeps, moves, three_phases, three_sweeps, three_moves, looked, full_sweeps,
                      solution->cost);
        else if (three_opt_width)
            log_debug("Or-opt polish over lists of %d with 3-opt over %d: %d rounds, %ld 2-opt sweeps (%ld moves), %ld Or-opt sweeps (%ld moves), "
                      "%d 3-opt phases, %ld sweeps (%ld moves), cost %f", or_opt_nl_k, three_opt_width, rounds, sweeps, two_opt_moves, or_sweeps,
                      moves, three_phases, three_sweeps, three_moves, solution->cost);
        else log_debug("Or-opt polish over lists of %d: %d rounds, %ld 2-opt sweeps (%ld moves), %ld Or-opt sweeps (%ld moves), cost %f",
                       or_opt_nl_k, rounds, sweeps, two_opt_moves, or_sweeps, moves, solution->cost);
        thread_done(lease);
        return from_rc(rc);
    }
    const int rc = tspgpu_local_search(g, solution->path, &solution->cost, time_left(), &sweeps, &moves, &rounds);
    if (or_opt_refusal(from_rc(rc))) log_warn("tspgpu_local_search: %s", tspgpu_last_error(g));
    else if (rc != 0 && rc != DEADLINE_EXCEEDED) log_error("tspgpu_local_search: %s", tspgpu_last_error(g));
    else log_debug("Or-opt polish: %d rounds, %ld 2-opt sweeps, %ld Or-opt moves, cost %f", rounds, sweeps, moves, solution->cost);
    thread_done(lease);
    return from_rc(rc);
}

/* h_greedy_2opt with the 2-opt + Or-opt descent from EVERY start (tspgpu_multistart_local_search: the starts of a chunk
 * descend together), not only as a polish of the 2-opt winner; the incumbent, starting_node and the deadline are handled as
 * in h_greedy_2opt.  An instance the descent does not take (matrix-free, fewer than 8 nodes, rows past the LDS limit, an
 * asymmetric matrix) gets a warning and the plain h_greedy_2opt. */
ERROR_CODE h_greedy_local_search(void)
{
    log_info("running All Nearest Neighbour + 2OPT + Or-opt");
    if (past_deadline()) { log_warn("time limit exceeded in greedy local search"); return DEADLINE_EXCEEDED; }
    tspgpu_ctx *g = tsp_gpu();
    if (!g) return UNAVAILABLE;
    if (tsp_matrix_free) {
        log_warn("TSP_OR_OPT_EVERY_START=1: Or-opt needs the cost matrix and the instance runs matrix-free; running the plain multi-start");
        return h_greedy_2opt();
    }
    tsp_solution s;
    tsp_init_solution(tsp_inst.nnodes, &s);
    int start = -1;
    long sweeps = 0, moves = 0;
    struct tspgpu_multi *m = tsp_gpu_multi();
    const double t0 = utils_timeelapsed(&tsp_inst.c);
    int rc = m ? tspgpu_multi_multistart_local_search(m, NULL, tsp_inst.nnodes, time_left(), s.path, &s.cost, &start, &sweeps, &moves)
               : tspgpu_multistart_local_search(g, NULL, tsp_inst.nnodes, time_left(), s.path, &s.cost, &start, &sweeps, &moves, NULL);
    ERROR_CODE e = from_rc(rc);
    if (or_opt_refusal(e)) {
        log_warn("TSP_OR_OPT_EVERY_START=1: %s; running the plain multi-start", m ? tspgpu_multi_last_error(m) : tspgpu_last_error(g));
        free(s.path); free(s.comp);
        return h_greedy_2opt();
    }
    multi_stats("h_greedy_local_search", m, tsp_inst.nnodes, sweeps, utils_timeelapsed(&tsp_inst.c) - t0, s.cost);
    if (rc != 0 && rc != DEADLINE_EXCEEDED) {
        log_error("tspgpu_multistart_local_search: %s", m ? tspgpu_multi_last_error(m) : tspgpu_last_error(g));
    } else {
        ERROR_CODE u = tsp_update_best_solution(&s);
        if (!err_ok(u)) log_error("code %d : Error in local search solution update", u);
        if (rc == 0) tsp_inst.starting_node = tsp_inst.nnodes - 1;
        else log_warn("time limit exceeded in greedy local search");
        log_debug("best start %d, cost %f, %ld 2-opt sweeps, %ld Or-opt moves", start, s.cost, sweeps, moves);
    }
    free(s.path); free(s.comp);
    return e;
}

/* TSP_EVERY_START_NEIGHBOURS=K, K in 1..16 (tsp_run_algorithm): h_greedy_2opt with the descent over neighbour lists of K nodes
 * from EVERY start (tspgpu_multistart_local_search_nl: the starts of a chunk descend together, every launch serves all of them
 * that still descend).  It takes a matrix-free instance as it is; the incumbent, starting_node and the deadline are handled as
 * in h_greedy_2opt.  An instance the descent does not take (fewer than 8 nodes, an asymmetric matrix) gets a warning and the
 * plain h_greedy_2opt.
 * TSP_EVERY_START_3OPT_WIDTH=W, W in 1..16, with it: that descent gets the 3-opt phase over the first W list entries
 * (tspgpu_multistart_local_search_nl3).
 * TSP_EVERY_START_DONT_LOOK=1, with TSP_EVERY_START_NEIGHBOURS=K [and TSP_EVERY_START_3OPT_WIDTH=W]: every start descends with
 * don't-look bits (tspgpu_multistart_local_search_nl3_dl, on one device: it has no sharded form), closing = 0 unless
 * TSP_DONT_LOOK_CLOSING=1 */
static int every_start_nl_k = 0, every_start_width3 = 0, every_start_dont_look = 0;

ERROR_CODE h_greedy_local_search_nl(void)
{
    log_info("running All Nearest Neighbour + neighbour-list 2OPT + Or-opt");
    if (past_deadline()) { log_warn("time limit exceeded in greedy neighbour-list local search"); return DEADLINE_EXCEEDED; }
    tspgpu_ctx *g = tsp_gpu();
    if (!g) return UNAVAILABLE;
    struct tspgpu_multi *m = every_start_dont_look ? NULL : tsp_gpu_multi();
    tsp_solution s;
    tsp_init_solution(tsp_inst.nnodes, &s);
    int start = -1;
    long sweeps = 0, two_opt_moves = 0, or_sweeps = 0, moves = 0, three_sweeps = 0, three_moves = 0, looked = 0, full_sweeps = 0;
    const int w3 = every_start_width3;
    const double t0 = utils_timeelapsed(&tsp_inst.c);
    /* the lists belong to the costs in place: built when the context holds none of that length */
    const int kp = every_start_nl_k < tsp_inst.nnodes - 1 ? every_start_nl_k : tsp_inst.nnodes - 1;
    int rc = m ? tspgpu_multi_neighbours_build(m, every_start_nl_k)
               : tspgpu_info(g, 42) == kp ? 0 : tspgpu_neighbours_build(g, every_start_nl_k);
    if (rc == 0 && every_start_dont_look)
        rc = tspgpu_multistart_local_search_nl3_dl(g, w3, batch_dl_closing, NULL, tsp_inst.nnodes, time_left(), s.path, &s.cost, &start, &sweeps,
                                                   &two_opt_moves, &or_sweeps, &moves, &three_sweeps, &three_moves, &looked, &full_sweeps, NULL);
    else if (rc == 0 && w3)
        rc = m ? tspgpu_multi_multistart_local_search_nl3(m, w3, NULL, tsp_inst.nnodes, time_left(), s.path, &s.cost, &start, &sweeps,
                                                          &two_opt_moves, &or_sweeps, &moves, &three_sweeps, &three_moves)
               : tspgpu_multistart_local_search_nl3(g, w3, NULL, tsp_inst.nnodes, time_left(), s.path, &s.cost, &start, &sweeps, &two_opt_moves,
                                                    &or_sweeps, &moves, &three_sweeps, &three_moves, NULL);
    else if (rc == 0)
        rc = m ? tspgpu_multi_multistart_local_search_nl(m, NULL, tsp_inst.nnodes, time_left(), s.path, &s.cost, &start, &sweeps,
                                                         &two_opt_moves, &or_sweeps, &moves)
               : tspgpu_multistart_local_search_nl(g, NULL, tsp_inst.nnodes, time_left(), s.path, &s.cost, &start, &sweeps, &two_opt_moves,
                                                   &or_sweeps, &moves, NULL);
    ERROR_CODE e = from_rc(rc);
    if (or_opt_refusal(e)) {
        log_warn("TSP_EVERY_START_NEIGHBOURS=%d: %s; running the plain multi-start", every_start_nl_k,
                 m ? tspgpu_multi_last_error(m) : tspgpu_last_error(g));
        free(s.path); free(s.comp);
        return h_greedy_2opt();
    }
    multi_stats("h_greedy_local_search_nl", m, tsp_inst.nnodes, sweeps + or_sweeps + three_sweeps, utils_timeelapsed(&tsp_inst.c) - t0, s.cost);
    if (rc != 0 && rc != DEADLINE_EXCEEDED) {
        log_error("tspgpu_multistart_local_search_nl: %s", m ? tspgpu_multi_last_error(m) : tspgpu_last_error(g));
    } else {
        ERROR_CODE u = tsp_update_best_solution(&s);
        if (!err_ok(u)) log_error("code %d : Error in neighbour-list local search solution update", u);
        if (rc == 0) tsp_inst.starting_node = tsp_inst.nnodes - 1;
        else log_warn("time limit exceeded in greedy neighbour-list local search");
        log_debug("best start %d, cost %f, %ld 2-opt sweeps (%ld moves), %ld Or-opt sweeps (%ld moves), %ld 3-opt sweeps (%ld moves)", start,
                  s.cost, sweeps, two_opt_moves, or_sweeps, moves, three_sweeps, three_moves);
        if (every_start_dont_look) log_debug("with don't-look bits: %ld units looked at, %ld full sweeps", looked, full_sweeps);
    }
    free(s.path); free(s.comp);
    return e;
}

/* TSP_OR_OPT (1 = polish the incumbent after the heuristic), TSP_OR_OPT_EVERY_START (1 = -alg 2OPT_GREEDY runs
 * h_greedy_local_search) and TSP_OR_OPT_MATRIX_FREE (1 = the TSP_OR_OPT polish also runs on a matrix-free instance,
 * TSPGPU_OPT_OR_MATRIX_FREE), TSP_2OPT_MULTI (1 = ref_2opt, and with it every iteration of mh_VNS's host loop, runs the
 * parallel-move descent tspgpu_two_opt_multi): unset or 0 = off; anything else is an error (-1).  TSP_OR_OPT_NEIGHBOURS=K
 * (env_neighbours) makes the TSP_OR_OPT polish the descent over neighbour lists of K nodes, on a matrix-free instance too */
static int env_switch(const char *name)
{
    const char *v = getenv(name);
    if (!v || !strcmp(v, "0")) return 0;
    if (!strcmp(v, "1")) return 1;
    fprintf(stderr, "tsp: %s=\"%s\": expected 0 or 1\n", name, v);     /* (shown under -q too: a mistyped switch must not pass silently) */
    return -1;
}

/* TSP_2OPT_NEIGHBOURS, TSP_OR_OPT_NEIGHBOURS, and TSP_3OPT_WIDTH, TSP_EVERY_START_3OPT_WIDTH, TSP_VNS_3OPT_WIDTH (the part of a
 * list the 3-opt chains use: in the TSP_OR_OPT polish, in the multi-start over the lists, in the walks over the lists): unset or 0 = off,
 * 1..16 = the list length; anything else is an error (-1) */
static int env_neighbours(const char *name)
{
    const char *v = getenv(name);
    if (!v) return 0;
    char *end = NULL;
    const long k = strtol(v, &end, 10);
    if (*v && !*end && k >= 0 && k <= 16) return (int)k;
    fprintf(stderr, "tsp: %s=\"%s\": expected a list length from 1 to 16 (or 0: off)\n", name, v);
    return -1;
}

/* TSP_LOWER_BOUND=<iters>: after the algorithm has finished, the Held-Karp ascent (tspgpu_lower_bound, an extension) runs that many
 * iterations with the incumbent's cost as the upper bound, on the process-wide context (device 0's when several are configured).
 * Unset or 0 = off, 1..100000 = the iterations; anything else is an error (-1) */
static int env_lower_bound(void)
{
    const char *v = getenv("TSP_LOWER_BOUND");
    if (!v) return 0;
    char *end = NULL;
    const long k = strtol(v, &end, 10);
    if (*v && !*end && k >= 0 && k <= 100000) return (int)k;
    fprintf(stderr, "tsp: TSP_LOWER_BOUND=\"%s\": expected an iteration count from 1 to 100000 (or 0: off)\n", v);
    return -1;
}

/* one line on stderr (and one more under TSP_GPU_STATS=1); the solution, the exit code and every other output stay as they are */
static void lower_bound_report(int iters)
{
    tspgpu_ctx *g = tsp_gpu();
    if (!g) { fprintf(stderr, "tsp: TSP_LOWER_BOUND: no device context\n"); return; }
    const double cost = tsp_inst.best_solution.cost, t0 = utils_timeelapsed(&tsp_inst.c);
    double bound = 0;
    int done = 0, reason = 0;
    const int rc = tspgpu_lower_bound(g, cost, iters, 10, -1.0, NULL, &bound, NULL, NULL, &done, &reason);
    if (rc != 0 && rc != 4) { fprintf(stderr, "tsp: TSP_LOWER_BOUND: the bound was not computed (code %d: %s)\n", rc, tspgpu_last_error(g)); return; }
    const double gap = bound > 0 ? (cost - bound) / bound : 0.0, secs = utils_timeelapsed(&tsp_inst.c) - t0;
    fprintf(stderr, "tsp: lower bound %.0f after %d iterations (reason %d), gap %.4f %%\n", bound, done, reason, 100.0 * gap);
    const char *on = getenv("TSP_GPU_STATS");
    if (on && atoi(on))
        fprintf(stderr, "tspgpu-stats: {\"call\": \"lower_bound\", \"bound\": %.0f, \"iterations\": %d, \"reason\": %d, \"gap\": %.6f, "
                        "\"seconds\": %.6f, \"best_cost\": %.2f}\n", bound, done, reason, gap, secs, cost);
}

static ERROR_CODE run_algorithm(void);

/* ===================================================================== main.c:4-87 */
ERROR_CODE tsp_run_algorithm(void)
{
    const int lb_iters = env_lower_bound();
    if (lb_iters < 0) return INVALID_ARGUMENT;
    const ERROR_CODE e = run_algorithm();
    if (lb_iters && (e == T_OK || e == DEADLINE_EXCEEDED)) lower_bound_report(lb_iters);
    return e;
}

static ERROR_CODE run_algorithm(void)
{
    const int polish = env_switch("TSP_OR_OPT"), every_start = env_switch("TSP_OR_OPT_EVERY_START");
    const int polish_mf = env_switch("TSP_OR_OPT_MATRIX_FREE");
    const int multi = env_switch("TSP_2OPT_MULTI");
    const int nl_k = env_neighbours("TSP_2OPT_NEIGHBOURS"), or_nl_k = env_neighbours("TSP_OR_OPT_NEIGHBOURS");
    const char *nl_polish_set = getenv("TSP_2OPT_NEIGHBOURS_POLISH");
    const int nl_polish = nl_polish_set ? env_switch("TSP_2OPT_NEIGHBOURS_POLISH") : 1;
    if (polish < 0 || every_start < 0 || polish_mf < 0 || multi < 0 || nl_k < 0 || nl_polish < 0 || or_nl_k < 0) return INVALID_ARGUMENT;
    if (or_nl_k && nl_k && or_nl_k != nl_k) {       /* a context holds one set of lists */
        fprintf(stderr, "tsp: TSP_OR_OPT_NEIGHBOURS=%d and TSP_2OPT_NEIGHBOURS=%d: the two list lengths must be equal\n", or_nl_k, nl_k);
        return INVALID_ARGUMENT;
    }
    /* TSP_EVERY_START_NEIGHBOURS=K (env_neighbours): -alg 2OPT_GREEDY runs h_greedy_local_search_nl over lists of K nodes */
    const int es_k = env_neighbours("TSP_EVERY_START_NEIGHBOURS");
    if (es_k < 0) return INVALID_ARGUMENT;
    /* TSP_3OPT_WIDTH=W (env_neighbours): the TSP_OR_OPT polish over the lists gets a 3-opt phase over their first W entries */
    const int width3 = env_neighbours("TSP_3OPT_WIDTH");
    if (width3 < 0) return INVALID_ARGUMENT;
    /* TSP_DONT_LOOK=1 (env_switch): that polish over the lists runs with don't-look bits */
    const int dont_look = env_switch("TSP_DONT_LOOK");
    if (dont_look < 0) return INVALID_ARGUMENT;
    if (es_k && ((nl_k && nl_k != es_k) || (or_nl_k && or_nl_k != es_k))) {
        fprintf(stderr, "tsp: TSP_EVERY_START_NEIGHBOURS=%d and TSP_%s_NEIGHBOURS=%d: the list lengths must be equal\n", es_k,
                nl_k && nl_k != es_k ? "2OPT" : "OR_OPT", nl_k && nl_k != es_k ? nl_k : or_nl_k);
        return INVALID_ARGUMENT;
    }
    if (es_k && every_start) {
        fprintf(stderr, "tsp: TSP_EVERY_START_NEIGHBOURS=%d and TSP_OR_OPT_EVERY_START=1: one descent from every start, not both\n", es_k);
        return INVALID_ARGUMENT;
    }
    /* TSP_VNS_NEIGHBOURS=K (env_neighbours): -alg VNS runs TSP_VNS_WALKS walks of the neighbour-list VNS over lists of K nodes */
    const int vns_k = env_neighbours("TSP_VNS_NEIGHBOURS");
    if (vns_k < 0) return INVALID_ARGUMENT;
    if (vns_k && ((nl_k && nl_k != vns_k) || (or_nl_k && or_nl_k != vns_k))) {
        fprintf(stderr, "tsp: TSP_VNS_NEIGHBOURS=%d and TSP_%s_NEIGHBOURS=%d: the list lengths must be equal\n", vns_k,
                nl_k && nl_k != vns_k ? "2OPT" : "OR_OPT", nl_k && nl_k != vns_k ? nl_k : or_nl_k);
        return INVALID_ARGUMENT;
    }
    /* TSP_EVERY_START_3OPT_WIDTH=W / TSP_VNS_3OPT_WIDTH=W (env_neighbours): the multi-start / the walks over the lists run the
     * descent with the 3-opt phase over the first W list entries */
    const int es_w3 = env_neighbours("TSP_EVERY_START_3OPT_WIDTH"), vns_w3 = env_neighbours("TSP_VNS_3OPT_WIDTH");
    if (es_w3 < 0 || vns_w3 < 0) return INVALID_ARGUMENT;
    /* TSP_VNS_DONT_LOOK=1 / TSP_EVERY_START_DONT_LOOK=1 (env_switch): the walks / the multi-start over the lists run with don't-look
     * bits; TSP_DONT_LOOK_CLOSING=1: their phases close with a full sweep */
    const int vns_dl = env_switch("TSP_VNS_DONT_LOOK"), es_dl = env_switch("TSP_EVERY_START_DONT_LOOK");
    const int dl_closing = env_switch("TSP_DONT_LOOK_CLOSING");
    if (vns_dl < 0 || es_dl < 0 || dl_closing < 0) return INVALID_ARGUMENT;
    /* TSP_GREEDY_EDGE_NEIGHBOURS=K (env_neighbours): -alg GREEDY builds the greedy-edge tour over lists of K nodes */
    const int ge_k = env_neighbours("TSP_GREEDY_EDGE_NEIGHBOURS");
    if (ge_k < 0) return INVALID_ARGUMENT;
    {
        const struct { const char *name; int k; } others[] = {{"2OPT", nl_k}, {"OR_OPT", or_nl_k}, {"EVERY_START", es_k}, {"VNS", vns_k}};
        for (size_t x = 0; ge_k && x < sizeof others / sizeof others[0]; x++)
            if (others[x].k && others[x].k != ge_k) {
                fprintf(stderr, "tsp: TSP_GREEDY_EDGE_NEIGHBOURS=%d and TSP_%s_NEIGHBOURS=%d: the list lengths must be equal\n", ge_k,
                        others[x].name, others[x].k);
                return INVALID_ARGUMENT;
            }
    }
    greedy_edge_k = tsp_inst.alg == ALG_GREEDY ? ge_k : 0;
    if (ge_k && tsp_inst.alg == ALG_GREEDY)
        log_warn("TSP_GREEDY_EDGE_NEIGHBOURS=%d: -alg GREEDY builds the greedy-edge tour, not the nearest-neighbour tour; results differ from "
                 "the reference's", ge_k);
    else if (ge_k) log_warn("TSP_GREEDY_EDGE_NEIGHBOURS=%d has no effect without -alg GREEDY", ge_k);
    int vns_w = 1;
    {
        const char *v = getenv("TSP_VNS_WALKS");
        char *end = NULL;
        const long w = v ? strtol(v, &end, 10) : 1;
        if (v && (!*v || *end || w < 1 || w > VNS_NL_NUMBERS / (32 + 1024))) {
            fprintf(stderr, "tsp: TSP_VNS_WALKS=\"%s\": expected a walk count from 1 to %d\n", v, VNS_NL_NUMBERS / (32 + 1024));
            return INVALID_ARGUMENT;
        }
        vns_w = (int)w;
    }
    vns_nl_k = tsp_inst.alg == ALG_VNS ? vns_k : 0;
    vns_nl_walks = vns_w;
    if (vns_k && tsp_inst.alg == ALG_VNS)
        log_warn("TSP_VNS_NEIGHBOURS=%d: mh_VNS runs %d walk%s of the neighbour-list VNS; results differ from the reference's trajectory",
                 vns_k, vns_w, vns_w == 1 ? "" : "s");
    else if (vns_k) log_warn("TSP_VNS_NEIGHBOURS=%d has no effect without -alg VNS", vns_k);
    else if (getenv("TSP_VNS_WALKS")) log_warn("TSP_VNS_WALKS has no effect without TSP_VNS_NEIGHBOURS");
    vns_nl_width3 = vns_nl_k ? vns_w3 : 0;
    if (vns_w3 && !vns_nl_k) log_warn("TSP_VNS_3OPT_WIDTH=%d has no effect without -alg VNS and TSP_VNS_NEIGHBOURS=K", vns_w3);
    vns_nl_dont_look = vns_nl_k ? vns_dl : 0;
    if (vns_nl_dont_look) log_warn("TSP_VNS_DONT_LOOK=1: the walks run with don't-look bits; behind a kick only the nodes at changed edges are looked at");
    else if (vns_dl) log_warn("TSP_VNS_DONT_LOOK=1 has no effect without -alg VNS and TSP_VNS_NEIGHBOURS=K");
    every_start_dont_look = es_k && tsp_inst.alg == ALG_2OPT_GREEDY ? es_dl : 0;
    if (every_start_dont_look) log_warn("TSP_EVERY_START_DONT_LOOK=1: every start descends with don't-look bits, on one device");
    else if (es_dl) log_warn("TSP_EVERY_START_DONT_LOOK=1 has no effect without -alg 2OPT_GREEDY and TSP_EVERY_START_NEIGHBOURS=K");
    batch_dl_closing = vns_nl_dont_look || every_start_dont_look ? dl_closing : 0;
    if (dl_closing && !batch_dl_closing) log_warn("TSP_DONT_LOOK_CLOSING=1 has no effect without TSP_VNS_DONT_LOOK=1 or TSP_EVERY_START_DONT_LOOK=1");
    every_start_nl_k = es_k;
    if (es_k && tsp_inst.alg == ALG_2OPT_GREEDY)
        log_warn("TSP_EVERY_START_NEIGHBOURS=%d: every start runs the descent over the neighbour lists; results differ from the reference's trajectory",
                 es_k);
    else if (es_k) log_warn("TSP_EVERY_START_NEIGHBOURS=%d has no effect without -alg 2OPT_GREEDY", es_k);
    every_start_width3 = es_k && tsp_inst.alg == ALG_2OPT_GREEDY ? es_w3 : 0;
    if (es_w3 && !every_start_width3)
        log_warn("TSP_EVERY_START_3OPT_WIDTH=%d has no effect without -alg 2OPT_GREEDY and TSP_EVERY_START_NEIGHBOURS=K", es_w3);
    or_opt_nl_k = polish > 0 ? or_nl_k : 0;
    if (or_nl_k && !polish) log_warn("TSP_OR_OPT_NEIGHBOURS=%d has no effect without TSP_OR_OPT=1", or_nl_k);
    three_opt_width = or_opt_nl_k ? width3 : 0;
    if (width3 && !or_opt_nl_k) log_warn("TSP_3OPT_WIDTH=%d has no effect without TSP_OR_OPT=1 and TSP_OR_OPT_NEIGHBOURS=K", width3);
    dont_look_on = or_opt_nl_k ? dont_look : 0;
    if (dont_look && !or_opt_nl_k) log_warn("TSP_DONT_LOOK=1 has no effect without TSP_OR_OPT=1 and TSP_OR_OPT_NEIGHBOURS=K");
    two_opt_multi_on = multi;
    two_opt_nl_k = nl_k;
    two_opt_nl_polish = nl_polish;
    if (nl_k) log_warn("TSP_2OPT_NEIGHBOURS=%d: ref_2opt runs the neighbour-list descent%s; results differ from the reference's trajectory",
                       nl_k, nl_polish ? " and the parallel-move polish" : ", no polish: a local optimum of the list neighbourhood only");
    else if (multi) log_warn("TSP_2OPT_MULTI=1: ref_2opt runs the parallel-move descent; results differ from the reference's trajectory");
    free(tsp_inst.best_solution.path);
    tsp_inst.best_solution.path = (int *)calloc((size_t)tsp_inst.nnodes, sizeof(int));
    ERROR_CODE e;
    switch (tsp_inst.alg) {
    case ALG_GREEDY: e = h_Greedy(); break;
    case ALG_GREEDY_ITER: e = h_Greedy_iterative(); break;
    case ALG_2OPT_GREEDY: e = es_k ? h_greedy_local_search_nl() : every_start ? h_greedy_local_search() : h_greedy_2opt(); break;
    case ALG_TABU_SEARCH: e = mh_TabuSearch(); break;
    case ALG_VNS: e = mh_VNS(); break;
    case ALG_EXTRAMILEAGE: e = h_ExtraMileage(); break;
    default:
        log_error("algorithm %d belongs to the CPLEX path, which this library leaves to the reference build", tsp_inst.alg);
        return UNIMPLEMENTED;
    }
    if (!polish || (e != T_OK && e != DEADLINE_EXCEEDED)) return e;
    if (tsp_matrix_free && !polish_mf && !or_opt_nl_k) {
        log_warn("TSP_OR_OPT=1: Or-opt needs the cost matrix and the instance runs matrix-free; the polish is skipped");
        return e;
    }
    if (tsp_matrix_free && !or_opt_nl_k) {      /* TSP_OR_OPT_MATRIX_FREE=1: the single-tour descent from the coordinates */
        tspgpu_ctx *g = tsp_gpu();
        if (!g) return UNAVAILABLE;
        const int rc = tspgpu_set_option(g, TSPGPU_OPT_OR_MATRIX_FREE, 1);
        if (rc) { log_error("TSPGPU_OPT_OR_MATRIX_FREE: %s", tspgpu_last_error(g)); return from_rc(rc); }
    }
    /* the polish works on a copy: tsp_update_best_solution takes it only if it is a tour and strictly better */
    tsp_solution s;
    const int n = tsp_inst.nnodes;
    tsp_init_solution(n, &s);
    memcpy(s.path, tsp_inst.best_solution.path, (size_t)n * sizeof(int));
    s.cost = tsp_inst.best_solution.cost;
    const ERROR_CODE pe = tsp_or_opt_polish(&s);
    if (pe == T_OK || pe == DEADLINE_EXCEEDED) {
        const ERROR_CODE u = tsp_update_best_solution(&s);
        if (!err_ok(u)) log_error("code %d : error in updating the best solution after the Or-opt polish", u);
    }
    free(s.path); free(s.comp);
    if (or_opt_refusal(pe)) {       /* as in matrix-free mode: the heuristic's result stands */
        log_warn("TSP_OR_OPT=1: Or-opt does not take this instance (code %d); the polish is skipped", pe);
        return e;
    }
    if (pe != T_OK && pe != DEADLINE_EXCEEDED) return pe;
    return pe == DEADLINE_EXCEEDED ? pe : e;
}
