/* Plain C restatement of the neighbour-list 2-opt defined in include/tspgpu.h ("Neighbour-list 2-opt"): the lists, the
 * candidates of a sweep and the descent with its polish, over a double matrix (c != NULL) or over coordinates (c == NULL,
 * the weights of two_opt_multi_model.c).  That file is included unmodified for its cost source (src, W), its key order
 * (key_less) and the parallel-move sweep the polish runs (tom_sweep); rules 2-5 are restated here behind the new candidates.
 * tests/test_two_opt_nl.py pins this file to a brute-force Python restatement; tools/make_golden_two_opt_nl.py runs it
 * where it takes more than a few seconds.  Only the list build is threaded (stripes of rows).
 * gcc -O2 -ffp-contract=off -shared -fPIC -pthread. */
#include "two_opt_multi_model.c"

/* ---- lists: N(v) = the K nodes u != v with the smallest (W(v, u), u), ascending.  K <= n - 1. */
typedef struct { const src *S; int K, v0, v1; int *nodes; double *w; } ljob;

static void *list_rows(void *arg)
{
    ljob *J = (ljob *)arg;
    const src *S = J->S;
    const int n = S->n, K = J->K;
    for (int v = J->v0; v < J->v1; v++) {
        int *nd = J->nodes + (size_t)v * K;
        double *wd = J->w + (size_t)v * K;
        int have = 0;
        for (int u = 0; u < n; u++) {
            if (u == v) continue;
            const double x = W(S, v, u);
            if (have == K && !(x < wd[K - 1])) continue;    /* u ascends: an equal cost comes behind */
            int at = have < K ? have++ : K - 1;
            while (at > 0 && x < wd[at - 1]) { wd[at] = wd[at - 1]; nd[at] = nd[at - 1]; at--; }
            wd[at] = x; nd[at] = u;
        }
    }
    return NULL;
}

/* -> 0; nodes / w [n * K'] with K' = min(K, n - 1), returned in *kp */
int nlm_lists(const double *c, const double *xy, int n, int kind, int K, int threads, int *nodes, double *w, int *kp)
{
    const src S = {c, xy, n, kind};
    if (K > n - 1) K = n - 1;
    *kp = K;
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    if (threads > n) threads = n;
    ljob J[64];
    pthread_t th[64];
    for (int k = 0; k < threads; k++) {
        const ljob j = {&S, K, (int)((long)n * k / threads), (int)((long)n * (k + 1) / threads), nodes, w};
        J[k] = j;
        pthread_create(&th[k], NULL, list_rows, &J[k]);
    }
    for (int k = 0; k < threads; k++) pthread_join(th[k], NULL);
    return 0;
}

/* One sweep over the lists `nodes` [n * K].  Arguments and results as tom_sweep's; cand_d[a] = DBL_MAX, cand_b[a] = -1 where
 * B(a) is empty. -> 0, or 1 when memory ran out. */
int nlm_sweep(const double *c, const double *xy, int n, int kind, int K, const int *nodes, int *path,
              double *cand_d, int *cand_b, int *m_out, int *ca, int *cb, int *ci, int *cj, double *cdl, int *acc,
              int *nacc, int *moves_ab, double *deltas, double *cost, int apply)
{
    const src S = {c, xy, n, kind};
    double *cnext = (double *)malloc((size_t)n * sizeof(double));
    int *P = (int *)malloc((size_t)n * sizeof(int)), *ord = (int *)malloc((size_t)n * sizeof(int));
    int *sel = (int *)malloc((size_t)n * sizeof(int)), *pred = (int *)malloc((size_t)n * sizeof(int));
    if (!cnext || !P || !ord || !sel || !pred) { free(cnext); free(P); free(ord); free(sel); free(pred); return 1; }
    for (int v = 0; v < n; v++) { cnext[v] = W(&S, v, path[v]); pred[path[v]] = v; }
    for (int i = 0, v = 0; i < n; i++, v = path[v]) { P[v] = i; ord[i] = v; }      /* rule 2: cut at node 0 */
    for (int a = 0; a < n; a++) {
        const int sa = path[a];
        double best = DBL_MAX;
        int bb = -1;
        for (int j = 0; j < 2 * K; j++) {
            const int b = j < K ? nodes[(size_t)a * K + j] : pred[nodes[(size_t)sa * K + j - K]];
            const int sb = path[b];
            if (sa == sb || a == sb || b == sa) continue;                       /* refinment.c:55 */
            const double d = (W(&S, a, b) + W(&S, sa, sb)) - (cnext[a] + cnext[b]);   /* refinment.c:60-62 */
            if (bb < 0 || d < best || (d == best && b < bb)) { best = d; bb = b; }
        }
        cand_d[a] = best;
        cand_b[a] = bb;
    }
    int m = 0;
    for (int a = 0; a < n; a++) {
        const int b = cand_b[a];
        if (b < 0 || !(cand_d[a] < EPS)) continue;
        if (cand_b[b] == a && b < a) continue;      /* two nodes that chose each other: the pair once */
        const int ab = P[a] < P[b];
        ca[m] = ab ? a : b; cb[m] = ab ? b : a;
        ci[m] = ab ? P[a] : P[b]; cj[m] = ab ? P[b] : P[a];
        cdl[m] = cand_d[a];
        m++;
    }
    int k = 0;
    for (int x = 0; x < m; x++) {                   /* rules 3 and 4: one round */
        int ok = 1;
        for (int y = 0; y < m && ok; y++)
            if (y != x && ci[y] <= cj[x] && ci[x] <= cj[y] && !key_less(cdl[x], ca[x], cb[x], cdl[y], ca[y], cb[y])) ok = 0;
        acc[x] = ok;
        if (ok) sel[k++] = x;
    }
    for (int u = 1; u < k; u++) {                   /* ascending key */
        const int x = sel[u];
        int v = u;
        while (v > 0 && key_less(cdl[x], ca[x], cb[x], cdl[sel[v - 1]], ca[sel[v - 1]], cb[sel[v - 1]])) { sel[v] = sel[v - 1]; v--; }
        sel[v] = x;
    }
    double sum = 0.0;
    for (int u = 0; u < k; u++) {
        const int x = sel[u];
        moves_ab[2 * u] = ca[x]; moves_ab[2 * u + 1] = cb[x]; deltas[u] = cdl[x];
        sum += cdl[x];
        if (apply) {                                /* rule 5 */
            const int i = ci[x], j = cj[x], sb = ord[(j + 1) % n];
            path[ord[i]] = ord[j];
            for (int p = j; p > i + 1; p--) path[ord[p]] = ord[p - 1];
            path[ord[i + 1]] = sb;
        }
    }
    if (apply && cost) *cost += sum;
    *m_out = m;
    *nacc = k;
    free(cnext); free(P); free(ord); free(sel); free(pred);
    return 0;
}

/* the descent over the lists, then (polish != 0) parallel-move sweeps on the result with the running cost.  Each phase
 * counts its last, empty sweep.  nl_path (may be NULL) receives the tour between the two phases. -> 0 */
int nlm_descent(const double *c, const double *xy, int n, int kind, int K, const int *nodes, int *path, int polish, int threads,
                double *cost, long *sweeps, long *moves, double *nl_cost, int *nl_path, long *psweeps, long *pmoves)
{
    const src S = {c, xy, n, kind};
    double *cand_d = (double *)malloc((size_t)n * sizeof(double)), *cdl = (double *)malloc((size_t)n * sizeof(double));
    double *deltas = (double *)malloc((size_t)n * sizeof(double));
    int *ib = (int *)malloc((size_t)8 * n * sizeof(int));
    if (!cand_d || !cdl || !deltas || !ib) { free(cand_d); free(cdl); free(deltas); free(ib); return 1; }
    double total = 0.0;
    for (int i = 0; i < n; i++) total += W(&S, i, path[i]);      /* refinment.c:6-9 */
    *cost = total;
    *sweeps = *moves = *psweeps = *pmoves = 0;
    int rc = 0;
    for (int phase = 0; phase < (polish ? 2 : 1) && !rc; phase++) {
        for (;;) {
            int m = 0, k = 0;
            if (phase == 0)
                rc = nlm_sweep(c, xy, n, kind, K, nodes, path, cand_d, ib, &m, ib + n, ib + 2 * n, ib + 3 * n, ib + 4 * n, cdl, ib + 5 * n,
                               &k, ib + 6 * n, deltas, cost, 1);
            else
                rc = tom_sweep(c, xy, n, kind, path, threads, cand_d, ib, &m, ib + n, ib + 2 * n, ib + 3 * n, ib + 4 * n, cdl, ib + 5 * n,
                               &k, ib + 6 * n, deltas, cost, 1);
            if (rc) break;
            *(phase ? psweeps : sweeps) += 1;
            *(phase ? pmoves : moves) += k;
            if (k == 0) break;
        }
        if (phase == 0) {
            *nl_cost = *cost;
            if (nl_path) for (int i = 0; i < n; i++) nl_path[i] = path[i];
        }
    }
    free(cand_d); free(cdl); free(deltas); free(ib);
    return rc;
}
