/* Plain C restatement of the parallel-move 2-opt sweep defined in include/tspgpu.h ("Parallel-move 2-opt", rules 1-6),
 * over a double matrix (c != NULL) or -- the coordinate variant, c == NULL -- over points with the TSPLIB 95 weights as the
 * project computes them: EUC_2D (0) the float root of the double sum, rounded; ATT (1); CEIL_2D (2).
 * tests/test_two_opt_multi.py pins it to a brute-force Python restatement; tools/make_golden_two_opt_multi.py runs it where
 * it takes more than a few seconds.  Only the candidate scan is threaded (stripes of nodes: the result does not depend on them).
 * gcc -O2 -ffp-contract=off -shared -fPIC -pthread. */
#include <float.h>
#include <math.h>
#include <pthread.h>
#include <stdlib.h>

#define EPS (-1.0e-7)

typedef struct { const double *c, *xy; int n, kind; } src;

static double W(const src *S, int a, int b)
{
    if (S->c) return S->c[(size_t)a * S->n + b];
    const double *xy = S->xy;
    const double dx = xy[2 * b] - xy[2 * a], dy = xy[2 * b + 1] - xy[2 * a + 1];
    const double sq = dx * dx + dy * dy;
    if (S->kind == 0) return (double)((int)((double)sqrtf((float)sq) + 0.5));
    if (S->kind == 1) {
        const double r = sqrt(sq / 10.0), t = (double)(long)(r + 0.5);
        return t < r ? t + 1.0 : t;
    }
    return ceil(sqrt(sq));
}

typedef struct { const src *S; const int *path; const double *cnext; int a0, a1; double *cand_d; int *cand_b; } job;

/* rule 1: for every node a of the stripe the first strict minimum over b ascending (any sign) */
static void *scan(void *arg)
{
    job *J = (job *)arg;
    const src *S = J->S;
    const int n = S->n;
    for (int a = J->a0; a < J->a1; a++) {
        const int sa = J->path[a];
        double best = DBL_MAX;
        int bb = -1;
        for (int b = 0; b < n; b++) {
            const int sb = J->path[b];
            if (sa == sb || a == sb || b == sa) continue;                       /* refinment.c:55 */
            const double d = (W(S, a, b) + W(S, sa, sb)) - (J->cnext[a] + J->cnext[b]);   /* refinment.c:60-62 */
            if (d < best) { best = d; bb = b; }
        }
        J->cand_d[a] = best;
        J->cand_b[a] = bb;
    }
    return NULL;
}

static int key_less(double d1, int a1, int b1, double d2, int a2, int b2)
{
    const int l1 = a1 < b1 ? a1 : b1, h1 = a1 < b1 ? b1 : a1, l2 = a2 < b2 ? a2 : b2, h2 = a2 < b2 ? b2 : a2;
    if (d1 != d2) return d1 < d2;
    if (l1 != l2) return l1 < l2;
    return h1 < h2;
}

/* One sweep.  Out, [n] each: cand_d / cand_b by node (rule 1, before the threshold); the m candidates in ascending order of
 * the choosing node, once per pair -- ca / cb the nodes at P = ci < cj, cdl the delta, acc 1 when accepted (rules 2-4);
 * the accepted ones again in ascending key order in moves_ab [2 nacc] / deltas.  apply != 0: rule 5 on path and *cost.
 * -> 0, or 1 when memory ran out. */
int tom_sweep(const double *c, const double *xy, int n, int kind, int *path, int threads,
              double *cand_d, int *cand_b, int *m_out, int *ca, int *cb, int *ci, int *cj, double *cdl, int *acc,
              int *nacc, int *moves_ab, double *deltas, double *cost, int apply)
{
    const src S = {c, xy, n, kind};
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    if (threads > n) threads = n;
    double *cnext = (double *)malloc((size_t)n * sizeof(double));
    int *P = (int *)malloc((size_t)n * sizeof(int)), *ord = (int *)malloc((size_t)n * sizeof(int));
    int *sel = (int *)malloc((size_t)n * sizeof(int));
    if (!cnext || !P || !ord || !sel) { free(cnext); free(P); free(ord); free(sel); return 1; }
    for (int v = 0; v < n; v++) cnext[v] = W(&S, v, path[v]);
    for (int i = 0, v = 0; i < n; i++, v = path[v]) { P[v] = i; ord[i] = v; }      /* rule 2: cut at node 0 */
    job J[64];
    pthread_t th[64];
    for (int k = 0; k < threads; k++) {
        const job j = {&S, path, cnext, (int)((long)n * k / threads), (int)((long)n * (k + 1) / threads), cand_d, cand_b};
        J[k] = j;
        pthread_create(&th[k], NULL, scan, &J[k]);
    }
    for (int k = 0; k < threads; k++) pthread_join(th[k], NULL);
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
    for (int u = 1; u < k; u++) {                   /* ascending key (insertion sort: k is small next to the scan) */
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
        if (apply) {                                /* rule 5, from the positions before the sweep (the ranges are disjoint) */
            const int i = ci[x], j = cj[x], sb = ord[(j + 1) % n];
            path[ord[i]] = ord[j];
            for (int p = j; p > i + 1; p--) path[ord[p]] = ord[p - 1];
            path[ord[i + 1]] = sb;
        }
    }
    if (apply && cost) *cost += sum;
    *m_out = m;
    *nacc = k;
    free(cnext); free(P); free(ord); free(sel);
    return 0;
}

/* rule 6 -> 0; *sweeps counts the last, empty sweep; *max_k the most moves one sweep accepted, *multi the sweeps with two or more */
int tom_descent(const double *c, const double *xy, int n, int kind, int *path, int threads, double *cost, long *sweeps, long *moves,
                int *max_k, long *multi)
{
    const src S = {c, xy, n, kind};
    double *cand_d = (double *)malloc((size_t)n * sizeof(double)), *cdl = (double *)malloc((size_t)n * sizeof(double));
    double *deltas = (double *)malloc((size_t)n * sizeof(double));
    int *ib = (int *)malloc((size_t)8 * n * sizeof(int));
    if (!cand_d || !cdl || !deltas || !ib) { free(cand_d); free(cdl); free(deltas); free(ib); return 1; }
    double total = 0.0;
    for (int i = 0; i < n; i++) total += W(&S, i, path[i]);      /* refinment.c:6-9 */
    *cost = total;
    *sweeps = *moves = *multi = 0;
    *max_k = 0;
    int rc = 0;
    for (;;) {
        int m = 0, k = 0;
        rc = tom_sweep(c, xy, n, kind, path, threads, cand_d, ib, &m, ib + n, ib + 2 * n, ib + 3 * n, ib + 4 * n, cdl, ib + 5 * n,
                       &k, ib + 6 * n, deltas, cost, 1);
        if (rc) break;
        *sweeps += 1;
        *moves += k;
        if (k > *max_k) *max_k = k;
        if (k >= 2) *multi += 1;
        if (k == 0) break;
    }
    free(cand_d); free(cdl); free(deltas); free(ib);
    return rc;
}
