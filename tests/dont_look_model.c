/* Plain C restatement of "Don't-look bits" in include/tspgpu.h: the sweep with looks of the three neighbour-list families,
 * the phase with its `closing` flag, the descent and the kick, over a double matrix (c != NULL) or over coordinates
 * (c == NULL).  three_opt_nl_model.c is included unmodified: the candidates of every unit come from the plain models' own
 * sweeps (nlm_sweep, onl_sweep, t3m_sweep with apply = 0), the units outside Q lose theirs, and compaction, range, the one
 * selection round and the apply are restated here behind them, with the carry and the ends of rule 4.
 * tests/test_dont_look.py pins the first all-awake sweep of this file to the plain models; tools/make_golden_dont_look.py
 * runs it on pr1002.
 * gcc -O2 -ffp-contract=off -shared -fPIC -pthread. */
#include <string.h>
#include "three_opt_nl_model.c"

static void dlm_tour(int n, const int *path, int *P, int *ord, int *pred)
{
    for (int v = 0; v < n; v++) pred[path[v]] = v;
    for (int i = 0, v = 0; i < n; i++, v = path[v]) { P[v] = i; ord[i] = v; }
}

/* One sweep with looks of family f (0 the 2-opt, 1 Or-opt, 2 the 3-opt) on path, *cost and the sets awake [3 n] (rules 2-5).
 * Out: *nacc the accepted moves, *nq = |Q|, looked [n] (may be NULL) the members of Q.  -> 0, or 1 when memory ran out. */
int dlm_sweep(const double *c, const double *xy, int n, int kind, int K, int width, const int *nodes, int f, int *path,
              unsigned char *awake, double *cost, int *nacc, int *nq, unsigned char *looked)
{
    double *cand_d = (double *)malloc((size_t)n * sizeof(double)), *cdl = (double *)malloc((size_t)n * sizeof(double));
    double *deltas = (double *)malloc((size_t)n * sizeof(double));
    int *ib = (int *)malloc((size_t)15 * n * sizeof(int));
    unsigned char *nf = (unsigned char *)calloc((size_t)n, 1), *inq = (unsigned char *)calloc((size_t)n, 1);
    if (!cand_d || !cdl || !deltas || !ib || !nf || !inq) { free(cand_d); free(cdl); free(deltas); free(ib); free(nf); free(inq); return 1; }
    int *cand_b = ib, *ca = ib + n, *cb = ib + 2 * n, *ci = ib + 3 * n, *cj = ib + 4 * n, *acc = ib + 5 * n, *scratch = ib + 6 * n;
    int *P = ib + 10 * n, *ord = ib + 11 * n, *pred = ib + 12 * n, *sel = ib + 13 * n, *nord = ib + 14 * n;
    unsigned char *A = awake + (size_t)f * n;
    int m = 0, k = 0, rc;
    /* the plain candidates of every unit; nothing is applied */
    if (f == 0) rc = nlm_sweep(c, xy, n, kind, K, nodes, path, cand_d, cand_b, &m, ca, cb, ci, cj, cdl, acc, &k, scratch, deltas, NULL, 0);
    else if (f == 1) rc = onl_sweep(c, xy, n, kind, K, nodes, path, cand_d, cand_b, &m, ca, cb, ci, cj, cdl, acc, &k, scratch, deltas, NULL, 0);
    else rc = t3m_sweep(c, xy, n, kind, K, width, nodes, path, cand_d, cand_b, &m, ca, cb, ci, cj, cdl, acc, &k, scratch, deltas, NULL, 0);
    if (rc) { free(cand_d); free(cdl); free(deltas); free(ib); free(nf); free(inq); return rc; }
    dlm_tour(n, path, P, ord, pred);
    for (int i = 0; i < n; i++) nord[i] = ord[i];
    /* rule 2: Q; rule 3: no candidate outside it */
    const int fwd = f == 1 ? 2 : 0;
    int q = 0;
    for (int v = 0; v < n; v++) {
        int in = 0;
        for (int w = 0, u = v; w <= fwd && !in; w++, u = path[u]) in = A[u] != 0;
        inq[v] = (unsigned char)in;
        q += in;
        if (!in) { cand_b[v] = -1; cand_d[v] = DBL_MAX; }
    }
    if (looked) memcpy(looked, inq, (size_t)n);
    /* the families' compaction on those candidates, and the carry of rule 4 */
    m = 0;
    for (int v = 0; v < n; v++) {
        const int b = cand_b[v];
        if (b < 0 || !(cand_d[v] < EPS)) continue;
        if (f == 0) {
            nf[v] = 1; nf[path[v]] = 1;
            if (cand_b[b] == v && b < v) continue;          /* two nodes that chose each other: the pair once */
            const int ab = P[v] < P[b];
            ca[m] = ab ? v : b; cb[m] = ab ? b : v;
            ci[m] = ab ? P[v] : P[b]; cj[m] = ab ? P[b] : P[v];
        } else if (f == 1) {
            const int L = b >> 18, qq = (b >> 1) & 0x1ffff, i = P[v], j = P[qq];
            for (int w = 0, u = v; w < L; w++, u = path[u]) nf[u] = 1;
            ca[m] = v; cb[m] = b;
            ci[m] = i - 1 < j ? i - 1 : j;
            cj[m] = i + L - 1 > j ? i + L - 1 : j;
        } else {
            t3chain C;
            nf[v] = 1;
            t3_decode(&C, v, b, K, nodes, path, pred);
            t3_classify(&C, P);
            ca[m] = v; cb[m] = b; ci[m] = C.i; cj[m] = C.k;
        }
        cdl[m] = cand_d[v];
        m++;
    }
    k = 0;
    for (int x = 0; x < m; x++) {                           /* one selection round */
        int ok = 1;
        for (int y = 0; y < m && ok; y++)
            if (y != x && ci[y] <= cj[x] && ci[x] <= cj[y] && !key_less(cdl[x], ca[x], cb[x], cdl[y], ca[y], cb[y])) ok = 0;
        if (ok) sel[k++] = x;
    }
    for (int u = 1; u < k; u++) {                           /* ascending key: the order of the cost sum */
        const int x = sel[u];
        int v = u;
        while (v > 0 && key_less(cdl[x], ca[x], cb[x], cdl[sel[v - 1]], ca[sel[v - 1]], cb[sel[v - 1]])) { sel[v] = sel[v - 1]; v--; }
        sel[v] = x;
    }
    double sum = 0.0;
    for (int u = 0; u < k; u++) {                           /* ends and apply, from the order before the sweep */
        const int x = sel[u];
        int e[6], ne = 6, lo, hi;
        sum += cdl[x];
        if (f == 0) {
            const int i = ci[x], j = cj[x];
            e[0] = ord[i]; e[1] = ord[i + 1]; e[2] = ord[j]; e[3] = ord[(j + 1) % n];
            ne = 4;
            for (int p = i + 1; p <= j; p++) nord[p] = ord[i + 1 + j - p];
            lo = i; hi = j;
        } else if (f == 1) {
            const int s = ca[x], pk = cb[x], L = pk >> 18, qq = (pk >> 1) & 0x1ffff, rev = pk & 1, i = P[s], j = P[qq];
            e[0] = ord[i - 1]; e[1] = s; e[2] = ord[i + L - 1]; e[3] = ord[(i + L) % n]; e[4] = qq; e[5] = ord[(j + 1) % n];
            lo = ci[x]; hi = cj[x];
            int at = lo + 1;                                /* the positions lo + 1 .. hi refilled */
            if (j > i) {                                    /* behind: x .. q, then the segment */
                for (int p = i + L; p <= j; p++) nord[at++] = ord[p];
                for (int w = 0; w < L; w++) nord[at++] = rev ? ord[i + L - 1 - w] : ord[i + w];
            } else {                                        /* in front: the segment, then q' .. p */
                for (int w = 0; w < L; w++) nord[at++] = rev ? ord[i + L - 1 - w] : ord[i + w];
                for (int p = j + 1; p <= i - 1; p++) nord[at++] = ord[p];
            }
        } else {
            t3chain C;
            t3_decode(&C, ca[x], cb[x], K, nodes, path, pred);
            t3_classify(&C, P);
            e[0] = ord[C.i]; e[1] = ord[C.i + 1]; e[2] = ord[C.j]; e[3] = ord[C.j + 1]; e[4] = ord[C.k]; e[5] = ord[(C.k + 1) % n];
            const int la = C.j - C.i, lb = C.k - C.j;
            int at = C.i + 1;
            if (C.kind == 0) {
                for (int w = 0; w < la; w++) nord[at++] = ord[C.j - w];
                for (int w = 0; w < lb; w++) nord[at++] = ord[C.k - w];
            } else {
                for (int w = 0; w < lb; w++) nord[at++] = C.kind == 2 ? ord[C.k - w] : ord[C.j + 1 + w];
                for (int w = 0; w < la; w++) nord[at++] = C.kind == 3 ? ord[C.j - w] : ord[C.i + 1 + w];
            }
            lo = C.i; hi = C.k;
        }
        for (int w = 0; w < ne; w++) { nf[e[w]] = 1; awake[e[w]] = 1; awake[(size_t)n + e[w]] = 1; awake[2 * (size_t)n + e[w]] = 1; }
        ci[x] = lo; cj[x] = hi;
    }
    for (int u = 0; u < k; u++)
        for (int p = ci[sel[u]]; p <= cj[sel[u]]; p++) path[nord[p]] = nord[(p + 1) % n];
    *cost += sum;
    memcpy(A, nf, (size_t)n);
    *nacc = k;
    *nq = q;
    free(cand_d); free(cdl); free(deltas); free(ib); free(nf); free(inq);
    return 0;
}

static int dlm_empty(const unsigned char *A, int n)
{
    for (int v = 0; v < n; v++) if (A[v]) return 0;
    return 1;
}

/* rule 6.  cnt [4] += sweeps, moves, looked, full sweeps of the phase (the caller zeroes it).  -> 0 */
int dlm_phase(const double *c, const double *xy, int n, int kind, int K, int width, const int *nodes, int f, int closing, long max_sweeps,
              int *path, unsigned char *awake, double *cost, long *cnt, long *moves_out)
{
    unsigned char *A = awake + (size_t)f * n;
    long sweeps = 0, moves = 0;
    if (moves_out) *moves_out = 0;
    if (max_sweeps == 0) return 0;
    if (dlm_empty(A, n)) {
        if (!closing) return 0;
        memset(A, 1, (size_t)n);
    }
    for (;;) {
        int k = 0, q = 0;
        const int rc = dlm_sweep(c, xy, n, kind, K, width, nodes, f, path, awake, cost, &k, &q, NULL);
        if (rc) return rc;
        sweeps++; moves += k;
        cnt[0] += 1; cnt[1] += k; cnt[2] += q; cnt[3] += q == n;
        if (k == 0) {
            if (q == n || !closing) break;
            memset(A, 1, (size_t)n);                        /* not full: every node wakes, and the phase goes on */
        }
        if (max_sweeps > 0 && sweeps >= max_sweeps) break;
    }
    if (moves_out) *moves_out = moves;
    return 0;
}

/* rule 8 on the running cost (the caller recomputes it for the host-tour form).  cnt [3][4]: per family sweeps, moves, looked,
 * full sweeps; *rounds the 2-opt phases, *phases3 the 3-opt phases.  -> 0 */
int dlm_descent(const double *c, const double *xy, int n, int kind, int K, int width, const int *nodes, int closing, int *path,
                unsigned char *awake, double *cost, long *cnt, int *rounds, int *phases3)
{
    memset(cnt, 0, 12 * sizeof(long));
    *rounds = *phases3 = 0;
    for (;;) {
        long m = 0;
        int rc;
        for (;;) {
            if ((rc = dlm_phase(c, xy, n, kind, K, width, nodes, 0, closing, -1, path, awake, cost, cnt, &m))) return rc;
            *rounds += 1;
            if ((rc = dlm_phase(c, xy, n, kind, K, width, nodes, 1, closing, -1, path, awake, cost, cnt + 4, &m))) return rc;
            if (m == 0) break;
        }
        if (width == 0) break;
        if ((rc = dlm_phase(c, xy, n, kind, K, width, nodes, 2, closing, -1, path, awake, cost, cnt + 8, &m))) return rc;
        *phases3 += 1;
        if (m == 0) break;
    }
    return 0;
}

/* rule 9 on path, *cost and the sets (awake may be NULL); *delta the value the cost grew by.  -> 0 */
int dlm_kick(const double *c, const double *xy, int n, int kind, int *path, int i, int j, int k, unsigned char *awake, double *cost,
             double *delta)
{
    const src S = {c, xy, n, kind};
    int *ord = (int *)malloc((size_t)2 * n * sizeof(int)), *nord = ord + n;
    if (!ord) return 1;
    for (int p = 0, v = 0; p < n; p++, v = path[v]) { ord[p] = v; nord[p] = v; }
    const int a = ord[i], a1 = ord[i + 1], b = ord[j], b1 = ord[j + 1], cc = ord[k], c1 = ord[(k + 1) % n];
    const double d = ((W(&S, a, b1) + W(&S, cc, a1)) + W(&S, b, c1)) - ((W(&S, a, a1) + W(&S, b, b1)) + W(&S, cc, c1));
    int at = i + 1;
    for (int p = j + 1; p <= k; p++) nord[at++] = ord[p];
    for (int p = i + 1; p <= j; p++) nord[at++] = ord[p];
    for (int p = i; p <= k; p++) path[nord[p]] = nord[(p + 1) % n];
    *cost += d;
    *delta = d;
    if (awake) {
        const int e[6] = {a, a1, b, b1, cc, c1};
        for (int w = 0; w < 6; w++) { awake[e[w]] = 1; awake[(size_t)n + e[w]] = 1; awake[2 * (size_t)n + e[w]] = 1; }
    }
    free(ord);
    return 0;
}
