/* Plain C restatement of the neighbour-list 3-opt defined in include/tspgpu.h ("Neighbour-list 3-opt", rules 1-10): the
 * candidate chains of a sweep, the one selection round, the apply and the descent that runs the 3-opt phase behind the
 * alternation of "Neighbour-list Or-opt" (rule 8), over a double matrix (c != NULL) or over coordinates (c == NULL).
 * or_opt_nl_model.c is included unmodified for its cost source (src, W), the lists (nlm_lists) and the two phases of rule 8
 * (nlm_sweep, onl_sweep).
 * tests/test_three_opt_nl.py pins this file to a brute-force Python restatement written from the move side;
 * tools/make_golden_three_opt_nl.py runs it where it takes more than a few seconds.
 * gcc -O2 -ffp-contract=off -shared -fPIC -pthread. */
#include "or_opt_nl_model.c"

#define T3_CODE(s2, j3, s4, j5, s6) (1 << 30 | (s2) << 10 | (j3) << 6 | (s4) << 5 | (j5) << 1 | (s6))

typedef struct { int t[6], s[3], e[3], i, j, k, kind; } t3chain;

/* rule 4 for a chain whose nodes t[] and directions s[] are filled in: the positions of the removed edges, the roles
 * (edge rank, tail or head) of the six chain nodes, the kind of the added set -> 1 and i, j, k, kind, or 0: not kept */
static int t3_classify(t3chain *C, const int *P)
{
    int role[6], mate[6];
    const int *t = C->t;
    for (int m = 0; m < 3; m++) C->e[m] = P[C->s[m] ? t[2 * m + 1] : t[2 * m]];      /* the tail's position */
    if (C->e[0] == C->e[1] || C->e[0] == C->e[2] || C->e[1] == C->e[2]) return 0;
    for (int m = 0; m < 3; m++) {
        const int r = (C->e[m] > C->e[(m + 1) % 3]) + (C->e[m] > C->e[(m + 2) % 3]);
        role[2 * m] = 2 * r + (C->s[m] ? 1 : 0);            /* 0 a, 1 a', 2 b, 3 b', 4 c, 5 c' */
        role[2 * m + 1] = 2 * r + (C->s[m] ? 0 : 1);
    }
    for (int m = 0; m < 3; m++) {                           /* added: {t2,t3}, {t4,t5}, {t6,t1} */
        const int x = 2 * m + 1, y = (2 * m + 2) % 6;
        mate[role[x]] = role[y];
        mate[role[y]] = role[x];
        if (t[x] == t[y]) return 0;
        for (int r = 0; r < 3; r++)
            if ((t[x] == t[2 * r] && t[y] == t[2 * r + 1]) || (t[x] == t[2 * r + 1] && t[y] == t[2 * r])) return 0;
    }
    const int pa = mate[0], pb = mate[1];
    C->kind = pa == 2 && pb == 4 ? 0 : pa == 3 && pb == 4 ? 1 : pa == 4 && pb == 3 ? 2 : pa == 3 && pb == 5 ? 3 : -1;
    if (C->kind < 0) return 0;
    for (int m = 0; m < 3; m++) {
        const int r = (C->e[m] > C->e[(m + 1) % 3]) + (C->e[m] > C->e[(m + 2) % 3]);
        if (r == 0) C->i = C->e[m]; else if (r == 1) C->j = C->e[m]; else C->k = C->e[m];
    }
    return 1;
}

/* the chain of (t1, code) on the tour path / pred */
static void t3_decode(t3chain *C, int t1, int code, int K, const int *nodes, const int *path, const int *pred)
{
    const int s2 = (code >> 10) & 1, j3 = (code >> 6) & 15, s4 = (code >> 5) & 1, j5 = (code >> 1) & 15, s6 = code & 1;
    C->s[0] = s2; C->s[1] = s4; C->s[2] = s6;
    C->t[0] = t1;
    C->t[1] = s2 ? pred[t1] : path[t1];
    C->t[2] = nodes[(size_t)C->t[1] * K + j3];
    C->t[3] = s4 ? pred[C->t[2]] : path[C->t[2]];
    C->t[4] = nodes[(size_t)C->t[3] * K + j5];
    C->t[5] = s6 ? pred[C->t[4]] : path[C->t[4]];
}

static int t3_key_less(double d1, int a1, int c1, double d2, int a2, int c2)
{
    if (d1 != d2) return d1 < d2;
    if (a1 != a2) return a1 < a2;
    return c1 < c2;
}

/* One sweep over the first Wd = min(width, K) entries of the lists `nodes` [n * K].  Out, [n] each: cand_d / cand_b by t1
 * (rule 4, before the threshold; cand_b the code, -1 and DBL_MAX where t1 has no chain); the m candidates in ascending t1 --
 * cs the node t1, cb the code, ci / cj the range [i, k], cdl the delta, acc 1 when accepted (rule 7); the accepted ones again
 * in ascending key order in moves [4 nacc] (i, j, k, kind) / deltas.  apply != 0: rule 8 on path and *cost.
 * -> 0, or 1 when memory ran out. */
int t3m_sweep(const double *c, const double *xy, int n, int kind, int K, int width, const int *nodes, int *path,
              double *cand_d, int *cand_b, int *m_out, int *cs, int *cb, int *ci, int *cj, double *cdl, int *acc,
              int *nacc, int *moves, double *deltas, double *cost, int apply)
{
    const src S = {c, xy, n, kind};
    const int Wd = width < K ? width : K;
    double *cnext = (double *)malloc((size_t)n * sizeof(double));
    int *P = (int *)malloc((size_t)n * sizeof(int)), *ord = (int *)malloc((size_t)n * sizeof(int));
    int *sel = (int *)malloc((size_t)n * sizeof(int)), *pred = (int *)malloc((size_t)n * sizeof(int));
    int *nord = (int *)malloc((size_t)n * sizeof(int));
    if (!cnext || !P || !ord || !sel || !pred || !nord) { free(cnext); free(P); free(ord); free(sel); free(pred); free(nord); return 1; }
    for (int v = 0; v < n; v++) { cnext[v] = W(&S, v, path[v]); pred[path[v]] = v; }
    for (int i = 0, v = 0; i < n; i++, v = path[v]) { P[v] = i; ord[i] = v; nord[i] = v; }     /* rule 1 */
    for (int t1 = 0; t1 < n; t1++) {
        double best = DBL_MAX;
        int bc = -1;
        t3chain C;
        C.t[0] = t1;
        for (int s2 = 0; s2 < 2; s2++) {
            C.s[0] = s2;
            C.t[1] = s2 ? pred[t1] : path[t1];
            const double c12 = s2 ? cnext[C.t[1]] : cnext[t1];
            for (int j3 = 0; j3 < Wd; j3++) {
                C.t[2] = nodes[(size_t)C.t[1] * K + j3];
                const double c23 = W(&S, C.t[1], C.t[2]);
                for (int s4 = 0; s4 < 2; s4++) {
                    C.s[1] = s4;
                    C.t[3] = s4 ? pred[C.t[2]] : path[C.t[2]];
                    const double c34 = s4 ? cnext[C.t[3]] : cnext[C.t[2]];
                    for (int j5 = 0; j5 < Wd; j5++) {
                        C.t[4] = nodes[(size_t)C.t[3] * K + j5];
                        const double c45 = W(&S, C.t[3], C.t[4]);
                        for (int s6 = 0; s6 < 2; s6++) {
                            C.s[2] = s6;
                            C.t[5] = s6 ? pred[C.t[4]] : path[C.t[4]];
                            const double c56 = s6 ? cnext[C.t[5]] : cnext[C.t[4]];
                            if (!t3_classify(&C, P)) continue;
                            const double d = ((c23 + c45) + W(&S, C.t[5], t1)) - ((c12 + c34) + c56);      /* rule 3 */
                            const int code = T3_CODE(s2, j3, s4, j5, s6);
                            if (bc < 0 || d < best || (d == best && code < bc)) { best = d; bc = code; }
                        }
                    }
                }
            }
        }
        cand_d[t1] = best;
        cand_b[t1] = bc;
    }
    int m = 0;
    for (int t1 = 0; t1 < n; t1++) {
        if (cand_b[t1] < 0 || !(cand_d[t1] < EPS)) continue;
        t3chain C;
        t3_decode(&C, t1, cand_b[t1], K, nodes, path, pred);
        t3_classify(&C, P);
        cs[m] = t1; cb[m] = cand_b[t1]; cdl[m] = cand_d[t1];
        ci[m] = C.i; cj[m] = C.k;                           /* rule 6 */
        m++;
    }
    int k = 0;
    for (int x = 0; x < m; x++) {                           /* rule 7: one round */
        int ok = 1;
        for (int y = 0; y < m && ok; y++)
            if (y != x && ci[y] <= cj[x] && ci[x] <= cj[y] && !t3_key_less(cdl[x], cs[x], cb[x], cdl[y], cs[y], cb[y])) ok = 0;
        acc[x] = ok;
        if (ok) sel[k++] = x;
    }
    for (int u = 1; u < k; u++) {                           /* ascending key */
        const int x = sel[u];
        int v = u;
        while (v > 0 && t3_key_less(cdl[x], cs[x], cb[x], cdl[sel[v - 1]], cs[sel[v - 1]], cb[sel[v - 1]])) { sel[v] = sel[v - 1]; v--; }
        sel[v] = x;
    }
    double sum = 0.0;
    for (int u = 0; u < k; u++) {
        const int x = sel[u];
        t3chain C;
        t3_decode(&C, cs[x], cb[x], K, nodes, path, pred);
        t3_classify(&C, P);
        moves[4 * u] = C.i; moves[4 * u + 1] = C.j; moves[4 * u + 2] = C.k; moves[4 * u + 3] = C.kind;
        deltas[u] = cdl[x];
        sum += cdl[x];
        const int la = C.j - C.i, lb = C.k - C.j;           /* |A|, |B| */
        int at = C.i + 1;                                   /* rule 8: the positions i + 1 .. k refilled from the old order */
        if (C.kind == 0) {
            for (int q = 0; q < la; q++) nord[at++] = ord[C.j - q];
            for (int q = 0; q < lb; q++) nord[at++] = ord[C.k - q];
        } else {
            for (int q = 0; q < lb; q++) nord[at++] = C.kind == 2 ? ord[C.k - q] : ord[C.j + 1 + q];
            for (int q = 0; q < la; q++) nord[at++] = C.kind == 3 ? ord[C.j - q] : ord[C.i + 1 + q];
        }
    }
    if (apply) {
        for (int u = 0; u < k; u++)                         /* (from the moves, so that path stays untouched where nothing moved) */
            for (int p = moves[4 * u]; p <= moves[4 * u + 2]; p++) path[nord[p]] = nord[(p + 1) % n];
        if (cost) *cost += sum;
    }
    *m_out = m;
    *nacc = k;
    free(cnext); free(P); free(ord); free(sel); free(pred); free(nord);
    return 0;
}

/* rule 10 -> 0.  The cost is recomputed once; then { rule 8 of "Neighbour-list Or-opt" to its end on the running cost; the
 * 3-opt phase } until a 3-opt phase applies nothing.  Every phase counts its last, empty sweep.  first_path [n] / first
 * [6] (each may be NULL) receive the tour and (cost, two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, rounds) at the end
 * of the first rule-8 part.  *max_k the most moves one 3-opt sweep accepted.  limit_sweeps > 0 caps the sweeps of all kinds
 * together (a safety net for tests: -> 2 when it is hit). */
int t3m_descent(const double *c, const double *xy, int n, int kind, int K, int width, const int *nodes, int *path, long limit_sweeps,
                double *cost, long *two_opt_sweeps, long *two_opt_moves, long *or_sweeps, long *or_moves, int *rounds,
                long *three_sweeps, long *three_moves, int *three_phases, int *max_k, int *first_path, double *first)
{
    const src S = {c, xy, n, kind};
    double *cand_d = (double *)malloc((size_t)n * sizeof(double)), *cdl = (double *)malloc((size_t)n * sizeof(double));
    double *deltas = (double *)malloc((size_t)n * sizeof(double));
    int *ib = (int *)malloc((size_t)10 * n * sizeof(int));
    if (!cand_d || !cdl || !deltas || !ib) { free(cand_d); free(cdl); free(deltas); free(ib); return 1; }
    double total = 0.0;
    for (int i = 0; i < n; i++) total += W(&S, i, path[i]);      /* refinment.c:6-9 */
    *cost = total;
    *two_opt_sweeps = *two_opt_moves = *or_sweeps = *or_moves = *three_sweeps = *three_moves = 0;
    *rounds = *three_phases = *max_k = 0;
    int rc = 0;
    long left = limit_sweeps;
    for (int phase = 0; !rc;) {                             /* 0: list 2-opt, 1: list Or-opt, 2: list 3-opt */
        long applied = 0;
        if (phase == 0) *rounds += 1;
        if (phase == 2) *three_phases += 1;
        for (;;) {
            int m = 0, k = 0;
            if (limit_sweeps > 0 && left-- <= 0) { rc = 2; break; }
            if (phase == 0)
                rc = nlm_sweep(c, xy, n, kind, K, nodes, path, cand_d, ib, &m, ib + n, ib + 2 * n, ib + 3 * n, ib + 4 * n, cdl, ib + 5 * n,
                               &k, ib + 6 * n, deltas, cost, 1);
            else if (phase == 1)
                rc = onl_sweep(c, xy, n, kind, K, nodes, path, cand_d, ib, &m, ib + n, ib + 2 * n, ib + 3 * n, ib + 4 * n, cdl, ib + 5 * n,
                               &k, ib + 6 * n, deltas, cost, 1);
            else
                rc = t3m_sweep(c, xy, n, kind, K, width, nodes, path, cand_d, ib, &m, ib + n, ib + 2 * n, ib + 3 * n, ib + 4 * n, cdl,
                               ib + 5 * n, &k, ib + 6 * n, deltas, cost, 1);
            if (rc) break;
            *(phase == 0 ? two_opt_sweeps : phase == 1 ? or_sweeps : three_sweeps) += 1;
            *(phase == 0 ? two_opt_moves : phase == 1 ? or_moves : three_moves) += k;
            applied += k;
            if (phase == 2 && k > *max_k) *max_k = k;
            if (k == 0) break;
        }
        if (rc) break;
        if (phase == 0) phase = 1;
        else if (phase == 1 && applied) phase = 0;
        else if (phase == 1) {
            if (*three_phases == 0) {
                if (first_path) for (int i = 0; i < n; i++) first_path[i] = path[i];
                if (first) {
                    first[0] = *cost; first[1] = (double)*two_opt_sweeps; first[2] = (double)*two_opt_moves;
                    first[3] = (double)*or_sweeps; first[4] = (double)*or_moves; first[5] = (double)*rounds;
                }
            }
            phase = 2;
        } else if (applied) phase = 0;
        else break;
    }
    free(cand_d); free(cdl); free(deltas); free(ib);
    return rc;
}
