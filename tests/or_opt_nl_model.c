/* Plain C restatement of the neighbour-list Or-opt defined in include/tspgpu.h ("Neighbour-list Or-opt", rules 1-8): the
 * candidates of a sweep, the one selection round, the apply and the descent that alternates with the neighbour-list 2-opt,
 * over a double matrix (c != NULL) or over coordinates (c == NULL).  two_opt_nl_model.c is included unmodified for its cost
 * source (src, W), the lists (nlm_lists) and the 2-opt phase of the descent (nlm_sweep).
 * tests/test_or_opt_nl.py pins this file to a brute-force Python restatement; tools/make_golden_or_opt_nl.py runs it where
 * it takes more than a few seconds.
 * gcc -O2 -ffp-contract=off -shared -fPIC -pthread. */
#include "two_opt_nl_model.c"

#define ONL_PACK(L, q, rev) ((L) << 18 | (q) << 1 | (rev))

/* key (delta, s, L, q, rev); pk = the packed (L, q, rev) */
static int onl_key_less(double d1, int s1, int pk1, double d2, int s2, int pk2)
{
    if (d1 != d2) return d1 < d2;
    if (s1 != s2) return s1 < s2;
    return pk1 < pk2;
}

/* One sweep over the lists `nodes` [n * K].  Out, [n] each: cand_d / cand_b by segment start (rule 2, before the threshold;
 * cand_b the packed (L, q, rev), -1 and DBL_MAX where s has no candidate); the m candidates in ascending s -- cs the start,
 * cb the packed move, ci / cj the range [lo, hi] of rule 4, cdl the delta, acc 1 when accepted (rule 5); the accepted ones
 * again in ascending key order in moves [4 nacc] (s, L, q, rev) / deltas.  apply != 0: rule 6 on path and *cost.
 * -> 0, or 1 when memory ran out. */
int onl_sweep(const double *c, const double *xy, int n, int kind, int K, const int *nodes, int *path,
              double *cand_d, int *cand_b, int *m_out, int *cs, int *cb, int *ci, int *cj, double *cdl, int *acc,
              int *nacc, int *moves, double *deltas, double *cost, int apply)
{
    const src S = {c, xy, n, kind};
    double *cnext = (double *)malloc((size_t)n * sizeof(double));
    int *P = (int *)malloc((size_t)n * sizeof(int)), *ord = (int *)malloc((size_t)n * sizeof(int));
    int *sel = (int *)malloc((size_t)n * sizeof(int)), *pred = (int *)malloc((size_t)n * sizeof(int));
    if (!cnext || !P || !ord || !sel || !pred) { free(cnext); free(P); free(ord); free(sel); free(pred); return 1; }
    for (int v = 0; v < n; v++) { cnext[v] = W(&S, v, path[v]); pred[path[v]] = v; }
    for (int i = 0, v = 0; i < n; i++, v = path[v]) { P[v] = i; ord[i] = v; }
    for (int s = 0; s < n; s++) {
        double best = DBL_MAX;
        int bk = -1;
        const int p = pred[s];
        int seg[3];
        seg[0] = s; seg[1] = path[s]; seg[2] = path[seg[1]];
        for (int L = 1; L <= 3; L++) {
            const int t = seg[L - 1], x = path[t];
            if (t == 0 || s == 0) break;                    /* the segment holds node 0, and so does every longer one */
            const double cpx = W(&S, p, x), rem0 = cnext[p] + cnext[t];
            for (int end = 0; end < (L == 1 ? 1 : 2); end++) {
                const int w = end ? t : s;
                for (int j = 0; j < K; j++) {
                    const int u = nodes[(size_t)w * K + j];
                    for (int form = 0; form < 2; form++) {
                        /* (A) q = u, h = w; (B) q' = u, e = w */
                        const int q = form ? pred[u] : u, qn = path[q];
                        if (q == p || q == seg[0] || (L > 1 && q == seg[1]) || (L > 2 && q == seg[2])) continue;
                        const int rev = L == 1 ? 0 : form ? (w == s) : (w == t);
                        const int h = rev ? t : s, e = rev ? s : t;
                        const double d = ((cpx + W(&S, q, h)) + W(&S, e, qn)) - (rem0 + cnext[q]);
                        const int pk = ONL_PACK(L, q, rev);
                        if (bk < 0 || d < best || (d == best && pk < bk)) { best = d; bk = pk; }
                    }
                }
            }
        }
        cand_d[s] = best;
        cand_b[s] = bk;
    }
    int m = 0;
    for (int s = 0; s < n; s++) {
        const int pk = cand_b[s];
        if (pk < 0 || !(cand_d[s] < EPS)) continue;
        const int L = pk >> 18, q = (pk >> 1) & 0x1ffff, i = P[s], j = P[q];
        cs[m] = s; cb[m] = pk; cdl[m] = cand_d[s];
        ci[m] = i - 1 < j ? i - 1 : j;                      /* rule 4 */
        cj[m] = i + L - 1 > j ? i + L - 1 : j;
        m++;
    }
    int k = 0;
    for (int x = 0; x < m; x++) {                           /* rule 5: one round */
        int ok = 1;
        for (int y = 0; y < m && ok; y++)
            if (y != x && ci[y] <= cj[x] && ci[x] <= cj[y] && !onl_key_less(cdl[x], cs[x], cb[x], cdl[y], cs[y], cb[y])) ok = 0;
        acc[x] = ok;
        if (ok) sel[k++] = x;
    }
    for (int u = 1; u < k; u++) {                           /* ascending key */
        const int x = sel[u];
        int v = u;
        while (v > 0 && onl_key_less(cdl[x], cs[x], cb[x], cdl[sel[v - 1]], cs[sel[v - 1]], cb[sel[v - 1]])) { sel[v] = sel[v - 1]; v--; }
        sel[v] = x;
    }
    double sum = 0.0;
    for (int u = 0; u < k; u++) {
        const int x = sel[u], s = cs[x], pk = cb[x], L = pk >> 18, q = (pk >> 1) & 0x1ffff, rev = pk & 1;
        moves[4 * u] = s; moves[4 * u + 1] = L; moves[4 * u + 2] = q; moves[4 * u + 3] = rev;
        deltas[u] = cdl[x];
        sum += cdl[x];
        if (apply) {                                        /* rule 6, from the positions before the sweep (the ranges are disjoint) */
            const int i = P[s], g1 = ord[(i + 1) % n], g2 = ord[(i + 2) % n];
            const int t = L == 1 ? s : L == 2 ? g1 : g2;
            const int p = ord[i - 1], x2 = ord[(i + L) % n], qn = ord[(P[q] + 1) % n];
            const int h = rev ? t : s, e = rev ? s : t;
            path[p] = x2;
            path[q] = h;
            if (rev && L == 2) path[g1] = s;
            if (rev && L == 3) { path[g2] = g1; path[g1] = s; }
            path[e] = qn;
        }
    }
    if (apply && cost) *cost += sum;
    *m_out = m;
    *nacc = k;
    free(cnext); free(P); free(ord); free(sel); free(pred);
    return 0;
}

/* rule 8 -> 0.  Every phase counts its last, empty sweep; *rounds the 2-opt phases; *max_k the most moves one Or-opt sweep
 * accepted.  limit_sweeps > 0 caps the sweeps of both kinds together (a safety net for tests: -> 2 when it is hit). */
int onl_descent(const double *c, const double *xy, int n, int kind, int K, const int *nodes, int *path, long limit_sweeps,
                double *cost, long *two_opt_sweeps, long *two_opt_moves, long *or_sweeps, long *or_moves, int *rounds, int *max_k)
{
    const src S = {c, xy, n, kind};
    double *cand_d = (double *)malloc((size_t)n * sizeof(double)), *cdl = (double *)malloc((size_t)n * sizeof(double));
    double *deltas = (double *)malloc((size_t)n * sizeof(double));
    int *ib = (int *)malloc((size_t)10 * n * sizeof(int));
    if (!cand_d || !cdl || !deltas || !ib) { free(cand_d); free(cdl); free(deltas); free(ib); return 1; }
    double total = 0.0;
    for (int i = 0; i < n; i++) total += W(&S, i, path[i]);      /* refinment.c:6-9 */
    *cost = total;
    *two_opt_sweeps = *two_opt_moves = *or_sweeps = *or_moves = 0;
    *rounds = *max_k = 0;
    int rc = 0;
    long left = limit_sweeps;
    for (int phase = 0; !rc; phase ^= 1) {
        long applied = 0;
        if (phase == 0) *rounds += 1;
        for (;;) {
            int m = 0, k = 0;
            if (limit_sweeps > 0 && left-- <= 0) { rc = 2; break; }
            if (phase == 0)
                rc = nlm_sweep(c, xy, n, kind, K, nodes, path, cand_d, ib, &m, ib + n, ib + 2 * n, ib + 3 * n, ib + 4 * n, cdl, ib + 5 * n,
                               &k, ib + 6 * n, deltas, cost, 1);
            else
                rc = onl_sweep(c, xy, n, kind, K, nodes, path, cand_d, ib, &m, ib + n, ib + 2 * n, ib + 3 * n, ib + 4 * n, cdl, ib + 5 * n,
                               &k, ib + 6 * n, deltas, cost, 1);
            if (rc) break;
            *(phase ? or_sweeps : two_opt_sweeps) += 1;
            *(phase ? or_moves : two_opt_moves) += k;
            applied += k;
            if (phase && k > *max_k) *max_k = k;
            if (k == 0) break;
        }
        if (phase && applied == 0) break;
    }
    free(cand_d); free(cdl); free(deltas); free(ib);
    return rc;
}
