/* Plain C restatement of the Held-Karp lower bound defined in include/tspgpu.h ("Held-Karp lower bound"), over a double matrix
 * of integer values (c != NULL) or over coordinates (c == NULL, the weights of two_opt_multi_model.c, which is included
 * unmodified for its cost source (src, W)).
 *   hkm_one_tree  rule 2: Prim in O(n^2) under the key order (w, a, b) over the nodes 1 .. n - 1, then node 0's two smallest keys;
 *   hkm_ascent    rule 3, literally.
 * All arithmetic is in 64-bit integers, in units of 1/128 of a cost unit.
 * gcc -O2 -ffp-contract=off -shared -fPIC -pthread. */
#include "two_opt_multi_model.c"
#include <limits.h>
#include <string.h>

#define HK_S 128
#define HK_PI_MAX (1ll << 45)
typedef long long i64;

static i64 hk_w(const src *S, const i64 *pi, int a, int b) { return HK_S * (i64)W(S, a, b) + pi[a] + pi[b]; }

static int hk_lt(i64 w1, int a1, int b1, i64 w2, int a2, int b2)
{
    if (w1 != w2) return w1 < w2;
    if (a1 != a2) return a1 < a2;
    return b1 < b2;
}

static int pair_cmp(const void *x, const void *y)
{
    const int *p = (const int *)x, *q = (const int *)y;
    if (p[0] != q[0]) return p[0] < q[0] ? -1 : 1;
    return p[1] < q[1] ? -1 : p[1] > q[1];
}

/* T(pi): edges [2n] (n pairs a < b, ascending by pair), deg [n], the sum of w over T; scratch: bw [n], bu [n], in [n].  -> 0 */
static int one_tree(const src *S, const i64 *pi, int *edges, int *deg, i64 *wsum, i64 *bw, int *bu, char *in)
{
    const int n = S->n;
    int m = 0;
    i64 sum = 0;
    memset(deg, 0, (size_t)n * sizeof(int));
    memset(in, 0, (size_t)n);
    in[1] = 1;
    for (int v = 2; v < n; v++) { bw[v] = hk_w(S, pi, 1, v); bu[v] = 1; }
    for (int k = 2; k < n; k++) {
        int best = -1;
        for (int v = 2; v < n; v++) {
            if (in[v]) continue;
            if (best < 0) { best = v; continue; }
            const int a1 = v < bu[v] ? v : bu[v], b1 = v < bu[v] ? bu[v] : v;
            const int a2 = best < bu[best] ? best : bu[best], b2 = best < bu[best] ? bu[best] : best;
            if (hk_lt(bw[v], a1, b1, bw[best], a2, b2)) best = v;
        }
        const int u = bu[best];
        edges[2 * m] = best < u ? best : u; edges[2 * m + 1] = best < u ? u : best; m++;
        deg[best]++; deg[u]++; sum += bw[best];
        in[best] = 1;
        for (int v = 2; v < n; v++) {
            if (in[v]) continue;
            const i64 w = hk_w(S, pi, best < v ? best : v, best < v ? v : best);
            const int a1 = v < best ? v : best, b1 = v < best ? best : v;
            const int a2 = v < bu[v] ? v : bu[v], b2 = v < bu[v] ? bu[v] : v;
            if (hk_lt(w, a1, b1, bw[v], a2, b2)) { bw[v] = w; bu[v] = best; }
        }
    }
    int u1 = -1, u2 = -1;                   /* node 0: the two smallest keys (w, 0, u) */
    i64 w1 = 0, w2 = 0;
    for (int u = 1; u < n; u++) {
        const i64 w = hk_w(S, pi, 0, u);
        if (u1 < 0 || w < w1) { u2 = u1; w2 = w1; u1 = u; w1 = w; }
        else if (u2 < 0 || w < w2) { u2 = u; w2 = w; }
    }
    edges[2 * m] = 0; edges[2 * m + 1] = u1; m++;
    edges[2 * m] = 0; edges[2 * m + 1] = u2; m++;
    deg[0] = 2; deg[u1]++; deg[u2]++; sum += w1 + w2;
    if (m != n) return 2;
    qsort(edges, (size_t)n, 2 * sizeof(int), pair_cmp);
    *wsum = sum;
    return 0;
}

/* -> 0; 1: memory ran out; 2: a mistake in this file.  pi NULL: all zero; edges, deg may be NULL */
int hkm_one_tree(const double *c, const double *xy, int n, int kind, const i64 *pi, int *edges, int *deg, i64 *L)
{
    const src S = {c, xy, n, kind};
    i64 *p = (i64 *)calloc((size_t)n, sizeof(i64)), *bw = (i64 *)malloc((size_t)n * sizeof(i64));
    int *bu = (int *)malloc((size_t)n * sizeof(int)), *e = (int *)malloc((size_t)n * 2 * sizeof(int)), *d = (int *)malloc((size_t)n * sizeof(int));
    char *in = (char *)malloc((size_t)n);
    int rc = 1;
    if (p && bw && bu && e && d && in) {
        i64 sum = 0, spi = 0;
        if (pi) memcpy(p, pi, (size_t)n * sizeof(i64));
        rc = one_tree(&S, p, e, d, &sum, bw, bu, in);
        for (int v = 0; v < n; v++) spi += p[v];
        *L = sum - 2 * spi;
        if (edges) memcpy(edges, e, (size_t)n * 2 * sizeof(int));
        if (deg) memcpy(deg, d, (size_t)n * sizeof(int));
    }
    free(p); free(bw); free(bu); free(e); free(d); free(in);
    return rc;
}

/* the tour a 1-tree with every degree 2 is, from node 0 towards the smaller of its two neighbours -> successor array */
static int tree_tour(int n, const int *edges, int *path)
{
    int *adj = (int *)malloc((size_t)n * 2 * sizeof(int)), *cnt = (int *)calloc((size_t)n, sizeof(int));
    if (!adj || !cnt) { free(adj); free(cnt); return 1; }
    for (int k = 0; k < n; k++) {
        const int a = edges[2 * k], b = edges[2 * k + 1];
        adj[2 * a + cnt[a]++] = b; adj[2 * b + cnt[b]++] = a;
    }
    int prev = 0, v = adj[0] < adj[1] ? adj[0] : adj[1], rc = 0;
    path[0] = v;
    for (int k = 1; k < n; k++) {
        const int next = adj[2 * v] == prev ? adj[2 * v + 1] : adj[2 * v];
        path[v] = next; prev = v; v = next;
    }
    if (v != 0) rc = 2;
    free(adj); free(cnt);
    return rc;
}

/* rule 3.  best: the largest L (units of 1/128); bound = ceil(best / 128) is the caller's.  path [n] is written on reason 1 */
int hkm_ascent(const double *c, const double *xy, int n, int kind, i64 UB, int iters, int patience, const i64 *pi_in, i64 *best_out,
               i64 *pi_out, int *path, int *iters_done, int *reason, int *h_out)
{
    const src S = {c, xy, n, kind};
    i64 *p = (i64 *)calloc((size_t)n, sizeof(i64)), *pb = (i64 *)calloc((size_t)n, sizeof(i64)), *bw = (i64 *)malloc((size_t)n * sizeof(i64));
    int *bu = (int *)malloc((size_t)n * sizeof(int)), *e = (int *)malloc((size_t)n * 2 * sizeof(int)), *d = (int *)malloc((size_t)n * sizeof(int));
    char *in = (char *)malloc((size_t)n);
    int rc = 1;
    if (!(p && pb && bw && bu && e && d && in)) goto out;
    if (pi_in) memcpy(p, pi_in, (size_t)n * sizeof(i64));
    int h = 0, bad = 0, have = 0, it = 0, why = 0;
    i64 best = 0;
    for (; it < iters; ) {
        i64 sum = 0, spi = 0, q = 0;
        if ((rc = one_tree(&S, p, e, d, &sum, bw, bu, in))) goto out;
        for (int v = 0; v < n; v++) spi += p[v];
        const i64 L = sum - 2 * spi;
        if (!have || L > best) { best = L; have = 1; memcpy(pb, p, (size_t)n * sizeof(i64)); bad = 0; }
        else if (++bad >= patience) { h++; bad = 0; }
        it++;
        for (int v = 0; v < n; v++) q += (i64)(d[v] - 2) * (d[v] - 2);
        if (q == 0) { why = 1; if (path && (rc = tree_tour(n, e, path))) goto out; break; }
        const i64 gap = HK_S * UB - L;
        if (gap <= 0) { why = 2; break; }
        const i64 t = h >= 62 ? 0 : ((2 * gap) >> h) / q;
        if (t == 0) { why = 3; break; }
        int over = 0;
        for (int v = 0; v < n; v++) {
            const i64 x = p[v] + t * (d[v] - 2);
            if (x > HK_PI_MAX || x < -HK_PI_MAX) over = 1;
        }
        if (over) { why = 5; break; }
        for (int v = 0; v < n; v++) p[v] += t * (d[v] - 2);
    }
    rc = 0;
    *best_out = best; *iters_done = it; *reason = why; *h_out = h;
    if (pi_out) memcpy(pi_out, pb, (size_t)n * sizeof(i64));
out:
    free(p); free(pb); free(bw); free(bu); free(e); free(d); free(in);
    return rc;
}
