/* Plain C restatement of the greedy-edge construction defined in include/tspgpu.h ("Greedy-edge construction"), over a double
 * matrix (c != NULL) or over coordinates (c == NULL, the weights of two_opt_multi_model.c).  two_opt_nl_model.c is included
 * unmodified for its cost source (src, W) and its lists (nlm_lists).
 *   gem_greedy  the sequential rule: E1 sorted by key and taken in order, then E2 sorted and taken in order (rules 3-5);
 *   gem_rounds  the parallel form (rule 7): rounds of locally dominant edges, which is what the device runs -- it gives the
 *               round counts of the golden, and tests/test_greedy_edge.py holds both to a Python restatement and to each other.
 * Both return the successor array from node 0 (rule 5), the cost summed in node order, the edges at every node before the
 * closing edge (adj[2v] <= adj[2v + 1], -1: none), the edges phase 1 accepted and the free nodes entering phase 2.
 * gcc -O2 -ffp-contract=off -shared -fPIC -pthread. */
#include "two_opt_nl_model.c"
#include <string.h>

typedef struct { double w; int a, b; } gedge;

static int gedge_cmp(const void *x, const void *y)
{
    const gedge *p = (const gedge *)x, *q = (const gedge *)y;
    if (p->w != q->w) return p->w < q->w ? -1 : 1;
    if (p->a != q->a) return p->a < q->a ? -1 : 1;
    return p->b < q->b ? -1 : p->b > q->b;
}

static int key_lt(double w1, int a1, int b1, double w2, int a2, int b2)
{
    if (w1 != w2) return w1 < w2;
    if (a1 != a2) return a1 < a2;
    return b1 < b2;
}

typedef struct { int n, count; int *deg, *oe, *adj; } frag;

static int frag_new(frag *F, int n)
{
    F->n = n; F->count = 0;
    F->deg = (int *)calloc((size_t)n, sizeof(int));
    F->oe = (int *)malloc((size_t)n * sizeof(int));
    F->adj = (int *)malloc((size_t)n * 2 * sizeof(int));
    if (!F->deg || !F->oe || !F->adj) return 1;
    for (int v = 0; v < n; v++) { F->oe[v] = v; F->adj[2 * v] = F->adj[2 * v + 1] = -1; }
    return 0;
}

static void frag_free(frag *F) { free(F->deg); free(F->oe); free(F->adj); }

static int frag_valid(const frag *F, int a, int b) { return a != b && F->deg[a] < 2 && F->deg[b] < 2 && F->oe[a] != b; }

static void frag_link(frag *F, int a, int b)
{
    const int oa = F->oe[a], ob = F->oe[b];
    F->adj[2 * a + F->deg[a]++] = b;
    F->adj[2 * b + F->deg[b]++] = a;
    F->oe[oa] = ob; F->oe[ob] = oa;
    F->count++;
}

/* the edges before the closing one, then the closed tour from node 0 towards its smaller neighbour, and its cost in node order */
static int frag_finish(frag *F, const src *S, int *adj_out, int *path, double *cost)
{
    const int n = F->n;
    if (F->count != n - 1) return 2;
    for (int v = 0; v < n; v++) {
        int x = F->adj[2 * v], y = F->adj[2 * v + 1];
        if (y >= 0 && y < x) { const int t = x; x = y; y = t; }      /* (a node with one edge shows (u, -1)) */
        adj_out[2 * v] = x; adj_out[2 * v + 1] = y;
    }
    for (int v = 0; v < n; v++)
        if (F->deg[v] == 1) F->adj[2 * v + 1] = F->oe[v];
    int prev = 0, v = F->adj[0] < F->adj[1] ? F->adj[0] : F->adj[1];
    path[0] = v;
    for (int k = 1; k < n; k++) {
        const int next = F->adj[2 * v] == prev ? F->adj[2 * v + 1] : F->adj[2 * v];
        path[v] = next; prev = v; v = next;
    }
    if (v != 0) return 3;
    double total = 0;
    for (int i = 0; i < n; i++) total += W(S, i, path[i]);
    *cost = total;
    return 0;
}

static int free_list(const frag *F, int *fl)
{
    int m = 0;
    for (int v = 0; v < F->n; v++)
        if (F->deg[v] < 2) fl[m++] = v;
    return m;
}

/* -> 0; 1: memory ran out; 2, 3: the result is no tour (a mistake in this file) */
int gem_greedy(const double *c, const double *xy, int n, int kind, int K, const int *nodes, int *path, double *cost, int *adj_out,
               int *edges1, int *free_nodes)
{
    const src S = {c, xy, n, kind};
    frag F;
    if (frag_new(&F, n)) return 1;
    int rc = 0;
    size_t m1 = 0;
    gedge *E = (gedge *)malloc((size_t)n * K * sizeof(gedge));
    int *fl = (int *)malloc((size_t)n * sizeof(int));
    if (!E || !fl) { rc = 1; goto out; }
    for (int v = 0; v < n; v++)
        for (int j = 0; j < K; j++) {
            const int u = nodes[(size_t)v * K + j], a = v < u ? v : u, b = v < u ? u : v;
            const gedge e = {W(&S, a, b), a, b};
            E[m1++] = e;
        }
    qsort(E, m1, sizeof(gedge), gedge_cmp);
    for (size_t i = 0; i < m1; i++)
        if (frag_valid(&F, E[i].a, E[i].b)) frag_link(&F, E[i].a, E[i].b);      /* (the second copy of an edge is never valid) */
    *edges1 = F.count;
    const int m = free_list(&F, fl);
    *free_nodes = m;
    free(E);
    E = (gedge *)malloc(((size_t)m * (m - 1) / 2 + 1) * sizeof(gedge));
    if (!E) { rc = 1; goto out; }
    size_t m2 = 0;
    for (int i = 0; i < m; i++)
        for (int j = i + 1; j < m; j++) {
            const gedge e = {W(&S, fl[i], fl[j]), fl[i], fl[j]};
            E[m2++] = e;
        }
    qsort(E, m2, sizeof(gedge), gedge_cmp);
    for (size_t i = 0; i < m2 && F.count < n - 1; i++)
        if (frag_valid(&F, E[i].a, E[i].b)) frag_link(&F, E[i].a, E[i].b);
    rc = frag_finish(&F, &S, adj_out, path, cost);
out:
    free(E); free(fl); frag_free(&F);
    return rc;
}

/* one round behind best(): the lower end of best(a) = {a, b} accepts it iff it is best(b) too and smaller than the bests of the
 * far ends of both fragments; every accepted edge is linked only after all were decided.  live[0 .. m): the nodes of degree < 2;
 * bw / ba / bb: best(v), ba < 0: none.  -> edges accepted */
static int round_accept(frag *F, const int *live, int m, const double *bw, const int *ba, const int *bb, int *take)
{
    int k = 0;
    for (int i = 0; i < m; i++) {
        const int a = live[i];
        if (ba[a] != a) continue;
        const int b = bb[a];
        if (ba[b] != a || bb[b] != b) continue;
        const int oa = F->oe[a], ob = F->oe[b];
        if (oa != a && ba[oa] >= 0 && !key_lt(bw[a], a, b, bw[oa], ba[oa], bb[oa])) continue;
        if (ob != b && ba[ob] >= 0 && !key_lt(bw[a], a, b, bw[ob], ba[ob], bb[ob])) continue;
        take[k++] = a;
    }
    for (int i = 0; i < k; i++) frag_link(F, take[i], bb[take[i]]);
    return k;
}

static void post(double *bw, int *ba, int *bb, int v, double w, int a, int b)
{
    if (ba[v] < 0 || key_lt(w, a, b, bw[v], ba[v], bb[v])) { bw[v] = w; ba[v] = a; bb[v] = b; }
}

int gem_rounds(const double *c, const double *xy, int n, int kind, int K, const int *nodes, int *path, double *cost, int *adj_out,
               int *edges1, int *free_nodes, int *rounds1, int *rounds2)
{
    const src S = {c, xy, n, kind};
    frag F;
    if (frag_new(&F, n)) return 1;
    int rc = 0;
    double *bw = (double *)malloc((size_t)n * sizeof(double));
    int *ba = (int *)malloc((size_t)n * sizeof(int)), *bb = (int *)malloc((size_t)n * sizeof(int));
    int *live = (int *)malloc((size_t)n * sizeof(int)), *take = (int *)malloc((size_t)n * sizeof(int));
    if (!bw || !ba || !bb || !live || !take) { rc = 1; goto out; }
    *rounds1 = *rounds2 = 0;
    for (;;) {                              /* phase 1: the list edges, posted to both ends */
        const int m = free_list(&F, live);
        for (int i = 0; i < m; i++) ba[live[i]] = -1;
        for (int i = 0; i < m; i++) {
            const int v = live[i];
            for (int j = 0; j < K; j++) {
                const int u = nodes[(size_t)v * K + j];
                if (!frag_valid(&F, v, u)) continue;
                const int a = v < u ? v : u, b = v < u ? u : v;
                const double w = W(&S, a, b);
                post(bw, ba, bb, v, w, a, b);
                post(bw, ba, bb, u, w, a, b);
            }
        }
        if (!round_accept(&F, live, m, bw, ba, bb, take)) break;
        ++*rounds1;
    }
    *edges1 = F.count;
    *free_nodes = free_list(&F, live);
    while (F.count < n - 1) {               /* phase 2: all pairs of free nodes */
        const int m = free_list(&F, live);
        for (int i = 0; i < m; i++) ba[live[i]] = -1;
        for (int i = 0; i < m; i++)
            for (int j = i + 1; j < m; j++) {
                const int a = live[i], b = live[j];
                if (!frag_valid(&F, a, b)) continue;
                const double w = W(&S, a, b);
                post(bw, ba, bb, a, w, a, b);
                post(bw, ba, bb, b, w, a, b);
            }
        if (!round_accept(&F, live, m, bw, ba, bb, take)) { rc = 2; goto out; }
        ++*rounds2;
    }
    rc = frag_finish(&F, &S, adj_out, path, cost);
out:
    free(bw); free(ba); free(bb); free(live); free(take); frag_free(&F);
    return rc;
}
