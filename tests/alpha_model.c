/* Plain C statement of the alpha-nearness of an edge under the 1-tree T(pi) of include/tspgpu.h ("Held-Karp lower bound", rules 1
 * and 2): beta(a, b), a != b both >= 1, is the largest w(e) on the path between a and b in the spanning tree of T(pi) on the nodes
 * 1 .. n - 1; beta(0, u) = w(0, u2), {0, u2} the larger of node 0's two edges; alpha = max(0, w - beta).  Lists: the K' = min(K,
 * n - 1) nodes u != v with the smallest key (alpha(v, u), c[v][u], u), ascending.  The method: the Prim tree of
 * tests/held_karp_model.c (included unmodified), then one depth-first walk per source node that carries the running maximum of the
 * path -- it shares nothing with the level rule of Boruvka rounds that tests/test_alpha_nearness.py holds against it.
 *   alm_all_pairs  alpha(a, b) for every ordered pair, [n][n], the diagonal 0;
 *   alm_row        alpha(v, .) and c[v][.] from a GIVEN edge list of a 1-tree (n pairs, node 0's two among them), O(n);
 *   alm_lists      A(v) for every v by a plain sort on the key (alpha, c, u).
 * Among the nodes >= 1, w >= beta follows from the cut property: it is asserted (code 3).
 * All arithmetic is in 64-bit integers, in units of 1/128 of a cost unit.
 * gcc -O2 -ffp-contract=off -shared -fPIC -pthread. */
#include "held_karp_model.c"

typedef struct {
    int n;
    int *head, *next, *to;      /* adjacency of the spanning tree on 1 .. n - 1: 2 (n - 2) arcs */
    int *stack, *par;
    i64 *beta;
    i64 b0;                     /* w(0, u2) */
} walk;

static void walk_free(walk *K) { free(K->head); free(K->next); free(K->to); free(K->stack); free(K->par); free(K->beta); }

/* edges: n pairs a < b; the two with a == 0 are node 0's.  -> 0; 1: memory; 2: the list is no 1-tree */
static int walk_init(walk *K, const src *S, const i64 *pi, const int *edges)
{
    const int n = S->n;
    memset(K, 0, sizeof *K);
    K->n = n;
    K->head = (int *)malloc((size_t)n * sizeof(int)); K->next = (int *)malloc((size_t)n * 2 * sizeof(int));
    K->to = (int *)malloc((size_t)n * 2 * sizeof(int)); K->stack = (int *)malloc((size_t)n * sizeof(int));
    K->par = (int *)malloc((size_t)n * sizeof(int)); K->beta = (i64 *)malloc((size_t)n * sizeof(i64));
    if (!(K->head && K->next && K->to && K->stack && K->par && K->beta)) return 1;
    for (int v = 0; v < n; v++) K->head[v] = -1;
    int arcs = 0, zeros = 0, z[2] = {-1, -1};
    for (int k = 0; k < n; k++) {
        const int a = edges[2 * k], b = edges[2 * k + 1];
        if (a < 0 || b <= a || b >= n) return 2;
        if (a == 0) { if (zeros < 2) z[zeros] = b; zeros++; continue; }
        K->to[arcs] = b; K->next[arcs] = K->head[a]; K->head[a] = arcs++;
        K->to[arcs] = a; K->next[arcs] = K->head[b]; K->head[b] = arcs++;
    }
    if (zeros != 2 || arcs != 2 * (n - 2)) return 2;
    const i64 w0 = hk_w(S, pi, 0, z[0]), w1 = hk_w(S, pi, 0, z[1]);
    K->b0 = hk_lt(w0, 0, z[0], w1, 0, z[1]) ? w1 : w0;         /* the larger key of the two */
    return 0;
}

/* beta(a, .) over the nodes >= 1 into K->beta (beta[a] itself is not defined: LLONG_MIN); a >= 1.  -> 0; 2: the tree is not connected */
static int walk_from(walk *K, const src *S, const i64 *pi, int a)
{
    int top = 0, seen = 1;
    K->stack[top++] = a; K->par[a] = -1; K->beta[a] = LLONG_MIN;
    while (top) {
        const int v = K->stack[--top];
        for (int e = K->head[v]; e >= 0; e = K->next[e]) {
            const int u = K->to[e];
            if (u == K->par[v]) continue;
            const i64 w = hk_w(S, pi, v < u ? v : u, v < u ? u : v);
            K->par[u] = v;
            K->beta[u] = w > K->beta[v] ? w : K->beta[v];
            K->stack[top++] = u; seen++;
            if (seen > K->n) return 2;
        }
    }
    return seen == K->n - 1 ? 0 : 2;
}

/* alpha(v, .) [n] (alpha[v] = 0) and, where cost != NULL, c[v][.] (cost[v] = -1).  -> 0; 2; 3: w < beta among the nodes >= 1 */
static int row_of(walk *K, const src *S, const i64 *pi, int v, i64 *alpha, i64 *cost)
{
    const int n = S->n;
    int rc = 0;
    if (v >= 1 && (rc = walk_from(K, S, pi, v))) return rc;
    for (int u = 0; u < n; u++) {
        if (u == v) { alpha[u] = 0; if (cost) cost[u] = -1; continue; }
        const int a = v < u ? v : u, b = v < u ? u : v;
        const i64 w = hk_w(S, pi, a, b);
        i64 beta;
        if (a == 0) beta = K->b0;
        else { beta = K->beta[u]; if (w < beta) return 3; }
        alpha[u] = w > beta ? w - beta : 0;
        if (cost) cost[u] = (i64)W(S, a, b);
    }
    return 0;
}

static i64 *pi_copy(const i64 *pi, int n)
{
    i64 *p = (i64 *)calloc((size_t)n, sizeof(i64));
    if (p && pi) memcpy(p, pi, (size_t)n * sizeof(i64));
    return p;
}

/* the model's own tree -> edges (malloc'd [2n]).  -> 0; 1; 2 */
static int model_tree(const src *S, const i64 *p, int **edges_out)
{
    const int n = S->n;
    i64 *bw = (i64 *)malloc((size_t)n * sizeof(i64)), sum = 0;
    int *bu = (int *)malloc((size_t)n * sizeof(int)), *e = (int *)malloc((size_t)n * 2 * sizeof(int)), *d = (int *)malloc((size_t)n * sizeof(int));
    char *in = (char *)malloc((size_t)n);
    int rc = 1;
    if (bw && bu && e && d && in) rc = one_tree(S, p, e, d, &sum, bw, bu, in);
    free(bw); free(bu); free(d); free(in);
    if (rc) { free(e); e = NULL; }
    *edges_out = e;
    return rc;
}

int alm_row(const double *c, const double *xy, int n, int kind, const i64 *pi, const int *edges, int v, i64 *alpha, i64 *cost)
{
    const src S = {c, xy, n, kind};
    i64 *p = pi_copy(pi, n);
    walk K;
    int rc = p ? walk_init(&K, &S, p, edges) : 1;
    if (!p) memset(&K, 0, sizeof K);
    if (rc == 0) rc = (v < 0 || v >= n) ? 2 : row_of(&K, &S, p, v, alpha, cost);
    walk_free(&K); free(p);
    return rc;
}

int alm_all_pairs(const double *c, const double *xy, int n, int kind, const i64 *pi, i64 *alpha /* [n][n] */)
{
    const src S = {c, xy, n, kind};
    i64 *p = pi_copy(pi, n);
    int *edges = NULL;
    walk K;
    memset(&K, 0, sizeof K);
    int rc = p ? model_tree(&S, p, &edges) : 1;
    if (rc == 0) rc = walk_init(&K, &S, p, edges);
    for (int v = 0; v < n && rc == 0; v++) rc = row_of(&K, &S, p, v, alpha + (size_t)v * n, NULL);
    walk_free(&K); free(edges); free(p);
    return rc;
}

typedef struct { i64 alpha, cost; int u; } cand;

static int cand_cmp(const void *x, const void *y)
{
    const cand *p = (const cand *)x, *q = (const cand *)y;
    if (p->alpha != q->alpha) return p->alpha < q->alpha ? -1 : 1;
    if (p->cost != q->cost) return p->cost < q->cost ? -1 : 1;
    return p->u < q->u ? -1 : p->u > q->u;
}

/* the lists for every v: nodes [n][K'], costs [n][K'], K' = min(K, n - 1) */
int alm_lists(const double *c, const double *xy, int n, int kind, const i64 *pi, int K, int *nodes, i64 *costs)
{
    const src S = {c, xy, n, kind};
    const int Kp = K < n - 1 ? K : n - 1;
    i64 *p = pi_copy(pi, n), *al = (i64 *)malloc((size_t)n * sizeof(i64)), *co = (i64 *)malloc((size_t)n * sizeof(i64));
    cand *cs = (cand *)malloc((size_t)n * sizeof(cand));
    int *edges = NULL;
    walk K_;
    memset(&K_, 0, sizeof K_);
    int rc = (p && al && co && cs) ? model_tree(&S, p, &edges) : 1;
    if (rc == 0) rc = walk_init(&K_, &S, p, edges);
    for (int v = 0; v < n && rc == 0; v++) {
        if ((rc = row_of(&K_, &S, p, v, al, co))) break;
        int m = 0;
        for (int u = 0; u < n; u++)
            if (u != v) { cs[m].alpha = al[u]; cs[m].cost = co[u]; cs[m].u = u; m++; }
        qsort(cs, (size_t)m, sizeof(cand), cand_cmp);
        for (int j = 0; j < Kp; j++) { nodes[(size_t)v * Kp + j] = cs[j].u; costs[(size_t)v * Kp + j] = cs[j].cost; }
    }
    walk_free(&K_); free(edges); free(p); free(al); free(co); free(cs);
    return rc;
}
