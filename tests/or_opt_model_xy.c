/* The Or-opt sweep of include/tspgpu.h ("Or-opt") restated over COORDINATES, for the sizes where no n x n matrix can be
 * held (tests/test_or_opt_matrix_free.py, tools/make_golden_or_opt_matrix_free.py).  The weights are the TSPLIB 95
 * definitions as the project computes them: EUC_2D (0) the float root of the double sum, rounded; ATT (1); CEIL_2D (2).
 * The tour is walked position by position; thread k takes a stripe of positions and keeps, for the three nodes a
 * segment that starts at the position can hold, one array of weights to every q -- n weights per position instead of six
 * per (position, q).  The result is the lexicographic minimum of (delta, s, L, q, rev), the definition's order, whatever
 * the stripes; the CPU test pins it to the plain model of tests/test_or_opt.py.
 * gcc -O2 -ffp-contract=off -shared -fPIC -pthread. */
#include <float.h>
#include <math.h>
#include <pthread.h>
#include <stdlib.h>

static double weight(const double *xy, int kind, int a, int b)
{
    const double dx = xy[2 * b] - xy[2 * a], dy = xy[2 * b + 1] - xy[2 * a + 1];
    const double sq = dx * dx + dy * dy;
    if (kind == 0) return (double)((int)((double)sqrtf((float)sq) + 0.5));
    if (kind == 1) {
        const double r = sqrt(sq / 10.0), t = (double)(long)(r + 0.5);
        return t < r ? t + 1.0 : t;
    }
    return ceil(sqrt(sq));
}

typedef struct {
    const double *xy; const int *path, *ord; const double *cnext;     /* cnext[v] = c[v][path[v]] */
    int n, kind, k0, k1;
    double best; int mv[4];
} job;

static int better(double d, int s, int L, int q, int rev, const job *J)
{
    if (d != J->best) return d < J->best;
    if (J->mv[0] < 0) return 1;
    if (s != J->mv[0]) return s < J->mv[0];
    if (L != J->mv[1]) return L < J->mv[1];
    if (q != J->mv[2]) return q < J->mv[2];
    return rev < J->mv[3];
}

static void fill(const job *J, double *w, int node)
{
    for (int q = 0; q < J->n; q++) w[q] = q == node ? -1.0 : weight(J->xy, J->kind, q, node);
}

static void *run(void *arg)
{
    job *J = (job *)arg;
    const int n = J->n;
    double *buf = (double *)malloc((size_t)3 * n * sizeof(double));
    double *w[3] = {buf, buf + n, buf + 2 * n};
    J->best = DBL_MAX; J->mv[0] = J->mv[1] = J->mv[2] = J->mv[3] = -1;
    if (J->k0 >= J->k1 || !buf) { free(buf); return NULL; }
    fill(J, w[0], J->ord[J->k0 % n]);
    fill(J, w[1], J->ord[(J->k0 + 1) % n]);
    for (int k = J->k0; k < J->k1; k++) {
        fill(J, w[2], J->ord[(k + 2) % n]);
        const int p = J->ord[(k - 1 + n) % n];
        int seg[3];
        for (int j = 0; j < 3; j++) seg[j] = J->ord[(k + j) % n];
        const int s = seg[0];
        for (int L = 1; L <= 3; L++) {
            const int t = seg[L - 1], x = J->path[t];
            const double cpx = weight(J->xy, J->kind, p, x), rem0 = J->cnext[p] + J->cnext[t];
            const double *ws = w[0], *wt = w[L - 1];
            for (int q = 0; q < n; q++) {
                if (q == p || q == seg[0] || (L > 1 && q == seg[1]) || (L > 2 && q == seg[2])) continue;
                const int qn = J->path[q];
                const double removed = rem0 + J->cnext[q];
                for (int rev = 0; rev < (L > 1 ? 2 : 1); rev++) {
                    const double *wh = rev ? wt : ws, *we = rev ? ws : wt;
                    const double d = ((cpx + wh[q]) + we[qn]) - removed;
                    if (d <= J->best && better(d, s, L, q, rev, J)) { J->best = d; J->mv[0] = s; J->mv[1] = L; J->mv[2] = q; J->mv[3] = rev; }
                }
            }
        }
        double *w0 = w[0];
        w[0] = w[1]; w[1] = w[2]; w[2] = w0;
    }
    free(buf);
    return NULL;
}

/* -> 0; *delta and mv[4] = {s, L, q, rev} of the sweep's best candidate (path: a successor array that is one tour) */
int orx_best_move(const double *xy, int n, int kind, const int *path, int threads, double *delta, int *mv)
{
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    if (threads > n) threads = n;
    int *ord = (int *)malloc((size_t)n * sizeof(int));
    double *cnext = (double *)malloc((size_t)n * sizeof(double));
    if (!ord || !cnext) { free(ord); free(cnext); return 1; }
    for (int i = 0, v = 0; i < n; i++, v = path[v]) ord[i] = v;
    for (int v = 0; v < n; v++) cnext[v] = weight(xy, kind, v, path[v]);
    job J[64];
    pthread_t th[64];
    for (int k = 0; k < threads; k++) {
        job j = {xy, path, ord, cnext, n, kind, (int)((long)n * k / threads), (int)((long)n * (k + 1) / threads), DBL_MAX, {-1, -1, -1, -1}};
        J[k] = j;
        pthread_create(&th[k], NULL, run, &J[k]);
    }
    job B = J[0];
    for (int k = 0; k < threads; k++) {
        pthread_join(th[k], NULL);
        if (k == 0) B = J[0];
        else if (J[k].mv[0] >= 0 && (J[k].best < B.best || (J[k].best == B.best && better(J[k].best, J[k].mv[0], J[k].mv[1], J[k].mv[2], J[k].mv[3], &B)))) B = J[k];
    }
    *delta = B.best;
    for (int i = 0; i < 4; i++) mv[i] = B.mv[i];
    free(ord); free(cnext);
    return 0;
}
