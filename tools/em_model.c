/*
 * tools/em_model.c -- a CPU restatement of Extra Mileage (h_ExtraMileage EM_MAX, src/algorithms/heuristics.c:156-210,
 * and h_extramileage_util, :290-367) in the INCREMENTAL form the device runs: every unvisited node keeps its best
 * (delta, edge) over the current edges; after x is inserted into edge e only the nodes whose best edge was e rescan
 * all edges, every other node compares the two changed edges.  Written from the algorithm, not from the reference's
 * code; weights straight from the coordinates (the reference's EUC_2D, TSPLIB ATT / CEIL_2D), OpenMP over nodes and
 * stale rescans.  What it is for: the goldens of instances too large for the reference's O(n^3) loop (d18512,
 * pla85900; tools/make_golden_em.py --large), after it has been checked against the reference on the small sets
 * (tests/test_extra_mileage.py).
 *
 *   gcc -O3 -fopenmp -ffp-contract=off -fno-math-errno -o em_model tools/em_model.c -lm
 *   em_model XY.bin N KIND [A B]    (XY.bin: N (x, y) doubles; KIND 0 EUC_2D, 1 ATT, 2 CEIL_2D; A B: the starting
 *                                    pair, default the farthest pair)
 *   prints: a b cost fnv1a(successor array) stale_rescans
 */
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

static int n, kind;
static double *X, *Y;

static inline long w_xy(double ax, double ay, double bx, double by)
{
    const double dx = bx - ax, dy = by - ay, sq = dx * dx + dy * dy;
    if (kind == 0) return (long)((double)sqrtf((float)sq) + 0.5);      /* src/tsp.c:629 */
    if (kind == 1) {                                                    /* TSPLIB ATT */
        const double r = sqrt(sq / 10.0), t = (double)(long long)(r + 0.5);
        return (long)(t < r ? t + 1.0 : t);
    }
    return (long)ceil(sqrt(sq));                                        /* TSPLIB CEIL_2D */
}
static inline long w(int i, int j) { return w_xy(X[i], Y[i], X[j], Y[j]); }

int main(int argc, char **argv)
{
    if (argc != 4 && argc != 6) { fprintf(stderr, "usage: em_model XY.bin N KIND [A B]\n"); return 2; }
    n = atoi(argv[2]); kind = atoi(argv[3]);
    if (n < 2 || kind < 0 || kind > 2) { fprintf(stderr, "bad N or KIND\n"); return 2; }
    X = malloc(sizeof(double) * n); Y = malloc(sizeof(double) * n);
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    for (int i = 0; i < n; i++) {
        double p[2];
        if (fread(p, sizeof p, 1, f) != 1) { fprintf(stderr, "short read\n"); return 2; }
        X[i] = p[0]; Y[i] = p[1];
    }
    fclose(f);

    int a = 0, b = 1;
    if (argc == 6) { a = atoi(argv[4]); b = atoi(argv[5]); }
    else {                                             /* first strict maximum over i < j, row-major (:165-177) */
        long best = 0; long long bl = -1;
#pragma omp parallel
        {
            long tb = 0; long long tl = -1;
#pragma omp for schedule(dynamic, 16)
            for (int i = 0; i < n; i++)
                for (int j = i + 1; j < n; j++) {
                    const long c = w(i, j);
                    const long long l = (long long)i * n + j;
                    if (c > tb || (c == tb && c > 0 && (tl < 0 || l < tl))) { tb = c; tl = l; }
                }
#pragma omp critical
            if (tb > best || (tb == best && tb > 0 && tl >= 0 && (bl < 0 || tl < bl))) { best = tb; bl = tl; }
        }
        if (best > 0) { a = (int)(bl / n); b = (int)(bl % n); }
    }

    int *eu = malloc(sizeof(int) * n), *ev = malloc(sizeof(int) * n), *succ = malloc(sizeof(int) * n);
    long *ec = malloc(sizeof(long) * n), *bd = malloc(sizeof(long) * n);
    double *eux = malloc(sizeof(double) * n), *euy = malloc(sizeof(double) * n);
    double *evx = malloc(sizeof(double) * n), *evy = malloc(sizeof(double) * n);
    int *bj = malloc(sizeof(int) * n), *stale = malloc(sizeof(int) * n);
    char *unv = malloc(n);
    int k = 0;
#define SET_EDGE(J, U, V) do { eu[J] = (U); ev[J] = (V); ec[J] = w((U), (V)); eux[J] = X[U]; euy[J] = Y[U]; evx[J] = X[V]; evy[J] = Y[V]; } while (0)
    SET_EDGE(0, a, b); SET_EDGE(1, b, a); k = 2;
    for (int i = 0; i < n; i++) { unv[i] = i != a && i != b; succ[i] = -1; }
    succ[a] = b; succ[b] = a;
    double cost = 2.0 * (double)w(a, b);
#pragma omp parallel for
    for (int i = 0; i < n; i++) {
        if (!unv[i]) continue;
        const long d0 = w(a, i) + w(i, b) - ec[0], d1 = w(b, i) + w(i, a) - ec[1];
        bd[i] = d1 < d0 ? d1 : d0; bj[i] = d1 < d0 ? 1 : 0;
    }
    long long nstale = 0;
    for (int step = 0; step < n - 2; step++) {
        /* winner: the lexicographic minimum of (bd, i) */
        long gd = LONG_MAX; int gx = n;
#pragma omp parallel
        {
            long td = LONG_MAX; int tx = n;
#pragma omp for nowait
            for (int i = 0; i < n; i++)
                if (unv[i] && (bd[i] < td || (bd[i] == td && i < tx))) { td = bd[i]; tx = i; }
#pragma omp critical
            if (td < gd || (td == gd && tx < gx)) { gd = td; gx = tx; }
        }
        const int x = gx, e = bj[x], u = eu[e], v = ev[e], m = k;
        SET_EDGE(e, u, x); SET_EDGE(m, x, v); k++;
        succ[u] = x; succ[x] = v;
        cost += (double)gd;
        unv[x] = 0;
        const long cux = ec[e], cxv = ec[m];
        int ns = 0;
#pragma omp parallel for
        for (int i = 0; i < n; i++) {
            if (!unv[i]) continue;
            if (bj[i] == e) { int q;
#pragma omp atomic capture
                q = ns++;
                stale[q] = i; continue; }
            long d = bd[i]; int j = bj[i];
            const long de = w(u, i) + w(i, x) - cux;
            if (de < d || (de == d && e < j)) { d = de; j = e; }
            const long dm = w(x, i) + w(i, v) - cxv;
            if (dm < d) { d = dm; j = m; }
            bd[i] = d; bj[i] = j;
        }
        nstale += ns;
#pragma omp parallel for schedule(dynamic, 1)
        for (int q = 0; q < ns; q++) {
            const int i = stale[q];
            const double px = X[i], py = Y[i];
            long md = LONG_MAX;
#pragma omp simd reduction(min:md)
            for (int j = 0; j < k; j++) {
                const long d = w_xy(eux[j], euy[j], px, py) + w_xy(px, py, evx[j], evy[j]) - ec[j];
                md = d < md ? d : md;
            }
            int fj = 0;
            for (int j = 0; j < k; j++)
                if (w_xy(eux[j], euy[j], px, py) + w_xy(px, py, evx[j], evy[j]) - ec[j] == md) { fj = j; break; }
            bd[i] = md; bj[i] = fj;
        }
    }
    uint64_t h = 0xcbf29ce484222325ULL;
    for (int i = 0; i < n; i++) { h ^= (unsigned)succ[i]; h *= 0x100000001b3ULL; }
    printf("%d %d %.1f %016llx %lld\n", a, b, cost, (unsigned long long)h, nstale);
    return 0;
}
