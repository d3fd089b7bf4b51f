/* Plain C restatement of the Or-opt sweep defined in include/tspgpu.h ("Or-opt"), for the sizes where the numpy model
 * of tests/test_or_opt.py is too slow.  Compiled by the test (gcc -O2 -ffp-contract=off) and checked there against
 * the numpy model.  The scan order IS the definition: s ascending, L = 1, 2, 3, q ascending, rev = 0 before 1, and
 * the first strictly smaller delta wins. */
#include <float.h>
#include <stdlib.h>

int orm_best_move(const double *c, int n, const int *path, double *delta, int *mv)
{
    int *prev = (int *)malloc((size_t)n * sizeof(int));
    if (!prev) return 1;
    for (int i = 0; i < n; i++) prev[path[i]] = i;
    double best = DBL_MAX;
    mv[0] = mv[1] = mv[2] = mv[3] = -1;
#define C(i, j) c[(size_t)(i) * n + (j)]
    for (int s = 0; s < n; s++) {
        const int p = prev[s];
        int seg[3];
        seg[0] = s; seg[1] = path[s]; seg[2] = path[seg[1]];
        for (int L = 1; L <= 3; L++) {
            const int t = seg[L - 1], x = path[t];
            const double cpx = C(p, x), rem0 = C(p, s) + C(t, x);
            for (int q = 0; q < n; q++) {
                if (q == p || q == seg[0] || (L > 1 && q == seg[1]) || (L > 2 && q == seg[2])) continue;
                const int qn = path[q];
                const double removed = rem0 + C(q, qn);
                for (int rev = 0; rev < (L > 1 ? 2 : 1); rev++) {
                    const int h = rev ? t : s, e = rev ? s : t;
                    const double added = (cpx + C(q, h)) + C(e, qn);
                    const double d = added - removed;
                    if (d < best) { best = d; mv[0] = s; mv[1] = L; mv[2] = q; mv[3] = rev; }
                }
            }
        }
    }
#undef C
    free(prev);
    *delta = best;
    return 0;
}
