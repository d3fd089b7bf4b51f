// csrc/tspgpu_lds_tmat.h on the CPU: the index arithmetic of the tour-ordered matrix copy, and the protocol that the TM
// instantiations of k_lds2opt follow around it, modelled with W workgroups of E + 1 rows each.  Stand-alone (built with
// AddressSanitizer and UBSan by tests/test_lds_tmat_model.py).
//   lds_tmat                the arithmetic checks, then the protocol in three workgroup orders: prints "lds_tmat ok"
//   lds_tmat --no-copy-rule the protocol with the copy row (row E) fetched from tmat like the others: the checks must
//                           catch it -- exit status 3 and a line that begins "violation:"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tspgpu_lds_tmat.h"

typedef unsigned short u16;
static const u16 POISON = 16383;

#define CHECK(c, ...) do { if (!(c)) { std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned)(rng_state >> 11); }

// ---- arithmetic -------------------------------------------------------------------------------------------------------
static void reversed(const std::vector<u16> &old, int lo, int M, std::vector<u16> &out)
{
    const int n = (int)old.size();
    out = old;
    for (int u = 0; u < M; u++) out[(lo + u) & (n - 1)] = old[(lo + M - 1 - u) & (n - 1)];
}

// the row behind the move assembled from the row before it, chunk by chunk, as the kernel does; returns the number of
// chunks that did not go whole
static int assemble(const std::vector<u16> &old, int lo, int M, std::vector<u16> &out)
{
    const int n = (int)old.size();
    out.assign(n, 0xffff);
    int cw[3], slow = 0;
    lds_tmat::cellwise_chunks(lo, M, n, cw);
    for (int q0 = 0; q0 < n; q0 += 8) {
        int start = -1;
        const int cls = lds_tmat::chunk_class(q0, lo, M, n, start);
        if (cls == lds_tmat::CELLWISE) {
            slow++;
            CHECK(q0 >> 3 == cw[0] || q0 >> 3 == cw[1] || q0 >> 3 == cw[2], "n %d lo %d M %d chunk %d is not listed", n, lo, M, q0 >> 3);
            continue;
        }
        CHECK(start >= 0 && start + 8 <= n, "n %d lo %d M %d chunk %d starts at %d", n, lo, M, q0 >> 3, start);
        CHECK(cls != lds_tmat::SAME || start == q0, "n %d lo %d M %d chunk %d", n, lo, M, q0 >> 3);
        for (int j = 0; j < 8; j++) out[q0 + j] = cls == lds_tmat::MIRROR ? old[start + 7 - j] : old[start + j];
    }
    for (int i = 0; i < 24; i++) {                       // the listed chunks cell by cell, whatever their class
        CHECK(cw[i >> 3] >= 0 && cw[i >> 3] < n / 8, "n %d lo %d M %d", n, lo, M);
        const int q = cw[i >> 3] * 8 + (i & 7), s = lds_tmat::src_cell(q, lo, M, n);
        CHECK(s >= 0 && s < n, "n %d lo %d M %d cell %d source %d", n, lo, M, q, s);
        CHECK(out[q] == 0xffff || out[q] == old[s], "n %d lo %d M %d cell %d: whole and cell by cell differ", n, lo, M, q);
        out[q] = old[s];
    }
    return slow;
}

static void check_move(const std::vector<u16> &old, int lo, int M)
{
    const int n = (int)old.size();
    std::vector<u16> want, got;
    reversed(old, lo, M, want);
    const int slow = assemble(old, lo, M, got);
    CHECK(slow <= 3, "n %d lo %d M %d: %d chunks go cell by cell", n, lo, M, slow);
    CHECK(got == want, "n %d lo %d M %d: the assembled row is not the reversed row", n, lo, M);
    for (int q = 0; q < n; q++) {
        CHECK(lds_tmat::in_range(q, lo, M, n) == (((q - lo + n) % n) < M), "n %d lo %d M %d q %d", n, lo, M, q);
        CHECK(want[q] == old[lds_tmat::src_cell(q, lo, M, n)], "n %d lo %d M %d q %d", n, lo, M, q);
    }
    // write-back: the chunks lie inside the row, none twice, and every cell that changed is in one of them
    const int c0 = lds_tmat::wb_first(lo), cnt = lds_tmat::wb_count(lo, M), C = n / 8;
    CHECK(c0 >= 0 && c0 < C && cnt >= 1 && cnt <= C, "n %d lo %d M %d: write-back chunks %d + %d", n, lo, M, c0, cnt);
    std::vector<char> covered(n, 0);
    for (int j = 0; j < cnt; j++) {
        const int c = (c0 + j) & (C - 1);
        CHECK(!covered[8 * c], "n %d lo %d M %d: chunk %d written twice", n, lo, M, c);
        for (int v = 0; v < 8; v++) covered[8 * c + v] = 1;
    }
    for (int q = 0; q < n; q++) CHECK(covered[q] || !lds_tmat::in_range(q, lo, M, n), "n %d lo %d M %d: cell %d is not written back", n, lo, M, q);
}

static void arithmetic()
{
    for (int n : {16, 64}) {
        std::vector<u16> old(n);
        for (int q = 0; q < n; q++) old[q] = (u16)(1000 + q);      // (distinct values: a wrong source cell shows)
        for (int lo = 0; lo < n; lo++)
            for (int M = 2; M <= n / 2; M++) check_move(old, lo, M);
    }
    {
        const int n = 1024;
        std::vector<u16> old(n);
        for (int q = 0; q < n; q++) old[q] = (u16)(1000 + q);
        bool lo8[8] = {}, m8[8] = {}, wraps = false;
        // lo: every residue mod 8 near the array's start, middle and end; M: every residue, short, medium and up to n/2
        for (int lo = 0; lo < n; lo += (lo < 24 || lo >= n - 24 || (lo >= 500 && lo < 524)) ? 1 : 37)
            for (int M = 2; M <= n / 2; M += (M < 40 || M > n / 2 - 20) ? 1 : 29) {
                check_move(old, lo, M);
                lo8[lo & 7] = true; m8[M & 7] = true; wraps = wraps || lo + M > n;
            }
        for (int i = 0; i < 8; i++) CHECK(lo8[i] && m8[i], "the sample misses a residue");
        CHECK(wraps, "the sample has no range across the array end");
    }
}

// ---- protocol ---------------------------------------------------------------------------------------------------------
struct Model {
    int W, E, n;
    bool copy_rule;
    std::vector<u16> c;                      // [n][n] the matrix, node order
    std::vector<int> ord;                    // node at every array cell
    std::vector<u16> tmat;                   // [n][n]
    std::vector<std::vector<u16>> lds;       // [W * (E + 1)] rows of n cells
    std::vector<int> readers, reader_wg, writers, writer_wg;
    u16 truth(int x, int q) const { return ord[q] == x ? POISON : c[(size_t)x * n + ord[q]]; }
    std::vector<u16> &row(int g, int r) { return lds[(size_t)g * (E + 1) + r]; }
};

static int violation(const char *what, int a, int b, int c)
{
    std::printf("violation: %s (%d, %d, %d)\n", what, a, b, c);
    return 3;
}

// one move, the workgroups taking their turn at fetch + write-back in the order `order`; 0, or the violation's exit status
static int move(Model &m, int lo, int M, const std::vector<int> &order)
{
    const int n = m.n, E = m.E, mask = n - 1;
    // labels: every workgroup's own copy, all alike
    std::vector<int> nord = m.ord;
    for (int u = 0; u < M; u++) nord[(lo + u) & mask] = m.ord[(lo + M - 1 - u) & mask];
    m.ord = nord;
    // in-LDS part: rows that stay are reversed in place, rows whose node stays among the own cells change places
    std::vector<unsigned> need(m.W, 0);
    for (int g = 0; g < m.W; g++) {
        const int k0 = g * E;
        std::vector<int> mir(E + 1, -1);
        for (int r = 0; r <= E; r++) {
            const int p = (k0 + r) & mask;
            if (lds_tmat::in_range(p, lo, M, n)) {
                const int pm = lds_tmat::src_cell(p, lo, M, n), rm = (pm - k0) & mask;
                if (rm > E) need[g] |= 1u << r; else mir[r] = rm;
            }
        }
        for (int r = 0; r <= E; r++)
            if (!((need[g] >> r) & 1)) { std::vector<u16> t; reversed(m.row(g, r), lo, M, t); m.row(g, r) = t; }
        for (int r = 0; r <= E; r++)
            if (mir[r] > r) { CHECK(!((need[g] >> mir[r]) & 1), "a row changes places with a row that is fetched"); std::swap(m.row(g, r), m.row(g, mir[r])); }
    }
    std::fill(m.readers.begin(), m.readers.end(), 0);
    std::fill(m.writers.begin(), m.writers.end(), 0);
    for (int g : order) {
        const int k0 = g * E;
        // fetch
        for (int r = 0; r <= E; r++) {
            if (!((need[g] >> r) & 1)) continue;
            const int x = m.ord[(k0 + r) & mask];
            if (r == E && m.copy_rule) {                 // the copy row: from the matrix, gathered by the labels
                for (int q = 0; q < n; q++) m.row(g, r)[q] = m.ord[q] == x ? POISON : m.c[(size_t)x * n + m.ord[q]];
                continue;
            }
            m.readers[x]++; m.reader_wg[x] = g;
            const std::vector<u16> old(m.tmat.begin() + (size_t)x * n, m.tmat.begin() + (size_t)(x + 1) * n);
            assemble(old, lo, M, m.row(g, r));
        }
        // write-back: rows 0 .. E-1, the chunks over the range
        const int c0 = lds_tmat::wb_first(lo), cnt = lds_tmat::wb_count(lo, M), C = n / 8;
        for (int r = 0; r < E; r++) {
            const int x = m.ord[k0 + r];
            m.writers[x]++; m.writer_wg[x] = g;
            for (int j = 0; j < cnt; j++) {
                const int cc = (c0 + j) & (C - 1);
                std::memcpy(&m.tmat[(size_t)x * n + 8 * cc], &m.row(g, r)[8 * cc], 16);
            }
        }
    }
    // who touched which row of tmat
    for (int x = 0; x < n; x++) {
        if (m.writers[x] != 1) return violation("a row of tmat without exactly one writer in a sweep", x, m.writers[x], 0);
        if (m.readers[x] > 1) return violation("a row of tmat read by two workgroups in a sweep", x, m.readers[x], 0);
        if (m.readers[x] == 1 && m.reader_wg[x] != m.writer_wg[x]) return violation("a row of tmat read by one workgroup and written by another in a sweep", x, m.reader_wg[x], m.writer_wg[x]);
    }
    for (int x = 0; x < n; x++)
        for (int q = 0; q < n; q++)
            if (m.tmat[(size_t)x * n + q] != m.truth(x, q)) return violation("tmat differs from the truth", x, q, m.tmat[(size_t)x * n + q]);
    for (int g = 0; g < m.W; g++)
        for (int r = 0; r <= E; r++) {
            const int x = m.ord[(g * E + r) & mask];
            for (int q = 0; q < n; q++)
                if (m.row(g, r)[q] != m.truth(x, q)) return violation("an LDS row differs from the truth", g, r, q);
        }
    return 0;
}

// order: 0 ascending, 1 descending (the neighbour g + 1 writes before g reads), 2 shuffled every move
static int protocol(int W, int E, int moves, int order_kind, bool copy_rule)
{
    Model m;
    m.W = W; m.E = E; m.n = W * E; m.copy_rule = copy_rule;
    const int n = m.n;
    m.c.assign((size_t)n * n, 0);
    for (int x = 0; x < n; x++)
        for (int y = 0; y < x; y++) m.c[(size_t)x * n + y] = m.c[(size_t)y * n + x] = (u16)(1 + rnd() % 16000);
    m.ord.resize(n);
    for (int q = 0; q < n; q++) m.ord[q] = q;
    for (int q = n - 1; q > 0; q--) std::swap(m.ord[q], m.ord[rnd() % (q + 1)]);
    m.tmat.assign((size_t)n * n, 0);
    m.lds.assign((size_t)W * (E + 1), std::vector<u16>(n));
    m.readers.assign(n, 0); m.reader_wg.assign(n, -1); m.writers.assign(n, 0); m.writer_wg.assign(n, -1);
    // first load + fill
    for (int g = 0; g < W; g++)
        for (int r = 0; r <= E; r++) {
            const int x = m.ord[(g * E + r) & (n - 1)];
            for (int q = 0; q < n; q++) m.row(g, r)[q] = m.truth(x, q);
            if (r < E) std::memcpy(&m.tmat[(size_t)x * n], m.row(g, r).data(), (size_t)n * 2);
        }
    std::vector<int> order(W);
    for (int g = 0; g < W; g++) order[g] = order_kind == 1 ? W - 1 - g : g;
    for (int it = 0; it < moves; it++) {
        if (order_kind == 2) for (int g = W - 1; g > 0; g--) std::swap(order[g], order[rnd() % (g + 1)]);
        const int lo = (int)(rnd() % n), M = 2 + (int)(rnd() % (n / 2 - 1));
        if (const int rc = move(m, lo, M, order)) { std::printf("  at move %d: lo %d M %d, W %d E %d, order %d\n", it, lo, M, W, E, order_kind); return rc; }
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "--no-copy-rule")) {
        const int rc = protocol(16, 4, 5000, 1, false);
        if (!rc) std::printf("the protocol without the copy rule passed every check\n");
        return rc;
    }
    arithmetic();
    for (int kind = 0; kind < 3; kind++) {
        if (const int rc = protocol(16, 4, 5000, kind, true)) return rc;
        if (const int rc = protocol(8, 2, 1000, kind, true)) return rc;
        if (const int rc = protocol(4, 16, 1000, kind, true)) return rc;
    }
    std::printf("lds_tmat ok\n");
    return 0;
}
