// csrc/tspgpu_mem.h over a fake backend (malloc, a table of what is live, "fail the k-th allocation from now"):
// every owner and both all-or-none routines, with a failure injected at every allocation of each operation in turn.
// Built with -fsanitize=address,undefined and run by tests/test_mem_owner.py; exit status 0 = every check held and
// nothing is left allocated (LeakSanitizer looks at the malloc'ed blocks behind the backend).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "tspgpu_mem.h"

#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed (k = %d)\n", __FILE__, __LINE__, #cond, g_k); exit(2); } \
    } while (0)

static int g_k = 0;     // the failure being injected (for the message)

struct Fake {
    typedef int error;
    static constexpr error ok = 0;
    static std::map<void *, bool> live;     // block -> pinned
    static long fail_alloc_in, fail_op_in;  // k > 0: the k-th allocation / fill-or-copy from now fails
    static long allocs, ops, syncs;

    static error get(void **p, size_t bytes, bool pinned)
    {
        allocs++;
        if (fail_alloc_in > 0 && --fail_alloc_in == 0) return 2;
        *p = malloc(bytes ? bytes : 1);
        memset(*p, 0xa5, bytes);            // never what a fill leaves
        live[*p] = pinned;
        return ok;
    }
    static void put(void *p, bool pinned)
    {
        auto it = live.find(p);
        CHECK(it != live.end() && it->second == pinned);    // freed once, and as what it was allocated
        live.erase(it);
        ::free(p);
    }
    static error alloc(void **p, size_t bytes) { return get(p, bytes, false); }
    static void free(void *p) { put(p, false); }
    static error alloc_pinned(void **p, size_t bytes) { return get(p, bytes, true); }
    static void free_pinned(void *p) { put(p, true); }
    static bool op_fails() { ops++; return fail_op_in > 0 && --fail_op_in == 0; }
    error fill(void *p, int byte, size_t bytes) { if (op_fails()) return 3; memset(p, byte, bytes); return ok; }
    error copy(void *dst, const void *src, size_t bytes) { if (op_fails()) return 3; memcpy(dst, src, bytes); return ok; }
    error sync() { syncs++; return ok; }
};
std::map<void *, bool> Fake::live;
long Fake::fail_alloc_in = 0, Fake::fail_op_in = 0, Fake::allocs = 0, Fake::ops = 0, Fake::syncs = 0;

template <class T> using Dev = tspmem::DevBuf<Fake, T>;
template <class T> using Pin = tspmem::PinBuf<Fake, T>;
using tspmem::Row;
using tspmem::Rows;

// ---- a buffer: alloc, reserve, move-assignment.  Three allocations; k = 0 injects nothing -------------------------------
static long buffers(int k)
{
    const long before = Fake::allocs;
    Fake::fail_alloc_in = k;
    {
        Dev<int> a;
        Pin<double> b;
        CHECK(!a && a.n == 0);
        int e = a.alloc(4);                                 // allocation 1
        CHECK((e != Fake::ok) == (k == 1));
        if (e) CHECK(!a.p && a.n == 0 && Fake::live.empty());
        else { CHECK(a.p && a.n == 4 && Fake::live.size() == 1); a[3] = 7; }
        int *const held = a.p;
        if (held) CHECK(a.reserve(2) == Fake::ok && a.p == held);   // grow-only: nothing happens
        e = a.reserve(9);                                   // allocation 2: the old block goes first
        CHECK((e != Fake::ok) == (k == 2));
        if (e) CHECK(!a.p && a.n == 0 && Fake::live.empty());
        else { CHECK(a.n == 9 && Fake::live.size() == 1); a[8] = 1; }
        e = b.alloc(3);                                     // allocation 3, pinned
        CHECK((e != Fake::ok) == (k == 3));
        if (e) CHECK(!b.p && b.n == 0);
        else { CHECK(b.n == 3 && Fake::live.at(b.p)); b[2] = 0.5; }
        const size_t both = Fake::live.size();
        Pin<double> c;
        CHECK(c.alloc(1) == Fake::ok);
        double *const bp = b.p; const size_t bn = b.n;
        c = std::move(b);                                   // c's block is freed, b is left empty
        CHECK(c.p == bp && c.n == bn && !b.p && b.n == 0 && Fake::live.size() == both);
        Pin<double> d(std::move(c));
        CHECK(d.p == bp && !c.p && Fake::live.size() == both);
        a.reset();
        CHECK(!a.p && a.n == 0);
    }
    CHECK(Fake::live.empty());
    Fake::fail_alloc_in = 0;
    return Fake::allocs - before - 1;       // (c's own allocation is not part of the ladder)
}

// ---- alloc_all over three buffers of different element sizes, one of them holding something ----------------------------
static long all_or_none(int k)
{
    Dev<char> a; Dev<int> b; Pin<double> c;
    CHECK(b.alloc(2) == Fake::ok);
    const long before = Fake::allocs;
    Fake::fail_alloc_in = k;
    const int e = tspmem::alloc_all<Fake>({{&a, 5}, {&b, 7}, {&c, 3}});
    Fake::fail_alloc_in = 0;
    CHECK((e != Fake::ok) == (k >= 1 && k <= 3));
    if (e) CHECK(!a.p && !b.p && !c.p && a.n + b.n + c.n == 0 && Fake::live.empty());
    else {
        CHECK(a.n == 5 && b.n == 7 && c.n == 3 && Fake::live.size() == 3 && !Fake::live.at(a.p) && Fake::live.at(c.p));
        a[4] = 1; b[6] = 1; c[2] = 1;       // (the sanitizer checks the sizes)
    }
    return Fake::allocs - before;
}

// ---- grow: a view of four arrays from 2 to 5 units of 3 elements ---------------------------------------------------------
struct View { int *kept; double *kept_slack; unsigned *capped; unsigned char *scratch; };
static const size_t SLACK = 16;

static Rows view_rows(View &v)
{
    return {{&v.kept, 3 * sizeof(int), 0, 0, true},
            {&v.kept_slack, 3 * sizeof(double), SLACK, 0, true},
            {&v.capped, 3 * sizeof(unsigned), 0, 0xff, false},
            {&v.scratch, 3, 0, Row::NO_FILL, false, true}};        // pinned, not filled
}

// fail_alloc / fail_op: which allocation / which fill or copy of the growth fails (0: none)
static void grown(int fail_alloc, int fail_op, long *allocs, long *ops)
{
    Fake mem;
    View v{};
    size_t units = 0;
    CHECK(tspmem::grow(mem, view_rows(v), units, 2) == Fake::ok);
    units = 2;
    CHECK(Fake::live.size() == 4);
    for (int i = 0; i < 6; i++) { v.kept[i] = 100 + i; v.kept_slack[i] = 0.25 * i; v.capped[i] = 7u; v.scratch[i] = (unsigned char)(9 + i); }
    const View old = v;
    std::vector<std::vector<unsigned char>> bytes;
    const Rows rows = view_rows(v);
    for (const Row &r : rows) bytes.emplace_back((unsigned char *)*r.slot, (unsigned char *)*r.slot + r.bytes(2));

    const long a0 = Fake::allocs, o0 = Fake::ops, s0 = Fake::syncs;
    Fake::fail_alloc_in = fail_alloc; Fake::fail_op_in = fail_op;
    const int e = tspmem::grow(mem, rows, units, 5);
    if (e == Fake::ok) units = 5;
    *allocs = Fake::allocs - a0;
    *ops = Fake::ops - o0;
    Fake::fail_alloc_in = Fake::fail_op_in = 0;
    const bool injected = (fail_alloc >= 1 && fail_alloc <= 4) || (fail_op >= 1 && fail_op <= 5);
    CHECK((e != Fake::ok) == injected);
    if (e) {    // as before the call: the slots, the unit count, every byte, what is live
        CHECK(units == 2 && memcmp(&v, &old, sizeof v) == 0 && Fake::live.size() == 4);
        for (size_t k = 0; k < rows.size(); k++) CHECK(memcmp(*rows[k].slot, bytes[k].data(), bytes[k].size()) == 0);
    } else {
        CHECK(units == 5 && Fake::live.size() == rows.size() && Fake::syncs == s0 + 1);
        CHECK(v.kept != old.kept && v.kept_slack != old.kept_slack && v.capped != old.capped && v.scratch != old.scratch);
        CHECK(!Fake::live.at(v.kept) && Fake::live.at(v.scratch));
        CHECK(memcmp(v.kept, bytes[0].data(), 2 * 3 * sizeof(int)) == 0);                 // kept rows begin with the old bytes
        CHECK(memcmp(v.kept_slack, bytes[1].data(), 2 * 3 * sizeof(double)) == 0);
        for (int i = 6; i < 15; i++) CHECK(v.kept[i] == 0);                               // ... and go on with the fill,
        const unsigned char *ks = (const unsigned char *)v.kept_slack;
        for (size_t i = 2 * 3 * sizeof(double); i < 5 * 3 * sizeof(double) + SLACK; i++) CHECK(ks[i] == 0);      // slack included
        for (int i = 0; i < 15; i++) CHECK(v.capped[i] == 0xffffffffu);                   // not kept: the fill from the start
        for (int i = 0; i < 15; i++) CHECK(v.scratch[i] == 0xa5);                         // neither kept nor filled
    }
    tspmem::free_rows<Fake>(rows);
    CHECK(!v.kept && !v.kept_slack && !v.capped && !v.scratch && Fake::live.empty());
}

// ---- a row of no unit bytes is allocated with the first growth and kept by the later ones --------------------------------
static void once_row(int k)
{
    Fake mem;
    struct { int *per_unit; int *once; } v{};
    const Rows rows = {{&v.per_unit, 4, 0, 0, true}, {&v.once, 0, 40}};
    Fake::fail_alloc_in = k;
    int e = tspmem::grow(mem, rows, 0, 2);
    Fake::fail_alloc_in = 0;
    CHECK((e != Fake::ok) == (k == 1 || k == 2));
    if (e) { CHECK(!v.per_unit && !v.once && Fake::live.empty()); return; }
    v.once[9] = 42; v.per_unit[1] = 5;
    int *const once = v.once;
    Fake::fail_alloc_in = k == 3 ? 1 : 0;
    e = tspmem::grow(mem, rows, 2, 4);
    Fake::fail_alloc_in = 0;
    CHECK((e != Fake::ok) == (k == 3));
    CHECK(v.once == once && v.once[9] == 42 && v.per_unit[1] == 5 && Fake::live.size() == 2);
    if (!e) CHECK(v.per_unit[3] == 0);
    CHECK(tspmem::rows_bytes(rows, 4) == 4 * 4 + 40);
    tspmem::free_rows<Fake>(rows);
    CHECK(Fake::live.empty());
}

int main()
{
    const long nb = buffers(0);
    CHECK(nb == 3);
    for (g_k = 1; g_k <= nb; g_k++) buffers(g_k);

    g_k = 0;
    const long na = all_or_none(0);
    CHECK(na == 3 && Fake::live.empty());
    for (g_k = 1; g_k <= na; g_k++) { all_or_none(g_k); CHECK(Fake::live.empty()); }

    g_k = 0;
    long allocs = 0, ops = 0;
    grown(0, 0, &allocs, &ops);
    CHECK(allocs == 4 && ops == 5);         // three fills and two copies
    for (g_k = 1; g_k <= 4; g_k++) grown(g_k, 0, &allocs, &ops);
    for (g_k = 1; g_k <= 5; g_k++) grown(0, g_k, &allocs, &ops);

    for (g_k = 0; g_k <= 3; g_k++) once_row(g_k);

    CHECK(Fake::live.empty());
    puts("mem_owner ok");
    return 0;
}
