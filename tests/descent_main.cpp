// csrc/tspgpu_descent.h -- the descent over the neighbour lists on one tour -- against the three loops it replaced, over a
// scripted phase function.  The models below are those loops as they stood (ornl_descent, nl3_descent with its nested call,
// dl_descent), with the phase runner and the context's counters replaced by the script's.  Compared field by field: the code,
// every counter, the peaks of max_k, late, the looked totals and the ordered list of phases asked for.  Built with
// -fsanitize=address,undefined and run by tests/test_descent.py; exit status 0 = every check held.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "tspgpu_descent.h"

static std::string g_case;
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed (%s)\n", __FILE__, __LINE__, #cond, g_case.c_str()); exit(2); } \
    } while (0)

static const int E_OK = 0, E_INTERNAL = 13;

struct M2Counters { long sweeps = 0, moves = 0, max_k = 0; };
struct DlCount {
    long looked = 0, full = 0, max_q = 0;
    void operator+=(const DlCount &d) { looked += d.looked; full += d.full; max_q = std::max(max_q, d.max_q); }
};

// The script.  The p-th phase asked for (from 0) is a 2-opt phase or a control phase (Or-opt, 3-opt: its moves decide what
// follows).  The c-th control phase applies something iff bit c of `mask`; a 2-opt phase applies (5 p) mod 3 moves.  Phase
// `late_at` ends late, phase `fail_at` answers `E_INTERNAL` with its counters untouched (-1: none).  Phases past the 64th fail
// the test: every descent here ends long before
struct Script {
    unsigned mask = 0;
    int late_at = -1, fail_at = -1;
    // the state of one run
    int asked = 0, control = 0;
    std::string order;                              // '2', 'o', '3' per phase
    M2Counters count[3];                            // what m2_record leaves in the context, per family
    long ornl_rounds = -7, nl3_phases = -7;         // (-7: never written)
    bool nl3_count_written = false;

    int phase(int family, long *sweeps, long *moves, DlCount *dl, bool *late)
    {
        const int p = asked++;
        CHECK(p < 64);
        order += "2o3"[family];
        *late = false;
        *sweeps = 0; *moves = 0;
        if (dl) *dl = DlCount{};
        count[family] = M2Counters{};
        if (p == fail_at) return E_INTERNAL;
        long m;
        if (family == 0) m = (5 * p) % 3;
        else m = (mask >> control++) & 1u ? 2 + p % 4 : 0;
        *moves = m;
        *sweeps = m + 1 + p % 2;
        *late = p == late_at;
        count[family] = M2Counters{*sweeps, *moves, m ? 1 + (7 * p) % 5 : 0};
        if (dl) *dl = DlCount{10 + 3 * p, p % 3, (11 * p) % 7};
        return E_OK;
    }
};

struct Got {
    int rc = 0;
    bool late = false;
    Descent D;
    long omk = 0, mk = 0;
    DlCount dl;
    std::string order;
    long ornl_rounds = 0, nl3_phases = 0;
    M2Counters ornl_count, nl3_count;
};

// ---- the models ------------------------------------------------------------------------------------------------------------

struct Descent3 { long ts = 0, tm = 0; int np = 0; };

static int model_ornl_descent(Script &x, Descent *out, bool *late)
{
    Descent D;
    long mk = 0;
    int rc = E_OK;
    *late = false;
    x.count[1] = M2Counters{};
    for (;;) {
        long s = 0, m = 0;
        if ((rc = x.phase(0, &s, &m, nullptr, late))) break;
        D.tw += s; D.tm += m; D.nr++;
        if (*late) break;
        if ((rc = x.phase(1, &s, &m, nullptr, late))) break;
        D.os += s; D.om += m; mk = std::max(mk, x.count[1].max_k);
        if (*late || m == 0) break;
    }
    x.count[1] = M2Counters{D.os, D.om, mk}; x.ornl_rounds = D.nr;
    *out = D;
    return rc;
}

static int model_nl3_descent(Script &x, Descent *out, Descent3 *out3, bool *late)
{
    Descent D;
    Descent3 D3;
    long mk = 0, omk = 0;
    int rc = E_OK;
    *late = false;
    x.count[2] = M2Counters{};
    for (;;) {
        Descent d;
        rc = model_ornl_descent(x, &d, late);
        D += d; omk = std::max(omk, x.count[1].max_k);
        if (rc || *late) break;
        long s = 0, m = 0;
        if ((rc = x.phase(2, &s, &m, nullptr, late))) break;
        D3.ts += s; D3.tm += m; D3.np++; mk = std::max(mk, x.count[2].max_k);
        if (*late || m == 0) break;
    }
    x.count[1] = M2Counters{D.os, D.om, omk}; x.ornl_rounds = D.nr;
    x.count[2] = M2Counters{D3.ts, D3.tm, mk}; x.nl3_phases = D3.np; x.nl3_count_written = true;
    *out = D; *out3 = D3;
    return rc;
}

static int model_dl_descent(Script &x, int width, Descent *out, Descent3 *out3, DlCount *dl, bool *late)
{
    Descent D;
    Descent3 D3;
    DlCount total, d;
    long mk = 0, omk = 0;
    int rc = E_OK;
    *late = false;
    x.count[1] = M2Counters{};
    x.count[2] = M2Counters{};
    for (bool more = true; more && !rc && !*late;) {
        for (;;) {
            long s = 0, m = 0;
            if ((rc = x.phase(0, &s, &m, &d, late))) break;
            D.tw += s; D.tm += m; D.nr++; total += d;
            if (*late) break;
            if ((rc = x.phase(1, &s, &m, &d, late))) break;
            D.os += s; D.om += m; total += d; omk = std::max(omk, x.count[1].max_k);
            if (*late || m == 0) break;
        }
        if (rc || *late || width == 0) break;
        long s = 0, m = 0;
        if ((rc = x.phase(2, &s, &m, &d, late))) break;
        D3.ts += s; D3.tm += m; D3.np++; total += d; mk = std::max(mk, x.count[2].max_k);
        more = m != 0;
    }
    x.count[1] = M2Counters{D.os, D.om, omk}; x.ornl_rounds = D.nr;
    if (width) { x.count[2] = M2Counters{D3.ts, D3.tm, mk}; x.nl3_phases = D3.np; x.nl3_count_written = true; }
    *out = D; *out3 = D3; *dl = total;
    return rc;
}

static Got run_model(Script x, int width, bool looks)
{
    Got g;
    Descent3 D3;
    if (looks) g.rc = model_dl_descent(x, width, &g.D, &D3, &g.dl, &g.late);
    else if (width) g.rc = model_nl3_descent(x, &g.D, &D3, &g.late);
    else g.rc = model_ornl_descent(x, &g.D, &g.late);
    g.D.hs = D3.ts; g.D.hm = D3.tm; g.D.np = D3.np;
    g.order = x.order;
    g.ornl_count = x.count[1]; g.ornl_rounds = x.ornl_rounds;
    g.omk = x.count[1].max_k;
    if (x.nl3_count_written) { g.nl3_count = x.count[2]; g.nl3_phases = x.nl3_phases; g.mk = x.count[2].max_k; }
    return g;
}

// ---- the alternation, used as the library's nl_descent uses it ---------------------------------------------------------------

static Got run_new(Script x, int width, bool looks)
{
    Got g;
    descent::Peaks P;
    g.rc = descent::alternate(
        width,
        [&](descent::Family f, long *sweeps, long *moves, bool *late) {
            DlCount dl;
            const int e = x.phase((int)f, sweeps, moves, looks ? &dl : nullptr, late);
            if (!e) g.dl += dl;
            return e;
        },
        [&](descent::Family f) { return x.count[f].max_k; }, &g.D, &P, &g.late);
    g.order = x.order;
    g.omk = P.k[descent::OR_OPT]; g.mk = P.k[descent::THREE_OPT];
    g.ornl_count = M2Counters{g.D.os, g.D.om, g.omk}; g.ornl_rounds = g.D.nr;
    if (width) { g.nl3_count = M2Counters{g.D.hs, g.D.hm, g.mk}; g.nl3_phases = g.D.np; }
    return g;
}

static bool same(const M2Counters &a, const M2Counters &b) { return a.sweeps == b.sweeps && a.moves == b.moves && a.max_k == b.max_k; }

static long g_runs = 0, g_phases = 0;

static void compare(const Script &x, int width, bool looks)
{
    const Got a = run_model(x, width, looks), b = run_new(x, width, looks);
    g_case = "mask " + std::to_string(x.mask) + " width " + std::to_string(width) + (looks ? " looks" : " plain") + " late_at " +
             std::to_string(x.late_at) + " fail_at " + std::to_string(x.fail_at) + ": model " + a.order + ", new " + b.order;
    CHECK(a.order == b.order);
    CHECK(a.rc == b.rc && a.late == b.late);
    CHECK(a.D.tw == b.D.tw && a.D.tm == b.D.tm && a.D.os == b.D.os && a.D.om == b.D.om && a.D.nr == b.D.nr);
    CHECK(a.D.hs == b.D.hs && a.D.hm == b.D.hm && a.D.np == b.D.np);
    CHECK(a.omk == b.omk && a.mk == b.mk);
    CHECK(a.dl.looked == b.dl.looked && a.dl.full == b.dl.full && a.dl.max_q == b.dl.max_q);
    CHECK(same(a.ornl_count, b.ornl_count) && a.ornl_rounds == b.ornl_rounds);
    CHECK(same(a.nl3_count, b.nl3_count) && a.nl3_phases == b.nl3_phases);
    if (width == 0) CHECK(a.order.find('3') == std::string::npos);
    g_runs++; g_phases += (long)a.order.size();
}

int main()
{
    // Twelve control phases: three outer rounds of three Or-opt phases and a 3-opt phase each.  Every pattern of them, and
    // behind each the lateness and the failure of every phase the undisturbed descent asks for (and of the one behind its last)
    long longest = 0;
    for (unsigned mask = 0; mask < (1u << 12); mask++)
        for (int width : {0, 5})
            for (bool looks : {false, true}) {
                Script x;
                x.mask = mask;
                compare(x, width, looks);
                const int phases = (int)run_model(x, width, looks).order.size();
                longest = std::max(longest, (long)phases);
                for (int k = 0; k <= phases; k++) {
                    Script l = x, f = x;
                    l.late_at = k;
                    f.fail_at = k;
                    compare(l, width, looks);
                    compare(f, width, looks);
                }
            }
    // what the enumeration must have reached: the full three-by-three pattern (2o2o2o3 three times) is 21 phases
    CHECK(longest >= 21);
    {
        Script x;
        x.mask = 0x3bb;                             // 0b0011'1011'1011, lowest bit first: + + 0 +, + + 0 +, + + 0 0
        CHECK(run_model(x, 5, false).order == "2o2o2o32o2o2o32o2o2o3");
        CHECK(run_new(x, 5, true).order == "2o2o2o32o2o2o32o2o2o3");
        // nr counts a 2-opt phase that ends late; a phase that fails counts nothing
        Script l = x, f = x;
        l.late_at = 2; f.fail_at = 2;
        CHECK(run_new(l, 5, false).D.nr == 2 && run_new(l, 5, false).late && run_new(l, 5, false).order == "2o2");
        CHECK(run_new(f, 5, false).D.nr == 1 && run_new(f, 5, false).rc == E_INTERNAL);
    }
    CHECK(g_runs > 100000 && g_phases > g_runs);
    printf("descent ok\n");
    return 0;
}
