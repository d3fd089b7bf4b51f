// csrc/tspgpu_relaunch.h -- the relaunch protocol of the one-launch descents -- over a scripted launch and a clock that the
// script advances: the gate and its back-off, the sweep budgets, the retries, the hand-over, and what the family's callables
// decide.  Every expected number is worked out here, by this file's own arithmetic.  Built with -fsanitize=address,undefined
// and run by tests/test_relaunch_protocol.py; exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "tspgpu_relaunch.h"

static const char *g_case = "";
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed (%s)\n", __FILE__, __LINE__, #cond, g_case); exit(2); } \
    } while (0)

using relaunch::Gate;
using relaunch::Result;

static const int E_INTERNAL = 13, E_EXHAUSTED = 8;
static const int NEVER = 1073741824;

// what one launch answers, and how long it takes on the fake clock
struct Step { int status; int sweeps; double dt; int code; };    // status: LP_ST_* or relaunch::REFUSED; code: the family's own error
static Step st(int status, int sweeps = 0, double dt = 0, int code = 0) { return {status, sweeps, dt, code}; }

static double g_now = 0;

struct Run {
    Result r;
    std::vector<int> budgets;       // what every launch was given
    std::vector<bool> firsts;
    std::vector<bool> lost_firsts;  // what `lost` was asked
    double left;                    // the caller's time_left in/out
};

typedef std::function<int(int, int)> Completed;
typedef std::function<int(bool)> Lost;

// a plain descent, as the families': an optimum or the cap ends it
static int plain(int status, int) { return status == LP_ST_OPTIMUM || status == LP_ST_CAPPED ? relaunch::STOP : 0; }    // (0 is GO_ON)
static int hands_over(bool) { return relaunch::HAND_OVER; }

// time_left < 0: no deadline
static Run run(Gate &gate, double time_left, double sweep_s, const std::vector<Step> &script, Completed completed = plain, Lost lost = hands_over)
{
    Run out;
    out.left = time_left;
    const double t_end = time_left >= 0 ? g_now + time_left : -1;
    size_t at = 0;
    out.r = relaunch::drive(
        gate, [] { return g_now; }, t_end, sweep_s, &out.left,
        [&](int budget, bool first, int &status, int &sweeps) {
            CHECK(at < script.size());          // never a launch past the script
            const Step &s = script[at++];
            out.budgets.push_back(budget);
            out.firsts.push_back(first);
            g_now += s.dt;
            status = s.status; sweeps = s.sweeps;
            return s.code;
        },
        completed, [&](bool first) { out.lost_firsts.push_back(first); return lost(first); });
    return out;
}

// the rule, restated: a third of the time left over the time of a sweep, at least 1, at most 2^20
static int budget_of(double left, double sweep_s)
{
    double b = left / 3.0 / sweep_s;
    if (b < 1.0) b = 1.0;
    if (b > 1048576.0) b = 1048576.0;
    return (int)b;
}

static bool gate_is(const Gate &g, int skip, int backoff) { return g.skip == skip && g.backoff == backoff; }
static bool stepped_aside(const Result &r) { return r.code == 0 && !r.ran && !r.late && !r.handed; }

static void no_deadline_optimum()
{
    g_case = "no deadline, optimum";
    Gate g;
    CHECK(gate_is(g, 0, 16));
    const Run x = run(g, -1, 8e-6, {st(LP_ST_OPTIMUM, 7, 0.5)});
    CHECK(x.budgets.size() == 1 && x.budgets[0] == -1 && x.firsts[0]);
    CHECK(x.r.code == 0 && x.r.ran && !x.r.late && !x.r.handed && x.r.sweeps == 7);
    CHECK(gate_is(g, 0, 16) && x.left == -1);
    g_case = "no deadline, cap";
    const Run y = run(g, -1, 8e-6, {st(LP_ST_BUDGET, 3), st(LP_ST_CAPPED, 4)});
    CHECK(y.budgets.size() == 2 && y.budgets[1] == -1 && !y.firsts[1] && y.r.ran && y.r.sweeps == 7);
}

static void step_aside_and_back_off()
{
    g_case = "step aside and back off";
    Gate g;
    const int skips[] = {16, 32, 64, 128, 256, 512, 1024, 1024, 1024};
    for (int k = 0; k < 9; k++) {
        CHECK(!g.skip_this());                  // this descent launches
        const Run x = run(g, -1, 8e-6, {st(LP_ST_NO_RENDEZVOUS)});
        CHECK(x.budgets.size() == 1 && stepped_aside(x.r) && x.r.sweeps == 0);
        CHECK(gate_is(g, skips[k], k < 6 ? 2 * skips[k] : 1024));
        for (int d = 0; d < skips[k]; d++) { CHECK(g.skip_this()); CHECK(g.skip == skips[k] - d - 1); }   // ... these do not
    }
    CHECK(!g.skip_this() && gate_is(g, 0, 1024));
    const Run y = run(g, -1, 8e-6, {st(LP_ST_OPTIMUM, 1)});     // one launch that comes up
    CHECK(y.r.ran && gate_is(g, 0, 16));
    g.skip = 5; g.backoff = 256;
    g.rearm();                                  // what setting PERSIST, STREAM_PERSIST or option 97 does
    CHECK(gate_is(g, 0, 16));
}

static void launch_refused()
{
    g_case = "refused on the first launch";
    Gate g;
    const Run x = run(g, -1, 8e-6, {st(relaunch::REFUSED)});
    CHECK(x.budgets.size() == 1 && stepped_aside(x.r) && gate_is(g, NEVER, 16));
    CHECK(g.skip_this() && g.skip == NEVER - 1);
    g_case = "refused on a later launch";
    Gate h;
    const Run y = run(h, -1, 8e-6, {st(LP_ST_BUDGET, 5), st(relaunch::REFUSED)});
    CHECK(y.budgets.size() == 2 && y.r.code == E_INTERNAL && !y.r.ran && !y.r.handed && y.r.sweeps == 5 && gate_is(h, 0, 16));
    g_case = "the family's launch fails otherwise";
    const Run z = run(h, -1, 8e-6, {st(LP_ST_OPTIMUM, 9, 0, E_EXHAUSTED)});
    CHECK(z.r.code == E_EXHAUSTED && !z.r.ran && z.r.sweeps == 0 && gate_is(h, 0, 16));
}

static void deadline_budgets()
{
    g_case = "deadline budgets";
    Gate g;
    g_now = 100.0;
    const double t_end = g_now + 0.9, guess = 8e-6;
    double now = g_now, t0 = now;
    const int b1 = budget_of(t_end - now, guess);                   // the family's first guess
    now += 0.2;
    double sweep_s = (now - t0) / 1000;                             // 1000 sweeps in 0.2 s
    const int b2 = budget_of(t_end - now, sweep_s);
    t0 = now; now += 0.35;
    sweep_s = (now - t0) / 1166;                                    // 1166 sweeps in 0.35 s
    const int b3 = budget_of(t_end - now, sweep_s);
    now += 0.05;
    const int b4 = budget_of(t_end - now, sweep_s);                 // a launch of no sweeps measures nothing
    CHECK(b1 == 37500 && b2 == 1166 && b3 == 388 && b4 == 333);     // (the same by hand)
    const Run x = run(g, 0.9, guess, {st(LP_ST_BUDGET, 1000, 0.2), st(LP_ST_BUDGET, 1166, 0.35), st(LP_ST_BUDGET, 0, 0.05), st(LP_ST_OPTIMUM, 17, 0.01)});
    CHECK(x.budgets.size() == 4 && x.budgets[0] == b1 && x.budgets[1] == b2 && x.budgets[2] == b3 && x.budgets[3] == b4);
    CHECK(x.r.code == 0 && x.r.ran && !x.r.late && !x.r.handed && x.r.sweeps == 1000 + 1166 + 17);
    CHECK(x.left == 0.9 && gate_is(g, 0, 16));                      // (written only at a hand-over)

    g_case = "budget clamps";
    g_now = 0;
    CHECK(budget_of(1e-6, 1.0) == 1 && budget_of(1000.0, 1e-9) == 1048576);
    const Run lo = run(g, 1e-6, 1.0, {st(LP_ST_OPTIMUM, 1)});
    CHECK(lo.budgets.size() == 1 && lo.budgets[0] == 1 && lo.r.ran);
    const Run hi = run(g, 1000.0, 1e-9, {st(LP_ST_OPTIMUM, 1)});
    CHECK(hi.budgets.size() == 1 && hi.budgets[0] == 1048576 && hi.r.ran);

    g_case = "the clock passes the deadline between launches";
    const Run late = run(g, 1.0, 1e-3, {st(LP_ST_BUDGET, 10, 2.0)});
    CHECK(late.budgets.size() == 1 && late.budgets[0] == budget_of(1.0, 1e-3) && late.budgets[0] == 333);
    CHECK(late.r.code == 0 && late.r.ran && late.r.late && !late.r.handed && late.r.sweeps == 10);
    const Run just = run(g, 1.0, 1e-3, {st(LP_ST_BUDGET, 10, 1.0)});    // left == 0 is late too
    CHECK(just.budgets.size() == 1 && just.r.late && just.r.ran);
}

static void mid_descent_failure()
{
    g_case = "mid-descent failure";
    Gate g;
    g_now = 50.0;
    const Run x = run(g, 10.0, 1e-3, {st(LP_ST_BUDGET, 100, 1.0), st(LP_ST_NO_RENDEZVOUS, 0, 0.5), st(LP_ST_NO_RENDEZVOUS, 0, 0.5),
                                      st(LP_ST_NO_RENDEZVOUS, 0, 0.5), st(LP_ST_NO_RENDEZVOUS, 0, 0.5)});
    CHECK(x.budgets.size() == 5);               // three relaunches after the first failure, then the hand-over
    CHECK(x.budgets[0] == budget_of(10.0, 1e-3) && x.budgets[0] == 3333);
    for (int k = 1; k < 5; k++) CHECK(x.budgets[k] == budget_of(10.0 - 1.0 - 0.5 * (k - 1), 1.0 / 100) && !x.firsts[k]);
    CHECK(x.r.code == 0 && !x.r.ran && x.r.handed && !x.r.late && x.r.sweeps == 100);
    CHECK(gate_is(g, 16, 32) && x.left == 7.0);
    g_case = "mid-descent failure, no deadline";
    Gate h;
    const Run y = run(h, -1, 1e-3, {st(LP_ST_BUDGET, 1), st(LP_ST_NO_RENDEZVOUS), st(LP_ST_NO_RENDEZVOUS), st(LP_ST_NO_RENDEZVOUS), st(LP_ST_OPTIMUM, 2)});
    CHECK(y.budgets.size() == 5 && y.r.ran && !y.r.handed && y.r.sweeps == 3 && gate_is(h, 0, 16) && y.left == -1);   // three failures are borne
}

static void retries_are_cumulative()
{
    g_case = "retries are cumulative";
    Gate g;
    const Run x = run(g, -1, 1e-3, {st(LP_ST_BUDGET, 4), st(LP_ST_NO_RENDEZVOUS), st(LP_ST_NO_RENDEZVOUS), st(LP_ST_BUDGET, 4),
                                    st(LP_ST_NO_RENDEZVOUS), st(LP_ST_NO_RENDEZVOUS)});
    CHECK(x.budgets.size() == 6 && x.r.code == 0 && !x.r.ran && x.r.handed && x.r.sweeps == 8 && gate_is(g, 16, 32));
}

static void lost_exchange()
{
    g_case = "lost on the first launch";
    Gate g;
    const Run x = run(g, -1, 1e-3, {st(LP_ST_LOST, 3)});
    CHECK(x.budgets.size() == 1 && stepped_aside(x.r) && x.r.sweeps == 0 && gate_is(g, 16, 32));
    CHECK(x.lost_firsts.size() == 1 && x.lost_firsts[0]);
    g_case = "lost after a completed launch";
    Gate h;
    g_now = 10.0;
    const Run y = run(h, 4.0, 1e-3, {st(LP_ST_BUDGET, 6, 1.0), st(LP_ST_LOST, 3, 0.5)});
    CHECK(y.budgets.size() == 2 && y.r.code == 0 && !y.r.ran && y.r.handed && y.r.sweeps == 6 && gate_is(h, 16, 32) && y.left == 2.5);
    CHECK(y.lost_firsts.size() == 1 && !y.lost_firsts[0]);
    g_case = "lost, and the family refuses (as the tabu walk)";
    Gate t;
    const Lost walk = [](bool first) { return first ? (int)relaunch::HAND_OVER : E_INTERNAL; };
    const Run z = run(t, 4.0, 1e-3, {st(LP_ST_BUDGET, 6, 1.0), st(LP_ST_LOST, 3, 0.5)}, plain, walk);
    CHECK(z.budgets.size() == 2 && z.r.code == E_INTERNAL && !z.r.ran && !z.r.handed && gate_is(t, 0, 16) && z.left == 4.0);
    const Run w = run(t, -1, 1e-3, {st(LP_ST_LOST)}, plain, walk);
    CHECK(stepped_aside(w.r) && gate_is(t, 16, 32));
}

static void no_status()
{
    g_case = "no status written";
    Gate g;
    const Run x = run(g, -1, 1e-3, {st(LP_ST_RUNNING, 3)});
    CHECK(relaunch::INTERNAL == E_INTERNAL && relaunch::GO_ON == 0 && relaunch::HAND_OVER == 0);
    CHECK(x.budgets.size() == 1 && x.r.code == E_INTERNAL && !x.r.ran && !x.r.handed && x.r.sweeps == 0 && gate_is(g, 0, 16));
}

static void the_family_decides()
{
    g_case = "completed: go on, stop";
    Gate g;
    std::vector<int> seen;
    const Completed vns = [&](int status, int sweeps) {
        seen.push_back(status * 100 + sweeps);
        return status == LP_ST_VNS_DONE ? relaunch::STOP : status == LP_ST_NEED_RAND || status == LP_ST_OPTIMUM ? relaunch::GO_ON : (int)E_EXHAUSTED;
    };
    const Run x = run(g, -1, 1e-3, {st(LP_ST_NEED_RAND, 1), st(LP_ST_OPTIMUM, 2), st(LP_ST_NEED_RAND, 3), st(LP_ST_VNS_DONE, 4), st(LP_ST_OPTIMUM, 5)}, vns);
    CHECK(x.budgets.size() == 4 && x.r.code == 0 && x.r.ran && x.r.sweeps == 10);
    CHECK(seen == std::vector<int>({701, 102, 703, 604}));
    g_case = "completed: an error code";
    const Run y = run(g, -1, 1e-3, {st(LP_ST_NEED_RAND, 1), st(LP_ST_CAPPED, 2), st(LP_ST_VNS_DONE, 3)}, vns);
    CHECK(y.budgets.size() == 2 && y.r.code == E_EXHAUSTED && !y.r.ran && !y.r.handed && y.r.sweeps == 3 && gate_is(g, 0, 16));
}

int main()
{
    no_deadline_optimum();
    step_aside_and_back_off();
    launch_refused();
    deadline_budgets();
    mid_descent_failure();
    retries_are_cumulative();
    lost_exchange();
    no_status();
    the_family_decides();
    puts("relaunch ok");
    return 0;
}
