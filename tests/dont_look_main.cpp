// The host's part of a phase with looks (include/tspgpu.h "Don't-look bits", rule 6): looks::after_stop of csrc/tspgpu_looks.h
// under looks::drive, over a scripted device.  The device here is what the kernels do to the two control blocks: a sweep
// counts itself, a sweep that accepts nothing or spends the budget raises `stop`, launches behind `stop` do nothing, an empty
// set at the head of a phase ends it without a sweep (closing = 0) or looks at every node (closing != 0).
// Stand-alone: g++ -fsanitize=address,undefined, run directly (tests/test_dont_look.py).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tspgpu_looks.h"

#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); std::exit(1); } } while (0)

namespace {
struct Sweep { int q, k; };     // |Q| of the awake set as it stands (0: empty) and the moves the sweep accepts

struct Device {
    int n;
    bool closing;
    std::vector<Sweep> script;  // the sweeps in the order they run; a woken-all sweep reads q = n whatever the script says
    size_t at = 0;
    bool all = false;           // the host woke every node
    int stop = 0, last_k = 0, last_q = 0;
    long long sweeps = 0, moves = 0, budget = -1, looked = 0, full = 0;
    int launches = 0, wakes = 0;

    void round()
    {
        launches++;
        if (stop) return;
        CHECK(at < script.size());
        Sweep s = script[at];
        if (all) s.q = n;
        if (s.q == 0 && !closing) { stop = 1; return; }       // (no sweep counted; the script entry is not consumed)
        if (s.q == 0) s.q = n;
        at++;
        all = false;
        last_q = s.q; looked += s.q; full += s.q == n;
        last_k = s.k; sweeps++; moves += s.k;
        bool st = s.k == 0;
        if (budget >= 0) { budget--; st |= budget <= 0; }
        if (st) stop = 1;
    }
};

struct Out { long long sweeps, moves, looked, full; int wakes, launches; bool late; };

Out phase(Device &D, long max_sweeps, double t_end, double dt)
{
    double t = 0;
    D.budget = max_sweeps;
    const looks::Result r = looks::drive(
        [&] { const double x = t; t += dt; return x; }, t_end, 4, [&] { D.round(); return 0; },
        [&]() -> int {
            if (!D.stop) return looks::GO_ON;
            const looks::AfterStop next = looks::after_stop(D.closing, D.sweeps, D.last_k, D.last_q, D.n, D.budget);
            if (next == looks::AfterStop::END) return looks::STOP;
            D.all = true; D.wakes++;
            if (next == looks::AfterStop::WAKE_END) return looks::STOP;
            D.stop = 0;
            return looks::GO_ON;
        });
    CHECK(r.code == 0);
    return Out{D.sweeps, D.moves, D.looked, D.full, D.wakes, D.launches, r.late};
}
} // namespace

int main()
{
    using looks::AfterStop;
    // the decision table
    CHECK(looks::after_stop(false, 3, 0, 5, 100, -1) == AfterStop::END);        // no closing
    CHECK(looks::after_stop(true, 0, 0, 0, 100, -1) == AfterStop::END);         // nothing ran
    CHECK(looks::after_stop(true, 3, 2, 5, 100, 0) == AfterStop::END);          // the budget ended it behind a sweep with moves
    CHECK(looks::after_stop(true, 3, 0, 100, 100, -1) == AfterStop::END);       // the last sweep was full
    CHECK(looks::after_stop(true, 3, 0, 5, 100, -1) == AfterStop::WAKE_GO);
    CHECK(looks::after_stop(true, 3, 0, 5, 100, 7) == AfterStop::WAKE_GO);
    CHECK(looks::after_stop(true, 3, 0, 5, 100, 0) == AfterStop::WAKE_END);

    {   // closing: a partial sweep that finds nothing wakes all; the full sweep finds a move; two more; the closing full sweep
        Device D{100, true, {{100, 3}, {9, 1}, {4, 0}, {0, 2}, {6, 0}, {0, 0}}};
        const Out o = phase(D, -1, -1, 0);
        CHECK(o.sweeps == 6 && o.moves == 6 && o.wakes == 2 && !o.late);
        CHECK(o.looked == 100 + 9 + 4 + 100 + 6 + 100 && o.full == 3);
        CHECK(o.launches == 12);            // three groups of four; the launches behind a stop do nothing
    }
    {   // not closing: the first empty sweep ends the phase, nothing wakes
        Device D{100, false, {{100, 3}, {9, 1}, {4, 0}}};
        const Out o = phase(D, -1, -1, 0);
        CHECK(o.sweeps == 3 && o.moves == 4 && o.wakes == 0 && o.full == 1 && o.looked == 113);
    }
    {   // an empty set on entry: no sweep and no counter without closing, one full sweep with it
        Device D{100, false, {{0, 0}}};
        Out o = phase(D, -1, -1, 0);
        CHECK(o.sweeps == 0 && o.looked == 0 && o.wakes == 0 && o.launches == 4);
        Device E{100, true, {{0, 0}}};
        o = phase(E, -1, -1, 0);
        CHECK(o.sweeps == 1 && o.looked == 100 && o.full == 1 && o.wakes == 0);
    }
    {   // max_sweeps = 1, closing: the cut sweep found nothing and was not full -- every node wakes, the phase ends
        Device D{100, true, {{7, 0}, {0, 0}}};
        Out o = phase(D, 1, -1, 0);
        CHECK(o.sweeps == 1 && o.wakes == 1 && D.all && o.looked == 7);
        D.stop = 0; D.sweeps = D.moves = D.looked = D.full = 0; D.wakes = 0;      // the next call: one full sweep ends it
        o = phase(D, 1, -1, 0);
        CHECK(o.sweeps == 1 && o.full == 1 && o.wakes == 0);
    }
    {   // a deadline: one round per group, and the phase is late in front of the group behind the deadline
        Device D{100, true, {{100, 3}, {9, 1}, {4, 0}, {0, 0}}};
        const Out o = phase(D, -1, 2.5, 1.0);
        CHECK(o.late && o.sweeps == 3 && o.launches == 3 && o.wakes == 1);
    }
    std::printf("dont_look ok\n");
    return 0;
}
