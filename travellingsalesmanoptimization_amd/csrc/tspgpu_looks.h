// The look loop of the drivers that launch rounds on a stream and now and then read a control block back: m2_run (plain and,
// with an M2Looks, the phase with looks, which asks after_stop below), or_run, the Or-opt phase of or_descent_batch,
// nlb_descent, the sweep loop of nlv_walks and the rounds of greedy_phase.  Host-only and free of HIP headers, as
// tspgpu_relaunch.h: templated on a clock and on the callables of its user (tests/looks_main.cpp scripts them).
//
// A GROUP is: the deadline check, the group hook, the rounds, one look.  Before each group, t_end >= 0 and now() >= t_end make
// the result late and nothing more is launched.  A group has one round under a deadline, else per_look rounds.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace looks {
// round() answers an error code or 0; look() answers GO_ON, STOP or an error code
enum : int { GO_ON = 0, STOP = -1 };

// late: the deadline passed in front of a group (the caller may still read its control block once).  max_live: drive_live's
// longest list at the head of a group
struct Result { int code = 0; bool late = false; long max_live = 0; };

// a round that answers a code ends the loop with it at once, with no look behind it
template <class Clock, class Group, class Round, class Look>
Result drive(Clock &&now, double t_end, int per_look, Group &&group, Round &&round, Look &&look)
{
    Result r;
    for (;;) {
        if (t_end >= 0 && now() >= t_end) { r.late = true; return r; }
        group(r);
        const int K = t_end >= 0 ? 1 : per_look;
        for (int i = 0; i < K; i++)
            if ((r.code = round())) return r;
        const int next = look();
        if (next == STOP) return r;
        if (next != GO_ON) { r.code = next; return r; }
    }
}

template <class Clock, class Round, class Look>
Result drive(Clock &&now, double t_end, int per_look, Round &&round, Look &&look)
{
    return drive(now, t_end, per_look, [](Result &) {}, round, look);
}

// What the host does when it finds a phase with looks ("Don't-look bits") stopped, from the control blocks it read: the phase's
// sweeps and budget left (< 0: no cap), the moves of its last sweep and that sweep's |Q|.
//   END      the phase is over: nothing ran, the last sweep accepted something (so the budget ended it), the last sweep was
//            full, or the phase does not close
//   WAKE_END the last sweep accepted nothing and was not full, and the phase closes: every node wakes, but the budget is spent
//   WAKE_GO  ... and the phase goes on
enum class AfterStop { END, WAKE_END, WAKE_GO };
inline AfterStop after_stop(bool closing, long long sweeps, int last_k, int last_q, int n, long long budget)
{
    if (!closing || sweeps == 0 || last_k != 0 || last_q >= n) return AfterStop::END;
    return budget == 0 ? AfterStop::WAKE_END : AfterStop::WAKE_GO;
}

// The same over a list of live entries, until it is empty (an empty list on entry launches nothing).  group(len) runs at the
// head of a group; round(len) launches for the first len entries; read() fetches the control blocks (an error code or 0);
// stopped(entry) says whether an entry leaves.  The list keeps its order, and set_live(list) uploads it (an error code or 0)
// only when it shrank and is not empty: the caller uploads the list it enters with.
template <class Clock, class Group, class Round, class Read, class Stopped, class SetLive>
Result drive_live(Clock &&now, double t_end, int per_look, std::vector<int> &live, Group &&group, Round &&round, Read &&read, Stopped &&stopped,
                  SetLive &&set_live)
{
    if (live.empty()) return Result{};
    return drive(
        now, t_end, per_look,
        [&](Result &r) {
            r.max_live = std::max(r.max_live, (long)live.size());
            group((int)live.size());
        },
        [&] { return round((int)live.size()); },
        [&]() -> int {
            const int rc = read();
            if (rc) return rc;
            size_t k = 0;
            for (int e : live)
                if (!stopped(e)) live[k++] = e;
            if (k == live.size()) return GO_ON;
            live.resize(k);
            return k ? set_live(live) : (int)STOP;
        });
}
} // namespace looks
