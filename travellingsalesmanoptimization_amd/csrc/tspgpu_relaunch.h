// The relaunch protocol of the one-launch descents (k_lds2opt, k_lds2opt_w, k_str2opt): what keeps a persistent, whole-chip
// kernel honest on a GPU that other work may be using.  Host-only and free of HIP headers, as tspgpu_mem.h: the driver is
// templated on a clock and on three callables of the family it serves (tests/relaunch_main.cpp scripts them).
#pragma once
#include <algorithm>

// what a launch leaves in its status word (ctl[1]): the kernels write these, the driver reads them
enum { LP_ST_RUNNING = 0, LP_ST_OPTIMUM = 1, LP_ST_CAPPED = 2, LP_ST_NO_RENDEZVOUS = 3, LP_ST_LOST = 4, LP_ST_BUDGET = 5,
       LP_ST_VNS_DONE = 6, LP_ST_NEED_RAND = 7 };

namespace relaunch {
// The grid did not come up co-resident: the next `skip` descents keep to the one-launch-per-sweep path, then it is tried
// again -- 16, 32, ... 1024 descents apart while it keeps failing.  Deliberate, all three: there is ONE gate per context,
// shared by the three kernels; it survives a new instance (the chip is as busy as it was); and a descent that asks both
// families in turn (STREAM_PERSIST = 2 with PERSIST = 1) passes it twice and counts twice.
struct Gate {
    int skip = 0, backoff = 16;
    bool skip_this() { if (skip <= 0) return false; skip--; return true; }
    void back_off() { skip = backoff; backoff = std::min(1024, 2 * backoff); }
    void never() { skip = 1 << 30; }        // this device does not grant the launch at all
    void completed() { backoff = 16; }      // a launch came up
    void rearm() { skip = 0; backoff = 16; }
};

// launch(budget, first, status, sweeps) answers an error code or 0; status: what the launch wrote, or REFUSED (not granted)
// completed(status, sweeps) answers GO_ON, STOP or an error code; lost(first) answers HAND_OVER or an error code
enum : int { REFUSED = -1, GO_ON = 0, STOP = -1, HAND_OVER = 0, INTERNAL = 13 };    // INTERNAL: the driver's own error code

// ran = false, code 0: the per-sweep path takes over -- handed: from the tour the last completed launch left; else untouched
struct Result { int code = 0; bool ran = false, late = false, handed = false; long sweeps = 0; };

// t_end < 0: no deadline.  sweep_s: the family's first guess of a sweep's duration; measured from the first launch on
template <class Clock, class Launch, class Completed, class Lost>
Result drive(Gate &gate, Clock &&now, double t_end, double sweep_s, double *time_left_io, Launch &&launch, Completed &&completed, Lost &&lost)
{
    Result r;
    bool first = true;
    int retries = 0;                // failed rendezvous of later launches, over the whole descent
    // hand the rest of the descent to the per-sweep path (nothing of the failed launch was written: the slot is consistent)
    auto hand_over = [&]() {
        r.handed = !first;
        gate.back_off();
        if (time_left_io && t_end >= 0) *time_left_io = std::max(0.0, t_end - now());
        return r;
    };
    for (;;) {
        int budget = -1, status = LP_ST_RUNNING, sweeps = 0;    // budget: the sweeps this launch may run, a third of the time left
        if (t_end >= 0) {
            const double left = t_end - now();
            if (left <= 0) { r.late = true; break; }
            budget = (int)std::min(1048576.0, std::max(1.0, left / 3.0 / sweep_s));
        }
        const double t0 = now();
        if ((r.code = launch(budget, first, status, sweeps))) return r;
        if (status == REFUSED) { if (first) gate.never(); else r.code = INTERNAL; return r; }    // (the family worded the message)
        if (status == LP_ST_NO_RENDEZVOUS) {
            if (first) { gate.back_off(); return r; }       // nothing written: the other path takes over
            if (++retries > 3) return hand_over();          // another context holds CUs (counted over the whole descent)
            continue;
        }
        if (status == LP_ST_LOST)                           // an exchange timed out mid-launch: the grid is no longer co-resident
            return (r.code = lost(first)) != HAND_OVER ? r : hand_over();
        if (status == LP_ST_RUNNING) { r.code = INTERNAL; return r; }      // no status written (the family worded the message)
        first = false;
        gate.completed();
        r.sweeps += sweeps;
        const int next = completed(status, sweeps);
        if (sweeps > 0) sweep_s = (now() - t0) / sweeps;
        if (next == STOP) break;
        if (next != GO_ON) { r.code = next; return r; }
    }
    r.ran = true;
    return r;
}
} // namespace relaunch
