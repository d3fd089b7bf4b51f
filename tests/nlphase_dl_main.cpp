// The phase machine of a tour of a batched descent with don't-look bits (csrc/tspgpu_nlphase.h: nlphase_close(NlbDlCtl),
// nlphase_empty), stand-alone on the CPU, stepped as k_nlb_queue and the apply's close step it.
//
//   nlphase_dl <file>   every line of the file is a case: THREE closing n count, then count events "K q":
//                       K >= 0: a sweep over a queue of q units that accepted K moves;  K = -1: the queue pass found the set of
//                       the phase empty and the phase does not close (no sweep).
// Per case three lines: the index of the event that ended the descent (-1: none did; -2: an event came behind the end; -3: a
// pending "wake all" met a queue that was not full), the eight counters, looked, full sweeps, the largest partial |Q|;  the
// phase in front of every event;  the "wake all" mark behind every event.
#include <cstdio>
#include <cstring>
#include <vector>

#include "tspgpu_nlphase.h"

template <bool THREE>
static void run(int closing, int n, const std::vector<int> &ev)
{
    NlbCtl c;
    LookCtl k;
    memset(&c, 0, sizeof c);
    memset(&k, 0, sizeof k);
    c.rounds = 1;
    int ended = -1;
    std::vector<int> phases, wakes;
    for (size_t e = 0; e * 2 < ev.size(); e++) {
        const int K = ev[2 * e], q = ev[2 * e + 1];
        if (c.stop) { ended = -2; break; }
        phases.push_back(c.phase);
        int next;
        if (K < 0)
            next = nlphase_empty<THREE>(&c);
        else {
            if (k.wake_all && q != n) { ended = -3; break; }    // (the queue pass: every node, and the mark is taken down)
            k.wake_all = 0;
            k.qlen = k.last_q = q;
            k.looked += q;
            if (q == n) k.full += 1;
            else k.max_q = k.max_q > q ? k.max_q : q;
            NlbDlCtl r{c.stop, 0, &c, &k, closing, n};
            next = nlphase_close<THREE>(&r, K);
        }
        wakes.push_back(k.wake_all);
        if (next == NLPHASE_STOP) ended = (int)e;
        if ((next == NLPHASE_STOP) != (c.stop != 0)) ended = -4;
    }
    printf("%d %lld %lld %lld %lld %d %lld %lld %d %lld %lld %d\n", ended, c.two_opt_sweeps, c.two_opt_moves, c.or_sweeps, c.or_moves, c.rounds,
           c.three_sweeps, c.three_moves, c.three_phases, k.looked, k.full, k.max_q);
    for (int p : phases) printf("%d ", p);
    printf("\n");
    for (int w : wakes) printf("%d ", w);
    printf("\n");
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    int three, closing, n, count;
    while (fscanf(f, "%d %d %d %d", &three, &closing, &n, &count) == 4) {
        std::vector<int> ev((size_t)count * 2);
        for (int &v : ev)
            if (fscanf(f, "%d", &v) != 1) { fclose(f); return 3; }
        if (three) run<true>(closing, n, ev);
        else run<false>(closing, n, ev);
    }
    fclose(f);
    return 0;
}
