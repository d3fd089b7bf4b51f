// The phase machine of a tour of a batched neighbour-list descent: the control block and what the close of a sweep does to it.
// Plain C++ for host and device, free of HIP headers: the device's m2_close(NlbCtl) (tspgpu_nlbatch.inc) calls nlphase_close,
// and tests/nlphase_main.cpp feeds it the accepted counts of the CPU model's sweeps (tests/nlphase_dl_main.cpp: the form with
// don't-look bits).  The rule is in include/tspgpu.h ("Batched neighbour-list descent", "Batched neighbour-list 3-opt",
// "Batched don't-look bits") and DESIGN 4.16 / 4.22 / 4.23.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NLPHASE_HD __host__ __device__ inline
#else
#define NLPHASE_HD inline
#endif

struct NlbCtl {             // one per slot of the range a batched descent runs on
    int phase;              // 0: neighbour-list 2-opt, 1: neighbour-list Or-opt, 2: neighbour-list 3-opt
    int stop;               // 1: the descent of this tour has ended: later launches return at once
    int m;                  // candidates of the current sweep (k_nlb_compact)
    int last_k;             // moves the last sweep accepted
    int max_k;              // the most one sweep accepted
    int rounds;             // 2-opt phases begun
    long long phase_moves;  // moves applied since the phase began
    long long two_opt_sweeps, two_opt_moves, or_sweeps, or_moves;   // running totals (the empty sweep of every phase included)
    long long three_sweeps, three_moves;                            // the same of the 3-opt phases
    int three_phases;       // 3-opt phases begun
    int three_max_k;        // the most one 3-opt sweep accepted
};

// what the close of a sweep asks of the slot
enum : int {
    NLPHASE_GO = 0,         // the sweep accepted something: the phase goes on
    NLPHASE_SWITCH = 1,     // the phase has ended and the next one begins: done = 0, nsweeps = 0, cap_sweeps = -1
    NLPHASE_STOP = 2        // the descent has ended: done = 1
};

// The close of a sweep that accepted K moves.  THREE: the descent has a 3-opt phase behind every alternation of the other two
// that has run to its end; without it the Or-opt phase that applied nothing ends the descent.
//   0 -> 1;  1 -> 0, a round begins, if the Or-opt phase applied something;  1 -> 2 (THREE) or the end, if it applied nothing;
//   2 -> 0, a round begins, if the 3-opt phase applied something;  2 -> the end, if it applied nothing
// nlphase_count: the counters of a sweep of the phase in hand.  nlphase_next: the phase has ended
template <bool THREE>
NLPHASE_HD void nlphase_count(NlbCtl *c, int K)
{
    c->last_k = K;
    c->max_k = c->max_k > K ? c->max_k : K;
    c->phase_moves += K;
    if (c->phase == 0) { c->two_opt_sweeps += 1; c->two_opt_moves += K; }
    else if (!THREE || c->phase == 1) { c->or_sweeps += 1; c->or_moves += K; }
    else { c->three_sweeps += 1; c->three_moves += K; c->three_max_k = c->three_max_k > K ? c->three_max_k : K; }
}

template <bool THREE>
NLPHASE_HD int nlphase_next(NlbCtl *c)
{
    const bool idle = c->phase_moves == 0;
    if (c->phase == 0) c->phase = 1;
    else if (c->phase == 1 && !idle) { c->phase = 0; c->rounds += 1; }      // back to 2-opt: a round begins
    else if (c->phase == 1 && THREE) { c->phase = 2; c->three_phases += 1; }
    else if (idle) { c->stop = 1; return NLPHASE_STOP; }    // an Or-opt phase (no 3-opt) or a 3-opt phase that applied nothing
    else { c->phase = 0; c->rounds += 1; }                  // behind a 3-opt phase that applied something: a new alternation
    c->phase_moves = 0;
    return NLPHASE_SWITCH;
}

template <bool THREE>
NLPHASE_HD int nlphase_close(NlbCtl *c, int K)
{
    nlphase_count<THREE>(c, K);
    if (K) return NLPHASE_GO;
    return nlphase_next<THREE>(c);
}

// ---- the same with don't-look bits ("Batched don't-look bits") ----------------------------------------------
struct LookCtl {            // one per context (a phase with looks on a slot: reset before it), and one per slot of a batch with looks
    int qlen;               // |Q| of the sweep in hand
    int last_q;             // |Q| of the last sweep that ran
    int max_q;              // the largest |Q| of a sweep that was not full
    int wake_all;           // batch: the close left "every node wakes" for the next queue pass (a closing phase)
    long long looked;       // sum of |Q|
    long long full;         // sweeps with |Q| = n
};

// What the apply of a tour of a batch with looks hands its bodies as their control block: the two cells they read, copied in
// front of them, and where the close writes.  The type picks m2_close's and nlphase_close's overloads, as NlbCtl3 does
struct NlbDlCtl {
    int stop, m;            // NlbCtl::stop and NlbCtl::m as the workgroup found them
    NlbCtl *c;
    LookCtl *k;
    int closing, n;
};

// The close of a sweep of |Q| = k->last_q units that accepted K moves.  A sweep that accepted nothing and was not full does
// not end a closing phase (looks::after_stop's WAKE_GO, taken here instead of on the host): it counts, and the next queue pass
// finds every node awake.  Everything else is nlphase_close
template <bool THREE>
NLPHASE_HD int nlphase_close(NlbDlCtl *r, int K)
{
    if (K == 0 && r->closing && r->k->last_q < r->n) {
        nlphase_count<THREE>(r->c, 0);
        r->k->wake_all = 1;
        return NLPHASE_GO;
    }
    return nlphase_close<THREE>(r->c, K);
}

// The queue pass found the phase's set empty and the phase does not close: the phase ends with no sweep counted, as a phase
// that applied nothing (it began with this pass: no sweep of it ran)
template <bool THREE>
NLPHASE_HD int nlphase_empty(NlbCtl *c)
{
    return nlphase_next<THREE>(c);
}
