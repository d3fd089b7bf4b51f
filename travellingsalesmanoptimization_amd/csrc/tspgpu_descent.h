// The descent over the neighbour lists as the host runs it on one tour, and the record of what any descent did.  The rule
// ("Neighbour-list Or-opt" rule 8 and "Neighbour-list 3-opt" in include/tspgpu.h):
//   { list 2-opt to its end; list Or-opt until a sweep accepts nothing } until an Or-opt phase applies nothing;
//   then, where the descent has one, a 3-opt phase; all of it until a 3-opt phase applies nothing.
// This is its one statement on the host; the device's is tspgpu_nlphase.h.  Host-only and free of HIP headers, as
// tspgpu_looks.h: templated on the callables of its user (tests/descent_main.cpp scripts them).
#pragma once
#include <algorithm>

// what a descent did on one tour: 2-opt sweeps and moves, Or-opt sweeps and moves, rounds; 3-opt sweeps, moves and phases;
// looked units and full sweeps.  A family, a descent without a 3-opt phase or one without looks leaves what it has none of 0
struct Descent {
    long tw = 0, tm = 0, os = 0, om = 0;
    int nr = 0;
    long hs = 0, hm = 0;
    int np = 0;
    long lk = 0, lf = 0;
    void operator+=(const Descent &d)
    {
        tw += d.tw; tm += d.tm; os += d.os; om += d.om; nr += d.nr; hs += d.hs; hm += d.hm; np += d.np; lk += d.lk; lf += d.lf;
    }
};

// the caller's arrays for them, each optional, in the order of Descent's members
struct DescentOut {
    long *tw = nullptr, *tm = nullptr, *os = nullptr, *om = nullptr;
    int *nr = nullptr;
    long *hs = nullptr, *hm = nullptr;
    int *np = nullptr;
    long *lk = nullptr, *lf = nullptr;
};

// D[0 .. count) to the caller's arrays
inline void descent_out(const Descent *D, int count, const DescentOut &o)
{
    for (int i = 0; i < count; i++) {
        if (o.tw) o.tw[i] = D[i].tw;
        if (o.tm) o.tm[i] = D[i].tm;
        if (o.os) o.os[i] = D[i].os;
        if (o.om) o.om[i] = D[i].om;
        if (o.nr) o.nr[i] = D[i].nr;
        if (o.hs) o.hs[i] = D[i].hs;
        if (o.hm) o.hm[i] = D[i].hm;
        if (o.np) o.np[i] = D[i].np;
        if (o.lk) o.lk[i] = D[i].lk;
        if (o.lf) o.lf[i] = D[i].lf;
    }
}

namespace descent {
enum Family : int { TWO_OPT = 0, OR_OPT = 1, THREE_OPT = 2 };   // NlbCtl::phase's numbers

// the most one sweep of a family accepted, over the phases of the descent
struct Peaks { long k[3] = {0, 0, 0}; };

// phase(family, &sweeps, &moves, &late) runs one phase to its end and answers an error code or 0; peak(family) is the most one
// sweep of the phase just run accepted.  width: the 3-opt phase's, 0: the descent has none.  A phase that answers a code or
// ends late ends the descent; a 2-opt phase that ends late has begun its round (nr counts it), a phase that answers a code
// counts nothing.  *out, *peaks and *late are written whatever the answer
template <class Phase, class Peak>
int alternate(int width, Phase &&phase, Peak &&peak, Descent *out, Peaks *peaks, bool *late)
{
    Descent D;
    Peaks P;
    int rc = 0;
    *late = false;
    for (;;) {
        long s = 0, m = 0;
        if ((rc = phase(TWO_OPT, &s, &m, late))) break;
        D.tw += s; D.tm += m; D.nr++; P.k[TWO_OPT] = std::max(P.k[TWO_OPT], (long)peak(TWO_OPT));
        if (*late) break;
        if ((rc = phase(OR_OPT, &s, &m, late))) break;
        D.os += s; D.om += m; P.k[OR_OPT] = std::max(P.k[OR_OPT], (long)peak(OR_OPT));
        if (*late) break;
        if (m != 0) continue;               // the Or-opt phase applied something: a round begins
        if (width == 0) break;
        if ((rc = phase(THREE_OPT, &s, &m, late))) break;
        D.hs += s; D.hm += m; D.np++; P.k[THREE_OPT] = std::max(P.k[THREE_OPT], (long)peak(THREE_OPT));
        if (*late || m == 0) break;
    }
    *out = D; *peaks = P;
    return rc;
}
} // namespace descent
