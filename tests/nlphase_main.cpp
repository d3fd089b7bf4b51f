// The phase machine of a tour of a batched neighbour-list descent (csrc/tspgpu_nlphase.h), driven on the host by the accepted
// counts of a tour's sweeps.  tests/test_nl3_batch.py writes one case per line into the file named by argv[1]:
//     THREE len K_0 K_1 ... K_{len-1}
// and reads one line per case back:
//     at two_opt_sweeps two_opt_moves or_sweeps or_moves rounds three_sweeps three_moves three_phases three_max_k max_k switches
// `at` is the index of the sweep whose close ended the descent (-1: the sequence ran out first); nothing behind it is fed.
// After every close the program checks what the device relies on: GO exactly for K > 0, phase in range, phase_moves zeroed by a
// switch, stop raised by STOP alone.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tspgpu_nlphase.h"

template <bool THREE>
static int run(const std::vector<int> &seq, NlbCtl &c, int &switches)
{
    memset(&c, 0, sizeof c);
    c.rounds = 1;                   // as nlb_descent arms a control block
    switches = 0;
    for (size_t x = 0; x < seq.size(); x++) {
        const int phase = c.phase;
        const long long moved = c.phase_moves + seq[x];
        const int next = nlphase_close<THREE>(&c, seq[x]);
        if ((next == NLPHASE_GO) != (seq[x] > 0)) { fprintf(stderr, "sweep %zu: code %d for K = %d\n", x, next, seq[x]); exit(2); }
        if (c.phase < 0 || c.phase > (THREE ? 2 : 1)) { fprintf(stderr, "sweep %zu: phase %d\n", x, c.phase); exit(2); }
        if (c.last_k != seq[x]) { fprintf(stderr, "sweep %zu: last_k %d\n", x, c.last_k); exit(2); }
        if ((c.stop != 0) != (next == NLPHASE_STOP)) { fprintf(stderr, "sweep %zu: stop %d behind code %d\n", x, c.stop, next); exit(2); }
        if (next == NLPHASE_GO && (c.phase != phase || c.phase_moves != moved)) { fprintf(stderr, "sweep %zu: a sweep with moves switched\n", x); exit(2); }
        if (next == NLPHASE_SWITCH) {
            if (c.phase == phase || c.phase_moves != 0) { fprintf(stderr, "sweep %zu: a switch to phase %d with %lld moves\n", x, c.phase, c.phase_moves); exit(2); }
            switches++;
        }
        if (next == NLPHASE_STOP) return (int)x;
    }
    return -1;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: nlphase <cases>\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    int three, len;
    while (fscanf(f, "%d %d", &three, &len) == 2) {
        if (len < 0) { fclose(f); return 2; }
        std::vector<int> seq((size_t)len);
        for (int &k : seq)
            if (fscanf(f, "%d", &k) != 1) { fclose(f); return 2; }
        NlbCtl c;
        int switches;
        const int at = three ? run<true>(seq, c, switches) : run<false>(seq, c, switches);
        printf("%d %lld %lld %lld %lld %d %lld %lld %d %d %d %d\n", at, c.two_opt_sweeps, c.two_opt_moves, c.or_sweeps, c.or_moves, c.rounds,
               c.three_sweeps, c.three_moves, c.three_phases, c.three_max_k, c.max_k, switches);
    }
    fclose(f);
    return 0;
}
