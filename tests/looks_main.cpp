// csrc/tspgpu_looks.h -- rounds of launches between looks at a control block -- over scripted rounds and looks and a clock
// that the script advances.  Every expected count is worked out here.  Built with -fsanitize=address,undefined and run by
// tests/test_looks.py; exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "tspgpu_looks.h"

static const char *g_case = "";
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed (%s)\n", __FILE__, __LINE__, #cond, g_case); exit(2); } \
    } while (0)

using looks::Result;

static const int E_EXHAUSTED = 8, E_INTERNAL = 13;
static double g_now = 0;
static double now() { return g_now; }

// a single tour: every round takes round_dt; round number fail_round (from 1) answers fail_code; look number L answers
// looks[L - 1] (GO_ON past the script's end is a failure of the test: the loop must have ended)
struct Single {
    double round_dt = 0;
    int fail_round = 0, fail_code = 0;
    std::vector<int> looks_;
    int rounds = 0, nlooks = 0;
    std::string order;              // 'r' per round, 'l' per look
    Result run(double time_left, int per_look)
    {
        const double t_end = time_left >= 0 ? g_now + time_left : -1;
        return looks::drive(
            now, t_end, per_look,
            [&] { rounds++; order += 'r'; g_now += round_dt; return rounds == fail_round ? fail_code : 0; },
            [&] { CHECK((size_t)nlooks < looks_.size()); order += 'l'; return looks_[nlooks++]; });
    }
};

static std::string groups(int n, int per) { std::string s; for (int g = 0; g < n; g++) s += std::string(per, 'r') + 'l'; return s; }

static void single_tour()
{
    for (int per : {4, 8}) {
        g_case = "no deadline: per_look rounds between looks";
        Single a;
        a.looks_ = {looks::GO_ON, looks::GO_ON, looks::STOP};
        a.round_dt = 1000.0;                        // the clock does not matter without a deadline
        const Result r = a.run(-1, per);
        CHECK(r.code == 0 && !r.late && a.rounds == 3 * per && a.nlooks == 3 && a.order == groups(3, per));

        g_case = "a deadline: one round per look";
        Single b;
        b.looks_ = {looks::GO_ON, looks::GO_ON, looks::GO_ON, looks::STOP};
        b.round_dt = 0.1;
        const Result q = b.run(10.0, per);
        CHECK(q.code == 0 && !q.late && b.rounds == 4 && b.nlooks == 4 && b.order == groups(4, 1));

        g_case = "a deadline already passed: nothing runs";
        Single c;
        const Result z = c.run(0.0, per);           // now() >= t_end holds at once
        CHECK(z.code == 0 && z.late && c.rounds == 0 && c.nlooks == 0);

        g_case = "the deadline passes between groups";
        Single d;
        d.looks_ = {looks::GO_ON, looks::GO_ON, looks::GO_ON};
        d.round_dt = 0.4;                           // groups start at 0, 0.4, 0.8; at 1.2 the deadline of 1.0 is behind
        const Result l = d.run(1.0, per);
        CHECK(l.code == 0 && l.late && d.rounds == 3 && d.nlooks == 3 && d.order == groups(3, 1));

        g_case = "an error from the k-th round of a group: no look behind it";
        for (int k = 1; k <= per; k++) {
            Single e;
            e.looks_ = {looks::GO_ON};
            e.fail_round = per + k; e.fail_code = E_EXHAUSTED;      // the k-th round of the second group
            const Result x = e.run(-1, per);
            CHECK(x.code == E_EXHAUSTED && !x.late && e.rounds == per + k && e.nlooks == 1 && e.order == groups(1, per) + std::string(k, 'r'));
        }

        g_case = "an error from a look";
        Single f;
        f.looks_ = {looks::GO_ON, E_INTERNAL};
        const Result y = f.run(-1, per);
        CHECK(y.code == E_INTERNAL && !y.late && f.rounds == 2 * per && f.nlooks == 2);

        g_case = "a stop at the first look";
        Single g;
        g.looks_ = {looks::STOP};
        const Result s = g.run(-1, per);
        CHECK(s.code == 0 && !s.late && g.rounds == per && g.nlooks == 1 && s.max_live == 0);
    }
    g_case = "an error under a deadline";
    Single h;
    h.looks_ = {looks::GO_ON};
    h.fail_round = 2; h.fail_code = E_EXHAUSTED;
    h.round_dt = 0.1;
    const Result x = h.run(10.0, 4);
    CHECK(x.code == E_EXHAUSTED && !x.late && h.order == "rlr");
}

// a live list: entry e stops once `stop_after[e]` looks have been taken
struct Live {
    std::vector<int> list, stop_after = std::vector<int>(16, 1 << 30);
    double round_dt = 0;
    int fail_read = 0, fail_upload = 0;             // the look / upload (from 1) that answers code 13
    int rounds = 0, reads = 0, uploads = 0;
    std::vector<int> group_lens, round_lens;
    std::vector<std::vector<int>> uploaded;
    Result run(double time_left, int per_look)
    {
        const double t_end = time_left >= 0 ? g_now + time_left : -1;
        return looks::drive_live(
            now, t_end, per_look, list, [&](int len) { group_lens.push_back(len); },
            [&](int len) { rounds++; round_lens.push_back(len); g_now += round_dt; return 0; },
            [&] { reads++; return reads == fail_read ? E_INTERNAL : 0; }, [&](int e) { return reads >= stop_after[e]; },
            [&](const std::vector<int> &l) { uploads++; uploaded.push_back(l); return uploads == fail_upload ? E_INTERNAL : 0; });
    }
};

typedef std::vector<int> V;

static void live_list()
{
    g_case = "live list: entries leave by the predicate, the order stays, uploads only on a shrink to a non-empty list";
    Live a;
    a.list = {7, 3, 9, 5, 11};
    a.stop_after[3] = 1; a.stop_after[5] = 1;       // leave at look 1
    a.stop_after[7] = 3;                            // look 2 drops nobody; look 3 drops 7
    a.stop_after[9] = 4; a.stop_after[11] = 4;      // look 4 empties the list
    const Result r = a.run(-1, 4);
    CHECK(r.code == 0 && !r.late && a.list.empty());
    CHECK(a.reads == 4 && a.rounds == 16 && a.group_lens == V({5, 3, 3, 2}) && r.max_live == 5);
    CHECK(a.round_lens == V({5, 5, 5, 5, 3, 3, 3, 3, 3, 3, 3, 3, 2, 2, 2, 2}));
    CHECK(a.uploads == 2 && a.uploaded[0] == V({7, 9, 11}) && a.uploaded[1] == V({9, 11}));    // not after look 2, not the empty list

    g_case = "live list: per_look 8, and a deadline gives one round per look";
    Live b;
    b.list = {0, 1};
    b.stop_after[0] = 2; b.stop_after[1] = 2;
    const Result q = b.run(-1, 8);
    CHECK(q.code == 0 && b.rounds == 16 && b.reads == 2 && b.uploads == 0 && b.group_lens == V({2, 2}) && q.max_live == 2);
    Live c;
    c.list = {4, 2, 6};
    c.stop_after[2] = 2; c.stop_after[4] = 3; c.stop_after[6] = 3;
    c.round_dt = 0.01;
    const Result z = c.run(100.0, 8);
    CHECK(z.code == 0 && !z.late && c.rounds == 3 && c.reads == 3 && c.group_lens == V({3, 3, 2}) && c.uploads == 1 && c.uploaded[0] == V({4, 6}));

    g_case = "live list: empty on entry";
    Live d;
    const Result e = d.run(-1, 4);
    CHECK(e.code == 0 && !e.late && e.max_live == 0 && d.rounds == 0 && d.reads == 0 && d.uploads == 0 && d.group_lens.empty());
    Live d2;
    const Result e2 = d2.run(0.0, 4);               // ... is not late either: nothing was left to do
    CHECK(e2.code == 0 && !e2.late && d2.rounds == 0 && d2.reads == 0);

    g_case = "live list: deadlines";
    Live f;
    f.list = {1, 2, 3};
    const Result l0 = f.run(0.0, 4);
    CHECK(l0.late && l0.code == 0 && l0.max_live == 0 && f.rounds == 0 && f.reads == 0 && f.group_lens.empty() && f.list == V({1, 2, 3}));
    Live g;
    g.list = {1, 2, 3};
    g.stop_after[2] = 1;
    g.round_dt = 0.6;                               // groups start at 0 and 0.6; at 1.2 the deadline of 1.0 is behind
    const Result l1 = g.run(1.0, 4);
    CHECK(l1.late && l1.code == 0 && g.rounds == 2 && g.reads == 2 && g.group_lens == V({3, 2}) && l1.max_live == 3 && g.list == V({1, 3}));
    CHECK(g.uploads == 1);

    g_case = "live list: errors from the read and from the upload";
    Live h;
    h.list = {1, 2};
    h.fail_read = 2;
    const Result x = h.run(-1, 4);
    CHECK(x.code == E_INTERNAL && h.rounds == 8 && h.reads == 2 && h.uploads == 0 && x.max_live == 2);
    Live i;
    i.list = {1, 2, 3};
    i.stop_after[1] = 1;
    i.fail_upload = 1;
    const Result y = i.run(-1, 4);
    CHECK(y.code == E_INTERNAL && i.rounds == 4 && i.reads == 1 && i.uploads == 1 && i.list == V({2, 3}));
}

int main()
{
    single_tour();
    live_list();
    puts("looks ok");
    return 0;
}
