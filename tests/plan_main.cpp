// csrc/tspgpu_plan.h over the case table of tests/golden/golden_plan.json: every decision printed, one line per case, for
// tests/test_plan.py to compare with the recorded ones.  `plan_main FILE` prints the table's decisions; `plan_main anchors`
// checks the figures that the code's own comments state and the caller's contract around a refusal.
#include "tspgpu_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

typedef std::vector<long> Row;

// ---- the decisions under test, as rows of integers ------------------------------------------------------------------------
// [refusal, kernel, G, P, BT, NCH, D, T, lds, lds_fused, pipe2 + 2 pipe2_sweep + 4 tabu_fits + 8 otf_early]; a refusal: its kind,
// and G where the message names it
static Row sweep_row(const plan::In &in, int ntours, bool early, int occ)
{
    const plan::Sweep s = plan::decide(in, ntours, early, [&](plan::Kernel, int, size_t) { return occ; });
    if (s.refused != plan::Refusal::NONE) return Row{(long)s.refused, 0, s.refused == plan::Refusal::WGS ? s.G : 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return Row{0, s.kernel, s.G, s.P, s.BT, s.NCH, s.D, s.T, (long)s.lds, (long)s.lds_fused,
               s.pipe2 + 2 * s.pipe2_sweep + 4 * s.tabu_fits + 8 * s.otf_early};
}
// [otf8, otf_early] + the sweep's row
static Row otf_row(const plan::In &in, bool tabu, int ntours)
{
    const bool early = plan::otf_early(in, tabu);
    Row r{plan::otf8(in.cost_bound, in.n), early};
    const Row s = sweep_row(in, ntours, early, 0);
    r.insert(r.end(), s.begin(), s.end());
    return r;
}
// [form, E, W, Ws, nstage, lds, neither form applies to a plain descent]
static Row resident_row(const plan::In &in, bool tabu)
{
    const plan::Resident r = plan::resident(in, tabu);
    return Row{(long)r.form, r.E, r.W, r.Ws, r.nstage, (long)r.lds, plan::resident(in, false).form == plan::Form::NONE};
}
// [fits, P, W, BT, NCH, lds], zeros where it does not fit
static Row stream_row(const plan::In &in)
{
    const plan::Stream s = plan::stream(in);
    if (!s.fits) return Row{0, 0, 0, 0, 0, 0};
    return Row{1, s.P, s.W, s.BT, s.NCH, (long)s.lds};
}
// family 0: the Or-opt sweep's arguments (four rows, OR_EXTRA, R in [max(2, n / 1024), OR_RMAX]); 1: the parallel-move sweep's
static Row geom_row(const plan::In &in, int family)
{
    const plan::SweepGeom g = family == 0
        ? plan::sweep_geom(in, 4, 3072, std::max(2, (in.n + plan::MAX_WGS_PER_TOUR - 1) / plan::MAX_WGS_PER_TOUR), 64, {1, 2, 3}, 16)
        : plan::sweep_geom(in, 1, 1024, 4, 60, {1, 2, 4, 10}, 16);
    return Row{g.BT, g.NCH, g.R, g.W, g.occ, (long)g.lds};
}

// ---- the case table ---------------------------------------------------------------------------------------------------------
// the integers of the (nested) array behind "key":
static std::vector<long> ints(const std::string &text, const char *key)
{
    const std::string k = std::string("\"") + key + "\":";
    size_t i = text.find(k);
    if (i == std::string::npos) { fprintf(stderr, "no key %s\n", key); exit(2); }
    i = text.find('[', i);
    std::vector<long> v;
    int depth = 0;
    for (; i < text.size(); i++) {
        const char c = text[i];
        if (c == '[') depth++;
        else if (c == ']') { if (--depth == 0) break; }
        else if (c == '-' || (c >= '0' && c <= '9')) {
            char *end;
            v.push_back(strtol(text.c_str() + i, &end, 10));
            i = (size_t)(end - text.c_str()) - 1;
        }
    }
    return v;
}

static void print(const char *what, const Row &r)
{
    printf("%s", what);
    for (long x : r) printf(" %ld", x);
    printf("\n");
}

// the engine's padding rule: rows 128-byte aligned for every element kind
static plan::In input(long cus, long lds_max, long elem, long n)
{
    plan::In in;
    in.cus = (int)cus; in.lds_max = (size_t)lds_max; in.elem = (int)elem; in.n = (int)n; in.ld = ((int)n + 31) & ~31;
    in.has_matrix = true;
    return in;
}

static int table(const char *path)
{
    std::ifstream f(path);
    if (!f) { fprintf(stderr, "cannot read %s\n", path); return 2; }
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string text = ss.str();
    const std::vector<long> devices = ints(text, "devices"), occ_count = ints(text, "occ_count"), occ = ints(text, "occ"), elems = ints(text, "elems"),
                            ns = ints(text, "ns"), ntours = ints(text, "ntours"), options = ints(text, "options"), option_ntours = ints(text, "option_ntours"),
                            otf = ints(text, "otf"), edges = ints(text, "persist_edges"), windows = ints(text, "persist_window"),
                            resident_max_n = ints(text, "resident_max_n"), sp_nch = ints(text, "sp_nch"), none = ints(text, "none");
    const size_t ndev = devices.size() / 2;
    // sweep: device x its occupancy scripts x elem x n x ntours at default options (occ: the scripts of all devices, one after another)
    size_t o0 = 0;
    for (size_t d = 0; d < ndev; o0 += (size_t)occ_count[d], d++)
        for (long k = 0; k < occ_count[d]; k++)
            for (long e : elems)
                for (long n : ns)
                    for (long t : ntours) print("sweep", sweep_row(input(devices[2 * d], devices[2 * d + 1], e, n), (int)t, false, (int)occ[o0 + (size_t)k]));
    // option: [opt_kernel, opt_block, opt_wgs, opt_depth, opt_pipe2] x elem x n x ntours on the first device, occupancy 2
    for (size_t o = 0; o + 5 <= options.size(); o += 5)
        for (long e : elems)
            for (long n : ns)
                for (long t : option_ntours) {
                    plan::In in = input(devices[0], devices[1], e, n);
                    in.opt_kernel = (int)options[o]; in.opt_block = (int)options[o + 1]; in.opt_wgs = (int)options[o + 2];
                    in.opt_depth = (int)options[o + 3]; in.opt_pipe2 = (int)options[o + 4];
                    print("option", sweep_row(in, (int)t, false, 2));
                }
    // otf: [cus, n, cost_bound, int_points, opt_otf_early, opt_ablate, tabu, ntours]
    for (size_t i = 0; i + 8 <= otf.size(); i += 8) {
        plan::In in = input(otf[i], 163840, plan::ELEM_I32, otf[i + 1]);
        in.otf = true; in.has_matrix = false; in.cost_bound = (double)otf[i + 2]; in.int_points = otf[i + 3] != 0;
        in.opt_otf_early = (int)otf[i + 4]; in.opt_ablate = (int)otf[i + 5];
        print("otf", otf_row(in, otf[i + 6] != 0, (int)otf[i + 7]));
    }
    // resident: device x n (up to resident_max_n) x opt_persist_edges x opt_persist_window x tabu, uint16 cells
    for (size_t d = 0; d < ndev; d++)
        for (long n : ns)
            for (long e : edges)
                for (long w : windows)
                    for (int tabu = 0; tabu < 2 && n <= resident_max_n[0]; tabu++) {
                        plan::In in = input(devices[2 * d], devices[2 * d + 1], plan::ELEM_U16, n);
                        in.opt_persist_edges = (int)e; in.opt_persist_window = (int)w;
                        print("resident", resident_row(in, tabu != 0));
                    }
    // stream: device x n x opt_sp_nch, uint16 cells
    for (size_t d = 0; d < ndev; d++)
        for (long n : ns)
            for (long c : sp_nch) {
                plan::In in = input(devices[2 * d], devices[2 * d + 1], plan::ELEM_U16, n);
                in.opt_sp_nch = (int)c;
                print("stream", stream_row(in));
            }
    // none: [elem, otf, symmetric, has_matrix, n] on the first device -- what the one-launch descents do not take
    for (size_t i = 0; i + 5 <= none.size(); i += 5) {
        plan::In in = input(devices[0], devices[1], none[i], none[i + 4]);
        in.otf = none[i + 1] != 0; in.symmetric = none[i + 2] != 0; in.has_matrix = none[i + 3] != 0;
        Row r = resident_row(in, false);
        const Row s = stream_row(in);
        r.insert(r.end(), s.begin(), s.end());
        print("none", r);
    }
    // geom: device x elem x n x {matrix, matrix-free} x {Or-opt, parallel moves}
    for (size_t d = 0; d < ndev; d++)
        for (long e : elems)
            for (long n : ns)
                for (int o = 0; o < 2; o++)
                    for (int fam = 0; fam < 2; fam++) {
                        plan::In in = input(devices[2 * d], devices[2 * d + 1], e, n);
                        in.otf = o != 0;
                        print("geom", geom_row(in, fam));
                    }
    return 0;
}

// ---- anchors: figures from the comments of the code, and the contract around a refusal -------------------------------------
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static bool same(const plan::Sweep &a, const plan::Sweep &b)
{
    return a.kernel == b.kernel && a.G == b.G && a.P == b.P && a.BT == b.BT && a.NCH == b.NCH && a.D == b.D && a.T == b.T && a.lds == b.lds &&
           a.lds_fused == b.lds_fused && a.pipe2 == b.pipe2 && a.pipe2_sweep == b.pipe2_sweep && a.tabu_fits == b.tabu_fits &&
           a.otf_early == b.otf_early && a.refused == b.refused;
}

static int anchors()
{
    auto occ2 = [](plan::Kernel, int, size_t) { return 2; };
    // a whole MI355X, uint16 cells: n = 4096 whole rows, 16 edges on 256 workgroups, all of the LDS; n = 1024 4 edges on 256
    plan::Resident r = plan::resident(input(256, 163840, plan::ELEM_U16, 4096), false);
    CHECK(r.form == plan::Form::ROWS && r.E == 16 && r.W == 256 && r.lds == 163840);
    r = plan::resident(input(256, 163840, plan::ELEM_U16, 1024), false);
    CHECK(r.form == plan::Form::ROWS && r.E == 4 && r.W == 256);
    // fnl4461: past the whole rows, half-window rows
    r = plan::resident(input(256, 163840, plan::ELEM_U16, 4461), false);
    CHECK(r.form == plan::Form::WINDOW && r.Ws > 0 && r.Ws <= 4461 && r.lds <= 163840);
    // what the caller does with a refusal: decide answers a value, and only an accepted one replaces the plan
    const plan::Sweep kept = plan::decide(input(256, 163840, plan::ELEM_U16, 2048), 1, false, occ2);
    CHECK(kept.refused == plan::Refusal::NONE && kept.kernel == 3 && kept.T == 1);
    plan::Sweep cur = kept;
    plan::In big = input(256, 163840, plan::ELEM_F64, 12288);
    big.opt_kernel = 3;
    const plan::Sweep s = plan::decide(big, 64, false, occ2);
    CHECK(s.refused == plan::Refusal::RES_ROWS);
    if (s.refused == plan::Refusal::NONE) cur = s;
    CHECK(same(cur, kept));
    printf("anchors ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s golden_plan.json | anchors\n", argv[0]); return 2; }
    return strcmp(argv[1], "anchors") == 0 ? anchors() : table(argv[1]);
}
