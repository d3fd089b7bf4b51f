// Where the 2-opt launch geometries are decided: the per-sweep plan (kernel variant, threads, workgroups per tour, edges per
// run, LDS bytes), whether and how the one-launch descents apply (k_lds2opt's whole rows, k_lds2opt_w's half windows,
// k_str2opt), the matrix-free kernel, and the geometry of the candidate sweeps.  Host-only and free of HIP headers, as
// tspgpu_relaunch.h and tspgpu_looks.h: arithmetic on what the device and the costs are (In), nothing that launches.  The one
// question that only the runtime answers -- how many workgroups of a kernel a CU holds -- is a callable of the caller's
// (tests/plan_main.cpp scripts it; tests/golden/golden_plan.json pins every decision).
#pragma once
#include <algorithm>
#include <cstddef>
#include <initializer_list>

namespace plan {
// TSPGPU_ELEM_* of include/tspgpu.h (tspgpu.hip asserts the equality)
enum : int { ELEM_F64 = 1, ELEM_I32 = 2, ELEM_U16 = 3 };
inline size_t elem_size(int elem) { return elem == ELEM_F64 ? 8 : elem == ELEM_I32 ? 4 : 2; }

constexpr int MAX_WGS_PER_TOUR = 1024;
// the matrix sweeps pack a pair as min(a,b) << 16 | max(a,b): labels 0..65535
constexpr int MATRIX_MAX_N = 64 * 1024;
constexpr size_t PARTIAL_BYTES = 16;   // sizeof(Partial): a workgroup's best move, {double delta, u64 key}
// k_lds2opt / k_lds2opt_w: tour edges per workgroup at most, threads
constexpr int LP_EMAX = 16, LP_BT = 512;
constexpr int LW_EMAX = 24, LW_BT = 768;    // (768 threads: 170 registers each, ten rows in flight)
// k_sweep_otf8
constexpr int OTF8_RUN = 16;        // tour edges per workgroup: the per-b arrays (36 bytes per b) are streamed once per RUN pairs
constexpr int OTF8_RUN_INT = 64;    // ... with integer points (KIND_CEIL_INT): behind the early-out the sweep is bound by streaming the per-b
// k_str2opt's dynamic LDS: four rows, the node-per-cell array, a run's nodes, the scratch
constexpr size_t sp_lds_rows(int ld) { return (size_t)4 * ld * 2; }
constexpr size_t sp_lds_ord(int n) { return (size_t)((n + 15) & ~7) * 2; }
constexpr size_t sp_lds_nodes(int P) { return (size_t)((P + 2 + 3) & ~3) * 4 + 16; }
constexpr size_t SP_LDS_SCRATCH = 32 * PARTIAL_BYTES + 64 + 16 * 8 * 2;

// what the decisions read: the device, the costs, the options
struct In {
    int cus = 256;
    size_t lds_max = 65536;
    int n = 0, ld = 0, elem = 0;
    bool otf = false, symmetric = true, has_matrix = false;     // otf: matrix-free
    bool int_points = false;    // the integer ceil points exist (ceil_int() && d_ipts)
    double cost_bound = 0;
    int opt_kernel = 0, opt_block = 0, opt_wgs = 0, opt_depth = 0, opt_pipe2 = 1, opt_ablate = 0, opt_otf_early = 0;
    int opt_persist_edges = 0, opt_persist_window = 0, opt_sp_nch = 0;
};

// ---- the instantiations that exist: the selectors of tspgpu.hip (pipe_kernel, pipe2_kernel, res_kernel, fused_kernel) answer
// null where these say no, and the plan asks these ------------------------------------------------------------------------
// k_sweep_pipe<T, nch, depth>: one, two or four 16-byte vectors per thread, three for uint16 cells
inline bool has_pipe(int elem, int nch) { return nch == 1 || nch == 2 || nch == 4 || (nch == 3 && elem == ELEM_U16); }
// ... its two-edge form (depth 9: pipe_stream2, four LDS row buffers): symmetric matrices, plain 2-opt, nch <= 3
inline bool has_pipe2(int elem, int nch) { return nch == 1 || nch == 2 || (nch == 3 && elem == ELEM_U16); }
// k_sweep_res<T, nch>
inline bool has_res(int, int nch) { return nch == 1 || nch == 2; }
// k_sweep_fused<T, nch>: kernel 3: resident rows; kernel 2: streamed rows
inline bool has_fused(int, int nch, int kernel) { return (kernel == 3 || kernel == 2) && (nch == 1 || nch == 2); }

// register-prefetch depth per chunk count: D * NCH 16-byte vectors stay in flight per thread
inline int pipe_depth(int nch, int want)
{
    const int dmax = nch <= 1 ? 8 : nch <= 2 ? 4 : 2; // deeper sets would spill under the 128-VGPR cap
    int d = want > 0 ? want : 2; // measured: deeper sets do not pay (the step is latency-, not bandwidth-bound)
    d = d >= 8 ? 8 : d >= 4 ? 4 : 2;
    return std::min(d, dmax);
}

inline int pow2_ceil(int x) { int p = 1; while (p < x) p <<= 1; return p; }

// ---- matrix-free mode -------------------------------------------------------------------------------------------------------
// the 8-edge matrix-free kernel (k_sweep_otf8) applies: costs below 2^25, 17-bit labels; k_sweep_otf otherwise
inline bool otf8(double cost_bound, int n) { return cost_bound < 33554432.0 && n < 131072; }

// the matrix-free sweep over integer points runs two instantiations with different run lengths (early-out: 64 edges per
// workgroup; full evaluation: 16), so the number of partials a sweep leaves -- what k_apply reduces -- follows the variant
inline bool otf_early(const In &in, bool tabu)
{
    if (!in.otf || tabu || in.opt_ablate == 3 || in.opt_otf_early == 2 || !otf8(in.cost_bound, in.n)) return false;
    if (in.opt_otf_early == 1) return true;          // (hook 91: every weight kind, every size -- tests)
    // automatic: integer points (the tests are integer subtractions and f32 products) and enough 64-edge runs for two workgroups
    // per CU.  Measured (tools/otf_rate.py): pla85900 3.94 -> 0.93 ms per sweep, 85 900 uniform-random integer points (no
    // locality in the node order: only the pair tests reject) 4.01 -> 2.94; but n = 20 000 305 -> 360 us (313 workgroups), and
    // with double points (f64 subtractions in every test) d18512 296 -> 322 us, n = 16 384 uniform 210 -> 345 us
    return in.int_points && in.n >= 128 * in.cus;
}

// ---- the per-sweep plan -----------------------------------------------------------------------------------------------------
// RES_ROWS / PIPE_ROWS: TSPGPU_OPT_KERNEL = 3 / 2 and the resident sweep's rows / three rows do not fit; WGS: the resident sweep
// needs more than MAX_WGS_PER_TOUR workgroups per tour (G says how many); ROW: not even one row fits LDS; MATRIX_N: n over MATRIX_MAX_N
enum class Refusal { NONE, RES_ROWS, PIPE_ROWS, WGS, ROW, MATRIX_N };

// kernel: 1 k_sweep_simple, 2 k_sweep_pipe, 3 k_sweep_res, 4 the matrix-free sweep; 0 no plan.  G workgroups per tour of P tour
// edges, BT threads, NCH 16-byte vectors per thread and row, D the register-prefetch depth, T the tours in flight it was made for
struct Sweep {
    int kernel = 0, G = 0, P = 0, BT = 0, NCH = 0, D = 0, T = 0;
    size_t lds = 0;
    size_t lds_fused = 0;       // dynamic LDS of the one-launch-per-sweep kernel (four row buffers in its two-edge streaming form)
    bool pipe2 = false;         // the fused pipelined kernel streams two tour edges per barrier interval (pipe_stream2)
    bool pipe2_sweep = false;   // ... and so does the plain pipelined sweep (batches; symmetric, not tabu)
    bool tabu_fits = true;      // the tabu variants' extra n + 32 LDS bytes fit beside the rows
    bool otf_early = false;     // the matrix-free plan is the early-out kernel's (runs of 64 edges: plain 2-opt over integer points)
    Refusal refused = Refusal::NONE;
};

// dynamic LDS of a tabu sweep: n + 32 verdict bytes behind everything else (k_sweep_simple keeps none)
inline size_t tabu_lds(const Sweep &s, int n) { return s.kernel != 1 ? ((s.lds + 15) & ~(size_t)15) + n + 32 : s.lds; }

// the kernel whose occupancy decide() asks for: 1 k_sweep_simple<T>, 2 k_sweep_pipe<T, nch, depth> (plain 2-opt both)
struct Kernel { int kernel, nch, depth; };

// Decide kernel variant, block size, workgroups per tour for `ntours` tours in flight.  occupancy(Kernel, threads, lds bytes)
// answers the workgroups of that kernel a CU holds, registers counted, or 0 for "no answer".  A refusal answers a Sweep whose
// `refused` says which; the caller keeps the plan it had
template <class Occ> Sweep decide(const In &in, int ntours, bool early, Occ &&occupancy)
{
    Sweep s;
    s.T = ntours; s.otf_early = early;
    auto refuse = [&](Refusal r) { s.refused = r; return s; };
    const int n = in.n, ld = in.ld;
    const size_t esz = elem_size(in.elem);
    const int V = 16 / (int)esz;
    const int nvec = ld / V;
    const size_t row = (size_t)ld * esz;
    const size_t slack = 1024; // nodes[] + reduction scratch

    int BT = in.opt_block;
    if (BT <= 0) BT = std::min(1024, std::max(64, (nvec + 63) & ~63)); // one 16-byte vector per thread, whole waves
    BT = std::min(1024, std::max(64, (BT + 63) & ~63));

    int kernel = in.opt_kernel;
    int nch = 0;
    auto pipe_fits = [&](int, int P) {
        return 3 * row + (size_t)(P + 4) * 4 + slack <= in.lds_max;
    };
    // provisional G / P
    auto plan_GP = [&](size_t lds, int bt, int &G, int &P, Kernel k) {
        int occ = (int)std::min<size_t>(in.lds_max / std::max<size_t>(lds, 1), (size_t)(2048 / bt));
        const int api = occupancy(k, bt, lds); // registers count too: ask the runtime for this very kernel
        if (api > 0) occ = std::min(occ, api);
        occ = std::max(1, std::min(occ, 8));
        if (bt >= 1024) occ = 1; // measured: one 16-wave workgroup per CU beats two (tools/tune_sweep.py)
        G = in.opt_wgs > 0 ? in.opt_wgs : std::max(1, (in.cus * occ + ntours - 1) / ntours);
        G = std::min(G, MAX_WGS_PER_TOUR);
        G = std::min(G, std::max(1, n / 2));
        P = (n + G - 1) / G;
        G = (n + P - 1) / P;
    };
    int G = 1, P = n;
    if (in.otf) {
        // matrix-free: 8 tour edges per workgroup, the whole b range per workgroup
        P = otf8(in.cost_bound, n) ? (early ? OTF8_RUN_INT : OTF8_RUN) : 8;     // (k_sweep_otf8 / k_sweep_otf: see launch_sweep)
        G = (n + P - 1) / P;
        s.kernel = 4; s.G = G; s.P = P; s.BT = 256;
        return s;
    }
    // resident sweep: all P+1 (<= 9) rows of a run in LDS at once.  One chunk per thread for
    // uint16 (two would spill), at most two otherwise.
    const int res_bt = std::min(1024, std::max(64, (nvec + 63) & ~63));
    const int res_nch = (nvec + res_bt - 1) / res_bt;
    auto res_P = [&]() { // rows that fit: prefer two workgroups per CU when that still gives P = 8
        const size_t extra = slack + 64;
        if (9 * row + extra <= in.lds_max / 2) return 8;
        const long fit = (long)((in.lds_max - extra) / row) - 1;
        return (int)std::min<long>(8, fit);
    };
    const bool res_ok = res_nch <= (in.elem == ELEM_U16 ? 1 : 2) && res_P() >= 2 && n >= 8;
    const bool batch_streams = ntours > 1 && n >= 256 && (size_t)n * row <= ((size_t)256 << 20) && in.opt_wgs <= 0;
    if (kernel == 3 && !res_ok) return refuse(Refusal::RES_ROWS);
    if (kernel == 0) {
        // uint16: resident whenever it fits.  int32 / f64: resident only while 9 rows leave room
        // for two workgroups per CU (small n, multi-start batches); else pipelined; else simple.
        // A single tour whose resident runs would not all be on the chip at once (more than two
        // workgroups per CU's worth: a second, mostly empty round) streams instead.
        const bool res_one_round = ntours > 1 || (n + res_P() - 1) / std::max(1, res_P()) <= 2 * in.cus;
        // A batch of tours (multi-start) over a matrix the last-level cache holds: the streamed kernel with runs of 16 .. 64
        // edges (below) beats the resident one's 8-edge runs at every size from n = 512 up -- a run's fixed cost (the tour
        // state derived, the first rows landed: ~4 us) is paid once per 16 .. 64 rows instead of once per 8:
        // tools/tune_multistart.py, profiles/r03_multistart_plan.txt (pr1002 all starts 94.7 -> 59 ms, n=4096 x 64 330 -> 181 ms,
        // n=8192 x 32 1579 -> 718 ms; f64 pr1002 x 256 82 -> 45 ms)
        if (batch_streams && pipe_fits(BT, 64)) kernel = 2;
        else if (res_ok && (res_one_round || !pipe_fits(BT, 64)) && (in.elem == ELEM_U16 || 9 * row + slack <= in.lds_max / 2)) kernel = 3;
        else kernel = pipe_fits(BT, 64) ? 2 : 1;
    }
    if (kernel == 3) {
        BT = in.opt_block > 0 ? BT : res_bt;
        nch = (nvec + BT - 1) / BT;
        if (nch > (in.elem == ELEM_U16 ? 1 : 2)) { BT = res_bt; nch = res_nch; }
        P = res_P();
        if (in.opt_wgs > 0) P = std::max(2, std::min(P, (n + in.opt_wgs - 1) / in.opt_wgs));
        // a single small tour is latency-bound: shorter runs on more workgroups (up to two per CU)
        // cut the step chain; the extra row per run costs nothing at these sizes (measured:
        // n=1024 11.1 -> 8.7 us per sweep, n=2048 11.9 -> 10.5)
        else if (ntours == 1) P = std::max(2, std::min(P, (n + 2 * in.cus - 1) / (2 * in.cus)));
        G = (n + P - 1) / P;
        if (G > MAX_WGS_PER_TOUR) { s.G = G; return refuse(Refusal::WGS); }
        s.D = 0;
        s.lds = (size_t)(P + 1) * row + (size_t)((P + 2 + 3) & ~3) * 4 + 16 * PARTIAL_BYTES + 64;
    }
    if (kernel == 2) {
        // a single uint16 tour past the resident kernel's size: two 16-byte vectors per thread on half as many threads
        // (tools/tune_n4461.py: fnl4461 24.6 -> 18.2 us per sweep -- 9-wave workgroups fill the SIMDs unevenly --, n = 5000 /
        // 6000 / 8192: 3-5 % faster; n = 16384 takes this shape anyway)
        if (in.opt_block <= 0 && in.elem == ELEM_U16 && ntours == 1 && nvec > 512)
            BT = std::min(1024, std::max(256, ((nvec + 1) / 2 + 63) & ~63));
        nch = (nvec + BT - 1) / BT;
        while (nch > 4 && BT < 1024) { BT *= 2; nch = (nvec + BT - 1) / BT; }
        int inst = nch <= 1 ? 1 : nch <= 2 ? 2 : (nch == 3 && in.elem == ELEM_U16) ? 3 : 4;
        if (nch > 4 || !pipe_fits(BT, 64)) {
            if (in.opt_kernel == 2) return refuse(Refusal::PIPE_ROWS);
            kernel = 1;
        } else {
            nch = inst;
            s.D = pipe_depth(nch, in.opt_depth);
            plan_GP(3 * row + slack, BT, G, P, Kernel{2, nch, s.D});
            if (in.opt_wgs <= 0 && ntours == 1) {
                // a whole number of workgroups per CU (an uneven last round costs a full one), the
                // most that keeps runs of >= 8 edges (each run fetches P+1 rows: extra row <= 12 %)
                int k = std::max(1, G / in.cus);
                // (at most two workgroups per CU: a third one -- 320 .. 448-thread workgroups of uint16 tours around n = 6000
                // fit three -- costs more in row traffic (P + 1 rows per P edges) and skew than it hides: n=6144 30.3 us per
                // sweep with G = 768, 23.2 with G = 512; tools/tune_mid.py)
                k = std::min(k, 2);
                while (k > 1 && (n + in.cus * k - 1) / (in.cus * k) < 8) k--;
                if ((n + in.cus * k - 1) / (in.cus * k) >= 8) { P = (n + in.cus * k - 1) / (in.cus * k); G = (n + P - 1) / P; }
            }
            if (batch_streams) {
                // runs of n/64 edges, 16 .. 64 (f64 rows: n/16, 32 .. 256), shorter while the batch has fewer than four
                // workgroups per CU (the optimum is flat: +-50 % of the run length costs 1-3 %)
                P = in.elem == ELEM_F64 ? std::min(256, std::max(32, n / 16)) : std::min(64, std::max(16, n / 64));
                while (P > 8 && (long)ntours * ((n + P - 1) / P) < 4L * in.cus) P /= 2;
                G = (n + P - 1) / P;
            }
            if (in.opt_wgs <= 0 && P < 8) {
                P = std::min(n, 8); G = (n + P - 1) / P;
            }
            while (!pipe_fits(BT, P) && G < MAX_WGS_PER_TOUR) { G *= 2; P = (n + G - 1) / G; G = (n + P - 1) / P; }
            s.lds = 3 * row + (size_t)((P + 2 + 3) & ~3) * 4 + 16 + 16 * PARTIAL_BYTES + 64;
            s.pipe2 = in.opt_pipe2 && nch <= 2 && P >= 2 && s.lds + row <= in.lds_max;
            s.pipe2_sweep = in.opt_pipe2 && has_pipe2(in.elem, nch) && P >= 2 && s.lds + row <= in.lds_max;
        }
    }
    if (kernel == 1) {
        if (row + slack > in.lds_max) return refuse(Refusal::ROW);
        if (in.opt_block <= 0) BT = std::min(1024, std::max(64, pow2_ceil(nvec / 4)));
        plan_GP(row + slack, BT, G, P, Kernel{1, 0, 0});
        s.lds = row + 16 * PARTIAL_BYTES + 64;
        nch = 0;
    }
    if (n > MATRIX_MAX_N) return refuse(Refusal::MATRIX_N);
    s.kernel = kernel; s.G = G; s.P = P; s.BT = BT; s.NCH = nch;
    if (kernel != 2) s.pipe2 = s.pipe2_sweep = false;
    s.lds_fused = s.lds + (s.pipe2 ? row : 0);
    s.tabu_fits = tabu_lds(s, n) <= in.lds_max;      // plain 2-opt must not fail for the tabu variant's sake
    return s;
}

// ---- the one-launch descents ------------------------------------------------------------------------------------------------
enum class Form { NONE, ROWS, WINDOW };
// E tour edges per workgroup on W workgroups, lds bytes each; the half-window form: Ws window cells per row, nstage staging rows
struct Resident { Form form = Form::NONE; int E = 0, W = 0, Ws = 0, nstage = 0; size_t lds = 0; };

// The LDS-resident descent (k_lds2opt) where it applies: uint16 cells, one tour, a whole chip whose LDS holds the matrix.
inline bool rows_fit(const In &in, bool tabu, Resident &r)
{
    const int n = in.n;
    if (in.elem != ELEM_U16 || in.otf || !in.symmetric || !in.has_matrix || n < 64 || n > 4096) return false;
    int e = (n + in.cus - 1) / in.cus;
    if (in.opt_persist_edges > e) e = in.opt_persist_edges;
    if (e > LP_EMAX || e > n / 4) return false;
    const size_t nl = (size_t)((n + 7) & ~7);
    const size_t lds = (size_t)(e + 1) * nl * 2 + nl * 4 + std::max<size_t>(nl * 2, 256) + (tabu ? nl * 2 : 0);   // (+ the nodes' ages)
    if (lds > in.lds_max) return false;
    const int W = (n + e - 1) / e;
    if (!(W <= in.cus && W <= 256)) return false;        // (the exchange keeps two candidate sets of 4 polling waves: 256 slots)
    r = Resident{Form::ROWS, e, W, 0, 0, lds};
    return true;
}

// The half-window form (k_lds2opt_w): every row kept as the window of E + n/2 + 16.. cells ahead of the workgroup's first own
// cell, so that instances a little past n = 4096 (fnl4461, BASELINE config 3) stay LDS-resident.  Plain 2-opt only.
inline bool window_fits(const In &in, bool tabu, Resident &r)
{
    const int n = in.n;
    if (in.elem != ELEM_U16 || in.otf || !in.symmetric || !in.has_matrix || n < 64 || n > 8191) return false;
    int e = (n + std::min(in.cus, 256) - 1) / std::min(in.cus, 256);
    if (in.opt_persist_edges > e) e = in.opt_persist_edges;
    if (e > LW_EMAX) return false;
    const int ws = (e + n / 2 + 23) & ~7;             // window cells per row (see k_lds2opt_w)
    if (ws > n || (ws >> 3) - 1 > LW_BT) return false;
    const size_t nl = (size_t)((n + 7) & ~7);
    if ((nl >> 3) > (size_t)LW_BT) return false;
    const size_t fixed = (size_t)(e + 1) * ws * 2 + (nl + 8) * 4 + 512 + (tabu ? (nl + 16) * 2 : 0);   // (+ the nodes' ages)
    int ns = 2;
    if (fixed + 2 * nl * 2 > in.lds_max) ns = 1;
    if (fixed + (size_t)ns * nl * 2 > in.lds_max) return false;
    const int W = (n + e - 1) / e;
    if (!(W <= in.cus && W <= 256)) return false;
    r = Resident{Form::WINDOW, e, W, ws, ns, fixed + (size_t)ns * nl * 2};
    return true;
}

// which form runs (tabu: the walk's, with the nodes' ages in LDS).  opt_persist_window: 0 half-window rows where whole rows do
// not fit, 1 half-window rows wherever they fit, 2 never.  run_persist, the streamed descent's "neither applies" in run_sweeps
// and tspgpu_info 16-19 all ask this
inline Resident resident(const In &in, bool tabu)
{
    Resident r;
    if (in.opt_persist_window == 1 && window_fits(in, tabu, r)) return r;
    if (rows_fit(in, tabu, r)) return r;
    if (in.opt_persist_window != 2) window_fits(in, tabu, r);
    return r;
}

// The streamed persistent descent (k_str2opt) where it applies: uint16 cells, one tour, a symmetric matrix too large for the
// LDS-resident kernels, four rows + the node-per-cell array in one workgroup's LDS, a whole idle chip.
struct Stream { bool fits = false; int P = 0, W = 0, BT = 0, NCH = 0; size_t lds = 0; };
inline Stream stream(const In &in)
{
    Stream s;
    const int n = in.n, ld = in.ld;
    if (in.elem != ELEM_U16 || in.otf || !in.symmetric || !in.has_matrix || n < 1024 || n >= 16384) return s;
    const int cus = std::min(in.cus, 256);
    s.P = (n + cus - 1) / cus;
    s.W = (n + s.P - 1) / s.P;
    s.NCH = ld / 8 <= 1024 ? 1 : 2;
    if (in.opt_sp_nch > 0) s.NCH = in.opt_sp_nch;    // undocumented (option 93): force one / two 16-byte vectors per thread
    s.BT = std::max(256, ((ld / 8 + s.NCH - 1) / s.NCH + 63) & ~63);     // (at least the 256 lanes that poll the exchange slots)
    if (s.BT > 1024 || s.P < 2 || s.P > 64) return s;
    s.lds = sp_lds_rows(ld) + sp_lds_ord(n) + sp_lds_nodes(s.P) + SP_LDS_SCRATCH;
    s.lds = std::max<size_t>(s.lds, 84 * 1024);           // more than half a CU's LDS: one workgroup per CU, every CU one
    s.fits = s.lds <= in.lds_max && s.W <= 256;
    return s;
}

// ---- the candidate sweeps (Or-opt, parallel-move 2-opt) ---------------------------------------------------------------------
// geometry of a candidate sweep: threads, 16-byte vectors per thread and row, tour positions per workgroup, workgroups, the
// workgroups a CU holds, dynamic LDS bytes, and the kernel (the caller's to fill in)
struct SweepGeom { int BT, NCH, R, W, occ; size_t lds; const void *fn; };

// ... for a kernel that keeps `rows` matrix rows and `extra` more bytes in LDS: R is one wave of workgroups over the chip,
// clamped to [rmin, rmax]; NCH is the first of `nchs` (ascending) that covers a row.  Matrix-free mode: BT = 256, NCH = 0,
// R = otf_run, no dynamic LDS
inline SweepGeom sweep_geom(const In &in, int rows, size_t extra, int rmin, int rmax, std::initializer_list<int> nchs, int otf_run)
{
    SweepGeom P{};
    const int n = in.n;
    if (in.otf) {
        P.BT = 256; P.R = otf_run; P.W = (n + P.R - 1) / P.R;
        return P;
    }
    const size_t esz = elem_size(in.elem);
    const int nvec = in.ld / (int)(16 / esz);
    P.BT = nvec <= 256 ? 256 : nvec <= 1024 ? 512 : 1024;
    for (int c : nchs) { P.NCH = c; if (c * P.BT >= nvec) break; }
    P.lds = rows * (size_t)in.ld * esz + extra;
    P.occ = (int)std::max<size_t>(1, std::min<size_t>(in.lds_max / P.lds, (size_t)(2048 / P.BT)));
    const int target = in.cus * P.occ;
    P.R = std::min(std::max((n + target - 1) / target, rmin), rmax);
    P.W = (n + P.R - 1) / P.R;
    return P;
}
} // namespace plan
