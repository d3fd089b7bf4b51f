// ---------------------------------------------------------------------------
// k_lds2opt_w: the LDS-resident descent (tspgpu_lds2opt.inc) for instances whose uint16 matrix does NOT fit the chip's LDS:
// 4096 < n <= ~5400 (BASELINE config 3: fnl4461, n = 4461, 39.8 MB).  ref_2opt / ref_2opt_once / ref_reverse_path,
// src/algorithms/refinment.c:3-37, :39-93, :95-114.  Included by tspgpu.hip behind tspgpu_lds2opt.inc.
//
// A pair of tour edges {k, m} has two owners and is evaluated by the owner of k when m lies at most n/2 array cells AHEAD
// of k -- so a workgroup never reads the other half of its rows.  Here it does not keep it either:
//
//   * workgroup g (one per CU, 768 threads) owns the E = ceil(n / CUs) tour edges at array cells [k0, k0+E) and keeps, of
//     the E+1 matrix rows of their end nodes (in tour order: G_x[q] = c[x][ord q]), only the WINDOW of Ws cells that starts
//     at c_lo = k0 rounded down to 8:  local column j  <->  array cell (c_lo + j) mod n,  Ws = 8-aligned E + n/2 + 18.
//     (E+1) * Ws * 2 bytes: 86 KB at n = 4461 instead of 170.  Every stored column holds valid data (pairs a window holds
//     beyond the n/2 cells ahead are pairs the other owner sees too: same key), so the inner loop carries no mask.
//   * evaluation: 8-cell column chunks x groups of own edges: thread (g, c) takes chunk c against the edges of group g
//     (2 groups of 9 edges at n = 4461), delta(k, m) = G_k[m] + G_{k+1}[m+1] - w[k] - w[m] from two consecutive LDS
//     reads as in k_lds2opt (poisoned diagonal, packed 16-bit arithmetic where every cost <= 16383).
//   * one grid-wide exchange per sweep (the same tagged 16-byte slot records; labels and cells are 13-bit fields here).
//   * the move reverses the array range R = [lo, lo+M), M <= n/2.  In window coordinates a range that lies inside the
//     window is a plain sub-range (no wrap-around): reversed in place, row by row.  A range that lies outside touches
//     nothing.  A range that crosses a window end: with a cells inside the window and b outside, a - b inside cells
//     mirror among themselves (reversed in place), the other min(a, b) are re-read from the matrix by their new labels,
//     c[x][ord q] -- one gather round trip, only in the workgroups whose window end the range crosses; more than LW_FIX
//     such cells per row reload the rows whole.
//     Rows whose own cell lies inside R change node: swapped with their mirror row or reloaded, as in k_lds2opt.
//   * a whole row is (re)loaded coalesced in node order into a staging row and gathered into the window by the labels.
// ---------------------------------------------------------------------------
using plan::LW_EMAX;      // tour edges per workgroup at most, threads (tspgpu_plan.h: 768 threads, 170 registers each)
using plan::LW_BT;
static constexpr int LW_RB = 10, LW_FIX = 128;   // (ten rows in flight)
typedef v4u32 v4u32_a4 __attribute__((aligned(4)));       // 16 bytes of LDS at a 4-byte boundary
static constexpr u64 LW_NONE = 0x3FFFFull << 26;         // "no improving pair": delta field (18 bits) all ones, labels 0

// TABU: tabu_best_move instead of ref_2opt_once (metaheuristic.c:188-245), as in k_lds2opt<., true>: the nodes' ages by array
// cell in LDS (the half windows leave room for them at every n this kernel takes: the tabu walk at n = 4096 .. 5400 stays
// LDS-resident), the cells of a row's own node and of its two tour neighbours poisoned and kept so by four two-cell
// patches per move, linear tenure policy, incumbent and cost trace in the kernel.
template <bool PK16, bool TABU, bool VNS = false>
__global__ void __launch_bounds__(LW_BT) k_lds2opt_w(PersistArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int BT = LW_BT;
    constexpr unsigned POISON = PK16 ? 16383u : 65535u;     // on the diagonal: delta(k, k) = 2 POISON - 2 w[k] >= 0
    const int n = A.n, nl = A.nl, ld = A.ld, E = A.E, Ws = A.Ws, W = (int)gridDim.x, wg = (int)blockIdx.x, tid = (int)threadIdx.x, t = A.slot;
    const size_t tn = (size_t)t * n;
    // LDS: E+1 window rows of Ws cells | wt: nl + 8 words (w | label << 16), by ARRAY CELL, cells n .. n+7 a copy of cells
    // 0 .. 7 (the 8 cells of a window chunk are consecutive entries wherever the chunk starts) | 1 or 2 staging rows | scratch
    u16 *rows = reinterpret_cast<u16 *>(smem);
    u16 *wt16 = reinterpret_cast<u16 *>(smem + (size_t)(E + 1) * Ws * 2);      // [2q] = w[q], [2q+1] = ord[q]
    unsigned *wt = reinterpret_cast<unsigned *>(wt16);
    u16 *stage = reinterpret_cast<u16 *>(smem + (size_t)(E + 1) * Ws * 2 + (size_t)(nl + 8) * 4);
    u64 *scr = reinterpret_cast<u64 *>(smem + (size_t)(E + 1) * Ws * 2 + (size_t)(nl + 8) * 4 + (size_t)A.nstage * nl * 2);
    int *scr32 = reinterpret_cast<int *>(scr);         // [0] workgroup key, [2..17] exchange candidates, ints [40..55] wave minima
    u16 *age16 = reinterpret_cast<u16 *>(scr + 64);    // TABU: iterations since the node at the cell was moved (0xFFFF: never), cells n .. n+8
                                                       // a copy of cells 0 .. 8
    constexpr int DINF = 0x7fffffff;
    const int k0 = min(wg * E, n - E);                 // own edges: array cells k0 .. k0+E-1; own rows: cells k0 .. k0+E
    const int c_lo = k0 & ~7, a0 = k0 - c_lo;          // the window starts at cell c_lo; local column of the first own cell
    const int NC = (Ws >> 3) - 1;                      // column chunks evaluated (the last stored chunk only lends its first cell)
    auto cell_of = [&](int j) __attribute__((always_inline)) { int q = c_lo + j; return q >= n ? q - n : q; };   // (Ws <= n)

    auto give_up = [&](int status) __attribute__((always_inline)) {
        if (tid == 0) {
            atomicCAS(A.ctl + 1, LP_ST_RUNNING, status);
            __hip_atomic_store(A.ctl, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    // the grid-wide exchange of k_lds2opt (see there)
    auto exchange = [&](int s, bool have, u64 w0, u64 w1, u64 &r0, u64 &r1, long limit) __attribute__((always_inline)) {
        u64 *buf = A.slots + (size_t)(s & 1) * W * 8;
        const u64 tag = (u64)((s % 15) + 1) << 60;
        if (have) lp_st128(buf + (size_t)wg * 8, tag | w0, tag | w1);
        u64 a = LP_KEYMASK, b = 0;
        if (tid < W) {
            const long tp = wall_clock64();
            for (int spins = 0;;) {
                lp_ld128(buf + (size_t)tid * 8, a, b);
                if ((a >> 60) == (tag >> 60) && (b >> 60) == (tag >> 60)) { a &= LP_KEYMASK; break; }
                for (int z = 0; z < A.poll_sleep; z++) __builtin_amdgcn_s_sleep(1);     // (probe hook 95: 64 cycles each between polls)
                if ((++spins & 7) == 0 &&
                    (wall_clock64() - tp > limit || __hip_atomic_load(A.ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) { a = 0; break; }
            }
        }
        const long long wm = wave_min_i64((long long)a);
        const int wv = tid >> 6, nwp = (W + 63) >> 6;         // (W <= 256: at most 4 polling waves)
        u64 *cand = scr + 2 + (s & 1) * 8;
        if (wv < nwp && (long long)a == wm) { cand[2 * wv] = a; cand[2 * wv + 1] = b; }
        __syncthreads();
        u64 x0 = cand[0], x1 = cand[1];
        for (int i = 1; i < nwp; i++) { const u64 y = cand[2 * i]; if (y < x0) { x0 = y; x1 = cand[2 * i + 1]; } }
        r0 = ((u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(x0 >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)x0);
        r1 = ((u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(x1 >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)x1);
    };

    // ---- rendezvous: is the whole grid resident?
    u64 r0, r1;
    exchange(0, tid == 0 && (A.hello_ticks > 0 || wg != 0), 1ull << 26, 0, r0, r1, A.hello_ticks > 0 ? A.hello_ticks : -A.hello_ticks);
    if (r0 == 0) { give_up(LP_ST_NO_RENDEZVOUS); return; }

    int dir = A.S.dir[t];
    const int cap = A.S.cap_sweeps[t];
    int kd = A.S.nsweeps[t];                          // sweeps completed (this call)
    int sdone = 0;                                    // ... by this launch
    long long sumd = 0;
    int lastd = 0;
    double cost0 = A.S.cost[t];

    {   // wt from the tour state
        const int *ord = A.S.ord + tn;
        const int *dp = reinterpret_cast<const int *>(A.S.dpos + tn);
        for (int q = tid; q < n + 8; q += BT) {
            const int src = q < n ? q : q - n;
            wt[q] = ((unsigned)dp[src] & 0xffffu) | ((unsigned)ord[src] << 16);
        }
        if constexpr (TABU) for (int q = tid; q < n + 16; q += BT) age16[q] = 0xFFFFu;     // tabu_init (metaheuristic.c:65-84)
    }
    __syncthreads();

    // (re)load the window rows in `need` (bit r = own cell k0 + r): the rows are requested LW_RB at a time (coalesced, node
    // order), each is written to a staging row and gathered into the window by the labels of the window's cells.  With two
    // staging rows one barrier per row, with one (n close to the limit) two.
    auto reload = [&](unsigned need) __attribute__((always_inline)) {
        const int lane = tid & 63;
        int oc = k0 + min(lane, E); if (oc >= n) oc -= n;
        const unsigned ownlab = wt16[2 * oc + 1];                  // lane r: the node at the own cell r
        const bool gact = tid < (Ws >> 3), lact = tid < (nl >> 3);
        unsigned offs[4];                                          // byte offsets of this thread's window cells in a node-order row, two a word
        if (gact) {
            const unsigned *wq = wt + cell_of(tid * 8);
            const v4u32 la = *reinterpret_cast<const v4u32_a4 *>(wq), lb = *reinterpret_cast<const v4u32_a4 *>(wq + 4);
            offs[0] = (la.x >> 16 << 1) | (la.y >> 16 << 17); offs[1] = (la.z >> 16 << 1) | (la.w >> 16 << 17);
            offs[2] = (lb.x >> 16 << 1) | (lb.y >> 16 << 17); offs[3] = (lb.z >> 16 << 1) | (lb.w >> 16 << 17);
        }
        auto gather = [&](const unsigned char *buf, int rdst) __attribute__((always_inline)) {
            if (gact) {
                unsigned g[8];
#pragma unroll
                for (int v = 0; v < 8; v++) g[v] = *reinterpret_cast<const u16 *>(buf + ((v & 1) ? offs[v >> 1] >> 16 : offs[v >> 1] & 0xffffu));
                const v4u32 out = {g[0] | g[1] << 16, g[2] | g[3] << 16, g[4] | g[5] << 16, g[6] | g[7] << 16};
                *reinterpret_cast<v4u32 *>(rows + (size_t)rdst * Ws + tid * 8) = out;
            }
        };
        const bool two = A.nstage == 2;
        unsigned char *bprev = nullptr;
        int rprev = 0, cnt = 0;
        unsigned rem = need;
        // a rolling window of LW_RB rows in flight: a row's register is refilled with the request for the row LW_RB further
        // down as soon as it has been written to its staging row, so only the first request's latency is exposed
        v4u32 R[LW_RB];
        int rr[LW_RB];
#pragma unroll
        for (int b = 0; b < LW_RB; b++) {
            rr[b] = -1;
            if (rem) {
                rr[b] = __builtin_ctz(rem); rem &= rem - 1;
                const int x = __builtin_amdgcn_readlane((int)ownlab, rr[b]);
                if (lact) R[b] = *reinterpret_cast<const v4u32 *>(A.mat + (size_t)x * ld + tid * 8);
            }
        }
#pragma unroll
        for (int i = 0; i <= LW_EMAX; i++) {
            const int b = i % LW_RB;
            if (rr[b] >= 0) {
                const int r = rr[b];
                const unsigned x = (unsigned)__builtin_amdgcn_readlane((int)ownlab, r);
                unsigned char *buf = reinterpret_cast<unsigned char *>(stage + (two ? (size_t)(cnt & 1) * nl : 0));
                cnt++;
                if (lact) {
                    v4u32 v = R[b];
                    if ((int)(x >> 3) == tid) {                // the diagonal cell: poisoned (delta(k, k) can never win)
                        const unsigned sel = (x & 7u) >> 1;
                        unsigned c[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                        for (int q = 0; q < 4; q++)
                            if ((unsigned)q == sel) c[q] = (x & 1u) ? (c[q] & 0xffffu) | (POISON << 16) : (c[q] & 0xffff0000u) | POISON;
                        v = v4u32{c[0], c[1], c[2], c[3]};
                    }
                    *reinterpret_cast<v4u32 *>(buf + (size_t)tid * 16) = v;
                }
                rr[b] = -1;
                if (rem) {                                     // refill the slot
                    rr[b] = __builtin_ctz(rem); rem &= rem - 1;
                    const int xn = __builtin_amdgcn_readlane((int)ownlab, rr[b]);
                    if (lact) R[b] = *reinterpret_cast<const v4u32 *>(A.mat + (size_t)xn * ld + tid * 8);
                }
                if (two) {
                    if (bprev) gather(bprev, rprev);
                    __syncthreads();
                    bprev = buf; rprev = r;
                } else {
                    __syncthreads();
                    gather(buf, r);
                    __syncthreads();
                }
            }
        }
        if (two) { if (bprev) gather(bprev, rprev); __syncthreads(); }
        if constexpr (TABU) {                         // the cells of the node's two tour neighbours (the own cell came poisoned)
            if (tid <= E && ((need >> tid) & 1)) {
                u16 *row = rows + (size_t)tid * Ws + a0 + tid;      // (the own cell r sits at the local column a0 + r)
                if (a0 + tid > 0) row[-1] = (u16)POISON;
                row[1] = (u16)POISON;
            }
            __syncthreads();
        }
    };
    const unsigned allrows = (2u << E) - 1u;
    reload(allrows);

    int status = LP_ST_RUNNING;
    if (cap >= 0 && kd >= cap) status = LP_ST_CAPPED;        // (cap 0: not one sweep)
    // VNS: the incumbent's cost, iteration counter, numbers consumed, and the loop body behind a local optimum
    double best = A.best0;
    int vit = A.vns_it0, vcur = 0;
    u16 *vns_lab = rows;                              // (rows 0 and 1, 2 Ws >= n cells: loaded again behind the kicks)
    auto vns_mirror = [&]() __attribute__((always_inline)) { if (tid < 8) wt[n + tid] = wt[tid]; };
#include "tspgpu_lds_vns.inc"
    if constexpr (VNS) {
        if (A.vns_phase == 1 && status == LP_ST_RUNNING) {
            const int st = vns_step(false);
            if (st != LP_ST_RUNNING) status = st;
        }
    }
    int tenure = A.tenure0, tup = A.up0, iters = 0;  // TABU
    if (TABU && A.tabu_k <= 0) status = LP_ST_CAPPED;
    auto tabu_edge = [&](int q) __attribute__((always_inline)) {      // one of the two nodes of the edge at cell q is tabu
        int q1 = q + 1; if (q1 >= n) q1 -= n;
        return (int)age16[q] < tenure || (int)age16[q1] < tenure;    // is_tabu, metaheuristic.c:416-418 (age = iter - tabu_list[node])
    };
    // phase clocks (TSPGPU_OPT_STAMPS): thread 0 of every workgroup sums wall-clock ticks per phase
    // (the sums live in LDS, not in registers)
    const bool clk = A.stamps != nullptr && tid == 0;
    unsigned long long *ph = scr + 32;                 // [0..5] phases, [6] reloads, [7] rows reloaded, [8] gather fix-ups
    if (clk) for (int i = 0; i < 9; i++) ph[i] = 0;
    unsigned long long tc = clk ? wall_clock64() : 0ull;
#define LW_PHASE(i) do { if (clk) { const unsigned long long now_ = wall_clock64(); ph[i] += now_ - tc; tc = now_; } } while (0)
    // Evaluation geometry (the same every sweep): as many groups of own edges as the threads allow, thread (g, ch) takes the
    // column chunk ch against the edges of group g.
    int ng = min(BT / NC, E);
    const int rpg = (E + ng - 1) / ng;                 // edges per group
    ng = (E + rpg - 1) / rpg;
    const int grp = tid / NC, ch = tid - grp * NC;
    const bool eact = grp < ng;
    const int rlo = eact ? grp * rpg : 0, rcnt = eact ? min(rpg, E - rlo) : 0;
    const int me0 = ch * 8;                            // first local column of the chunk
    const u16 *rchunk = rows + (size_t)rlo * Ws + me0; // this thread's 8 cells of its first row
    const u16 *rex = rchunk + 8;                       // ... and the cell behind them
    const unsigned *wq0 = wt + cell_of(me0);           // the chunk's 8 cells in wt (consecutive thanks to the copy behind cell n-1)
    const u16 *aq0 = age16 + cell_of(me0);             // ... and their ages (+ the cell behind them)
    while (status == LP_ST_RUNNING) {
        // ---- evaluation: for each of the 8 own columns the minimum over the thread's own edges of G_k[m] + G_{k+1}[m+1] - w[k]
        int col[8];
        int tmin = 0x7fffffff;
        unsigned etmask = 0;                          // TABU: bit r = the own edge k0 + r has a tabu node
        if constexpr (TABU) {
            const int r = tid & 63;
            etmask = (unsigned)__ballot(r < E && tabu_edge(k0 + min(r, E - 1)));
        }
        if (eact) {
            unsigned acc[4] = {0x7fff7fffu, 0x7fff7fffu, 0x7fff7fffu, 0x7fff7fffu};
#pragma unroll
            for (int v = 0; v < 8; v++) col[v] = 0x7fffffff;
            v4u32 X = *reinterpret_cast<const v4u32 *>(rchunk);
            v4u32 Xn = *reinterpret_cast<const v4u32 *>(rchunk + Ws);
            unsigned exn = rex[Ws];
            unsigned wk = wt16[2 * (k0 + rlo)];
            for (int r = 0; r < rcnt; r++) {
                const v4u32 Xc = Xn;
                const unsigned exc = exn, wkc = wk;
                const int rn = min(r + 2, rcnt);
                Xn = *reinterpret_cast<const v4u32 *>(rchunk + (size_t)rn * Ws);
                exn = rex[(size_t)rn * Ws];
                wk = wt16[2 * (k0 + rlo + min(r + 1, rcnt - 1))];
                const unsigned Y[4] = {__builtin_amdgcn_alignbit(Xc.y, Xc.x, 16), __builtin_amdgcn_alignbit(Xc.z, Xc.y, 16),
                                       __builtin_amdgcn_alignbit(Xc.w, Xc.z, 16), (Xc.w >> 16) | (exc << 16)};
                const unsigned Xa[4] = {X.x, X.y, X.z, X.w};
                if (!TABU || !((etmask >> (rlo + r)) & 1)) {
                    if constexpr (PK16) {
                        const unsigned wk2 = wkc | (wkc << 16);
#pragma unroll
                        for (int j = 0; j < 4; j++) acc[j] = lp_pk_min(acc[j], lp_pk_sub(lp_pk_add(Xa[j], Y[j]), wk2));
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            int d0 = (int)(Xa[j] & 0xffffu) + (int)(Y[j] & 0xffffu) - (int)wkc;
                            int d1 = (int)(Xa[j] >> 16) + (int)(Y[j] >> 16) - (int)wkc;
                            if constexpr (TABU) {           // a poisoned cell: a pair of adjacent edges
                                if ((Xa[j] & 0xffffu) == POISON) d0 = DINF;
                                if ((Xa[j] >> 16) == POISON) d1 = DINF;
                            }
                            col[2 * j] = min(col[2 * j], d0); col[2 * j + 1] = min(col[2 * j + 1], d1);
                        }
                    }
                }
                X = Xc;
            }
            const v4u32 wa = *reinterpret_cast<const v4u32_a4 *>(wq0), wb = *reinterpret_cast<const v4u32_a4 *>(wq0 + 4);
            const unsigned wm[8] = {wa.x & 0xffffu, wa.y & 0xffffu, wa.z & 0xffffu, wa.w & 0xffffu,
                                    wb.x & 0xffffu, wb.y & 0xffffu, wb.z & 0xffffu, wb.w & 0xffffu};
            unsigned tabm = 0;                        // TABU: bit v = the edge at the chunk's cell v has a tabu node
            if constexpr (TABU) {
                const v4u32 ag = *reinterpret_cast<const v4u32_a2 *>(aq0);
                const unsigned agx = aq0[8];
                const unsigned a9[9] = {ag.x & 0xffffu, ag.x >> 16, ag.y & 0xffffu, ag.y >> 16, ag.z & 0xffffu, ag.z >> 16,
                                        ag.w & 0xffffu, ag.w >> 16, agx};
#pragma unroll
                for (int v = 0; v < 8; v++) tabm |= (((int)a9[v] < tenure || (int)a9[v + 1] < tenure) ? 1u : 0u) << v;
            }
#pragma unroll
            for (int v = 0; v < 8; v++) {
                if constexpr (PK16) col[v] = (v & 1) ? ((int)acc[v >> 1] >> 16) : (int)(short)(acc[v >> 1] & 0xffffu);
                if constexpr (TABU) {
                    if (col[v] < DINF) col[v] -= (int)wm[v];
                    // PK16: nothing found (0x7fff), or a pair of adjacent edges (2 * 16383 - 2 costs > 16383 > any valid delta)
                    if (PK16 && col[v] > 16383) col[v] = DINF;
                    if ((tabm >> v) & 1) col[v] = DINF;
                } else col[v] -= (int)wm[v];
                tmin = min(tmin, col[v]);
            }
        }
        LW_PHASE(0);                                  // evaluation
        const int wmin = wave_min_i32(tmin);
        if ((tid & 63) == 0) scr32[40 + (tid >> 6)] = wmin;
        if (tid == 0) scr[0] = ~0ull;
        __syncthreads();
        int dmin = scr32[40];
#pragma unroll
        for (int i = 1; i < BT / 64; i++) dmin = min(dmin, scr32[40 + i]);
        dmin = __builtin_amdgcn_readfirstlane(dmin);
        // ---- the workgroup's best pair in the reference's order: smallest delta, then smallest a, then smallest b.
        // The wave that holds a column with the minimum resolves it together: lane r takes the r-th edge of the column's thread.
        u64 mykey = ~0ull, mypay = 0;
        const bool found = TABU ? dmin < DINF : dmin < 0;      // (tabu_best_move takes the best admissible pair whatever its sign)
        if (found) {
            unsigned cm = 0;
            if (eact && tmin == dmin) {
#pragma unroll
                for (int v = 0; v < 8; v++) cm |= (col[v] == dmin ? 1u : 0u) << v;
            }
            unsigned long long ball = __ballot(cm != 0);
            const int lane = tid & 63;
            while (ball) {
                const int src = __builtin_ctzll(ball);
                ball &= ball - 1;
                unsigned cms = (unsigned)__builtin_amdgcn_readlane((int)cm, src);
                const int m0s = __builtin_amdgcn_readlane(me0, src);
                const int rlos = __builtin_amdgcn_readlane(rlo, src), rcnts = __builtin_amdgcn_readlane(rcnt, src);
                while (cms) {
                    const int v = __builtin_ctz(cms);
                    cms &= cms - 1;
                    const int ml = m0s + v, m = cell_of(ml);
                    if (lane < rcnts) {
                        const int r = rlos + lane;
                        int k = k0 + r; if (k >= n) k -= n;
                        const unsigned xa = rows[(size_t)r * Ws + ml], yb = rows[(size_t)(r + 1) * Ws + ml + 1];
                        const int d = (int)xa + (int)yb - (int)wt16[2 * k] - (int)wt16[2 * m];
                        bool ok = d == dmin;
                        if constexpr (TABU) ok = ok && xa != POISON && !((etmask >> r) & 1);
                        if (ok) {
                            const int kp = k + 1 == n ? 0 : k + 1, mp = m + 1 == n ? 0 : m + 1;
                            const unsigned lk = dir > 0 ? wt16[2 * k + 1] : wt16[2 * kp + 1];
                            const unsigned lm = dir > 0 ? wt16[2 * m + 1] : wt16[2 * mp + 1];
                            const unsigned la = min(lk, lm), lb = max(lk, lm);
                            const u64 key = ((u64)(unsigned)(dmin + LP_DBIAS) << 26) | ((u64)la << 13) | lb;
                            if (key < mykey) {
                                mykey = key;
                                const unsigned e1 = (unsigned)min(k, m), e2 = (unsigned)max(k, m);
                                const unsigned l1 = k < m ? lk : lm;          // label of the edge at the smaller cell
                                mypay = ((u64)(l1 == la ? 1u : 0u) << 58) | ((u64)e1 << 45) | ((u64)e2 << 32) | ((u64)xa << 16) | yb;
                            }
                        }
                    }
                }
            }
            if (mykey != ~0ull) __hip_atomic_fetch_min(&scr[0], mykey, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        __syncthreads();
        const u64 kmin = scr[0];
        const bool have = found ? mykey == kmin : tid == 0;
        LW_PHASE(1);                                  // workgroup reduction + tie order
        // ---- exchange
        sdone++;
        exchange(sdone, have, found ? mykey : LW_NONE, mypay, r0, r1, A.spin_ticks);
        if (r0 == 0) { give_up(LP_ST_LOST); return; }
        LW_PHASE(2);                                  // exchange
        kd++;
        const bool nomove = (r0 >> 26) == 0x3FFFFull;
        if (nomove && !TABU) {                        // the final, non-improving sweep
            lastd = 0;
            if (wg == 0 && tid == 0 && t == 0 && kd <= A.hist.cap) { A.hist.a[kd - 1] = -1; A.hist.b[kd - 1] = -1; A.hist.d[kd - 1] = 0.0; }
            if constexpr (!VNS) { status = LP_ST_OPTIMUM; break; }
            else {
                // mh_VNS: incumbent, trace, kicks; then the next iteration's local search
                const int st = vns_step(true);
                if (st != LP_ST_RUNNING) { status = st; break; }
                if (A.budget >= 0 && sdone >= A.budget) { status = LP_ST_BUDGET; break; }
                continue;
            }
        }
        if (!nomove) {                                // (TABU: an iteration in which every pair is tabu moves nothing)
        const int d = (int)((r0 >> 26) & 0x3FFFFu) - LP_DBIAS;
        const int la = (int)((r0 >> 13) & 0x1fffu), lb = (int)(r0 & 0x1fffu);
        const int e1 = (int)((r1 >> 45) & 0x1fffu), e2 = (int)((r1 >> 32) & 0x1fffu);
        const unsigned wTT = (unsigned)((r1 >> 16) & 0xffffu), wHH = (unsigned)(r1 & 0xffffu);
        const bool e1_is_a = (r1 >> 58) & 1;
        sumd += d; lastd = d;
        if (wg == 0 && tid == 0 && t == 0 && kd <= A.hist.cap) { A.hist.a[kd - 1] = la; A.hist.b[kd - 1] = lb; A.hist.d[kd - 1] = (double)d; }

        // ---- the move as an array operation (see Tours): ref_reverse_path flips the arc succ a .. b; flipping the other
        // arc and toggling dir gives the same successor function, so the shorter arc [lo, lo+M) is reversed
        const int ea = e1_is_a ? e1 : e2, eb = e1_is_a ? e2 : e1;
        const int s1 = dir > 0 ? ea : eb, s2 = dir > 0 ? eb : ea;
        int L = s2 - s1; if (L < 0) L += n;
        const bool other = n - L < L;
        const int M = other ? n - L : L;
        int lo = (other ? s2 : s1) + 1; if (lo == n) lo = 0;
        if (other) dir = -dir;
        int eTT = lo - 1; if (eTT < 0) eTT += n;          // the edge in front of the range joins the two tails,
        int eHH = lo + M - 1; if (eHH >= n) eHH -= n;     // the edge at its last cell the two heads
        const int hs = M >> 1, hw = (M - 1) >> 1;
        unsigned wOldTT = 0, wOldHH = 0;              // TABU: the costs of the two edges the move removes (for the poison patches)
        if constexpr (TABU) {
            wOldTT = wt16[2 * eTT]; wOldHH = wt16[2 * eHH];
            __syncthreads();                          // (read by every wave before the last thread writes the new costs)
        }
        // own cells inside the range hold other nodes afterwards: a row whose node stays among the own cells changes places
        // with its mirror row, the others are fetched.  Lane r looks at the own cell r (every wave computes the same words).
        unsigned need = 0, swp = 0;                   // swp bit r: row r changes places with the row mirv (lane r) above it
        int mirv = 0;
        {
            int off = k0 - lo; if (off < 0) off += n;
            if (off < M || off + E >= n) {
                const int r = tid & 63;
                bool nd = false, sw = false;
                if (r <= E) {
                    int rel = off + r; if (rel >= n) rel -= n;
                    if (rel < M) {
                        int pm = lo + (M - 1 - rel); if (pm >= n) pm -= n;
                        int rm = pm - k0; if (rm < 0) rm += n;
                        nd = rm > E; sw = !nd && rm > r; mirv = rm;
                    }
                }
                need = (unsigned)__ballot(nd); swp = (unsigned)__ballot(sw);
            }
        }
        // The range in window coordinates: inside (a plain sub-range: reversed in place), outside (nothing), or across a
        // window end.  Across the far end the window holds the first a1 cells of the range, across the near end (the range
        // re-enters at column 0) its last a2.  With a cells inside and b = M - a outside, the mirror of an inside cell is inside
        // too unless it is one of the b cells nearest the crossing end of the RANGE: the other a - b cells (if any) mirror
        // among themselves -- reversed in place --, those b cells (all a when a <= b) are re-read by their new labels.
        int jl = lo - c_lo; if (jl < 0) jl += n;
        const bool inside = jl + M <= Ws;
        const int a1 = inside || jl >= Ws ? 0 : Ws - jl;
        const int a2 = jl + M > n ? jl + M - n : 0;
        int rjl = jl, rM = inside ? M : 0;            // reversed in place: local columns rjl .. rjl + rM - 1
        int fjl = 0, fcnt = 0;                        // re-read: local columns fjl .. fjl + fcnt - 1
        if (a1 && a2) { need = allrows; swp = 0; }    // (both ends at once: M within a few cells of n/2)
        else if (a1) { const int b = M - a1; fjl = jl; if (a1 > b) { rjl = jl + b; rM = a1 - b; fcnt = b; } else fcnt = a1; }
        else if (a2) { const int b = M - a2; if (a2 > b) { rjl = 0; rM = a2 - b; fjl = a2 - b; fcnt = b; } else fcnt = a2; }
        if (fcnt > LW_FIX) { need = allrows; swp = 0; }    // a long crossing: every row whole
        const int rhs = rM >> 1;
        if (rM >= 2 && rM <= 16) {
            // a short range (7 of 10 moves): 8 lanes a row
            const int item = tid >> 3, u = tid & 7;
            if (item <= E && !((need >> item) & 1) && u < rhs) {
                u16 *base = rows + (size_t)item * Ws + rjl;
                const u16 x = base[u], y = base[rM - 1 - u];
                base[u] = y; base[rM - 1 - u] = x;
            }
        } else if (rM > 16) {
            // 8 cells from either end of the range per item (16-byte LDS accesses at 2-byte alignment), reversed in registers;
            // 2^lgi threads per row, two rows in flight; the up to 7 swaps per row left in the middle cell by cell
            const int I = rhs >> 3;
            {
                int lgi = 0;
                while ((1 << lgi) < I && lgi < 8) lgi++;          // (I <= 255: n < 8192; 768 >> lgi stays exact)
                const int rpi = BT >> lgi, j0 = tid & ((1 << lgi) - 1), rs0 = tid >> lgi;
                const int a = rjl + 8 * j0, b = rjl + rM - 8 * j0 - 8;
                for (int row0 = 0; row0 <= E; row0 += 2 * rpi) {
                    v4u32 va[2], vb[2];
                    bool ok[2];
#pragma unroll
                    for (int q = 0; q < 2; q++) {
                        const int row = row0 + q * rpi + rs0;
                        ok[q] = row <= E && j0 < I && !((need >> row) & 1);
                        if (ok[q]) {
                            va[q] = *reinterpret_cast<const v4u32_a2 *>(rows + (size_t)row * Ws + a);
                            vb[q] = *reinterpret_cast<const v4u32_a2 *>(rows + (size_t)row * Ws + b);
                        }
                    }
#pragma unroll
                    for (int q = 0; q < 2; q++) {
                        const int row = row0 + q * rpi + rs0;
                        if (ok[q]) {
                            const v4u32 ra = {__builtin_amdgcn_alignbit(vb[q].w, vb[q].w, 16), __builtin_amdgcn_alignbit(vb[q].z, vb[q].z, 16),
                                              __builtin_amdgcn_alignbit(vb[q].y, vb[q].y, 16), __builtin_amdgcn_alignbit(vb[q].x, vb[q].x, 16)};
                            const v4u32 rb = {__builtin_amdgcn_alignbit(va[q].w, va[q].w, 16), __builtin_amdgcn_alignbit(va[q].z, va[q].z, 16),
                                              __builtin_amdgcn_alignbit(va[q].y, va[q].y, 16), __builtin_amdgcn_alignbit(va[q].x, va[q].x, 16)};
                            *reinterpret_cast<v4u32_a2 *>(rows + (size_t)row * Ws + a) = ra;
                            *reinterpret_cast<v4u32_a2 *>(rows + (size_t)row * Ws + b) = rb;
                        }
                    }
                }
            }
            for (int it = tid; it < (E + 1) * 8; it += BT) {      // the middle of every matrix row
                const int row = it >> 3, u = 8 * I + (it & 7);
                if (u < rhs && !((need >> row) & 1)) {
                    u16 *base = rows + (size_t)row * Ws + rjl;
                    const u16 x = base[u], y = base[rM - 1 - u];
                    base[u] = y; base[rM - 1 - u] = x;
                }
            }
        }
        // the labels and the M-1 edge costs inside the range (and, TABU, the ages: they travel with their nodes), by array cell
        if (M <= 16) {
            const int item = (tid >> 3) - (BT / 8 - 3), u = tid & 7;      // the last three groups of 8 lanes
            if (item >= 1) {
                const bool lab = item == 1;
                const int last = lab ? M - 1 : M - 2, cnt = lab ? hs : hw;
                u16 *base = wt16 + (lab ? 1 : 0);
                if (u < cnt) {
                    int p1 = lo + u; if (p1 >= n) p1 -= n;
                    int p2 = lo + last - u; if (p2 >= n) p2 -= n;
                    const u16 x = base[2 * p1], y = base[2 * p2];
                    base[2 * p1] = y; base[2 * p2] = x;
                }
            } else if (TABU && item == 0 && u < hs) {
                int p1 = lo + u; if (p1 >= n) p1 -= n;
                int p2 = lo + M - 1 - u; if (p2 >= n) p2 -= n;
                const u16 x = age16[p1], y = age16[p2];
                age16[p1] = y; age16[p2] = x;
            }
        } else {
            if constexpr (TABU) {
                for (int u = tid; u < hs; u += BT) {
                    int p1 = lo + u; if (p1 >= n) p1 -= n;
                    int p2 = lo + M - 1 - u; if (p2 >= n) p2 -= n;
                    const u16 x = age16[p1], y = age16[p2];
                    age16[p1] = y; age16[p2] = x;
                }
            }
            for (int u = tid; u < hs; u += BT) {
                int p1 = lo + u; if (p1 >= n) p1 -= n;
                int p2 = lo + M - 1 - u; if (p2 >= n) p2 -= n;
                const u16 x = wt16[2 * p1 + 1], y = wt16[2 * p2 + 1];
                wt16[2 * p1 + 1] = y; wt16[2 * p2 + 1] = x;
            }
            for (int u = tid; u < hw; u += BT) {
                int p1 = lo + u; if (p1 >= n) p1 -= n;
                int p2 = lo + M - 2 - u; if (p2 >= n) p2 -= n;
                const u16 x = wt16[2 * p1], y = wt16[2 * p2];
                wt16[2 * p1] = y; wt16[2 * p2] = x;
            }
        }
        if (tid == BT - 1) { wt16[2 * eTT] = (u16)wTT; wt16[2 * eHH] = (u16)wHH; }
        LW_PHASE(5);                                  // (decode + own swaps, before the barrier)
        __syncthreads();
        if (lo < 8 || lo + M > n || eTT < 8 || eHH < 8) {  // the copy of cells 0 .. 7 behind cell n-1
            if (tid < 8) wt[n + tid] = wt[tid];
            __syncthreads();
        }
        if (swp) {
            unsigned s = swp;
            while (s) {
                const int r = __builtin_ctz(s);
                s &= s - 1;
                const int mr = __builtin_amdgcn_readlane(mirv, r);
                if (tid < (Ws >> 3)) {
                    v4u32 *qa = reinterpret_cast<v4u32 *>(rows + (size_t)r * Ws + tid * 8);
                    v4u32 *qb = reinterpret_cast<v4u32 *>(rows + (size_t)mr * Ws + tid * 8);
                    const v4u32 a = *qa, b = *qb;
                    *qa = b; *qb = a;
                }
            }
            __syncthreads();
        }
        if (fcnt > 0 && need != allrows) {
            // the range crosses a window end: the window cells whose mirror cell lies outside, by their new labels, straight
            // from the matrix (four loads in flight per lane)
            const int lane = tid & 63;
            for (int row = tid >> 6; row <= E; row += BT / 64) {
                if ((need >> row) & 1) continue;
                int oc = k0 + row; if (oc >= n) oc -= n;
                const unsigned x = wt16[2 * oc + 1];
                const u16 *mrow = A.mat + (size_t)x * ld;
                u16 *drow = rows + (size_t)row * Ws + fjl;
                const int jown = a0 + row;                 // local column of the row's own cell
                for (int c0 = lane; c0 < fcnt; c0 += 256) {
                    unsigned val[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int c = c0 + 64 * u;
                        if (c < fcnt) {
                            const unsigned lq = wt16[2 * cell_of(fjl + c) + 1];
                            val[u] = lq == x ? POISON : (unsigned)mrow[lq];
                            if (TABU && (unsigned)(fjl + c - jown + 1) <= 2u) val[u] = POISON;     // (the own node's two tour neighbours)
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int c = c0 + 64 * u;
                        if (c < fcnt) drow[c] = (u16)val[u];
                    }
                }
            }
            if (clk) ph[8]++;
            __syncthreads();
        }
        if constexpr (TABU) {
            // the four nodes of the move -- now at the cells eTT, lo, eHH, eHH+1 -- are tabu from the next iteration on
            // (tabu_list[.] = iter, metaheuristic.c:236-243), and each of them has lost one tour neighbour and won one:
            // its row gets the lost neighbour's cell back (the cost of the removed edge) and the new one's cell poisoned
            // (where the window holds those cells)
            int cD = eHH + 1; if (cD == n) cD = 0;
            if (tid < 4) {
                const int cell = tid == 0 ? eTT : tid == 1 ? lo : tid == 2 ? eHH : cD;
                const int back = tid == 0 ? eHH : tid == 1 ? cD : tid == 2 ? eTT : lo;      // cell that holds the lost neighbour
                const int won = tid == 0 ? lo : tid == 1 ? eTT : tid == 2 ? cD : eHH;       // cell that holds the new neighbour
                const unsigned val = (tid == 0 || tid == 2) ? wOldTT : wOldHH;
                age16[cell] = 0;
                int r = cell - k0; if (r < 0) r += n;
                if (r <= E && !((need >> r) & 1)) {
                    int jb = back - c_lo; if (jb < 0) jb += n;
                    int jw = won - c_lo; if (jw < 0) jw += n;
                    if (jb < Ws) rows[(size_t)r * Ws + jb] = (u16)val;
                    if (jw < Ws) rows[(size_t)r * Ws + jw] = (u16)POISON;
                }
            }
            __syncthreads();
        }
        LW_PHASE(3);                                  // reversal
        if (need) { reload(need); if (clk) { ph[6]++; ph[7] += __builtin_popcount(need); } }
        LW_PHASE(4);                                  // rows fetched
        if (clk && wg == 0 && sdone < 4000) A.stamps[8192 + sdone] = ((unsigned long long)M << 48) | (wall_clock64() & 0xFFFFFFFFFFFFull);
        }   // (!nomove)
        if constexpr (TABU) {
            // mh_TabuSearch's loop body behind the move (metaheuristic.c:126-143): incumbent, trace, the linear tenure policy
            iters++;
            const double cur = cost0 + (double)sumd;
            if (!nomove && cur < best) {              // every workgroup its own cells of the best tour
                best = cur;
                if (tid < E) A.best_ord[k0 + tid] = (int)wt16[2 * (k0 + tid) + 1];
                if (wg == 0 && tid == 0) { A.best_dir[0] = dir; A.best_dir[1] = 1; }
            }
            if (wg == 0 && tid == 0) A.trace[iters - 1] = cur;
            for (int q = tid; q < n; q += BT) { const unsigned a = age16[q]; if (a != 0xFFFFu) age16[q] = (u16)(a + 1); }
            if (tenure == A.t_max || tenure == A.t_min) tup = !tup;
            tenure += tup ? 1 : -1;
            if (iters >= A.tabu_k) status = LP_ST_CAPPED;
            __syncthreads();
            if (tid < 9) age16[n + tid] = age16[tid];  // the copy of cells 0 .. 8 behind cell n-1
            __syncthreads();
        } else {
            if (cap >= 0 && kd >= cap) status = LP_ST_CAPPED;
            else if (A.budget >= 0 && sdone >= A.budget) status = LP_ST_BUDGET;
        }
    }
#undef LW_PHASE
    if (clk) {
        unsigned long long *o = A.stamps + (size_t)wg * 16;
        for (int i = 0; i < 8; i++) o[i] = ph[i];
        o[8] = (unsigned long long)sdone; o[9] = ph[8];
    }
    // ---- the tour state back to the slot (every workgroup its own cells)
    if (tid < E) {
        const int p = k0 + tid;
        int pn = p + 1; if (pn == n) pn = 0;
        int pp = p - 1; if (pp < 0) pp += n;
        const int lab = wt16[2 * p + 1];
        A.S.ord[tn + p] = lab;
        reinterpret_cast<int *>(A.S.dpos + tn)[p] = (int)wt16[2 * p];
        A.S.pos[tn + lab] = p;
        A.S.succ[tn + lab] = dir > 0 ? (int)wt16[2 * pn + 1] : (int)wt16[2 * pp + 1];
        reinterpret_cast<int *>(A.S.dnb + tn)[lab] = dir > 0 ? (int)wt16[2 * p] : (int)wt16[2 * pp];
    }
    if (wg == 0 && tid == 0) {
        A.S.dir[t] = dir;
        A.S.cost[t] = cost0 + (double)sumd;
        A.S.nsweeps[t] = kd;
        if (sdone > 0) A.S.last_delta[t] = (double)lastd;
        if (status == LP_ST_OPTIMUM || status == LP_ST_CAPPED) A.S.done[t] = 1;
        if constexpr (TABU || VNS) *A.best_out = best;
        if constexpr (VNS) { A.vns_state[0] = vit; A.vns_state[1] = vcur; A.vns_state[2] = status == LP_ST_NEED_RAND ? 1 : 0; }
        A.ctl[1] = status; A.ctl[2] = sdone;
    }
}
