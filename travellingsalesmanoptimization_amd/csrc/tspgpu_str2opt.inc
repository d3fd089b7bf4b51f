// ---------------------------------------------------------------------------
// k_str2opt: ONE launch for a whole 2-opt descent with the matrix STREAMED (ref_2opt, src/algorithms/refinment.c:6-37;
// ref_2opt_once :39-95; ref_reverse_path :97-114) -- single tours whose uint16 matrix no longer fits the chip's LDS
// (n > ~5 400: past k_lds2opt_w) and that the one-launch-per-sweep kernel serves badly: at n = 5 600 ... 9 000 a sweep's
// rows stream in 10 ... 20 us out of the Infinity Cache, and a launch boundary + the dependent prologue of k_sweep_fused
// (key -> record -> state records -> rows requested) + its tail cost another ~8 us every sweep.
// Included by tspgpu.hip (uses BState / sweep_step_as / pipe_stream2 / block_best and the slot exchange of k_lds2opt).
//
//   * grid = one workgroup per CU, co-resident (rendezvous as in k_lds2opt); workgroup g owns the P = ceil(n / W) tour edges
//     at array cells [gP, gP + P) and, per sweep, streams the P + 1 matrix rows of the nodes at those cells exactly as
//     k_sweep_pipe / k_sweep_fused do (pipe_stream2: a row lives in registers as "row of a" and in LDS as "row of succ a",
//     two tour edges per barrier interval) -- the evaluation, the block ownership of pairs and the argmin are sweep_step_as;
//   * what a launch boundary used to carry stays ON THE CHIP: every thread keeps the direction-free records of its own
//     b's -- array cell, both array neighbours, both edge costs (k_sweep_fused's `Fused` state: 2.5 registers per b) -- in
//     REGISTERS for the whole descent, every workgroup the node-per-cell array in LDS (2n bytes).  A move reverses an
//     array range: cells inside reflect and their nodes swap (left, right); the four nodes at its ends get one new
//     neighbour and one new edge cost.  Every workgroup applies that to its own copy from the exchanged record alone
//     (O(1) per b, no memory trip except two scalar loads of the new edges' costs);
//   * a sweep ends in ONE grid-wide exchange (the tagged 16-byte slot records of k_lds2opt): key (delta, a, b) in the
//     reference's first-found best-improvement order, and the two array cells + the two successors of the winning pair.
//
// Same moves, same tours as every other sweep kernel (tests: move by move against the oracle).
// ---------------------------------------------------------------------------
struct StreamArgs {
    Tours S;
    const u16 *mat;
    int n, ld, slot;
    int P;                 // tour edges per workgroup
    int budget;            // sweeps this launch may run (< 0: until the local optimum / the sweep cap)
    int poll_sleep;
    int ablate;            // diagnostics only (option 99): 1 = no pair evaluation, 2 = no row traffic (results are wrong)
    u64 *slots;            // [2][W][8] exchange records, 64-byte stride, zeroed before the launch
    int *ctl;              // [0] abort flag  [1] status (LP_ST_*)  [2] sweeps run by this launch
    HistBuf hist;
    long hello_ticks, spin_ticks;
    unsigned long long *stamps;
};

static constexpr u64 SP_KEYMASK = (1ull << 60) - 1;
static constexpr int SP_DBIAS = 131072;                  // |delta| < 2 * 65535
static constexpr u64 SP_NONE = 0x3FFFFull << 28;         // "no improving pair": delta field all ones, labels 0

// LDS bytes of k_str2opt for (n, ld, P) -- the host asks for at least 82 KB so that one workgroup owns a CU
using plan::sp_lds_rows;       // (tspgpu_plan.h: the host sizes the launch with the same functions)
using plan::sp_lds_ord;
using plan::sp_lds_nodes;
using plan::SP_LDS_SCRATCH;

template <int NCH, int MAXBT>
__global__ void __launch_bounds__(MAXBT) k_str2opt(StreamArgs A)
{
    typedef u16 T;
    typedef Elem<T>::vec VT;
    constexpr int V = 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int n = A.n, ld = A.ld, W = (int)gridDim.x, wg = (int)blockIdx.x, tid = (int)threadIdx.x, BT = (int)blockDim.x, t = A.slot;
    const size_t tn = (size_t)t * n;
    // LDS: 4 row buffers | ord16: node per array cell | nodes[-1 .. P] | reduction scratch, (64 spare bytes), exchange candidates
    T *rows = reinterpret_cast<T *>(smem);
    u16 *ord16 = reinterpret_cast<u16 *>(smem + sp_lds_rows(ld));
    int *nodes = reinterpret_cast<int *>(smem + sp_lds_rows(ld) + sp_lds_ord(n)) + 1;
    unsigned char *scr0 = smem + sp_lds_rows(ld) + sp_lds_ord(n) + sp_lds_nodes(A.P);
    Partial *scratch = reinterpret_cast<Partial *>(scr0);
    u64 *cands = reinterpret_cast<u64 *>(scr0 + 32 * sizeof(Partial) + 64);
    const unsigned lds0 = (unsigned)(uintptr_t)(lds_u8 *)smem;

    auto give_up = [&](int status) __attribute__((always_inline)) {
        if (tid == 0) {
            atomicCAS(A.ctl + 1, LP_ST_RUNNING, status);
            __hip_atomic_store(A.ctl, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    // One grid-wide exchange (k_lds2opt's): lanes with `have` publish (w0, w1) as this workgroup's record of step s; returns
    // the record with the smallest 60-bit key over all workgroups, 0 when the exchange failed.
    auto publish = [&](int s, bool have, u64 w0, u64 w1) __attribute__((always_inline)) {
        u64 *buf = A.slots + (size_t)(s & 1) * W * 8;
        const u64 tag = (u64)((s % 15) + 1) << 60;
        if (have) lp_st128(buf + (size_t)wg * 8, tag | w0, tag | w1);
    };
    auto collect = [&](int s, u64 &r0, u64 &r1, long limit) __attribute__((always_inline)) {
        u64 *buf = A.slots + (size_t)(s & 1) * W * 8;
        const u64 tag = (u64)((s % 15) + 1) << 60;
        u64 a = SP_KEYMASK, b = 0;
        if (tid < W) {
            const long tp = wall_clock64();
            for (int spins = 0;;) {
                lp_ld128(buf + (size_t)tid * 8, a, b);
                if ((a >> 60) == (tag >> 60) && (b >> 60) == (tag >> 60)) { a &= SP_KEYMASK; break; }
                for (int z = 0; z < A.poll_sleep; z++) __builtin_amdgcn_s_sleep(1);
                if ((++spins & 7) == 0 &&
                    (wall_clock64() - tp > limit || __hip_atomic_load(A.ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) { a = 0; break; }
            }
        }
        const long long wm = wave_min_i64((long long)a);
        const int wv = tid >> 6, nwp = (W + 63) >> 6;
        u64 *cand = cands + (s & 1) * 16;
        if (wv < nwp && (long long)a == wm) { cand[2 * wv] = a; cand[2 * wv + 1] = b; }
        __syncthreads();
        u64 x0 = cand[0], x1 = cand[1];
        for (int i = 1; i < nwp; i++) { const u64 y = cand[2 * i]; if (y < x0) { x0 = y; x1 = cand[2 * i + 1]; } }
        r0 = ((u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(x0 >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)x0);
        r1 = ((u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(x1 >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)x1);
    };

    // ---- rendezvous: is the whole grid resident?
    u64 r0, r1;
    publish(0, tid == 0 && (A.hello_ticks > 0 || wg != 0), 1ull << 28, 0);
    collect(0, r0, r1, A.hello_ticks > 0 ? A.hello_ticks : -A.hello_ticks);
    if (r0 == 0) { give_up(LP_ST_NO_RENDEZVOUS); return; }

    int dir = A.S.dir[t];
    const int cap = A.S.cap_sweeps[t];
    int kd = A.S.nsweeps[t];                          // sweeps completed (this call)
    int sdone = 0;                                    // ... by this launch
    long long sumd = 0;
    int lastd = 0;
    const double cost0 = A.S.cost[t];

    // ---- the tour state: node per cell in LDS; per own b (every workgroup holds ALL nodes: thread (c, tid) the 8 nodes from
    // (c BT + tid) 8 on) its array cell, its two array neighbours (left | right << 16) and the costs of the two edges
    // (left | right << 16), in registers for the whole launch
    // (succ-side word = what BState holds: the LDS byte offset of succ b | c[b][succ b] << 16; pred-side word: the same for
    // the predecessor.  A move swaps the two words of the nodes inside the reversed range -- or, when the other arc is the one
    // reversed and the direction toggles, of the nodes outside it)
    unsigned qp[NCH][V / 2], pd[NCH][V];
    BState<T, NCH> B;
    B.skm = 0;
    {
        const int *ord = A.S.ord + tn, *pos = A.S.pos + tn;
        const int *dp = reinterpret_cast<const int *>(A.S.dpos + tn);
        const bool fwd0 = dir > 0;
        for (int q = tid; q < n; q += BT) ord16[q] = (u16)ord[q];
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            const int ub0 = (c * BT + tid) * V;
            int pv[V];
            load_run<V>(pos + min(ub0, ld - V), pv);
#pragma unroll
            for (int v = 0; v < V; v++) {
                const int b = ub0 + v;
                unsigned q = 0, l = 0, r = 0, dl = 0, dr = 0;
                if (b < n) {
                    q = (unsigned)pv[v];
                    const int ql = q == 0 ? n - 1 : (int)q - 1, qr = (int)q + 1 == n ? 0 : (int)q + 1;
                    l = (unsigned)ord[ql]; r = (unsigned)ord[qr];
                    dl = (unsigned)dp[ql]; dr = (unsigned)dp[q];
                }
                if (v & 1) qp[c][v >> 1] |= q << 16; else qp[c][v >> 1] = q;
                const unsigned wl_ = (l << 1) | (dl << 16), wr_ = (r << 1) | (dr << 16);
                B.sb[c][v] = (int)(fwd0 ? wr_ : wl_);
                pd[c][v] = fwd0 ? wl_ : wr_;
            }
        }
    }

    const int p0 = wg * A.P;
    const int cnt = min(A.P, n - p0);                 // (host: >= 1 for every workgroup)
    int status = LP_ST_RUNNING;
    if (cap >= 0 && kd >= cap) status = LP_ST_CAPPED;        // (cap 0: not one sweep)

    SweepArgs SA;
    SA.mat = A.mat; SA.n = n; SA.ld = ld; SA.ablate = A.ablate; SA.symmetric = 1; SA.P = A.P;

    // phase clocks (TSPGPU_OPT_STAMPS): thread 0 of every workgroup sums wall-clock ticks per phase
    unsigned long long ph[6] = {0, 0, 0, 0, 0, 0};
    const bool clk = A.stamps != nullptr && tid == 0;
    unsigned long long tc = clk ? wall_clock64() : 0ull;
#define SP_PHASE(i) do { if (clk) { const unsigned long long now_ = wall_clock64(); ph[i] += now_ - tc; tc = now_; } } while (0)

    __syncthreads();                                  // ord16 complete
    while (status == LP_ST_RUNNING) {
        // ---- the run in TOUR order: nodes[s] = a of step s, nodes[s+1] = its successor, nodes[-1] = its predecessor
        for (int i = tid - 1; i <= cnt; i += BT) {
            int p = p0 + (dir > 0 ? i : cnt - i);
            if (p < 0) p += n; else if (p >= n) p -= n;
            nodes[i] = (int)ord16[p];
        }
        const bool fwd = dir > 0;
        __syncthreads();                              // nodes[] visible
        SP_PHASE(0);
        Best q;
        best_init<false>(q);
        pipe_stream2<T, NCH, (NCH == 1 || MAXBT <= 512 ? 2 : 1)>(q, SA, B, rows, nodes, lds0, cnt, nullptr);
        SP_PHASE(1);

        // ---- the workgroup's best pair; its one finder leaves the record
        double d;
        u64 key;
        const bool winner = block_best<T, false>(q, d, key, scratch);
        u64 mykey = SP_NONE, mypay = 0;
        const bool found = key != 0;                  // (workgroup-uniform)
        if (found) {
            const int la = (int)(key >> 32), lb = (int)(key & 0xffffffffu);      // la < lb
            int own = -1, idx = 0, other = 0;
            if (winner) {
                // which of the two labels is the thread's own b (see k_sweep_fused: with several chunks per thread both can be)
                int idx_a = -1, idx_b = -1;
#pragma unroll
                for (int c = 0; c < NCH; c++) {
                    const int b0c = (c * BT + tid) * V;
                    if ((unsigned)(lb - b0c) < (unsigned)V) idx_b = c * V + (lb - b0c);
                    if ((unsigned)(la - b0c) < (unsigned)V) idx_a = c * V + (la - b0c);
                }
                bool own_is_b = idx_b >= 0;
                if (idx_a >= 0 && idx_b >= 0) {
                    const int NBk = (n + 64 * V - 1) / (64 * V), blka = la / (64 * V), blkb = lb / (64 * V);
                    const int dblk = blkb - blka;
                    own_is_b = dblk == 0 || 2 * dblk < NBk || (2 * dblk == NBk && blka < blkb);
                }
                own = own_is_b ? lb : la; idx = own_is_b ? idx_b : idx_a;
                other = own_is_b ? la : lb;
            }
            // where in the run the pair's run node sits: the winner's own wave looks (lane l at nodes[l]; cnt <= 64), no barrier
            int sidx = 0;
            const u64 wl = __ballot(winner);
            if (wl) {
                const int oth = __builtin_amdgcn_readlane(other, __builtin_ctzll(wl));
                const int lane = tid & 63;
                const u64 hit = __ballot(lane < cnt && nodes[lane] == oth);
                sidx = __builtin_ctzll(hit | (1ull << 63));
            }
            if (winner) {
                unsigned q_own = 0, sb_own = 0;
#pragma unroll
                for (int c = 0; c < NCH; c++)
#pragma unroll
                    for (int v = 0; v < V; v++)
                        if (c * V + v == idx) {
                            q_own = (v & 1) ? qp[c][v >> 1] >> 16 : qp[c][v >> 1] & 0xffffu;
                            sb_own = ((unsigned)B.sb[c][v] & 0xffffu) >> 1;
                        }
                const unsigned sa = (unsigned)nodes[sidx + 1];
                int cell_o = p0 + (fwd ? sidx : cnt - sidx);
                if (cell_o >= n) cell_o -= n;
                const bool own_la = own == la;
                const unsigned cell_la = own_la ? q_own : (unsigned)cell_o, cell_lb = own_la ? (unsigned)cell_o : q_own;
                const unsigned s_la = own_la ? sb_own : sa, s_lb = own_la ? sa : sb_own;
                mykey = ((u64)(unsigned)((int)d + SP_DBIAS) << 28) | ((u64)(unsigned)la << 14) | (unsigned)lb;
                mypay = (u64)cell_la | ((u64)cell_lb << 14) | ((u64)s_la << 28) | ((u64)s_lb << 42);
            }
        }
        const bool have = found ? winner : tid == 0;
        SP_PHASE(2);
        // ---- exchange
        sdone++;
        publish(sdone, have, mykey, mypay);
        collect(sdone, r0, r1, A.spin_ticks);
        if (r0 == 0) { give_up(LP_ST_LOST); return; }
        SP_PHASE(3);
        kd++;
        const bool nomove = (r0 >> 28) == 0x3FFFFull;
        if (nomove) {                                 // the final, non-improving sweep
            lastd = 0;
            if (wg == 0 && tid == 0 && t == 0 && kd <= A.hist.cap) { A.hist.a[kd - 1] = -1; A.hist.b[kd - 1] = -1; A.hist.d[kd - 1] = 0.0; }
            status = LP_ST_OPTIMUM;
            break;
        }
        {
            const int md = (int)((r0 >> 28) & 0x3FFFFu) - SP_DBIAS;
            const int ma = (int)((r0 >> 14) & 0x3fffu), mb = (int)(r0 & 0x3fffu);
            const int i = (int)(r1 & 0x3fffu), j = (int)((r1 >> 14) & 0x3fffu);
            const int sma = (int)((r1 >> 28) & 0x3fffu), smb = (int)((r1 >> 42) & 0x3fffu);
            sumd += md; lastd = md;
            if (wg == 0 && tid == 0 && t == 0 && kd <= A.hist.cap) { A.hist.a[kd - 1] = ma; A.hist.b[kd - 1] = mb; A.hist.d[kd - 1] = (double)md; }
            // the two new edges {a, b}, {succ a, succ b}: two vector loads (every lane the same cell) issued NOW and waited for
            // behind the reversal -- scalar loads would share lgkmcnt with the LDS traffic below and be waited for at its first read
            // (plain loads: the compiler waits for them at their first use, in the patch behind the update loop)
            const unsigned cab = A.mat[(size_t)ma * ld + mb], css = A.mat[(size_t)sma * ld + smb];
            // ---- the move as an array operation (k_sweep_fused): reverse cells [lo, lo + M - 1] (cyclic)
            int L = (j - i) * dir;
            if (L < 0) L += n;
            const bool other = n - L < L;
            const int M = other ? n - L : L;
            const int first = other ? wrap(j + dir, n) : wrap(i + dir, n);
            const int lo = dir > 0 ? first : wrap(first - (M - 1), n);
            const int ndir = other ? -dir : dir;
            int x0, x1, x2, x3;
            if (!other) { if (dir > 0) { x0 = ma; x1 = sma; x2 = mb; x3 = smb; } else { x0 = smb; x1 = mb; x2 = sma; x3 = ma; } }
            else        { if (dir > 0) { x0 = mb; x1 = smb; x2 = ma; x3 = sma; } else { x0 = sma; x1 = ma; x2 = smb; x3 = mb; } }
            // node per cell
            for (int u = tid; u < (M >> 1); u += BT) {
                int c1 = lo + u; if (c1 >= n) c1 -= n;
                int c2 = lo + M - 1 - u; if (c2 >= n) c2 -= n;
                const u16 a1 = ord16[c1], a2 = ord16[c2];
                ord16[c1] = a2; ord16[c2] = a1;
            }
            // the own b's: cells inside the range reflect; the nodes whose successor side flips -- inside the range, or, when the
            // direction toggles, outside it -- swap their two words
            const int wrap_end = lo + M - n;          // > 0 only when the range wraps round the array end
            const int refl = lo + M - 1;
#pragma unroll
            for (int c = 0; c < NCH; c++) {
#pragma unroll
                for (int v = 0; v < V; v++) {
                    const unsigned qq = (v & 1) ? qp[c][v >> 1] >> 16 : qp[c][v >> 1] & 0xffffu;
                    const bool inr = ((unsigned)((int)qq - lo) < (unsigned)M) | ((int)qq < wrap_end);
                    int r = (int)qq - lo; if (r < 0) r += n;      // new cell = (lo + M - 1 - r) mod n
                    int qn = refl - r; if (qn >= n) qn -= n;
                    const unsigned qv = inr ? (unsigned)qn : qq;
                    if (v & 1) qp[c][v >> 1] = (qp[c][v >> 1] & 0xffffu) | (qv << 16);
                    else qp[c][v >> 1] = (qp[c][v >> 1] & 0xffff0000u) | qv;
                    const bool sw = inr != other;
                    const unsigned s0 = (unsigned)B.sb[c][v], p0w = pd[c][v];
                    B.sb[c][v] = (int)(sw ? p0w : s0);
                    pd[c][v] = sw ? s0 : p0w;
                }
            }
            // x0 | [x1 .. x2] | x3 becomes x0 | [x2 .. x1] | x3: x0's right neighbour is x2 over wA, x3's left neighbour x1 over wB
            // (right = the successor side when the new direction is forward)
            const unsigned wA = dir > 0 ? cab : css, wB = dir > 0 ? css : cab;
            const bool nf = ndir > 0;
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const int ub0 = (c * BT + tid) * V;
                if (((unsigned)(x0 - ub0) < (unsigned)V) | ((unsigned)(x1 - ub0) < (unsigned)V) | ((unsigned)(x2 - ub0) < (unsigned)V) |
                    ((unsigned)(x3 - ub0) < (unsigned)V)) {
#pragma unroll
                    for (int v = 0; v < V; v++) {
                        const int b = ub0 + v;
                        unsigned rt = nf ? (unsigned)B.sb[c][v] : pd[c][v], lt = nf ? pd[c][v] : (unsigned)B.sb[c][v];
                        if (b == x0) rt = ((unsigned)x2 << 1) | (wA << 16);
                        if (b == x3) lt = ((unsigned)x1 << 1) | (wB << 16);
                        if (b == x1) rt = ((unsigned)x3 << 1) | (wB << 16);
                        if (b == x2) lt = ((unsigned)x0 << 1) | (wA << 16);
                        B.sb[c][v] = (int)(nf ? rt : lt);
                        pd[c][v] = nf ? lt : rt;
                    }
                }
            }
            dir = ndir;
        }
        __syncthreads();                              // ord16 reversed
        SP_PHASE(4);
        if (cap >= 0 && kd >= cap) status = LP_ST_CAPPED;
        else if (A.budget >= 0 && sdone >= A.budget) status = LP_ST_BUDGET;
    }
#undef SP_PHASE
    if (clk) {
        unsigned long long *o = A.stamps + (size_t)wg * 16;
        for (int i = 0; i < 6; i++) o[i] = ph[i];
        o[8] = (unsigned long long)sdone;
    }
    // ---- the tour state back to the slot: every workgroup holds all of it; workgroup 0 writes
    if (wg == 0) {
        int *dp = reinterpret_cast<int *>(A.S.dpos + tn), *dnb = reinterpret_cast<int *>(A.S.dnb + tn);
        const bool fwd = dir > 0;
#pragma unroll
        for (int c = 0; c < NCH; c++)
#pragma unroll
            for (int v = 0; v < V; v++) {
                const int b = (c * BT + tid) * V + v;
                if (b < n) {
                    const int qq = (int)((v & 1) ? qp[c][v >> 1] >> 16 : qp[c][v >> 1] & 0xffffu);
                    const unsigned sw_ = (unsigned)B.sb[c][v], rt = fwd ? sw_ : pd[c][v];
                    A.S.pos[tn + b] = qq;
                    A.S.ord[tn + qq] = b;
                    dp[qq] = (int)(rt >> 16);                       // edge between cells qq and qq + 1
                    A.S.succ[tn + b] = (int)((sw_ & 0xffffu) >> 1);
                    dnb[b] = (int)(sw_ >> 16);
                }
            }
        if (tid == 0) {
            A.S.dir[t] = dir;
            A.S.cost[t] = cost0 + (double)sumd;
            A.S.nsweeps[t] = kd;
            if (sdone > 0) A.S.last_delta[t] = (double)lastd;
            if (status == LP_ST_OPTIMUM || status == LP_ST_CAPPED) A.S.done[t] = 1;
            A.ctl[1] = status; A.ctl[2] = sdone;
        }
    }
}
