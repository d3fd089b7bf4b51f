// ---------------------------------------------------------------------------
// k_lds2opt: the whole uint16 matrix resident in LDS, ONE launch for a whole 2-opt descent
// (ref_2opt, src/algorithms/refinment.c:6-37; ref_2opt_once :39-95; ref_reverse_path :97-114).
// Included by tspgpu.hip (uses Tours, HistBuf, the DPP helpers).
//
// A uint16 matrix of n <= 4096 (33.5 MB) is smaller than the chip's LDS (256 x 160 KiB = 41.9 MB) and a move
// changes a median of 3 array cells, so nothing has to be streamed from HBM per sweep at all:
//
//   * workgroup g (one per CU, 512 threads) owns the E = ceil(n / CUs) tour edges at array cells
//     [gE, gE+E) and keeps the E+1 matrix rows of their end nodes in LDS -- PERMUTED INTO TOUR ORDER:
//         G_x[q] = c[x][ord[q]]                       (row of node x, indexed by array cell q)
//     together with wt[q] = (c[ord q][ord q+1], ord[q]).  With the rows in tour order the 2-opt delta of
//     the edge pair (k, m) needs no gather:
//         delta(k, m) = G_{ord k}[m] + G_{ord k+1}[m+1] - w[k] - w[m]
//     (both operands are consecutive reads; the pair is the reference's (a, b) = the two edge tails in
//     the tour's direction, a < b by label; delta is symmetric).  Adjacent edges give exactly 0 and the
//     pair (k, k) is kept out by a poisoned diagonal, so the inner loop carries no mask.  With every
//     cost <= 16383 the loop runs in packed 16-bit arithmetic (two pairs per instruction).  With n a
//     multiple of 16 a pair is evaluated by one of its two owners only (see "evaluation geometry").
//   * a sweep ends in ONE grid-wide exchange: every workgroup publishes its best pair as a tagged
//     16-byte record in its own 64-byte slot (agent-scope store), every workgroup polls all slots
//     (agent-scope loads) and takes the minimum of (delta, a, b) -- the reference's first-found
//     best-improvement order.  No atomics, no second trip: the record carries the two array cells and
//     the two new edge costs.  (Measured on MI355X: 2.5-2.7 us for 256 workgroups; an atomic-min +
//     counter barrier: 5.9 us; a kernel boundary: 2.7 us + the 6 us it takes to stream the rows again.)
//   * every workgroup applies the move to its own copy: the reversed cell range is reversed in wt and in
//     each of its rows (the shorter arc, <= n/2 cells, as k_apply does).  A workgroup whose own cells lie
//     inside the range gets other nodes: a row whose node stays in the workgroup changes places with
//     its mirror row, the others are fetched from the matrix (coalesced), staged in LDS and permuted
//     into tour order.
//
// The grid must be co-resident (one workgroup per CU, 160 KiB of LDS each): the kernel starts with a
// rendezvous exchange under a short wall-clock limit and leaves without touching the tour when it
// fails (the host then runs the one-launch-per-sweep path); every later spin is bounded as well, so
// the grid always drains.
// ---------------------------------------------------------------------------
typedef unsigned v4u32 __attribute__((ext_vector_type(4)));
typedef v4u32 v4u32_a2 __attribute__((aligned(2)));       // 16 bytes of LDS at a 2-byte boundary (unaligned DS access)
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

struct PersistArgs {
    Tours S;
    const u16 *mat;
    int n, ld, slot;
    int E;                 // tour edges per workgroup (<= LP_EMAX)
    int nl;                // LDS row stride in cells: n rounded up to 8
    int budget;            // sweeps this launch may run (< 0: until the local optimum / the sweep cap)
    int Ws, nstage;        // k_lds2opt_w: window cells per row, staging rows (1 or 2)
    int poll_sleep;        // s_sleep(1) repetitions between two polls of a slot (0: none)
    u64 *slots;            // [2][W][8] exchange records, 64-byte stride, zeroed before the launch
    int *ctl;              // [0] abort flag  [1] status (LP_ST_*)  [2] sweeps run by this launch
    HistBuf hist;
    long hello_ticks, spin_ticks;   // wall_clock64 (100 MHz) limits of the rendezvous / of a later exchange
    unsigned long long *stamps;
    // TABU instance (mh_TabuSearch, metaheuristic.c:86-245: k iterations of tabu_best_move under the linear tenure policy)
    int tabu_k, tenure0, t_min, t_max, up0;
    double best0;          // cost of the best tour so far (the tour the call starts from)
    int *best_ord;         // [n] the best tour as node-per-array-cell, every workgroup its own cells (written whenever the cost
                           // improves; by CELL, whose owner never changes: two workgroups never write one address at
                           // different times, which the per-XCD write-back L2s would not order)
    int *best_dir;         // [0] direction of that tour, [1] set once the cost has improved (k_lds_best_succ turns both into
                           // the successor array behind the kernel boundary)
    double *trace;         // [tabu_k] cost after every iteration
    double *best_out;      // the best cost at the end
    // VNS instance (mh_VNS, metaheuristic.c:279-318: k iterations of local search + kicks; tspgpu_lds_vns.inc).  Shares best0,
    // best_ord, best_dir, trace (cost of every local optimum of this launch) and best_out with the tabu walk.
    int vns_k;             // iterations this launch may complete (0: a plain descent)
    int vns_it0;           // iterations completed before this launch
    int vns_phase;         // 1: the launch resumes in the kick phase of iteration vns_it0 (its local optimum is the slot's tour)
    int vns_nrand;         // rand() values in vns_rand
    const int *vns_rand;   // the caller's random numbers in the order the reference consumes them
    int *vns_state;        // out: [0] iterations completed, [1] numbers consumed, [2] 1 = stopped in front of a kick phase for want of numbers
    // TM instantiations of the shaped k_lds2opt: [n][n] the matrix with its columns in tour order (tspgpu_lds_tmat.h), filled by
    // every launch.  A row is written by whichever workgroup holds its node, at different times by different ones: every access
    // is agent scope (sc1), and a workgroup publishes its record of a sweep only behind the acknowledgement of its stores.
    u16 *tmat;
};

using plan::LP_EMAX;      // tour edges per workgroup at most, threads (tspgpu_plan.h)
using plan::LP_BT;
static constexpr u64 LP_KEYMASK = (1ull << 60) - 1;
static constexpr u64 LP_NONE = 0xFFFFFFFFFull << 24;     // "no improving pair": delta field all ones, labels 0
static constexpr int LP_DBIAS = 131072;

__device__ __forceinline__ void lp_ld128(const u64 *p, u64 &a, u64 &b)
{
    v4u32 r;
    asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(r) : "v"(p) : "memory");
    a = r.x | (u64)r.y << 32; b = r.z | (u64)r.w << 32;
}
__device__ __forceinline__ void lp_st128(u64 *p, u64 a, u64 b)
{
    const v4u32 r = {(unsigned)a, (unsigned)(a >> 32), (unsigned)b, (unsigned)(b >> 32)};
    asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(p), "v"(r) : "memory");
}
__device__ __forceinline__ int wave_min_i32(int x)
{
#define STEP(C, R) { const int o = (int)dpp_u32<C, R>((unsigned)x); x = o < x ? o : x; }
    DPP_WAVE_STEPS(STEP)
#undef STEP
    return __builtin_amdgcn_readlane(x, 63);
}
__device__ __forceinline__ int wave_sum_i32(int x)        // the wave's sum (valid in every lane)
{
#define STEP(C, R) x += __builtin_amdgcn_update_dpp(0, x, C, R, 0xf, false);
    DPP_WAVE_STEPS(STEP)
#undef STEP
    return __builtin_amdgcn_readlane(x, 63);
}
__device__ __forceinline__ unsigned lp_pk_add(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, (u16x2)(__builtin_bit_cast(u16x2, a) + __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ unsigned lp_pk_sub(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, (s16x2)(__builtin_bit_cast(s16x2, a) - __builtin_bit_cast(s16x2, b)));
}
__device__ __forceinline__ unsigned lp_pk_min(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b)));
}
__device__ __forceinline__ unsigned lp_pk_minu(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
// lds_tmat::pk_bias of the low half of a wt word (w | label << 16) in ONE instruction: a packed subtraction whose second operand
// is the word's low half for both halves of the result
__device__ __forceinline__ unsigned lp_pk_bias(unsigned wtword)
{
    unsigned b;
    asm("v_pk_sub_u16 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(b) : "v"(lds_tmat::PK_BIAS), "v"(wtword));
    return b;
}
// TABU: tabu_best_move instead of ref_2opt_once -- the best pair none of whose four nodes is tabu, whatever the sign of its
// delta (metaheuristic.c:188-245), applied every iteration; the nodes' ages (iterations since they were last moved) live
// in LDS beside the labels.  Pairs of adjacent edges must now lose for real (a delta of 0 can be the minimum): the cells
// of a row's own node AND of its two tour neighbours are poisoned -- both operands of an invalid pair are poisoned
// cells, no operand of a valid pair is -- and kept so by four two-cell patches per move.  PK16 then needs every cost
// <= 8190 (2 * 16383 - 2 * cost must exceed every valid delta); the 32-bit form recognises the poison by its value.
// VNS: mh_VNS's loop around the descent (tspgpu_lds_vns.inc) -- its own instantiation, so that the plain descent carries
// none of its code or registers.
// NLC, EC: the SHAPED form of the plain packed descent (NLC > 0): the host promises n == nl == NLC (a power of two, so that
// every wrap of an array cell is a mask), E == EC (even) and W == NLC / EC workgroups, hence the "once" evaluation geometry,
// k0 = wg * EC and no overlapping last workgroup.  The sweep loop then knows its strides and trip counts: the evaluation is
// unrolled over the EC/2 rows of the thread's half with immediate LDS offsets, the half's w[k] arrive in wide reads, the
// minima stay packed until a column is known to hold the workgroup's minimum, and the exchange reads its wave candidates
// with independent wide reads.  Same algorithm, keys, records, slots and barriers; NLC == 0 is the generic kernel, unchanged.
// (The shaped form reads A again from the kernel-argument segment at offset 0: PersistArgs must stay the ONLY argument.)
// TM: the shaped form with the rows that a move brings to a workgroup read from A.tmat -- the matrix kept in TOUR order in device
// memory by the workgroups that hold the rows -- with plain wide loads straight into place, the reversal applied on the way in,
// instead of read from the matrix in node order and permuted through LDS (reload: a barrier and 8 label gathers per row).
//   * fill: behind the first reload every workgroup stores its rows 0 .. E-1 to tmat[node of the row];
//   * write-back: behind every move every workgroup stores, for each row r < E it holds NOW, the aligned 8-cell chunks that
//     overlap the reversed range -- each node sits at one cell, so each row of tmat has one writer per sweep;
//   * fetch: a needed row r < E of node x is read from tmat[x], which nobody but this workgroup touches in this sweep and which
//     is still in the order before the move: cell q takes the cell tspgpu_lds_tmat.h's src_cell names.  A thread's chunk is
//     fetched whole (as it is, or the mirrored 8 cells reversed in registers) unless it is one of the at most three chunks a
//     row has that mix both kinds or whose mirrored run crosses the array end: those go cell by cell, one lane a cell;
//   * row E, the copy of the neighbour's first row, keeps reload()'s path through the matrix: its owner reads and rewrites
//     tmat[x] in this very sweep;
//   * every thread waits for its stores (vmcnt(0)) in front of the last barrier before the exchange: a published record implies
//     that the workgroup's tmat is up to date, and a row is read only behind the exchange of the sweep that moves it.
// CLK: the shaped form with the phase clocks (TSPGPU_OPT_STAMPS).  Their counters live in every thread across the whole sweep
// loop, so the shaped form that production runs (CLK false) has none of them; the other forms keep theirs whatever CLK says.
template <bool PK16, bool TABU, bool VNS = false, int NLC = 0, int EC = 0, bool TM = false, bool CLK = false>
__global__ void __launch_bounds__(LP_BT) k_lds2opt(PersistArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int EMAX = LP_EMAX, BT = LP_BT;
    constexpr bool SH = NLC > 0;
    constexpr bool CLOCKS = !SH || CLK;
    static_assert(SH || !CLK, "the clocked instantiation is a shaped one: the other forms always carry their clocks");
    constexpr int WC = NLC / (EC > 0 ? EC : 1);             // workgroups of the shaped form
    typedef __attribute__((address_space(4))) const PersistArgs c_PersistArgs;      // (the kernel arguments where they lie)
    static_assert(!SH || (PK16 && !TABU && !VNS), "the shaped form is the plain packed descent");
    static_assert(!TM || SH, "the tour-ordered copy needs the shaped form: n == nl a power of two, k0 = wg * E, no overlapping workgroup");
    static_assert(!SH || ((NLC & (NLC - 1)) == 0 && NLC % 16 == 0 && NLC / 8 <= LP_BT), "shaped n: a power of two, at most 8 cells a thread");
    static_assert(!SH || (EC >= 2 && EC % 2 == 0 && EC <= LP_EMAX && NLC % EC == 0 && NLC / EC <= 256), "shaped E: even, W = n / E <= 256");
    constexpr unsigned POISON = PK16 ? 16383u : 65535u;     // on the diagonal: delta(k, k) = 2 POISON - 2 w[k] >= 0
    const int n = SH ? NLC : A.n, nl = SH ? NLC : A.nl, ld = A.ld, E = SH ? EC : A.E, W = SH ? WC : (int)gridDim.x,
              wg = (int)blockIdx.x, tid = (int)threadIdx.x, t = A.slot;
    // array cells wrap at n: from above (p < 2n), from below (p >= -n), at n exactly -- one mask in the shaped form
#define LP_WRAP_HI(p) if constexpr (SH) p &= NLC - 1; else if (p >= n) p -= n
#define LP_WRAP_LO(p) if constexpr (SH) p &= NLC - 1; else if (p < 0) p += n
#define LP_WRAP_EQS(p) if constexpr (SH) p &= NLC - 1; else if (p == n) p = 0
#define LP_TID (SH ? tid_sweep : tid)
#define LP_LM0 (SH ? lm0_sweep : lm0)
#define LP_WRAP_EQ(p) (SH ? ((p) & (NLC - 1)) : ((p) == n ? 0 : (p)))
    const size_t tn = (size_t)t * n;
    // LDS: E+1 rows of nl cells | wt: nl words (w | label << 16) | one staging row (scratch between the staging uses)
    u16 *rows = reinterpret_cast<u16 *>(smem);
    u16 *wt16 = reinterpret_cast<u16 *>(smem + (size_t)(E + 1) * nl * 2);     // [2q] = w[q], [2q+1] = ord[q]
    unsigned *wt = reinterpret_cast<unsigned *>(wt16);
    u16 *stage = reinterpret_cast<u16 *>(smem + (size_t)(E + 1) * nl * 2 + (size_t)nl * 4);
    u64 *scr = reinterpret_cast<u64 *>(stage);        // [0] workgroup key, [2..17] exchange candidates (two sets in turn)
    int *scr32 = reinterpret_cast<int *>(stage);      // [40..47] wave minima
    u16 *age16 = stage + max(nl, 128);                // TABU: iterations since the node at the cell was moved (0xFFFF: never)
    constexpr int DINF = 0x7fffffff;
    const int k0 = SH ? wg * E : min(wg * E, n - E);  // own edges: array cells k0 .. k0+E-1 (the last workgroup overlaps its neighbour:
                                                      // a pair found twice is found with the same key); own rows: cells k0 .. k0+E
    const int m0 = tid * 8;                           // the 8 array cells this thread evaluates against every own edge
    const bool act = m0 < nl;
    const int mex = m0 + 8 >= nl ? 0 : m0 + 8;        // cell behind the chunk (cell n == cell 0: kept as a copy when n < nl)

    auto give_up = [&](int status) __attribute__((always_inline)) {
        if (tid == 0) {
            atomicCAS(A.ctl + 1, LP_ST_RUNNING, status);
            __hip_atomic_store(A.ctl, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    // One grid-wide exchange: lanes with `have` publish (w0, w1) as this workgroup's record of step s (duplicates must be
    // bit-identical); returns the record with the smallest 60-bit key over all workgroups, 0 when the exchange failed.
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
        const int wv = tid >> 6, nwp = (W + 63) >> 6;
        u64 *cand = scr + 2 + (s & 1) * 8;            // (two sets in turn: the next exchange does not wait for this one's readers)
        if (wv < nwp && (long long)a == wm) { cand[2 * wv] = a; cand[2 * wv + 1] = b; }
        __syncthreads();
        u64 x0, x1;
        if constexpr (SH) {
            // every wave's candidate in one 16-byte read of its own, all in flight together; the minimum is taken in registers
            constexpr int NWP = (WC + 63) >> 6;
            v4u32 c[NWP];
#pragma unroll
            for (int i = 0; i < NWP; i++) c[i] = *reinterpret_cast<const v4u32 *>(cand + 2 * i);
            x0 = c[0].x | (u64)c[0].y << 32; x1 = c[0].z | (u64)c[0].w << 32;
#pragma unroll
            for (int i = 1; i < NWP; i++) {
                const u64 y0 = c[i].x | (u64)c[i].y << 32, y1 = c[i].z | (u64)c[i].w << 32;
                const bool lt = y0 < x0;
                x0 = lt ? y0 : x0; x1 = lt ? y1 : x1;
            }
        } else {
            x0 = cand[0]; x1 = cand[1];
            for (int i = 1; i < nwp; i++) { const u64 y = cand[2 * i]; if (y < x0) { x0 = y; x1 = cand[2 * i + 1]; } }
        }
        r0 = ((u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(x0 >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)x0);
        r1 = ((u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(x1 >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)x1);
    };

    // ---- rendezvous: is the whole grid resident?
    u64 r0, r1;
    exchange(0, tid == 0 && (A.hello_ticks > 0 || wg != 0), 1ull << 24, 0, r0, r1, A.hello_ticks > 0 ? A.hello_ticks : -A.hello_ticks);
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
        for (int q = tid; q < nl; q += BT) {
            const int src = q < n ? q : (q == n ? 0 : -1);
            const unsigned lab = src >= 0 ? (unsigned)ord[src] : 0u, w = src >= 0 ? (unsigned)dp[src] : 0u;
            wt[q] = (w & 0xffffu) | (lab << 16);
            if constexpr (TABU) age16[q] = 0xFFFFu;  // tabu_init: nobody is tabu (metaheuristic.c:65-84)
        }
    }
    __syncthreads();

    // (re)load the rows of the own cells in `need` (bit r = cell k0 + r): every row requested at once (coalesced), then one
    // after the other written to an LDS buffer in node order and gathered into tour order by the labels.  Two buffers
    // in turn -- the staging row and the LDS row of the LAST cell to be loaded (free until its own turn, which takes the
    // staging row) -- so that one barrier per row is enough.
    auto reload = [&](unsigned need) __attribute__((always_inline)) {
        const int lane = tid & 63;
        int oc = k0 + min(lane, E); LP_WRAP_HI(oc);
        const unsigned ownlab = wt16[2 * oc + 1];                  // lane r: the node at the own cell r
        unsigned offs[8];                                          // byte offsets of the own chunk's labels in a node-order row
        if (act) {
            const v4u32 la = *reinterpret_cast<const v4u32 *>(wt + m0), lb = *reinterpret_cast<const v4u32 *>(wt + m0 + 4);
            offs[0] = la.x >> 16 << 1; offs[1] = la.y >> 16 << 1; offs[2] = la.z >> 16 << 1; offs[3] = la.w >> 16 << 1;
            offs[4] = lb.x >> 16 << 1; offs[5] = lb.y >> 16 << 1; offs[6] = lb.z >> 16 << 1; offs[7] = lb.w >> 16 << 1;
        }
        v4u32 R[EMAX + 1];
#pragma unroll
        for (int r = 0; r <= EMAX; r++) {
            if ((need >> r) & 1) {
                const int x = __builtin_amdgcn_readlane((int)ownlab, r);
                if (act) R[r] = *reinterpret_cast<const v4u32 *>(A.mat + (size_t)x * ld + m0);
            }
        }
        // (shaped form: the row mask is opaque from here on, so that its bits are tested again where the rows are written and
        // not kept as 17 lane masks across the loads)
        if constexpr (SH && !TM) asm volatile("" : "+s"(need));
        const int last = 31 - __builtin_clz(need);
        int left = __builtin_popcount(need);                       // rows still to be written to a buffer
        unsigned char *bufT = reinterpret_cast<unsigned char *>(rows + (size_t)last * nl);
        unsigned char *bufS = reinterpret_cast<unsigned char *>(stage);
        unsigned char *bprev = nullptr;
        int rprev = 0;
        auto gather = [&](const unsigned char *buf, int rdst) __attribute__((always_inline)) {
            if (act) {
                unsigned g[8];
#pragma unroll
                for (int v = 0; v < 8; v++) g[v] = *reinterpret_cast<const u16 *>(buf + offs[v]);
                const v4u32 out = {g[0] | g[1] << 16, g[2] | g[3] << 16, g[4] | g[5] << 16, g[6] | g[7] << 16};
                *reinterpret_cast<v4u32 *>(rows + (size_t)rdst * nl + m0) = out;
            }
        };
#pragma unroll
        for (int r = 0; r <= EMAX; r++) {
            if ((need >> r) & 1) {
                const unsigned x = (unsigned)__builtin_amdgcn_readlane((int)ownlab, r);
                unsigned char *buf = (left & 1) ? bufS : bufT;     // the last row (left == 1) takes the staging row
                left--;
                if (act) {
                    v4u32 v = R[r];
                    if ((int)(x >> 3) == tid) {                    // the diagonal cell: poisoned (delta(k, k) can never win)
                        const unsigned sel = (x & 7u) >> 1;
                        unsigned c[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                        for (int q = 0; q < 4; q++)
                            if ((unsigned)q == sel) c[q] = (x & 1u) ? (c[q] & 0xffffu) | (POISON << 16) : (c[q] & 0xffff0000u) | POISON;
                        v = v4u32{c[0], c[1], c[2], c[3]};
                    }
                    *reinterpret_cast<v4u32 *>(buf + (size_t)m0 * 2) = v;
                }
                if (bprev) gather(bprev, rprev);
                __syncthreads();
                bprev = buf; rprev = r;
            }
        }
        gather(bprev, rprev);
        __syncthreads();
        if constexpr (TABU) {                         // the cells of the node's two tour neighbours (the own cell came poisoned)
            if (tid <= E && ((need >> tid) & 1)) {
                int p = k0 + tid; if (p >= n) p -= n;
                int pl = p - 1; if (pl < 0) pl += n;
                int pr = p + 1; if (pr == n) pr = 0;
                rows[(size_t)tid * nl + pl] = (u16)POISON; rows[(size_t)tid * nl + pr] = (u16)POISON;
                if (n < nl && (pl == 0 || pr == 0)) rows[(size_t)tid * nl + n] = (u16)POISON;
            }
            __syncthreads();
        }
    };
    const unsigned allrows = (2u << E) - 1u;
    reload(allrows);
    // TM: the descriptor of A.tmat (out-of-range offsets are dropped by the hardware), built where it is used from the
    // kernel arguments where they lie (see the tour state's write-back below): nothing of it lives across the sweep loop
    auto tm_rsrc = [&]() __attribute__((always_inline)) {
        c_PersistArgs *Ak = (c_PersistArgs *)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(Ak));
        return __builtin_amdgcn_make_buffer_rsrc(Ak->tmat, 0, NLC * NLC * 2, 0x00020000);
    };
    constexpr int TM_SC1 = 16;                        // (the cache-policy word of the buffer builtins: agent scope)
    if constexpr (TM) {                               // fill: the own rows 0 .. E-1 as they lie in LDS
        const auto rs = tm_rsrc();
#pragma unroll 4
        for (int i = tid; i < EC * (NLC / 8); i += BT) {
            const int row = i / (NLC / 8), c = i & (NLC / 8 - 1);
            const unsigned x = wt16[2 * (k0 + row) + 1];
            const v4u32 v = *reinterpret_cast<const v4u32 *>(rows + (size_t)row * NLC + 8 * c);
            __builtin_amdgcn_raw_buffer_store_b128(v, rs, (int)((x * NLC + 8 * c) * 2), 0, TM_SC1);
        }
    }
    // TM: the rows in `need` behind the move that reversed [lo, lo + M) -- labels, edge costs and the rows that stay are final
    // (tidv: the thread index, opaque inside a sweep -- LP_TID -- so that the lane masks of the cell-by-cell pass are computed here)
    auto fetch_tm = [&](unsigned need, int lo, int M, int tidv) __attribute__((always_inline)) {
        if constexpr (!TM) return;
        const auto rs = tm_rsrc();
        const int lane = tid & 63;
        const unsigned ownlab = wt16[2 * ((k0 + min(lane, EC)) & (NLC - 1)) + 1];      // lane r: the node at the own cell r
        int start = 0;
        const int cls = act ? lds_tmat::chunk_class(m0, lo, M, NLC, start) : (int)lds_tmat::CELLWISE;
        v4u32 R[EC > 0 ? EC : 1], Rc = {0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < EC; r++)                  // (every thread loads: a chunk that goes cell by cell is loaded and dropped)
            if ((need >> r) & 1)
                R[r] = __builtin_amdgcn_raw_buffer_load_b128(rs, start * 2, __builtin_amdgcn_readlane((int)ownlab, r) * (NLC * 2), TM_SC1);
        asm volatile("" : "+s"(need));                // (as in reload(): the bits are tested again where the rows are written)
        const bool copy = (need >> EC) & 1;
        const unsigned xc = (unsigned)__builtin_amdgcn_readlane((int)ownlab, EC);
        if (copy && act) {                            // (matrix and stride from the kernel arguments as well; xc * ld < 2^32)
            c_PersistArgs *Ak = (c_PersistArgs *)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(Ak));
            Rc = *reinterpret_cast<const v4u32 *>(Ak->mat + (size_t)(xc * (unsigned)Ak->ld) + m0);
        }
        // the cells of the three chunks that may not go whole: 24 lanes a row
        int cw[3];
        lds_tmat::cellwise_chunks(lo, M, NLC, cw);
        const int sr = tidv / 24, si = tidv - sr * 24;
        const bool sact = sr < EC && ((need >> sr) & 1);
        const int sq = (si < 8 ? cw[0] : si < 16 ? cw[1] : cw[2]) * 8 + (si & 7);
        const unsigned sx = wt16[2 * (k0 + min(sr, EC - 1)) + 1];
        const u16 sv = __builtin_amdgcn_raw_buffer_load_b16(rs, (int)((sx * NLC + lds_tmat::src_cell(sq, lo, M, NLC)) * 2), 0, TM_SC1);
#pragma unroll
        for (int r = 0; r < EC; r++) {
            if ((need >> r) & 1) {
                const v4u32 v = R[r];
                const v4u32 m = {__builtin_amdgcn_alignbit(v.w, v.w, 16), __builtin_amdgcn_alignbit(v.z, v.z, 16),
                                 __builtin_amdgcn_alignbit(v.y, v.y, 16), __builtin_amdgcn_alignbit(v.x, v.x, 16)};
                if (cls != lds_tmat::CELLWISE) *reinterpret_cast<v4u32 *>(rows + (size_t)r * NLC + m0) = cls == lds_tmat::MIRROR ? m : v;
            }
        }
        if (sact) rows[(size_t)sr * NLC + sq] = sv;
        // (the cell's load has landed in EVERY lane from here on: a load left pending in the idle lanes would make the compiler
        // wait for all memory operations -- the write-back's stores among them -- where its register is used next)
        asm volatile("" :: "v"((unsigned)sv));
        if (copy) {                                 // as reload(): in node order to the staging row, gathered by the labels
            if (act) {
                v4u32 v = Rc;
                if ((int)(xc >> 3) == tid) {
                    const unsigned sel = (xc & 7u) >> 1;
                    unsigned c[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        if ((unsigned)q == sel) c[q] = (xc & 1u) ? (c[q] & 0xffffu) | (POISON << 16) : (c[q] & 0xffff0000u) | POISON;
                    v = v4u32{c[0], c[1], c[2], c[3]};
                }
                *reinterpret_cast<v4u32 *>(stage + m0) = v;
            }
            __syncthreads();
            if (act) {
                const v4u32 la = *reinterpret_cast<const v4u32 *>(wt + m0), lb = *reinterpret_cast<const v4u32 *>(wt + m0 + 4);
                const unsigned l[8] = {la.x >> 16, la.y >> 16, la.z >> 16, la.w >> 16, lb.x >> 16, lb.y >> 16, lb.z >> 16, lb.w >> 16};
                unsigned g[8];
#pragma unroll
                for (int v = 0; v < 8; v++) g[v] = stage[l[v]];
                const v4u32 out = {g[0] | g[1] << 16, g[2] | g[3] << 16, g[4] | g[5] << 16, g[6] | g[7] << 16};
                *reinterpret_cast<v4u32 *>(rows + (size_t)EC * NLC + m0) = out;
            }
        }
        __syncthreads();
    };
    // TM: behind the move, the chunks of the rows 0 .. E-1 that overlap the reversed range, from LDS to the rows' nodes in tmat
    // (2^lg >= the chunk count threads a row, 512 >> lg rows a pass)
    auto write_back_tm = [&](int lo, int M, int tidv) __attribute__((always_inline)) {
        if constexpr (!TM) return;
        const auto rs = tm_rsrc();
        const int nch = lds_tmat::wb_count(lo, M), c0 = lds_tmat::wb_first(lo);
        const int lg = nch > 1 ? 32 - __builtin_clz(nch - 1) : 0;
        const int j = tidv & ((1 << lg) - 1), rpi = BT >> lg;
        if (j < nch) {
            const int c = (c0 + j) & (NLC / 8 - 1);
            for (int row = tidv >> lg; row < EC; row += rpi) {
                const unsigned x = wt16[2 * (k0 + row) + 1];
                const v4u32 v = *reinterpret_cast<const v4u32 *>(rows + (size_t)row * NLC + 8 * c);
                __builtin_amdgcn_raw_buffer_store_b128(v, rs, (int)((x * NLC + 8 * c) * 2), 0, TM_SC1);
            }
        }
    };

    int status = LP_ST_RUNNING;
    if (cap >= 0 && kd >= cap) status = LP_ST_CAPPED;        // (cap 0: not one sweep)
    int tenure = A.tenure0, tup = A.up0, iters = 0;          // TABU
    double best = A.best0;
    if (TABU && A.tabu_k <= 0) status = LP_ST_CAPPED;
    // VNS (not TABU): iteration counter, numbers consumed, and the loop body behind a local optimum
    int vit = A.vns_it0, vcur = 0;
    u16 *vns_lab = rows;                              // (row 0: loaded again behind the kicks)
    auto vns_mirror = [&]() __attribute__((always_inline)) { if (n < nl && tid == 0) wt[n] = wt[0]; };
#include "tspgpu_lds_vns.inc"
    if constexpr (VNS) {
        if (A.vns_phase == 1 && status == LP_ST_RUNNING) {
            const int st = vns_step(false);
            if (st != LP_ST_RUNNING) status = st;
        }
    }
    auto tabu_edge = [&](int q) __attribute__((always_inline)) {      // one of the two nodes of the edge at cell q is tabu
        int q1 = q + 1; if (q1 >= n) q1 -= n;
        return (int)age16[q] < tenure || (int)age16[q1] < tenure;    // is_tabu, metaheuristic.c:416-418 (age = iter - tabu_list[node])
    };
    // phase clocks (TSPGPU_OPT_STAMPS): thread 0 of every workgroup sums wall-clock ticks per phase
    [[maybe_unused]] unsigned long long ph[6] = {0, 0, 0, 0, 0, 0}, nreload = 0, nrows = 0, ph2[4] = {0, 0, 0, 0};
    bool clk = false;
    if constexpr (CLOCKS) clk = A.stamps != nullptr && tid == 0;
    [[maybe_unused]] unsigned long long tc = clk ? wall_clock64() : 0ull;
#define LP_PHASE2(i) do { if constexpr (CLOCKS) if (clk) { const unsigned long long now_ = wall_clock64(); ph2[i] += now_ - tc; tc = now_; } } while (0)
#define LP_PHASE(i) do { if constexpr (CLOCKS) if (clk) { const unsigned long long now_ = wall_clock64(); ph[i] += now_ - tc; tc = now_; } } while (0)
    // Evaluation geometry (the same every sweep).  A pair of tour edges {k, m} has two owners; with n a multiple of 16 it is
    // evaluated by ONE of them -- the owner of k takes the m at most n/2 cells ahead of k -- which halves the arithmetic:
    // the thread owns one 8-cell chunk out of the n/16 chunks ahead of its half of the own edges (threads [0, n/16): the
    // first half of the edges, [n/16, n/8): the second), and the two chunks per edge the halves do not reach are taken
    // by 2E lanes, one (edge, chunk) each.  Chunks are whole, so some pairs are still seen twice: with the same key.
    // For other n up to 4047 the same split with a window of n/16 + 4 chunks per half: enough for the n/2 cells ahead of
    // any of the half's edges whatever the alignment and the padding of the last chunk, no (edge, chunk) lanes needed.
    // Otherwise (one edge per workgroup, or 4048 <= n < 4096 with n % 16 != 0) thread t takes chunk t against every own edge.
    const bool once = (n & 15) == 0 && E >= 2;
    const int C = nl >> 3, a0 = k0 & 7, cb = k0 >> 3, Ea = (E + 1) >> 1;
    const bool once2 = !once && E >= 2 && 2 * ((n >> 4) + 4) <= BT && (n >> 4) + 4 <= C;
    const int H = once ? C >> 1 : (n >> 4) + 4;
    int me0 = m0, rlo = 0, rcnt = E;
    bool eact = act;
    if (once || once2) {
        const int h = tid >= H ? 1 : 0;
        rlo = h ? Ea : 0; rcnt = h ? E - Ea : Ea;
        int ch = cb + ((a0 + rlo + 1) >> 3) + (tid - h * H); if (ch >= C) ch -= C;
        me0 = ch * 8; eact = tid < 2 * H;
    }
    const int mexe = me0 + 8 >= nl ? 0 : me0 + 8;     // cell behind the chunk (cell n == cell 0: kept as a copy when n < nl)
    const bool lact = once && tid < 2 * E;            // lane pair (edge lr, the two chunks behind its half's n/16)
    int lr = 0, lm0 = 0, lmex = 0;
    if (lact) {
        lr = tid >> 1;
        int ch = cb + ((a0 + (lr >= Ea ? Ea : 0) + 1) >> 3) + H + (tid & 1); if (ch >= C) ch -= C;
        lm0 = ch * 8; lmex = lm0 + 8 >= nl ? 0 : lm0 + 8;
    }
    const u16 *rchunk = rows + (size_t)rlo * nl + me0;     // this thread's 8 cells of its first row
    const u16 *rex = rows + (size_t)rlo * nl + mexe;       // ... and the cell behind them
    while (status == LP_ST_RUNNING) {
        // shaped form: the thread index is opaque inside a sweep (LP_TID), so that the lane masks and small indices derived
        // from it are computed where they are used (one compare each) and not held in scalar registers across the whole loop
        int tid_sweep = 0;
        int lm0_sweep = 0;                            // (likewise the first cell of the lane's (edge, chunk) item: LP_LM0)
        if constexpr (SH) { tid_sweep = tid; lm0_sweep = lm0; asm volatile("" : "+v"(tid_sweep), "+v"(lm0_sweep)); }
        // ---- evaluation: for each of the 8 own columns the minimum over the thread's own edges of
        // G_k[m] + G_{k+1}[m+1] - w[k] (one row ahead in registers: the next row's loads are in flight under this row's arithmetic)
        int col[8], lcol[8];
        int tmin = 0x7fffffff;
        unsigned etmask = 0;                          // TABU: bit r = the own edge k0 + r has a tabu node
        if constexpr (TABU) {
            const int r = tid & 63;
            etmask = (unsigned)__ballot(r < E && tabu_edge(k0 + min(r, E - 1)));
        }
        unsigned pacc[4] = {0, 0, 0, 0};              // shaped form: the 8 columns' minima, packed, w[m] subtracted
        if constexpr (SH) {
            // EC/2 rows, unrolled: row r of the half lies r * NLC cells behind rchunk (an immediate offset), the half's w[k] are
            // EC/2 consecutive words of wt.  Every thread is active or idle for good (n == nl: no padding cell, no mirror).
            constexpr int RC = EC / 2;
            if (NLC / 8 >= BT || eact) {
                unsigned wkw[RC];
                {
                    const unsigned *wp = wt + k0 + rlo;           // (k0 and rlo are multiples of EC/2 words)
                    if constexpr (RC % 4 == 0) {
#pragma unroll
                        for (int q = 0; q < RC / 4; q++) {
                            const v4u32 w4 = *reinterpret_cast<const v4u32 *>(wp + 4 * q);
                            wkw[4 * q] = w4.x; wkw[4 * q + 1] = w4.y; wkw[4 * q + 2] = w4.z; wkw[4 * q + 3] = w4.w;
                        }
                    } else if constexpr (RC % 2 == 0) {
#pragma unroll
                        for (int q = 0; q < RC / 2; q++) {
                            const u64 w2 = *reinterpret_cast<const u64 *>(wp + 2 * q);
                            wkw[2 * q] = (unsigned)w2; wkw[2 * q + 1] = (unsigned)(w2 >> 32);
                        }
                    } else {
#pragma unroll
                        for (int q = 0; q < RC; q++) wkw[q] = wp[q];
                    }
                }
                // The deltas are carried with a bias of 0x8000 a half: acc = min(X + Y + (0x8000 - w[k])), one three-operand 32-bit
                // add a register.  Every cost <= 16383 (the poison included): a half of the sum lies in [16385, 65534], so no
                // carry crosses the halves and the UNSIGNED packed minimum orders the halves as the signed one orders the deltas.
                unsigned acc[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
                v4u32 X = *reinterpret_cast<const v4u32 *>(rchunk);
                v4u32 Xn = *reinterpret_cast<const v4u32 *>(rchunk + NLC);
                unsigned exn = rex[NLC];
#pragma unroll
                for (int r = 0; r < RC; r++) {
                    const v4u32 Xc = Xn;
                    const unsigned exc = exn;
                    if (r + 1 < RC) {                             // (one row ahead: the loads fly under this row's arithmetic)
                        Xn = *reinterpret_cast<const v4u32 *>(rchunk + (size_t)(r + 2) * NLC);
                        exn = rex[(size_t)(r + 2) * NLC];
                    }
                    const unsigned Y[4] = {__builtin_amdgcn_alignbit(Xc.y, Xc.x, 16), __builtin_amdgcn_alignbit(Xc.z, Xc.y, 16),
                                           __builtin_amdgcn_alignbit(Xc.w, Xc.z, 16), __builtin_amdgcn_alignbit(exc, Xc.w, 16)};
                    const unsigned Xa[4] = {X.x, X.y, X.z, X.w};
                    const unsigned bk = lp_pk_bias(wkw[r]);       // 0x8000 - w[k] in both halves (lds_tmat::pk_bias)
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[j] = lp_pk_minu(acc[j], lds_tmat::pk_biased(Xa[j], Y[j], bk));
                    X = Xc;
                }
                // - w[m], still packed (a half stays in [2, 65534]: no borrow), and the bias taken off: the signed packed deltas
                // (|delta| <= 2 * 16383: no 16-bit overflow); unpacked only where the minimum turns out to be
                const v4u32 wa = *reinterpret_cast<const v4u32 *>(wt + me0), wb = *reinterpret_cast<const v4u32 *>(wt + me0 + 4);
                pacc[0] = lp_pk_sub(acc[0], __builtin_amdgcn_perm(wa.y, wa.x, 0x05040100u)) ^ lds_tmat::PK_BIAS;
                pacc[1] = lp_pk_sub(acc[1], __builtin_amdgcn_perm(wa.w, wa.z, 0x05040100u)) ^ lds_tmat::PK_BIAS;
                pacc[2] = lp_pk_sub(acc[2], __builtin_amdgcn_perm(wb.y, wb.x, 0x05040100u)) ^ lds_tmat::PK_BIAS;
                pacc[3] = lp_pk_sub(acc[3], __builtin_amdgcn_perm(wb.w, wb.z, 0x05040100u)) ^ lds_tmat::PK_BIAS;
                const unsigned pm = lp_pk_min(lp_pk_min(pacc[0], pacc[1]), lp_pk_min(pacc[2], pacc[3]));
                tmin = min((int)(short)(pm & 0xffffu), (int)pm >> 16);
            }
        } else
        if (eact) {
            unsigned acc[4] = {0x7fff7fffu, 0x7fff7fffu, 0x7fff7fffu, 0x7fff7fffu};
#pragma unroll
            for (int v = 0; v < 8; v++) col[v] = 0x7fffffff;
            v4u32 X = *reinterpret_cast<const v4u32 *>(rchunk);
            v4u32 Xn = *reinterpret_cast<const v4u32 *>(rchunk + nl);
            unsigned exn = rex[nl];
            unsigned wk = wt16[2 * (k0 + rlo)];
            for (int r = 0; r < rcnt; r++) {
                const v4u32 Xc = Xn;
                const unsigned exc = exn, wkc = wk;
                const int rn = min(r + 2, rcnt);
                Xn = *reinterpret_cast<const v4u32 *>(rchunk + (size_t)rn * nl);
                exn = rex[(size_t)rn * nl];
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
            const v4u32 wa = *reinterpret_cast<const v4u32 *>(wt + me0), wb = *reinterpret_cast<const v4u32 *>(wt + me0 + 4);
            const unsigned wm[8] = {wa.x & 0xffffu, wa.y & 0xffffu, wa.z & 0xffffu, wa.w & 0xffffu,
                                    wb.x & 0xffffu, wb.y & 0xffffu, wb.z & 0xffffu, wb.w & 0xffffu};
            unsigned tabm = 0;                        // TABU: bit v = the edge at cell me0 + v has a tabu node
            if constexpr (TABU) {
                const v4u32 ag = *reinterpret_cast<const v4u32 *>(age16 + me0);
                const unsigned agx = age16[mexe];
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
                if (me0 + v >= n) col[v] = 0x7fffffff;
                tmin = min(tmin, col[v]);
            }
        }
        if (lact) {                                   // the (edge, chunk) items the halves do not reach: one per lane
            const u16 *ra = rows + (size_t)lr * nl;
            const v4u32 Xa4 = *reinterpret_cast<const v4u32 *>(ra + LP_LM0), Xb4 = *reinterpret_cast<const v4u32 *>(ra + nl + LP_LM0);
            const unsigned exb = ra[nl + lmex];
            const int wkl = (int)wt16[2 * (k0 + lr)];
            const v4u32 wa = *reinterpret_cast<const v4u32 *>(wt + LP_LM0), wb = *reinterpret_cast<const v4u32 *>(wt + LP_LM0 + 4);
            const unsigned xs[9] = {Xb4.x & 0xffffu, Xb4.x >> 16, Xb4.y & 0xffffu, Xb4.y >> 16, Xb4.z & 0xffffu, Xb4.z >> 16,
                                    Xb4.w & 0xffffu, Xb4.w >> 16, exb};
            const unsigned as[8] = {Xa4.x & 0xffffu, Xa4.x >> 16, Xa4.y & 0xffffu, Xa4.y >> 16, Xa4.z & 0xffffu, Xa4.z >> 16,
                                    Xa4.w & 0xffffu, Xa4.w >> 16};
            const unsigned wm[8] = {wa.x & 0xffffu, wa.y & 0xffffu, wa.z & 0xffffu, wa.w & 0xffffu,
                                    wb.x & 0xffffu, wb.y & 0xffffu, wb.z & 0xffffu, wb.w & 0xffffu};
            unsigned ltab = 0;
            if constexpr (TABU) {
                const v4u32 ag = *reinterpret_cast<const v4u32 *>(age16 + lm0);
                const unsigned agx = age16[lmex];
                const unsigned a9[9] = {ag.x & 0xffffu, ag.x >> 16, ag.y & 0xffffu, ag.y >> 16, ag.z & 0xffffu, ag.z >> 16,
                                        ag.w & 0xffffu, ag.w >> 16, agx};
#pragma unroll
                for (int v = 0; v < 8; v++) ltab |= (((int)a9[v] < tenure || (int)a9[v + 1] < tenure) ? 1u : 0u) << v;
                if ((etmask >> lr) & 1) ltab = 0xffu;
            }
#pragma unroll
            for (int v = 0; v < 8; v++) {
                lcol[v] = (int)as[v] + (int)xs[v + 1] - wkl - (int)wm[v];
                if constexpr (TABU) { if (as[v] == POISON || ((ltab >> v) & 1)) lcol[v] = DINF; }
                tmin = min(tmin, lcol[v]);
            }
        }
        LP_PHASE(0);                                  // evaluation
        const int wmin = wave_min_i32(tmin);
        if ((LP_TID & 63) == 0) scr32[40 + (LP_TID >> 6)] = wmin;
        if (LP_TID == 0) scr[0] = ~0ull;
        __syncthreads();
        int dmin = scr32[40];
#pragma unroll
        for (int i = 1; i < BT / 64; i++) dmin = min(dmin, scr32[40 + i]);
        dmin = __builtin_amdgcn_readfirstlane(dmin);
        // ---- the workgroup's best pair in the reference's order: smallest delta, then smallest a, then smallest b.
        // The wave that holds a column with the minimum resolves it together: lane r takes the r-th edge of the column's
        // thread; the (edge, chunk) lanes resolve their own item.
        u64 mykey = ~0ull, mypay = 0;
        const bool found = TABU ? dmin < DINF : dmin < 0;      // (tabu_best_move takes the best admissible pair whatever its sign)
        if (found) {
            auto offer = [&](int k, int m, unsigned xa, unsigned yb) __attribute__((always_inline)) {
                const int kp = LP_WRAP_EQ(k + 1), mp = LP_WRAP_EQ(m + 1);
                const unsigned lk = dir > 0 ? wt16[2 * k + 1] : wt16[2 * kp + 1];
                const unsigned lm = dir > 0 ? wt16[2 * m + 1] : wt16[2 * mp + 1];
                const unsigned la = min(lk, lm), lb = max(lk, lm);
                const u64 key = ((u64)(unsigned)(dmin + LP_DBIAS) << 24) | ((u64)la << 12) | lb;
                if (key < mykey) {
                    mykey = key;
                    const unsigned e1 = (unsigned)min(k, m), e2 = (unsigned)max(k, m);
                    const unsigned l1 = k < m ? lk : lm;          // label of the edge at the smaller cell
                    mypay = ((u64)(l1 == la ? 1u : 0u) << 56) | ((u64)e1 << 44) | ((u64)e2 << 32) | ((u64)xa << 16) | yb;
                }
            };
            if (lact) {
#pragma unroll
                for (int v = 0; v < 8; v++) {
                    if (lcol[v] == dmin) {
                        const int m = LP_LM0 + v, mp = LP_WRAP_EQ(m + 1);
                        offer(k0 + lr, m, rows[(size_t)lr * nl + m], rows[(size_t)(lr + 1) * nl + mp]);
                    }
                }
            }
            unsigned cm = 0;
            if (eact && tmin == dmin) {
#pragma unroll
                for (int v = 0; v < 8; v++) {
                    if constexpr (SH) col[v] = (v & 1) ? ((int)pacc[v >> 1] >> 16) : (int)(short)(pacc[v >> 1] & 0xffffu);
                    cm |= (col[v] == dmin ? 1u : 0u) << v;
                }
            }
            unsigned long long ball = __ballot(cm != 0);
            const int lane = LP_TID & 63;
            while (ball) {
                const int src = __builtin_ctzll(ball);
                ball &= ball - 1;
                unsigned cms = (unsigned)__builtin_amdgcn_readlane((int)cm, src);
                const int m0s = __builtin_amdgcn_readlane(me0, src);
                const int rlos = __builtin_amdgcn_readlane(rlo, src), rcnts = __builtin_amdgcn_readlane(rcnt, src);
                while (cms) {
                    const int v = __builtin_ctz(cms);
                    cms &= cms - 1;
                    const int m = m0s + v, mp = LP_WRAP_EQ(m + 1);
                    if (lane < rcnts) {
                        const int r = rlos + lane, k = k0 + r;
                        const unsigned xa = rows[(size_t)r * nl + m], yb = rows[(size_t)(r + 1) * nl + mp];
                        const int d = (int)xa + (int)yb - (int)wt16[2 * k] - (int)wt16[2 * m];
                        bool ok = d == dmin;
                        if constexpr (TABU) ok = ok && xa != POISON && !((etmask >> r) & 1);
                        if (ok) offer(k, m, xa, yb);
                    }
                }
            }
            if (mykey != ~0ull) __hip_atomic_fetch_min(&scr[0], mykey, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        // TM: every thread's stores to tmat (the fill, the last move's write-back) acknowledged before the record goes out
        if constexpr (TM) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const u64 kmin = scr[0];
        const bool have = found ? mykey == kmin : LP_TID == 0;
        LP_PHASE(1);                                  // workgroup reduction + tie order
        // ---- exchange
        sdone++;
        exchange(sdone, have, found ? mykey : LP_NONE, mypay, r0, r1, A.spin_ticks);
        if (r0 == 0) { give_up(LP_ST_LOST); return; }
        LP_PHASE(2);                                  // exchange
        kd++;
        const bool nomove = (r0 >> 24) == 0xFFFFFFFFFull;
        if (nomove && !TABU) {                        // the final, non-improving sweep
            lastd = 0;
            if (wg == 0 && LP_TID == 0 && t == 0 && kd <= A.hist.cap) { A.hist.a[kd - 1] = -1; A.hist.b[kd - 1] = -1; A.hist.d[kd - 1] = 0.0; }
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
        const int d = (int)((r0 >> 24) & 0x3FFFFu) - LP_DBIAS;
        const int la = (int)((r0 >> 12) & 0xfffu), lb = (int)(r0 & 0xfffu);
        const int e1 = (int)((r1 >> 44) & 0xfffu), e2 = (int)((r1 >> 32) & 0xfffu);
        const unsigned wTT = (unsigned)((r1 >> 16) & 0xffffu), wHH = (unsigned)(r1 & 0xffffu);
        const bool e1_is_a = (r1 >> 56) & 1;
        sumd += d; lastd = d;
        if (wg == 0 && LP_TID == 0 && t == 0 && kd <= A.hist.cap) { A.hist.a[kd - 1] = la; A.hist.b[kd - 1] = lb; A.hist.d[kd - 1] = (double)d; }

        // ---- the move as an array operation (see Tours): ref_reverse_path flips the arc succ a .. b; flipping the other
        // arc and toggling dir gives the same successor function, so the shorter arc [lo, lo+M) is reversed
        const int ea = e1_is_a ? e1 : e2, eb = e1_is_a ? e2 : e1;
        const int s1 = dir > 0 ? ea : eb, s2 = dir > 0 ? eb : ea;
        int L = s2 - s1; LP_WRAP_LO(L);
        const bool other = n - L < L;
        const int M = other ? n - L : L;
        int lo = (other ? s2 : s1) + 1; LP_WRAP_EQS(lo);
        if (other) dir = -dir;
        int eTT = lo - 1; LP_WRAP_LO(eTT);          // the edge in front of the range joins the two tails,
        int eHH = lo + M - 1; LP_WRAP_HI(eHH);     // the edge at its last cell the two heads
        const int hs = M >> 1, hw = (M - 1) >> 1, nrow = E + 1;
        unsigned wOldTT = 0, wOldHH = 0;              // TABU: the costs of the two edges the move removes (for the poison patches)
        if constexpr (TABU) {
            wOldTT = wt16[2 * eTT]; wOldHH = wt16[2 * eHH];
            __syncthreads();                          // (read by every wave before the last thread writes the new costs)
        }
        LP_PHASE2(0);
        // own cells inside the range hold other nodes afterwards: a row whose node stays among the own cells changes places
        // with its mirror row (each thread its own 16 bytes of both), the others are fetched (and are not reversed first).
        // Lane r looks at the own cell r (every wave computes the same words).
        unsigned need = 0, swp = 0;                   // swp bit r: row r changes places with the row mirv (lane r) above it
        int mirv = 0;
        {
            int off = k0 - lo; LP_WRAP_LO(off);
            if (off < M || off + E >= n) {
                const int r = LP_TID & 63;
                bool nd = false, sw = false;
                if (r <= E) {
                    int rel = off + r; LP_WRAP_HI(rel);
                    if (rel < M) {
                        int pm = lo + (M - 1 - rel); LP_WRAP_HI(pm);
                        int rm = pm - k0; LP_WRAP_LO(rm);
                        nd = rm > E; sw = !nd && rm > r; mirv = rm;
                    }
                }
                need = (unsigned)__ballot(nd); swp = (unsigned)__ballot(sw);
            }
        }
        LP_PHASE2(1);
        if (M <= 16) {
            // a short range (7 of 10 moves): every swap there is -- rows, labels, edge costs -- in one step, 8 lanes an item
            const int item = LP_TID >> 3, u = LP_TID & 7;
            u16 *base = rows + (size_t)item * nl;
            int st = 1, last = M - 1, cnt = item <= E && !((need >> item) & 1) ? hs : 0;
            if (item == E + 1) { base = wt16 + 1; st = 2; cnt = hs; }
            if (item == E + 2) { base = wt16; st = 2; last = M - 2; cnt = hw; }
            if (TABU && item == E + 3) { base = age16; st = 1; cnt = hs; }
            if (u < cnt) {
                int p1 = lo + u; LP_WRAP_HI(p1);
                int p2 = lo + last - u; LP_WRAP_HI(p2);
                const u16 x = base[p1 * st], y = base[p2 * st];
                base[p1 * st] = y; base[p2 * st] = x;
            }
        } else {
            // the swaps.  Matrix rows: 8 cells from either end of the range per item (16-byte LDS accesses at 2-byte alignment:
            // gfx950 has unaligned DS access), reversed in registers; 2^lgi threads per row, two rows in flight; the up to 7
            // swaps per row left in the middle, and the labels, cell by cell.
            {
                const int I = hs >> 3;
                if (I > 0) {
                    int lgi = 0;
                    while ((1 << lgi) < I && lgi < 9) lgi++;
                    const int rpi = BT >> lgi, j0 = LP_TID & ((1 << lgi) - 1), rs0 = LP_TID >> lgi;
                    int a = lo + 8 * j0; LP_WRAP_HI(a);
                    int b = lo + M - 8 * j0 - 8; LP_WRAP_HI(b);
                    const bool wrapped = a + 8 > n || b + 8 > n;      // the item crosses the array end: cell by cell
                    for (int row0 = 0; row0 <= E; row0 += 2 * rpi) {
                        v4u32 va[2], vb[2];
                        bool ok[2];
    #pragma unroll
                        for (int q = 0; q < 2; q++) {
                            const int row = row0 + q * rpi + rs0;
                            ok[q] = row <= E && j0 < I && !((need >> row) & 1);
                            if (ok[q] && !wrapped) {
                                va[q] = *reinterpret_cast<const v4u32_a2 *>(rows + (size_t)row * nl + a);
                                vb[q] = *reinterpret_cast<const v4u32_a2 *>(rows + (size_t)row * nl + b);
                            }
                        }
    #pragma unroll
                        for (int q = 0; q < 2; q++) {
                            const int row = row0 + q * rpi + rs0;
                            if (ok[q] && !wrapped) {
                                const v4u32 ra = {__builtin_amdgcn_alignbit(vb[q].w, vb[q].w, 16), __builtin_amdgcn_alignbit(vb[q].z, vb[q].z, 16),
                                                  __builtin_amdgcn_alignbit(vb[q].y, vb[q].y, 16), __builtin_amdgcn_alignbit(vb[q].x, vb[q].x, 16)};
                                const v4u32 rb = {__builtin_amdgcn_alignbit(va[q].w, va[q].w, 16), __builtin_amdgcn_alignbit(va[q].z, va[q].z, 16),
                                                  __builtin_amdgcn_alignbit(va[q].y, va[q].y, 16), __builtin_amdgcn_alignbit(va[q].x, va[q].x, 16)};
                                *reinterpret_cast<v4u32_a2 *>(rows + (size_t)row * nl + a) = ra;
                                *reinterpret_cast<v4u32_a2 *>(rows + (size_t)row * nl + b) = rb;
                            } else if (ok[q]) {
                                u16 *base = rows + (size_t)row * nl;
                                for (int c = 0; c < 8; c++) {
                                    int p1 = a + c; LP_WRAP_HI(p1);
                                    int p2 = b + 7 - c; LP_WRAP_HI(p2);
                                    const u16 x = base[p1], y = base[p2];
                                    base[p1] = y; base[p2] = x;
                                }
                            }
                        }
                    }
                }
                {   // the middle of every matrix row
                    const int row = LP_TID >> 3, u = 8 * I + (LP_TID & 7);
                    if (row <= E && u < hs && !((need >> row) & 1)) {
                        int p1 = lo + u; LP_WRAP_HI(p1);
                        int p2 = lo + M - 1 - u; LP_WRAP_HI(p2);
                        u16 *base = rows + (size_t)row * nl;
                        const u16 x = base[p1], y = base[p2];
                        base[p1] = y; base[p2] = x;
                    }
                }
                for (int u = LP_TID; u < hs; u += BT) {      // the labels
                    int p1 = lo + u; LP_WRAP_HI(p1);
                    int p2 = lo + M - 1 - u; LP_WRAP_HI(p2);
                    const u16 x = wt16[2 * p1 + 1], y = wt16[2 * p2 + 1];
                    wt16[2 * p1 + 1] = y; wt16[2 * p2 + 1] = x;
                }
            }
            LP_PHASE2(2);
            for (int u = LP_TID; u < hw; u += BT) {          // the M-1 edge costs inside the range
                int p1 = lo + u; LP_WRAP_HI(p1);
                int p2 = lo + M - 2 - u; LP_WRAP_HI(p2);
                const u16 x = wt16[2 * p1], y = wt16[2 * p2];
                wt16[2 * p1] = y; wt16[2 * p2] = x;
            }
            if constexpr (TABU) {
                for (int u = tid; u < hs; u += BT) {      // the ages travel with their nodes
                    int p1 = lo + u; if (p1 >= n) p1 -= n;
                    int p2 = lo + M - 1 - u; if (p2 >= n) p2 -= n;
                    const u16 x = age16[p1], y = age16[p2];
                    age16[p1] = y; age16[p2] = x;
                }
            }
        }
        if (LP_TID == BT - 1) { wt16[2 * eTT] = (u16)wTT; wt16[2 * eHH] = (u16)wHH; }
        LP_PHASE(5);                                  // (decode + own swaps, before the barrier)
        __syncthreads();
        if (swp) {
#pragma unroll
            for (int r = 0; r <= EMAX; r++) {
                if ((swp >> r) & 1) {
                    if (act) {
                        v4u32 *qa = reinterpret_cast<v4u32 *>(rows + (size_t)r * nl + m0);
                        v4u32 *qb = reinterpret_cast<v4u32 *>(rows + (size_t)__builtin_amdgcn_readlane(mirv, r) * nl + m0);
                        const v4u32 a = *qa, b = *qb;
                        *qa = b; *qb = a;
                    }
                }
            }
            __syncthreads();
        }
        if constexpr (TABU) {
            // the four nodes of the move -- now at the cells eTT, lo, eHH, eHH+1 -- are tabu from the next iteration on
            // (tabu_list[.] = iter, metaheuristic.c:236-243), and each of them has lost one tour neighbour and won one:
            // its row gets the lost neighbour's cell back (the cost of the removed edge) and the new one's cell poisoned
            int cD = eHH + 1; if (cD == n) cD = 0;
            if (tid < 4) {
                const int cell = tid == 0 ? eTT : tid == 1 ? lo : tid == 2 ? eHH : cD;
                const int back = tid == 0 ? eHH : tid == 1 ? cD : tid == 2 ? eTT : lo;      // cell that holds the lost neighbour
                const int won = tid == 0 ? lo : tid == 1 ? eTT : tid == 2 ? cD : eHH;       // cell that holds the new neighbour
                const unsigned val = (tid == 0 || tid == 2) ? wOldTT : wOldHH;
                age16[cell] = 0;
                int r = cell - k0; if (r < 0) r += n;
                if (r <= E && !((need >> r) & 1)) {
                    rows[(size_t)r * nl + back] = (u16)val;
                    rows[(size_t)r * nl + won] = (u16)POISON;
                }
            }
            __syncthreads();
        }
        if (n < nl) {                                   // cell n mirrors cell 0
            if (tid < nrow) rows[(size_t)tid * nl + n] = rows[(size_t)tid * nl];
            if (tid == nrow) wt[n] = wt[0];
            if (TABU && tid == nrow + 1) age16[n] = age16[0];
            __syncthreads();
        }
        LP_PHASE(3);                                  // reversal
        if (need) {
            if constexpr (TM) fetch_tm(need, lo, M, LP_TID); else reload(need);
            if constexpr (CLOCKS) { nreload++; nrows += __builtin_popcount(need); }
        }
        LP_PHASE(4);                                  // rows fetched
        if constexpr (TM) { write_back_tm(lo, M, LP_TID); LP_PHASE2(3); }
        if constexpr (CLOCKS) if (clk && wg == 0 && sdone < 4000) A.stamps[8192 + sdone] = ((unsigned long long)M << 48) | (wall_clock64() & 0xFFFFFFFFFFFFull);
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
            for (int q = tid; q < nl; q += BT) { const unsigned a = age16[q]; if (a != 0xFFFFu) age16[q] = (u16)(a + 1); }
            if (tenure == A.t_max || tenure == A.t_min) tup = !tup;
            tenure += tup ? 1 : -1;
            if (iters >= A.tabu_k) status = LP_ST_CAPPED;
            __syncthreads();
        } else {
            if (cap >= 0 && kd >= cap) status = LP_ST_CAPPED;
            else if (A.budget >= 0 && sdone >= A.budget) status = LP_ST_BUDGET;
        }
    }
#undef LP_PHASE
#undef LP_PHASE2
#undef LP_WRAP_HI
#undef LP_WRAP_LO
#undef LP_WRAP_EQS
#undef LP_WRAP_EQ
#undef LP_TID
#undef LP_LM0
    if constexpr (CLOCKS) if (clk) {
        unsigned long long *o = A.stamps + (size_t)wg * 16;
        for (int i = 0; i < 6; i++) o[i] = ph[i];
        o[6] = nreload; o[7] = nrows; o[8] = (unsigned long long)sdone;
        for (int i = 0; i < 4; i++) o[9 + i] = ph2[i];
        if constexpr (VNS) { o[13] = vns_ph[0]; o[14] = vns_ph[1]; o[15] = vns_ph[2]; }
    }
    // ---- the tour state back to the slot (every workgroup its own cells).  Shaped form: the slot's arrays are read from the
    // kernel arguments AGAIN, through a pointer the compiler cannot see through -- a dozen 64-bit pointers that are used
    // before and behind the sweep loop only would otherwise live (spilled to lanes) across all of it.
#define LP_WRITE_BACK(S_, t_, tn_, ctl_)                                                                                  \
    if (tid < E) {                                                                                                        \
        const int p = k0 + tid;                                                                                           \
        int pn = p + 1; if (pn == n) pn = 0;                                                                              \
        int pp = p - 1; if (pp < 0) pp += n;                                                                              \
        const int lab = wt16[2 * p + 1];                                                                                  \
        S_.ord[tn_ + p] = lab;                                                                                            \
        reinterpret_cast<int *>(S_.dpos + tn_)[p] = (int)wt16[2 * p];                                                     \
        S_.pos[tn_ + lab] = p;                                                                                            \
        S_.succ[tn_ + lab] = dir > 0 ? (int)wt16[2 * pn + 1] : (int)wt16[2 * pp + 1];                                     \
        reinterpret_cast<int *>(S_.dnb + tn_)[lab] = dir > 0 ? (int)wt16[2 * p] : (int)wt16[2 * pp];                      \
    }                                                                                                                     \
    if (wg == 0 && tid == 0) {                                                                                            \
        S_.dir[t_] = dir;                                                                                                 \
        S_.cost[t_] = cost0 + (double)sumd;                                                                               \
        S_.nsweeps[t_] = kd;                                                                                              \
        if (sdone > 0) S_.last_delta[t_] = (double)lastd;                                                                 \
        if (status == LP_ST_OPTIMUM || status == LP_ST_CAPPED) S_.done[t_] = 1;                                           \
        if constexpr (TABU || VNS) *A.best_out = best;                                                                    \
        if constexpr (VNS) { A.vns_state[0] = vit; A.vns_state[1] = vcur; A.vns_state[2] = status == LP_ST_NEED_RAND ? 1 : 0; } \
        ctl_[1] = status; ctl_[2] = sdone;                                                                                \
    }
    if constexpr (SH) {
        // (the kernel-argument segment begins with the explicit arguments: PersistArgs, the only one, lies at offset 0)
        static_assert(std::is_same_v<decltype(&k_lds2opt<PK16, TABU, VNS, NLC, EC, TM, CLK>), void (*)(PersistArgs)>, "PersistArgs must stay the kernel's only argument");
        c_PersistArgs *Ak = (c_PersistArgs *)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(Ak));
        const int tk = Ak->slot;
        const size_t tnk = (size_t)tk * n;
        LP_WRITE_BACK(Ak->S, tk, tnk, Ak->ctl)
    } else {
        LP_WRITE_BACK(A.S, t, tn, A.ctl)
    }
#undef LP_WRITE_BACK
}

// the best tour of the tabu walk as a successor array (behind the kernel boundary: every cell of best_ord is visible)
__global__ void __launch_bounds__(256) k_lds_best_succ(const int *__restrict__ best_ord, const int *__restrict__ best_dir, int *__restrict__ best_succ, int n)
{
    if (!best_dir[1]) return;                         // never improved: the successor array the walk started from stands
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int q = best_dir[0] > 0 ? (p + 1 == n ? 0 : p + 1) : (p == 0 ? n - 1 : p - 1);
    best_succ[best_ord[p]] = best_ord[q];
}
