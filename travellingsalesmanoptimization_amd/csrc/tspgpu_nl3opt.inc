// ---------------------------------------------------------------------------
// Neighbour-list 3-opt: the pure 3-opt moves (segment insertion of any length, the double reversal and the two mixed forms)
// whose new edges come from the K-nearest-neighbour lists, and every accepted move of a sweep applied in one launch.
// Included by tspgpu.hip behind tspgpu_ornl.inc (uses Tours, Elem, wave_argmin, key_better, or_cell / or_ecell, OrMatCost /
// OrPtsCost, M2Buf, M2Ctl, NlBuf, m2_counted_scan, m2_sum_close, m2_reverse_cells, k_m2_select).  The rule is in include/tspgpu.h
// ("Neighbour-list 3-opt") and DESIGN 4.19; conflict and selection are those of tspgpu_multi2opt.inc.
//
// A candidate is a chain t1 .. t6: the tour edges {t1,t2}, {t3,t4}, {t5,t6} go, {t2,t3}, {t4,t5}, {t6,t1} come; t3 is among
// the first W of N(t2), t5 among the first W of N(t4).  It travels through M2Buf as a = t1, b = code (bit 30 set: b > a, and
// m2_key(a, b) = a << 32 | b orders by (t1, code)), i / j = the range [i, k].
//
// Per sweep four launches on the slot's stream:
//   k_nl3_sweep / k_nl3_sweep_otf   one wave per t1 (NL3_NODES per workgroup).  The 4 W first-level choices (s2, j3, s4) lie
//                                   across the lanes, 64 / (4 W) lanes each (one at W = 16, three at W = 5), which share the
//                                   2 W second-level choices (j5, s6) among them.  c[t2][t3] and c[t4][t5] are the lists'
//                                   weights, the removed edges come from dnb, c[t6][t1] is the one gather from the cost
//                                   source; succ and pred come from pos, ord and dir.  The kind test runs only for a chain
//                                   that would beat the lane's best so far.  A DPP argmin by (delta, code) leaves
//                                   raw_d[t1] / raw_b[t1].  No LDS.
//   k_nl3_compact                   one workgroup: m2_counted_scan over the improving nodes; the chain of (t1, code) is decoded to
//                                   its three edge positions, counted from node 0 in the slot's direction.
//   k_m2_select                     unchanged.
//   k_nl3_apply / k_nl3_apply_otf   workgroup per accepted move (grid-stride).  The chain is decoded again; the new order of
//                                   the positions i + 1 .. k is made of two or three in-place reversals (m2_reverse_cells)
//                                   with barriers between them; then the three new edge cells from the cost source, and the
//                                   node view (succ, dnb) of the range from the cells.  Ranges are disjoint, so a launch's
//                                   moves touch disjoint cells, edges and nodes (two moves may share an end node: the k + 1
//                                   of one, of which only pos is read, and the i of the other, whose position stays).
//                                   Workgroup 0 first sums the accepted deltas and closes the sweep as k_m2_apply does.
//   k_nl3_describe                  (tspgpu_three_opt_nl_once only) j and kind of every compacted candidate into raw_b[x],
//                                   which nothing reads between the compaction and the next sweep.
// ---------------------------------------------------------------------------
static constexpr int NL3_NODES = 4;         // nodes t1 per workgroup of the sweep (256 threads, a wave per node)
static constexpr int NL3_APPLY_BT = 256;    // threads of an apply workgroup
static constexpr int NL3_BIT = 1 << 30;

static_assert(NL_KMAX == 16 && OR_QB == 17, "packing of a neighbour-list 3-opt candidate: j3 and j5 in four bits, labels below bit 30");

__device__ __forceinline__ int nl3_code(int s2, int j3, int s4, int j5, int s6) { return NL3_BIT | s2 << 10 | j3 << 6 | s4 << 5 | j5 << 1 | s6; }

// the tour of a slot as positions: f the position of a cell along the slot's direction, P = f - f(node 0) the rule's position
struct Nl3Pos {
    const int *ord, *pos;
    int n, dir, f0;
    __device__ __forceinline__ int f_of(int v) const { const int c = pos[v]; return dir > 0 ? c : n - 1 - c; }
    __device__ __forceinline__ int at(int f) const { f = wrap(f, n); return ord[dir > 0 ? f : n - 1 - f]; }    // f in [-1, n]
    __device__ __forceinline__ int P(int f) const { return wrap(f - f0, n); }
};

__device__ __forceinline__ Nl3Pos nl3_pos(const Tours &S, int n, int t)
{
    Nl3Pos T{S.ord + (size_t)t * n, S.pos + (size_t)t * n, n, S.dir[t], 0};
    T.f0 = T.f_of(0);
    return T;
}

// the other end x of the tour edge at v (s = 0: succ(v), 1: pred(v)) and the edge's position e; fv = f_of(v)
__device__ __forceinline__ void nl3_step(const Nl3Pos &T, int fv, int s, int &x, int &e)
{
    x = T.at(s ? fv - 1 : fv + 1);
    e = T.P(s ? fv - 1 : fv);
}

// rule 4's kind of a chain from the positions of its removed edges and its three directions, -1: none.  The six chain nodes
// take the roles 2 rank + (head ? 1 : 0) = a, a', b, b', c, c'; the added pairs are a perfect matching of the roles
__device__ __forceinline__ int nl3_kind(int e1, int e2, int e3, int s2, int s4, int s6)
{
    if (e1 == e2 || e1 == e3 || e2 == e3) return -1;
    const int r1 = (e1 > e2) + (e1 > e3), r2 = (e2 > e1) + (e2 > e3), r3 = (e3 > e1) + (e3 > e2);
    const int q1 = 2 * r1 + s2, q2 = 2 * r1 + (s2 ^ 1), q3 = 2 * r2 + s4, q4 = 2 * r2 + (s4 ^ 1), q5 = 2 * r3 + s6, q6 = 2 * r3 + (s6 ^ 1);
    const unsigned mate = (unsigned)q3 << 3 * q2 | (unsigned)q2 << 3 * q3 | (unsigned)q5 << 3 * q4 | (unsigned)q4 << 3 * q5 |
                          (unsigned)q1 << 3 * q6 | (unsigned)q6 << 3 * q1;
    const int pa = mate & 7, pb = (mate >> 3) & 7;          // the partners of a and a'
    return pa == 2 && pb == 4 ? 0 : pa == 3 && pb == 4 ? 1 : pa == 4 && pb == 3 ? 2 : pa == 3 && pb == 5 ? 3 : -1;
}

__device__ __forceinline__ bool nl3_same(int x, int y, int u, int v) { return (x == u && y == v) || (x == v && y == u); }

// rule 4's third test, by label: no added edge is a loop or one of the removed edges
__device__ __forceinline__ bool nl3_labels_ok(int t1, int t2, int t3, int t4, int t5, int t6)
{
    auto bad = [&](int x, int y) { return x == y || nl3_same(x, y, t1, t2) || nl3_same(x, y, t3, t4) || nl3_same(x, y, t5, t6); };
    return !(bad(t2, t3) || bad(t4, t5) || bad(t6, t1));
}

struct Nl3Move { int i, j, k, kind; };

// the chain of (t1, code) on the tour as it stands -> the positions of its removed edges in ascending order and its kind
__device__ __forceinline__ Nl3Move nl3_decode(const Nl3Pos &T, const NlBuf &NL, int t1, int code)
{
    const int s2 = (code >> 10) & 1, j3 = (code >> 6) & 15, s4 = (code >> 5) & 1, j5 = (code >> 1) & 15, s6 = code & 1;
    int t2, t4, t6, e1, e2, e3;
    nl3_step(T, T.f_of(t1), s2, t2, e1);
    const int t3 = NL.node[(size_t)t2 * NL.K + j3];
    nl3_step(T, T.f_of(t3), s4, t4, e2);
    const int t5 = NL.node[(size_t)t4 * NL.K + j5];
    nl3_step(T, T.f_of(t5), s6, t6, e3);
    Nl3Move M;
    M.i = min(e1, min(e2, e3));
    M.k = max(e1, max(e2, e3));
    M.j = e1 + e2 + e3 - M.i - M.k;
    M.kind = nl3_kind(e1, e2, e3, s2, s4, s6);
    return M;
}

template <typename AT, typename CS>
__device__ __forceinline__ void nl3_sweep_unit(const Tours &S, const CS cs, int n, int t, const NlBuf &NL, int W, const M2Buf &B, int t1)
{
    const int lane = threadIdx.x & 63;      // t1: this wave's node, 0 <= t1 < n
    const Nl3Pos T = nl3_pos(S, n, t);
    const AT *dnb = dnb_of<AT>(S, t, n), *lw = reinterpret_cast<const AT *>(NL.w);
    const int K = NL.K, F = 4 * W, per = 64 / F;            // lanes per first-level choice: 1 at W = 16, 16 at W = 1
    const int f = lane / per, sub = lane - f * per;

    double bd = DBL_MAX;
    u64 bk = KEY_NONE;
    if (f < F) {
        const int s2 = f >= 2 * W ? 1 : 0, g = f - s2 * 2 * W, j3 = g >> 1, s4 = g & 1;
        int t2, t4, e1, e2;
        nl3_step(T, T.f_of(t1), s2, t2, e1);
        const AT c12 = dnb[s2 ? t2 : t1];
        const int t3 = NL.node[(size_t)t2 * K + j3];
        const AT c23 = lw[(size_t)t2 * K + j3];
        nl3_step(T, T.f_of(t3), s4, t4, e2);
        const AT c34 = dnb[s4 ? t4 : t3];
        if (e1 != e2) {
            for (int x = sub; x < 2 * W; x += per) {
                const int j5 = x >> 1, s6 = x & 1;
                const int t5 = NL.node[(size_t)t4 * K + j5];
                const AT c45 = lw[(size_t)t4 * K + j5];
                int t6, e3;
                nl3_step(T, T.f_of(t5), s6, t6, e3);
                const AT c56 = dnb[s6 ? t6 : t5];
                const AT d = ((c23 + c45) + cs(t6, t1)) - ((c12 + c34) + c56);     // rule 3, this order
                const u64 key = (u64)nl3_code(s2, j3, s4, j5, s6);
                if (key_better((double)d, key, bd, bk) && nl3_kind(e1, e2, e3, s2, s4, s6) >= 0 && nl3_labels_ok(t1, t2, t3, t4, t5, t6)) {
                    bd = (double)d;
                    bk = key;
                }
            }
        }
    }
    wave_argmin(bd, bk);
    if (lane == 0) {
        B.raw_d[t1] = bd;
        B.raw_b[t1] = bk == KEY_NONE ? -1 : (int)bk;
    }
}

// the plain sweep: workgroup g takes the nodes g NL3_NODES .. g NL3_NODES + NL3_NODES - 1
template <typename AT, typename CS>
__device__ __forceinline__ void nl3_sweep_node(const Tours &S, const CS cs, int n, int t, const NlBuf &NL, int W, const M2Buf &B)
{
    const int t1 = (int)blockIdx.x * NL3_NODES + (threadIdx.x >> 6);
    if (t1 >= n) return;                    // (a whole wave: no barrier below)
    nl3_sweep_unit<AT>(S, cs, n, t, NL, W, B, t1);
}

template <typename T>
__global__ void __launch_bounds__(256) k_nl3_sweep(Tours S, const T *__restrict__ mat, int n, int ld, int t, NlBuf NL, int W, M2Buf B, const M2Ctl *ctl)
{
    if (ctl->stop) return;
    nl3_sweep_node<typename Elem<T>::acc>(S, OrMatCost<T>{mat, ld}, n, t, NL, W, B);
}

template <int KIND>
__global__ void __launch_bounds__(256) k_nl3_sweep_otf(Tours S, const typename OrPt<KIND>::type *__restrict__ pts, int n, int t, NlBuf NL, int W,
                                                       M2Buf B, const M2Ctl *ctl)
{
    if (ctl->stop) return;
    nl3_sweep_node<int>(S, OrPtsCost<KIND>{pts}, n, t, NL, W, B);
}

// the improving candidates through m2_counted_scan, with the ranges of their decoded chains.  For the control block of a single
// descent or of a tour of a batch (tspgpu_nlbatch.inc)
template <typename CTL>
__device__ __forceinline__ void nl3_compact_tour(const Tours &S, int n, int t, const NlBuf &NL, const M2Buf &B, CTL *ctl, int *cnts)
{
    const Nl3Pos T = nl3_pos(S, n, t);
    m2_counted_scan(
        n, ctl, cnts, [&](int s) { return B.raw_b[s] >= 0 && B.raw_d[s] < TWO_OPT_EPS; },
        [&](int s, int at) {
            const int code = B.raw_b[s];
            const Nl3Move M = nl3_decode(T, NL, s, code);
            B.d[at] = B.raw_d[s];
            B.a[at] = s;
            B.b[at] = code;
            B.i[at] = M.i;                  // 0 <= i < k <= n - 1: no range wraps
            B.j[at] = M.k;
        });
}

__global__ void __launch_bounds__(1024) k_nl3_compact(Tours S, int n, int t, NlBuf NL, M2Buf B, M2Ctl *ctl)
{
    __shared__ int cnts[1024];
    nl3_compact_tour(S, n, t, NL, B, ctl, cnts);
}

// j << 2 | kind of candidate x into raw_b[x] (the sweep's raw_b is spent once the compaction has run)
__global__ void __launch_bounds__(256) k_nl3_describe(Tours S, int n, int t, NlBuf NL, M2Buf B, const M2Ctl *ctl)
{
    const int m = ctl->m;
    const Nl3Pos T = nl3_pos(S, n, t);
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < m; x += gridDim.x * blockDim.x) {
        const Nl3Move M = nl3_decode(T, NL, B.a[x], B.b[x]);
        B.raw_b[x] = M.j << 2 | M.kind;
    }
}

// (every return and `continue` in front of a barrier is block-uniform: the trip count of the move loop depends only on
// blockIdx.x, gridDim.x and m, and acc[y] is one cell for the whole workgroup)
template <typename T, typename CS, typename CTL>
__device__ __forceinline__ void nl3_apply_tour(const Tours &S, const CS cs, int n, int t, const NlBuf &NL, const M2Buf &B, CTL *ctl)
{
    typedef typename Elem<T>::acc AT;
    const int tid = threadIdx.x, BT = NL3_APPLY_BT;
    const int m = ctl->m;                   // (0 once `stop` is up: k_nl3_compact)
    if (blockIdx.x == 0 && !m2_sum_close(S, t, B, ctl, m, BT)) return;      // the close of k_m2_apply
    int *ord = S.ord + (size_t)t * n, *pos = S.pos + (size_t)t * n, *succ = S.succ + (size_t)t * n;
    AT *dp = dpos_of<AT>(S, t, n), *dnb = dnb_of<AT>(S, t, n);
    const Nl3Pos T0 = nl3_pos(S, n, t);     // node 0 is in no moved range: its cell stays
    const int dir = T0.dir, f0 = T0.f0;
    for (int y = blockIdx.x; y < m; y += gridDim.x) {
        if (!B.acc[y]) continue;
        // the chain's nodes lie in this move's range [i, k + 1]: no other move of the launch moves them, and the reads end
        // at the barrier, before this workgroup writes
        const Nl3Move M = nl3_decode(T0, NL, B.a[y], B.b[y]);
        const int i = M.i, j = M.j, k = M.k, la = j - i, lb = k - j;
        __syncthreads();
        if (M.kind != 3) m2_reverse_cells(ord, pos, dp, n, dir, f0 + i, la);       // A: positions i + 1 .. j
        if (M.kind != 2) m2_reverse_cells(ord, pos, dp, n, dir, f0 + j, lb);       // B: positions j + 1 .. k
        __syncthreads();
        if (M.kind != 0) {                  // 1: rev A, rev B -> B A;  2: rev A -> rev B, A;  3: rev B -> B, rev A
            m2_reverse_cells(ord, pos, dp, n, dir, f0 + i, la + lb);
            __syncthreads();
        }
        if (tid < 3) {                      // the three new edges: behind a, between the two blocks, in front of c'
            const int e = tid == 0 ? i : tid == 2 ? k : M.kind == 0 ? j : i + lb;
            const int u = ord[or_cell(f0 + e, n, dir)], v = ord[or_cell(f0 + e + 1, n, dir)];
            dp[or_ecell(f0 + e, n, dir)] = cs(u, v);
        }
        __syncthreads();
        for (int p = i + tid; p <= k; p += BT) {            // node view of the range from its cells
            const int v = ord[or_cell(f0 + p, n, dir)];
            succ[v] = ord[or_cell(f0 + p + 1, n, dir)];
            dnb[v] = dp[or_ecell(f0 + p, n, dir)];
        }
        __syncthreads();
    }
}

template <typename T>
__global__ void __launch_bounds__(NL3_APPLY_BT) k_nl3_apply(Tours S, const T *__restrict__ mat, int n, int ld, int t, NlBuf NL, M2Buf B, M2Ctl *ctl)
{
    nl3_apply_tour<T>(S, OrMatCost<T>{mat, ld}, n, t, NL, B, ctl);
}

template <int KIND>
__global__ void __launch_bounds__(NL3_APPLY_BT) k_nl3_apply_otf(Tours S, const typename OrPt<KIND>::type *__restrict__ pts, int n, int t, NlBuf NL,
                                                                M2Buf B, M2Ctl *ctl)
{
    nl3_apply_tour<int>(S, OrPtsCost<KIND>{pts}, n, t, NL, B, ctl);
}
