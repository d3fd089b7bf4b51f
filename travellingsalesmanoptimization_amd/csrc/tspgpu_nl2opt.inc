// ---------------------------------------------------------------------------
// Neighbour-list 2-opt: the candidates of a parallel-move sweep come from K-nearest-neighbour lists instead of all b.
// Included by tspgpu.hip behind tspgpu_multi2opt.inc (uses Tours, Elem, wave_min_i64, dpp_u64, key_better, or_cell,
// OrMatCost / OrPtsCost / or_weight, M2Buf, M2Ctl).  The rule is in include/tspgpu.h ("Neighbour-list 2-opt") and
// DESIGN 4.14; rules 2-5 are the parallel-move section's: k_m2_compact, k_m2_select and k_m2_apply run unchanged behind
// the sweep of this file.
//
//   k_nl_build / k_nl_build_otf   one wave per node v: N(v), the K' nodes u != v with the smallest (c[v][u], u), ascending.
//                                 A lane streams over the cells lane, lane + 64, .. of the row (matrix mode: 16-byte
//                                 coalesced loads, the row is read once; matrix-free mode: the weight from the points)
//                                 and keeps its NL_KMAX best keys sorted in registers -- one comparison per cell against
//                                 the worst of them, the insertion (NL_KMAX compare-and-swaps at fixed register numbers)
//                                 only for a cell that enters.  The wave's K' best are among the lanes' lists: K' rounds
//                                 of two wave minima (cost, then node among the lanes whose head has that cost) pop them
//                                 in order.  No LDS, no switch in block size or vectors per thread: one loop.
//   k_nl_sweep / k_nl_sweep_otf   32 lanes per node a (two nodes per wave, NL_NODES per workgroup): lane l < 16 takes
//                                 b = N(a)[l], lane 16 + l takes b = pred(N(sa)[l]); the weight the list stores is one of
//                                 the two new edges, the other is one gather (a matrix cell or a weight from two points).
//                                 A DPP argmin over the 32 lanes by (delta, b) leaves raw_d[a] / raw_b[a] as k_m2_sweep does.
// ---------------------------------------------------------------------------
static constexpr int NL_KMAX = 16;          // the longest list
static constexpr int NL_NODES = 8;          // nodes per workgroup of the sweep (256 threads, 32 lanes per node)
static constexpr int NL_BUILD_ROWS = 4;     // rows per workgroup of the build (256 threads, a wave per row)

struct NlBuf {              // the lists of the cost source in place, [n][K] each
    int K;                  // K' = min(K asked for, n - 1); 0: no lists
    int *node;              // N(v)[j]
    double *w;              // c[v][N(v)[j]]: 8-byte slots, integer modes use the first 4 n K bytes (as Tours::dnb)
};

// the order of costs as a signed integer: the cost itself for integer cells, for doubles the bits folded so that the
// integer order is the doubles' order (-0.0 is taken as +0.0: the two compare equal as doubles)
__device__ __forceinline__ int nl_ck(int c) { return c; }
__device__ __forceinline__ long long nl_ck(double c)
{
    const long long b = __double_as_longlong(c + 0.0);
    return b ^ ((b >> 63) & 0x7fffffffffffffffll);
}
__device__ __forceinline__ int nl_cost(int k) { return k; }
__device__ __forceinline__ double nl_cost(long long k) { return __longlong_as_double(k ^ ((k >> 63) & 0x7fffffffffffffffll)); }
template <typename KT> struct NlLim;
template <> struct NlLim<int> { static constexpr int max = INT_MAX; };
template <> struct NlLim<long long> { static constexpr long long max = LLONG_MAX; };

// a lane's NL_KMAX best (cost key, node), ascending, in registers (every index is a constant after unrolling)
template <typename KT> struct NlTop {
    KT c[NL_KMAX];
    int u[NL_KMAX];
    __device__ __forceinline__ void init()
    {
#pragma unroll
        for (int j = 0; j < NL_KMAX; j++) { c[j] = NlLim<KT>::max; u[j] = INT_MAX; }
    }
    __device__ __forceinline__ void offer(KT ck, int node)
    {
        if (!(ck < c[NL_KMAX - 1] || (ck == c[NL_KMAX - 1] && node < u[NL_KMAX - 1]))) return;
#pragma unroll
        for (int j = 0; j < NL_KMAX; j++) {
            if (ck < c[j] || (ck == c[j] && node < u[j])) {
                const KT tc = c[j]; const int tu = u[j];
                c[j] = ck; u[j] = node;
                ck = tc; node = tu;
            }
        }
    }
    __device__ __forceinline__ void pop()
    {
#pragma unroll
        for (int j = 0; j + 1 < NL_KMAX; j++) { c[j] = c[j + 1]; u[j] = u[j + 1]; }
        c[NL_KMAX - 1] = NlLim<KT>::max; u[NL_KMAX - 1] = INT_MAX;
    }
};

// the K best of the wave's 64 sorted lists, in order, to node[] / w[] of row v (K <= n - 1 real entries exist)
template <typename KT, typename AT>
__device__ __forceinline__ void nl_merge(NlTop<KT> &top, int K, int *__restrict__ node, AT *__restrict__ w, int lane)
{
    for (int j = 0; j < K; j++) {
        const long long mc = wave_min_i64((long long)top.c[0]);
        const bool tie = (long long)top.c[0] == mc;
        const int mu = (int)wave_min_i64(tie ? (long long)top.u[0] : (long long)INT_MAX);
        if (tie && top.u[0] == mu) top.pop();       // one lane: a node sits in one lane's list
        if (lane == 0) { node[j] = mu; w[j] = (AT)nl_cost((KT)mc); }
    }
}

template <typename T>
__global__ void __launch_bounds__(256) k_nl_build(const T *__restrict__ mat, int n, int ld, NlBuf L)
{
    typedef typename Elem<T>::acc AT;
    typedef typename Elem<T>::vec VT;
    typedef decltype(nl_ck((AT)0)) KT;
    constexpr int V = Elem<T>::V;
    const int lane = threadIdx.x & 63, v = (int)blockIdx.x * NL_BUILD_ROWS + (threadIdx.x >> 6);
    if (v >= n) return;                                     // (a whole wave: no barrier below)
    const VT *row = reinterpret_cast<const VT *>(mat + (size_t)v * ld);
    const int nvec = ld / V;                                // ld is a multiple of 32 cells: whole vectors, inside the row
    NlTop<KT> top;
    top.init();
    for (int i = lane; i < nvec; i += 64) {
        const VT x = row[i];
#pragma unroll
        for (int e = 0; e < V; e++) {
            const int u = i * V + e;
            if (u < n && u != v) top.offer(nl_ck((AT)vget(x, e)), u);
        }
    }
    nl_merge<KT, AT>(top, L.K, L.node + (size_t)v * L.K, reinterpret_cast<AT *>(L.w) + (size_t)v * L.K, lane);
}

template <int KIND>
__global__ void __launch_bounds__(256) k_nl_build_otf(const typename OrPt<KIND>::type *__restrict__ pts, int n, NlBuf L)
{
    typedef typename OrPt<KIND>::type PT;
    const int lane = threadIdx.x & 63, v = (int)blockIdx.x * NL_BUILD_ROWS + (threadIdx.x >> 6);
    if (v >= n) return;
    const PT pv = pts[v];
    NlTop<int> top;
    top.init();
    for (int u = lane; u < n; u += 64)
        if (u != v) top.offer(or_weight<KIND>(pv, pts[u]), u);
    nl_merge<int, int>(top, L.K, L.node + (size_t)v * L.K, reinterpret_cast<int *>(L.w) + (size_t)v * L.K, lane);
}

// lexicographic minimum of (d, key) over each half of the wave (lanes 0-31, 32-63): valid in lanes 31 and 63.
// The steps of wave_argmin without the last broadcast, which would join the halves.
__device__ __forceinline__ void half_argmin(double &d, u64 &key)
{
#define STEP(C, R) { const double od = __longlong_as_double((long long)dpp_u64<C, R>((u64)__double_as_longlong(d))); \
                     const u64 ok = dpp_u64<C, R>(key);                                                                 \
                     if (key_better(od, ok, d, key)) { d = od; key = ok; } }
    STEP(0xB1, 0xf) STEP(0x4E, 0xf) STEP(0x141, 0xf) STEP(0x140, 0xf) STEP(0x142, 0xa)
#undef STEP
}

template <typename AT, typename CS>
__device__ __forceinline__ void nl_sweep_unit(const Tours &S, const CS cs, int n, int t, const NlBuf &L, const M2Buf &B, int a)
{
    const int l = threadIdx.x & 31;         // a: this half-wave's node; a >= n: it has none (the queued sweep's tail)
    // (no early return: the DPP steps read lanes of both halves; a lane without a candidate carries "none")
    double dd = DBL_MAX;
    u64 key = KEY_NONE;
    if (a < n) {
        const int *ord = S.ord + (size_t)t * n, *pos = S.pos + (size_t)t * n, *succ = S.succ + (size_t)t * n;
        const AT *dnb = dnb_of<AT>(S, t, n), *lw = reinterpret_cast<const AT *>(L.w);
        const int K = L.K, j = l & 15;
        if (j < K) {
            const int dir = S.dir[t], sa = succ[a];
            int b, sb;
            AT cab, css;
            if (l < 16) {               // b in N(a): the list holds c[a][b]
                b = L.node[(size_t)a * K + j];
                cab = lw[(size_t)a * K + j];
                sb = succ[b];
                css = cs(sa, sb);
            } else {                    // sb in N(sa), b = pred(sb): the list holds c[sa][sb]
                sb = L.node[(size_t)sa * K + j];
                css = lw[(size_t)sa * K + j];
                const int p = pos[sb] - dir;            // dir = +1: succ(ord[p]) = ord[p + 1]
                b = ord[p < 0 ? p + n : (p >= n ? p - n : p)];
                cab = cs(a, b);
            }
            if (!(sa == sb || a == sb || b == sa)) {    // refinment.c:55
                const AT d = (cab + css) - (dnb[a] + dnb[b]);       // refinment.c:60-62, this order
                dd = (double)d;
                key = (u64)b;
            }
        }
    }
    half_argmin(dd, key);
    if (l == 31 && a < n) {
        B.raw_d[a] = dd;
        B.raw_b[a] = key == KEY_NONE ? -1 : (int)key;
    }
}

// the plain sweep: workgroup g takes the nodes g NL_NODES .. g NL_NODES + NL_NODES - 1
template <typename AT, typename CS>
__device__ __forceinline__ void nl_sweep_node(const Tours &S, const CS cs, int n, int t, const NlBuf &L, const M2Buf &B)
{
    nl_sweep_unit<AT>(S, cs, n, t, L, B, (int)blockIdx.x * NL_NODES + (threadIdx.x >> 5));
}

template <typename T>
__global__ void __launch_bounds__(256) k_nl_sweep(Tours S, const T *__restrict__ mat, int n, int ld, int t, NlBuf L, M2Buf B, const M2Ctl *ctl)
{
    if (ctl->stop) return;
    nl_sweep_node<typename Elem<T>::acc>(S, OrMatCost<T>{mat, ld}, n, t, L, B);
}

template <int KIND>
__global__ void __launch_bounds__(256) k_nl_sweep_otf(Tours S, const typename OrPt<KIND>::type *__restrict__ pts, int n, int t, NlBuf L, M2Buf B,
                                                      const M2Ctl *ctl)
{
    if (ctl->stop) return;
    nl_sweep_node<int>(S, OrPtsCost<KIND>{pts}, n, t, L, B);
}
