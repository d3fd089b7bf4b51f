// Held-Karp lower bound: 1-trees in Boruvka rounds and the subgradient ascent over them (include/tspgpu.h "Held-Karp lower
// bound", DESIGN 4.24).  Included by tspgpu.hip behind tspgpu_oropt.inc (OrPt, or_weight) and the kernels above it (Elem,
// vget, wave_min_i64).
//
// One iteration of the ascent is a fixed chain of launches; no kernel waits on another workgroup, what one launch writes the
// next reads, and nothing is read back:
//   k_hk_init                     every node a component of its own, no edges
//   k_hk_zero                     one workgroup: node 0's two smallest keys
//   per round (ceil(log2(n - 1)) of them; HkCtl::done makes the rounds after the last merge return at once):
//     k_hk_scan / k_hk_scan_otf   the hot path.  One wave per node v >= 1 streams row v (matrix mode: 16-byte coalesced loads;
//                                 matrix-free mode: the weight from the points) and keeps per lane the smallest
//                                 w = 128 c[v][u] + pi[u] over the u >= 1 of another component.  A lane sees its u ascending and
//                                 for one v the order of the pairs {v, u} is the order of u, so a strict comparison keeps the
//                                 smallest key.  Two wave minima (the weight, then u among the ties) give best(v); lane 0 posts
//                                 the weight to the component with a 64-bit atomic minimum.  comp[] and pi[] are staged in LDS
//                                 where 12 ld bytes fit (STAGE), else read through L2.
//     k_hk_cmin                   the packed pair of every node whose weight is its component's minimum: a second atomic minimum
//     k_hk_hook                   one thread per component: its edge is accepted (recorded once when both components chose it,
//                                 degrees, the weight into the tree's sum) and the component hooks onto the other one -- of a
//                                 mutual pair the smaller label stays a root
//     k_hk_flat                   every node follows the hooks to the root (the hooks are read-only here), the components'
//                                 minima are reset, thread 0 keeps the books
//   k_hk_step                     one workgroup: L, q, best / pi*, the stop reasons, t, the 2^45 guard and the pi update
// Every kernel returns at once when HkCtl::stop is set, so the iterations enqueued behind the last one cost a launch each.

constexpr int HK_BT = 256;
constexpr int HK_ROWS = 8;                  // nodes per workgroup of the scan (512 threads, a wave per node)
constexpr int HK_STEP_BT = 1024;
constexpr long long HK_S = 128;
constexpr long long HK_PI_MAX = 1ll << 45;
constexpr long long HK_WMAX = LLONG_MAX;
constexpr u64 HK_ENONE = ~0ull;

struct HkCtl {
    long long wsum;             // the sum of w(e) over the edges of the tree in hand
    unsigned nedges;            // its tree edges so far (n - 2 when complete); node 0's two edges are not counted
    unsigned seen;              // ... as the last k_hk_flat saw it
    int done;                   // the tree is complete (written by k_hk_flat and k_hk_init only)
    int rounds;                 // rounds that accepted an edge
    int err;                    // 1: a hook chain longer than n, or more edges than a tree has (a mistake in this file)
    int stop;                   // the ascent ended: reason + 1 (the reason of rule 3; 0 while it runs)
    int h, bad, iters, have_best;
    long long best;             // the largest L so far
    long long ubs;              // S * UB
    int patience, pad;
};

struct HkBuf {
    long long *pi, *pibest;     // [ld + 64] the multipliers and pi*
    int *comp;                  // [ld + 64] the label of v's component: its root node
    int *up;                    // [n] the hook of a label (itself: a root); labels that were hooked are never read again
    long long *bw; u64 *be;     // [n] best(v): weight, and (a << 32 | b)
    long long *cw; u64 *ce;     // [n] by label: the component's minimum
    int *deg;                   // [n]
    u64 *edges;                 // [n] the tree: [0], [1] node 0's edges, then the tree edges in no particular order
    HkCtl *ctl;
};

__device__ __forceinline__ void hk_min(long long *p, long long x) { __hip_atomic_fetch_min(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void hk_min(u64 *p, u64 x) { __hip_atomic_fetch_min(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void hk_add(long long *p, long long x)
{
    __hip_atomic_fetch_add(reinterpret_cast<u64 *>(p), (u64)x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ u64 hk_pair(int v, int u) { return v < u ? ((u64)(unsigned)v << 32) | (unsigned)u : ((u64)(unsigned)u << 32) | (unsigned)v; }

__global__ void __launch_bounds__(HK_BT) k_hk_init(HkBuf H, int n)
{
    HkCtl *C = H.ctl;
    if (C->stop) return;
    const int v = blockIdx.x * HK_BT + threadIdx.x;
    if (v < n) {
        H.comp[v] = v; H.up[v] = v;
        H.cw[v] = HK_WMAX; H.ce[v] = HK_ENONE;
        H.deg[v] = 0;
    }
    if (v == 0) { C->wsum = 0; C->nedges = 0; C->seen = 0; C->done = n <= 2 ? 1 : 0; C->rounds = 0; }
}

// node 0's edges: the two smallest keys (w(0, u), 0, u), u >= 1.  One workgroup; the weight of {0, u} through the cost functor
template <typename CS>
__device__ __forceinline__ void hk_zero(const HkBuf &H, const CS cs, int n)
{
    __shared__ long long sw[HK_BT / 64];
    __shared__ int su[HK_BT / 64];
    if (H.ctl->stop) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long p0 = H.pi[0];
    int first = -1;
    for (int pass = 0; pass < 2; pass++) {
        long long bw = HK_WMAX; int bu = INT_MAX;
        for (int u = 1 + tid; u < n; u += HK_BT) {
            if (u == first) continue;
            const long long w = HK_S * (long long)cs(0, u) + p0 + H.pi[u];
            if (w < bw) { bw = w; bu = u; }
        }
        const long long mw = wave_min_i64(bw);
        const int mu = (int)wave_min_i64(bw == mw ? (long long)bu : (long long)INT_MAX);
        if (lane == 0) { sw[wv] = mw; su[wv] = mu; }
        __syncthreads();
        long long w = sw[0]; int u = su[0];
        for (int k = 1; k < HK_BT / 64; k++)
            if (sw[k] < w || (sw[k] == w && su[k] < u)) { w = sw[k]; u = su[k]; }
        __syncthreads();
        if (tid == 0 && u < n) {
            H.edges[pass] = hk_pair(0, u);
            atomicAdd(&H.deg[u], 1);
            hk_add(&H.ctl->wsum, w);
            if (pass == 1) H.deg[0] = 2;
        }
        first = u;
    }
}

template <typename T> struct HkMatCost {
    const T *__restrict__ mat; int ld;
    __device__ __forceinline__ int operator()(int a, int b) const { return (int)mat[(size_t)a * ld + b]; }
};

template <typename T>
__global__ void __launch_bounds__(HK_BT) k_hk_zero(HkBuf H, const T *__restrict__ mat, int n, int ld)
{
    hk_zero(H, HkMatCost<T>{mat, ld}, n);
}
template <int KIND>
__global__ void __launch_bounds__(HK_BT) k_hk_zero_otf(HkBuf H, const typename OrPt<KIND>::type *__restrict__ pts, int n)
{
    hk_zero(H, OrPtsCost<KIND>{pts}, n);
}

// comp[] and pi[] of the nodes 0 .. ld - 1 into the workgroup's dynamic LDS: [ld] multipliers, then [ld] labels
__device__ __forceinline__ void hk_stage(const HkBuf &H, int ld, long long *lpi, int *lcomp)
{
    for (int i = threadIdx.x; i < ld; i += HK_ROWS * 64) { lpi[i] = H.pi[i]; lcomp[i] = H.comp[i]; }
    __syncthreads();
}

// best(v) of the wave's lane-local (bw, bu), bw without pi[v]: the weight to the component, both to the node
__device__ __forceinline__ void hk_post(const HkBuf &H, int v, int cv, long long pv, long long bw, int bu, int lane)
{
    const long long mw = wave_min_i64(bw);
    const int mu = (int)wave_min_i64(bw == mw ? (long long)bu : (long long)INT_MAX);
    if (lane != 0) return;
    if (mw == HK_WMAX) { H.bw[v] = HK_WMAX; H.be[v] = HK_ENONE; return; }
    H.bw[v] = mw + pv; H.be[v] = hk_pair(v, mu);
    hk_min(&H.cw[cv], mw + pv);
}

template <typename T, bool STAGE>
__global__ void __launch_bounds__(HK_ROWS * 64) k_hk_scan(HkBuf H, const T *__restrict__ mat, int n, int ld)
{
    typedef typename Elem<T>::vec VT;
    constexpr int V = Elem<T>::V;
    extern __shared__ __attribute__((aligned(16))) unsigned char hk_lds[];
    if (H.ctl->stop || H.ctl->done) return;             // (the whole grid alike: no barrier is left waiting)
    const long long *gpi = H.pi;
    const int *gcomp = H.comp;
    if constexpr (STAGE) {
        long long *lpi = reinterpret_cast<long long *>(hk_lds);
        int *lcomp = reinterpret_cast<int *>(hk_lds + (size_t)ld * 8);
        hk_stage(H, ld, lpi, lcomp);
        gpi = lpi; gcomp = lcomp;
    }
    const int lane = threadIdx.x & 63, v = 1 + (int)blockIdx.x * HK_ROWS + (threadIdx.x >> 6);
    if (v >= n) return;                                     // (a whole wave, behind the only barrier)
    const int cv = gcomp[v];
    const long long pv = gpi[v];
    const VT *row = reinterpret_cast<const VT *>(mat + (size_t)v * ld);
    const int nvec = ld / V;                                // ld is a multiple of 32 cells: whole vectors, inside the row
    long long bw = HK_WMAX; int bu = INT_MAX;
    for (int i = lane; i < nvec; i += 64) {
        const VT x = row[i];
        const int u0 = i * V;
        int cu[V]; long long pu[V];
        load_run<V>(gcomp + u0, cu);
        load_run<V>(gpi + u0, pu);
#pragma unroll
        for (int e = 0; e < V; e++) {
            const int u = u0 + e;
            const long long w = HK_S * (long long)vget(x, e) + pu[e];
            if (u >= 1 && u < n && cu[e] != cv && w < bw) { bw = w; bu = u; }
        }
    }
    hk_post(H, v, cv, pv, bw, bu, lane);
}

template <int KIND, bool STAGE>
__global__ void __launch_bounds__(HK_ROWS * 64) k_hk_scan_otf(HkBuf H, const typename OrPt<KIND>::type *__restrict__ pts, int n, int ld)
{
    typedef typename OrPt<KIND>::type PT;
    extern __shared__ __attribute__((aligned(16))) unsigned char hk_lds[];
    if (H.ctl->stop || H.ctl->done) return;
    const long long *gpi = H.pi;
    const int *gcomp = H.comp;
    if constexpr (STAGE) {
        long long *lpi = reinterpret_cast<long long *>(hk_lds);
        int *lcomp = reinterpret_cast<int *>(hk_lds + (size_t)ld * 8);
        hk_stage(H, ld, lpi, lcomp);
        gpi = lpi; gcomp = lcomp;
    }
    const int lane = threadIdx.x & 63, v = 1 + (int)blockIdx.x * HK_ROWS + (threadIdx.x >> 6);
    if (v >= n) return;
    const int cv = gcomp[v];
    const long long pv = gpi[v];
    const PT p = pts[v];
    long long bw = HK_WMAX; int bu = INT_MAX;
    for (int u = lane; u < n; u += 64) {
        if (u == 0 || gcomp[u] == cv) continue;             // (v itself is of v's component)
        const long long w = HK_S * (long long)or_weight<KIND>(p, pts[u]) + gpi[u];
        if (w < bw) { bw = w; bu = u; }
    }
    hk_post(H, v, cv, pv, bw, bu, lane);
}

__global__ void __launch_bounds__(HK_BT) k_hk_cmin(HkBuf H, int n)
{
    if (H.ctl->stop || H.ctl->done) return;
    const int v = 1 + blockIdx.x * HK_BT + threadIdx.x;
    if (v >= n) return;
    const long long w = H.bw[v];
    const int c = H.comp[v];
    if (w != HK_WMAX && w == H.cw[c]) hk_min(&H.ce[c], H.be[v]);
}

// one thread per label c that is a root with an edge {a, b}: a in c, b in c2 (or the other way round)
__global__ void __launch_bounds__(HK_BT) k_hk_hook(HkBuf H, int n)
{
    HkCtl *C = H.ctl;
    if (C->stop || C->done) return;
    const int c = 1 + blockIdx.x * HK_BT + threadIdx.x;
    if (c >= n || H.comp[c] != c) return;
    const u64 e = H.ce[c];
    if (e == HK_ENONE) return;
    const int a = (int)(e >> 32), b = (int)(unsigned)e;
    if ((unsigned)a >= (unsigned)n || (unsigned)b >= (unsigned)n) { C->err = 1; return; }
    const int ca = H.comp[a], c2 = ca == c ? H.comp[b] : ca;
    const bool mutual = H.ce[c2] == e;      // (equal pairs are equal keys)
    if (mutual && c < c2) return;           // the smaller label stays a root, the other one records the edge
    H.up[c] = c2;
    const unsigned k = atomicAdd(&C->nedges, 1u);
    if (k >= (unsigned)(n - 2)) { C->err = 1; return; }
    H.edges[2 + k] = e;
    atomicAdd(&H.deg[a], 1); atomicAdd(&H.deg[b], 1);
    hk_add(&C->wsum, H.cw[c]);
}

__global__ void __launch_bounds__(HK_BT) k_hk_flat(HkBuf H, int n)
{
    HkCtl *C = H.ctl;
    if (C->stop || C->done) return;
    const int v = blockIdx.x * HK_BT + threadIdx.x;
    const unsigned k = C->nedges;            // (the hooks of this round are all in)
    if (v >= 1 && v < n) {
        int r = H.comp[v], steps = 0;
        for (int p = H.up[r]; p != r && steps <= n; p = H.up[r], steps++) r = p;
        if (steps > n) C->err = 1;
        H.comp[v] = r;
        H.cw[v] = HK_WMAX; H.ce[v] = HK_ENONE;
    }
    if (v == 0) {
        if (k != C->seen) { C->rounds += 1; C->seen = k; }
        if (k >= (unsigned)(n - 2)) C->done = 1;
    }
}

// block-wide sum / maximum of a 64-bit value over HK_STEP_BT threads, valid in every thread (scratch: HK_STEP_BT / 64 slots)
template <bool MAX> __device__ __forceinline__ long long hk_block(long long x, long long *scratch)
{
    for (int off = 32; off > 0; off >>= 1) {
        const long long o = __shfl_xor(x, off);
        x = MAX ? (o > x ? o : x) : x + o;
    }
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = x;
    __syncthreads();
    long long r = scratch[0];
    for (int k = 1; k < HK_STEP_BT / 64; k++) r = MAX ? (scratch[k] > r ? scratch[k] : r) : r + scratch[k];
    __syncthreads();
    return r;
}

// rule 3 behind the tree in hand, one workgroup
__global__ void __launch_bounds__(HK_STEP_BT) k_hk_step(HkBuf H, int n)
{
    __shared__ long long scratch[HK_STEP_BT / 64];
    HkCtl *C = H.ctl;
    if (C->stop) return;
    const int tid = threadIdx.x;
    if (!C->done || C->err) { if (tid == 0) C->stop = 6 + 1; return; }     // (no tree: the host answers INTERNAL)
    long long spi = 0, q = 0;
    for (int v = tid; v < n; v += HK_STEP_BT) {
        const long long g = H.deg[v] - 2;
        spi += H.pi[v]; q += g * g;
    }
    spi = hk_block<false>(spi, scratch);
    q = hk_block<false>(q, scratch);
    const long long L = C->wsum - 2 * spi;
    const int h0 = C->h, bad0 = C->bad;
    const bool better = !C->have_best || L > C->best;
    __syncthreads();                        // (every thread has read the state thread 0 rewrites)
    if (better)
        for (int v = tid; v < n; v += HK_STEP_BT) H.pibest[v] = H.pi[v];
    int h = h0;
    if (!better && bad0 + 1 >= C->patience) h = h0 + 1;
    const long long gap = C->ubs - L;
    const long long t = (q == 0 || gap <= 0 || h >= 62) ? 0 : ((2 * gap) >> h) / q;
    int why = q == 0 ? 1 : gap <= 0 ? 2 : t == 0 ? 3 : 0;
    if (!why) {
        long long over = 0;
        for (int v = tid; v < n; v += HK_STEP_BT) {
            const long long x = H.pi[v] + t * (long long)(H.deg[v] - 2);
            over |= (x > HK_PI_MAX || x < -HK_PI_MAX) ? 1 : 0;
        }
        if (hk_block<true>(over, scratch)) why = 5;
    }
    if (!why)
        for (int v = tid; v < n; v += HK_STEP_BT) H.pi[v] += t * (long long)(H.deg[v] - 2);
    if (tid == 0) {
        if (better) { C->best = L; C->have_best = 1; C->bad = 0; }
        else if (bad0 + 1 >= C->patience) { C->h = h; C->bad = 0; }
        else C->bad = bad0 + 1;
        C->iters += 1;
        if (why) C->stop = why + 1;
    }
}
