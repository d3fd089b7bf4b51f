// Greedy-edge tour construction over the neighbour lists (include/tspgpu.h "Greedy-edge construction", DESIGN 4.21).
// Included by tspgpu.hip behind tspgpu_nl2opt.inc (NlBuf) and the kernels above it (Tours, cell<T>).
//
// The sequential rule takes edges in ascending key order (c[a][b], a, b) and accepts each one that is valid when reached.  The
// kernels compute the same set in rounds of locally dominant edges, with no sort: best(v) is the smallest valid key at v, a
// fragment's best the smaller of its two ends', and an edge is accepted iff it is the best of both fragments it joins.  Accepted
// edges of a round join disjoint pairs of fragments, so one thread per edge links them with plain stores.
//
// A round is four launches (phase 1: two passes of atomic minima over the lists, accept, link; phase 2: compact the free nodes,
// a wave per free node over the free list, accept, link).  No kernel waits on another workgroup; what one launch writes the next
// reads.  The host launches rounds in batches; every kernel returns at once when the phase's `done` word is set.
//   accept and link are two launches: accept reads best() and other_end[] of OTHER fragments' ends, which link rewrites.

constexpr u64 GE_NONE = ~0ull;
constexpr int GE_BT = 256;

struct GeCtl {              // control block of one construction (zeroed by the host in front of it)
    int done[2];            // per phase: 0 running; r + 1: finished by the link of its round r
    unsigned acc[2];        // edges accepted by the round in hand, by round parity (the link of round r zeroes the other one)
    unsigned nfree[2];      // phase 2: the length of the free list, by round parity
    unsigned rounds[2];     // rounds that accepted an edge, per phase
    unsigned edges[2];      // edges accepted, per phase
    unsigned free_in;       // free nodes (degree < 2) entering phase 2
    int pad;
};

struct GeBuf {
    u64 *bw, *be;           // [n] best(v): the cost's order key and (a << 32 | b); GE_NONE: no valid edge at v
    int *adj;               // [2n] the accepted edges at v: adj[2v], adj[2v + 1]; -1: none yet
    int *deg, *oe, *acc;    // [n] degree; the far end of the fragment v is an end of (a node of its own: v); v accepts its best
    int *fl;                // [n] phase 2: the nodes of degree < 2, in no particular order
    int *nxt, *dist;        // [2][2n] list ranking over the darts 2v + side
    GeCtl *ctl;
};

// the order of costs as an unsigned integer: doubles' bits folded so that the integer order is the doubles' order (-0.0 is
// taken as +0.0: the two compare equal as doubles).  Integer cells are exact as doubles
template <typename AT> __device__ __forceinline__ u64 ge_wkey(AT w)
{
    const u64 b = (u64)__double_as_longlong((double)w + 0.0);
    return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
}
__device__ __forceinline__ u64 ge_ekey(int a, int b) { return a < b ? ((u64)(unsigned)a << 32) | (unsigned)b : ((u64)(unsigned)b << 32) | (unsigned)a; }
__device__ __forceinline__ bool ge_less(u64 w1, u64 e1, u64 w2, u64 e2) { return w1 < w2 || (w1 == w2 && e1 < e2); }
__device__ __forceinline__ void ge_min(u64 *p, u64 x) { __hip_atomic_fetch_min(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(GE_BT) k_ge_init(GeBuf G, int n)
{
    const int v = blockIdx.x * GE_BT + threadIdx.x;
    if (v >= n) return;
    G.bw[v] = GE_NONE; G.be[v] = GE_NONE;
    G.adj[2 * v] = -1; G.adj[2 * v + 1] = -1;
    G.deg[v] = 0; G.oe[v] = v; G.acc[v] = 0;
}

// Phase 1, the two passes over the list edges {v, u}, u in N(v), valid now: degree < 2 at both ends and u not the far end of
// v's fragment.  PASS 0 posts the cost key to both ends, PASS 1 the edge among those whose cost is the end's minimum.  The
// weights are the lists' own (AT: int in the integer modes, double for f64 cells), so no cost source is read
template <typename AT, int PASS>
__global__ void __launch_bounds__(GE_BT) k_ge_p1(GeBuf G, NlBuf L, int n)
{
    if (G.ctl->done[0]) return;
    const int v = blockIdx.x * GE_BT + threadIdx.x;
    if (v >= n || G.deg[v] >= 2) return;
    const int K = L.K, oev = G.oe[v];
    const int *nd = L.node + (size_t)v * K;
    const AT *w = reinterpret_cast<const AT *>(L.w) + (size_t)v * K;
    const u64 bv = PASS ? G.bw[v] : 0;
    u64 mine = GE_NONE;
    for (int j = 0; j < K; j++) {
        const int u = nd[j];
        if ((unsigned)u >= (unsigned)n || u == v || u == oev || G.deg[u] >= 2) continue;
        const u64 k = ge_wkey<AT>(w[j]);
        if (PASS == 0) {
            mine = k < mine ? k : mine;
            ge_min(&G.bw[u], k);
        } else {
            const u64 e = ge_ekey(v, u);
            if (k == bv && e < mine) mine = e;
            if (k == G.bw[u]) ge_min(&G.be[u], e);
        }
    }
    if (mine != GE_NONE) ge_min(PASS ? &G.be[v] : &G.bw[v], mine);
}

// Phase 2: the free list of this round, one ballot and one atomic add per wave
__global__ void __launch_bounds__(GE_BT) k_ge_p2_compact(GeBuf G, int n, int par)
{
    if (G.ctl->done[1]) return;
    const int v = blockIdx.x * GE_BT + threadIdx.x, lane = threadIdx.x & 63;
    const bool is_free = v < n && G.deg[v] < 2;
    const u64 mask = __ballot(is_free);
    if (!mask) return;
    const int leader = __ffsll((long long)mask) - 1;
    unsigned base = 0;
    if (lane == leader) base = __hip_atomic_fetch_add(&G.ctl->nfree[par], (unsigned)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = __shfl(base, leader);
    const unsigned at = base + (unsigned)__popcll(mask & ((1ull << lane) - 1));
    if (is_free && at < (unsigned)n) G.fl[at] = v;
}

// Phase 2: a wave per free node a scans the free list for the smallest key {a, b}, b not the far end of a's fragment.  The edge
// set is symmetric (both ends see the edge), so no atomics: lane 0 stores best(a).  Costs through cell<T>, lower node first
template <typename T>
__global__ void __launch_bounds__(GE_BT) k_ge_p2_best(GeBuf G, const T *__restrict__ mat, const double2 *__restrict__ pts, int kind, int ld, int n,
                                                      int par)
{
    typedef typename Elem<T>::acc AT;
    if (G.ctl->done[1]) return;
    const int m = (int)min(G.ctl->nfree[par], (unsigned)n);
    const int lane = threadIdx.x & 63, nwaves = (gridDim.x * GE_BT) >> 6;
    for (int i = (blockIdx.x * GE_BT + threadIdx.x) >> 6; i < m; i += nwaves) {
        const int a = G.fl[i], oea = G.oe[a];
        u64 bw = GE_NONE, be = GE_NONE;
        for (int j = lane; j < m; j += 64) {
            const int b = G.fl[j];
            if (b == a || b == oea) continue;
            const AT c = a < b ? cell<T>(mat, pts, kind, ld, a, b) : cell<T>(mat, pts, kind, ld, b, a);
            const u64 k = ge_wkey<AT>(c), e = ge_ekey(a, b);
            if (ge_less(k, e, bw, be)) { bw = k; be = e; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const u64 ow = __shfl_xor(bw, off), oe2 = __shfl_xor(be, off);
            if (ge_less(ow, oe2, bw, be)) { bw = ow; be = oe2; }
        }
        if (lane == 0) { G.bw[a] = bw; G.be[a] = be; }
    }
}

// Both phases: the lower end a of best(a) = {a, b} accepts it iff it is best(b) too and smaller than the bests of the two
// fragments' far ends.  acc[v] for every node, the round's count by one atomic add per wave
__global__ void __launch_bounds__(GE_BT) k_ge_accept(GeBuf G, int n, int ph, int par)
{
    if (G.ctl->done[ph]) return;
    const int v = blockIdx.x * GE_BT + threadIdx.x;
    bool ok = false;
    if (v < n && G.deg[v] < 2) {
        const u64 bw = G.bw[v], be = G.be[v];
        const int a = (int)(be >> 32), b = (int)(unsigned)be;
        if (bw != GE_NONE && a == v && (unsigned)b < (unsigned)n && G.deg[b] < 2 && G.bw[b] == bw && G.be[b] == be) {
            const int oa = G.oe[a], ob = G.oe[b];
            ok = (oa == a || ge_less(bw, be, G.bw[oa], G.be[oa])) && (ob == b || ge_less(bw, be, G.bw[ob], G.be[ob]));
        }
    }
    if (v < n) G.acc[v] = ok ? 1 : 0;
    const u64 mask = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && mask)
        __hip_atomic_fetch_add(&G.ctl->acc[par], (unsigned)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Both phases, round r of phase ph: the accepting nodes link (adjacency, degrees, other_end: the two fragments of an accepted
// edge are touched by its thread alone), every best() is reset, and thread 0 keeps the books: the phase is over when the round
// accepted nothing (no valid edge is left: the globally smallest one is always accepted) or, in phase 2, when n - 1 edges stand
__global__ void __launch_bounds__(GE_BT) k_ge_link(GeBuf G, int n, int ph, int r)
{
    GeCtl *C = G.ctl;
    const int d = C->done[ph];
    if (d && d != r + 1) return;        // (r + 1: thread 0 of this very launch wrote it)
    const int par = r & 1;
    const unsigned k = C->acc[par];
    const int v = blockIdx.x * GE_BT + threadIdx.x;
    if (v < n) {
        if (k && G.acc[v]) {
            const int a = v, b = (int)(unsigned)G.be[v];
            const int oa = G.oe[a], ob = G.oe[b], da = G.deg[a], db = G.deg[b];
            if (da < 2 && db < 2) {
                G.adj[2 * a + da] = b; G.adj[2 * b + db] = a;
                G.deg[a] = da + 1; G.deg[b] = db + 1;
                G.oe[oa] = ob; G.oe[ob] = oa;
            }
        }
        G.bw[v] = GE_NONE; G.be[v] = GE_NONE;
    }
    if (v == 0) {
        C->acc[par ^ 1] = 0;
        if (ph == 1 && r == 0) C->free_in = C->nfree[0];
        C->nfree[par ^ 1] = 0;
        if (k) { C->rounds[ph] += 1; C->edges[ph] += k; }
        if (k == 0 || (ph == 1 && C->edges[0] + C->edges[1] >= (unsigned)(n - 1))) C->done[ph] = r + 1;
    }
}

// the edge between the two ends of the single fragment closes the tour
__global__ void __launch_bounds__(GE_BT) k_ge_close(GeBuf G, int n)
{
    const int v = blockIdx.x * GE_BT + threadIdx.x;
    if (v < n && G.deg[v] == 1) { G.adj[2 * v + 1] = G.oe[v]; G.deg[v] = 2; }
}

// ---- the closed adjacency into ord[]: list ranking by pointer jumping over the 2n darts d = 2v + side ("at v, leaving through
// adj[d]"), cut at node 0.  The darts form the two directions of the tour; the darts of node 0 are the ends of both lists.
__global__ void __launch_bounds__(GE_BT) k_ge_rank_init(GeBuf G, int n)
{
    const int d = blockIdx.x * GE_BT + threadIdx.x;
    if (d >= 2 * n) return;
    const int v = d >> 1, u = G.adj[d];
    if (v == 0 || (unsigned)u >= (unsigned)n) { G.nxt[d] = d; G.dist[d] = 0; return; }
    G.nxt[d] = 2 * u + (G.adj[2 * u] == v ? 1 : 0);   // at u, leaving through the side that does not lead back
    G.dist[d] = 1;
}

__global__ void __launch_bounds__(GE_BT) k_ge_rank_jump(const int *__restrict__ nxt, const int *__restrict__ dist, int *__restrict__ nxt2,
                                                        int *__restrict__ dist2, int n2)
{
    const int d = blockIdx.x * GE_BT + threadIdx.x;
    if (d >= n2) return;
    const int t = nxt[d];
    dist2[d] = dist[d] + dist[t];
    nxt2[d] = nxt[t];
}

// Orientation: the order starts at node 0 and goes on to the smaller-numbered of its two neighbours.  The darts of that direction
// end in the dart of node 0 that leaves towards that neighbour; such a dart at v is n - P(v) hops away from it
__global__ void __launch_bounds__(GE_BT) k_ge_rank_out(GeBuf G, const int *__restrict__ nxt, const int *__restrict__ dist, Tours S, int slot, int n)
{
    const int d = blockIdx.x * GE_BT + threadIdx.x;
    if (d >= 2 * n) return;
    int *ord = S.ord + (size_t)slot * n;
    if (d < 2) { if (d == 0) ord[0] = 0; return; }
    const int d0 = G.adj[0] < G.adj[1] ? 0 : 1;
    const int p = n - dist[d];
    if (nxt[d] == d0 && p >= 1 && p < n) ord[p] = d >> 1;
}
