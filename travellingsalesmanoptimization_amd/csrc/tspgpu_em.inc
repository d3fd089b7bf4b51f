// ---------------------------------------------------------------------------
// Extra Mileage: h_ExtraMileage (src/algorithms/heuristics.c:156-210) and h_extramileage_util (:290-367).
// Included by tspgpu.hip (uses Elem, edge_w, wave_min_i64, wall_clock64).
//
// Farthest pair (EM_MAX, :165-177): the first strictly largest c(i, j) over i < j in row-major order = the largest
// packed key  w << 35 | (2^35 - 1 - (i n + j))  (w < 2^27, i n + j < n^2 <= 2^34): one workgroup per row i, one 64-bit
// atomic max per workgroup.  All costs 0 -> (0, 1), the reference's initial values.
//
// Cheapest insertion (:311-363) in its INCREMENTAL form.  The reference rescans every (unvisited i, edge j) each step
// and keeps the first strict minimum of delta = c[u][i] + c[i][v] - c[u][v], i.e. the lexicographic minimum of
// (delta, i, j).  Here every unvisited i keeps best[i] = min (delta(i, j), j) over the current edges.  Inserting x
// into edge e = (u, v) sets E[e] = (u, x) in place and appends E[m] = (x, v), m = the edge count; then per unvisited i:
//   * bj[i] == e: the edge i relied on changed -> i is STALE and rescans all edges;
//   * else best[i] = lexmin(best[i], (delta(i, e), e), (delta(i, m), m)) (m is the largest index: a strict < on delta).
// The next winner is min (bd[i], i) over the unvisited nodes.  Weights are integers below 2^27 (checked on the host),
// so every delta and key is an exact integer.
//
// Device state (one allocation per call): E as three arrays (u, v, c(u, v): an evaluation costs two weights), succ,
// skey[i] = (bd + EM_BIAS) << 34 | bj << 17 | v(bj) (EM_NONE: visited, or stale while it is rescanned), three stale
// lists, and the control block EmCtl.  A step s (s = 0 .. n-3) is two phases:
//   A  every workgroup reads the winner of step s (x, e; u = E[e].u, which never changes; v from skey[x], written when
//      bj[x] was last set and valid since: a change of E[bj] would have made x stale), updates the nodes it owns
//      (contiguous strides of the grid), lists the stale ones, and offers its best non-stale key for step s + 1;
//      workgroup 0 lane 0 applies the insertion (E, succ, the delta sum).
//   B  the stale nodes are rescanned over all edges, the grid split into groups of W / (stale count) workgroups per
//      node, each group member a slice of the edges (block minimum, one atomic min into skey[i], one into the step key);
//      workgroup 0 lane 0 marks x visited, clears the buffers of step s + 2 and checks the deadline.
// Keys of three consecutive steps live in three rotating buffers, so a buffer is cleared two phases after its last read.
//
// Two forms with the same phases: RESIDENT -- one launch for the whole construction, one workgroup per CU, a grid
// barrier (drained stores, agent-scope release, a counter, agent-scope acquire, then plain loads) between
// phases, a 2 ms rendezvous first (as k_lds2opt) -- and PER STEP (the default: faster, DESIGN 4.11) -- k_em_init then k_em_a / k_em_b per step,
// enqueued back to back (the kernel boundary is the barrier).  Words touched by atomics (keys, skey, counters) are
// read with agent-scope atomic loads; E / succ / the stale lists are plain stores released at the barrier.
// ---------------------------------------------------------------------------
static constexpr int EM_BT = 256;
static constexpr int EM_IB = 17;                               // bits of a node / edge index (n <= 131 072)
static constexpr u64 EM_IM = (1ull << EM_IB) - 1;
static constexpr long long EM_BIAS = 1ll << 27;                // delta in (-2^27, 2^28): biased, 29 bits
static constexpr u64 EM_NONE = 0x7FFFFFFFFFFFFFFFull;          // above every real key (signed or not)
static constexpr u64 EM_FMASK = (1ull << 35) - 1;
enum { EM_ST_OK = 0, EM_ST_NO_RENDEZVOUS = 1, EM_ST_LOST = 2, EM_ST_BROKEN = 3 };

struct EmCtl {              // zeroed before every call (one 96-byte memset)
    u64 keys[3];            // step keys, COMPLEMENTED (0 = none yet): ~((d + EM_BIAS) << 34 | i << 17 | j), atomic max
    long long dsum;         // sum of the inserted deltas (workgroup 0, lane 0; like every word here, agent-scope atomics)
    long long stale;        // stale rescans so far
    long long t0;           // wall clock (10 ns ticks) at the start
    int cnt[3];             // stale-list lengths
    int bar;                // grid-barrier arrivals (resident form)
    int status;             // EM_ST_*
    int stop;               // 1: the deadline passed (the partial tour is not returned)
    int cab;                // c(a, b)
    int steps;              // insertions applied
    int pad[4];
};
static_assert(sizeof(EmCtl) == 96, "EmCtl is memset as 96 bytes");

// integer weight c[u][v]: the resident matrix (any cell type) or the coordinates (matrix-free, the sweeps' edge_w)
template <typename T> struct EmMat {
    const T *mat; int ld; bool sym;
    __device__ __forceinline__ int operator()(int u, int v) const { return (int)mat[(size_t)u * ld + v]; }
    // c[i][v] read from row v when the matrix is symmetric (coalesced over consecutive i)
    __device__ __forceinline__ int out(int i, int v) const { return sym ? (int)mat[(size_t)v * ld + i] : (int)mat[(size_t)i * ld + v]; }
};
template <int KIND> struct EmPts {
    const double2 *pts;
    __device__ __forceinline__ int operator()(int u, int v) const { const double2 a = pts[u], b = pts[v]; return edge_w<KIND>(a.x, a.y, b.x, b.y); }
    __device__ __forceinline__ int out(int i, int v) const { return (*this)(i, v); }
};

struct EmArgs {
    const void *mat; const double2 *pts; int ld, n; bool sym;
    int *eu, *ev, *ec;      // edges [n]
    int *succ;              // [n]
    u64 *skey;              // [n]
    int *stale;             // [3][n]
    EmCtl *ctl;
    long long limit;        // deadline in ticks after t0 (< 0: none)
    long long hello, spin;  // rendezvous / barrier limits in ticks
};

template <typename WF> __device__ __forceinline__ WF em_wf(const EmArgs &A);
template <> __device__ __forceinline__ EmMat<u16> em_wf(const EmArgs &A) { return {(const u16 *)A.mat, A.ld, A.sym}; }
template <> __device__ __forceinline__ EmMat<int> em_wf(const EmArgs &A) { return {(const int *)A.mat, A.ld, A.sym}; }
template <> __device__ __forceinline__ EmMat<double> em_wf(const EmArgs &A) { return {(const double *)A.mat, A.ld, A.sym}; }
template <> __device__ __forceinline__ EmPts<0> em_wf(const EmArgs &A) { return {A.pts}; }
template <> __device__ __forceinline__ EmPts<1> em_wf(const EmArgs &A) { return {A.pts}; }
template <> __device__ __forceinline__ EmPts<2> em_wf(const EmArgs &A) { return {A.pts}; }

__device__ __forceinline__ u64 em_ld(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void em_st(u64 *p, u64 x) { __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int em_ldi(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void em_sti(int *p, int x) { __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ u64 em_pack(long long d, int hi, int lo) { return (u64)(d + EM_BIAS) << 34 | (u64)hi << EM_IB | (u64)lo; }
__device__ __forceinline__ long long em_d(u64 k) { return (long long)(k >> 34) - EM_BIAS; }

// block-wide minimum of a key below 2^63 (valid in lane 0 of wave 0)
__device__ __forceinline__ u64 em_block_min(u64 k, u64 *scr)
{
    k = (u64)wave_min_i64((long long)k);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) scr[w] = k;
    __syncthreads();
    if (threadIdx.x == 0) for (int i = 1; i < (int)(blockDim.x >> 6); i++) k = scr[i] < k ? scr[i] : k;
    __syncthreads();
    return k;
}

// grid barrier of the resident form: every wave drains its stores, lane 0 releases, counts, polls, acquires.  Returns
// false (uniform) when the wait passed `limit` ticks or another workgroup gave up; `code` is then recorded.
__device__ __forceinline__ bool em_barrier(EmCtl *C, int target, long long limit, int code)
{
    __shared__ int ok;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_fetch_add(&C->bar, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int r = 1;
        const long long tp = wall_clock64();
        for (int spins = 0; em_ldi(&C->bar) < target;) {
            __builtin_amdgcn_s_sleep(1);
            if ((++spins & 15) == 0 && (em_ldi(&C->status) != EM_ST_OK || wall_clock64() - tp > limit)) { r = 0; break; }
        }
        if (!r) {
            int expect = EM_ST_OK;
            __hip_atomic_compare_exchange_strong(&C->status, &expect, code, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ok = r;
    }
    __syncthreads();
    return ok != 0;
}

// start: E[0] = (a, b), E[1] = (b, a), succ, cost 2 c(a, b) (:162-186, :297-302); best of every other node over both edges
template <typename WF>
__device__ __forceinline__ void em_init(const EmArgs &A, int a, int b, u64 *scr)
{
    const WF c = em_wf<WF>(A);
    const int n = A.n, tid = threadIdx.x, gs = (int)(gridDim.x * blockDim.x);
    const int cab = c(a, b), cba = c(b, a);
    u64 best = EM_NONE;
    for (int i = blockIdx.x * blockDim.x + tid; i < n; i += gs) {
        if (i == a || i == b) { em_st(A.skey + i, EM_NONE); continue; }
        const long long d0 = (long long)c(a, i) + c.out(i, b) - cab, d1 = (long long)c(b, i) + c.out(i, a) - cba;
        const bool one = d1 < d0;
        const long long d = one ? d1 : d0;
        em_st(A.skey + i, em_pack(d, one ? 1 : 0, one ? a : b));
        const u64 k = em_pack(d, i, one ? 1 : 0);
        best = k < best ? k : best;
    }
    best = em_block_min(best, scr);
    if (tid == 0) {
        if (best != EM_NONE) __hip_atomic_fetch_max(&A.ctl->keys[0], ~best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (blockIdx.x == 0) {
            A.eu[0] = a; A.ev[0] = b; A.ec[0] = cab;
            A.eu[1] = b; A.ev[1] = a; A.ec[1] = cba;
            A.succ[a] = b; A.succ[b] = a;
            em_sti(&A.ctl->cab, cab);
            __hip_atomic_store(&A.ctl->t0, (long long)wall_clock64(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// phase A of step s: insert the winner of step s, update the non-stale nodes, list the stale ones
template <typename WF>
__device__ __forceinline__ void em_phase_a(const EmArgs &A, int s, u64 *scr)
{
    const WF c = em_wf<WF>(A);
    const int n = A.n, tid = threadIdx.x, gs = (int)(gridDim.x * blockDim.x);
    EmCtl *C = A.ctl;
    const u64 K = ~em_ld(&C->keys[s % 3]);
    const long long dx = em_d(K);
    const int x = (int)((K >> EM_IB) & EM_IM), e = (int)(K & EM_IM), m = s + 2;
    // (a winner outside the state -- no candidate was offered -- would index past the arrays: stop, uniformly)
    if (x >= n || e >= m) { if (blockIdx.x == 0 && tid == 0) em_sti(&C->status, EM_ST_BROKEN); em_sti(&C->stop, 1); return; }
    const int u = A.eu[e], v = (int)(em_ld(A.skey + x) & EM_IM);
    if (v >= n) { if (blockIdx.x == 0 && tid == 0) em_sti(&C->status, EM_ST_BROKEN); em_sti(&C->stop, 1); return; }
    const int cux = c(u, x), cxv = c(x, v);
    if (blockIdx.x == 0 && tid == 0) {      // the insertion (:339-360): E[e] = (u, x) in place, E[m] = (x, v)
        A.ev[e] = x; A.ec[e] = cux;
        A.eu[m] = x; A.ev[m] = v; A.ec[m] = cxv;
        A.succ[u] = x; A.succ[x] = v;
        __hip_atomic_fetch_add(&C->dsum, dx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        em_sti(&C->steps, s + 1);
    }
    if (s == n - 3) return;                 // the last node is in
    const int nb = (s + 1) % 3;
    u64 best = EM_NONE;
    for (int i = blockIdx.x * blockDim.x + tid; i < n; i += gs) {
        if (i == x) continue;
        const u64 sk = em_ld(A.skey + i);
        if (sk == EM_NONE) continue;        // visited
        const int bj = (int)((sk >> EM_IB) & EM_IM);
        if (bj == e) {                      // stale: rescanned in phase B
            em_st(A.skey + i, EM_NONE);
            const int q = __hip_atomic_fetch_add(&C->cnt[nb], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            A.stale[(size_t)nb * n + q] = i;
            continue;
        }
        long long bd = em_d(sk);
        int j = bj, bv = (int)(sk & EM_IM);
        const long long de = (long long)c(u, i) + c.out(i, x) - cux;
        if (de < bd || (de == bd && e < j)) { bd = de; j = e; bv = x; }
        const long long dm = (long long)c(x, i) + c.out(i, v) - cxv;
        if (dm < bd) { bd = dm; j = m; bv = v; }
        if (j != bj) em_st(A.skey + i, em_pack(bd, j, bv));
        const u64 k = em_pack(bd, i, j);
        best = k < best ? k : best;
    }
    best = em_block_min(best, scr);
    if (tid == 0 && best != EM_NONE) __hip_atomic_fetch_max(&C->keys[nb], ~best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// phase B of step s: rescan the stale nodes over the s + 3 edges; bookkeeping; the deadline
template <typename WF>
__device__ __forceinline__ void em_phase_b(const EmArgs &A, int s, u64 *scr)
{
    const WF c = em_wf<WF>(A);
    const int n = A.n, tid = threadIdx.x, W = (int)gridDim.x, wg = (int)blockIdx.x, k = s + 3;
    EmCtl *C = A.ctl;
    const int nb = (s + 1) % 3;
    const int cnt = em_ldi(&C->cnt[nb]);
    if (cnt > 0) {
        const int G = cnt <= W ? W / cnt : 1;                  // workgroups per stale node
        const int q0 = wg / G, r = wg % G;
        const int j0 = (int)((long long)r * k / G), j1 = (int)((long long)(r + 1) * k / G);
        for (int q = q0; q < cnt; q += W) {             // (cnt <= W: one node per group)
            const int i = A.stale[(size_t)nb * n + q];
            u64 best = EM_NONE;
            for (int j = j0 + tid; j < j1; j += blockDim.x) {
                const int eu = A.eu[j], ev = A.ev[j];
                const long long d = (long long)c(eu, i) + c.out(i, ev) - A.ec[j];
                const u64 kk = em_pack(d, j, ev);
                best = kk < best ? kk : best;
            }
            best = em_block_min(best, scr);
            if (tid == 0 && best != EM_NONE) {
                __hip_atomic_fetch_min(A.skey + i, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const u64 gk = em_pack(em_d(best), i, (int)((best >> EM_IB) & EM_IM));
                __hip_atomic_fetch_max(&C->keys[nb], ~gk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (wg == 0 && tid == 0) {
        const u64 K = ~em_ld(&C->keys[s % 3]);
        const int x = (int)((K >> EM_IB) & EM_IM);
        if (x < n) em_st(A.skey + x, EM_NONE);   // x is in the tour (every workgroup has read its v)
        em_st(&C->keys[(s + 2) % 3], 0);
        em_sti(&C->cnt[(s + 2) % 3], 0);
        __hip_atomic_fetch_add(&C->stale, (long long)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (A.limit >= 0 && wall_clock64() - __hip_atomic_load(&C->t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > A.limit)
            em_sti(&C->stop, 1);
    }
}

template <typename WF>
__global__ void __launch_bounds__(EM_BT) k_em_resident(EmArgs A, int a, int b)
{
    __shared__ u64 scr[EM_BT / 64];
    const int W = (int)gridDim.x;
    int nbar = 0;
    if (!em_barrier(A.ctl, ++nbar * W, A.hello, EM_ST_NO_RENDEZVOUS)) return;
    em_init<WF>(A, a, b, scr);
    if (!em_barrier(A.ctl, ++nbar * W, A.spin, EM_ST_LOST)) return;
    for (int s = 0; s <= A.n - 3; s++) {
        if (em_ldi(&A.ctl->stop)) return;
        em_phase_a<WF>(A, s, scr);
        if (s == A.n - 3 || em_ldi(&A.ctl->status) == EM_ST_BROKEN) return;
        if (!em_barrier(A.ctl, ++nbar * W, A.spin, EM_ST_LOST)) return;
        em_phase_b<WF>(A, s, scr);
        if (!em_barrier(A.ctl, ++nbar * W, A.spin, EM_ST_LOST)) return;
    }
}

template <typename WF>
__global__ void __launch_bounds__(EM_BT) k_em_init(EmArgs A, int a, int b)
{
    __shared__ u64 scr[EM_BT / 64];
    em_init<WF>(A, a, b, scr);
}
template <typename WF>
__global__ void __launch_bounds__(EM_BT) k_em_a(EmArgs A, int s)
{
    __shared__ u64 scr[EM_BT / 64];
    if (em_ldi(&A.ctl->stop)) return;
    em_phase_a<WF>(A, s, scr);
}
template <typename WF>
__global__ void __launch_bounds__(EM_BT) k_em_b(EmArgs A, int s)
{
    __shared__ u64 scr[EM_BT / 64];
    if (em_ldi(&A.ctl->stop)) return;
    em_phase_b<WF>(A, s, scr);
}

// farthest pair: one workgroup per row i, j > i
template <typename WF>
__global__ void __launch_bounds__(EM_BT) k_em_farthest(EmArgs A, u64 *out)
{
    __shared__ u64 scr[EM_BT / 64];
    const WF c = em_wf<WF>(A);
    const int n = A.n, i = (int)blockIdx.x;
    u64 best = 0;
    for (int j = i + 1 + (int)threadIdx.x; j < n; j += blockDim.x) {
        const u64 k = (u64)c(i, j) << 35 | (EM_FMASK & ~((u64)i * (u64)n + (u64)j));
        best = k > best ? k : best;
    }
    // block maximum through the minimum of the complement (keys < 2^62: the complement's top bit is set, so negate it
    // into the signed range first)
    const u64 mn = em_block_min(EM_NONE - best, scr);
    if (threadIdx.x == 0 && mn != EM_NONE) __hip_atomic_fetch_max(out, EM_NONE - mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a caller matrix Extra Mileage can run on: every off-diagonal cell an integer in [0, 2^27)
template <typename T>
__global__ void __launch_bounds__(256) k_em_check(const T *__restrict__ m, int n, int ld, int *flag)
{
    const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n || i == j) return;
    const double x = Elem<T>::widen(m[(size_t)i * ld + j]);
    if (!(x == __builtin_trunc(x) && x >= 0.0 && x < 134217728.0)) flag[0] = 1;
}
