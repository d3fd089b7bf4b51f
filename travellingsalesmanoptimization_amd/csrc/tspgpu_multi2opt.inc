// ---------------------------------------------------------------------------
// Parallel-move 2-opt: one sweep keeps a candidate per tour edge and applies every accepted candidate at once.
// Included by tspgpu.hip (uses Tours, Partial, Elem, key_better, block_argmin, dpos_of / dnb_of, or_cell / or_ecell,
// OrMatCost / OrPtsCost / or_weight).  The reference has nothing of the kind; the rule is in include/tspgpu.h
// ("Parallel-move 2-opt") and DESIGN 4.13.
//
// With sa = succ a, sb = succ b and the reference's skip test (refinment.c:55: sa == sb || a == sb || b == sa)
//     delta(a, b) = (c[a][b] + c[sa][sb]) - (c[a][sa] + c[b][sb])                      (refinment.c:60-62, this order)
// cand(a) = the first strict minimum over b ascending, a candidate if delta < -1e-7.  P(v) = the position of v counted
// from node 0 along the tour; a candidate {a, b} covers the closed range [min P, max P], two candidates conflict iff
// their ranges intersect, and a candidate is accepted iff its key (delta, lo label, hi label) is below the key of every
// candidate it conflicts with.  Accepted candidates have disjoint ranges: all of them are applied.
//
// Per sweep four launches on the slot's stream:
//   k_m2_sweep / k_m2_sweep_otf   workgroup g owns the tour positions [g R, g R + R) and leaves (delta, b) for the node
//                                 at each of them in raw_d / raw_b.  EVERY node looks at ALL b: n^2 evaluations, twice
//                                 the reference's half sweep -- the price of a rule that depends neither on the array
//                                 rotation nor on dir.
//                                 Matrix mode: c[a][b] is a coalesced read of row a that is used once (no LDS); the row
//                                 of sa sits in LDS for the gather c[sa][succ b], and the row of the next position is
//                                 on its way in registers while this one is evaluated (one LDS row: every instance
//                                 whose row fits LDS -- the matrix 2-opt's own limit -- is taken).
//                                 Matrix-free mode: a thread streams over b with coalesced loads of P_b, P_succ(b) and
//                                 c[b][succ b], and evaluates the run's R positions from LDS-resident points.
//   k_m2_compact                  one workgroup: the improving candidates, once per pair (of two nodes that chose each
//                                 other the smaller label stays), in node order -- a counted scan, so the list and all
//                                 that follows is the same in every run -- with their ranges from pos, dir and pos[0].
//   k_m2_select                   candidate x against all m candidates, tiles of 256 through LDS: m^2 range tests.
//   k_m2_apply                    workgroup per accepted move (grid-stride): the node view of the reversed nodes from
//                                 the old arrays, then the cells and the inner edge costs swapped in place, then the
//                                 two new edges.  Ranges are reversed as given: with several moves in one launch the
//                                 shorter-arc trick of k_apply (flip the complement, toggle dir) is not available.
//                                 Workgroup 0 first sums the accepted deltas (a tree of fixed shape) and closes the
//                                 sweep: cost, last_delta, nsweeps, done, the control block.
// ---------------------------------------------------------------------------
static constexpr int M2_RMAX = 60;          // tour positions per sweep workgroup, at most (matrix mode)
static constexpr int M2_RMIN = 4;
static constexpr int M2_EXTRA = 1024;       // LDS beside the row: nodes, their dnb, the reduction scratch (make_plan's own slack)
static_assert((M2_RMAX + 2) * 4 % 8 == 0 && (M2_RMAX + 2) * 4 + M2_RMAX * 8 + 16 * sizeof(Partial) <= M2_EXTRA, "k_m2_sweep's LDS layout");
static constexpr int M2_OTF_RUN = 16;       // tour positions per workgroup in matrix-free mode
static constexpr int M2_APPLY_WGS = 256;

struct M2Ctl {              // one per context; reset before every run
    int stop;               // 1: the last sweep accepted nothing, or the sweep budget is spent: later launches return at once
    int m;                  // candidates of the current sweep (k_m2_compact)
    int last_k;             // moves the last sweep accepted
    int max_k;              // the most one sweep accepted since the reset
    long long sweeps;       // sweeps since the reset (the last, empty one included)
    long long moves;        // moves applied since the reset
    long long budget;       // sweeps still allowed (< 0: no cap)
};

struct M2Buf {              // scratch of the slot a descent runs on, [n] each (allocated on first use)
    double *raw_d; int *raw_b;      // by node a: delta and b of cand(a) (b = -1: none)
    double *d; int *a, *b, *i, *j;  // the m compacted candidates: delta, the nodes at P = i < j
    int *acc;                       // 1: accepted
};

__device__ __forceinline__ u64 m2_key(int a, int b) { return (u64)min(a, b) << 32 | (u64)max(a, b); }

template <typename T, int NCH>
__global__ void __launch_bounds__(1024) k_m2_sweep(Tours S, const T *__restrict__ mat, int n, int ld, int t, int R, M2Buf B, const M2Ctl *ctl)
{
    typedef typename Elem<T>::acc AT;
    typedef typename Elem<T>::vec VT;
    constexpr int V = Elem<T>::V;
    extern __shared__ __attribute__((aligned(16))) unsigned char m2_smem[];
    if (ctl->stop) return;
    T *row = reinterpret_cast<T *>(m2_smem);                                          // [ld]: the row of succ(a)
    int *nodes = reinterpret_cast<int *>(m2_smem + (size_t)ld * sizeof(T));           // [R + 1]: positions k0 .. k0 + R
    double *dn8 = reinterpret_cast<double *>(nodes + M2_RMAX + 2);
    AT *dn = reinterpret_cast<AT *>(dn8);                                             // [R]: c[node][succ node]
    Partial *scratch = reinterpret_cast<Partial *>(dn8 + M2_RMAX);                    // [16]

    const int tid = threadIdx.x, BT = blockDim.x;
    const int k0 = (int)blockIdx.x * R, cnt = min(R, n - k0);
    const int dir = S.dir[t];
    const int *ord = S.ord + (size_t)t * n, *succ = S.succ + (size_t)t * n;
    const AT *dnb = dnb_of<AT>(S, t, n);
    const int nvec = ld / V;

    for (int j = tid; j < cnt + 1; j += BT) {
        const int v = ord[or_cell(k0 + j, n, dir)];
        nodes[j] = v;
        if (j < cnt) dn[j] = dnb[v];
    }
    __syncthreads();
    {
        const VT *src = reinterpret_cast<const VT *>(mat + (size_t)nodes[1] * ld);
        VT *dst = reinterpret_cast<VT *>(row);
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            const int idx = tid + c * BT;
            if (idx < nvec) dst[idx] = src[idx];
        }
    }
    __syncthreads();

    for (int i = 0; i < cnt; i++) {
        const bool more = i + 1 < cnt;      // the row of position k0 + i + 2 starts its way in
        VT nxt[NCH];
        if (more) {
            const VT *src = reinterpret_cast<const VT *>(mat + (size_t)nodes[i + 2] * ld);
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const int idx = tid + c * BT;
                if (idx < nvec) nxt[c] = src[idx];
            }
        }
        const int a = nodes[i], sa = nodes[i + 1];
        const T *ra = mat + (size_t)a * ld;
        const AT casa = dn[i];
        AT bd = Elem<T>::lim();
        int bb = -1;
        for (int b = tid; b < n; b += BT) {         // ascending per thread: the strict < keeps the first minimum
            const int sb = succ[b];
            const AT d = ((AT)ra[b] + (AT)row[sb]) - (casa + dnb[b]);
            const bool ok = !(b == a || a == sb || b == sa);
            if (ok && d < bd) { bd = d; bb = b; }
        }
        double dd = bb < 0 ? DBL_MAX : (double)bd;
        u64 key = bb < 0 ? KEY_NONE : (u64)bb;
        block_argmin(dd, key, scratch);             // (its barriers also end every read of `row`)
        if (tid == 0) {
            B.raw_d[a] = dd;
            B.raw_b[a] = key == KEY_NONE ? -1 : (int)key;
        }
        if (more) {
            VT *dst = reinterpret_cast<VT *>(row);
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const int idx = tid + c * BT;
                if (idx < nvec) dst[idx] = nxt[c];
            }
        }
        __syncthreads();
    }
}

template <int KIND>
__global__ void __launch_bounds__(256) k_m2_sweep_otf(Tours S, const typename OrPt<KIND>::type *__restrict__ pts,
                                                      const typename OrPt<KIND>::type *__restrict__ spts, int n, int t, M2Buf B, const M2Ctl *ctl)
{
    typedef typename OrPt<KIND>::type PT;
    constexpr int R = M2_OTF_RUN;
    __shared__ int nodes[R + 1];            // positions k0 .. k0 + R
    __shared__ PT npt[R + 1];
    __shared__ int dn[R];                   // c[node][succ node]
    __shared__ Partial scratch[16];
    if (ctl->stop) return;
    const int tid = threadIdx.x, BT = blockDim.x;
    const int k0 = (int)blockIdx.x * R, cnt = min(R, n - k0);
    const int dir = S.dir[t];
    const int *ord = S.ord + (size_t)t * n, *succ = S.succ + (size_t)t * n;
    const int *dnb = dnb_of<int>(S, t, n);

    if (tid < cnt + 1) {
        const int v = ord[or_cell(k0 + tid, n, dir)];
        nodes[tid] = v;
        npt[tid] = pts[v];
        if (tid < cnt) dn[tid] = dnb[v];
    }
    __syncthreads();

    int bd[R], bb[R];
#pragma unroll
    for (int i = 0; i < R; i++) { bd[i] = INT_MAX; bb[i] = -1; }
    for (int b = tid; b < n; b += BT) {             // ascending per thread: the strict < keeps the first minimum
        const PT pb = pts[b], ps = spts[b];
        const int sb = succ[b], cbb = dnb[b];
#pragma unroll
        for (int i = 0; i < R; i++) {
            if (i < cnt) {
                const int a = nodes[i], sa = nodes[i + 1];
                const int d = (or_weight<KIND>(npt[i], pb) + or_weight<KIND>(npt[i + 1], ps)) - (dn[i] + cbb);
                const bool ok = !(b == a || a == sb || b == sa);
                if (ok && d < bd[i]) { bd[i] = d; bb[i] = b; }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < R; i++) {
        if (i < cnt) {
            double dd = bb[i] < 0 ? DBL_MAX : (double)bd[i];
            u64 key = bb[i] < 0 ? KEY_NONE : (u64)bb[i];
            block_argmin(dd, key, scratch);
            if (tid == 0) {
                B.raw_d[nodes[i]] = dd;
                B.raw_b[nodes[i]] = key == KEY_NONE ? -1 : (int)key;
            }
        }
    }
}

// The counted scan of every family's compaction.  One workgroup of 1024 threads; thread k owns the nodes [k C, k C + C), counts
// those that are valid(node), and after an inclusive scan over cnts ([1024] in LDS) calls emit(node, at) for each of them with
// its place in the list: node order, the same in every run.  valid runs twice per node.  ctl->m := the length of the list, 0
// once `stop` is up.  For the control block of a single descent or of a tour of a batch (tspgpu_nlbatch.inc)
template <typename CTL, typename Valid, typename Emit>
__device__ __forceinline__ void m2_counted_scan(int n, CTL *ctl, int *cnts, Valid valid, Emit emit)
{
    const int tid = threadIdx.x;
    if (ctl->stop) {
        if (tid == 0) ctl->m = 0;
        return;
    }
    const int C = (n + 1023) / 1024, a0 = min(n, tid * C), a1 = min(n, a0 + C);
    int c = 0;
    for (int a = a0; a < a1; a++) c += valid(a) ? 1 : 0;
    cnts[tid] = c;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = tid >= off ? cnts[tid - off] : 0;
        __syncthreads();
        cnts[tid] += v;
        __syncthreads();
    }
    int at = cnts[tid] - c;
    for (int a = a0; a < a1; a++)
        if (valid(a)) emit(a, at++);
    if (tid == 1023) ctl->m = cnts[1023];
}

// the improving candidates, once per pair, with their ranges from pos, dir and pos[0].  (dir and pos[0] are read in front of
// the scan's `stop` test, here and in the other two callers: a few loads of valid slot memory that a stopped tour does not need)
template <typename CTL>
__device__ __forceinline__ void m2_compact_tour(const Tours &S, int n, int t, const M2Buf &B, CTL *ctl, int *cnts)
{
    const int *pos = S.pos + (size_t)t * n;
    const int dir = S.dir[t];
    const int f0 = dir > 0 ? pos[0] : n - 1 - pos[0];
    m2_counted_scan(
        n, ctl, cnts,
        [&](int a) {
            const int b = B.raw_b[a];
            return b >= 0 && B.raw_d[a] < TWO_OPT_EPS && !(B.raw_b[b] == a && b < a);   // mutual choice: the same pair, the same delta
        },
        [&](int a, int at) {
            const int b = B.raw_b[a];
            int pa = (dir > 0 ? pos[a] : n - 1 - pos[a]) - f0, pb = (dir > 0 ? pos[b] : n - 1 - pos[b]) - f0;
            if (pa < 0) pa += n;
            if (pb < 0) pb += n;
            const bool ab = pa < pb;
            B.d[at] = B.raw_d[a];
            B.a[at] = ab ? a : b;
            B.b[at] = ab ? b : a;
            B.i[at] = ab ? pa : pb;
            B.j[at] = ab ? pb : pa;
        });
}

__global__ void __launch_bounds__(1024) k_m2_compact(Tours S, int n, int t, M2Buf B, M2Ctl *ctl)
{
    __shared__ int cnts[1024];
    m2_compact_tour(S, n, t, B, ctl, cnts);
}

// candidate x of the m against all of them (the body of k_m2_select; blocks at or past m return at once)
__device__ __forceinline__ void m2_select_tour(const M2Buf &B, int m)
{
    __shared__ double sd[256];
    __shared__ u64 sk[256];
    __shared__ int si[256], sj[256];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x * 256 >= m) return;
    const int x = blockIdx.x * 256 + tid;
    const bool live = x < m;
    const double dx = live ? B.d[x] : 0.0;
    const u64 kx = live ? m2_key(B.a[x], B.b[x]) : 0;
    const int ix = live ? B.i[x] : 1, jx = live ? B.j[x] : 0;
    bool beaten = false;
    for (int base = 0; base < m; base += 256) {
        const int y = base + tid;
        if (y < m) { sd[tid] = B.d[y]; sk[tid] = m2_key(B.a[y], B.b[y]); si[tid] = B.i[y]; sj[tid] = B.j[y]; }
        else { sd[tid] = 0.0; sk[tid] = KEY_NONE; si[tid] = INT_MAX; sj[tid] = -1; }    // an empty range meets nothing
        __syncthreads();
        for (int u = 0; u < 256; u++)
            beaten |= si[u] <= jx && ix <= sj[u] && key_better(sd[u], sk[u], dx, kx);
        __syncthreads();
    }
    if (live) B.acc[x] = beaten ? 0 : 1;
}

__global__ void __launch_bounds__(256) k_m2_select(M2Buf B, const M2Ctl *ctl)
{
    m2_select_tour(B, ctl->m);
}

// the close of a sweep (one thread): the slot's cost, last delta and sweep counter, the control block; a sweep that accepted
// nothing, or the last one of the budget, ends the run.  tspgpu_nlbatch.inc has the form for a tour of a batch
__device__ __forceinline__ void m2_close(const Tours &S, int t, M2Ctl *ctl, double sum, double mn, int K)
{
    const long long budget = ctl->budget;
    S.cost[t] += sum;
    S.last_delta[t] = mn;
    S.nsweeps[t] += 1;
    ctl->last_k = K;
    ctl->max_k = max(ctl->max_k, K);
    ctl->sweeps += 1;
    ctl->moves += K;
    bool stop = K == 0;
    if (budget >= 0) { ctl->budget = budget - 1; stop |= budget - 1 <= 0; }
    if (stop) { ctl->stop = 1; S.done[t] = 1; }
}

// the cells at the forward positions F + 1 .. F + M and the M - 1 edge costs between them, swapped end for end in place by
// the threads of one workgroup (tspgpu_nl3opt.inc composes its moves of these; the caller's barriers stand around it)
template <typename AT>
__device__ __forceinline__ void m2_reverse_cells(int *ord, int *pos, AT *dp, int n, int dir, int F, int M)
{
    const int tid = threadIdx.x, BT = blockDim.x;
    for (int k = tid; k < M / 2; k += BT) {
        const int pk = or_cell(F + 1 + k, n, dir), qk = or_cell(F + M - k, n, dir);
        const int u = ord[pk], v = ord[qk];
        ord[pk] = v; ord[qk] = u;
        pos[v] = pk; pos[u] = qk;
    }
    for (int k = tid; k < (M - 1) / 2; k += BT) {           // the M - 1 inner edges F + 1 .. F + M - 1
        const int pe = or_ecell(F + 1 + k, n, dir), qe = or_ecell(F + M - 1 - k, n, dir);
        const AT eu = dp[pe], ev = dp[qe];
        dp[pe] = ev; dp[qe] = eu;
    }
}

// Workgroup 0's part of every family's apply launch, by BT <= 256 threads: sum, minimum and count of the m candidates' accepted
// deltas -- strided per thread, then a halving tree of fixed shape, so the double sum is the same in every run -- and the
// close of the sweep.  false: `stop` is up, the launch has nothing to do
template <typename CTL>
__device__ __forceinline__ bool m2_sum_close(const Tours &S, int t, const M2Buf &B, CTL *ctl, int m, int BT)
{
    __shared__ double rs[256], rm[256];
    __shared__ int rk[256];
    const int tid = threadIdx.x;
    if (ctl->stop) return false;
    double s = 0.0, mn = 0.0;
    int k = 0;
    for (int x = tid; x < m; x += BT)
        if (B.acc[x]) { const double d = B.d[x]; s += d; mn = fmin(mn, d); k++; }
    rs[tid] = s; rm[tid] = mn; rk[tid] = k;
    __syncthreads();
    for (int off = BT >> 1; off > 0; off >>= 1) {
        if (tid < off) { rs[tid] += rs[tid + off]; rm[tid] = fmin(rm[tid], rm[tid + off]); rk[tid] += rk[tid + off]; }
        __syncthreads();
    }
    if (tid == 0) m2_close(S, t, ctl, rs[0], rm[0], rk[0]);
    return true;
}

template <typename T, typename CS, typename CTL>
__device__ __forceinline__ void m2_apply_tour(const Tours &S, const CS cs, int n, int t, const M2Buf &B, CTL *ctl)
{
    typedef typename Elem<T>::acc AT;
    const int tid = threadIdx.x, BT = blockDim.x;
    const int m = ctl->m;                   // (0 once `stop` is up: k_m2_compact)
    if (blockIdx.x == 0 && !m2_sum_close(S, t, B, ctl, m, BT)) return;
    int *ord = S.ord + (size_t)t * n, *pos = S.pos + (size_t)t * n, *succ = S.succ + (size_t)t * n;
    AT *dp = dpos_of<AT>(S, t, n), *dnb = dnb_of<AT>(S, t, n);
    const int dir = S.dir[t];
    const int f0 = dir > 0 ? pos[0] : n - 1 - pos[0];       // node 0 is in no reversed range: its cell stays
    for (int x = blockIdx.x; x < m; x += gridDim.x) {
        if (!B.acc[x]) continue;
        const int a = B.a[x], b = B.b[x], F = f0 + B.i[x], M = B.j[x] - B.i[x];      // reversed: forward positions F + 1 .. F + M
        const int sa = ord[or_cell(F + 1, n, dir)], sb = ord[or_cell(F + M + 1, n, dir)];
        // node view of the nodes at F + 2 .. F + M, from the old arrays: they point at their old predecessors over the same edges
        for (int k = 2 + tid; k <= M; k += BT) {
            const int v = ord[or_cell(F + k, n, dir)], p = ord[or_cell(F + k - 1, n, dir)];
            const AT w = dp[or_ecell(F + k - 1, n, dir)];
            succ[v] = p;
            dnb[v] = w;
        }
        __syncthreads();                    // every read of the old ord / dpos of this range is complete
        m2_reverse_cells(ord, pos, dp, n, dir, F, M);
        if (tid == 0) {
            const AT wab = cs(a, b), wss = cs(sa, sb);
            dp[or_ecell(F, n, dir)] = wab;
            dp[or_ecell(F + M, n, dir)] = wss;
            succ[a] = b;   dnb[a] = wab;
            succ[sa] = sb; dnb[sa] = wss;
        }
        __syncthreads();
    }
}

template <typename T>
__global__ void __launch_bounds__(256) k_m2_apply(Tours S, const T *__restrict__ mat, int n, int ld, int t, M2Buf B, M2Ctl *ctl)
{
    m2_apply_tour<T>(S, OrMatCost<T>{mat, ld}, n, t, B, ctl);
}

template <int KIND>
__global__ void __launch_bounds__(256) k_m2_apply_otf(Tours S, const typename OrPt<KIND>::type *__restrict__ pts, int n, int t, M2Buf B, M2Ctl *ctl)
{
    m2_apply_tour<int>(S, OrPtsCost<KIND>{pts}, n, t, B, ctl);
}
