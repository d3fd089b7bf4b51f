// ---------------------------------------------------------------------------
// Neighbour-list Or-opt: the candidates of a segment start come from the K-nearest-neighbour lists of the segment's ends,
// and every accepted move of a sweep is applied in one launch.
// Included by tspgpu.hip behind tspgpu_nl2opt.inc (uses Tours, Elem, wave_argmin, key_better, or_cell / or_ecell, OR_QB,
// OrMatCost / OrPtsCost, M2Buf, M2Ctl, NlBuf, m2_counted_scan, m2_sum_close, k_m2_select).  The rule is in include/tspgpu.h ("Neighbour-list Or-opt") and
// DESIGN 4.15; move and delta are those of tspgpu_oropt.inc, conflict and selection those of tspgpu_multi2opt.inc.
//
// Per sweep four launches on the slot's stream:
//   k_ornl_sweep / k_ornl_sweep_otf   one wave per segment start s (ORNL_STARTS per workgroup).  For L >= 2 the 64 lanes are
//                                     (end w: s | t) x (form A: q = u | B: q' = u) x (u = N(w)[0 .. 15]); L = 1 has one end
//                                     and uses 32 lanes.  The list holds one new edge weight, c[u][w]; the other new edge is
//                                     one gather from the cost source; c[q][q'], c[p][s], c[t][x] come from dnb, c[p][x] is
//                                     one gather per (s, L); pred(u) comes from pos, ord and dir.  A lane keeps its best over
//                                     the three L, a DPP argmin by (delta, L | q | rev) leaves raw_d[s] / raw_b[s].
//                                     A segment that holds node 0 is no candidate.  No LDS.
//   k_ornl_compact                    one workgroup: the improving candidates in node order -- m2_counted_scan, as
//                                     k_m2_compact but without a mutual-choice rule -- with a = s, b = the packed (L, q, rev)
//                                     and the range [lo, hi] of positions counted from node 0.
//   k_m2_select                       unchanged: b > a for every candidate (below), so its key (delta, min, max) is
//                                     (delta, s, L, q, rev).
//   k_ornl_apply / k_ornl_apply_otf   workgroup per accepted move (grid-stride): the block between segment and insertion
//                                     point moves L cells in chunks of one cell per thread, ordered so that no cell is
//                                     overwritten before it was read; the segment (held in registers) lands in the freed
//                                     cells.  Edge costs travel with their cells, the three new edges come from the cost
//                                     source.  Ranges are disjoint: a launch's moves touch disjoint cells, edges and nodes
//                                     (two moves may share an end node: the hi + 1 of one, which only is read, and the lo
//                                     of the other, whose position does not change).  Workgroup 0 first sums the accepted
//                                     deltas and closes the sweep as k_m2_apply does.
// ---------------------------------------------------------------------------
static constexpr int ORNL_STARTS = 4;       // segment starts per workgroup of the sweep (256 threads, a wave per start)
static constexpr int ORNL_LSHIFT = OR_QB + 1;
static constexpr int ORNL_APPLY_BT = 256;   // threads of an apply workgroup = cells per chunk of the shifted block

// a candidate travels through M2Buf as a = s, b = L << 18 | q << 1 | rev.  Labels are below 2^17 (new_instance), so b >= 2^18 > a
// for every candidate: m2_key(a, b) = a << 32 | b, and k_m2_select orders by (delta, s, L, q, rev) without a change
static_assert(OR_QB == 17 && (1 << ORNL_LSHIFT) > (1 << OR_QB) - 1 && NL_KMAX == 16, "packing of a neighbour-list Or-opt candidate");

__device__ __forceinline__ int ornl_pack(int L, int q, int rev) { return L << ORNL_LSHIFT | q << 1 | rev; }

// position of cell c counted along the tour's direction
__device__ __forceinline__ int ornl_fwd(int c, int n, int dir) { return dir > 0 ? c : n - 1 - c; }

template <typename AT, typename CS>
__device__ __forceinline__ void ornl_sweep_unit(const Tours &S, const CS cs, int n, int t, const NlBuf &NL, const M2Buf &B, int s)
{
    const int lane = threadIdx.x & 63;      // s: this wave's segment start, 0 <= s < n
    const int *ord = S.ord + (size_t)t * n, *pos = S.pos + (size_t)t * n, *succ = S.succ + (size_t)t * n;
    const AT *dnb = dnb_of<AT>(S, t, n), *lw = reinterpret_cast<const AT *>(NL.w);
    const int K = NL.K, dir = S.dir[t];
    const int j = lane & 15, form = (lane >> 4) & 1, far = lane >> 5;       // far: the end w is t, not s

    // the nodes around s: p = pred(s), the two behind s and the one behind those
    const int ks = ornl_fwd(pos[s], n, dir);
    const int p = ord[or_cell(ks - 1, n, dir)], n1 = ord[or_cell(ks + 1, n, dir)], n2 = ord[or_cell(ks + 2, n, dir)],
              n3 = ord[or_cell(ks + 3, n, dir)];
    const AT cps = dnb[p];

    // the list entry of end w: q, q' = succ(q), the weight c[u][w] and c[q][q']
    int q = -1, qn = 0;
    AT cuw = 0, cqq = 0;
    auto entry = [&](int w) {
        const int u = NL.node[(size_t)w * K + j];
        cuw = lw[(size_t)w * K + j];
        if (form == 0) { q = u; qn = succ[u]; }
        else { qn = u; q = ord[or_cell(ornl_fwd(pos[u], n, dir) - 1, n, dir)]; }
        cqq = dnb[q];
    };
    if (j < K && !far) entry(s);

    double bd = DBL_MAX;
    u64 bk = KEY_NONE;
#pragma unroll
    for (int L = 1; L <= 3; L++) {
        const int tn = L == 1 ? s : L == 2 ? n1 : n2, x = L == 1 ? n1 : L == 2 ? n2 : n3;
        if (s == 0 || tn == 0) break;           // the segment holds node 0, and so does every longer one (wave-uniform)
        if (L >= 2 && j < K && far) entry(tn);
        const bool live = j < K && (L >= 2 || !far);
        if (live) {
            const int w = far ? tn : s, o = far ? s : tn;                   // this lane's end and the other one
            const bool ok = q != p && q != s && (L < 2 || q != n1) && (L < 3 || q != n2);
            if (ok) {
                // form A: (q, h = w) is the list's edge, (e = o, q') the gather; form B: (e = w, q') the list's, (q, h = o) the gather
                const AT cqh = form == 0 ? cuw : cs(q, o), ceq = form == 0 ? cs(o, qn) : cuw;
                const AT d = ((cs(p, x) + cqh) + ceq) - ((cps + dnb[tn]) + cqq);
                const int rev = L >= 2 ? (far ^ form) : 0;
                const u64 key = (u64)ornl_pack(L, q, rev);
                if (key_better((double)d, key, bd, bk)) { bd = (double)d; bk = key; }
            }
        }
    }
    wave_argmin(bd, bk);
    if (lane == 0) {
        B.raw_d[s] = bd;
        B.raw_b[s] = bk == KEY_NONE ? -1 : (int)bk;
    }
}

// the plain sweep: workgroup g takes the starts g ORNL_STARTS .. g ORNL_STARTS + ORNL_STARTS - 1
template <typename AT, typename CS>
__device__ __forceinline__ void ornl_sweep_start(const Tours &S, const CS cs, int n, int t, const NlBuf &NL, const M2Buf &B)
{
    const int s = (int)blockIdx.x * ORNL_STARTS + (threadIdx.x >> 6);
    if (s >= n) return;                     // (a whole wave: no barrier below)
    ornl_sweep_unit<AT>(S, cs, n, t, NL, B, s);
}

template <typename T>
__global__ void __launch_bounds__(256) k_ornl_sweep(Tours S, const T *__restrict__ mat, int n, int ld, int t, NlBuf NL, M2Buf B, const M2Ctl *ctl)
{
    if (ctl->stop) return;
    ornl_sweep_start<typename Elem<T>::acc>(S, OrMatCost<T>{mat, ld}, n, t, NL, B);
}

template <int KIND>
__global__ void __launch_bounds__(256) k_ornl_sweep_otf(Tours S, const typename OrPt<KIND>::type *__restrict__ pts, int n, int t, NlBuf NL, M2Buf B,
                                                        const M2Ctl *ctl)
{
    if (ctl->stop) return;
    ornl_sweep_start<int>(S, OrPtsCost<KIND>{pts}, n, t, NL, B);
}

// the improving candidates through m2_counted_scan (cnts: [1024] in LDS), with their ranges
template <typename CTL>
__device__ __forceinline__ void ornl_compact_tour(const Tours &S, int n, int t, const M2Buf &B, CTL *ctl, int *cnts)
{
    const int *pos = S.pos + (size_t)t * n;
    const int dir = S.dir[t];
    const int f0 = ornl_fwd(pos[0], n, dir);
    m2_counted_scan(
        n, ctl, cnts, [&](int s) { return B.raw_b[s] >= 0 && B.raw_d[s] < TWO_OPT_EPS; },
        [&](int s, int at) {
            const int b = B.raw_b[s], L = b >> ORNL_LSHIFT, q = (b >> 1) & (int)OR_QM;
            int i = ornl_fwd(pos[s], n, dir) - f0, j = ornl_fwd(pos[q], n, dir) - f0;     // P(s), P(q)
            if (i < 0) i += n;
            if (j < 0) j += n;
            B.d[at] = B.raw_d[s];
            B.a[at] = s;
            B.b[at] = b;
            B.i[at] = min(i - 1, j);        // node 0 is in no segment: 1 <= i, i + L - 1 <= n - 1, no range wraps
            B.j[at] = max(i + L - 1, j);
        });
}

__global__ void __launch_bounds__(1024) k_ornl_compact(Tours S, int n, int t, M2Buf B, M2Ctl *ctl)
{
    __shared__ int cnts[1024];
    ornl_compact_tour(S, n, t, B, ctl, cnts);
}

template <typename T, typename CS, typename CTL>
__device__ __forceinline__ void ornl_apply_tour(const Tours &S, const CS cs, int n, int t, const M2Buf &B, CTL *ctl)
{
    typedef typename Elem<T>::acc AT;
    const int tid = threadIdx.x, BT = ORNL_APPLY_BT;
    const int m = ctl->m;                   // (0 once `stop` is up: k_ornl_compact)
    if (blockIdx.x == 0 && !m2_sum_close(S, t, B, ctl, m, BT)) return;      // the close of k_m2_apply
    int *ord = S.ord + (size_t)t * n, *pos = S.pos + (size_t)t * n, *succ = S.succ + (size_t)t * n;
    AT *dp = dpos_of<AT>(S, t, n), *dnb = dnb_of<AT>(S, t, n);
    const int dir = S.dir[t];
    for (int y = blockIdx.x; y < m; y += gridDim.x) {
        if (!B.acc[y]) continue;
        const int s = B.a[y], pk = B.b[y];
        const int rev = pk & 1, q = (pk >> 1) & (int)OR_QM, L = pk >> ORNL_LSHIFT;
        // forward positions of s and q: both lie in this move's range, which no other move of the launch writes
        const int a = ornl_fwd(pos[s], n, dir);
        int b = ornl_fwd(pos[q], n, dir);
        if (b < a) b += n;                  // (a - 1 and b as the positions of one stretch a - 1 .. a - 1 + n)
        // the segment and its inner edges, the four neighbours, the three new costs: all read before anything moves
        // (cells past the segment may belong to another move of this launch: they are not looked at)
        const int g0 = s, g1 = L >= 2 ? ord[or_cell(a + 1, n, dir)] : s, g2 = L == 3 ? ord[or_cell(a + 2, n, dir)] : s;
        const AT w0 = L >= 2 ? dp[or_ecell(a, n, dir)] : (AT)0, w1 = L == 3 ? dp[or_ecell(a + 1, n, dir)] : (AT)0;
        const int p = ord[or_cell(a - 1, n, dir)], x = ord[or_cell(a + L, n, dir)], qn = ord[or_cell(b + 1, n, dir)];
        const int tn = L == 1 ? g0 : L == 2 ? g1 : g2;
        const int h = rev ? tn : s, e = rev ? s : tn;
        const AT wpx = cs(p, x), wqh = cs(q, h), weq = cs(e, qn);
        // behind (P(q) > P(s)): the block x .. q moves L cells back; in front: the block q' .. p moves L cells forward.
        // Which of the two is decided by the positions counted from node 0 (the range [lo, hi] = B.i, B.j holds both)
        const int f0 = ornl_fwd(pos[0], n, dir);
        int ps = a - f0;
        if (ps < 0) ps += n;
        const bool front = B.i[y] != ps - 1;                            // lo = P(q) < P(s) - 1
        const int m1 = b - (a + L) + 1;                                 // cells of the block x .. q
        const int mb = front ? n - L - m1 : m1;                         // cells of the block that moves
        const int B0 = front ? b + 1 : a + L, D = front ? L : -L;
        __syncthreads();
        for (int base = 0; base < mb; base += BT) {
            const int jj = base + tid, j = front ? mb - 1 - jj : jj;    // forward moves run from the block's far end
            const bool act = jj < mb, edge = act && j < mb - 1;
            int v = 0;
            AT w = 0;
            if (act) v = ord[or_cell(B0 + j, n, dir)];
            if (edge) w = dp[or_ecell(B0 + j, n, dir)];
            __syncthreads();
            if (act) {
                const int c = or_cell(B0 + j + D, n, dir);
                ord[c] = v;
                pos[v] = c;
            }
            if (edge) dp[or_ecell(B0 + j + D, n, dir)] = w;
            __syncthreads();
        }
        if (tid == 0) {
            const int F0 = front ? b + 1 : a + m1;                      // forward position of the segment's new first cell
            const int g[3] = {g0, g1, g2};
            const AT wi[2] = {w0, w1};
            for (int i = 0; i < L; i++) {
                const int v = rev ? g[L - 1 - i] : g[i], c = or_cell(F0 + i, n, dir);
                ord[c] = v;
                pos[v] = c;
            }
            for (int i = 0; i + 1 < L; i++) dp[or_ecell(F0 + i, n, dir)] = rev ? wi[L - 2 - i] : wi[i];
            dp[or_ecell(F0 - 1, n, dir)] = wqh;
            dp[or_ecell(F0 + L - 1, n, dir)] = weq;
            dp[or_ecell(front ? b + L + mb : a - 1, n, dir)] = wpx;
            // node view
            if (rev) {
                if (L == 2) { succ[g1] = g0; dnb[g1] = w0; }
                if (L == 3) { succ[g2] = g1; dnb[g2] = w1; succ[g1] = g0; dnb[g1] = w0; }
            }
            succ[p] = x;  dnb[p] = wpx;
            succ[q] = h;  dnb[q] = wqh;
            succ[e] = qn; dnb[e] = weq;
        }
        __syncthreads();
    }
}

template <typename T>
__global__ void __launch_bounds__(ORNL_APPLY_BT) k_ornl_apply(Tours S, const T *__restrict__ mat, int n, int ld, int t, M2Buf B, M2Ctl *ctl)
{
    ornl_apply_tour<T>(S, OrMatCost<T>{mat, ld}, n, t, B, ctl);
}

template <int KIND>
__global__ void __launch_bounds__(ORNL_APPLY_BT) k_ornl_apply_otf(Tours S, const typename OrPt<KIND>::type *__restrict__ pts, int n, int t, M2Buf B,
                                                                  M2Ctl *ctl)
{
    ornl_apply_tour<int>(S, OrPtsCost<KIND>{pts}, n, t, B, ctl);
}
