// ---------------------------------------------------------------------------
// Or-opt: move a run of 1-3 consecutive tour nodes to another place of the tour, either way round.
// Included by tspgpu.hip (uses Tours, Partial, Elem, key_better, block_argmin, dpos_of / dnb_of).
// The reference has no Or-opt; the move is defined in include/tspgpu.h ("Or-opt") and DESIGN 4.12.
//
// A candidate (s, L, q, rev): segment s .. t (L nodes, t = L - 1 steps after s), p = pred(s), x = succ(t), q a node
// outside the segment and != p, q' = succ(q), (h, e) = (s, t) or -- rev -- (t, s):
//     delta = ((c[p][x] + c[q][h]) + c[e][q']) - ((c[p][s] + c[t][x]) + c[q][q'])
// in exactly this order for double cells.  A sweep returns the lexicographic minimum of (delta, s, L, q, rev).
//
// k_oropt_sweep: workgroup g owns the tour positions [g R, g R + R) (positions counted along the tour's direction).
// The segments that start at position k have their head / tail in the rows of the nodes at k, k + 1, k + 2, so the
// workgroup streams the rows of positions g R .. g R + R + 1 ONCE each through a ring of four LDS buffers (three in
// use, one being filled: 16-byte global loads held in registers across the evaluation, one barrier per position).
// With the symmetric matrix c[q][h] = row_h[q] is a linear LDS read and c[e][q'] = row_e[succ q] an LDS gather:
// six LDS reads serve the five candidates (L = 1; L = 2, 3 in both orientations) of one (position, q).
// c[q][q'] comes from the slot's dnb view, q' from succ, c[p][s] and c[t][x] from dnb of the tour neighbours,
// c[p][x] (three per position) from the matrix in one round of loads before the first row is evaluated.
//
// k_oropt_apply: one workgroup reduces the partials, decides delta < -1e-7 and rewrites the slot.  In the position
// array the move is a rotation: the block x .. q moves L cells towards p, or the complementary block q' .. p moves L
// cells the other way -- whichever is shorter (<= n / 2 cells) --, in chunks of one element per thread ordered so that
// no cell is overwritten before it was read; the segment (held in registers) then lands in the L cells that became
// free.  Edge costs travel with their cells; the three new edges are three reads of the cost source: the matrix
// (OrMatCost) or -- matrix-free mode, k_oropt_apply_otf -- the weight function over the points (OrPtsCost).
// ---------------------------------------------------------------------------
static constexpr int OR_RMAX = 64;          // tour positions per sweep workgroup, at most
static constexpr int OR_EXTRA = 3072;       // LDS beside the four rows: nodes, their dnb, c[p][x], the reduction scratch
static constexpr int OR_QB = 17;            // bits of a node id (n <= 131 072)
static constexpr u64 OR_QM = (1ull << OR_QB) - 1;

struct OrCtl {              // one per context for the single-tour calls, one per slot for the batch; reset before every run
    double d;               // delta of the last applied move (0: the last sweep found nothing improving)
    int move[4];            // s, L, q, rev of it (-1: none)
    int applied;            // the last apply launch applied a move
    int stop;               // 1: nothing improves, or the move budget is spent: later launches return at once
    long long moves;        // moves applied since the reset
    long long budget;       // moves still allowed (< 0: no cap)
};

__device__ __forceinline__ u64 or_key(int s, int L, int q, int rev)
{
    return (u64)s << (OR_QB + 3) | (u64)L << (OR_QB + 1) | (u64)q << 1 | (u64)rev;
}

// forward position k (any k >= -n) -> array cell, and the dpos cell of the edge between forward k and k + 1
__device__ __forceinline__ int or_cell(int k, int n, int dir)
{
    int kk = k % n;
    if (kk < 0) kk += n;
    return dir > 0 ? kk : n - 1 - kk;
}
__device__ __forceinline__ int or_ecell(int k, int n, int dir)
{
    int kk = k % n;
    if (kk < 0) kk += n;
    return dir > 0 ? kk : (kk == n - 1 ? n - 1 : n - 2 - kk);
}

template <typename T, int NCH>
__global__ void __launch_bounds__(1024) k_oropt_sweep(Tours S, const T *__restrict__ mat, int n, int ld, int t, int R, const OrCtl *ctl)
{
    typedef typename Elem<T>::acc AT;
    typedef typename Elem<T>::vec VT;
    constexpr int V = Elem<T>::V;
    extern __shared__ __attribute__((aligned(16))) unsigned char or_smem[];
    if (ctl->stop) return;
    T *rows = reinterpret_cast<T *>(or_smem);                                         // [4][ld]
    int *nodes = reinterpret_cast<int *>(or_smem + (size_t)4 * ld * sizeof(T));       // [R + 4]: positions k0 - 1 .. k0 + R + 2
    double *dn8 = reinterpret_cast<double *>(nodes + OR_RMAX + 4);
    AT *dn = reinterpret_cast<AT *>(dn8);                                             // [R + 4]: c[node][succ node]
    AT *pxc = reinterpret_cast<AT *>(dn8 + OR_RMAX + 4);                              // [R][3]: c[p][x] for L = 1, 2, 3
    Partial *scratch = reinterpret_cast<Partial *>(dn8 + OR_RMAX + 4 + 3 * OR_RMAX);  // [16]

    const int tid = threadIdx.x, BT = blockDim.x;
    const int k0 = (int)blockIdx.x * R, cnt = min(R, n - k0);
    const int dir = S.dir[t];
    const int *ord = S.ord + (size_t)t * n, *succ = S.succ + (size_t)t * n;
    const AT *dnb = dnb_of<AT>(S, t, n);
    const int nvec = ld / V;

    for (int j = tid; j < cnt + 4; j += BT) {
        const int v = ord[or_cell(k0 - 1 + j, n, dir)];
        nodes[j] = v;
        dn[j] = dnb[v];
    }
    __syncthreads();
    for (int j = tid; j < 3 * cnt; j += BT) {
        const int i = j / 3, L = j % 3 + 1;
        pxc[j] = (AT)mat[(size_t)nodes[i] * ld + nodes[i + 1 + L]];
    }
    // rows of positions k0, k0 + 1, k0 + 2 -> ring slots 0, 1, 2
    for (int r = 0; r < 3; r++) {
        const VT *src = reinterpret_cast<const VT *>(mat + (size_t)nodes[r + 1] * ld);
        VT *dst = reinterpret_cast<VT *>(rows + (size_t)r * ld);
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            const int idx = tid + c * BT;
            if (idx < nvec) dst[idx] = src[idx];
        }
    }
    __syncthreads();

    AT bd = Elem<T>::lim();
    u64 bk = KEY_NONE;
    for (int i = 0; i < cnt; i++) {
        // the row of position k0 + i + 3 starts its way in (it is evaluated from the next iteration on)
        const bool more = i + 3 <= cnt + 1;
        VT nxt[NCH];
        if (more) {
            const VT *src = reinterpret_cast<const VT *>(mat + (size_t)nodes[i + 4] * ld);
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const int idx = tid + c * BT;
                if (idx < nvec) nxt[c] = src[idx];
            }
        }
        const int p = nodes[i], s = nodes[i + 1], n1 = nodes[i + 2], n2 = nodes[i + 3];
        const T *rA = rows + (size_t)(i & 3) * ld, *rB = rows + (size_t)((i + 1) & 3) * ld, *rC = rows + (size_t)((i + 2) & 3) * ld;
        const AT cps = dn[i];
        const AT rem1 = cps + dn[i + 1], rem2 = cps + dn[i + 2], rem3 = cps + dn[i + 3];
        const AT px1 = pxc[3 * i], px2 = pxc[3 * i + 1], px3 = pxc[3 * i + 2];
        const u64 ks = (u64)s << (OR_QB + 3);
        for (int q = tid; q < n; q += BT) {
            const int qn = succ[q];
            const AT cqq = dnb[q];
            const AT aq = (AT)rA[q], bq = (AT)rB[q], cq = (AT)rC[q];
            const AT an = (AT)rA[qn], bn = (AT)rB[qn], cn = (AT)rC[qn];
            const bool ok1 = q != p && q != s, ok2 = ok1 && q != n1, ok3 = ok2 && q != n2;
            const u64 kq = ks | (u64)q << 1;
#define OR_CONSIDER(OK, HQ, EN, PX, REM, L, REV)                                                   \
            {                                                                                      \
                const AT d_ = ((PX + HQ) + EN) - (REM + cqq);                                      \
                const u64 k_ = kq | (u64)(L) << (OR_QB + 1) | (u64)(REV);                          \
                if ((OK) && (d_ < bd || (d_ == bd && k_ < bk))) { bd = d_; bk = k_; }              \
            }
            OR_CONSIDER(ok1, aq, an, px1, rem1, 1, 0)
            OR_CONSIDER(ok2, aq, bn, px2, rem2, 2, 0)
            OR_CONSIDER(ok2, bq, an, px2, rem2, 2, 1)
            OR_CONSIDER(ok3, aq, cn, px3, rem3, 3, 0)
            OR_CONSIDER(ok3, cq, an, px3, rem3, 3, 1)
#undef OR_CONSIDER
        }
        if (more) {
            VT *dst = reinterpret_cast<VT *>(rows + (size_t)((i + 3) & 3) * ld);
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const int idx = tid + c * BT;
                if (idx < nvec) dst[idx] = nxt[c];
            }
        }
        __syncthreads();
    }
    double d = bk == KEY_NONE ? DBL_MAX : (double)bd;
    block_argmin(d, bk, scratch);
    if (tid == 0) {
        Partial *part = S.partial + (size_t)t * S.pstride;
        part[blockIdx.x].d = d;
        part[blockIdx.x].key = bk;
    }
}

// where the apply takes its three new edge costs from: the resident matrix, or the points (matrix-free mode: the weights
// matrix mode would hold for the same points and kind -- edge_w / edge_w_ceil_i are the arithmetic of the build kernels)
template <typename T> struct OrMatCost {
    const T *__restrict__ mat;
    int ld;
    __device__ __forceinline__ typename Elem<T>::acc operator()(int u, int v) const { return (typename Elem<T>::acc)mat[(size_t)u * ld + v]; }
};
template <int KIND> struct OrPt { typedef double2 type; };
template <> struct OrPt<KIND_CEIL_INT> { typedef int2 type; };      // ceil_int(): the integer points of k_sweep_otf8<KIND_CEIL_INT>
template <int KIND>
__device__ __forceinline__ int or_weight(const typename OrPt<KIND>::type &u, const typename OrPt<KIND>::type &v)
{
    if constexpr (KIND == KIND_CEIL_INT) return edge_w_ceil_i(u.x, u.y, v.x, v.y);
    else return edge_w<KIND>(u.x, u.y, v.x, v.y);
}
template <int KIND> struct OrPtsCost {
    const typename OrPt<KIND>::type *__restrict__ pts;
    __device__ __forceinline__ int operator()(int u, int v) const { return or_weight<KIND>(pts[u], pts[v]); }
};

// the body of the apply kernels: one workgroup, tour slot t, G partials, that tour's control block
template <typename T, typename CS>
__device__ __forceinline__ void or_apply_tour(const Tours &S, const CS cs, int n, int t, int G, OrCtl *ctl)
{
    typedef typename Elem<T>::acc AT;
    __shared__ Partial scratch[16];
    if (ctl->stop) return;
    const int tid = threadIdx.x, BT = blockDim.x;

    double d = DBL_MAX;
    u64 key = KEY_NONE;
    const Partial *part = S.partial + (size_t)t * S.pstride;
    for (int g = tid; g < G; g += BT) {
        const Partial c = part[g];
        if (key_better(c.d, c.key, d, key)) { d = c.d; key = c.key; }
    }
    block_argmin(d, key, scratch);
    const long long budget = ctl->budget;
    __syncthreads();                        // everybody has read the control block
    if (!(key != KEY_NONE && d < TWO_OPT_EPS)) {
        if (tid == 0) {
            ctl->d = 0.0; ctl->move[0] = ctl->move[1] = ctl->move[2] = ctl->move[3] = -1;
            ctl->applied = 0; ctl->stop = 1;
            S.last_delta[t] = 0.0;
        }
        return;
    }
    const int rev = (int)(key & 1), q = (int)((key >> 1) & OR_QM), L = (int)((key >> (OR_QB + 1)) & 3), s = (int)(key >> (OR_QB + 3));
    int *ord = S.ord + (size_t)t * n, *pos = S.pos + (size_t)t * n, *succ = S.succ + (size_t)t * n;
    AT *dp = dpos_of<AT>(S, t, n), *dnb = dnb_of<AT>(S, t, n);
    const int dir = S.dir[t];
    const int a = dir > 0 ? pos[s] : n - 1 - pos[s], b = dir > 0 ? pos[q] : n - 1 - pos[q];
    // the segment and its inner edges, the four neighbours, the three new costs: all read before anything moves
    const int g0 = s, g1 = ord[or_cell(a + 1, n, dir)], g2 = ord[or_cell(a + 2, n, dir)];
    const AT w0 = dp[or_ecell(a, n, dir)], w1 = dp[or_ecell(a + 1, n, dir)];
    const int p = ord[or_cell(a - 1, n, dir)], x = ord[or_cell(a + L, n, dir)], qn = ord[or_cell(b + 1, n, dir)];
    const int tn = L == 1 ? g0 : L == 2 ? g1 : g2;
    const int h = rev ? tn : s, e = rev ? s : tn;
    const AT wpx = cs(p, x), wqh = cs(q, h), weq = cs(e, qn);
    int m1 = (b - (a + L)) % n;
    if (m1 < 0) m1 += n;
    m1 += 1;                                // cells of the block x .. q
    const int m2 = n - L - m1;              // cells of the block q' .. p
    const bool fwd = m2 < m1;               // the block q' .. p moves L cells forward, else x .. q moves L cells back
    const int B0 = fwd ? b + 1 : a + L, m = fwd ? m2 : m1, D = fwd ? L : -L;
    __syncthreads();
    for (int base = 0; base < m; base += BT) {
        const int jj = base + tid, j = fwd ? m - 1 - jj : jj;       // forward moves run from the block's far end
        const bool act = jj < m, edge = act && j < m - 1;
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
        const int f0 = fwd ? b + 1 : a + m1;                        // forward position of the segment's new first cell
        const int g[3] = {g0, g1, g2};
        const AT wi[2] = {w0, w1};
        for (int i = 0; i < L; i++) {
            const int v = rev ? g[L - 1 - i] : g[i], c = or_cell(f0 + i, n, dir);
            ord[c] = v;
            pos[v] = c;
        }
        for (int i = 0; i + 1 < L; i++) dp[or_ecell(f0 + i, n, dir)] = rev ? wi[L - 2 - i] : wi[i];
        dp[or_ecell(f0 - 1, n, dir)] = wqh;
        dp[or_ecell(f0 + L - 1, n, dir)] = weq;
        dp[or_ecell(fwd ? b + L + m2 : a - 1, n, dir)] = wpx;
        // node view
        if (rev) {
            if (L == 2) { succ[g1] = g0; dnb[g1] = w0; }
            if (L == 3) { succ[g2] = g1; dnb[g2] = w1; succ[g1] = g0; dnb[g1] = w0; }
        }
        succ[p] = x;  dnb[p] = wpx;
        succ[q] = h;  dnb[q] = wqh;
        succ[e] = qn; dnb[e] = weq;
        S.cost[t] += d;
        S.last_delta[t] = d;
        ctl->d = d; ctl->move[0] = s; ctl->move[1] = L; ctl->move[2] = q; ctl->move[3] = rev;
        ctl->applied = 1;
        ctl->moves += 1;
        if (budget >= 0) { ctl->budget = budget - 1; if (budget - 1 <= 0) ctl->stop = 1; }
    }
}

template <typename T>
__global__ void __launch_bounds__(1024) k_oropt_apply(Tours S, const T *__restrict__ mat, int n, int ld, int t, int G, OrCtl *ctl)
{
    or_apply_tour<T>(S, OrMatCost<T>{mat, ld}, n, t, G, ctl);
}

// ---------------------------------------------------------------------------
// Matrix-free mode (TSPGPU_OPT_OR_MATRIX_FREE = 1, single tours): the sibling of k_sweep_otf8.  Per move three launches:
// k_spts_gather (P_succ(q) for every q, from the tour the previous apply left), k_oropt_sweep_otf, k_oropt_apply_otf.
//
// k_oropt_sweep_otf: workgroup g owns the tour positions [g R, g R + R), R = OR_OTF_RUN.  The nodes of positions
// g R - 1 .. g R + R + 2, their points, their dnb and the three c[p][x] per position (computed here with the weight
// function) sit in LDS.  A thread streams over q, OR_OTF_VQ consecutive q per pass, with coalesced loads of P_q,
// P_succ(q) and c[q][q'] = dnb[q].  The five candidates of a (position, q) need w(q, .) and w(q', .) to the nodes at the
// position and the two behind it: a three-deep register window of (w(q, node_j), w(q', node_j)) slides along the run,
// so each weight is computed once per (q, j) and workgroup -- 2 (R + 2) weights for 5 R candidates -- and not per
// candidate.  Exclusions, key and order are those of k_oropt_sweep; deltas are int32 (three costs below 2^27 minus three).
//
// EARLY: the exact early-out.  With G(s, L) = (c[p][s] + c[t][x]) - c[p][x] a candidate improves iff
//     c[q][h] + c[e][q'] < G + c[q][q'],
// weights are >= 0 and integers, so BOTH c[q][h] <= T and c[e][q'] <= T with T = Gmax + c[q][q'] - 1 are necessary,
// Gmax the largest G of the run; h and e are nodes of the run's positions g R .. g R + R + 1.  A weight is a monotone
// function of the squared distance, so w <= T bounds the squared distance d2 (T < 0: nothing passes):
//     EUC_2D   w = (int)(c + 0.5), c = the f32 root of the f32-rounded d2:  c < T + 0.5, so d2 < (T + 0.5)^2 (1 + 2^-22)
//     CEIL_2D  w = ceil(sqrt(d2)) (f64 root, or exact over integer points):  d2 <= T^2 (1 + 2^-52)
//     ATT      w >= r = sqrt(d2 / 10) (f64):                                 d2 <= 10 T^2 (1 + 2^-51)
// The test compares, in f32, a LOWER bound of d2 -- the squared distance from the point to the bounding box of the run's
// nodes -- with that bound: the gaps lose 2^-24 each in the conversion, their squares and the fused sum 2^-22 in all, the
// f32 bound ((float)T, + 0.5, the square, the factor 10) another 2^-22; the bound carries a factor 1.000004 (2^-18).
// A pass of 64 x VQ q none of which is within the bound for q AND for q' holds no improving candidate for any position
// of the run and skips its weights.  Only candidates with delta >= 0 are left out: the argmin of an improving sweep and
// its tie order are unchanged, and a sweep without an improving candidate stops the descent in either form.
// ---------------------------------------------------------------------------
static constexpr int OR_OTF_RUN = 16;       // tour positions per workgroup (W = ceil(n / 16) <= the n / 8 + 8 partial slots of a tour)
static constexpr int OR_OTF_VQ = 4;         // consecutive q per thread and pass

// spts[q] = pts[succ q]; unlike k_gather_spts it does not look at the slot's 2-opt `done` flag (Or-opt runs on finished slots)
// but at `stop`, the flag of the control block of the descent that runs it (this one's, or the parallel-move 2-opt's)
template <typename PT>
__global__ void __launch_bounds__(256) k_spts_gather(Tours S, int n, int t, const PT *__restrict__ pts, PT *__restrict__ spts, const int *stop)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n || *stop) return;
    spts[q] = pts[S.succ[(size_t)t * n + q]];
}

template <int KIND>
__device__ __forceinline__ float or_d2_bound(int T)
{
    if (T < 0) return -1.0f;
    float tq = (float)T;
    if constexpr (KIND == TSPGPU_EUC_2D) tq += 0.5f;
    float b = tq * tq;
    if constexpr (KIND == TSPGPU_ATT) b *= 10.0f;
    return b * 1.000004f;
}

template <int KIND, bool EARLY>
__global__ void __launch_bounds__(256) k_oropt_sweep_otf(Tours S, const typename OrPt<KIND>::type *__restrict__ pts,
                                                         const typename OrPt<KIND>::type *__restrict__ spts, int n, int t, const OrCtl *ctl)
{
    typedef typename OrPt<KIND>::type PT;
    constexpr int R = OR_OTF_RUN, VQ = OR_OTF_VQ;
    __shared__ int nodes[R + 4];            // positions k0 - 1 .. k0 + R + 2
    __shared__ PT npt[R + 4];
    __shared__ int dn[R + 4];               // c[node][succ node]
    __shared__ int pxc[3 * R];              // c[p][x] for L = 1, 2, 3
    __shared__ Partial scratch[16];
    if (ctl->stop) return;
    const int tid = threadIdx.x, BT = blockDim.x;
    const int k0 = (int)blockIdx.x * R, cnt = min(R, n - k0);
    const int dir = S.dir[t];
    const int *ord = S.ord + (size_t)t * n;
    const int *dnb = dnb_of<int>(S, t, n);

    if (tid < cnt + 4) {
        const int v = ord[or_cell(k0 - 1 + tid, n, dir)];
        nodes[tid] = v;
        npt[tid] = pts[v];
        dn[tid] = dnb[v];
    }
    __syncthreads();
    if (tid < 3 * cnt) {
        const int i = tid / 3, L = tid % 3 + 1;
        pxc[tid] = or_weight<KIND>(npt[i], npt[i + 1 + L]);
    }
    __syncthreads();

    // EARLY: the largest G of the run and the box of the nodes that can be h or e (positions k0 .. k0 + cnt + 1)
    typedef typename std::conditional<KIND == KIND_CEIL_INT, int, double>::type CT;      // coordinate type
    int gmax = 0;
    CT bx0 = 0, bx1 = 0, by0 = 0, by1 = 0;
    if constexpr (EARLY) {
        gmax = INT_MIN;
        for (int i = 0; i < cnt; i++)
            for (int L = 1; L <= 3; L++) gmax = max(gmax, (dn[i] + dn[i + L]) - pxc[3 * i + L - 1]);
        bx0 = bx1 = npt[1].x; by0 = by1 = npt[1].y;
        for (int j = 2; j <= cnt + 2; j++) {
            const PT c = npt[j];
            bx0 = min(bx0, c.x); bx1 = max(bx1, c.x); by0 = min(by0, c.y); by1 = max(by1, c.y);
        }
    }
    auto box_d2 = [&](const PT &c) __attribute__((always_inline)) {      // squared distance from c to the box, rounded to f32
        float gx, gy;
        if constexpr (KIND == KIND_CEIL_INT) { gx = (float)max(max(bx0 - c.x, c.x - bx1), 0); gy = (float)max(max(by0 - c.y, c.y - by1), 0); }
        else { gx = (float)fmax(fmax(bx0 - c.x, c.x - bx1), 0.0); gy = (float)fmax(fmax(by0 - c.y, c.y - by1), 0.0); }
        return __builtin_fmaf(gy, gy, gx * gx);
    };

    int bd = INT_MAX;
    u64 bk = KEY_NONE;
    for (int base = 0; base < n; base += BT * VQ) {
        const int q0 = base + tid * VQ;
        PT pq[VQ], pn[VQ];
        int cqq[VQ];
#pragma unroll
        for (int v = 0; v < VQ; v++) {
            const int qq = min(q0 + v, n - 1);
            pq[v] = pts[qq];
            pn[v] = spts[qq];
            cqq[v] = dnb[qq];
        }
        if constexpr (EARLY) {
            bool maybe = false;
#pragma unroll
            for (int v = 0; v < VQ; v++) {
                const float b = or_d2_bound<KIND>(gmax + cqq[v] - 1);
                maybe |= (q0 + v < n) & (box_d2(pq[v]) <= b) & (box_d2(pn[v]) <= b);
            }
            if (!__ballot(maybe)) continue;
        }
        // the window: A = the node at the position, B, C = the two behind it
        int wqA[VQ], wnA[VQ], wqB[VQ], wnB[VQ];
        {
            const PT c1 = npt[1], c2 = npt[2];
#pragma unroll
            for (int v = 0; v < VQ; v++) {
                wqA[v] = or_weight<KIND>(pq[v], c1); wnA[v] = or_weight<KIND>(pn[v], c1);
                wqB[v] = or_weight<KIND>(pq[v], c2); wnB[v] = or_weight<KIND>(pn[v], c2);
            }
        }
        for (int i = 0; i < cnt; i++) {
            const PT c3 = npt[i + 3];
            const int p = nodes[i], s = nodes[i + 1], n1 = nodes[i + 2], n2 = nodes[i + 3];
            const int cps = dn[i];
            const int rem1 = cps + dn[i + 1], rem2 = cps + dn[i + 2], rem3 = cps + dn[i + 3];
            const int px1 = pxc[3 * i], px2 = pxc[3 * i + 1], px3 = pxc[3 * i + 2];
            const u64 ks = (u64)s << (OR_QB + 3);
#pragma unroll
            for (int v = 0; v < VQ; v++) {
                const int q = q0 + v;
                const int aq = wqA[v], bq = wqB[v], cq = or_weight<KIND>(pq[v], c3);
                const int an = wnA[v], bn = wnB[v], cn = or_weight<KIND>(pn[v], c3);
                const bool ok1 = q < n && q != p && q != s, ok2 = ok1 && q != n1, ok3 = ok2 && q != n2;
                const u64 kq = ks | (u64)q << 1;
#define OR_CONSIDER(OK, HQ, EN, PX, REM, L, REV)                                                   \
                {                                                                                  \
                    const int d_ = ((PX + HQ) + EN) - (REM + cqq[v]);                              \
                    const u64 k_ = kq | (u64)(L) << (OR_QB + 1) | (u64)(REV);                      \
                    if ((OK) && (d_ < bd || (d_ == bd && k_ < bk))) { bd = d_; bk = k_; }          \
                }
                OR_CONSIDER(ok1, aq, an, px1, rem1, 1, 0)
                OR_CONSIDER(ok2, aq, bn, px2, rem2, 2, 0)
                OR_CONSIDER(ok2, bq, an, px2, rem2, 2, 1)
                OR_CONSIDER(ok3, aq, cn, px3, rem3, 3, 0)
                OR_CONSIDER(ok3, cq, an, px3, rem3, 3, 1)
#undef OR_CONSIDER
                wqA[v] = bq; wqB[v] = cq; wnA[v] = bn; wnB[v] = cn;
            }
        }
    }
    double d = bk == KEY_NONE ? DBL_MAX : (double)bd;
    block_argmin(d, bk, scratch);
    if (tid == 0) {
        Partial *part = S.partial + (size_t)t * S.pstride;
        part[blockIdx.x].d = d;
        part[blockIdx.x].key = bk;
    }
}

template <int KIND>
__global__ void __launch_bounds__(1024) k_oropt_apply_otf(Tours S, const typename OrPt<KIND>::type *__restrict__ pts, int n, int t, int G, OrCtl *ctl)
{
    or_apply_tour<int>(S, OrPtsCost<KIND>{pts}, n, t, G, ctl);
}

// ---------------------------------------------------------------------------
// The batch: row y of the sweep grid (workgroup y of the apply grid) works on tour slot live[y] under that slot's own
// control block ctl[slot]; a tour whose `stop` is up costs an early return until the host drops it from the list.
// The sweep is k_oropt_sweep with one change: the q a thread visits are the same for every position of its workgroup,
// so succ[q] and dnb[q] are loaded once into registers (NCH * V of each: n <= ld <= BT * NCH * V) and not per position.
// ---------------------------------------------------------------------------
template <typename T, int NCH>
__global__ void __launch_bounds__(1024) k_oropt_sweep_batch(Tours S, const T *__restrict__ mat, int n, int ld, const int *__restrict__ live,
                                                            int R, const OrCtl *ctl)
{
    typedef typename Elem<T>::acc AT;
    typedef typename Elem<T>::vec VT;
    constexpr int V = Elem<T>::V, QN = NCH * V;
    extern __shared__ __attribute__((aligned(16))) unsigned char or_smem[];
    const int t = live[blockIdx.y];
    if (ctl[t].stop) return;
    T *rows = reinterpret_cast<T *>(or_smem);                                         // as k_oropt_sweep
    int *nodes = reinterpret_cast<int *>(or_smem + (size_t)4 * ld * sizeof(T));
    double *dn8 = reinterpret_cast<double *>(nodes + OR_RMAX + 4);
    AT *dn = reinterpret_cast<AT *>(dn8);
    AT *pxc = reinterpret_cast<AT *>(dn8 + OR_RMAX + 4);
    Partial *scratch = reinterpret_cast<Partial *>(dn8 + OR_RMAX + 4 + 3 * OR_RMAX);

    const int tid = threadIdx.x, BT = blockDim.x;
    const int k0 = (int)blockIdx.x * R, cnt = min(R, n - k0);
    const int dir = S.dir[t];
    const int *ord = S.ord + (size_t)t * n, *succ = S.succ + (size_t)t * n;
    const AT *dnb = dnb_of<AT>(S, t, n);
    const int nvec = ld / V;

    for (int j = tid; j < cnt + 4; j += BT) {
        const int v = ord[or_cell(k0 - 1 + j, n, dir)];
        nodes[j] = v;
        dn[j] = dnb[v];
    }
    int qnx[QN];
    AT cqx[QN];
#pragma unroll
    for (int j = 0; j < QN; j++) {
        const int q = tid + j * BT;
        qnx[j] = q < n ? succ[q] : 0;
        cqx[j] = q < n ? dnb[q] : (AT)0;
    }
    __syncthreads();
    for (int j = tid; j < 3 * cnt; j += BT) {
        const int i = j / 3, L = j % 3 + 1;
        pxc[j] = (AT)mat[(size_t)nodes[i] * ld + nodes[i + 1 + L]];
    }
    for (int r = 0; r < 3; r++) {
        const VT *src = reinterpret_cast<const VT *>(mat + (size_t)nodes[r + 1] * ld);
        VT *dst = reinterpret_cast<VT *>(rows + (size_t)r * ld);
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            const int idx = tid + c * BT;
            if (idx < nvec) dst[idx] = src[idx];
        }
    }
    __syncthreads();

    AT bd = Elem<T>::lim();
    u64 bk = KEY_NONE;
    for (int i = 0; i < cnt; i++) {
        const bool more = i + 3 <= cnt + 1;
        VT nxt[NCH];
        if (more) {
            const VT *src = reinterpret_cast<const VT *>(mat + (size_t)nodes[i + 4] * ld);
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const int idx = tid + c * BT;
                if (idx < nvec) nxt[c] = src[idx];
            }
        }
        const int p = nodes[i], s = nodes[i + 1], n1 = nodes[i + 2], n2 = nodes[i + 3];
        const T *rA = rows + (size_t)(i & 3) * ld, *rB = rows + (size_t)((i + 1) & 3) * ld, *rC = rows + (size_t)((i + 2) & 3) * ld;
        const AT cps = dn[i];
        const AT rem1 = cps + dn[i + 1], rem2 = cps + dn[i + 2], rem3 = cps + dn[i + 3];
        const AT px1 = pxc[3 * i], px2 = pxc[3 * i + 1], px3 = pxc[3 * i + 2];
        const u64 ks = (u64)s << (OR_QB + 3);
#pragma unroll
        for (int j = 0; j < QN; j++) {
            const int q = tid + j * BT;
            if (q < n) {
                const int qn = qnx[j];
                const AT cqq = cqx[j];
                const AT aq = (AT)rA[q], bq = (AT)rB[q], cq = (AT)rC[q];
                const AT an = (AT)rA[qn], bn = (AT)rB[qn], cn = (AT)rC[qn];
                const bool ok1 = q != p && q != s, ok2 = ok1 && q != n1, ok3 = ok2 && q != n2;
                const u64 kq = ks | (u64)q << 1;
#define OR_CONSIDER(OK, HQ, EN, PX, REM, L, REV)                                                   \
                {                                                                                  \
                    const AT d_ = ((PX + HQ) + EN) - (REM + cqq);                                  \
                    const u64 k_ = kq | (u64)(L) << (OR_QB + 1) | (u64)(REV);                      \
                    if ((OK) && (d_ < bd || (d_ == bd && k_ < bk))) { bd = d_; bk = k_; }          \
                }
                OR_CONSIDER(ok1, aq, an, px1, rem1, 1, 0)
                OR_CONSIDER(ok2, aq, bn, px2, rem2, 2, 0)
                OR_CONSIDER(ok2, bq, an, px2, rem2, 2, 1)
                OR_CONSIDER(ok3, aq, cn, px3, rem3, 3, 0)
                OR_CONSIDER(ok3, cq, an, px3, rem3, 3, 1)
#undef OR_CONSIDER
            }
        }
        if (more) {
            VT *dst = reinterpret_cast<VT *>(rows + (size_t)((i + 3) & 3) * ld);
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const int idx = tid + c * BT;
                if (idx < nvec) dst[idx] = nxt[c];
            }
        }
        __syncthreads();
    }
    double d = bk == KEY_NONE ? DBL_MAX : (double)bd;
    block_argmin(d, bk, scratch);
    if (tid == 0) {
        Partial *part = S.partial + (size_t)t * S.pstride;
        part[blockIdx.x].d = d;
        part[blockIdx.x].key = bk;
    }
}

template <typename T>
__global__ void __launch_bounds__(1024) k_oropt_apply_batch(Tours S, const T *__restrict__ mat, int n, int ld, const int *__restrict__ live,
                                                            int G, OrCtl *ctl)
{
    const int t = live[blockIdx.x];
    or_apply_tour<T>(S, OrMatCost<T>{mat, ld}, n, t, G, ctl + t);
}

// control blocks of the listed slots := "nothing applied yet, no move budget" (the start of a batch's Or-opt phase)
__global__ void k_or_arm(OrCtl *ctl, const int *__restrict__ list, int count)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    OrCtl c;
    c.d = 0.0; c.move[0] = c.move[1] = c.move[2] = c.move[3] = -1;
    c.applied = 0; c.stop = 0; c.moves = 0; c.budget = -1;
    ctl[list[i]] = c;
}
