// ---------------------------------------------------------------------------
// Don't-look bits for the neighbour-list families, and a kick on a slot.
// Included by tspgpu.hip behind tspgpu_nl3opt.inc (uses Tours, M2Buf, M2Ctl, NlBuf, nl_sweep_unit, ornl_sweep_unit,
// nl3_sweep_unit, Nl3Pos / nl3_decode, m2_reverse_cells, or_cell / or_ecell, OrMatCost / OrPtsCost).  The rule is in
// include/tspgpu.h ("Don't-look bits") and DESIGN 4.20.  Compaction, selection and apply are the families' own kernels,
// launched unchanged: a node outside Q carries raw_b = -1 and is no candidate to any of them.
//
// A slot has three byte arrays awake[f][n] (f = 0 2-opt, 1 Or-opt, 2 3-opt; 1: the node is in A_f).  Per sweep of family f six
// launches on the slot's stream:
//   k_look_queue<f>                   one workgroup of 16 waves; wave w owns a contiguous run of 64-node steps, a lane one node
//                                     of a step (coalesced reads of awake[f] and succ).  The window test of a step is one
//                                     __ballot, kept in LDS (n <= 131 072: 2 048 masks); the waves' counts meet at ONE
//                                     barrier; then every wave writes its looked units in ascending node order to
//                                     queue[0 .. |Q|) from the masks (a lane's place is a popcount below it), raw_b = -1 for
//                                     the others, and awake[f] := 0 in place -- every window read of the workgroup lies in
//                                     front of the barrier, which is what lets the set be cleared where it lies.  The pass
//                                     is O(n) like the compaction behind it.  An empty Q: the phase ends with no sweep
//                                     counted (closing = 0) or Q := every node (closing != 0).
//   k_nl_qsweep / k_ornl_qsweep / k_nl3_qsweep (and _otf)
//                                     the families' sweep bodies with the unit from queue[g], a grid-stride loop over
//                                     g < |Q| read from the device; lane layout and DPP reductions as in the plain kernels
//                                     (a half-wave of the 2-opt sweep without a unit carries "none" through the DPP steps).
//   the family's compaction, k_m2_select
//   k_look_wake<f>                    in front of the apply, on the tour the candidates were found on: carry of every looked
//                                     unit with a candidate into awake[f], ends of every accepted move into all three sets.
//                                     Byte stores of 1; equal concurrent stores need no atomics.
//   the family's apply
// k_tour_kick applies one segment swap (kind 1 of "Neighbour-list 3-opt") with the helpers of nl3_apply_tour.
// No kernel here waits for another workgroup.
// ---------------------------------------------------------------------------
static constexpr int LOOK_WGS_PER_CU = 4;   // workgroups of a queued sweep and of k_look_wake: at most this many per compute unit

struct LookBuf {
    unsigned char *awake;   // [3][n]: the slot's sets
    int *queue;             // [n]
    LookCtl *ctl;           // (tspgpu_nlphase.h)
};

// The queue pass of one workgroup of 16 waves, in two halves around the caller's decision on an empty Q (k_look_queue here,
// k_nlb_queue in tspgpu_nlbatch_dl.inc).  look_queue_scan: the window tests of set A over FWD positions into masks[], the
// waves' counts into wcnt[16], ONE barrier; answers |Q| and, in `at`, the place of this wave's first looked unit
__device__ __forceinline__ int look_queue_scan(const unsigned char *A, const int *succ, int n, int FWD, u64 *masks, int *wcnt, int &at)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int steps = (n + 63) >> 6, per = (steps + 15) / 16, s0 = min(steps, w * per), s1 = min(steps, s0 + per);
    int c = 0;
    for (int s = s0; s < s1; s++) {         // (uniform over the wave: the ballot is reached by all its lanes)
        const int a = s * 64 + lane;
        bool in = false;
        if (a < n) {
            in = A[a] != 0;                 // the window: the nodes at P(a), .., P(a) + FWD
            for (int x = 0, u = a; x < FWD && !in; x++) { u = succ[u]; in = A[u] != 0; }
        }
        const u64 m = __ballot(in);
        if (lane == 0) masks[s] = m;
        c += __popcll(m);
    }
    if (lane == 0) wcnt[w] = c;
    __syncthreads();                        // every window read of the workgroup lies in front of this barrier
    int total = 0;
    at = 0;
    for (int i = 0; i < 16; i++) {
        const int v = wcnt[i];
        if (i < w) at += v;
        total += v;
    }
    return total;
}

// look_queue_emit: the looked units in ascending node order to queue[0 .. |Q|) (all: every node), raw_b = -1 for the others,
// A := 0, and the look block's counts
__device__ __forceinline__ void look_queue_emit(unsigned char *A, int n, const LookBuf &K, const M2Buf &B, const u64 *masks, int at, int total,
                                                bool all)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int steps = (n + 63) >> 6, per = (steps + 15) / 16, s0 = min(steps, w * per), s1 = min(steps, s0 + per);
    for (int s = s0; s < s1; s++) {
        const int a = s * 64 + lane;
        const u64 m = masks[s];
        if (a < n) {
            if (all) K.queue[a] = a;
            else if ((m >> lane) & 1) K.queue[at + __popcll(m & ((1ull << lane) - 1))] = a;
            else B.raw_b[a] = -1;
            A[a] = 0;
        }
        at += __popcll(m);
    }
    if (tid == 0) {
        const int q = all ? n : total;
        LookCtl *L = K.ctl;
        L->qlen = q;
        L->last_q = q;
        L->looked += q;
        if (q == n) L->full += 1;
        else L->max_q = max(L->max_q, q);
    }
}

template <int F, int FWD>
__global__ void __launch_bounds__(1024) k_look_queue(Tours S, int n, int t, LookBuf K, M2Buf B, M2Ctl *ctl, int closing)
{
    __shared__ u64 masks[2048];             // the window bits of 64 nodes per step: n <= 131 072 (new_instance)
    __shared__ int wcnt[16];
    if (ctl->stop) return;
    unsigned char *A = K.awake + (size_t)F * n;
    int at;
    const int total = look_queue_scan(A, S.succ + (size_t)t * n, n, FWD, masks, wcnt, at);
    if (total == 0 && !closing) {           // nothing is awake: the phase ends here as every phase does (stop, done), no sweep is counted
        if (threadIdx.x == 0) { ctl->stop = 1; ctl->m = 0; K.ctl->qlen = 0; S.done[t] = 1; }
        return;
    }
    look_queue_emit(A, n, K, B, masks, at, total, total == 0);      // (an empty Q of a closing phase: one full sweep)
}

template <typename T>
__global__ void __launch_bounds__(256) k_nl_qsweep(Tours S, const T *__restrict__ mat, int n, int ld, int t, NlBuf L, M2Buf B, const M2Ctl *ctl,
                                                   LookBuf K)
{
    if (ctl->stop) return;
    const int qlen = K.ctl->qlen;
    for (int base = (int)blockIdx.x * NL_NODES; base < qlen; base += (int)gridDim.x * NL_NODES) {     // (uniform over the workgroup)
        const int g = base + (threadIdx.x >> 5);
        nl_sweep_unit<typename Elem<T>::acc>(S, OrMatCost<T>{mat, ld}, n, t, L, B, g < qlen ? K.queue[g] : n);
    }
}

template <int KIND>
__global__ void __launch_bounds__(256) k_nl_qsweep_otf(Tours S, const typename OrPt<KIND>::type *__restrict__ pts, int n, int t, NlBuf L, M2Buf B,
                                                       const M2Ctl *ctl, LookBuf K)
{
    if (ctl->stop) return;
    const int qlen = K.ctl->qlen;
    for (int base = (int)blockIdx.x * NL_NODES; base < qlen; base += (int)gridDim.x * NL_NODES) {
        const int g = base + (threadIdx.x >> 5);
        nl_sweep_unit<int>(S, OrPtsCost<KIND>{pts}, n, t, L, B, g < qlen ? K.queue[g] : n);
    }
}

template <typename T>
__global__ void __launch_bounds__(256) k_ornl_qsweep(Tours S, const T *__restrict__ mat, int n, int ld, int t, NlBuf NL, M2Buf B, const M2Ctl *ctl,
                                                     LookBuf K)
{
    if (ctl->stop) return;
    const int qlen = K.ctl->qlen;
    for (int g = (int)blockIdx.x * ORNL_STARTS + (threadIdx.x >> 6); g < qlen; g += (int)gridDim.x * ORNL_STARTS)    // (a whole wave)
        ornl_sweep_unit<typename Elem<T>::acc>(S, OrMatCost<T>{mat, ld}, n, t, NL, B, K.queue[g]);
}

template <int KIND>
__global__ void __launch_bounds__(256) k_ornl_qsweep_otf(Tours S, const typename OrPt<KIND>::type *__restrict__ pts, int n, int t, NlBuf NL, M2Buf B,
                                                         const M2Ctl *ctl, LookBuf K)
{
    if (ctl->stop) return;
    const int qlen = K.ctl->qlen;
    for (int g = (int)blockIdx.x * ORNL_STARTS + (threadIdx.x >> 6); g < qlen; g += (int)gridDim.x * ORNL_STARTS)
        ornl_sweep_unit<int>(S, OrPtsCost<KIND>{pts}, n, t, NL, B, K.queue[g]);
}

template <typename T>
__global__ void __launch_bounds__(256) k_nl3_qsweep(Tours S, const T *__restrict__ mat, int n, int ld, int t, NlBuf NL, int W, M2Buf B,
                                                    const M2Ctl *ctl, LookBuf K)
{
    if (ctl->stop) return;
    const int qlen = K.ctl->qlen;
    for (int g = (int)blockIdx.x * NL3_NODES + (threadIdx.x >> 6); g < qlen; g += (int)gridDim.x * NL3_NODES)        // (a whole wave)
        nl3_sweep_unit<typename Elem<T>::acc>(S, OrMatCost<T>{mat, ld}, n, t, NL, W, B, K.queue[g]);
}

template <int KIND>
__global__ void __launch_bounds__(256) k_nl3_qsweep_otf(Tours S, const typename OrPt<KIND>::type *__restrict__ pts, int n, int t, NlBuf NL, int W,
                                                        M2Buf B, const M2Ctl *ctl, LookBuf K)
{
    if (ctl->stop) return;
    const int qlen = K.ctl->qlen;
    for (int g = (int)blockIdx.x * NL3_NODES + (threadIdx.x >> 6); g < qlen; g += (int)gridDim.x * NL3_NODES)
        nl3_sweep_unit<int>(S, OrPtsCost<KIND>{pts}, n, t, NL, W, B, K.queue[g]);
}

// rule 3 of "Don't-look bits", on the tour as it stands in front of the apply: the sweep of family F looked at K.ctl->qlen
// units and has m candidates (the body of k_look_wake, and of k_nlb_wake in tspgpu_nlbatch_dl.inc)
template <int F>
__device__ __forceinline__ void look_wake_tour(const Tours &S, int n, int t, const NlBuf &NL, const LookBuf &K, const M2Buf &B, int m)
{
    unsigned char *own = K.awake + (size_t)F * n, *o1 = K.awake + (size_t)((F + 1) % 3) * n, *o2 = K.awake + (size_t)((F + 2) % 3) * n;
    const int *succ = S.succ + (size_t)t * n;
    const int qlen = K.ctl->qlen;
    const int gt = (int)(blockIdx.x * blockDim.x + threadIdx.x), GT = (int)(gridDim.x * blockDim.x);
    for (int g = gt; g < qlen; g += GT) {               // carry: the looked units with a candidate
        const int v = K.queue[g], b = B.raw_b[v];
        if (b < 0 || !(B.raw_d[v] < TWO_OPT_EPS)) continue;
        own[v] = 1;
        if (F == 0) own[succ[v]] = 1;
        if (F == 1) {
            const int L = b >> ORNL_LSHIFT;
            for (int i = 1, u = v; i < L; i++) { u = succ[u]; own[u] = 1; }
        }
    }
    const Nl3Pos T = nl3_pos(S, n, t);
    for (int x = gt; x < m; x += GT) {                  // ends: the end nodes of the removed edges of every accepted move
        if (!B.acc[x]) continue;
        int e[6];
        int ne = 6;
        if (F == 0) {
            const int a = B.a[x], b = B.b[x];
            e[0] = a; e[1] = succ[a]; e[2] = b; e[3] = succ[b];
            ne = 4;
        } else if (F == 1) {
            const int s = B.a[x], pk = B.b[x], L = pk >> ORNL_LSHIFT, q = (pk >> 1) & (int)OR_QM;
            int tn = s;
            for (int i = 1; i < L; i++) tn = succ[tn];
            e[0] = T.at(T.f_of(s) - 1); e[1] = s; e[2] = tn; e[3] = succ[tn]; e[4] = q; e[5] = succ[q];
        } else {
            const Nl3Move M = nl3_decode(T, NL, B.a[x], B.b[x]);
            const int fi = wrap(T.f0 + M.i, n), fj = wrap(T.f0 + M.j, n), fk = wrap(T.f0 + M.k, n);
            e[0] = T.at(fi); e[1] = T.at(fi + 1); e[2] = T.at(fj); e[3] = T.at(fj + 1); e[4] = T.at(fk); e[5] = T.at(fk + 1);
        }
        for (int i = 0; i < ne; i++) { own[e[i]] = 1; o1[e[i]] = 1; o2[e[i]] = 1; }
    }
}

template <int F>
__global__ void __launch_bounds__(256) k_look_wake(Tours S, int n, int t, NlBuf NL, LookBuf K, M2Buf B, const M2Ctl *ctl)
{
    if (ctl->stop) return;
    look_wake_tour<F>(S, n, t, NL, K, B, ctl->m);
}

// `count` nodes join the three sets of a slot (tspgpu_tour_wake)
__global__ void __launch_bounds__(256) k_look_set(unsigned char *awake, int n, const int *__restrict__ nodes, int count)
{
    for (int x = (int)(blockIdx.x * blockDim.x + threadIdx.x); x < count; x += (int)(gridDim.x * blockDim.x)) {
        const int v = nodes[x];
        awake[v] = 1; awake[(size_t)n + v] = 1; awake[2 * (size_t)n + v] = 1;
    }
}

// The kick: kind 1 of "Neighbour-list 3-opt" at the edge positions i < j < k, whatever its delta.  One workgroup; the new order
// of i + 1 .. k is three in-place reversals as in nl3_apply_tour, then the three new edge cells and the node view of the
// range.  awake (may be null: the slot counts as all awake): the six end nodes join the three sets
template <typename T, typename CS>
__device__ __forceinline__ void kick_tour(const Tours &S, const CS cs, int n, int t, int i, int j, int k, unsigned char *awake)
{
    typedef typename Elem<T>::acc AT;
    const int tid = threadIdx.x, BT = blockDim.x;
    int *ord = S.ord + (size_t)t * n, *pos = S.pos + (size_t)t * n, *succ = S.succ + (size_t)t * n;
    AT *dp = dpos_of<AT>(S, t, n), *dnb = dnb_of<AT>(S, t, n);
    const Nl3Pos T0 = nl3_pos(S, n, t);     // node 0 sits at position 0 <= i: its cell stays
    const int dir = T0.dir, f0 = T0.f0, la = j - i, lb = k - j;
    // the six ends and the three removed costs, read by every thread before anything moves
    const int a = ord[or_cell(f0 + i, n, dir)], a1 = ord[or_cell(f0 + i + 1, n, dir)], b = ord[or_cell(f0 + j, n, dir)],
              b1 = ord[or_cell(f0 + j + 1, n, dir)], c = ord[or_cell(f0 + k, n, dir)], c1 = ord[or_cell(f0 + k + 1, n, dir)];
    const AT waa = dp[or_ecell(f0 + i, n, dir)], wbb = dp[or_ecell(f0 + j, n, dir)], wcc = dp[or_ecell(f0 + k, n, dir)];
    __syncthreads();
    m2_reverse_cells(ord, pos, dp, n, dir, f0 + i, la);
    m2_reverse_cells(ord, pos, dp, n, dir, f0 + j, lb);
    __syncthreads();
    m2_reverse_cells(ord, pos, dp, n, dir, f0 + i, la + lb);
    __syncthreads();
    if (tid < 3) {                          // the three new edges: behind a, between B and A, in front of c'
        const int e = tid == 0 ? i : tid == 2 ? k : i + lb;
        const int u = ord[or_cell(f0 + e, n, dir)], v = ord[or_cell(f0 + e + 1, n, dir)];
        dp[or_ecell(f0 + e, n, dir)] = cs(u, v);
    }
    __syncthreads();
    for (int p = i + tid; p <= k; p += BT) {
        const int v = ord[or_cell(f0 + p, n, dir)];
        succ[v] = ord[or_cell(f0 + p + 1, n, dir)];
        dnb[v] = dp[or_ecell(f0 + p, n, dir)];
    }
    if (tid == 0) {
        const AT d = ((cs(a, b1) + cs(c, a1)) + cs(b, c1)) - ((waa + wbb) + wcc);
        S.cost[t] += (double)d;
        S.last_delta[t] = (double)d;
    }
    if (awake && tid < 6) {
        const int v = tid == 0 ? a : tid == 1 ? a1 : tid == 2 ? b : tid == 3 ? b1 : tid == 4 ? c : c1;
        awake[v] = 1; awake[(size_t)n + v] = 1; awake[2 * (size_t)n + v] = 1;
    }
}

template <typename T>
__global__ void __launch_bounds__(256) k_tour_kick(Tours S, const T *__restrict__ mat, int n, int ld, int t, int i, int j, int k, unsigned char *awake)
{
    kick_tour<T>(S, OrMatCost<T>{mat, ld}, n, t, i, j, k, awake);
}

template <int KIND>
__global__ void __launch_bounds__(256) k_tour_kick_otf(Tours S, const typename OrPt<KIND>::type *__restrict__ pts, int n, int t, int i, int j, int k,
                                                       unsigned char *awake)
{
    kick_tour<int>(S, OrPtsCost<KIND>{pts}, n, t, i, j, k, awake);
}
