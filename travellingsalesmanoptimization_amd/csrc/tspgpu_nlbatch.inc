// ---------------------------------------------------------------------------
// Batched neighbour-list descent: the descent over the lists (neighbour-list 2-opt phases and neighbour-list Or-opt phases in
// turn) on every live tour of a batch per launch.
// Included by tspgpu.hip behind tspgpu_ornl.inc (uses Tours, M2Buf, NlBuf, nl_sweep_node, ornl_sweep_start, m2_compact_tour,
// ornl_compact_tour, m2_select_tour, m2_apply_tour, ornl_apply_tour).  The rule is in include/tspgpu.h ("Batched neighbour-list
// descent") and DESIGN 4.16: every tour goes through exactly the sweeps tspgpu_tour_local_search_nl runs on it.
//
// blockIdx.y indexes the device list of live slots, blockIdx.x is what the single-tour kernels use: the device bodies of
// tspgpu_nl2opt.inc, tspgpu_multi2opt.inc and tspgpu_ornl.inc run as they stand on the tour's slot, its own view of the
// candidate arrays and its own control block.  The phase is a field of that control block and advances on the device: the
// workgroup that closes a sweep which accepted nothing (workgroup 0 of the tour's apply) switches it, so no host read stands
// between two phases of a tour and the tours of a batch need not be in the same phase.
//
//   k_nlb_sweep / k_nlb_sweep_otf   ceil(n / ORNL_STARTS) workgroups per tour; in the 2-opt phase the first
//                                   ceil(n / NL_NODES) of them run nl_sweep_node, the others return.  No LDS.
//   k_nlb_compact                   one workgroup per tour: the counted scan of k_m2_compact or of k_ornl_compact.
//   k_nlb_select                    ceil(n / 256) workgroups per tour, those at or past m return at once.
//   k_nlb_apply / k_nlb_apply_otf   NLB_APPLY_WGS workgroups per tour (grid-stride over the accepted moves); workgroup 0
//                                   closes the sweep and does the phase transition.
// A tour whose descent has ended (stop) costs one early return per workgroup until the host drops it from the list.
// ---------------------------------------------------------------------------
static constexpr int NLB_APPLY_WGS = 16;    // workgroups per tour of the apply (DESIGN 4.16: a sweep accepts 14 to 33 moves at most)
static_assert(NL_NODES >= ORNL_STARTS, "the Or-opt phase sets the workgroups per tour of the batched sweep");

struct NlbCtl {             // one per slot of the range a batched descent runs on
    int phase;              // 0: neighbour-list 2-opt, 1: neighbour-list Or-opt
    int stop;               // 1: the descent of this tour has ended: later launches return at once
    int m;                  // candidates of the current sweep (k_nlb_compact)
    int last_k;             // moves the last sweep accepted
    int max_k;              // the most one sweep accepted
    int rounds;             // 2-opt phases begun
    long long phase_moves;  // moves applied since the phase began
    long long two_opt_sweeps, two_opt_moves, or_sweeps, or_moves;   // running totals (the empty sweep of every phase included)
};

// the close of a sweep of a tour of a batch: the slot's cost, last delta and sweep counter as m2_close leaves them; a sweep
// that accepted nothing ends the phase.  The next phase begins as m2_arm / k_rearm would begin it (done = 0, no sweeps, no
// cap); an Or-opt phase that applied nothing ends the descent with done = 1 and the one sweep it ran, as m2_close does
__device__ __forceinline__ void m2_close(const Tours &S, int t, NlbCtl *c, double sum, double mn, int K)
{
    S.cost[t] += sum;
    S.last_delta[t] = mn;
    S.nsweeps[t] += 1;
    c->last_k = K;
    c->max_k = max(c->max_k, K);
    c->phase_moves += K;
    if (c->phase == 0) { c->two_opt_sweeps += 1; c->two_opt_moves += K; }
    else { c->or_sweeps += 1; c->or_moves += K; }
    if (K) return;
    if (c->phase == 1 && c->phase_moves == 0) { c->stop = 1; S.done[t] = 1; return; }
    if (c->phase == 1) c->rounds += 1;      // back to 2-opt: a round begins
    c->phase ^= 1;
    c->phase_moves = 0;
    S.done[t] = 0; S.nsweeps[t] = 0; S.cap_sweeps[t] = -1;
}

// the candidate arrays of the tour at place `at` of the range: [n] each behind the range's base
__device__ __forceinline__ M2Buf nlb_view(const M2Buf &B, int at, int n)
{
    const size_t o = (size_t)at * n;
    return M2Buf{B.raw_d + o, B.raw_b + o, B.d + o, B.a + o, B.b + o, B.i + o, B.j + o, B.acc + o};
}

template <typename AT, typename CS>
__device__ __forceinline__ void nlb_sweep_tour(const Tours &S, const CS cs, int n, const int *__restrict__ list, int slot0, const NlBuf &L,
                                               const M2Buf &B0, const NlbCtl *__restrict__ ctl)
{
    const int t = list[blockIdx.y];
    const NlbCtl *c = ctl + (t - slot0);
    if (c->stop) return;
    const M2Buf B = nlb_view(B0, t - slot0, n);
    if (c->phase == 0) {                    // (block-uniform)
        if ((int)blockIdx.x * NL_NODES >= n) return;
        nl_sweep_node<AT>(S, cs, n, t, L, B);
    } else
        ornl_sweep_start<AT>(S, cs, n, t, L, B);
}

template <typename T>
__global__ void __launch_bounds__(256) k_nlb_sweep(Tours S, const T *__restrict__ mat, int n, int ld, const int *__restrict__ list, int slot0,
                                                   NlBuf L, M2Buf B0, const NlbCtl *__restrict__ ctl)
{
    nlb_sweep_tour<typename Elem<T>::acc>(S, OrMatCost<T>{mat, ld}, n, list, slot0, L, B0, ctl);
}

template <int KIND>
__global__ void __launch_bounds__(256) k_nlb_sweep_otf(Tours S, const typename OrPt<KIND>::type *__restrict__ pts, int n,
                                                       const int *__restrict__ list, int slot0, NlBuf L, M2Buf B0, const NlbCtl *__restrict__ ctl)
{
    nlb_sweep_tour<int>(S, OrPtsCost<KIND>{pts}, n, list, slot0, L, B0, ctl);
}

__global__ void __launch_bounds__(1024) k_nlb_compact(Tours S, int n, const int *__restrict__ list, int slot0, M2Buf B0, NlbCtl *ctl)
{
    __shared__ int cnts[1024];
    const int t = list[blockIdx.y];
    NlbCtl *c = ctl + (t - slot0);
    const M2Buf B = nlb_view(B0, t - slot0, n);
    if (c->phase == 0) m2_compact_tour(S, n, t, B, c, cnts);
    else ornl_compact_tour(S, n, t, B, c, cnts);
}

__global__ void __launch_bounds__(256) k_nlb_select(int n, const int *__restrict__ list, int slot0, M2Buf B0, const NlbCtl *__restrict__ ctl)
{
    const int at = list[blockIdx.y] - slot0;
    m2_select_tour(nlb_view(B0, at, n), ctl[at].m);
}

// (the phase is read by every workgroup of the tour while workgroup 0 may switch it: it does so only behind a sweep that
// accepted nothing, and then neither body writes anything)
template <typename T, typename CS>
__device__ __forceinline__ void nlb_apply_tour(const Tours &S, const CS cs, int n, const int *__restrict__ list, int slot0, const M2Buf &B0,
                                               NlbCtl *ctl)
{
    const int t = list[blockIdx.y];
    NlbCtl *c = ctl + (t - slot0);
    const M2Buf B = nlb_view(B0, t - slot0, n);
    if (c->phase == 0) m2_apply_tour<T>(S, cs, n, t, B, c);
    else ornl_apply_tour<T>(S, cs, n, t, B, c);
}

template <typename T>
__global__ void __launch_bounds__(256) k_nlb_apply(Tours S, const T *__restrict__ mat, int n, int ld, const int *__restrict__ list, int slot0,
                                                   M2Buf B0, NlbCtl *ctl)
{
    nlb_apply_tour<T>(S, OrMatCost<T>{mat, ld}, n, list, slot0, B0, ctl);
}

template <int KIND>
__global__ void __launch_bounds__(256) k_nlb_apply_otf(Tours S, const typename OrPt<KIND>::type *__restrict__ pts, int n,
                                                       const int *__restrict__ list, int slot0, M2Buf B0, NlbCtl *ctl)
{
    nlb_apply_tour<int>(S, OrPtsCost<KIND>{pts}, n, list, slot0, B0, ctl);
}
