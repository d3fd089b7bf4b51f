// ---------------------------------------------------------------------------
// Batched neighbour-list descent: the descent over the lists (neighbour-list 2-opt phases and neighbour-list Or-opt phases in
// turn, and with THREE a neighbour-list 3-opt phase behind every alternation that has run to its end) on every live tour of a
// batch per launch.
// Included by tspgpu.hip behind tspgpu_nl3opt.inc (uses Tours, M2Buf, NlBuf, nl_sweep_node, ornl_sweep_start, nl3_sweep_node,
// m2_compact_tour, ornl_compact_tour, nl3_compact_tour, m2_select_tour, m2_apply_tour, ornl_apply_tour, nl3_apply_tour).  The
// rule is in include/tspgpu.h ("Batched neighbour-list descent", "Batched neighbour-list 3-opt") and DESIGN 4.16 / 4.22: every
// tour goes through exactly the sweeps tspgpu_tour_local_search_nl (THREE: tspgpu_tour_local_search_nl3) runs on it.
//
// blockIdx.y indexes the device list of live slots, blockIdx.x is what the single-tour kernels use: the device bodies of
// tspgpu_nl2opt.inc, tspgpu_multi2opt.inc, tspgpu_ornl.inc and tspgpu_nl3opt.inc run as they stand on the tour's slot, its own
// view of the candidate arrays and its own control block.  The phase is a field of that control block and advances on the
// device (nlphase_close, tspgpu_nlphase.h): the workgroup that closes a sweep which accepted nothing (workgroup 0 of the tour's
// apply) switches it, so no host read stands between two phases of a tour and the tours of a batch need not be in the same
// phase.  THREE is a template parameter of every kernel but the selection: the two-phase instantiations hold no 3-opt code.
//
//   k_nlb_sweep / k_nlb_sweep_otf   ceil(n / ORNL_STARTS) workgroups per tour; in the 2-opt phase the first
//                                   ceil(n / NL_NODES) of them run nl_sweep_node, the others return; in the 3-opt phase all of
//                                   them run nl3_sweep_node (a wave per t1) with the width W3 of the launch.  No LDS.
//   k_nlb_compact                   one workgroup per tour: the counted scan of k_m2_compact, of k_ornl_compact or of
//                                   k_nl3_compact.
//   k_nlb_select                    ceil(n / 256) workgroups per tour, those at or past m return at once.  (A 3-opt candidate's
//                                   b is its code, whose bit 30 keeps b > a.)
//   k_nlb_apply / k_nlb_apply_otf   NLB_APPLY_WGS workgroups per tour (grid-stride over the accepted moves); workgroup 0
//                                   closes the sweep and does the phase transition.
// A tour whose descent has ended (stop) costs one early return per workgroup until the host drops it from the list.
// ---------------------------------------------------------------------------
static constexpr int NLB_APPLY_WGS = 16;    // workgroups per tour of the apply (DESIGN 4.16: a sweep accepts 14 to 33 moves at most)
static_assert(NL_NODES >= ORNL_STARTS, "the Or-opt phase sets the workgroups per tour of the batched sweep");

static_assert(NL3_NODES == ORNL_STARTS, "the 3-opt phase runs on the Or-opt phase's workgroups per tour: a wave per node");
static_assert(NL3_APPLY_BT == 256, "the batched apply runs every phase's body with 256 threads");

struct NlbCtl3 : NlbCtl {}; // the control block of a tour whose descent has the 3-opt phase: picks m2_close's overload

// the close of a sweep of a tour of a batch: the slot's cost, last delta and sweep counter as m2_close leaves them; a sweep
// that accepted nothing ends the phase (nlphase_close).  The next phase begins as m2_arm / k_rearm would begin it (done = 0, no
// sweeps, no cap); the descent ends with done = 1 and the one sweep its last phase ran, as m2_close does
template <bool THREE>
__device__ __forceinline__ void nlb_close(const Tours &S, int t, NlbCtl *c, double sum, double mn, int K)
{
    S.cost[t] += sum;
    S.last_delta[t] = mn;
    S.nsweeps[t] += 1;
    const int next = nlphase_close<THREE>(c, K);
    if (next == NLPHASE_STOP) S.done[t] = 1;
    else if (next == NLPHASE_SWITCH) { S.done[t] = 0; S.nsweeps[t] = 0; S.cap_sweeps[t] = -1; }
}

__device__ __forceinline__ void m2_close(const Tours &S, int t, NlbCtl *c, double sum, double mn, int K) { nlb_close<false>(S, t, c, sum, mn, K); }
__device__ __forceinline__ void m2_close(const Tours &S, int t, NlbCtl3 *c, double sum, double mn, int K) { nlb_close<true>(S, t, c, sum, mn, K); }

template <bool THREE> struct NlbCtlOf { typedef NlbCtl type; };
template <> struct NlbCtlOf<true> { typedef NlbCtl3 type; };

// the candidate arrays of the tour at place `at` of the range: [n] each behind the range's base
__device__ __forceinline__ M2Buf nlb_view(const M2Buf &B, int at, int n)
{
    const size_t o = (size_t)at * n;
    return M2Buf{B.raw_d + o, B.raw_b + o, B.d + o, B.a + o, B.b + o, B.i + o, B.j + o, B.acc + o};
}

template <typename AT, bool THREE, typename CS>
__device__ __forceinline__ void nlb_sweep_tour(const Tours &S, const CS cs, int n, const int *__restrict__ list, int slot0, const NlBuf &L,
                                               const M2Buf &B0, const NlbCtl *__restrict__ ctl, int W3)
{
    const int t = list[blockIdx.y];
    const NlbCtl *c = ctl + (t - slot0);
    if (c->stop) return;
    const M2Buf B = nlb_view(B0, t - slot0, n);
    const int phase = c->phase;             // (block-uniform)
    if (phase == 0) {
        if ((int)blockIdx.x * NL_NODES >= n) return;
        nl_sweep_node<AT>(S, cs, n, t, L, B);
    } else if (!THREE || phase == 1)
        ornl_sweep_start<AT>(S, cs, n, t, L, B);
    else
        nl3_sweep_node<AT>(S, cs, n, t, L, W3, B);          // (the waves past n of the last workgroup return: no barrier in it)
}

template <typename T, bool THREE>
__global__ void __launch_bounds__(256) k_nlb_sweep(Tours S, const T *__restrict__ mat, int n, int ld, const int *__restrict__ list, int slot0,
                                                   NlBuf L, M2Buf B0, const NlbCtl *__restrict__ ctl, int W3)
{
    nlb_sweep_tour<typename Elem<T>::acc, THREE>(S, OrMatCost<T>{mat, ld}, n, list, slot0, L, B0, ctl, W3);
}

template <int KIND, bool THREE>
__global__ void __launch_bounds__(256) k_nlb_sweep_otf(Tours S, const typename OrPt<KIND>::type *__restrict__ pts, int n,
                                                       const int *__restrict__ list, int slot0, NlBuf L, M2Buf B0, const NlbCtl *__restrict__ ctl,
                                                       int W3)
{
    nlb_sweep_tour<int, THREE>(S, OrPtsCost<KIND>{pts}, n, list, slot0, L, B0, ctl, W3);
}

template <bool THREE>
__global__ void __launch_bounds__(1024) k_nlb_compact(Tours S, int n, const int *__restrict__ list, int slot0, M2Buf B0, NlbCtl *ctl, NlBuf L)
{
    __shared__ int cnts[1024];
    const int t = list[blockIdx.y];
    NlbCtl *c = ctl + (t - slot0);
    const M2Buf B = nlb_view(B0, t - slot0, n);
    const int phase = c->phase;
    if (phase == 0) m2_compact_tour(S, n, t, B, c, cnts);
    else if (!THREE || phase == 1) ornl_compact_tour(S, n, t, B, c, cnts);
    else nl3_compact_tour(S, n, t, L, B, c, cnts);
}

__global__ void __launch_bounds__(256) k_nlb_select(int n, const int *__restrict__ list, int slot0, M2Buf B0, const NlbCtl *__restrict__ ctl)
{
    const int at = list[blockIdx.y] - slot0;
    m2_select_tour(nlb_view(B0, at, n), ctl[at].m);
}

// (the phase is read by every workgroup of the tour while workgroup 0 may switch it -- among two phases or three: it does so
// only behind a sweep that accepted nothing, whose m is 0, and then none of the bodies writes anything, whichever of them the
// phase a workgroup read sends it into.  m itself is written by the compaction alone)
template <typename T, bool THREE, typename CS>
__device__ __forceinline__ void nlb_apply_tour(const Tours &S, const CS cs, int n, const int *__restrict__ list, int slot0, const M2Buf &B0,
                                               NlbCtl *ctl, const NlBuf &L)
{
    const int t = list[blockIdx.y];
    typename NlbCtlOf<THREE>::type *c = static_cast<typename NlbCtlOf<THREE>::type *>(ctl + (t - slot0));
    const M2Buf B = nlb_view(B0, t - slot0, n);
    const int phase = c->phase;             // (block-uniform: one load per thread of the same cell in front of every barrier)
    if (phase == 0) m2_apply_tour<T>(S, cs, n, t, B, c);
    else if (!THREE || phase == 1) ornl_apply_tour<T>(S, cs, n, t, B, c);
    else nl3_apply_tour<T>(S, cs, n, t, L, B, c);
}

template <typename T, bool THREE>
__global__ void __launch_bounds__(256) k_nlb_apply(Tours S, const T *__restrict__ mat, int n, int ld, const int *__restrict__ list, int slot0,
                                                   M2Buf B0, NlbCtl *ctl, NlBuf L)
{
    nlb_apply_tour<T, THREE>(S, OrMatCost<T>{mat, ld}, n, list, slot0, B0, ctl, L);
}

template <int KIND, bool THREE>
__global__ void __launch_bounds__(256) k_nlb_apply_otf(Tours S, const typename OrPt<KIND>::type *__restrict__ pts, int n,
                                                       const int *__restrict__ list, int slot0, M2Buf B0, NlbCtl *ctl, NlBuf L)
{
    nlb_apply_tour<int, THREE>(S, OrPtsCost<KIND>{pts}, n, list, slot0, B0, ctl, L);
}
