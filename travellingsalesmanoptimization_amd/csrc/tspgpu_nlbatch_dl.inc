// ---------------------------------------------------------------------------
// Don't-look bits for the batched neighbour-list descent: rule 8 of "Don't-look bits" on every live tour of a batch per launch.
// Included by tspgpu.hip behind tspgpu_nlbatch.inc (uses NlbCtl, nlb_view, NlbCtlOf's pattern and the kernels k_nlb_compact and
// k_nlb_select, which are launched as they stand; of tspgpu_looks_dl.inc LookBuf, look_queue_scan, look_queue_emit and
// look_wake_tour; the unit functions nl_sweep_unit, ornl_sweep_unit, nl3_sweep_unit and the three *_apply_tour).  The rule is
// in include/tspgpu.h ("Batched don't-look bits") and DESIGN 4.23: every tour goes through exactly the sweeps
// tspgpu_tour_local_search_nl3_dl runs on it.
//
// Per sweep round six launches for the whole batch; blockIdx.y (.x for the one-workgroup kernels) indexes the device list of
// live slots.  A tour has its own queue [n] and its own look block (LookCtl) by its place in the range, and its three sets
// where tspgpu_tour_awake reads them.
//   k_nlb_queue<THREE>              one workgroup of 16 waves per tour: the queue pass of the set of the tour's phase (window
//                                   0, 2, 0 positions).  An empty set of a phase that does not close ends the phase with no
//                                   sweep counted (nlphase_empty) and the workgroup goes on to the next phase's set, until a
//                                   set is not empty or the descent ends: a tour with nothing awake costs one launch.  Every
//                                   thread advances its own copy of the phase cells alike, so every loop trip and every
//                                   return is uniform over the workgroup; thread 0 writes them back behind the last barrier.
//                                   One barrier per trip: the waves' counts lie in two halves of LDS by the trip's parity.
//   k_nlb_qsweep / _otf             NLB_QSWEEP_WGS workgroups per tour, grid-stride over g < |Q|: the unit functions of the
//                                   tour's phase on queue[g], lane layouts as k_nl_qsweep / k_ornl_qsweep / k_nl3_qsweep.
//   k_nlb_compact, k_nlb_select     unchanged (a node outside Q carries raw_b = -1)
//   k_nlb_wake<THREE>               NLB_WAKE_WGS workgroups per tour: look_wake_tour of the tour's phase, in front of the apply
//   k_nlb_apply_dl / _otf           k_nlb_apply with the close of nlphase_close(NlbDlCtl): a sweep of a closing phase that
//                                   accepted nothing and was not full leaves "wake all" in the tour's look block instead of
//                                   ending the phase; its single writer is workgroup 0 of the apply, behind m = 0.
// No kernel here waits for another workgroup.
// ---------------------------------------------------------------------------
static constexpr int NLB_QSWEEP_WGS = 16;   // workgroups per tour of the queued sweep (DESIGN 4.23: |Q| behind a kick and in late sweeps)
static constexpr int NLB_WAKE_WGS = 4;      // ... of the wake pass: 1 024 threads, one pass over the queues the sets leave behind a kick

struct NlbDlCtl3 : NlbDlCtl {};             // as NlbCtl3: the descent has the 3-opt phase

template <bool THREE> struct NlbDlCtlOf { typedef NlbDlCtl type; };
template <> struct NlbDlCtlOf<true> { typedef NlbDlCtl3 type; };

struct NlbLooks {           // the look state of a range: the slots' sets, and a queue and a look block per place in the range
    unsigned char *awake;   // [slot][3][n]
    int *queue;             // [place][n]
    LookCtl *look;          // [place]
    int closing;
};

__device__ __forceinline__ LookBuf nlb_look(const NlbLooks &Q, int t, int at, int n)
{
    return LookBuf{Q.awake + (size_t)t * 3 * n, Q.queue + (size_t)at * n, Q.look + at};
}

// the close of nlb_close with the phase decision of a tour with looks
template <bool THREE>
__device__ __forceinline__ void nlb_dl_close(const Tours &S, int t, NlbDlCtl *r, double sum, double mn, int K)
{
    S.cost[t] += sum;
    S.last_delta[t] = mn;
    S.nsweeps[t] += 1;
    const int next = nlphase_close<THREE>(r, K);
    if (next == NLPHASE_STOP) S.done[t] = 1;
    else if (next == NLPHASE_SWITCH) { S.done[t] = 0; S.nsweeps[t] = 0; S.cap_sweeps[t] = -1; }
}

__device__ __forceinline__ void m2_close(const Tours &S, int t, NlbDlCtl *r, double sum, double mn, int K) { nlb_dl_close<false>(S, t, r, sum, mn, K); }
__device__ __forceinline__ void m2_close(const Tours &S, int t, NlbDlCtl3 *r, double sum, double mn, int K) { nlb_dl_close<true>(S, t, r, sum, mn, K); }

template <bool THREE>
__global__ void __launch_bounds__(1024) k_nlb_queue(Tours S, int n, const int *__restrict__ list, int slot0, M2Buf B0, NlbCtl *ctl, NlbLooks Q)
{
    __shared__ u64 masks[2048];             // as k_look_queue: n <= 131 072
    __shared__ int wcnt[2][16];
    const int t = list[blockIdx.x], place = t - slot0;
    NlbCtl *c = ctl + place;
    if (c->stop) return;                    // (block-uniform: thread 0 writes it behind the last barrier)
    const LookBuf K = nlb_look(Q, t, place, n);
    const M2Buf B = nlb_view(B0, place, n);
    const int *succ = S.succ + (size_t)t * n;
    const bool wake_all = Q.closing && K.ctl->wake_all;     // (cleared behind the barrier)
    NlbCtl lc;                              // the cells nlphase_empty reads and writes: every thread's own copy
    lc.phase = c->phase; lc.stop = 0; lc.rounds = c->rounds; lc.three_phases = c->three_phases; lc.phase_moves = c->phase_moves;
    for (int trip = 0;; trip++) {
        const int f = lc.phase;
        unsigned char *A = K.awake + (size_t)f * n;
        int at;
        const int total = look_queue_scan(A, succ, n, f == 1 ? 2 : 0, masks, wcnt[trip & 1], at);
        if (total == 0 && !Q.closing) {     // nothing of this phase's set is awake: the phase ends, no sweep is counted
            if (nlphase_empty<THREE>(&lc) != NLPHASE_STOP) continue;
            if (threadIdx.x == 0) {
                c->phase = lc.phase; c->rounds = lc.rounds; c->three_phases = lc.three_phases; c->phase_moves = lc.phase_moves;
                c->stop = 1; c->m = 0;
                K.ctl->qlen = 0;
                S.done[t] = 1; S.nsweeps[t] = 0; S.cap_sweeps[t] = -1;
            }
            return;
        }
        look_queue_emit(A, n, K, B, masks, at, total, total == 0 || wake_all);
        if (threadIdx.x == 0) {
            if (trip) {                     // the phases in between began and ended here, as m2_arm begins one
                c->phase = lc.phase; c->rounds = lc.rounds; c->three_phases = lc.three_phases; c->phase_moves = lc.phase_moves;
                S.done[t] = 0; S.nsweeps[t] = 0; S.cap_sweeps[t] = -1;
            }
            if (wake_all) K.ctl->wake_all = 0;
        }
        return;
    }
}

template <typename AT, bool THREE, typename CS>
__device__ __forceinline__ void nlb_qsweep_tour(const Tours &S, const CS cs, int n, const int *__restrict__ list, int slot0, const NlBuf &L,
                                                const M2Buf &B0, const NlbCtl *__restrict__ ctl, int W3, const NlbLooks &Q)
{
    const int t = list[blockIdx.y], place = t - slot0;
    const NlbCtl *c = ctl + place;
    if (c->stop) return;
    const M2Buf B = nlb_view(B0, place, n);
    const int *queue = Q.queue + (size_t)place * n;
    const int qlen = Q.look[place].qlen, phase = c->phase;  // (block-uniform)
    if (phase == 0) {
        for (int base = (int)blockIdx.x * NL_NODES; base < qlen; base += (int)gridDim.x * NL_NODES) {   // (uniform over the workgroup)
            const int g = base + (threadIdx.x >> 5);
            nl_sweep_unit<AT>(S, cs, n, t, L, B, g < qlen ? queue[g] : n);
        }
    } else if (!THREE || phase == 1) {
        for (int g = (int)blockIdx.x * ORNL_STARTS + (threadIdx.x >> 6); g < qlen; g += (int)gridDim.x * ORNL_STARTS)  // (a whole wave)
            ornl_sweep_unit<AT>(S, cs, n, t, L, B, queue[g]);
    } else {
        for (int g = (int)blockIdx.x * NL3_NODES + (threadIdx.x >> 6); g < qlen; g += (int)gridDim.x * NL3_NODES)
            nl3_sweep_unit<AT>(S, cs, n, t, L, W3, B, queue[g]);
    }
}

template <typename T, bool THREE>
__global__ void __launch_bounds__(256) k_nlb_qsweep(Tours S, const T *__restrict__ mat, int n, int ld, const int *__restrict__ list, int slot0,
                                                    NlBuf L, M2Buf B0, const NlbCtl *__restrict__ ctl, int W3, NlbLooks Q)
{
    nlb_qsweep_tour<typename Elem<T>::acc, THREE>(S, OrMatCost<T>{mat, ld}, n, list, slot0, L, B0, ctl, W3, Q);
}

template <int KIND, bool THREE>
__global__ void __launch_bounds__(256) k_nlb_qsweep_otf(Tours S, const typename OrPt<KIND>::type *__restrict__ pts, int n,
                                                        const int *__restrict__ list, int slot0, NlBuf L, M2Buf B0,
                                                        const NlbCtl *__restrict__ ctl, int W3, NlbLooks Q)
{
    nlb_qsweep_tour<int, THREE>(S, OrPtsCost<KIND>{pts}, n, list, slot0, L, B0, ctl, W3, Q);
}

template <bool THREE>
__global__ void __launch_bounds__(256) k_nlb_wake(Tours S, int n, const int *__restrict__ list, int slot0, NlBuf L, M2Buf B0,
                                                  const NlbCtl *__restrict__ ctl, NlbLooks Q)
{
    const int t = list[blockIdx.y], place = t - slot0;
    const NlbCtl *c = ctl + place;
    if (c->stop) return;
    const LookBuf K = nlb_look(Q, t, place, n);
    const M2Buf B = nlb_view(B0, place, n);
    const int phase = c->phase, m = c->m;
    if (phase == 0) look_wake_tour<0>(S, n, t, L, K, B, m);
    else if (!THREE || phase == 1) look_wake_tour<1>(S, n, t, L, K, B, m);
    else look_wake_tour<2>(S, n, t, L, K, B, m);
}

// (phase and stop are read by every workgroup of the tour while workgroup 0 may write them: as in nlb_apply_tour it does so
// only behind a sweep that accepted nothing, whose m is 0, and "wake all" is written under the same condition)
template <typename T, bool THREE, typename CS>
__device__ __forceinline__ void nlb_dl_apply_tour(const Tours &S, const CS cs, int n, const int *__restrict__ list, int slot0, const M2Buf &B0,
                                                  NlbCtl *ctl, const NlBuf &L, const NlbLooks &Q)
{
    const int t = list[blockIdx.y], place = t - slot0;
    NlbCtl *c = ctl + place;
    typename NlbDlCtlOf<THREE>::type r;
    r.stop = c->stop; r.m = c->m; r.c = c; r.k = Q.look + place; r.closing = Q.closing; r.n = n;
    const M2Buf B = nlb_view(B0, place, n);
    const int phase = c->phase;             // (block-uniform: one load per thread of the same cell in front of every barrier)
    if (phase == 0) m2_apply_tour<T>(S, cs, n, t, B, &r);
    else if (!THREE || phase == 1) ornl_apply_tour<T>(S, cs, n, t, B, &r);
    else nl3_apply_tour<T>(S, cs, n, t, L, B, &r);
}

template <typename T, bool THREE>
__global__ void __launch_bounds__(256) k_nlb_apply_dl(Tours S, const T *__restrict__ mat, int n, int ld, const int *__restrict__ list, int slot0,
                                                      M2Buf B0, NlbCtl *ctl, NlBuf L, NlbLooks Q)
{
    nlb_dl_apply_tour<T, THREE>(S, OrMatCost<T>{mat, ld}, n, list, slot0, B0, ctl, L, Q);
}

template <int KIND, bool THREE>
__global__ void __launch_bounds__(256) k_nlb_apply_dl_otf(Tours S, const typename OrPt<KIND>::type *__restrict__ pts, int n,
                                                          const int *__restrict__ list, int slot0, M2Buf B0, NlbCtl *ctl, NlBuf L, NlbLooks Q)
{
    nlb_dl_apply_tour<int, THREE>(S, OrPtsCost<KIND>{pts}, n, list, slot0, B0, ctl, L, Q);
}
