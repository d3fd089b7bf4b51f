// ---------------------------------------------------------------------------
// Neighbour-list VNS: W independent walks of "descent over the lists, incumbent, kicks", every live walk served by every
// launch, kicks and incumbents on the device.
// Included by tspgpu.hip behind tspgpu_nlbatch.inc (uses Tours, NlbCtl, M2Buf, nlb_view, tour_init_body, wrap).  The rule is
// in include/tspgpu.h ("Neighbour-list VNS") and DESIGN 4.18.
//
// The descent of a walk is the batched neighbour-list descent's: the four kernels of tspgpu_nlbatch.inc are launched as they
// stand on the list of live walks.  One more launch follows them in every sweep round:
//
//   k_nlv_step<T>   one workgroup of 1024 threads per live walk (blockIdx.x indexes the device list of live slots).  A walk
//                   whose descent has not ended (NlbCtl::stop clear) or that has halted costs one early return.  Otherwise:
//                   the incumbent (strict <, a copy of succ), the trace cell, the kick draws on thread 0 (serial by nature:
//                   a few dozen loads from the walk's number block), every kick as an array operation of the whole workgroup
//                   on a second order array, then the body of k_tour_init on the result and the walk's NlbCtl re-armed.
//                   <T, true>: the walks with don't-look bits, see in front of the kernel.
//                   The cost source is k_tour_init's: the matrix, or (mat NULL) the points.
//
// A kick in array form (DESIGN 4.9 (iii)): with the tour written from node 0 in its own direction and the sorted picks
// p1 < p2 < p3, succ[a] = sb; succ[c] = sa; succ[b] = sc moves the positions (p2, p3] in front of (p1, p2]; everything else,
// node 0 at position 0 included, stays.  The walk's scratch order array takes the tour at the start of the phase and every
// kick; the slot is written only once the whole phase has its numbers, so a phase that runs dry leaves it untouched.
// ---------------------------------------------------------------------------
struct NlvCtl {             // one per walk, beside its NlbCtl
    int it, k;              // iterations completed, iterations asked for
    int halt;               // 0 walking, 1 finished (it == k), 2 dry: the numbers ran out in front of a kick phase
    int kick_pending;       // the descent of iteration `it` has ended and its kicks have not run
    int resume;             // the walk entered in front of a kick phase: its first step takes no incumbent and writes no trace
    int pad;
    long long cursor, nrand;    // numbers used up to the end of the last kick phase, numbers in the walk's block
    long long kicks;        // kicks applied by this call
    double best;            // cost of the incumbent
};

// the rejection rule's probe of vns_kick_host: the NODE at position p of the tour, unwrapped
__device__ __forceinline__ int nlv_probe(const int *tour, int p, int n)
{
    return p < 0 ? 0 : p >= n ? ((n & 3) == 2 ? -2 : 0) : tour[p];
}

// thread 0: the three picks of one kick from rv[cur ...], sorted into pick[]; false: the numbers ran out
__device__ __forceinline__ bool nlv_draw(const int *tour, int n, const int *__restrict__ rv, long long nrand, long long &cur, int pick[3])
{
    for (int i = 0; i < 3; i++) {
        int r = -1;
        while (r < 0) {
            if (cur >= nrand) return false;
            r = (int)((unsigned)rv[cur++] % (unsigned)n);
            for (int j = 0; j < i; j++)
                if (r == pick[j] || r == nlv_probe(tour, pick[j] - 1, n) || r == nlv_probe(tour, pick[j] + 1, n)) { r = -1; break; }
        }
        pick[i] = r;
        for (int j = i; j > 0 && pick[j] < pick[j - 1]; j--) { const int x = pick[j]; pick[j] = pick[j - 1]; pick[j - 1] = x; }
    }
    return true;
}

// DL ("Batched don't-look bits", rule 7 of the walks with looks): the step also writes the walk's three sets, awake[slot][3][n]:
// exactly the nodes whose unordered pair of tour neighbours differs between the local optimum in front of the kick phase and
// the tour behind it.  The local optimum's neighbours are kept by node in two idle candidate arrays before the first kick
template <typename T, bool DL>
__global__ void __launch_bounds__(1024) k_nlv_step(Tours S, const T *__restrict__ mat, int n, int ld, const int *__restrict__ list, int slot0,
                                                   M2Buf B0, NlbCtl *ctl, NlvCtl *vctl, int *ord2, int *best_succ,
                                                   const int *__restrict__ rand_values, double *trace, const double2 *__restrict__ pts,
                                                   int kind, unsigned char *awake)
{
    __shared__ double chunk[1024];
    __shared__ int sh[4];       // the picks of a kick; [3]: kicks of the phase, then -1 once the numbers ran out
    const int t = list[blockIdx.x], at = t - slot0;
    NlbCtl *c = ctl + at;
    NlvCtl *v = vctl + at;
    if (!c->stop || v->halt) return;        // (block-uniform, in front of every barrier; thread 0 writes both behind the last one)
    const int tid = threadIdx.x;
    const bool resume = v->resume != 0;
    const int it = v->it;
    const long long nrand = v->nrand;
    const int *rv = rand_values + (size_t)at * (size_t)nrand;
    const int *succ = S.succ + (size_t)t * n;
    int *ord = S.ord + (size_t)t * n;
    int *X = ord2 + (size_t)at * n;         // the tour from node 0, then behind every kick
    int *Y = nlb_view(B0, at, n).a;         // (the candidate arrays are idle between two descents)

    // the incumbent and the trace cell (src/tsp.c:669-676)
    if (!resume) {
        const double cost = S.cost[t];
        if (cost < v->best) {               // (v->best is written behind the next barrier)
            int *bs = best_succ + (size_t)at * n;
            for (int i = tid; i < n; i += blockDim.x) bs[i] = succ[i];
        }
        __syncthreads();
        if (tid == 0) {
            if (cost < v->best) v->best = cost;
            if (trace) trace[(size_t)at * v->k + it] = cost;
            v->kick_pending = 1;
        }
    }

    // the tour from node 0 in its own direction
    {
        const int p0 = S.pos[(size_t)t * n], dir = S.dir[t];
        for (int p = tid; p < n; p += blockDim.x) X[p] = ord[wrap(p0 + (dir > 0 ? p : -p), n)];
    }
    long long cur = v->cursor;              // (thread 0's)
    if (tid == 0) {
        int kicks = -1;
        if (cur < nrand) { kicks = rv[cur++] % 9 - 2; if (kicks < 0) kicks = 0; }
        sh[3] = kicks;
    }
    __syncthreads();
    const int kicks = sh[3];
    int *osucc = nlb_view(B0, at, n).b, *opred = nlb_view(B0, at, n).i;     // (DL; idle as Y is, and no kick writes them)
    if (DL)                                 // X is whole behind the barrier above; its first kick writes it two barriers on
        for (int p = tid; p < n; p += blockDim.x) {
            const int u = X[p];
            osucc[u] = X[p + 1 == n ? 0 : p + 1];
            opred[u] = X[p == 0 ? n - 1 : p - 1];
        }
    for (int j = 0; j < kicks; j++) {
        if (tid == 0) {
            int pick[3];
            if (nlv_draw(X, n, rv, nrand, cur, pick)) { sh[0] = pick[0]; sh[1] = pick[1]; sh[2] = pick[2]; }
            else sh[3] = -1;
        }
        __syncthreads();
        if (sh[3] < 0) break;               // (block-uniform: nothing writes sh[3] before the next barrier)
        const int p1 = sh[0], p2 = sh[1], p3 = sh[2], len = p3 - p1, head = p3 - p2;
        for (int i = tid; i < len; i += blockDim.x) Y[i] = X[p1 + 1 + i];
        __syncthreads();
        for (int i = tid; i < len; i += blockDim.x) X[p1 + 1 + i] = i < head ? Y[p2 - p1 + i] : Y[i - head];
        __syncthreads();
    }
    if (sh[3] < 0) {                        // dry: the slot holds the local optimum, the cursor stays in front of the phase
        if (tid == 0) { v->halt = 2; v->kick_pending = 1; }
        return;
    }

    // a freshly loaded tour: the order from node 0, dir = +1, and k_tour_init's body
    for (int p = tid; p < n; p += blockDim.x) ord[p] = X[p];
    __syncthreads();
    tour_init_body<T>(S, mat, n, ld, t, -1, pts, kind, chunk);
    if (DL) {                               // one pass over the positions of the kicked tour (X: nothing wrote it since the last kick)
        unsigned char *A = awake + (size_t)t * 3 * n;
        for (int p = tid; p < n; p += blockDim.x) {
            const int u = X[p], ns = X[p + 1 == n ? 0 : p + 1], np = X[p == 0 ? n - 1 : p - 1], os = osucc[u], op = opred[u];
            const unsigned char w = (ns == os && np == op) || (ns == op && np == os) ? 0 : 1;
            A[u] = w; A[(size_t)n + u] = w; A[2 * (size_t)n + u] = w;
        }
    }
    if (tid == 0) {
        v->cursor = cur;
        v->kicks += kicks;
        v->kick_pending = 0;
        v->resume = 0;
        v->it = it + 1;
        if (it + 1 >= v->k) v->halt = 1;    // (stop stays set: the walk leaves the list at the host's next look)
        else { c->phase = 0; c->phase_moves = 0; c->rounds += 1; c->stop = 0; }
    }
}
