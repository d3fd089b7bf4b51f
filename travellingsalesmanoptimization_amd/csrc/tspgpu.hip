// tspgpu.hip -- MI355X (gfx950 / CDNA4) 2-opt local-search engine: kernels + C ABI.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared
//        (see csrc/Makefile; -ffp-contract=off keeps dx*dx+dy*dy as two rounded
//        multiplies and one add, like the reference binary -- SURVEY 7, hard part 2)
//
// What runs here, and the reference loop each kernel takes over (file:line in
// the reference checkout):
//   k_build_costs   src/tsp.c:616-633              n x n rounded-Euclidean matrix (uint16 / int32 / f64 cells)
//   k_nn_vec, k_nn  src/algorithms/heuristics.c:216-288   nearest-neighbour tour (matrix / matrix-free)
//   k_tour_init     src/algorithms/refinment.c:6-9,43-46  cost recompute, prev/pos
//   k_sweep_fused   src/algorithms/refinment.c:49-114     ONE launch per sweep: apply the previous
//                                                         move + full pair scan (plain 2-opt)
//   k_sweep_res / k_sweep_pipe / k_sweep_simple / k_sweep_otf
//                   src/algorithms/refinment.c:49-69      full pair scan, argmin (rows resident in
//                   src/algorithms/metaheuristic.c:198-222  LDS / streamed / one row / matrix-free);
//                                                         TABU variants
//   k_apply         src/algorithms/refinment.c:74-86,95-114  apply best move (batches, tabu)
//                   src/algorithms/metaheuristic.c:226-240,40-59 (TABU variant)
//   sweep_step(), BState, pipe_stream(): the step evaluation and row streaming the LDS sweeps share
//
// Tour representation on the device: position array ord[p] (+ inverse pos[],
// successor succ[] and dnext[b] = c[b][succ b]).  A 2-opt move (a,b) reverses
// the cyclic position range pos[a]+1 .. pos[b], which is exactly the segment
// succ_a .. b that ref_reverse_path flips, so the successor direction -- and
// with it every later (a,b) label and tie-break -- matches the reference.
//
// Argmin order: the reference scans a ascending, b ascending and keeps the
// first strictly smallest delta, i.e. it minimises the key (delta, a, b).  Here
// every workgroup minimises that same key over its share of the pairs, so the
// scan order on the device is free.
//
// There is no CPU fallback anywhere in this file.

#include <hip/hip_runtime.h>
#include <cstddef>

#include <algorithm>
#include <chrono>
#include <cfloat>
#include <climits>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "tspgpu.h"
#include "tspgpu_relaunch.h"    // LP_ST_*, and the host's protocol over them (run_persist, run_pstream)
#include "tspgpu_looks.h"       // rounds of launches between looks at a control block (m2_run, or_run, the batched descents)
#include "tspgpu_descent.h"     // Descent, descent_out, and the descent over the neighbour lists on one tour (nl_descent)
#include "tspgpu_plan.h"        // the launch plans: which kernel, what geometry (make_plan, run_persist, run_pstream, or_plan, m2_plan)
#include "tspgpu_nlphase.h"     // NlbCtl and the phase machine of a tour of a batched neighbour-list descent (tspgpu_nlbatch.inc)
#include "tspgpu_lds_tmat.h"    // index arithmetic of the tour-ordered matrix copy (k_lds2opt's TM instantiations)

#ifndef TSPGPU_RPC
#define TSPGPU_RPC 3   // rows landed per chunk in the resident bodies (tools: -DTSPGPU_RPC=2 to compare)
#endif

// reference ERROR_CODE numbering (src/utils/errors.h:33-51)
enum { E_OK = 0, E_INVALID = 3, E_DEADLINE = 4, E_EXHAUSTED = 8, E_PRECOND = 9,
       E_UNIMPL = 12, E_INTERNAL = 13, E_UNAVAILABLE = 14 };

#define TWO_OPT_EPS (-1.0E-7) /* src/tsp.h:19 */

typedef unsigned long long u64;

static constexpr u64 KEY_NONE = ~0ull;
using plan::MAX_WGS_PER_TOUR;

struct Partial {
    double d;
    u64 key; // (lo << 32) | hi, KEY_NONE when the workgroup found nothing
};
static_assert(sizeof(Partial) == plan::PARTIAL_BYTES, "the plans count a Partial's bytes");
static_assert(TSPGPU_ELEM_F64 == plan::ELEM_F64 && TSPGPU_ELEM_I32 == plan::ELEM_I32 && TSPGPU_ELEM_U16 == plan::ELEM_U16, "the plans' element kinds are the ABI's");

// ---------------------------------------------------------------------------
// element traits: the matrix is held either as doubles (any caller matrix) or
// as an exact int32 copy (every integer-valued matrix: EUC_2D, ATT, CEIL_2D)
// ---------------------------------------------------------------------------
typedef unsigned short u16;
typedef __attribute__((address_space(3))) unsigned char lds_u8;
typedef __attribute__((address_space(3))) unsigned short lds_u16;
typedef double v2f64 __attribute__((ext_vector_type(2)));
typedef int v4i32 __attribute__((ext_vector_type(4)));
typedef u16 v8u16 __attribute__((ext_vector_type(8)));

// T = storage type of a matrix cell, acc = the type deltas are computed in.
// uint16 cells hold exact integer costs 0..65534; 65535 is the diagonal (-1 in the reference).
template <typename T> struct Elem;
template <> struct Elem<double> {
    typedef v2f64 vec;
    typedef double acc;
    static constexpr int V = 2;
    __device__ static double lim() { return DBL_MAX; }
    __device__ static double big() { return 1.0e300; }   // poison: above any real delta, sums stay finite
    __device__ static double widen(double x) { return x; }
};
template <> struct Elem<int> {
    typedef v4i32 vec;
    typedef int acc;
    static constexpr int V = 4;
    __device__ static int lim() { return INT_MAX; }
    // poison; real costs lie in [-1, 2^27): a 2-opt delta (two weights against two) stays below 2^28 in magnitude, a
    // three-edge delta (Or-opt, 3-opt: three weights against three) below 3 * 2^27 -- both under the 2^29 poison and inside int32
    __device__ static int big() { return 1 << 29; }
    __device__ static double widen(int x) { return (double)x; }
};
template <> struct Elem<u16> {
    typedef v8u16 vec;
    typedef int acc;
    static constexpr int V = 8;
    __device__ static int lim() { return INT_MAX; }
    __device__ static int big() { return 1 << 29; }
    __device__ static double widen(u16 x) { return x == 0xFFFFu ? -1.0 : (double)x; }
};

__device__ __forceinline__ double vget(const v2f64 &v, int i) { return v[i]; }
__device__ __forceinline__ int vget(const v4i32 &v, int i) { return v[i]; }
__device__ __forceinline__ int vget(const v8u16 &v, int i) { return (int)v[i]; }

// V consecutive elements starting at p (16-byte vector loads; the arrays carry slack behind
// the last tour so that a read up to V-1 elements past n stays inside the allocation)
template <int V, typename E>
__device__ __forceinline__ void load_run(const E *p, E (&out)[V])
{
    constexpr int PER = 16 / (int)sizeof(E);
    typedef E vec_t __attribute__((ext_vector_type(PER)));
    static_assert(V % PER == 0 || V < PER, "run must be whole vectors");
    if constexpr (V >= PER) {
#pragma unroll
        for (int k = 0; k < V / PER; k++) {
            vec_t x;
            __builtin_memcpy(&x, p + k * PER, sizeof x);
#pragma unroll
            for (int e = 0; e < PER; e++) out[k * PER + e] = x[e];
        }
    } else {
        typedef E half_t __attribute__((ext_vector_type(V)));
        half_t x;
        __builtin_memcpy(&x, p, sizeof x);
#pragma unroll
        for (int e = 0; e < V; e++) out[e] = x[e];
    }
}

__device__ __forceinline__ bool key_better(double d1, u64 k1, double d2, u64 k2)
{
    return d1 < d2 || (d1 == d2 && k1 < k2);
}

// Wave-wide reductions through DPP (data-parallel primitives: the operand of a VALU instruction comes from another
// lane of the same 16-lane row, or, row_bcast15 / row_bcast31, from the last lane of the rows before) instead of
// __shfl_xor, which hipcc lowers to ds_bpermute: six dependent trips through the LDS crossbar per butterfly, at the end
// of EVERY sweep workgroup and in every nearest-neighbour step.  Quad swaps and the two mirrors leave each row with
// its minimum, the two broadcasts carry it across the rows; lane 63 ends with the wave's, v_readlane hands it out.
template <int CTRL, int ROWS> __device__ __forceinline__ unsigned dpp_u32(unsigned x)
{
    return (unsigned)__builtin_amdgcn_update_dpp((int)x, (int)x, CTRL, ROWS, 0xf, false);
}
template <int CTRL, int ROWS> __device__ __forceinline__ u64 dpp_u64(u64 x)
{
    return ((u64)dpp_u32<CTRL, ROWS>((unsigned)(x >> 32)) << 32) | dpp_u32<CTRL, ROWS>((unsigned)x);
}
__device__ __forceinline__ u64 lane63_u64(u64 x)
{
    return ((u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), 63) << 32) |
           (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, 63);
}
#define DPP_WAVE_STEPS(STEP)                                                                 \
    STEP(0xB1, 0xf)  /* quad_perm [1,0,3,2] */ STEP(0x4E, 0xf) /* quad_perm [2,3,0,1] */     \
    STEP(0x141, 0xf) /* row_half_mirror */     STEP(0x140, 0xf) /* row_mirror */             \
    STEP(0x142, 0xa) /* row_bcast15 -> rows 1, 3 */ STEP(0x143, 0xc) /* row_bcast31 -> rows 2, 3 */

// wave-wide minimum of a signed 64-bit key, valid in every lane
__device__ __forceinline__ long long wave_min_i64(long long k)
{
#define STEP(C, R) { const long long o = (long long)dpp_u64<C, R>((u64)k); k = o < k ? o : k; }
    DPP_WAVE_STEPS(STEP)
#undef STEP
    return (long long)lane63_u64((u64)k);
}

// wave-wide lexicographic minimum of (d, key), valid in every lane
__device__ __forceinline__ void wave_argmin(double &d, u64 &key)
{
#define STEP(C, R) { const double od = __longlong_as_double((long long)dpp_u64<C, R>((u64)__double_as_longlong(d))); \
                     const u64 ok = dpp_u64<C, R>(key);                                                                 \
                     if (key_better(od, ok, d, key)) { d = od; key = ok; } }
    DPP_WAVE_STEPS(STEP)
#undef STEP
    d = __longlong_as_double((long long)lane63_u64((u64)__double_as_longlong(d)));
    key = lane63_u64(key);
}

// block-wide lexicographic min of (d, key); result valid in every thread.
// scratch: 2 * 16 Partial-sized slots.
__device__ __forceinline__ void block_argmin(double &d, u64 &key, Partial *scratch)
{
    wave_argmin(d, key);
    const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) { scratch[w].d = d; scratch[w].key = key; }
    __syncthreads();
    d = scratch[0].d; key = scratch[0].key;
    for (int i = 1; i < nw; i++) {
        double od = scratch[i].d; u64 ok = scratch[i].key;
        if (key_better(od, ok, d, key)) { d = od; key = ok; }
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------
// K1: cost matrix.  grid (ceil(ld / (256*V)), n): one row per blockIdx.y, each
// thread stores one 16-byte vector.  Write-bound: sizeof(T) * n * ld bytes.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double edge_weight(double ax, double ay, double bx, double by, int kind)
{
    // src/tsp.c:629: (double)((int)(sqrtf(pow(dx,2)+pow(dy,2)) + 0.5)); the sum is a
    // double, sqrtf takes it narrowed to float, the root is widened before +0.5.
    double dx = bx - ax, dy = by - ay;
    double sq = dx * dx + dy * dy; // -ffp-contract=off: no fma
    if (kind == TSPGPU_EUC_2D) {
        float root = __builtin_sqrtf((float)sq); // correctly rounded (hipcc default)
        return (double)((int)((double)root + 0.5));
    }
    if (kind == TSPGPU_ATT) { // TSPLIB 95
        double r = __builtin_sqrt(sq / 10.0);
        double t = (double)(long long)(r + 0.5);
        return t < r ? t + 1.0 : t;
    }
    return __builtin_ceil(__builtin_sqrt(sq)); // CEIL_2D
}

// one matrix cell, from the resident matrix or -- matrix-free mode, mat == nullptr -- recomputed
// from the coordinates with the very same arithmetic
template <typename T>
__device__ __forceinline__ typename Elem<T>::acc cell(const T *mat, const double2 *pts, int kind, int ld, int u, int v)
{
    typedef typename Elem<T>::acc AT;
    if (mat) return (AT)mat[(size_t)u * ld + v];
    const double2 pu = pts[u], pv = pts[v];
    return (AT)edge_weight(pu.x, pu.y, pv.x, pv.y, kind);
}

// One integer edge weight, specialised on the kind (no branch in the inner loop).  EUC_2D: the
// correctly rounded f32 root written out exactly as hipcc expands sqrtf() -- v_sqrt_f32 (1 ulp)
// and one fix-up step on either side with two FMAs -- minus the denormal scaling and the class
// test that weights (0 or >= 1) cannot need.  KIND 3 = CEIL_2D on integer coordinates with every
// weight below 2^22 (ceil_int()): d2 is an exact integer below 2^44, so ceil(sqrt(d2)) is the
// smallest j with j*j >= d2.  The f32 root r is within 0.375 of sqrt(d2) (the conversion of d2
// costs the root 2^-25 relative, v_sqrt_f32 one ulp <= 0.25), so k = floor(r) is
// floor(sqrt(d2)) - 1, + 0 or + 1, and ONE exact remainder e = d2 - k*k (an integer of at most 24
// bits) decides between k - 1 .. k + 2 in 32-bit integer arithmetic:
//     e > 0:  (k+1)^2 >= d2  <=>  e <= 2k + 1  ->  k + 1, else k + 2
//     e = 0:  k
//     e < 0:  (k-1)^2 >= d2  <=>  e + 2k - 1 <= 0  ->  k - 1, else k
// (round 2's form corrected k three times in a row with f64 products: 14 f64 instructions per weight in a dependent chain.)
constexpr int KIND_CEIL_INT = 3;
// F32R (EUC_2D only): the final (int)((double)root + 0.5) in f32 -- exact while the root is below 2^22 (root + 0.5f is then
// representable: 0.5 is a multiple of the root's ulp), three f64 conversions / additions less per weight
template <int KIND, bool F32R = false>
__device__ __forceinline__ int edge_w(double ax, double ay, double bx, double by)
{
    const double dx = bx - ax, dy = by - ay;
    double sq;
    if constexpr (KIND == KIND_CEIL_INT) sq = __builtin_fma(dy, dy, dx * dx);   // (integers: every step exact, fused or not)
    else sq = dx * dx + dy * dy; // -ffp-contract=off: no fma
    if constexpr (KIND == TSPGPU_EUC_2D) {
        const float x = (float)sq;
        const float r = __builtin_amdgcn_sqrtf(x);
        const float rm = __int_as_float(__float_as_int(r) - 1), rp = __int_as_float(__float_as_int(r) + 1);
        const float em = __builtin_fmaf(-rm, r, x), ep = __builtin_fmaf(-rp, r, x);
        float c = 0.0f >= em ? rm : r;
        c = 0.0f < ep ? rp : c;
        if constexpr (F32R) return (int)(c + 0.5f);
        return (int)((double)c + 0.5);
    } else if constexpr (KIND == KIND_CEIL_INT) {
        const int ki = (int)__builtin_amdgcn_sqrtf((float)sq);
        const double k = (double)ki;
        const int e = (int)__builtin_fma(-k, k, sq), t1 = 2 * ki + 1;
        const int up = e > t1 ? 2 : 1, down = e + t1 <= 2 ? -1 : 0;
        return ki + (e > 0 ? up : e < 0 ? down : 0);
    } else return (int)edge_weight(ax, ay, bx, by, KIND);
}


// The same weight (CEIL_2D, integer coordinates, below 2^22) from INTEGER coordinates, without one f64 instruction -- the
// matrix-free sweep's form (k_sweep_otf8<KIND_CEIL_INT>): |dx|, |dy| < 2^22 fit the signed 24-bit multipliers
// (v_mul_i32_i24 / v_mad_i32_i24: full rate, low 32 bits of the 48-bit product), d2 mod 2^32 is all the remainder needs
// (|e| < 2^24 survives the wrap), and the f32 root may come from an f32 d2: (float)dx is exact, dx*dx and the fused sum
// cost d2 2^-23 relative, the root 2^-24 (0.25 at 2^22), v_sqrt_f32 one ulp (<= 0.25): within 0.5 of sqrt(d2), so
// k = floor(r) is floor(sqrt(d2)) - 1, + 0 or + 1 as in edge_w<KIND_CEIL_INT> and the same remainder decides.
__device__ __forceinline__ int edge_w_ceil_i(int ax, int ay, int bx, int by)
{
    const int dx = bx - ax, dy = by - ay;
    const float fx = (float)dx, fy = (float)dy;
    const int ki = (int)__builtin_amdgcn_sqrtf(__builtin_fmaf(fy, fy, fx * fx));
    const int d2lo = __mul24(dx, dx) + __mul24(dy, dy);      // d2 mod 2^32
    const int e = d2lo - (int)__umul24((unsigned)ki, (unsigned)ki), t1 = 2 * ki + 1;
    // k is the floor itself nearly always (0 <= e <= 2k): one compare-and-add; the two corrections sit behind a branch a
    // whole wave rarely takes (measured: the branch-free sum of three comparisons is 7 % slower on pla85900)
    int r = ki + (int)(e > 0);
    if (__builtin_expect((unsigned)e > (unsigned)t1, 0))      // e > 2k + 1 or e < 0
        r = e > 0 ? ki + 2 : (e + t1 <= 2 ? ki - 1 : ki);
    return r;
}

// K1 for the integer storages: the weight kind is a template parameter (no branch per cell), the integer weight is
// produced directly (edge_w: for EUC_2D the correctly rounded f32 root written out, see above), and a workgroup keeps
// the points of its 256 * V columns in registers while it walks BUILD_ROWS rows -- with one row per workgroup the
// kernel read 16 bytes of coordinates per 2-byte cell from L2 (268 MB for a 33.5 MB matrix at n=4096) and waited on
// them 78 % of the time.  Same cells as k_build_costs<T> below, which stays for f64 storage (weights that may exceed
// the int range; write-bound at 0.70 of the HBM peak as it is).
constexpr int BUILD_ROWS = 16;
template <typename T, int KIND>
__global__ void __launch_bounds__(256) k_build_costs_int(const double2 *__restrict__ pts, int n, int ld, T *__restrict__ out)
{
    typedef typename Elem<T>::vec VT;
    constexpr int V = Elem<T>::V;
    const int j0 = (blockIdx.x * 256 + threadIdx.x) * V;
    if (j0 >= ld) return;
    double2 pj[V];
#pragma unroll
    for (int k = 0; k < V; k++) pj[k] = pts[min(j0 + k, n - 1)];
    const int i0 = blockIdx.y * BUILD_ROWS, i1 = min(n, i0 + BUILD_ROWS);
    for (int i = i0; i < i1; i++) {
        const double2 pi = pts[i];                       // (wave-uniform: a scalar load)
        VT o;
#pragma unroll
        for (int k = 0; k < V; k++) {
            const int j = j0 + k;
            const int w = edge_w<KIND>(pi.x, pi.y, pj[k].x, pj[k].y);
            o[k] = j >= n ? (T)0 : j == i ? (T)-1 : (T)w;
        }
        *reinterpret_cast<VT *>(out + (size_t)i * ld + j0) = o;
    }
}

// K1, one triangle: the matrix is symmetric to the last bit (dx * dx == (-dx) * (-dx)), so a 64 x 64 tile (I, J), I <= J, is
// computed once and stored twice -- as it stands (rows of tile (I, J)) and, through an LDS transpose, as tile (J, I): half
// the arithmetic of k_build_costs_int (the kernel that was arithmetic-bound: ~20 vector instructions per cell, VERDICT r2
// "weak" 8), all stores 32-byte row segments.  Grid: one workgroup per tile of the upper triangle, diagonal included.
// Thread (r, s) of 64 x 4 takes row r, columns 16 s .. 16 s + 15 of the tile; the 128 points come from LDS.
constexpr int TRI = 64;
template <typename T, int KIND, bool F32R>
__global__ void __launch_bounds__(256) k_build_costs_tri(const double2 *__restrict__ pts, int n, int ld, int NT, T *__restrict__ out)
{
    constexpr int STR = TRI + 16 / (int)sizeof(T);        // transposed tile's row stride: rows stay 16-byte aligned
    __shared__ double2 P[2 * TRI];
    __shared__ __attribute__((aligned(16))) T TT[TRI * STR];
    // tile (I, J) of the upper triangle from the linear block index: row I holds NT - I tiles
    int I = 0, rest = (int)blockIdx.x;
    {   // (solve rest = I * NT - I (I - 1) / 2 + (J - I) without a loop: float guess, integer correction)
        const float a = (float)(2 * NT + 1);
        I = (int)((a - __builtin_sqrtf(a * a - 8.0f * (float)rest)) * 0.5f);
        I = max(0, min(I, NT - 1));
        while (I > 0 && I * NT - I * (I - 1) / 2 > rest) I--;
        while (I + 1 < NT && (I + 1) * NT - (I + 1) * I / 2 <= rest) I++;
        rest -= I * NT - I * (I - 1) / 2;
    }
    const int J = I + rest;
    const int tid = (int)threadIdx.x, r = tid >> 2, c0 = (tid & 3) * 16;
    if (tid < 2 * TRI) P[tid] = pts[min((tid < TRI ? I : J) * TRI + (tid & (TRI - 1)), n - 1)];
    __syncthreads();
    const int i = I * TRI + r, j0 = J * TRI + c0;
    const double2 pi = P[r];
    T w[16];
    const bool inner = I != J && (J + 1) * TRI <= n;      // no diagonal cell, no column past n: no masks (workgroup-uniform)
    if (inner) {
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const double2 pj = P[TRI + c0 + k];
            w[k] = (T)edge_w<KIND, F32R>(pi.x, pi.y, pj.x, pj.y);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const double2 pj = P[TRI + c0 + k];
            const int j = j0 + k;
            const int v = edge_w<KIND, F32R>(pi.x, pi.y, pj.x, pj.y);
            w[k] = j >= n ? (T)0 : j == i ? (T)-1 : (T)v;
        }
    }
    typedef T vec16 __attribute__((ext_vector_type(16)));
    if (i < n && j0 < ld) {
        vec16 o;
#pragma unroll
        for (int k = 0; k < 16; k++) o[k] = w[k];
        *reinterpret_cast<vec16 *>(out + (size_t)i * ld + j0) = o;
    }
    if (I == J) return;                                    // (a diagonal tile is its own transpose)
#pragma unroll
    for (int k = 0; k < 16; k++) TT[(c0 + k) * STR + r] = w[k];
    __syncthreads();
    const int jt = J * TRI + r, it0 = I * TRI + c0;        // row of tile (J, I), its first column (I < J: every column < n)
    if (jt < n) *reinterpret_cast<vec16 *>(out + (size_t)jt * ld + it0) = *reinterpret_cast<const vec16 *>(TT + r * STR + c0);
}

// The same with 128 x 128 tiles (round 4, n >= 1024): thread (rg, cc) of 32 x 8 takes rows rg, rg + 32, rg + 64, rg + 96 and columns
// 16 cc .. 16 cc + 15 of the tile, so that one store instruction writes eight 256-byte row segments (the 64 x 64 form: sixteen
// 128-byte ones, 8 KB apart -- its transposed half stored at about a third of the rate of whole rows); the thread's 16 column
// points stay in registers over its four rows.
constexpr int TRIB = 128;
template <typename T, int KIND, bool F32R>
__global__ void __launch_bounds__(256) k_build_costs_tri128(const double2 *__restrict__ pts, int n, int ld, int NT, T *__restrict__ out)
{
    constexpr int STR = TRIB + 16 / (int)sizeof(T);       // transposed tile's row stride: rows stay 16-byte aligned
    __shared__ double2 P[2 * TRIB];
    __shared__ __attribute__((aligned(16))) T TT[TRIB * STR];
    int I = 0, rest = (int)blockIdx.x;
    {
        const float a = (float)(2 * NT + 1);
        I = (int)((a - __builtin_sqrtf(a * a - 8.0f * (float)rest)) * 0.5f);
        I = max(0, min(I, NT - 1));
        while (I > 0 && I * NT - I * (I - 1) / 2 > rest) I--;
        while (I + 1 < NT && (I + 1) * NT - (I + 1) * I / 2 <= rest) I++;
        rest -= I * NT - I * (I - 1) / 2;
    }
    const int J = I + rest;
    const int tid = (int)threadIdx.x, rg = tid >> 3, c0 = (tid & 7) * 16;
    P[tid] = pts[min((tid < TRIB ? I : J) * TRIB + (tid & (TRIB - 1)), n - 1)];
    __syncthreads();
    double2 pj[16];
#pragma unroll
    for (int k = 0; k < 16; k++) pj[k] = P[TRIB + c0 + k];
    const int j0 = J * TRIB + c0;
    const bool inner = I != J && (J + 1) * TRIB <= n;     // no diagonal cell, no column past n: no masks (workgroup-uniform)
    typedef T vec16 __attribute__((ext_vector_type(16)));
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int r = rg + 32 * q, i = I * TRIB + r;
        const double2 pi = P[r];
        T w[16];
        if (inner) {
#pragma unroll
            for (int k = 0; k < 16; k++) w[k] = (T)edge_w<KIND, F32R>(pi.x, pi.y, pj[k].x, pj[k].y);
        } else {
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int j = j0 + k;
                const int v = edge_w<KIND, F32R>(pi.x, pi.y, pj[k].x, pj[k].y);
                w[k] = j >= n ? (T)0 : j == i ? (T)-1 : (T)v;
            }
        }
        if (i < n && j0 < ld) {
            vec16 o;
#pragma unroll
            for (int k = 0; k < 16; k++) o[k] = w[k];
            *reinterpret_cast<vec16 *>(out + (size_t)i * ld + j0) = o;
        }
        if (I != J) {
#pragma unroll
            for (int k = 0; k < 16; k++) TT[(c0 + k) * STR + r] = w[k];
        }
    }
    if (I == J) return;                                    // (a diagonal tile is its own transpose)
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int r = rg + 32 * q;
        const int jt = J * TRIB + r, it0 = I * TRIB + c0;  // row of tile (J, I), its first column (I < J: every column < n)
        if (jt < n) *reinterpret_cast<vec16 *>(out + (size_t)jt * ld + it0) = *reinterpret_cast<const vec16 *>(TT + r * STR + c0);
    }
}

template <typename T>
__global__ void __launch_bounds__(256) k_build_costs(const double2 *__restrict__ pts, int n, int ld, int kind,
                                                     T *__restrict__ out)
{
    typedef typename Elem<T>::vec VT;
    constexpr int V = Elem<T>::V;
    const int i = blockIdx.y;
    const int j0 = (blockIdx.x * 256 + threadIdx.x) * V;
    if (j0 >= ld) return;
    const double2 pi = pts[i];
    T v[V];
#pragma unroll
    for (int k = 0; k < V; k++) {
        const int j = j0 + k;
        if (j >= n) v[k] = (T)0;
        else if (j == i) v[k] = (T)-1;
        else {
            const double2 pj = pts[j];
            v[k] = (T)edge_weight(pi.x, pi.y, pj.x, pj.y, kind);
        }
    }
    VT o;
#pragma unroll
    for (int k = 0; k < V; k++) o[k] = v[k];
    *reinterpret_cast<VT *>(out + (size_t)i * ld + j0) = o;
}

// ingest of a caller matrix: flags[0] = some entry is not an int in [-1, 2^27),
// flags[1] = some c[i][j] != c[j][i], flags[2] = not representable as uint16 cells
// (off-diagonal integer in [0, 65534], diagonal exactly -1)
__global__ void __launch_bounds__(256) k_inspect(const double *__restrict__ m, int n, int ld, int *flags)
{
    const int i = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const double x = m[(size_t)i * ld + j];
    const double r = __builtin_trunc(x);
    if (!(r == x && x >= -1.0 && x < 134217728.0)) flags[0] = 1;
    if (j > i && m[(size_t)j * ld + i] != x) flags[1] = 1;
    if (i == j ? x != -1.0 : !(r == x && x >= 0.0 && x <= 65534.0)) flags[2] = 1;
    if (i != j && !(x <= 16383.0)) flags[3] = 1;
    if (i != j && !(x <= 8190.0)) flags[4] = 1;
}

template <typename TD>
__global__ void __launch_bounds__(256) k_from_f64(const double *__restrict__ m, int n, int ld, TD *__restrict__ out)
{
    const int i = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= ld) return;
    out[(size_t)i * ld + j] = j < n ? (TD)(int)m[(size_t)i * ld + j] : (TD)0; // -1 -> 0xFFFF for uint16
}

template <typename TS>
__global__ void __launch_bounds__(256) k_to_f64(const TS *__restrict__ m, int n, int ld, double *__restrict__ out)
{
    const int i = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= ld) return;
    out[(size_t)i * ld + j] = j < n ? Elem<TS>::widen(m[(size_t)i * ld + j]) : 0.0;
}

// ---------------------------------------------------------------------------
// tour state (structure of arrays over tour slots)
//
//   ord[p]   node at array position p
//   pos[v]   inverse of ord
//   dpos[p]  cost of the tour edge between array positions p and p+1 (cyclic),
//            in the tour's current direction
//   dir      +1: succ(ord[p]) = ord[p+1];  -1: succ(ord[p]) = ord[p-1]
//   succ[b], dnb[b]  node-indexed view for the sweeps: successor of b and c[b][succ b],
//            rebuilt by k_apply after each move so that every sweep workgroup reads them
//            with coalesced loads (deriving them per workgroup from pos/ord/dpos costs n
//            random reads per workgroup: measured 3-7 us per sweep)
//
// A 2-opt move flips one of the two arcs the removed edges cut the cycle into.
// ref_reverse_path flips the arc succ_a .. b; flipping the OTHER arc and
// toggling `dir` yields the identical successor function, so k_apply always
// reverses the shorter arc (<= n/2 array cells).  Reversing an array range also
// reverses the order of the edge costs inside it, and only the two boundary
// edges {a,b}, {succ_a,succ_b} are new: two matrix reads per move.
// ---------------------------------------------------------------------------
struct Tours {
    int *ord, *pos, *succ;   // [cap][n]
    double *dpos, *dnb;      // [cap][n] 8-byte slots; integer modes use the first 4n bytes of each
    double *cost, *last_delta; // [cap]
    int *dir, *done, *nsweeps, *cap_sweeps, *status; // [cap]
    Partial *partial;        // [cap][pstride]
    int pstride;             // partial slots per tour (>= workgroups per tour of any sweep)
};

struct TabuState {           // device-resident, slot 0 only
    int iter, tenure, t_min, t_max, up, resident;
    double best_cost;
};

struct HistBuf { int *a, *b; double *d; int cap; };

struct Fused {               // ping-pong state of the one-launch-per-sweep path, [parity]
    int *ord[2], *pos[2], *nl[2], *nr[2];   // [cap][n]
    double *dl[2], *dr[2];                  // [cap][n] 8-byte slots
    int *dir[2], *k[2], *stop[2];           // [cap]
    double *cost[2];                        // [cap]
    Partial *partial[2];                    // [cap][pstride]
    int *cur;                               // [cap] parity holding the result once `done`
    // uint16 cells: instead of partials every workgroup atomic-mins ONE packed 64-bit key per tour
    // (delta:19 | a:16 | b:16 | workgroup:13; three slots in rotation: read / written / reset) and
    // the workgroups leave the geometry of their best move in a record the next launch reads
    // with one scalar load: {cell a, cell b, a, succ a, b, succ b, c[a][b], c[sa][sb]}
    long long *bestkey;                     // [cap][4]
    int *payload[2];                        // [cap][pstride][8]
};

template <typename T>
__device__ __forceinline__ T *dpos_of(const Tours &S, int t, int n)
{
    return reinterpret_cast<T *>(S.dpos + (size_t)t * n);
}
template <typename T>
__device__ __forceinline__ T *dnb_of(const Tours &S, int t, int n)
{
    return reinterpret_cast<T *>(S.dnb + (size_t)t * n);
}

__device__ __forceinline__ int wrap(int p, int n) { return p < 0 ? p + n : (p >= n ? p - n : p); }

// ---------------------------------------------------------------------------
// k_tour_init: ord[] given (dir = +1); derive pos/dpos and the cost exactly as
// ref_2opt recomputes it (src/algorithms/refinment.c:6-9): sum over NODE index
// i = 0..n-1 of c[i][succ i], accumulated in that order (doubles), so that
// non-integer matrices give the same bits.  One workgroup per tour.
// ---------------------------------------------------------------------------
// (the body: k_tour_init on slot t, and the step kernel of tspgpu_nlvns.inc on the tour its kicks leave.  chunk: [1024]
// doubles of LDS; the whole workgroup calls it)
template <typename T>
__device__ __forceinline__ void tour_init_body(const Tours &S, const T *__restrict__ mat, int n, int ld, int t, int cap,
                                               const double2 *__restrict__ pts, int kind, double *chunk)
{
    typedef typename Elem<T>::acc AT;
    const int *ord = S.ord + (size_t)t * n;
    int *pos = S.pos + (size_t)t * n;
    AT *dp = dpos_of<AT>(S, t, n);
    AT *dnb = dnb_of<AT>(S, t, n);
    int *succ = S.succ + (size_t)t * n;
    for (int p = threadIdx.x; p < n; p += blockDim.x) {
        const int node = ord[p];
        const int s = ord[p + 1 == n ? 0 : p + 1];
        const AT w = cell<T>(mat, pts, kind, ld, node, s);
        pos[node] = p;
        dp[p] = w;
        succ[node] = s;
        dnb[node] = w;
    }
    __syncthreads();
    double total = 0;
    if constexpr (std::is_same<AT, int>::value) {
        long long part = 0;
        for (int i = threadIdx.x; i < n; i += blockDim.x) part += dnb[i];
        for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
        long long *acc = reinterpret_cast<long long *>(chunk);
        if ((threadIdx.x & 63) == 0) acc[threadIdx.x >> 6] = part;
        __syncthreads();
        if (threadIdx.x == 0) {
            long long s = 0;
            for (int w = 0; w < (int)((blockDim.x + 63) >> 6); w++) s += acc[w];
            total = (double)s;
        }
    } else {
        for (int base = 0; base < n; base += 1024) {
            const int m = min(1024, n - base);
            for (int i = threadIdx.x; i < m; i += blockDim.x) chunk[i] = dnb[base + i]; // c[i][succ i]
            __syncthreads();
            if (threadIdx.x == 0)
                for (int i = 0; i < m; i++) total += chunk[i];
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {
        S.cost[t] = total;
        S.last_delta[t] = 0;
        S.dir[t] = 1;
        S.done[t] = 0;
        S.nsweeps[t] = 0;
        S.cap_sweeps[t] = cap;
        S.status[t] = 0;
    }
}

template <typename T>
__global__ void __launch_bounds__(1024) k_tour_init(Tours S, const T *__restrict__ mat, int n, int ld, int slot0,
                                                    const int *__restrict__ caps, const double2 *__restrict__ pts, int kind)
{
    __shared__ double chunk[1024];
    tour_init_body<T>(S, mat, n, ld, slot0 + blockIdx.x, caps ? caps[blockIdx.x] : -1, pts, kind, chunk);
}

// ---------------------------------------------------------------------------
// K6: nearest-neighbour tour, one workgroup per start.  Thread tid owns nodes
// tid, tid+BT, ... (coalesced row reads) and keeps their visited bits in a
// register mask (n <= 64*BT).  Each step: masked row argmin by (weight, index)
// -> ties go to the lowest index, as the strict < of heuristics.c:258.
// ---------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(1024) k_nn(Tours S, const T *__restrict__ mat, int n, int ld, int slot0,
                                             const int *__restrict__ starts, const double2 *__restrict__ pts, int kind)
{
    __shared__ Partial red[2][16];
    __shared__ int fill_pos;
    const int t = slot0 + blockIdx.x;
    const int start = starts[blockIdx.x];
    int *ord = S.ord + (size_t)t * n;
    const int tid = threadIdx.x, BT = blockDim.x;
    const int nw = (BT + 63) >> 6;
    u64 seen = 0, seen_hi = 0; // bit k <-> node tid + k*BT (k < 128: n <= 128*BT)
    if (start % BT == tid) { const int k = start / BT; if (k < 64) seen |= 1ull << k; else seen_hi |= 1ull << (k - 64); }
    int cur = start;
    double total = 0;
    if (tid == 0) ord[0] = start;
    int step = 1;
    for (; step < n; step++) {
        const T *row = mat + (size_t)cur * ld;
        double2 pc = make_double2(0, 0);
        if (!mat) pc = pts[cur];
        double lo = DBL_MAX;
        u64 arg = KEY_NONE;
        for (int k = 0, i = tid; i < n; i += BT, k++) {
            if (((k < 64 ? seen >> k : seen_hi >> (k - 64)) & 1)) continue;
            double w;
            if (mat) w = Elem<T>::widen(row[i]);
            else { const double2 pi = pts[i]; w = i == cur ? -1.0 : edge_weight(pc.x, pc.y, pi.x, pi.y, kind); }
            if (w != -1.0 && w < lo) { lo = w; arg = (u64)i; } // NOT_CONNECTED, utils.h:35
        }
        for (int off = 32; off > 0; off >>= 1) {
            double od = __shfl_xor(lo, off);
            u64 oa = __shfl_xor(arg, off);
            if (key_better(od, oa, lo, arg)) { lo = od; arg = oa; }
        }
        Partial *r = red[step & 1];
        if ((tid & 63) == 0) { r[tid >> 6].d = lo; r[tid >> 6].key = arg; }
        __syncthreads();
        lo = r[0].d; arg = r[0].key;
        for (int w = 1; w < nw; w++)
            if (key_better(r[w].d, r[w].key, lo, arg)) { lo = r[w].d; arg = r[w].key; }
        if (arg == KEY_NONE) break; // nothing reachable: heuristics.c:268-272 closes the path here
        const int nxt = (int)arg;
        if (nxt % BT == tid) { const int k = nxt / BT; if (k < 64) seen |= 1ull << k; else seen_hi |= 1ull << (k - 64); }
        if (tid == 0) { ord[step] = nxt; total += lo; }
        cur = nxt;
    }
    if (step < n) {
        // Some node has no admissible edge left (NOT_CONNECTED entries of a caller matrix): the reference closes
        // the path early (heuristics.c:266-272) and ends with an invalid tour, which tsp_update_best_solution
        // rejects.  Here the remaining cells take the unvisited nodes so that ord[] stays a permutation (no
        // kernel ever gathers through garbage) and status 1 makes the host fail the call.
        if (tid == 0) fill_pos = step;
        __syncthreads();
        for (int k = 0, i = tid; i < n; i += BT, k++)
            if (!((k < 64 ? seen >> k : seen_hi >> (k - 64)) & 1)) ord[atomicAdd(&fill_pos, 1)] = i;
    }
    if (tid == 0) {
        total += mat ? Elem<T>::widen(mat[(size_t)cur * ld + start]) : (double)cell<T>(mat, pts, kind, ld, cur, start); // heuristics.c:281
        S.cost[t] = total;
        S.status[t] = (step == n) ? 0 : 1; // 1: tour left incomplete
    }
}

// ---------------------------------------------------------------------------
// K6, matrix mode: the same tour with 16-byte row reads.  A thread owns V consecutive nodes
// per chunk (chunk c: nodes (c BT + tid) V ...), visited bits in a 128-bit register mask
// (n <= 16 BT V).  Integer cells: the candidate is ONE unsigned 64-bit key (weight << 32 |
// index), so the (weight, index) argmin -- ties to the lowest index, the strict < of
// heuristics.c:258 -- is a plain min through the wave shuffles and the LDS round.  One memory
// trip, one barrier per step: 2-3x the step rate of the strided kernel above, which stays for
// the matrix-free mode.
// ---------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(1024) k_nn_vec(Tours S, const T *__restrict__ mat, int n, int ld, int slot0,
                                                 const int *__restrict__ starts)
{
    typedef typename Elem<T>::vec VT;
    constexpr int V = Elem<T>::V;
    constexpr bool INT = !std::is_same<T, double>::value;
    __shared__ Partial red[2][16];
    __shared__ int fill_pos;
    const int t = slot0 + blockIdx.x;
    const int start = starts[blockIdx.x];
    int *ord = S.ord + (size_t)t * n;
    const int tid = threadIdx.x, BT = blockDim.x;
    const int nw = (BT + 63) >> 6;
    const int nvec = ld / V;
    const int nch = (nvec + BT - 1) / BT;          // <= 16 (host)
    u64 seen = 0, seen_hi = 0;                     // bit c*V+v <-> node (c*BT + tid)*V + v
    auto mark = [&](int node) __attribute__((always_inline)) {
        const int vi = node / V, c = vi / BT;
        if (vi - c * BT == tid) { const int k = c * V + node % V; if (k < 64) seen |= 1ull << k; else seen_hi |= 1ull << (k - 64); }
    };
    mark(start);
    int cur = start;
    double total = 0;
    if (tid == 0) ord[0] = start;
    int step = 1;
    for (; step < n; step++) {
        const VT *row = reinterpret_cast<const VT *>(mat + (size_t)cur * ld);
        double lo = DBL_MAX;
        u64 arg = KEY_NONE;      // INT: the packed key itself; doubles: the index
        for (int c = 0; c < nch; c++) {
            const int vi = c * BT + tid;
            if (vi >= nvec) break;
            const VT x = row[vi];
            const u64 bits = (c * V < 64 ? seen >> (c * V) : seen_hi >> (c * V - 64));
#pragma unroll
            for (int v = 0; v < V; v++) {
                const int i = vi * V + v;
                const bool free_ = i < n && !((bits >> v) & 1);
                if constexpr (INT) {
                    const unsigned raw = (unsigned)x[v];
                    const bool conn = sizeof(T) == 2 ? raw != 0xFFFFu : (int)raw != -1;   // NOT_CONNECTED, utils.h:35
                    const u64 key = ((u64)raw << 32) | (unsigned)i;
                    arg = (free_ && conn && key < arg) ? key : arg;
                } else {
                    const double w = x[v];
                    if (free_ && w != -1.0 && w < lo) { lo = w; arg = (u64)i; }
                }
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            if constexpr (INT) {
                const u64 oa = __shfl_xor(arg, off);
                arg = oa < arg ? oa : arg;
            } else {
                double od = __shfl_xor(lo, off);
                u64 oa = __shfl_xor(arg, off);
                if (key_better(od, oa, lo, arg)) { lo = od; arg = oa; }
            }
        }
        Partial *r = red[step & 1];
        if ((tid & 63) == 0) { r[tid >> 6].d = lo; r[tid >> 6].key = arg; }
        __syncthreads();
        lo = r[0].d; arg = r[0].key;
        for (int w = 1; w < nw; w++) {
            if constexpr (INT) arg = r[w].key < arg ? r[w].key : arg;
            else if (key_better(r[w].d, r[w].key, lo, arg)) { lo = r[w].d; arg = r[w].key; }
        }
        if (arg == KEY_NONE) break; // nothing reachable: heuristics.c:268-272 closes the path here
        const int nxt = (int)(arg & 0xffffffffu);
        if constexpr (INT) lo = (double)(unsigned)(arg >> 32);
        mark(nxt);
        if (tid == 0) { ord[step] = nxt; total += lo; }
        cur = nxt;
    }
    if (step < n) {   // incomplete tour: see k_nn
        if (tid == 0) fill_pos = step;
        __syncthreads();
        for (int c = 0; c < nch; c++) {
            const int vi = c * BT + tid;
            const u64 bits = (c * V < 64 ? seen >> (c * V) : seen_hi >> (c * V - 64));
            for (int v = 0; v < V; v++) {
                const int i = vi * V + v;
                if (vi < nvec && i < n && !((bits >> v) & 1)) ord[atomicAdd(&fill_pos, 1)] = i;
            }
        }
    }
    if (tid == 0) {
        total += Elem<T>::widen(mat[(size_t)cur * ld + start]); // heuristics.c:281
        S.cost[t] = total;
        S.status[t] = (step == n) ? 0 : 1; // 1: tour left incomplete
    }
}

// ---------------------------------------------------------------------------
// K6, third form: nearest-neighbour tour from the COORDINATES through a uniform grid -- for every
// instance whose weights come from its points (EUC_2D / ATT / CEIL_2D, matrix or matrix-free).  The
// matrix kernels above pay one dependent row fetch + one workgroup barrier per step (1.6 us at n = 4096,
// 3.2 us at 16 384: SURVEY 8f rank 1, the seed tour had become 40 % of a single search); here a step is
// a handful of LDS reads and ~100 vector instructions in ONE wave, no barrier, no matrix traffic.
//
// Exactness.  Every weight kind is a monotone function of the squared distance as the kernels compute it
// (conversion, root, rounding are all monotone), so the reference's pick -- min over unvisited i of
// c[cur][i], strict <, i ascending (heuristics.c:253-263) = min of the key (weight << 32 | i) -- lies
// among the points closer than (best weight so far) + rounding.  The points are bucketed into G x G cells
// (host, tspgpu_set_points; cells row-major, points sorted by cell, so the cells cx-R..cx+R of one grid row
// are ONE contiguous range of sorted positions).  A step examines the (2R+1)^2 cells around the current
// node, R = 2 first, with the exact weight (edge_w: the arithmetic of k_build_costs); every point
// outside is at least R cells away, so once weight(R * cell - eps) > best the pick is final; else the
// square grows (only its new frame is examined).  The last 256 unvisited nodes move into registers
// (4 per lane): the end of an NN walk, where the nearest unvisited node is far away, costs no expansion.
// ---------------------------------------------------------------------------
struct GridArgs {
    Tours S;
    int n, slot0;
    const int *starts;
    const double2 *gxy;      // [n] points, sorted by cell
    const int *gidx;         // [n] sorted position -> node
    const int *gcell;        // [n] sorted position -> cell (cx | cy << 16)
    const int *gpos;         // [n] node -> sorted position
    const int *cstart;       // [G*G + 1] first sorted position of every cell
    int G;
    double cell, eps;
    const unsigned *knn;     // [n][NN_K] nearest neighbours of every point (k_knn_build), nullptr: none
};

constexpr int NN_K = 3;      // list length: the next node of an NN walk is among the 3 nearest in 83 % of the steps (n = 4096)

constexpr int NN_TAIL = 256;

// LDS_PTS / LDS_CS: points + node ids + cells / cell starts staged in LDS -- compile-time, so that every access is a
// ds_read with a 32-bit address (a run-time choice of pointer turns them all into flat loads).  KEY32: weights below
// 2^15 and n <= 2^17, the candidate key (weight, node) is ONE 32-bit word and a reduction step one v_min_u32.
// KNN: the NN_K nearest neighbours of every point by (weight, node), certified complete (weight below the bound of the
// first square; k_knn_build), sit in LDS: the first unvisited one IS the nearest unvisited node -- two LDS trips and a
// ballot instead of the candidate scan; the scan runs only when all of them are visited (17 % of the steps at n = 4096).
// KNN = 1: lists in LDS (single tours), 2: read from global memory (batches: one wave per start, the 12 n bytes stay in L1 / L2).
template <int KIND, bool LDS_PTS, bool LDS_CS, bool KEY32, int KNN = 0>
__global__ void __launch_bounds__(64) k_nn_grid(GridArgs A)
{
    // (the list entries are 32-bit -- weight < 2^15 | sorted position -- whatever the key of the candidate scan: a weight that
    // does not fit is simply not listed, k_knn_build)
    static_assert(KNN != 1 || KEY32, "lists in LDS: the 32-bit-key form only");
    static_assert(KNN != 1 || LDS_PTS, "lists in LDS ride on the LDS-resident form");
    typedef typename std::conditional<KEY32, unsigned, u64>::type K;
    constexpr K NONE = (K)~(K)0;
    constexpr int WSH = KEY32 ? 17 : 32;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int n = A.n, G = A.G, lane = threadIdx.x;
    const int t = A.slot0 + blockIdx.x;
    const int start = A.starts[blockIdx.x];
    int *ord = A.S.ord + (size_t)t * n;
    // LDS: visited bits | tail list | (cell starts) | (points, node ids, cells)
    const int nwords = (n + 31) >> 5;
    unsigned *vis = reinterpret_cast<unsigned *>(smem);
    int *tail = reinterpret_cast<int *>(vis + ((nwords + 3) & ~3));
    int *cs_l = tail + NN_TAIL;
    const int ncs = G * G + 1;
    double2 *pts_l = reinterpret_cast<double2 *>(cs_l + (LDS_CS ? ((ncs + 3) & ~3) : 0));
    int *idx_l = reinterpret_cast<int *>(pts_l + (LDS_PTS ? n : 0));
    int *cell_l = idx_l + (LDS_PTS ? n : 0);
    unsigned *knn_l = reinterpret_cast<unsigned *>(cell_l + (LDS_PTS ? n : 0));
    if constexpr (KNN == 1) for (int i = lane; i < n * NN_K; i += 64) knn_l[i] = A.knn[i];
    for (int w = lane; w < nwords; w += 64) vis[w] = 0;
    if constexpr (LDS_CS) for (int i = lane; i < ncs; i += 64) cs_l[i] = A.cstart[i];
    if constexpr (LDS_PTS) for (int i = lane; i < n; i += 64) { pts_l[i] = A.gxy[i]; idx_l[i] = A.gidx[i]; cell_l[i] = A.gcell[i]; }
    __syncthreads();
    auto cstart = [&](int i) __attribute__((always_inline)) { if constexpr (LDS_CS) return cs_l[i]; else return A.cstart[i]; };
    auto pts = [&](int i) __attribute__((always_inline)) { if constexpr (LDS_PTS) return pts_l[i]; else return A.gxy[i]; };
    auto gidx = [&](int i) __attribute__((always_inline)) { if constexpr (LDS_PTS) return idx_l[i]; else return A.gidx[i]; };
    auto gcell = [&](int i) __attribute__((always_inline)) { if constexpr (LDS_PTS) return cell_l[i]; else return A.gcell[i]; };

    int cur = A.gpos[start];                       // sorted position of the current node (wave-uniform)
    double2 P = A.gxy[cur];                        // its coordinates (wave-uniform)
    int ccell = A.gcell[cur];                      // its cell
    const double2 P0 = P;
    if (lane == 0) { ord[0] = start; vis[cur >> 5] |= 1u << (cur & 31); }
    __syncthreads();
    double total = 0;
    int step = 1;
    const int grid_steps = n - 1 > NN_TAIL ? n - 1 - NN_TAIL : 0;     // steps taken through the grid

    // wave-wide minimum of a key through DPP (no LDS crossbar: a ds_bpermute butterfly costs more than the whole
    // candidate scan): quad swaps and the two mirrors leave every 16-lane row with its minimum, row_bcast15 /
    // row_bcast31 carry it across the rows, lane 63 ends with the wave's
    auto wave_min = [&](K k) __attribute__((always_inline)) {
        auto stepmin = [&](auto ctrl_tag, auto rows_tag) __attribute__((always_inline)) {
            constexpr int CTRL = decltype(ctrl_tag)::value, ROWS = decltype(rows_tag)::value;
            if constexpr (KEY32) {
                const unsigned o = (unsigned)__builtin_amdgcn_update_dpp((int)k, (int)k, CTRL, ROWS, 0xf, false);
                k = o < k ? o : k;
            } else {
                const unsigned lo = (unsigned)k, hi = (unsigned)(k >> 32);
                const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp((int)lo, (int)lo, CTRL, ROWS, 0xf, false);
                const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp((int)hi, (int)hi, CTRL, ROWS, 0xf, false);
                const u64 o = ((u64)ohi << 32) | olo;
                k = o < k ? o : k;
            }
        };
        typedef std::integral_constant<int, 0xf> ALL;
        stepmin(std::integral_constant<int, 0xB1>{}, ALL{});      // quad_perm [1,0,3,2]
        stepmin(std::integral_constant<int, 0x4E>{}, ALL{});      // quad_perm [2,3,0,1]
        stepmin(std::integral_constant<int, 0x141>{}, ALL{});     // row_half_mirror
        stepmin(std::integral_constant<int, 0x140>{}, ALL{});     // row_mirror
        stepmin(std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xA>{});   // row_bcast15 -> rows 1, 3
        stepmin(std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xC>{});   // row_bcast31 -> rows 2, 3
        if constexpr (KEY32) return (K)(unsigned)__builtin_amdgcn_readlane((int)k, 63);
        else {
            const unsigned rlo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)k, 63);
            const unsigned rhi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(k >> 32), 63);
            return (K)(((u64)rhi << 32) | rlo);
        }
    };
    auto lane_f64 = [&](double x, int src) __attribute__((always_inline)) {      // x of lane `src` (wave-uniform) to all
        const long long b = __double_as_longlong(x);
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, src);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((u64)b >> 32), src);
        return __longlong_as_double((long long)(((u64)hi << 32) | lo));
    };
    auto make_key = [&](int w, unsigned id) __attribute__((always_inline)) { return (K)(((K)(unsigned)w << WSH) | (K)id); };
    auto key_w = [&](K k) __attribute__((always_inline)) { return (unsigned)(k >> WSH); };
    auto key_id = [&](K k) __attribute__((always_inline)) { return (int)(KEY32 ? (unsigned)k & 0x1ffffu : (unsigned)k); };

    // a single wave: LDS operations of one wave complete in order, so lane 0's update of the visited bits (a ds_or
    // without return: no read trip) needs neither a barrier nor a wait before the next step reads them -- only the
    // compiler must not move LDS accesses across it (__syncthreads() would also wait for the global store of
    // ord[step], a full memory round trip per step; an s_waitcnt lgkmcnt(0) for the LDS write: 0.05 us per step)
#define NN_WAVE_SYNC() asm volatile("" ::: "memory")
    const unsigned wlb2 = (unsigned)edge_w<KIND>(0.0, 0.0, fmax(0.0, 2.0 * A.cell - A.eps), 0.0);   // weight bound of the first square
    const int jl5 = lane / 12, k5 = lane - jl5 * 12;          // first square: 5 grid rows x 12 lanes

    bool pvalid = true;                             // P / ccell are those of `cur` (a list hit moves on without them)
    for (; step <= grid_steps; step++) {
        if constexpr (KNN) {
            const unsigned e = lane < NN_K ? (KNN == 1 ? knn_l[cur * NN_K + lane] : A.knn[(size_t)cur * NN_K + lane]) : ~0u;   // (weight << 17 | sorted position), ascending by (weight, node)
            const unsigned q = e & 0x1ffffu;
            const bool unv = e != ~0u && !((vis[min(q, (unsigned)n - 1) >> 5] >> (q & 31)) & 1u);
            const unsigned long long bal = __ballot(unv);
            if (bal) {
                const int src = __ffsll(bal) - 1;
                const unsigned we = (unsigned)__builtin_amdgcn_readlane((int)e, src);
                cur = (int)(we & 0x1ffffu);
                total += (double)(we >> 17);
                pvalid = false;
                if (lane == 0) { ord[step] = gidx(cur); __hip_atomic_fetch_or(&vis[cur >> 5], 1u << (cur & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
                NN_WAVE_SYNC();
                continue;
            }
            if (!pvalid) { P = pts(cur); ccell = __builtin_amdgcn_readfirstlane(gcell(cur)); pvalid = true; }
        }
        const int cx = ccell & 0xffff, cy = ccell >> 16;
        K best = NONE;                              // lane's best candidate: (weight, node) ...
        int bestp = 0;                              // ... and its sorted position
        // candidate at sorted position p, taken when `ok` (loads first, branch-free: a visited point just loses)
        auto cand = [&](int p, bool ok) __attribute__((always_inline)) {
            const unsigned vw = vis[p >> 5];
            const double2 Q = pts(p);
            const unsigned id = (unsigned)gidx(p);
            K key = make_key(edge_w<KIND>(P.x, P.y, Q.x, Q.y), id);
            key = (!ok || ((vw >> (p & 31)) & 1u)) ? NONE : key;
            if (key < best) { best = key; bestp = p; }
        };
        // first square, R = 2 (almost always the only one): one contiguous range of sorted positions per grid row,
        // two candidates per lane in straight-line code (their chains interleave), the rest of a long range in a loop
        {
            const int y = cy - 2 + jl5;
            const bool row = jl5 < 5 && y >= 0 && y < G;
            const int rowbase = row ? y * G : 0;
            const int s1 = cstart(rowbase + max(0, cx - 2)), e1 = row ? cstart(rowbase + min(G - 1, cx + 2) + 1) : 0;
            const int p0 = s1 + k5, p1 = p0 + 12;
            cand(min(p0, n - 1), p0 < e1);
            cand(min(p1, n - 1), p1 < e1);
            if (__ballot(p1 + 12 < e1))
                for (int p = p1 + 12; p < e1; p += 12) cand(p, true);
        }
        K win = wave_min(best);
        const bool whole2 = cx - 2 <= 0 && cy - 2 <= 0 && cx + 2 >= G - 1 && cy + 2 >= G - 1;
        if (!whole2 && (win == NONE || wlb2 <= key_w(win))) {
            int Rin = 2, R = 4;                     // cells within Rin of (cx, cy) are done
            for (;;) {
                const int ylo = max(0, cy - R), yhi = min(G - 1, cy + R);
                const int xlo = max(0, cx - R), xhi = min(G - 1, cx + R);
                const int nrows = yhi - ylo + 1;
                const int L = nrows >= 64 ? 1 : 64 / nrows;           // lanes per grid row
                const int rpp = 64 / L;                               // grid rows per pass
                for (int r0 = 0; r0 < nrows; r0 += rpp) {
                    const int jl = lane / L, k = lane - jl * L, j = r0 + jl;
                    if (jl < rpp && j < nrows) {
                        const int y = ylo + j;
                        const int rowbase = y * G;
                        // new cells of this row: the whole span outside the inner square's rows, its two flanks inside
                        const bool inner = y >= cy - Rin && y <= cy + Rin;
                        const int s1 = cstart(rowbase + xlo);
                        int e1, s2 = 0, e2 = 0;
                        if (!inner) e1 = cstart(rowbase + xhi + 1);
                        else {
                            const int ixlo = max(0, cx - Rin), ixhi = min(G - 1, cx + Rin);
                            e1 = cstart(rowbase + ixlo);
                            s2 = cstart(rowbase + ixhi + 1); e2 = cstart(rowbase + xhi + 1);
                        }
                        for (int p = s1 + k; p < e1; p += L) cand(p, true);
                        for (int p = s2 + k; p < e2; p += L) cand(p, true);
                    }
                }
                win = wave_min(best);
                const bool whole = xlo == 0 && ylo == 0 && xhi == G - 1 && yhi == G - 1;
                if (win != NONE) {
                    // every point not examined yet is at least R cells away from the current node
                    const double lb = fmax(0.0, (double)R * A.cell - A.eps);
                    if (whole || (unsigned)edge_w<KIND>(0.0, 0.0, lb, 0.0) > key_w(win)) break;
                } else if (whole) break;                              // (cannot happen: unvisited nodes remain)
                Rin = R;
                R += max(2, R >> 1);
            }
        }
        // the lane that holds the winner (node ids are unique) hands over its sorted position; coordinates and cell of
        // the new current node come from there (LDS: a uniform read; global arrays: the winner's lane loads them)
        const int src = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)__ballot(best == win)) - 1);
        cur = __builtin_amdgcn_readlane(bestp, src);
        if constexpr (LDS_PTS) { P = pts(cur); ccell = __builtin_amdgcn_readfirstlane(gcell(cur)); }
        else {
            const double2 Q = A.gxy[bestp];                           // (every lane loads its own best: in flight together)
            const int qc = A.gcell[bestp];
            P.x = lane_f64(Q.x, src); P.y = lane_f64(Q.y, src); ccell = __builtin_amdgcn_readlane(qc, src);
        }
        total += (double)key_w(win);
        if (lane == 0) { ord[step] = key_id(win); __hip_atomic_fetch_or(&vis[cur >> 5], 1u << (cur & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
        NN_WAVE_SYNC();
    }
#undef NN_WAVE_SYNC

    if constexpr (KNN) { if (!pvalid) P = pts(cur); }
    // ---- the last <= NN_TAIL unvisited nodes: in registers, four per lane
    {
        const int remaining = n - step;
        // compact list of the unvisited sorted positions (ascending), by a wave prefix sum over the visited words
        int cntl = 0;
        const int wpl = (nwords + 63) / 64;                        // words per lane (contiguous block)
        const int w0 = min(nwords, lane * wpl), w1 = min(nwords, w0 + wpl);
        for (int w = w0; w < w1; w++) {
            unsigned f = ~vis[w];
            if (w == nwords - 1 && (n & 31)) f &= (1u << (n & 31)) - 1u;
            cntl += __popc(f);
        }
        int pre = cntl;
        for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(pre, off); if (lane >= off) pre += o; }
        int at = pre - cntl;
        for (int w = w0; w < w1; w++) {
            unsigned f = ~vis[w];
            if (w == nwords - 1 && (n & 31)) f &= (1u << (n & 31)) - 1u;
            while (f) { const int b = __ffs(f) - 1; f &= f - 1; if (at < NN_TAIL) tail[at] = w * 32 + b; at++; }
        }
        __syncthreads();
        constexpr int U = NN_TAIL / 64;
        double2 Q[U];
        int qid[U];
        unsigned alive = 0;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int e = u * 64 + lane;
            Q[u] = make_double2(0, 0); qid[u] = -1;
            if (e < remaining) { const int p = tail[e]; Q[u] = A.gxy[p]; qid[u] = A.gidx[p]; alive |= 1u << u; }
        }
        for (; step < n; step++) {
            K best = NONE;
#pragma unroll
            for (int u = 0; u < U; u++) {
                const K key = make_key(edge_w<KIND>(P.x, P.y, Q[u].x, Q[u].y), (unsigned)qid[u]);
                best = (((alive >> u) & 1u) && key < best) ? key : best;
            }
            const K win = wave_min(best);
            const int nxt = key_id(win);
            total += (double)key_w(win);
            double px = 0, py = 0;
#pragma unroll
            for (int u = 0; u < U; u++)
                if (((alive >> u) & 1u) && qid[u] == nxt) { alive &= ~(1u << u); px = Q[u].x; py = Q[u].y; }
            const int src = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)__ballot(best == win)) - 1);
            P.x = lane_f64(px, src); P.y = lane_f64(py, src);
            if (lane == 0) ord[step] = nxt;
        }
        if (lane == 0) {
            total += (double)edge_w<KIND>(P.x, P.y, P0.x, P0.y);      // closing edge, heuristics.c:281
            A.S.cost[t] = total;
            A.S.status[t] = 0;
        }
    }
}

// The NN_K nearest neighbours of every point, by (weight, node) as heuristics.c:253-263 orders them, from the first square
// of the grid (cells within 2 of the point's): entry j = (weight << 17 | sorted position), ~0 where the list cannot be
// certified -- a weight not below the bound of everything outside the square (the bound k_nn_grid expands on).  Every
// point that is not in the list has a larger (weight, node) than every certified entry, so the first unvisited certified
// entry of the current node is the nearest unvisited node.  One thread per point; built once per instance.
template <int KIND>
__global__ void __launch_bounds__(256) k_knn_build(GridArgs A, unsigned *__restrict__ out)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int n = A.n, G = A.G;
    if (p >= n) return;
    const double2 P = A.gxy[p];
    const int cc = A.gcell[p], cx = cc & 0xffff, cy = cc >> 16;
    u64 best[NN_K];                                 // (weight << 34 | node << 17 | sorted position), ascending
#pragma unroll
    for (int j = 0; j < NN_K; j++) best[j] = ~0ull;
    for (int y = max(0, cy - 2); y <= min(G - 1, cy + 2); y++) {
        const int s1 = A.cstart[y * G + max(0, cx - 2)], e1 = A.cstart[y * G + min(G - 1, cx + 2) + 1];
        for (int q = s1; q < e1; q++) {
            if (q == p) continue;
            const double2 Q = A.gxy[q];
            u64 key = ((u64)(unsigned)edge_w<KIND>(P.x, P.y, Q.x, Q.y) << 34) | ((u64)(unsigned)A.gidx[q] << 17) | (unsigned)q;
#pragma unroll
            for (int j = 0; j < NN_K; j++) { if (key < best[j]) { const u64 t = best[j]; best[j] = key; key = t; } }
        }
    }
    const bool whole2 = cx - 2 <= 0 && cy - 2 <= 0 && cx + 2 >= G - 1 && cy + 2 >= G - 1;
    const unsigned wlb2 = (unsigned)edge_w<KIND>(0.0, 0.0, fmax(0.0, 2.0 * A.cell - A.eps), 0.0);
#pragma unroll
    for (int j = 0; j < NN_K; j++) {
        const unsigned w = (unsigned)(best[j] >> 34);
        const bool ok = best[j] != ~0ull && (whole2 || w < wlb2) && w < 32767u;
        out[(size_t)p * NN_K + j] = ok ? (w << 17) | (unsigned)(best[j] & 0x1ffffu) : ~0u;
    }
}

// ---------------------------------------------------------------------------
// sweep arguments
// ---------------------------------------------------------------------------
struct SweepArgs {
    Tours S;
    const void *mat;
    int n, ld, slot0, P;     // P = array positions (tour edges) per workgroup
    int g0;                  // first workgroup (run) of this launch: > 0 only when a sweep is sharded over ranks
    int tabu_lds;            // TABU: byte offset in the dynamic LDS of the per-node tabu bytes (n + 32 of them)
    int symmetric;
    int ablate;              // diagnostics only: 1 = no pair evaluation, 2 = no row traffic (results are wrong)
    unsigned long long *stamps; // diagnostics only: 64 wall-clock stamps (10 ns ticks) per workgroup, or null
    const double2 *pts;      // matrix-free mode: node coordinates, and
    const double2 *spts;     //   spts[b] = coordinates of succ b (gathered once per sweep)
    const int2 *ipts;        // k_sweep_otf8<KIND_CEIL_INT>: the coordinates as integers (offset to the bounding box's corner),
    const int2 *ispts;       //   and those of succ b
    int kind;                //   edge-weight kind
    const int *tabu_list;    // TABU only
    const TabuState *tabu;   // TABU only
    Fused F;                 // fused path only
    int parity;              //   this launch writes F.*[parity], reads F.*[1 - parity]
    HistBuf hist;            //   slot 0 move history
};

// acceptance rule for the pair {a,b} seen from a's workgroup.  Symmetric
// matrices: each unordered pair is owned by exactly one of its two workgroups
// (the one from which the other node is at most half way round the INDEX
// circle), which balances the triangular loop of refinment.c:49-50 perfectly.
// Otherwise only the reference's own orientation b > a is evaluated.
__device__ __forceinline__ bool pair_owned(int a, int b, int n, int symmetric)
{
    if (!symmetric) return b > a;
    int k = b - a;
    if (k < 0) k += n;
    const int k2 = 2 * k;
    return k2 < n || (k2 == n && a < b);
}

template <typename DT>
__device__ __forceinline__ void consider(DT delta, int a, int b, DT &best_d, u64 &best_key)
{
    if (delta <= best_d) {
        const u64 key = a < b ? ((u64)(unsigned)a << 32) | (unsigned)b : ((u64)(unsigned)b << 32) | (unsigned)a;
        if (delta < best_d || key < best_key) { best_d = delta; best_key = key; }
    }
}

__device__ __forceinline__ bool is_tabu(const int *tl, int node, int iter, int tenure)
{
    const int s = tl[node];
    return iter - s < tenure && s != -1; // metaheuristic.c:416-418
}

// ---------------------------------------------------------------------------
// K2/K3 "simple" sweep: one LDS row.  Workgroup g walks array positions
// [g*P, (g+1)*P); each position p is one tour edge (a, sa) = (ord[p], ord[p+1])
// (or the reverse when dir < 0).  Row sa is staged in LDS (gather target
// c[sa][sb]); row a is read coalesced from global; pos/ord/dpos come from L2.
// Used when three rows do not fit in LDS, and as an independent cross-check of
// the pipelined kernel.
// ---------------------------------------------------------------------------
template <typename T, bool TABU>
__global__ void __launch_bounds__(1024) k_sweep_simple(SweepArgs A)
{
    typedef typename Elem<T>::vec VT;
    constexpr int V = Elem<T>::V;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int n = A.n, ld = A.ld;
    const int t = A.slot0 + blockIdx.y;
    if (A.S.done[t]) return;
    const int tid = threadIdx.x, BT = blockDim.x;
    T *rowS = reinterpret_cast<T *>(smem);
    Partial *scratch = reinterpret_cast<Partial *>(smem + (size_t)ld * sizeof(T));
    const T *mat = static_cast<const T *>(A.mat);
    const int *ord = A.S.ord + (size_t)t * n;
    typedef typename Elem<T>::acc AT;
    const int *succ = A.S.succ + (size_t)t * n;
    const AT *dnb = dnb_of<AT>(A.S, t, n);
    const int dir = A.S.dir[t];

    int iter = 0, tenure = 0;
    if constexpr (TABU) { iter = A.tabu->iter; tenure = A.tabu->tenure; }

    AT best_d = TABU ? Elem<T>::lim() : (AT)0;
    u64 best_key = TABU ? KEY_NONE : 0; // key 0 cannot be beaten on a tie: "no move" is (0, 0)

    const int p0 = ((int)blockIdx.x + A.g0) * A.P;
    const int cnt = min(A.P, n - p0);
    for (int s = 0; s < cnt; s++) {
        const int p = p0 + s, p1 = p + 1 == n ? 0 : p + 1;
        const int a = dir > 0 ? ord[p] : ord[p1];
        const int sa = dir > 0 ? ord[p1] : ord[p];
        __syncthreads();
        {
            const VT *src = reinterpret_cast<const VT *>(mat + (size_t)sa * ld);
            VT *dst = reinterpret_cast<VT *>(rowS);
            for (int i = tid; i < ld / V; i += BT) dst[i] = src[i];
        }
        __syncthreads();
        if constexpr (TABU) {
            if (is_tabu(A.tabu_list, a, iter, tenure) || is_tabu(A.tabu_list, sa, iter, tenure)) continue;
        }
        const AT d_a = dnb[a];
        const T *rowA = mat + (size_t)a * ld;
        const int kmax = A.symmetric ? n / 2 : n - 1 - a;
        for (int k = 1 + tid; k <= kmax; k += BT) {
            int b = a + k;
            if (b >= n) b -= n;
            const int sb = succ[b];
            if (b == sa || sb == a) continue;          // refinment.c:55
            if (!pair_owned(a, b, n, A.symmetric)) continue;
            if constexpr (TABU) {
                if (is_tabu(A.tabu_list, b, iter, tenure) || is_tabu(A.tabu_list, sb, iter, tenure)) continue;
            }
            const AT made = (AT)rowA[b] + (AT)rowS[sb];              // c[a][b] + c[sa][sb]
            const AT kept = d_a + dnb[b];                            // c[a][sa] + c[b][sb]
            consider<AT>(made - kept, a, b, best_d, best_key);
        }
    }
    double d = (double)best_d;
    u64 key = best_key;
    __syncthreads();
    block_argmin(d, key, scratch);
    if (tid == 0) {
        Partial o; o.d = d; o.key = key;
        A.S.partial[(size_t)t * A.S.pstride + blockIdx.x + A.g0] = o;
    }
}

// ---------------------------------------------------------------------------
// Shared by the LDS sweeps (pipelined, resident, fused): per-thread state of the owned b's and
// the evaluation of one step (one tour edge (a, succ a) against the thread's b's).
//
// State.  A thread keeps the same V = 16 / sizeof(cell) node indices b per chunk for the whole
// kernel: the LDS byte offset of succ b and c[b][succ b] live in registers.  uint16 cells: both
// share ONE register per b, low / high half (the halves are SDWA operands, unpacking is free).
// No poison value exists then: tabu b's are a bit mask and pad lanes only ever meet the masked
// variant.  Other cells: two registers; a b that can never be part of a move from this thread
// (pad lane, tabu) gets c[b][succ b] = -BIG, which drives its deltas far above any real one.
//
// Which orientation of a pair evaluates it (both meet in LDS).  Symmetric matrix, plain 2-opt:
// by BLOCKS of 64 V node indices (= what one wave holds in one chunk).  Pair {a, b} in different
// blocks belongs to the orientation whose b block lies less than half way round the block
// circle ahead of a's block (exactly half way: to the lower block); inside a's own block to
// b > a.  So a wave is either wholly in, wholly out, or the one wave holding a's block -- no
// wave straddles a range boundary, and the b's of the two neighbours of a need no mask at all:
// their delta is exactly 0 (c[a][pa] + c[sa][a] - (c[a][sa] + c[pa][a]); IEEE addition
// commutes), never an improvement.  Tabu (every admissible pair counts, a zero delta can be the
// best one) keeps the blocks and masks the two neighbours per lane in the waves that hold them.
// Caller matrix not symmetric: the reference's own orientation b > a as the cyclic index range
// [lo, lo+len-1], masked per lane wherever a wave straddles its ends or holds one of the three
// nodes around a (refinment.c:55: b == a, b == succ a, succ b == a).
//
// Argmin.  The reference keeps the first strictly smaller delta in (a asc, b asc) order, i.e.
// it minimises (delta, min(a,b), max(a,b)).  Integer deltas (n <= 65536): ONE signed 64-bit word,
// delta in the high half, so "better" is a single compare and ties need no special path.
// uint16 cells go one step further: for a fixed a the labels of a thread's consecutive b's
// ascend with the slot number v, so per pair a 32-bit (delta << 3 | v) and ONE v_min suffice;
// c[a][succ a] (uniform) comes off after the min and the 64-bit key is built once per chunk,
// for the winner.  Doubles keep (delta, a, b) and a wave-uniform tie branch; operation order
// made = c[a][b] + c[sa][sb]; kept = c[a][sa] + c[b][sb]; made - kept (refinment.c:58-60).
// ---------------------------------------------------------------------------
template <typename T, int NCH> struct BState {
    typedef typename Elem<T>::acc AT;
    static constexpr int V = Elem<T>::V;
    static constexpr bool PKS = sizeof(T) == 2;
    int sb[NCH][V];                               // LDS byte offset of succ b (| c[b][succ b] << 16 when packed)
    AT dn[PKS ? 1 : NCH][PKS ? 1 : V];            // c[b][succ b]
    unsigned skm;                                 // packed + tabu: b's that take no part
};

template <typename T, int NCH>
__device__ __forceinline__ void bstate_set(BState<T, NCH> &B, int c, int v, int succ_b, typename Elem<T>::acc dn, bool skip, bool tabu)
{
    if constexpr (BState<T, NCH>::PKS) {
        B.sb[c][v] = (succ_b * (int)sizeof(T)) | ((int)dn << 16);
        if (tabu && skip) B.skm |= 1u << (c * BState<T, NCH>::V + v);
    } else {
        B.sb[c][v] = succ_b * (int)sizeof(T);
        B.dn[c][v] = skip ? -Elem<T>::big() : dn;   // kept = c[a][sa] + dn  ->  delta = made - kept ~ +BIG
    }
}

// Per-b state of the pipelined / resident sweeps from the node-indexed view (succ, c[b][succ b]:
// coalesced 16-byte loads), followed by ONE workgroup barrier.  Tabu: whether b or succ b is
// tabu decides if b takes part at all; the stamps of the own b's are a coalesced read, and every
// thread publishes its b's verdicts as bytes in LDS (behind the rows, A.tabu_lds bytes into the
// dynamic LDS) so that the test of succ b is an LDS byte read after the barrier instead of a
// random global gather per b.
template <typename T, int NCH, bool TABU>
__device__ __forceinline__ void load_bstate(BState<T, NCH> &B, const SweepArgs &A, unsigned char *smem, int t, int iter, int tenure)
{
    typedef typename Elem<T>::acc AT;
    constexpr int V = Elem<T>::V;
    const int n = A.n, ld = A.ld;
    const int tid = threadIdx.x, BT = blockDim.x;
    const int *succ = A.S.succ + (size_t)t * n;
    const AT *dnb = dnb_of<AT>(A.S, t, n);
    int sv[NCH][V];
    AT dv[NCH][V];
    unsigned char *tb = smem + A.tabu_lds;
    unsigned own = 0;                                   // tabu: bit c*V+v = own b is tabu
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const int b0 = min((c * BT + tid) * V, ld - V);   // lanes past the row: masked
        load_run<V>(succ + b0, sv[c]);
        load_run<V>(dnb + b0, dv[c]);
        if constexpr (TABU) {
            int st[V];
            load_run<V>(A.tabu_list + b0, st);
            unsigned char flag[V];
#pragma unroll
            for (int v = 0; v < V; v++) {
                const bool tb_v = iter - st[v] < tenure && st[v] != -1;   // metaheuristic.c:416-418
                flag[v] = tb_v ? 1 : 0;
                if (tb_v && (c * BT + tid) * V == b0) own |= 1u << (c * V + v);
            }
            if ((c * BT + tid) * V == b0) __builtin_memcpy(tb + b0, flag, V);   // V bytes, one store
        }
    }
    __syncthreads(); // nodes[] (and the tabu bytes) visible
#pragma unroll
    for (int c = 0; c < NCH; c++) {
#pragma unroll
        for (int v = 0; v < V; v++) {
            const int b = (c * BT + tid) * V + v;
            const int sb = b < n ? sv[c][v] : 0;
            bool sk = b >= n;
            if constexpr (TABU)
                if (b < n) sk = ((own >> (c * V + v)) & 1u) || tb[sb] != 0;
            bstate_set<T, NCH>(B, c, v, sb, dv[c][v], sk, TABU);
        }
    }
}

struct Best {
    long long k;          // packed key (integer deltas)
    double d;             // doubles: (d, a, b, have)
    int a, b;
    bool have;
};

template <bool TABU>
__device__ __forceinline__ void best_init(Best &q)
{
    q.k = TABU ? (long long)(((u64)0x7fffffffu << 32) | 0xffffffffu) : 0ll;   // (lim, none) / (0, no move)
    q.d = TABU ? DBL_MAX : 0.0;
    q.a = 0; q.b = 0; q.have = false;                                           // (0,0): "no move"; cannot win a tie
}

constexpr int TABU_NODE = 1 << 30, NODE_MASK = TABU_NODE - 1;   // nodes[] entries of the tabu kernels carry the node's tabu bit
constexpr int MASKED32 = 1 << 27;   // masked pair on the 32-bit key path: (x << 3) must not overflow

// bA: LDS row of a; bS: LDS row of succ a (ldsS: its LDS byte address).
// BLOCKS: block ownership (symmetric matrix, plain 2-opt); else the index range (symmetric or not).
// areg != nullptr (symmetric matrices only): the row of a comes from the REGISTERS that loaded it -- a thread's own
// b's of chunk c are exactly the vector it fetched for chunk c of that row -- and c[a][succ a] = c[succ a][a] from the
// LDS row of succ a; bA is not touched.
template <typename T, int NCH, bool TABU, bool BLOCKS>
__device__ __forceinline__ void sweep_step_as(Best &q, const BState<T, NCH> &B, const T *bA, const unsigned char *bS, unsigned ldsS,
                                              int a, int am, int sa, int n, int ld, int BT, int tid, int wave_base, bool symmetric,
                                              const typename Elem<T>::vec *areg = nullptr)
{
    typedef typename Elem<T>::vec VT;
    typedef typename Elem<T>::acc AT;
    constexpr int V = Elem<T>::V;
    constexpr bool PKS = sizeof(T) == 2;
    constexpr bool PACKED = std::is_same<AT, int>::value;
    const AT BIG = Elem<T>::big();
    const AT d_a = areg ? (AT)reinterpret_cast<const T *>(bS)[a] : (AT)bA[sa]; // c[a][succ a]
    constexpr bool blocks = BLOCKS;
    const int NB = (n + 64 * V - 1) / (64 * V);
    const int blka = a / (64 * V);
    const int lo = a + 1 == n ? 0 : a + 1;
    const int len = symmetric ? ((n & 1) ? (n - 1) / 2 : (a < n / 2 ? n / 2 : n / 2 - 1)) : n - 1 - a;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const int w0 = (c * BT + wave_base) * V;        // this wave's first b in chunk c (scalar)
        if (w0 >= n) continue;                          // pad wave
        bool clean, self = false;
        if (blocks) {
            const int blkb = w0 / (64 * V);
            int d = blkb - blka;
            if (d < 0) d += NB;
            self = d == 0;
            if (!self && !(2 * d < NB || (2 * d == NB && blka < blkb))) continue;   // the other orientation's
            // tabu: the two neighbours of a are real exclusions (a zero delta can be the best admissible one)
            const bool hit = TABU && ((unsigned)(am - w0) < (unsigned)(64 * V) || (unsigned)(sa - w0) < (unsigned)(64 * V));
            clean = !self && !hit && (!PKS || w0 + 64 * V <= n);   // packed state has no poison for pad lanes
        } else {
            int t0 = w0 - lo;
            if (t0 < 0) t0 += n;
            const bool nowrap = t0 + 64 * V <= n && w0 + 64 * V <= n;
            if (nowrap && t0 >= len) continue;              // wave entirely outside: wave-uniform skip
            clean = nowrap && t0 + 64 * V <= len && (unsigned)(am - w0) >= (unsigned)(64 * V) &&
                    (unsigned)(a - w0) >= (unsigned)(64 * V) && (unsigned)(sa - w0) >= (unsigned)(64 * V);
        }
        const int b0 = (c * BT + tid) * V;
        // all LDS reads of the chunk first (lanes past the row read its last vector), then the arithmetic
        const VT xa = areg ? areg[c] : *reinterpret_cast<const VT *>(bA + min(b0, ld - V));
        auto valid = [&](int b) __attribute__((always_inline)) {
            asm volatile("" : "+v"(b));     // b < n is step-invariant: hoisted, it costs an SGPR pair per b
            if (blocks) return ((b > a) | !self) & (b < n) & (!TABU | ((b != am) & (b != sa)));
            int tt = b - lo;
            tt += (tt >> 31) & n;
            return ((unsigned)tt < (unsigned)len) & (b != am) & (b != a) & (b != sa) & (b < n);
        };
        if constexpr (PKS) {
            int g[V];
#pragma unroll
            for (int v = 0; v < V; v++) {
                unsigned addr;
                asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0"
                    : "=v"(addr) : "v"(ldsS), "v"(B.sb[c][v]));
                g[v] = (int)*(const lds_u16 *)(uintptr_t)addr;
            }
            auto k32 = [&](auto check_tag) __attribute__((always_inline)) {
                constexpr bool CHECK = decltype(check_tag)::value;
                int m = 0x7fffffff;
#pragma unroll
                for (int v = 0; v < V; v++) {
                    int dl;
                    const int made = (int)vget(xa, v) + g[v];
                    asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1"
                        : "=v"(dl) : "v"(made), "v"(B.sb[c][v]));
                    if constexpr (CHECK) dl = valid(b0 + v) ? dl : MASKED32;
                    if constexpr (TABU) dl = ((B.skm >> (c * V + v)) & 1u) ? MASKED32 : dl;
                    m = min(m, (dl << 3) | v);
                }
                const int b = b0 + (m & 7);
                const unsigned lohi = ((unsigned)min(a, b) << 16) | (unsigned)max(a, b);
                const long long key = (long long)(((u64)(unsigned)((m >> 3) - d_a) << 32) | lohi);
                q.k = key < q.k ? key : q.k;
            };
            if (clean) k32(std::false_type{}); else k32(std::true_type{});
        } else if constexpr (PACKED) {
            AT g[V];
#pragma unroll
            for (int v = 0; v < V; v++) g[v] = (AT)*reinterpret_cast<const T *>(bS + B.sb[c][v]);
            // the chunk's own winner first (32-bit compares; for a fixed a the labels of consecutive
            // b's ascend with v, so the first strictly smallest delta in v order is the reference's
            // pick among them), then ONE 64-bit key meets the running best
            auto keys = [&](auto check_tag) __attribute__((always_inline)) {
                constexpr bool CHECK = decltype(check_tag)::value;
                int dm = 0x7fffffff, bv = 0;
#pragma unroll
                for (int v = 0; v < V; v++) {
                    int delta = (int)vget(xa, v) + g[v] - (d_a + B.dn[c][v]);
                    if constexpr (CHECK) delta = valid(b0 + v) ? delta : BIG;
                    const bool take = delta < dm;
                    dm = take ? delta : dm;
                    bv = take ? v : bv;
                }
                const int b = b0 + bv;
                const unsigned lohi = ((unsigned)min(a, b) << 16) | (unsigned)max(a, b);
                const long long key = (long long)(((u64)(unsigned)dm << 32) | lohi);
                q.k = key < q.k ? key : q.k;
            };
            if (clean) keys(std::false_type{}); else keys(std::true_type{});
        } else {
            AT g[V];
#pragma unroll
            for (int v = 0; v < V; v++) g[v] = (AT)*reinterpret_cast<const T *>(bS + B.sb[c][v]);
            // the chunk's own winner first: for a fixed a the labels of consecutive b's ascend with
            // v, so the first strictly smallest delta in v order is the reference's pick among
            // them; only that one meets the running best (and its tie branch)
            auto pairs = [&](auto check_tag) __attribute__((always_inline)) {
            constexpr bool CHECK = decltype(check_tag)::value;
            AT dm = 0;
            int bv = 0;
            bool okm = false;
#pragma unroll
            for (int v = 0; v < V; v++) {
                bool ok = true;
                if constexpr (CHECK) ok = valid(b0 + v);
                const AT made = (AT)vget(xa, v) + g[v];
                const AT kept = d_a + B.dn[c][v];
                const AT delta = made - kept;               // refinment.c:58-60
                const bool take = ok & (!okm | (delta < dm));
                dm = take ? delta : dm;
                bv = take ? v : bv;
                okm = okm | ok;
            }
            {
                const int b = b0 + bv;
                const AT delta = dm;
                const bool lt = okm & (delta < q.d);
                bool eq = okm & (delta == q.d);
                if constexpr (!TABU) eq &= delta < (AT)0;
                if (__ballot(eq)) {               // wave-uniform and rare: same delta, lower (a,b) wins
                    if (eq) {
                        const u64 kn = a < b ? ((u64)(unsigned)a << 32) | (unsigned)b : ((u64)(unsigned)b << 32) | (unsigned)a;
                        const u64 ko = q.a < q.b ? ((u64)(unsigned)q.a << 32) | (unsigned)q.b
                                                 : ((u64)(unsigned)q.b << 32) | (unsigned)q.a;
                        if (!q.have || kn < ko) { q.a = a; q.b = b; q.have = true; }
                    }
                }
                q.d = lt ? delta : q.d;
                q.a = lt ? a : q.a;
                q.b = lt ? b : q.b;
                q.have = q.have | lt;
            }
            };
            if (clean) pairs(std::false_type{}); else pairs(std::true_type{});
        }
    }
}

template <typename T, int NCH, bool TABU>
__device__ __forceinline__ void sweep_step(Best &q, const BState<T, NCH> &B, const T *bA, const unsigned char *bS, unsigned ldsS,
                                           int a, int am, int sa, int n, int ld, int BT, int tid, int wave_base, bool symmetric)
{
    if constexpr (TABU) {
        if (symmetric) sweep_step_as<T, NCH, true, true>(q, B, bA, bS, ldsS, a, am, sa, n, ld, BT, tid, wave_base, true);
        else sweep_step_as<T, NCH, true, false>(q, B, bA, bS, ldsS, a, am, sa, n, ld, BT, tid, wave_base, false);
    } else if (symmetric) sweep_step_as<T, NCH, false, true>(q, B, bA, bS, ldsS, a, am, sa, n, ld, BT, tid, wave_base, true);
    else sweep_step_as<T, NCH, false, false>(q, B, bA, bS, ldsS, a, am, sa, n, ld, BT, tid, wave_base, false);
}

// the thread's result as (delta, key) for block_argmin
template <typename T, bool TABU>
__device__ __forceinline__ void best_finish(const Best &q, double &d, u64 &key)
{
    typedef typename Elem<T>::acc AT;
    constexpr bool PKS = sizeof(T) == 2;
    constexpr bool PACKED = std::is_same<AT, int>::value;
    const double masked = PKS ? (double)(MASKED32 / 2) : (double)Elem<T>::big() / 2;
    double bd = q.d;
    int ba = q.a, bb = q.b;
    bool have = q.have;
    if constexpr (PACKED) {
        const int di = (int)(q.k >> 32);
        bd = (double)di;
        ba = (int)(((unsigned)q.k) >> 16);
        bb = (int)(((unsigned)q.k) & 0xffffu);
        have = TABU ? bd < masked : di < 0;
    }
    // a masked pair can only have "won" in TABU mode (nothing admissible): report none
    if (!have || bd >= masked) { d = TABU ? DBL_MAX : 0.0; key = TABU ? KEY_NONE : 0; }
    else { d = bd; key = ba < bb ? ((u64)(unsigned)ba << 32) | (unsigned)bb : ((u64)(unsigned)bb << 32) | (unsigned)ba; }
}

// The workgroup's best pair from the threads' running bests: (d, key) in every thread; true in the ONE thread that
// holds that pair (a pair is evaluated exactly once; no thread when nothing was found).  Integer deltas: the packed
// 64-bit key itself is reduced (one compare per step) and decoded once; doubles go through (delta, a, b).
template <typename T, bool TABU>
__device__ __forceinline__ bool block_best(const Best &q, double &d, u64 &key, Partial *scratch)
{
    constexpr bool PACKED = std::is_same<typename Elem<T>::acc, int>::value;
    const u64 none = TABU ? KEY_NONE : 0;
    if constexpr (PACKED) {
        long long k = wave_min_i64(q.k);
        const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
        if ((threadIdx.x & 63) == 0) scratch[w].key = (u64)k;
        __syncthreads();
        k = (long long)scratch[0].key;
        for (int i = 1; i < nw; i++) { const long long o = (long long)scratch[i].key; k = o < k ? o : k; }
        Best r = q;
        r.k = k;
        best_finish<T, TABU>(r, d, key);
        return q.k == k && key != none;
    } else {
        double d_own;
        u64 key_own;
        best_finish<T, TABU>(q, d_own, key_own);
        d = d_own; key = key_own;
        block_argmin(d, key, scratch);
        return key != none && key_own == key && d_own == d;
    }
}

// ---------------------------------------------------------------------------
// K2 "pipelined" sweep: the streaming form for rows that fit LDS three times (any cell type;
// uint16 rows up to n ~ 27 000).  Workgroup g owns a run of cnt consecutive tour edges and
// needs the cnt+1 matrix rows of the nodes on that run, each exactly once:
//     row r   (node a)  : c[a][b], read conflict-free from LDS at the thread's OWN b's
//     row r+1 (node sa) : c[sa][succ b], random LDS gather
//     rows r+2 .. r+1+D : in flight from HBM in D register sets; one of them is
//                         written to the third LDS buffer at the end of a step
//                         and its registers are re-issued for row r+2+D
// so every matrix byte is fetched once per sweep (+1 row per run) with 16-byte
// coalesced loads, up to D rows per workgroup are in flight at any time, and
// one barrier separates steps.  State, pair ownership and argmin: sweep_step().
// ---------------------------------------------------------------------------
// The streaming part of the pipelined sweep (after nodes[] and the per-b state are in place):
// rows through D register sets and three rotating LDS buffers, one barrier per step.
template <typename T, int NCH, int D, bool TABU>
__device__ __forceinline__ void pipe_stream(Best &q, const SweepArgs &A, const BState<T, NCH> &B, T *buf, const int *nodes, unsigned lds0,
                                            int cnt, int iter, int tenure, unsigned long long *stamp)
{
    typedef typename Elem<T>::vec VT;
    constexpr int V = Elem<T>::V;
    const int n = A.n, ld = A.ld;
    const int tid = threadIdx.x, BT = blockDim.x;
    const int nvec = ld / V;
    const T *mat = static_cast<const T *>(A.mat);
#define STAMP(i) do { if (stamp && tid == 0) stamp[i] = wall_clock64(); } while (0)
    VT R[D][NCH];
    auto issue = [&](VT(&Rs)[NCH], int r) __attribute__((always_inline)) {
        // Branch-free.  Lanes past the row end re-read its last vector (and later re-write
        // the same bytes).  Past the end of the run (r > cnt) every lane re-reads one hot
        // vector instead: the number of loads in flight is then the same on every path,
        // which lets hipcc place exact counted vmcnt waits in front of the LDS writes.
        const VT *src = reinterpret_cast<const VT *>(mat + (size_t)(nodes[min(r, cnt)] & NODE_MASK) * ld);
        const int lim = (r <= cnt && A.ablate != 2) ? nvec - 1 : 0;
#pragma unroll
        for (int c = 0; c < NCH; c++) Rs[c] = src[min(c * BT + tid, lim)];
    };
    auto land = [&](const VT(&Rs)[NCH], int slot) __attribute__((always_inline)) {
        VT *dst = reinterpret_cast<VT *>(buf + (size_t)slot * ld);
#pragma unroll
        for (int c = 0; c < NCH; c++) dst[min(c * BT + tid, nvec - 1)] = Rs[c];
    };
    // row r travels through register set r % D
#pragma unroll
    for (int r = 0; r < D; r++) issue(R[r], r);
    land(R[0], 0);
    land(R[1 % D], 1);
    issue(R[0], D);
    issue(R[1 % D], D + 1);
    __syncthreads();
    STAMP(2);

    const int wave_base = __builtin_amdgcn_readfirstlane(tid & ~63);

    auto step = [&](int s, VT(&Rs)[NCH]) __attribute__((always_inline)) {
        const int a_raw = __builtin_amdgcn_readfirstlane(nodes[s]), sa_raw = __builtin_amdgcn_readfirstlane(nodes[s + 1]);
        const int a = a_raw & NODE_MASK;                                        // wave-uniform: keep it scalar
        const int am = __builtin_amdgcn_readfirstlane(nodes[s - 1]) & NODE_MASK;
        const int sa = sa_raw & NODE_MASK;
        const T *bA = buf + (size_t)(s % 3) * ld;
        const unsigned char *bS = reinterpret_cast<const unsigned char *>(buf + (size_t)((s + 1) % 3) * ld);
        const unsigned ldsS = lds0 + (unsigned)(((s + 1) % 3) * ld) * (unsigned)sizeof(T);
        if (stamp && s == 10 && (tid & 63) == 0) stamp[32 + (tid >> 6)] = wall_clock64();   // per-wave: step 10 entered
        bool live = A.ablate != 1;
        if constexpr (TABU) live = live && !((a_raw | sa_raw) & TABU_NODE);
        if (live) sweep_step<T, NCH, TABU>(q, B, bA, bS, ldsS, a, am, sa, n, ld, BT, tid, wave_base, A.symmetric != 0);
        if (stamp && tid == 0 && s < 12) stamp[8 + 2 * s] = wall_clock64();      // compute done
        if (stamp && s == 10 && (tid & 63) == 0) stamp[48 + (tid >> 6)] = wall_clock64();   // per-wave: step 10 evaluated
        if (s + 2 <= cnt) land(Rs, (s + 2) % 3);
        issue(Rs, s + 2 + D);
        __syncthreads();
        if (stamp && tid == 0 && s < 12) stamp[9 + 2 * s] = wall_clock64();      // row landed, barrier passed
    };

    {
        int s = 0;
        for (; s + D <= cnt; s += D) { // unconditional body: exact vmcnt accounting
#pragma unroll
            for (int u = 0; u < D; u++) step(s + u, R[(u + 2) % D]);
        }
#pragma unroll
        for (int u = 0; u < D; u++)
            if (s + u < cnt) step(s + u, R[(u + 2) % D]);
    }

#undef STAMP
}

// Streaming, second form (symmetric matrices, plain 2-opt, rows that fit LDS FOUR times): TWO tour edges per barrier
// interval, and the row of a straight from the registers that loaded it.  In pipe_stream() a thread writes the vector
// it fetched into LDS and reads the very same bytes back one step later as c[a][own b's] -- only the row of succ a
// (random gather) has to be in LDS.  So a row lives in registers from its fetch until its step as "row of a", and in
// LDS only for its step as "row of succ a":
//     interval k, steps s = 2k and s+1:   rows s, s+1 in registers A0, A1 (row of a);  rows s+1, s+2 in LDS (gather)
//     then: rows s+3, s+4 (registers X0, X1, in flight since the previous interval) are written into the two LDS
//     buffers the previous interval gathered from, A0 <- N0 (row s+2), A1 <- X0, N0 <- X1, and X0, X1 are re-issued
//     for rows s+5, s+6; ONE barrier.
// Half the barriers and row-landing waits of pipe_stream(), two independent evaluation chains per interval, and a wave
// that owns no pair of one step usually owns pairs of the other (ownership goes by block distance from a, and a and
// succ a sit in different blocks): the 16 waves of a workgroup idle at the barrier far less.  c[a][succ a] is read as
// c[succ a][a] from the gather row (symmetric), so the row of a is never needed in LDS.
template <typename T, int NCH, int PAIRS>
__device__ __forceinline__ void pipe_stream2(Best &q, const SweepArgs &A, const BState<T, NCH> &B, T *buf, const int *nodes, unsigned lds0,
                                             int cnt, unsigned long long *stamp)
{
    typedef typename Elem<T>::vec VT;
    constexpr int V = Elem<T>::V;
    const int n = A.n, ld = A.ld;
    const int tid = threadIdx.x, BT = blockDim.x;
    const int nvec = ld / V;
    const T *mat = static_cast<const T *>(A.mat);
    // A0, A1: rows of a of the two steps of an interval; N0: the row after them (already gathered from, needed as a row
    // of a next interval); X (and, PAIRS = 2, Y): pairs of rows in flight, landed PAIRS intervals after their issue --
    // with two pairs up to four rows (4 x 32 KB at n=4096 f64) of a workgroup are on their way at any time (uint16 rows
    // with two chunks per thread keep one pair: seven register sets next to 16 b's of state would spill)
    VT A0[NCH], A1[NCH], N0[NCH], X0[NCH], X1[NCH], Y0[PAIRS == 2 ? NCH : 1], Y1[PAIRS == 2 ? NCH : 1];
    auto issue = [&](VT(&Rs)[NCH], int r) __attribute__((always_inline)) {
        // branch-free; past the end of the run every lane re-reads one hot vector (same load count on every path, which
        // lets hipcc place exact counted vmcnt waits in front of the LDS writes)
        const VT *src = reinterpret_cast<const VT *>(mat + (size_t)nodes[min(r, cnt)] * ld);
        const int lim = (r <= cnt && A.ablate != 2) ? nvec - 1 : 0;
#pragma unroll
        for (int c = 0; c < NCH; c++) Rs[c] = src[min(c * BT + tid, lim)];
    };
    auto land = [&](const VT(&Rs)[NCH], int r) __attribute__((always_inline)) {
        VT *dst = reinterpret_cast<VT *>(buf + (size_t)(r & 3) * ld);
#pragma unroll
        for (int c = 0; c < NCH; c++) dst[min(c * BT + tid, nvec - 1)] = Rs[c];
    };
    issue(A0, 0); issue(A1, 1); issue(N0, 2); issue(X0, 3); issue(X1, 4);
    if constexpr (PAIRS == 2) { issue(Y0, 5); issue(Y1, 6); }
    land(A1, 1);
    land(N0, 2);
    __syncthreads();
    if (stamp && tid == 0) stamp[2] = wall_clock64();
    const int wave_base = __builtin_amdgcn_readfirstlane(tid & ~63);
    auto step = [&](int s, const VT(&Ar)[NCH]) __attribute__((always_inline)) {
        const int a = __builtin_amdgcn_readfirstlane(nodes[s]);
        const int am = __builtin_amdgcn_readfirstlane(nodes[s - 1]);
        const int sa = __builtin_amdgcn_readfirstlane(nodes[s + 1]);
        const int slot = (s + 1) & 3;
        const unsigned char *bS = reinterpret_cast<const unsigned char *>(buf + (size_t)slot * ld);
        const unsigned ldsS = lds0 + (unsigned)(slot * ld) * (unsigned)sizeof(T);
        if (A.ablate != 1) sweep_step_as<T, NCH, false, true>(q, B, nullptr, bS, ldsS, a, am, sa, n, ld, BT, tid, wave_base, true, Ar);
    };
    // one interval: steps s, s+1; rows s+3, s+4 (pair P, issued two intervals ago) into the LDS buffers the previous
    // interval gathered from; registers rotate; the pair is re-issued for the rows four intervals' worth ahead
    auto interval = [&](int s, VT(&P0)[NCH], VT(&P1)[NCH], auto tail_tag) __attribute__((always_inline)) {
        constexpr bool TAIL = decltype(tail_tag)::value;
        step(s, A0);
        if (!TAIL || s + 1 < cnt) step(s + 1, A1);
        if (stamp && tid == 0 && s < 24) stamp[8 + s] = wall_clock64();
        if (!TAIL || s + 3 <= cnt) land(P0, s + 3);
        if (!TAIL || s + 4 <= cnt) land(P1, s + 4);
#pragma unroll
        for (int c = 0; c < NCH; c++) { A0[c] = N0[c]; A1[c] = P0[c]; N0[c] = P1[c]; }
        issue(P0, s + 3 + 2 * PAIRS);
        issue(P1, s + 4 + 2 * PAIRS);
        __syncthreads();
        if (stamp && tid == 0 && s < 24) stamp[9 + s] = wall_clock64();
    };
    int s = 0;
    if constexpr (PAIRS == 2) {
        for (; s + 4 <= cnt; s += 4) {      // unconditional body: exact vmcnt accounting
            interval(s, X0, X1, std::false_type{});
            interval(s + 2, Y0, Y1, std::false_type{});
        }
        if (s < cnt) interval(s, X0, X1, std::true_type{});
        if (s + 2 < cnt) interval(s + 2, Y0, Y1, std::true_type{});
    } else {
        for (; s + 2 <= cnt; s += 2) interval(s, X0, X1, std::false_type{});
        if (s < cnt) interval(s, X0, X1, std::true_type{});
    }
}

template <typename T, int NCH, int D, bool TABU>
__global__ void __launch_bounds__(1024) k_sweep_pipe(SweepArgs A)
{
    typedef typename Elem<T>::vec VT;
    typedef typename Elem<T>::acc AT;
    constexpr int V = Elem<T>::V;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int n = A.n, ld = A.ld;
    const int t = A.slot0 + blockIdx.y;
    if (A.S.done[t]) return;
    const int tid = threadIdx.x, BT = blockDim.x;
    const int nvec = ld / V; // 16-byte vectors per row

    // LDS: 3 row buffers (4 in the two-edge form, D == 9) | nodes[-1 .. P] | 16 spare bytes | reduction scratch
    constexpr int NBUF = D == 9 ? 4 : 3;
    T *buf = reinterpret_cast<T *>(smem);
    int *nodes = reinterpret_cast<int *>(smem + (size_t)NBUF * ld * sizeof(T)) + 1; // nodes[-1] = node before the run
    const size_t nodes_bytes = (size_t)((A.P + 2 + 3) & ~3) * 4;
    Partial *scratch = reinterpret_cast<Partial *>(smem + (size_t)NBUF * ld * sizeof(T) + nodes_bytes + 16);
    const unsigned lds0 = (unsigned)(uintptr_t)(lds_u8 *)smem;   // LDS byte address of the row buffers

    const T *mat = static_cast<const T *>(A.mat);
    const int *ord = A.S.ord + (size_t)t * n;
    const int dir = A.S.dir[t];

    int iter = 0, tenure = 0;
    if constexpr (TABU) { iter = A.tabu->iter; tenure = A.tabu->tenure; }

    unsigned long long *stamp = A.stamps ? A.stamps + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 64 : nullptr;
#define STAMP(i) do { if (stamp && tid == 0) stamp[i] = wall_clock64(); } while (0)
    STAMP(0);
    const int p0 = ((int)blockIdx.x + A.g0) * A.P;
    const int cnt = min(A.P, n - p0);
    // (host guarantees cnt >= 1 for every launched workgroup)
    // the run in TOUR order: nodes[s] = a of step s, nodes[s+1] = its successor, nodes[-1] = its predecessor
    // (tabu: bit 30 marks a tabu node, so that the steps need no global read for it)
    for (int i = tid - 1; i <= cnt; i += BT) {
        const int v = ord[wrap(p0 + (dir > 0 ? i : cnt - i), n)];
        int flag = 0;
        if constexpr (TABU) flag = is_tabu(A.tabu_list, v, iter, tenure) ? TABU_NODE : 0;
        nodes[i] = v | flag;
    }

    // per-thread state of the owned b's from the node-indexed view (coalesced 16-byte loads)
    BState<T, NCH> B;
    B.skm = 0;
    load_bstate<T, NCH, TABU>(B, A, smem, t, iter, tenure);   // (contains the barrier that also publishes nodes[])
    STAMP(1);

    Best q;
    best_init<TABU>(q);
    if constexpr (D == 9) pipe_stream2<T, NCH, 1>(q, A, B, buf, nodes, lds0, cnt, stamp);   // symmetric, plain 2-opt (host)
    else pipe_stream<T, NCH, D, TABU>(q, A, B, buf, nodes, lds0, cnt, iter, tenure, stamp);

    STAMP(3);
    double d;
    u64 key;
    block_best<T, TABU>(q, d, key, scratch);
    if (tid == 0) {
        Partial o; o.d = d; o.key = key;
        A.S.partial[(size_t)t * A.S.pstride + blockIdx.x + A.g0] = o;
    }
#undef STAMP
}


// ---------------------------------------------------------------------------
// K3 "resident" sweep: for rows small enough that the P+1 (<= 9) rows of a run fit LDS
// together (uint16 cells up to n ~ 9 000 at one workgroup per CU, int32 / f64 for small n
// and for multi-start batches).  The workgroup issues the loads of all its rows at once (one
// memory round trip for the whole run), lands them in chunks of three rows, and after each
// chunk's barrier every wave walks the steps whose two rows are in LDS on its own -- no
// barrier, no LDS write and no global access inside a step.  State, pair ownership and
// argmin: sweep_step().
// ---------------------------------------------------------------------------
template <typename T, int NCH, int PMAX, bool TABU>
__global__ void __launch_bounds__(1024) k_sweep_res(SweepArgs A)
{
    typedef typename Elem<T>::vec VT;
    typedef typename Elem<T>::acc AT;
    constexpr int V = Elem<T>::V;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int n = A.n, ld = A.ld;
    const int t = A.slot0 + blockIdx.y;
    if (A.S.done[t]) return;
    const int tid = threadIdx.x, BT = blockDim.x;
    const int nvec = ld / V;

    // LDS: (P+1) rows | nodes[-1 .. P] | reduction scratch
    T *rows = reinterpret_cast<T *>(smem);
    const size_t rows_bytes = (size_t)(A.P + 1) * ld * sizeof(T);
    int *nodes = reinterpret_cast<int *>(smem + rows_bytes) + 1;
    Partial *scratch = reinterpret_cast<Partial *>(smem + rows_bytes + (size_t)((A.P + 2 + 3) & ~3) * 4);
    const unsigned lds0 = (unsigned)(uintptr_t)(lds_u8 *)smem;

    const T *mat = static_cast<const T *>(A.mat);
    const int *ord = A.S.ord + (size_t)t * n;
    const int dir = A.S.dir[t];

    int iter = 0, tenure = 0;
    if constexpr (TABU) { iter = A.tabu->iter; tenure = A.tabu->tenure; }

    unsigned long long *stamp = A.stamps ? A.stamps + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 64 : nullptr;
#define STAMP(i) do { if (stamp && tid == 0) stamp[i] = wall_clock64(); } while (0)
    STAMP(0);
    const int p0 = ((int)blockIdx.x + A.g0) * A.P;
    const int cnt = min(A.P, n - p0);
    // the run in TOUR order: nodes[s] = a of step s, nodes[s+1] = its successor, nodes[-1] = its predecessor
    // (tabu: bit 30 marks a tabu node, so that the steps need no global read for it)
    for (int i = tid - 1; i <= cnt; i += BT) {
        const int v = ord[wrap(p0 + (dir > 0 ? i : cnt - i), n)];
        int flag = 0;
        if constexpr (TABU) flag = is_tabu(A.tabu_list, v, iter, tenure) ? TABU_NODE : 0;
        nodes[i] = v | flag;
    }

    // per-thread state of the owned b's: coalesced loads of the node-indexed view.  Issued
    // BEFORE the matrix rows: vector loads return in order, so anything younger than the rows
    // would only become usable after the last row has arrived.
    BState<T, NCH> B;
    B.skm = 0;
    load_bstate<T, NCH, TABU>(B, A, smem, t, iter, tenure);   // (contains the barrier that also publishes nodes[])
    STAMP(1);

    // every row of the run in flight at once
    VT R[PMAX + 1][NCH];
#pragma unroll
    for (int r = 0; r <= PMAX; r++) {
        if (r <= cnt && A.ablate != 2) {
            const VT *src = reinterpret_cast<const VT *>(mat + (size_t)(nodes[r] & NODE_MASK) * ld);
#pragma unroll
            for (int c = 0; c < NCH; c++) R[r][c] = src[min(c * BT + tid, nvec - 1)];
        }
    }

    const int wave_base = __builtin_amdgcn_readfirstlane(tid & ~63);
    Best q;
    best_init<TABU>(q);

    auto step = [&](int s) __attribute__((always_inline)) {
        const int a_raw = __builtin_amdgcn_readfirstlane(nodes[s]), sa_raw = __builtin_amdgcn_readfirstlane(nodes[s + 1]);
        const int a = a_raw & NODE_MASK;
        const int am = __builtin_amdgcn_readfirstlane(nodes[s - 1]) & NODE_MASK;
        const int sa = sa_raw & NODE_MASK;
        const T *bA = rows + (size_t)s * ld;
        const unsigned char *bS = reinterpret_cast<const unsigned char *>(rows + (size_t)(s + 1) * ld);
        const unsigned ldsS = lds0 + (unsigned)((s + 1) * ld) * (unsigned)sizeof(T);
        if (stamp && tid == 0 && s < 24) stamp[8 + s] = wall_clock64();
        bool live = A.ablate != 1;
        if constexpr (TABU) live = live && !((a_raw | sa_raw) & TABU_NODE);
        if (live) sweep_step<T, NCH, TABU>(q, B, bA, bS, ldsS, a, am, sa, n, ld, BT, tid, wave_base, A.symmetric != 0);
    };

    // Rows land in chunks of RPC; after each chunk one barrier, then every step whose two rows
    // are in LDS runs while the later rows are still in flight (3 barriers in all for P = 8).
    constexpr int RPC = TSPGPU_RPC;
    {
        int s = 0;
#pragma unroll
        for (int r0 = 0; r0 <= PMAX; r0 += RPC) {
#pragma unroll
            for (int r = r0; r < r0 + RPC && r <= PMAX; r++) {
                if (r <= cnt && A.ablate != 2) {
                    VT *dst = reinterpret_cast<VT *>(rows + (size_t)r * ld);
#pragma unroll
                    for (int c = 0; c < NCH; c++) dst[min(c * BT + tid, nvec - 1)] = R[r][c];
                }
            }
            __syncthreads();
            if (r0 == 0) STAMP(2);
            const int s_end = min(cnt, r0 + RPC - 1);   // steps s with row s+1 <= r0+RPC-1
            for (; s < s_end; s++) step(s);
        }
    }

    STAMP(3);
    double d;
    u64 key;
    block_best<T, TABU>(q, d, key, scratch);
    if (tid == 0) {
        Partial o; o.d = d; o.key = key;
        A.S.partial[(size_t)t * A.S.pstride + blockIdx.x + A.g0] = o;
    }
    STAMP(4);
#undef STAMP
}


// ---------------------------------------------------------------------------
// One launch per sweep ("fused"): k_sweep_fused = k_apply of the previous sweep's move +
// k_sweep_res, for symmetric matrices.  The tour state is kept twice (parity ping-pong) in a
// direction-free form -- ord/pos plus, per NODE, its two array neighbours (nl, nr) and the two
// edge costs (dl, dr); succ b = dir > 0 ? nr : nl.  A 2-opt move reverses an array range: nodes
// inside swap (nl,dl) <-> (nr,dr), four nodes around the ends get one new neighbour, positions
// reflect.  So every workgroup derives everything it needs of the NEW state from coalesced
// loads of the OLD one plus a handful of scalars (it reduces the previous launch's partials
// itself), and the new state is written piecewise: each workgroup records its own slice of
// nodes and its own cells of ord.  No separate apply launch, no gather, no inter-workgroup
// communication inside a launch.  k_fused_begin / k_fused_end convert from / to the Tours form.
// ---------------------------------------------------------------------------
// PACKED (uint16 cells, n <= 65536): the per-node records are 16-bit -- pos as uint16, (nl, nr) and
// (dl, dr) as halves of one 32-bit word each, in the same buffers -- which halves what every
// workgroup of every launch reads of them.
template <typename AT, bool PACKED>
__global__ void __launch_bounds__(256) k_fused_begin(Tours S, Fused F, int n, int slot0)
{
    const int t = slot0 + blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const size_t tn = (size_t)t * n;
    if (p < n) {
        const int *ord = S.ord + tn;
        const AT *dp = reinterpret_cast<const AT *>(S.dpos + tn);
        const int v = ord[p], pl = wrap(p - 1, n);
        F.ord[1][tn + p] = v;
        if constexpr (PACKED) {
            (reinterpret_cast<u16 *>(F.pos[1]) + tn)[v] = (u16)p;
            (reinterpret_cast<unsigned *>(F.nl[1]) + tn)[v] = (unsigned)ord[pl] | ((unsigned)ord[wrap(p + 1, n)] << 16);
            (reinterpret_cast<unsigned *>(F.dl[1]) + tn)[v] = (unsigned)dp[pl] | ((unsigned)dp[p] << 16);
        } else {
            F.pos[1][tn + v] = p;
            F.nl[1][tn + v] = ord[pl];
            F.nr[1][tn + v] = ord[wrap(p + 1, n)];
            reinterpret_cast<AT *>(F.dl[1] + tn)[v] = dp[pl];
            reinterpret_cast<AT *>(F.dr[1] + tn)[v] = dp[p];
        }
    }
    if (p == 0) {
        F.dir[1][t] = S.dir[t]; F.k[1][t] = 0; F.cost[1][t] = S.cost[t]; F.stop[1][t] = 0; F.stop[0][t] = 0;
        F.cur[t] = 1;
        F.bestkey[t * 4 + 0] = 0; F.bestkey[t * 4 + 1] = 0; F.bestkey[t * 4 + 2] = 0;
    }
}

template <typename AT, bool PACKED>
__global__ void __launch_bounds__(256) k_fused_end(Tours S, Fused F, int n, int slot0, int last_parity)
{
    const int t = slot0 + blockIdx.y;
    const int v = blockIdx.x * 256 + threadIdx.x;
    const size_t tn = (size_t)t * n;
    const int c = S.done[t] ? F.cur[t] : last_parity;   // not finished (deadline): the last state written
    const int dir = F.dir[c][t];
    if (v < n) {
        int p, l, r;
        AT dl, dr;
        if constexpr (PACKED) {
            p = (reinterpret_cast<const u16 *>(F.pos[c]) + tn)[v];
            const unsigned lr = (reinterpret_cast<const unsigned *>(F.nl[c]) + tn)[v], dd = (reinterpret_cast<const unsigned *>(F.dl[c]) + tn)[v];
            l = (int)(lr & 0xffffu); r = (int)(lr >> 16);
            dl = (AT)(dd & 0xffffu); dr = (AT)(dd >> 16);
        } else {
            p = F.pos[c][tn + v];
            l = F.nl[c][tn + v]; r = F.nr[c][tn + v];
            dl = reinterpret_cast<const AT *>(F.dl[c] + tn)[v]; dr = reinterpret_cast<const AT *>(F.dr[c] + tn)[v];
        }
        S.ord[tn + p] = v;
        S.pos[tn + v] = p;
        reinterpret_cast<AT *>(S.dpos + tn)[p] = dr;
        S.succ[tn + v] = dir > 0 ? r : l;
        reinterpret_cast<AT *>(S.dnb + tn)[v] = dir > 0 ? dr : dl;
    }
    if (v == 0) { S.dir[t] = dir; S.cost[t] = F.cost[c][t]; }
}

// Wave-uniform reads of the previous launch's state go through the scalar cache (constant
// address space: the compiler emits s_load and tracks lgkmcnt): every wave holds them in SGPRs,
// no LDS staging, no vector-memory queueing.
typedef __attribute__((address_space(4))) const int c_i32;
typedef __attribute__((address_space(4))) const double c_f64;
typedef __attribute__((address_space(4))) const long long c_i64;
template <typename T>
__device__ __forceinline__ typename Elem<T>::acc scalar_cell(const T *mat, size_t idx)
{
    if constexpr (sizeof(T) == 8) return ((c_f64 *)mat)[idx];
    else if constexpr (sizeof(T) == 4) return ((c_i32 *)mat)[idx];
    else {
        const unsigned w = (unsigned)((c_i32 *)mat)[idx >> 1];
        return (int)((idx & 1) ? w >> 16 : w & 0xffffu);
    }
}

// D = 0: rows resident (k_sweep_res's body, P <= PMAX); D > 0: rows streamed (pipe_stream).
template <typename T, int NCH, int PMAX, int D>
__global__ void __launch_bounds__(1024) k_sweep_fused(SweepArgs A)
{
    typedef typename Elem<T>::vec VT;
    typedef typename Elem<T>::acc AT;
    constexpr int V = Elem<T>::V;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int n = A.n, ld = A.ld;
    const int t = A.slot0 + blockIdx.y;
    if (A.S.done[t]) return;
    const int tid = threadIdx.x, BT = blockDim.x;
    const int nvec = ld / V;

    // LDS: (P+1) rows, or the 3 rotating row buffers | nodes[-1 .. P] | (16 spare bytes) | reduction scratch
    T *rows = reinterpret_cast<T *>(smem);
    const size_t rows_bytes = (size_t)(D >= 4 ? 4 : D > 0 ? 3 : A.P + 1) * ld * sizeof(T);
    int *nodes = reinterpret_cast<int *>(smem + rows_bytes) + 1;
    Partial *scratch = reinterpret_cast<Partial *>(smem + rows_bytes + (size_t)((A.P + 2 + 3) & ~3) * 4 + (D > 0 ? 16 : 0));

    constexpr bool TABU = false;
    const T *mat = static_cast<const T *>(A.mat);
    const int rd = 1 - A.parity, wr = A.parity;       // state read / written by this launch
    const size_t tn = (size_t)t * n;
    const int *ord_o = A.F.ord[rd] + tn, *pos_o = A.F.pos[rd] + tn;
    const int *nl_o = A.F.nl[rd] + tn, *nr_o = A.F.nr[rd] + tn;
    const AT *dl_o = reinterpret_cast<const AT *>(A.F.dl[rd] + tn), *dr_o = reinterpret_cast<const AT *>(A.F.dr[rd] + tn);
    c_i32 *ord_c = (c_i32 *)ord_o, *pos_c = (c_i32 *)pos_o;
    const int k_done = ((c_i32 *)A.F.k[rd])[t];        // sweeps completed before this launch
    const int dir_o = ((c_i32 *)A.F.dir[rd])[t];
    const int stop_o = ((c_i32 *)A.F.stop[rd])[t];
    const double cost_o = ((c_f64 *)A.F.cost[rd])[t];   // (used by workgroup 0 only; here it costs no dependent trip there)
    const int cap = A.S.cap_sweeps[t];
    // PAY (uint16 cells): the previous launch's result is one atomically minimised key + the
    // winner's geometry record; else: per-workgroup partials, reduced here by every workgroup
    constexpr bool PAY = sizeof(T) == 2;
    constexpr int PAYW = 16;                            // ints per workgroup record (10 used with f64 edge costs)
    const Partial *part = A.F.partial[rd] + (size_t)t * A.S.pstride;
    Partial pq0;
    pq0.d = 0.0; pq0.key = 0;
    if constexpr (!PAY) pq0 = part[min((int)threadIdx.x, (int)gridDim.x - 1)];   // issued before k_done is back: one trip less
    const long long K0 = PAY ? ((c_i64 *)A.F.bestkey)[t * 4 + 0] : 0, K1 = PAY ? ((c_i64 *)A.F.bestkey)[t * 4 + 1] : 0,
                    K2 = PAY ? ((c_i64 *)A.F.bestkey)[t * 4 + 2] : 0;      // all three slots: no trip behind k_done
    // the old records of the own b's depend on nothing either: in flight during the reduction
    // (up to 16 b's per thread; beyond that the registers are needed elsewhere: loaded chunk by chunk below)
    // uint16 cells: 16-bit records (k_fused_begin): pos as uint16, (nl | nr << 16), (dl | dr << 16)
    constexpr bool HOIST = NCH * V <= 16;
    constexpr int HC = HOIST ? NCH : 1;
    constexpr int QW = PAY ? 1 : V;                     // PAY: kept packed in registers, unpacked at use
    int qv[HC][V], lv[HC][V], rv[HC][QW];
    AT dlv[HC][V], drv[HC][QW];
    u16 q16[HC][PAY ? V : 1];
    auto load_old = [&](int c, int slot) __attribute__((always_inline)) {
        const int b0 = min((c * (int)blockDim.x + (int)threadIdx.x) * V, ld - V);
        if constexpr (PAY) {
            load_run<V>(reinterpret_cast<const u16 *>(A.F.pos[rd]) + tn + b0, q16[slot]);
            load_run<V>(reinterpret_cast<const int *>(A.F.nl[rd]) + tn + b0, lv[slot]);
            load_run<V>(reinterpret_cast<const int *>(A.F.dl[rd]) + tn + b0, dlv[slot]);
        } else {
            load_run<V>(pos_o + b0, qv[slot]);
            load_run<V>(nl_o + b0, lv[slot]);
            load_run<V>(nr_o + b0, rv[slot]);
            load_run<V>(dl_o + b0, dlv[slot]);
            load_run<V>(dr_o + b0, drv[slot]);
        }
    };
    if constexpr (HOIST) {
#pragma unroll
        for (int c = 0; c < NCH; c++) load_old(c, c);
    }
    // the nodes at the run's own array cells before the move: also independent of everything, and almost always the
    // nodes after it (a move reverses a median of 3 of 4096 cells on the benchmark trajectory) -- only a cell inside the
    // reversed range needs the dependent load of its mirror cell below
    const int p0 = ((int)blockIdx.x + A.g0) * A.P;
    const int cnt = min(A.P, n - p0);
    int node_spec = 0;
    if (tid <= cnt + 1) node_spec = ord_o[wrap(p0 + tid - 1, n)];
    // The workgroup also RECORDS the new state of its slice of nodes (position, both neighbours, both edge costs).  One
    // node per lane of the second wave, old record loaded here: a single thread doing its eight own nodes was a serial
    // tail of ~300 instructions in front of the workgroup's barrier.
    const int slice = (((n + (int)gridDim.x - 1) / (int)gridDim.x) + V - 1) / V * V;   // nodes recorded per workgroup
    const int S0 = BT >= 128 ? 64 : 0;                   // first slice lane
    int sq = 0, sl_o = 0, sr_o = 0;
    AT sdl = 0, sdr = 0;
    auto load_slice = [&](int b) __attribute__((always_inline)) {
        if constexpr (PAY) {
            sq = (int)(reinterpret_cast<const u16 *>(A.F.pos[rd]) + tn)[b];
            const unsigned lr = (reinterpret_cast<const unsigned *>(A.F.nl[rd]) + tn)[b], dd = (reinterpret_cast<const unsigned *>(A.F.dl[rd]) + tn)[b];
            sl_o = (int)(lr & 0xffffu); sr_o = (int)(lr >> 16);
            sdl = (AT)(dd & 0xffffu); sdr = (AT)(dd >> 16);
        } else {
            sq = pos_o[b]; sl_o = nl_o[b]; sr_o = nr_o[b]; sdl = dl_o[b]; sdr = dr_o[b];
        }
    };
    {
        const int sl = tid - S0, b = (int)blockIdx.x * slice + sl;
        if (sl >= 0 && sl < slice && b < n) load_slice(b);
    }

    unsigned long long *stamp = A.stamps ? A.stamps + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 64 : nullptr;
#define STAMP(i) do { if (stamp && tid == 0) stamp[i] = wall_clock64(); } while (0)
    const unsigned long long t_entry = stamp ? wall_clock64() : 0ull;   // recorded at STAMP(1): launches that leave early keep the last sweep's stamps

    // ---- the move found by the previous launch (every workgroup reduces the same partials)
    double md = 0.0;
    u64 mkey = 0;
    int pwg = 0;
    if constexpr (PAY) {
        if (k_done > 0) {
            const int sl = (k_done + 2) % 3;
            const long long K = sl == 0 ? K0 : sl == 1 ? K1 : K2;
            md = (double)(int)(K >> 45);
            mkey = ((u64)(unsigned)((K >> 29) & 0xffff) << 32) | (unsigned)((K >> 13) & 0xffff);
            pwg = (int)(K & 0x1fff);
        }
        if (blockIdx.x == 0 && tid == 0) A.F.bestkey[t * 4 + (k_done + 1) % 3] = 0;   // the slot the NEXT launch minimises into
    } else if (k_done > 0) {
        if (tid < (int)gridDim.x) { md = pq0.d; mkey = pq0.key; }
        for (int g = tid + BT; g < (int)gridDim.x; g += BT) {     // more workgroups than threads: not with the default plans
            const Partial q = part[g];
            if (key_better(q.d, q.key, md, mkey)) { md = q.d; mkey = q.key; }
        }
        block_argmin(md, mkey, scratch);
    }
    const unsigned long long t_red = stamp ? wall_clock64() : 0ull;
    const bool move = k_done > 0 && md < TWO_OPT_EPS;
    if (stop_o || (k_done > 0 && !move)) {
        // either the previous launch applied the last move a sweep cap allows, or the previous
        // sweep was the final, non-improving one: the state that launch left is the result.
        // (Every workgroup leaves here without writing, so a workgroup that starts after
        // workgroup 0 has raised `done` behaves the same.)
        if (blockIdx.x == 0 && tid == 0) {
            A.S.done[t] = 1; A.F.cur[t] = rd; A.S.nsweeps[t] = k_done;
            if (!stop_o) {
                A.S.last_delta[t] = md;
                if (t == 0 && k_done <= A.hist.cap) { A.hist.a[k_done - 1] = -1; A.hist.b[k_done - 1] = -1; A.hist.d[k_done - 1] = md; }
            }
        }
        return;
    }
    const bool last = cap >= 0 && k_done >= cap;     // apply this move, then stop sweeping
    const int ma = __builtin_amdgcn_readfirstlane((int)(mkey >> 32)), mb = __builtin_amdgcn_readfirstlane((int)(mkey & 0xffffffffu));

    // ---- the move as an array operation on the OLD state (see Tours): reverse cells [lo, lo+M-1]
    int lo = 0, M = 0, ndir = dir_o;
    int x0 = -1, x1 = -1, x2 = -1, x3 = -1;
    AT wA = 0, wB = 0;
    if (move) {
        int i, j, sma = 0, smb = 0;
        AT cab = 0, css = 0;
        if constexpr (PAY) {
            // the winner's record (one scalar load trip): cells of its two nodes, their successors, the two new edge costs
            c_i32 *pay = (c_i32 *)(A.F.payload[rd] + ((size_t)t * A.S.pstride + pwg) * PAYW);
            const bool sw = pay[2] > pay[4];            // the record is in the winner's orientation (a = its run node)
            i = sw ? pay[1] : pay[0]; j = sw ? pay[0] : pay[1];
            sma = sw ? pay[5] : pay[3]; smb = sw ? pay[3] : pay[5];
            cab = pay[6]; css = pay[7];
        } else { i = pos_c[ma]; j = pos_c[mb]; }
        int L = (j - i) * dir_o;
        if (L < 0) L += n;
        const bool other = n - L < L;
        M = other ? n - L : L;
        const int first = other ? wrap(j + dir_o, n) : wrap(i + dir_o, n);
        lo = dir_o > 0 ? first : wrap(first - (M - 1), n);
        if (other) ndir = -dir_o;
        if constexpr (PAY) {
            // the four nodes around the reversed range and the two new edge costs follow from the
            // record: no further memory trip
            if (!other) { if (dir_o > 0) { x0 = ma; x1 = sma; x2 = mb; x3 = smb; } else { x0 = smb; x1 = mb; x2 = sma; x3 = ma; } }
            else        { if (dir_o > 0) { x0 = mb; x1 = smb; x2 = ma; x3 = sma; } else { x0 = sma; x1 = ma; x2 = smb; x3 = mb; } }
            wA = dir_o > 0 ? cab : css; wB = dir_o > 0 ? css : cab;
        } else {
            // int32 / f64 cells: three dependent scalar trips (pos, ord, matrix).  A record as above was tried for them
            // too (round 2): the workgroup that found the pair has to be identified from the partials (an LDS exchange
            // and a barrier in every workgroup's prologue) and the record costs every workgroup two barriers at its
            // end -- 31.6 vs 30.9 us (f64), 21.1 vs 20.5 us (int32) per launch at n=4096: the scalar trips are cheap
            // while nothing else is in flight
            x0 = ord_c[wrap(lo - 1, n)]; x1 = ord_c[lo];
            x2 = ord_c[wrap(lo + M - 1, n)]; x3 = ord_c[wrap(lo + M, n)];
            wA = scalar_cell<T>(mat, (size_t)x0 * ld + x2);     // the two new edges {a,b}, {succ a, succ b}
            wB = scalar_cell<T>(mat, (size_t)x1 * ld + x3);
        }
    }
    auto new_cell = [&](int p) __attribute__((always_inline)) {   // old cell holding what cell p holds after the move
        int r = p - lo;
        if (r < 0) r += n;
        return r < M ? wrap(lo + M - 1 - r, n) : p;
    };

    // the run in TOUR order on the NEW state (thread j+1 takes array cell p0 + j, j = -1 .. cnt); this workgroup also
    // writes its cells of the new ord
    for (int j = tid - 1; j <= cnt; j += BT) {
        const int p = wrap(p0 + j, n);
        const int src = new_cell(p);
        int v = node_spec;
        if (src != p || j != tid - 1) v = ord_o[src];    // inside the reversed range (or a second round: tiny blocks)
        nodes[ndir > 0 ? j : cnt - j] = v;
        if (j >= 0 && j < cnt) A.F.ord[wr][tn + p] = v;
    }
    // Resident body, one chunk per thread: every row of the run is requested NOW, before the state derivation, which
    // needs nothing from memory any more and so runs under the rows' latency.  The explicit vmcnt(0) first: everything
    // loaded at entry has long arrived, and with it on the compiler's scoreboard the derivation below needs no wait of
    // its own -- without it the conditional load above makes the count unknown and the first use of an entry-loaded
    // register becomes a vmcnt(0) that waits for the rows (measured: 16.4 instead of 15.2 us per launch).
    VT R[D == 0 ? PMAX + 1 : 1][NCH];
    constexpr bool EARLY_ROWS = D == 0 && NCH == 1;
    auto issue_rows = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r <= (D == 0 ? PMAX : 0); r++) {
            if (r <= cnt && A.ablate != 2) {
                const VT *src = reinterpret_cast<const VT *>(mat + (size_t)nodes[r] * ld);
#pragma unroll
                for (int c = 0; c < NCH; c++) R[r][c] = src[min(c * BT + tid, nvec - 1)];
            }
        }
    };
    if constexpr (EARLY_ROWS) {
        __syncthreads();                               // nodes[] visible
        __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0), gfx9 encoding (expcnt 7, lgkmcnt 15: not waited for)
        issue_rows();
    }

    // per-thread state of the owned b's on the NEW state, from coalesced loads of the old one:
    // a node inside the reversed range swaps its left/right neighbour (and edge cost); the four
    // nodes around the range ends get one new neighbour.  No gather, no dependence on the move
    // beyond scalars.  Every thread needs only succ b and c[b][succ b] of its b's -- one range test
    // and two selects per b (the successor is the RIGHT neighbour iff the direction is forward XOR
    // the node sits inside the reversed range); the two nodes whose successor is new, and the lanes
    // past the row, are patched in a branch almost no wave takes.  The full new record (position,
    // both neighbours, both edge costs) is derived and stored only by the thread that owns the slice.
    static_assert(HOIST, "the fused kernels are instantiated for NCH * V <= 16 only");
    BState<T, NCH> B;
    B.skm = 0;
    const bool fwd = ndir > 0;
    const int wrap_end = lo + M - n;                      // > 0 only when the reversed range wraps round the array end
    const int spA = move ? (fwd ? x0 : x2) : -1, spA_s = fwd ? x2 : x0;    // successor spA_s over an edge of cost wA
    const int spB = move ? (fwd ? x1 : x3) : -1, spB_s = fwd ? x3 : x1;    // successor spB_s over an edge of cost wB
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const int ub0 = (c * BT + tid) * V;
#pragma unroll
        for (int v = 0; v < V; v++) {
            int q_o, sb;
            AT dn;
            if constexpr (PAY) q_o = (int)q16[c][v]; else q_o = qv[c][v];
            const bool inr = ((unsigned)(q_o - lo) < (unsigned)M) | (q_o < wrap_end);
            const bool use_r = inr != fwd;
            if constexpr (PAY) {
                const unsigned w = (unsigned)lv[c][v], d = (unsigned)dlv[c][v];
                sb = (int)((use_r ? w >> 16 : w) & 0xffffu);
                dn = (AT)((use_r ? d >> 16 : d) & 0xffffu);
            } else { sb = use_r ? rv[c][v] : lv[c][v]; dn = use_r ? drv[c][v] : dlv[c][v]; }
            bstate_set<T, NCH>(B, c, v, sb, dn, false, false);
        }
        if (((unsigned)(spA - ub0) < (unsigned)V) | ((unsigned)(spB - ub0) < (unsigned)V) | (ub0 + V > n)) {
#pragma unroll
            for (int v = 0; v < V; v++) {
                const int b = ub0 + v;
                if (b == spA) bstate_set<T, NCH>(B, c, v, spA_s, wA, false, false);
                if (b == spB) bstate_set<T, NCH>(B, c, v, spB_s, wB, false, false);
                if (b >= n) bstate_set<T, NCH>(B, c, v, 0, (AT)0, true, false);
            }
        }
    }
    // the new records of the workgroup's slice of nodes, one node per slice lane
    for (int sl = tid - S0; sl >= 0 && sl < slice; sl += BT - S0) {
        const int b = (int)blockIdx.x * slice + sl;
        if (b >= n) break;
        if (sl != tid - S0) load_slice(b);               // (a second round: slices longer than the lanes, tiny blocks)
        int r = sq - lo;
        if (r < 0) r += n;
        const bool inr = r < M;
        const int qn = inr ? wrap(lo + M - 1 - r, n) : sq;
        int l2 = inr ? sr_o : sl_o, r2 = inr ? sl_o : sr_o;
        AT dl2 = inr ? sdr : sdl, dr2 = inr ? sdl : sdr;
        if (move) {
            if (b == x0) { r2 = x2; dr2 = wA; }
            if (b == x3) { l2 = x1; dl2 = wB; }
            if (b == x1) { r2 = x3; dr2 = wB; }
            if (b == x2) { l2 = x0; dl2 = wA; }
        }
        if constexpr (PAY) {
            (reinterpret_cast<u16 *>(A.F.pos[wr]) + tn)[b] = (u16)qn;
            (reinterpret_cast<unsigned *>(A.F.nl[wr]) + tn)[b] = (unsigned)l2 | ((unsigned)r2 << 16);
            (reinterpret_cast<unsigned *>(A.F.dl[wr]) + tn)[b] = (unsigned)dl2 | ((unsigned)dr2 << 16);
        } else {
            A.F.pos[wr][tn + b] = qn; A.F.nl[wr][tn + b] = l2; A.F.nr[wr][tn + b] = r2;
            reinterpret_cast<AT *>(A.F.dl[wr] + tn)[b] = dl2;
            reinterpret_cast<AT *>(A.F.dr[wr] + tn)[b] = dr2;
        }
    }
    if (blockIdx.x == 0 && tid == 0) {                   // per-tour scalars of the new state
        const double cost_n = cost_o + (move ? md : 0.0);
        A.F.dir[wr][t] = ndir; A.F.k[wr][t] = k_done + (last ? 0 : 1); A.F.cost[wr][t] = cost_n;
        A.F.stop[wr][t] = last ? 1 : 0;
        A.S.nsweeps[t] = k_done + (last ? 0 : 1);
        if (move) {
            A.S.last_delta[t] = md;
            if (t == 0 && k_done <= A.hist.cap) { A.hist.a[k_done - 1] = ma; A.hist.b[k_done - 1] = mb; A.hist.d[k_done - 1] = md; }
        }
    }
    if (last) return;   // sweep cap reached: the move is applied and recorded, no further sweep (the next launch raises `done`)
    if constexpr (!EARLY_ROWS) __syncthreads(); // nodes[] visible
    if (stamp && tid == 0) { stamp[0] = t_entry; stamp[5] = t_red; }
    STAMP(1);

    Best q;
    best_init<false>(q);
    if constexpr (D >= 4) {      // 4: one pair of rows in flight, 5: two
        pipe_stream2<T, NCH, D - 3>(q, A, B, rows, nodes, (unsigned)(uintptr_t)(lds_u8 *)smem, cnt, stamp);
    } else if constexpr (D > 0) {
        pipe_stream<T, NCH, D, false>(q, A, B, rows, nodes, (unsigned)(uintptr_t)(lds_u8 *)smem, cnt, 0, 0, stamp);
    } else {
    // every row of the run in flight at once (one chunk per thread: since before the state derivation)
    if constexpr (!EARLY_ROWS) issue_rows();
    const int wave_base = __builtin_amdgcn_readfirstlane(tid & ~63);
    const unsigned lds0 = (unsigned)(uintptr_t)(lds_u8 *)smem;

    auto step = [&](int s) __attribute__((always_inline)) {
        const int a = __builtin_amdgcn_readfirstlane(nodes[s]);
        const int am = __builtin_amdgcn_readfirstlane(nodes[s - 1]);
        const int sa = __builtin_amdgcn_readfirstlane(nodes[s + 1]);
        const T *bA = rows + (size_t)s * ld;
        const unsigned char *bS = reinterpret_cast<const unsigned char *>(rows + (size_t)(s + 1) * ld);
        const unsigned ldsS = lds0 + (unsigned)((s + 1) * ld) * (unsigned)sizeof(T);
        if (stamp && tid == 0 && s < 24) stamp[8 + s] = wall_clock64();
        if (A.ablate == 1) return;
        sweep_step_as<T, NCH, false, true>(q, B, bA, bS, ldsS, a, am, sa, n, ld, BT, tid, wave_base, true);
    };

    // Rows land in chunks of RPC; after each chunk one barrier, then every step whose two rows
    // are in LDS runs while the later rows are still in flight (3 barriers in all for P = 8).
    // (group ends, exclusive: rows [0,3) [3,6) [6,9).  Measured at n=4096 uint16, us per launch: 3,6,9 14.40; 4,7,9
    // 14.40; 3,5,7,9 14.69; 3,6,8,9 14.73; 2,4,6,8,9 14.85 -- a fourth barrier costs more than the shorter tail after
    // the last row saves.  -DTSPGPU_RGROUPS=... to compare.)
#ifndef TSPGPU_RGROUPS
#define TSPGPU_RGROUPS 3, 6, 9
#endif
    {
        constexpr int ends[] = {TSPGPU_RGROUPS};
        constexpr int NG = (int)(sizeof(ends) / sizeof(ends[0]));
        static_assert(ends[NG - 1] == PMAX + 1, "the row groups must cover the PMAX + 1 rows of a run");
        int s = 0;
#pragma unroll
        for (int g = 0; g < NG; g++) {
            const int r0 = g == 0 ? 0 : ends[g - 1];
#pragma unroll
            for (int r = r0; r < ends[g]; r++) {
                if (r <= cnt && A.ablate != 2) {
                    VT *dst = reinterpret_cast<VT *>(rows + (size_t)r * ld);
#pragma unroll
                    for (int c = 0; c < NCH; c++) dst[min(c * BT + tid, nvec - 1)] = R[r][c];
                }
            }
            __syncthreads();
            if (g == 0) STAMP(2);
            const int s_end = min(cnt, ends[g] - 1);   // steps s with row s+1 < ends[g]
            for (; s < s_end; s++) step(s);
        }
    }

    }

    STAMP(3);
    double d;
    u64 key;
    const bool winner = block_best<T, false>(q, d, key, scratch);
    // uint16 cells: exactly one thread of the workgroup holds the workgroup's best pair (a pair is evaluated once): it
    // leaves the geometry record of that pair -- everything it has in registers and LDS anyway -- and takes part in the
    // tour-wide atomic min; other cells: thread 0 leaves the partial the next launch reduces
    if (PAY && key != 0) {                    // (workgroup-uniform: the block's best pair, if it found an improving one)
        int *xch = reinterpret_cast<int *>(scratch + 16);      // 16 ints of slack behind the reduction scratch
        const int la = (int)(key >> 32), lb = (int)(key & 0xffffffffu);      // la < lb
        int own = -1, idx = 0, other = 0;
        if (winner) {
            // which of the two labels is the thread's own b (the other one is the run node a).  With several chunks per
            // thread BOTH can be own b's -- la in one chunk, lb in another (|lb - la| within V of a multiple of BT * V) --:
            // then the orientation that was evaluated follows from the block rule of sweep_step_as (same block: b > a;
            // else the pair belongs to the a whose block has b's block less than half way round ahead of it).
            int idx_a = -1, idx_b = -1;
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const int b0c = (c * BT + tid) * V;
                if ((unsigned)(lb - b0c) < (unsigned)V) idx_b = c * V + (lb - b0c);
                if ((unsigned)(la - b0c) < (unsigned)V) idx_a = c * V + (la - b0c);
            }
            bool own_is_b = idx_b >= 0;
            if (idx_a >= 0 && idx_b >= 0) {
                const int NBk = (n + 64 * V - 1) / (64 * V), blka = la / (64 * V), blkb = lb / (64 * V);
                int dblk = blkb - blka;                 // (la < lb: dblk >= 0)
                own_is_b = dblk == 0 || 2 * dblk < NBk || (2 * dblk == NBk && blka < blkb);   // a = la evaluated b = lb
            }
            own = own_is_b ? lb : la; idx = own_is_b ? idx_b : idx_a;
            other = own_is_b ? la : lb;
            xch[0] = other;
        }
        // where in the run the pair's run node sits: one compare per thread instead of a serial walk by the winner
        __syncthreads();
        if (tid < cnt && nodes[tid] == xch[0]) xch[1] = tid;
        __syncthreads();
        if (winner) {
            unsigned pk = 0;
            int q_old = 0;                        // old array cell of the own node; its new cell follows from the move
#pragma unroll
            for (int c = 0; c < NCH; c++)
#pragma unroll
                for (int v = 0; v < V; v++)
                    if (c * V + v == idx) { pk = (unsigned)B.sb[c][v]; if constexpr (PAY) q_old = (int)q16[c][v]; else q_old = qv[c][v]; }
            int qr = q_old - lo;
            if (qr < 0) qr += n;
            const unsigned qq = (unsigned)(qr < M ? wrap(lo + M - 1 - qr, n) : q_old);
            const int sb = (int)(PAY ? pk & 0xffffu : pk) / (int)sizeof(T);
            const int sidx = xch[1];
            const int sa = nodes[sidx + 1];
            const int cell_a = wrap(p0 + (ndir > 0 ? sidx : cnt - sidx), n);
            AT w1, w2;
            if constexpr (D == 0) { w1 = (AT)rows[(size_t)sidx * ld + own]; w2 = (AT)rows[(size_t)(sidx + 1) * ld + sb]; }
            else { w1 = (AT)mat[(size_t)other * ld + own]; w2 = (AT)mat[(size_t)sa * ld + sb]; }
            int *pay = A.F.payload[wr] + ((size_t)t * A.S.pstride + blockIdx.x) * PAYW;
            *reinterpret_cast<v4i32 *>(pay) = v4i32{cell_a, (int)qq, other, sa};
            if constexpr (sizeof(AT) == 8) {
                pay[4] = own; pay[5] = sb;
                *reinterpret_cast<double *>(pay + 6) = w1;
                *reinterpret_cast<double *>(pay + 8) = w2;
            } else *reinterpret_cast<v4i32 *>(pay + 4) = v4i32{own, sb, (int)w1, (int)w2};
            if constexpr (PAY) {
                const long long K = ((long long)(int)d << 45) | ((long long)la << 29) | ((long long)lb << 13) | (long long)blockIdx.x;
                atomicMin(A.F.bestkey + t * 4 + k_done % 3, K);
            }
        }
    }
    if constexpr (!PAY) {
        if (tid == 0) {
            Partial o; o.d = d; o.key = key;
            A.F.partial[wr][(size_t)t * A.S.pstride + blockIdx.x] = o;
        }
    }
    STAMP(4);
#undef STAMP
}

// ---------------------------------------------------------------------------
// Matrix-free ("on the fly") sweep: for instances whose matrix row does not fit LDS or whose
// n x n matrix should not be built at all (BASELINE config 5: pla85900, 59 GB of doubles in the
// reference's format).  Every c[i][j] is recomputed from the coordinates with the arithmetic
// of k_build_costs, so the trajectory is the matrix trajectory.
//
// Workgroup g owns RUN consecutive tour edges (a_t, a_t+1); the RUN+1 points of its nodes sit
// in LDS (broadcast reads).  A thread streams over b with coalesced loads of four per-node
// arrays -- P_b, P_succ(b) (gathered once per sweep by k_gather_spts), c[b][succ b], pos[b] --
// and evaluates pair (a_t, b) for every t whose ownership range contains b:
//     delta = w(P_a_t, P_b) + w(P_a_t+1, P_succ b) - (c[a_t][a_t+1] + c[b][succ b]).
// The per-b data is read once per RUN pairs; there is no n^2 operand, so the HBM roofline
// does not apply: the bound is VALU issue (two edge weights = two f64 squared lengths and two
// correctly rounded roots per pair).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_gather_spts(Tours S, int n, int slot0, const double2 *__restrict__ pts,
                                                     double2 *__restrict__ spts)
{
    const int t = slot0 + blockIdx.y;
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n || S.done[t]) return;
    spts[(size_t)blockIdx.y * n + b] = pts[S.succ[(size_t)t * n + b]];
}

__global__ void __launch_bounds__(256) k_gather_ispts(Tours S, int n, int slot0, const int2 *__restrict__ ipts, int2 *__restrict__ ispts)
{
    const int t = slot0 + blockIdx.y;
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n || S.done[t]) return;
    ispts[(size_t)blockIdx.y * n + b] = ipts[S.succ[(size_t)t * n + b]];
}

// ---------------------------------------------------------------------------
// Matrix-free sweep, second form (costs below 2^25, n < 131 072): a thread holds FOUR
// consecutive b's (their points, the points of their successors, c[b][succ b]: 16-byte loads),
// a wave 256 -- a block, so the block ownership of sweep_step() applies (a wave is wholly
// in, wholly out, or holds a's own block; the neighbours of a need no mask: their delta is
// exactly 0) -- and for a fixed a the labels of the four b's ascend with the slot number, so
// per pair ONE 32-bit min on (w1 + w2 - c[b][sb]) << 2 | v keeps the reference's tie order.
// Per pair that leaves the two weights and three integer instructions.
// ---------------------------------------------------------------------------
using plan::OTF8_RUN;       // tour edges per workgroup, and with integer points behind the early-out (tspgpu_plan.h)
using plan::OTF8_RUN_INT;
template <int KIND, bool TABU, bool EARLY = false>
__global__ void __launch_bounds__(256) k_sweep_otf8(SweepArgs A)
{
    // 4 b's per thread with double2 points (8 need > 128 registers: two waves per SIMD only); 8 with int2 points
    // (runs of 64 edges behind the early-out, where streaming the per-b arrays is what is left; the full evaluation of every
    // pair -- tabu, the diagnostic build -- is fastest with 16: 3.9 vs 5.0 ms per sweep on pla85900)
    constexpr int RUN = (!TABU && EARLY) ? OTF8_RUN_INT : OTF8_RUN, VB = KIND == KIND_CEIL_INT ? 8 : 4, VSH = KIND == KIND_CEIL_INT ? 3 : 2;
    __shared__ int nodes_s[RUN + 2];
    // CEIL_2D on integer coordinates: the points as int2 and the weight without f64 (edge_w_ceil_i)
    constexpr bool IPT = KIND == KIND_CEIL_INT;
    typedef typename std::conditional<IPT, int2, double2>::type PT;
    __shared__ PT npt[RUN + 1];
    __shared__ int dstep[RUN];
    __shared__ Partial scratch[16];
    const int n = A.n;
    const int t = A.slot0 + blockIdx.y;
    if (A.S.done[t]) return;
    const int tid = threadIdx.x, BT = blockDim.x;
    const int *ord = A.S.ord + (size_t)t * n;
    const int *succ = A.S.succ + (size_t)t * n;
    const int *dnb = dnb_of<int>(A.S, t, n);
    const PT *pts, *spts;
    if constexpr (IPT) { pts = A.ipts; spts = A.ispts + (size_t)blockIdx.y * n; }
    else { pts = A.pts; spts = A.spts + (size_t)blockIdx.y * n; }
    auto weight = [](const PT &u, const PT &v) __attribute__((always_inline)) {
        if constexpr (IPT) return edge_w_ceil_i(u.x, u.y, v.x, v.y);
        else return edge_w<KIND>(u.x, u.y, v.x, v.y);
    };
    const int dir = A.S.dir[t];
    int *nodes = nodes_s + 1;

    int iter = 0, tenure = 0;
    if constexpr (TABU) { iter = A.tabu->iter; tenure = A.tabu->tenure; }

    const int p0 = ((int)blockIdx.x + A.g0) * RUN;
    const int cnt = min(RUN, n - p0);
    if (tid <= cnt + 1) {
        const int i = tid - 1;
        const int v = ord[wrap(p0 + (dir > 0 ? i : cnt - i), n)];
        int flag = 0;
        if constexpr (TABU) flag = is_tabu(A.tabu_list, v, iter, tenure) ? TABU_NODE : 0;
        nodes[i] = v | flag;
        if (i >= 0) npt[i] = pts[v];
        if (i >= 0 && i < cnt) dstep[i] = dnb[v];      // c[a_i][succ a_i]
    }
    __syncthreads();

    long long best_k = TABU ? 0x7fffffffffffffffll : 0ll;   // (delta << 34 | min(a,b) << 17 | max(a,b)); 0 = no improving move
    const int wave_lane0 = __builtin_amdgcn_readfirstlane(tid & ~63);
    const int NB = (n + 64 * VB - 1) / (64 * VB);
    // the run's own boxes (see the early-out below): its a's, their successors, and the largest threshold of its steps
    typedef typename std::conditional<IPT, int, double>::type CT;      // coordinate type
    constexpr bool BOUND = !TABU && EARLY;
    // threshold of an edge (u, v) of weight w: a pair can only improve if one of its new edges is shorter than the old edge it is
    // bracketed with.  Integer ceil-sqrt weights: shorter means weight <= w - 1, i.e. squared distance <= (w - 1)^2; the other kinds:
    // a weight is a monotone function of the squared distance as the kernels compute it, so shorter needs a smaller squared
    // distance.  f32 with a 2^-18 margin (the tests below lose at most 2^-22).
    auto thr = [](const PT &u, const PT &v, int w) __attribute__((always_inline)) {
        if constexpr (IPT) { const float tq = (float)(w - 1); return w > 0 ? tq * tq * 1.000004f : -1.0f; }
        else { const double dx = v.x - u.x, dy = v.y - u.y; return (float)(dx * dx + dy * dy) * 1.000004f; }
    };
    auto gap = [](CT lo, CT hi, CT qlo, CT qhi) __attribute__((always_inline)) {      // distance between the intervals [lo, hi] and [qlo, qhi]
        if constexpr (IPT) return (float)max(max(lo - qhi, qlo - hi), 0);
        else return (float)fmax(fmax(lo - qhi, qlo - hi), 0.0);
    };
    CT rax0 = 0, rax1 = 0, ray0 = 0, ray1 = 0, rsx0 = 0, rsx1 = 0, rsy0 = 0, rsy1 = 0;
    float ta2run = -1.0f;
    if constexpr (BOUND) {
        rax0 = rax1 = npt[0].x; ray0 = ray1 = npt[0].y; rsx0 = rsx1 = npt[1].x; rsy0 = rsy1 = npt[1].y;
        for (int s = 0; s < cnt; s++) {
            const PT pa = npt[s], ps = npt[s + 1];
            rax0 = min(rax0, pa.x); rax1 = max(rax1, pa.x); ray0 = min(ray0, pa.y); ray1 = max(ray1, pa.y);
            rsx0 = min(rsx0, ps.x); rsx1 = max(rsx1, ps.x); rsy0 = min(rsy0, ps.y); rsy1 = max(rsy1, ps.y);
            ta2run = fmaxf(ta2run, thr(pa, ps, dstep[s]));
        }
    }

    for (int base = 0; base < n; base += BT * VB) {
        const int w0 = base + wave_lane0 * VB;           // this wave's first b
        if (w0 >= n) continue;
        const int b0 = base + tid * VB;
        PT pb[VB], sp[VB];
        int dn[VB];
        unsigned skm = 0;
#pragma unroll
        for (int v = 0; v < VB; v++) {
            const int bb = min(b0 + v, n - 1);
            pb[v] = pts[bb];
            sp[v] = spts[bb];
            dn[v] = dnb[bb];
            if constexpr (TABU)
                if (is_tabu(A.tabu_list, bb, iter, tenure) || is_tabu(A.tabu_list, succ[bb], iter, tenure)) skm |= 1u << v;
        }
        // Exact early-out (plain 2-opt, integer ceil-sqrt weights): delta = [w(a,b) - w(a,sa)] + [w(sa,sb) - w(b,sb)] < 0 needs one
        // bracket negative, and a weight is a monotone function of the squared distance: w(a,b) < w(a,sa) implies
        // d2(a,b) <= (w(a,sa) - 1)^2, w(sa,sb) < w(b,sb) implies d2(sa,sb) <= (w(b,sb) - 1)^2.  A wave-step none of whose 64 x VB
        // pairs passes either test holds no improving pair and skips the two roots and the remainders; the f32 squared
        // distances (relative error 2^-23; the thresholds carry a 2^-19 margin) are the ones the weights start from anyway.
        // Same argmin: only pairs with delta >= 0 are left out, and those can never be chosen (refinment.c:63, :74).
        // In front of the per-pair tests, per thread and step: the same two tests against the BOUNDING BOXES of the thread's VB b's and
        // of their successors (a lower bound of every pair's squared distance against the largest threshold) -- consecutive node
        // indices are neighbours in most instance files, so one box test stands for VB pair tests.
        float tb2[BOUND ? VB : 1], tb2max = -1.0f;
        CT bx0 = 0, bx1 = 0, by0 = 0, by1 = 0, sx0 = 0, sx1 = 0, sy0 = 0, sy1 = 0;
        if constexpr (BOUND) {
            bx0 = bx1 = pb[0].x; by0 = by1 = pb[0].y; sx0 = sx1 = sp[0].x; sy0 = sy1 = sp[0].y;
#pragma unroll
            for (int v = 0; v < VB; v++) {
                tb2[v] = thr(pb[v], sp[v], dn[v]);
                tb2max = fmaxf(tb2max, tb2[v]);
                bx0 = min(bx0, pb[v].x); bx1 = max(bx1, pb[v].x); by0 = min(by0, pb[v].y); by1 = max(by1, pb[v].y);
                sx0 = min(sx0, sp[v].x); sx1 = max(sx1, sp[v].x); sy0 = min(sy0, sp[v].y); sy1 = max(sy1, sp[v].y);
            }
            // ... and the whole run at once: the b box against the box of the run's a's under its largest threshold, the
            // successor box against the box of the run's successors: a chunk far from the run skips its RUN steps together
            {
                const float ax = gap(bx0, bx1, rax0, rax1), ay = gap(by0, by1, ray0, ray1);
                const float ux = gap(sx0, sx1, rsx0, rsx1), uy = gap(sy0, sy1, rsy0, rsy1);
                const bool maybe = (__builtin_fmaf(ay, ay, ax * ax) <= ta2run) | (__builtin_fmaf(uy, uy, ux * ux) <= tb2max);
                if (!__ballot(maybe) || A.ablate == 6) continue;
            }
        }
        const int blkb = w0 / (64 * VB);
#pragma unroll 16
        for (int s = 0; s < RUN; s++) {               // (RUN = 16: fully unrolled)
            if (s >= cnt) break;
            const int a_raw = __builtin_amdgcn_readfirstlane(nodes[s]), sa_raw = __builtin_amdgcn_readfirstlane(nodes[s + 1]);
            if constexpr (TABU) { if ((a_raw | sa_raw) & TABU_NODE) continue; }
            const int a = a_raw & NODE_MASK, sa = sa_raw & NODE_MASK;
            const int am = __builtin_amdgcn_readfirstlane(nodes[s - 1]) & NODE_MASK;
            int d = blkb - a / (64 * VB);
            if (d < 0) d += NB;
            const bool self = d == 0;
            if (!self && !(2 * d < NB || (2 * d == NB && a / (64 * VB) < blkb))) continue;   // the other orientation's
            const bool hit = TABU && ((unsigned)(am - w0) < (unsigned)(64 * VB) || (unsigned)(sa - w0) < (unsigned)(64 * VB));
            const bool clean = !self && !hit && w0 + 64 * VB <= n;
            const PT pa = npt[s], ps = npt[s + 1];
            unsigned vmask = (1u << VB) - 1u;               // slots v some lane of which may hold an improving pair
            if constexpr (BOUND) {
                const float ta2 = thr(pa, ps, dstep[s]);
                {   // boxes first
                    const float ax = gap(bx0, bx1, pa.x, pa.x), ay = gap(by0, by1, pa.y, pa.y);
                    const float ux = gap(sx0, sx1, ps.x, ps.x), uy = gap(sy0, sy1, ps.y, ps.y);
                    const bool maybe = (__builtin_fmaf(ay, ay, ax * ax) <= ta2) | (__builtin_fmaf(uy, uy, ux * ux) <= tb2max);
                    if (!__ballot(maybe) || A.ablate == 4) continue;      // (4, 5, 6: diagnostics -- nothing behind the box / pair / run tests)
                }
                vmask = 0;
#pragma unroll
                for (int v = 0; v < VB; v++) {
                    const float fx = (float)(pb[v].x - pa.x), fy = (float)(pb[v].y - pa.y);
                    const float gx = (float)(sp[v].x - ps.x), gy = (float)(sp[v].y - ps.y);
                    const bool pass = (__builtin_fmaf(fy, fy, fx * fx) <= ta2) | (__builtin_fmaf(gy, gy, gx * gx) <= tb2[v]);
                    vmask |= __ballot(pass) ? 1u << v : 0u;
                }
                if (!vmask || A.ablate == 5) continue;
            }
            auto pairs = [&](auto check_tag) __attribute__((always_inline)) {
                constexpr bool CHECK = decltype(check_tag)::value;
                int m = 0x7fffffff;
#pragma unroll
                for (int v = 0; v < VB; v++) {
                    if constexpr (BOUND) { if (!((vmask >> v) & 1u)) continue; }    // (wave-uniform)
                    int dl = weight(pa, pb[v]) + weight(ps, sp[v]) - dn[v];
                    if constexpr (CHECK) {
                        const int b = b0 + v;
                        const bool ok = ((b > a) | !self) & (b < n) & (!TABU | ((b != am) & (b != sa)));
                        dl = ok ? dl : MASKED32;
                    }
                    if constexpr (TABU) dl = ((skm >> v) & 1u) ? MASKED32 : dl;
                    m = min(m, (dl << VSH) | v);
                }
                if (m == 0x7fffffff) return;                  // (every slot filtered out in every lane... cannot happen with vmask != 0)
                const int b = b0 + (m & (VB - 1));
                const long long key = ((long long)((m >> VSH) - dstep[s]) << 34) | ((long long)min(a, b) << 17) | (long long)max(a, b);
                best_k = key < best_k ? key : best_k;
            };
            if (clean) pairs(std::false_type{}); else pairs(std::true_type{});
        }
    }
    const int bd = (int)(best_k >> 34);
    const int la = (int)((best_k >> 17) & 0x1ffff), lb = (int)(best_k & 0x1ffff);
    const bool have = TABU ? bd < MASKED32 / 2 : bd < 0;
    double d = (double)bd;
    u64 key;
    if (!have) { d = TABU ? DBL_MAX : 0.0; key = TABU ? KEY_NONE : 0; }
    else key = ((u64)(unsigned)la << 32) | (unsigned)lb;
    block_argmin(d, key, scratch);
    if (tid == 0) {
        Partial o; o.d = d; o.key = key;
        A.S.partial[(size_t)t * A.S.pstride + blockIdx.x + A.g0] = o;
    }
}

template <bool TABU>
__global__ void __launch_bounds__(256) k_sweep_otf(SweepArgs A)
{
    constexpr int RUN = 8;
    __shared__ int nodes_s[RUN + 2];
    __shared__ double2 npt[RUN + 1];
    __shared__ int dstep[RUN];
    __shared__ Partial scratch[16];
    const int n = A.n;
    const int t = A.slot0 + blockIdx.y;
    if (A.S.done[t]) return;
    const int tid = threadIdx.x, BT = blockDim.x;
    const int *ord = A.S.ord + (size_t)t * n;
    const int *pos = A.S.pos + (size_t)t * n;
    const int *succ = A.S.succ + (size_t)t * n;
    const int *dnb = dnb_of<int>(A.S, t, n);
    const double2 *pts = A.pts;
    const double2 *spts = A.spts + (size_t)blockIdx.y * n;
    const int dir = A.S.dir[t];
    const int kind = A.kind;
    int *nodes = nodes_s + 1;

    int iter = 0, tenure = 0;
    if constexpr (TABU) { iter = A.tabu->iter; tenure = A.tabu->tenure; }

    const int p0 = ((int)blockIdx.x + A.g0) * RUN;
    const int cnt = min(RUN, n - p0);
    if (tid <= cnt + 1) {
        const int i = tid - 1;
        const int v = ord[wrap(p0 + (dir > 0 ? i : cnt - i), n)];
        nodes[i] = v;
        if (i >= 0) npt[i] = pts[v];
        if (i >= 0 && i < cnt) dstep[i] = dnb[v];      // c[a_i][succ a_i]
    }
    __syncthreads();

    const int BIG = 1 << 29;
    int best_d = TABU ? INT_MAX : 0;
    int best_a = 0, best_b = 0;
    bool have = false;
    const int wave_lane0 = __builtin_amdgcn_readfirstlane(tid & ~63);

    for (int base = 0; base < n; base += BT) {
        const int b = base + tid;
        const bool inb = b < n;
        const int bb = inb ? b : n - 1;
        const double2 pb = pts[bb];
        const double2 sp = spts[bb];
        int dn = dnb[bb];
        const int qb = pos[bb];
        if constexpr (TABU) {
            if (inb && (is_tabu(A.tabu_list, b, iter, tenure) || is_tabu(A.tabu_list, succ[bb], iter, tenure))) dn = -BIG;
        }
        if (!inb) dn = -BIG;
        int j = dir > 0 ? qb - p0 : p0 + cnt - qb;       // run index of b, if it is a node of this run
        if (j < -1) j += n;
        if (j > n - 2) j -= n;
        const int jl = ((j >= -1 && j <= cnt) ? j : 1 << 20) - 1;
        const int w0 = base + wave_lane0;                // this wave's first b
        if (w0 >= n) continue;
#pragma unroll
        for (int s = 0; s < RUN; s++) {
            if (s >= cnt) break;
            const int a = nodes[s];
            if constexpr (TABU) {
                if (is_tabu(A.tabu_list, a, iter, tenure) || is_tabu(A.tabu_list, nodes[s + 1], iter, tenure)) continue;
            }
            const int lo = a + 1 == n ? 0 : a + 1;
            const int len = (n & 1) ? (n - 1) / 2 : (a < n / 2 ? n / 2 : n / 2 - 1);
            int t0 = w0 - lo;
            if (t0 < 0) t0 += n;
            const bool nowrap = t0 + 64 <= n && w0 + 64 <= n;
            if (nowrap && t0 >= len) continue;           // wave entirely outside a's share
            bool ok = (unsigned)(s - jl) > 2u;           // not b in {pred a, a, succ a}
            if (!(nowrap && t0 + 64 <= len)) {
                int tt = b - lo;
                tt += (tt >> 31) & n;
                ok &= (unsigned)tt < (unsigned)len;
            }
            const double2 pa = npt[s], ps = npt[s + 1];
            const int made = (int)edge_weight(pa.x, pa.y, pb.x, pb.y, kind) + (int)edge_weight(ps.x, ps.y, sp.x, sp.y, kind);
            const int delta = made - (dstep[s] + dn);
            const bool lt = ok & (delta < best_d);
            bool eq = ok & (delta == best_d);
            if constexpr (!TABU) eq &= delta < 0;
            if (__ballot(eq)) {
                if (eq) {
                    const u64 kn = a < b ? ((u64)(unsigned)a << 32) | (unsigned)b : ((u64)(unsigned)b << 32) | (unsigned)a;
                    const u64 ko = best_a < best_b ? ((u64)(unsigned)best_a << 32) | (unsigned)best_b
                                                   : ((u64)(unsigned)best_b << 32) | (unsigned)best_a;
                    if (!have || kn < ko) { best_a = a; best_b = b; have = true; }
                }
            }
            best_d = lt ? delta : best_d;
            best_a = lt ? a : best_a;
            best_b = lt ? b : best_b;
            have = have | lt;
        }
    }
    double d = (double)best_d;
    u64 key;
    if (!have || best_d >= BIG / 2) { d = TABU ? DBL_MAX : 0.0; key = TABU ? KEY_NONE : 0; }
    else key = best_a < best_b ? ((u64)(unsigned)best_a << 32) | (unsigned)best_b : ((u64)(unsigned)best_b << 32) | (unsigned)best_a;
    __syncthreads();
    block_argmin(d, key, scratch);
    if (tid == 0) {
        Partial o; o.d = d; o.key = key;
        A.S.partial[(size_t)t * A.S.pstride + blockIdx.x + A.g0] = o;
    }
}

// ---------------------------------------------------------------------------
// K4 apply: one workgroup per tour.  Reduces the per-workgroup partials to the
// global (delta, a, b) and applies the move (see the Tours comment): reverse the
// shorter arc in ord/pos/dpos, toggle dir when that arc is not ref_reverse_path's
// succ_a .. b, write the two new boundary edge costs, update cost / sweep
// counter / done flag.  Four dependent memory round trips.
// TABU: always applies the best admissible move, stamps the tabu list, keeps
// the incumbent and advances the linear tenure policy.
// ---------------------------------------------------------------------------
struct ApplyArgs {
    Tours S;
    const void *mat;
    int n, ld, slot0, G, symmetric;
    const double2 *pts;  // matrix-free mode (mat == nullptr)
    int kind;
    int *tabu_list;      // TABU
    TabuState *tabu;     // TABU
    int *best_succ;      // TABU resident incumbent
    double *trace;       // TABU resident per-iteration costs (may be null)
    HistBuf hist;        // slot 0 move history (cap 0 = off)
};

template <typename T, bool TABU>
__global__ void __launch_bounds__(1024) k_apply(ApplyArgs A)
{
    __shared__ Partial scratch[16];
    const int n = A.n, ld = A.ld;
    const int t = A.slot0 + blockIdx.x;
    if (A.S.done[t]) return;
    const int tid = threadIdx.x, BT = blockDim.x;
    const T *mat = static_cast<const T *>(A.mat);

    double d = TABU ? DBL_MAX : 0.0;
    u64 key = TABU ? KEY_NONE : 0;
    const Partial *part = A.S.partial + (size_t)t * A.S.pstride;
    for (int g = tid; g < A.G; g += BT) {
        const Partial q = part[g];
        if (key_better(q.d, q.key, d, key)) { d = q.d; key = q.key; }
    }
    block_argmin(d, key, scratch);

    const int sweeps_now = A.S.nsweeps[t] + 1;
    const int cap = A.S.cap_sweeps[t];
    const bool move = TABU ? (key != KEY_NONE) : (d < TWO_OPT_EPS);
    const int a = (int)(key >> 32), b = (int)(key & 0xffffffffu);

    typedef typename Elem<T>::acc AT;
    int *ord = A.S.ord + (size_t)t * n, *pos = A.S.pos + (size_t)t * n;
    AT *dp = dpos_of<AT>(A.S, t, n);
    const int dir = A.S.dir[t];
    int ndir = dir; // direction after this move
    int sa = -1, sb = -1;
    if (move) {
        const int i = pos[a], j = pos[b];
        // forward arc succ_a .. b = positions i+dir, i+2dir, .., j  (L cells)
        int L = (j - i) * dir;
        if (L < 0) L += n;
        // flip the shorter arc; flipping the other one (succ_b .. a) needs dir toggled.
        // A non-symmetric matrix keeps the reference's arc: its edge costs are direction bound.
        const bool other = A.symmetric && (n - L < L);
        const int M = other ? n - L : L;
        const int first = other ? wrap(j + dir, n) : wrap(i + dir, n); // forward-first cell of the arc
        const int lo = dir > 0 ? first : wrap(first - (M - 1), n);     // lowest array cell of the arc
        // old neighbours of the arc (all read before anything moves)
        const int x0 = ord[wrap(lo - 1, n)], x1 = ord[lo];
        const int x2 = ord[wrap(lo + M - 1, n)], x3 = ord[wrap(lo + M, n)];
        sa = ord[wrap(i + dir, n)];
        sb = ord[wrap(j + dir, n)];
        int *succ = A.S.succ + (size_t)t * n;
        AT *dnb = dnb_of<AT>(A.S, t, n);
        if (other) ndir = -dir;
        if (A.symmetric) {
            // Node-indexed view, from the OLD arrays only (one independent round of loads): the
            // nodes of the reference's arc succ_a .. b now point at their old predecessors, over
            // the same edges (symmetric costs); succ_a and a get the two new edges below.
            // (four elements per thread per round: all loads first, then the stores -- the
            // stores go through pointers the compiler cannot prove distinct from the loads)
            for (int k0 = 2 + tid; k0 <= L; k0 += 4 * BT) {
                int vv[4], pr[4];
                AT ww[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int k = min(k0 + u * BT, L);
                    const int p = wrap(i + dir * k, n), pp = wrap(i + dir * (k - 1), n);
                    vv[u] = ord[p];
                    pr[u] = ord[pp];
                    ww[u] = dp[dir > 0 ? pp : p];   // edge between array cells pp and p
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {       // (a clamped duplicate rewrites the same values)
                    succ[vv[u]] = pr[u];
                    dnb[vv[u]] = ww[u];
                }
            }
            // the two new edges {a,b} and {succ a, succ b}: they are also the arc's boundary cells
            const AT wA = cell<T>(mat, A.pts, A.kind, ld, x0, x2), wB = cell<T>(mat, A.pts, A.kind, ld, x1, x3);
            const bool a_in_A = x0 == a || x2 == a;
            __syncthreads(); // every read of the old ord/dpos is complete
            // cells: swap k <-> M-1-k ; inner edges (M-1 of them): swap k <-> M-2-k
            for (int k = tid; k < M / 2; k += BT) {
                const int pk = wrap(lo + k, n), qk = wrap(lo + M - 1 - k, n);
                const int u = ord[pk], v = ord[qk];
                ord[pk] = v; ord[qk] = u;
                pos[v] = pk; pos[u] = qk;
            }
            for (int k = tid; k < (M - 1) / 2; k += BT) {
                const int pe = wrap(lo + k, n), qe = wrap(lo + M - 2 - k, n);
                const AT eu = dp[pe], ev = dp[qe];
                dp[pe] = ev; dp[qe] = eu;
            }
            if (tid == 0) {
                dp[wrap(lo - 1, n)] = wA;
                dp[wrap(lo + M - 1, n)] = wB;
                succ[a] = b;   dnb[a] = a_in_A ? wA : wB;
                succ[sa] = sb; dnb[sa] = a_in_A ? wB : wA;
                if (other) A.S.dir[t] = ndir;
            }
        } else {
            __syncthreads(); // everybody has read pos/ord before they change
            for (int k = tid; k < M / 2; k += BT) {
                const int pk = wrap(lo + k, n), qk = wrap(lo + M - 1 - k, n);
                const int u = ord[pk], v = ord[qk];
                ord[pk] = v; ord[qk] = u;
                pos[v] = pk; pos[u] = qk;
            }
            __syncthreads(); // cells final; re-read the costs of edges lo-1 .. lo+M-1 in tour direction
            for (int k = tid; k <= M; k += BT) {
                const int pe = wrap(lo - 1 + k, n);
                const int un = ord[pe], vn = ord[wrap(pe + 1, n)];
                dp[pe] = (AT)(dir > 0 ? mat[(size_t)un * ld + vn] : mat[(size_t)vn * ld + un]);
            }
            __syncthreads();
            for (int v = tid; v < n; v += BT) {   // direction-bound costs: rebuild the whole view
                const int qv = pos[v];
                succ[v] = ord[wrap(qv + ndir, n)];
                dnb[v] = dp[ndir > 0 ? qv : wrap(qv - 1, n)];
            }
        }
    }
    if constexpr (TABU) {
        TabuState *ts = A.tabu;
        const int iter = ts->iter;
        double cost_now = A.S.cost[t];
        if (move) cost_now += d;
        const bool improved = ts->resident && cost_now < ts->best_cost;
        __syncthreads(); // ord[]/dir final; all threads have read ts->iter / best_cost
        if (improved && A.best_succ) {
            const int *succ = A.S.succ + (size_t)t * n;
            for (int v = tid; v < n; v += BT) A.best_succ[v] = succ[v];
        }
        if (tid == 0) {
            if (move) {
                A.S.cost[t] = cost_now;
                A.tabu_list[a] = iter; A.tabu_list[b] = iter; A.tabu_list[sa] = iter; A.tabu_list[sb] = iter;
            }
            A.S.last_delta[t] = move ? d : 0.0;
            if (improved) ts->best_cost = cost_now;
            if (ts->resident && A.trace) A.trace[iter] = cost_now;
            // next iteration: linear policy, metaheuristic.c:40-59
            int tenure = ts->tenure, up = ts->up;
            if (tenure == ts->t_max || tenure == ts->t_min) up = !up;
            tenure += up ? 1 : -1;
            ts->tenure = tenure; ts->up = up; ts->iter = iter + 1;
            A.S.nsweeps[t] = sweeps_now;
            if (cap >= 0 && sweeps_now >= cap) A.S.done[t] = 1;
        }
    } else {
        if (tid == 0) {
            if (move) A.S.cost[t] += d;
            A.S.last_delta[t] = d;
            A.S.nsweeps[t] = sweeps_now;
            if (!move || (cap >= 0 && sweeps_now >= cap)) A.S.done[t] = 1;
            if (t == 0 && sweeps_now <= A.hist.cap) {
                A.hist.a[sweeps_now - 1] = move ? a : -1;
                A.hist.b[sweeps_now - 1] = move ? b : -1;
                A.hist.d[sweeps_now - 1] = d;
            }
        }
    }
}

__global__ void k_copy_tour(Tours S, int n, int dst, int src)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        S.ord[(size_t)dst * n + i] = S.ord[(size_t)src * n + i];
        S.pos[(size_t)dst * n + i] = S.pos[(size_t)src * n + i];
        S.dpos[(size_t)dst * n + i] = S.dpos[(size_t)src * n + i];
        S.succ[(size_t)dst * n + i] = S.succ[(size_t)src * n + i];
        S.dnb[(size_t)dst * n + i] = S.dnb[(size_t)src * n + i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        S.cost[dst] = S.cost[src]; S.last_delta[dst] = S.last_delta[src];
        S.dir[dst] = S.dir[src];
        S.done[dst] = S.done[src]; S.nsweeps[dst] = S.nsweeps[src];
        S.cap_sweeps[dst] = S.cap_sweeps[src]; S.status[dst] = S.status[src];
    }
}

__global__ void k_rearm(Tours S, int slot0, int count, int cap)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) { S.done[slot0 + i] = 0; S.nsweeps[slot0 + i] = 0; S.cap_sweeps[slot0 + i] = cap; }
}

// a slot that an earlier call left finished or at its sweep cap takes part again, its sweep count kept (the sharded sweep's
// two entry points: the caller decides when the descent ends)
__global__ void k_reopen(Tours S, int slot)
{
    S.done[slot] = 0; S.cap_sweeps[slot] = -1;
}

// the masked form: only the listed slots (a batch descent re-arms the tours still in it; a finished tour keeps done = 1)
__global__ void k_rearm_list(Tours S, const int *__restrict__ list, int count, int cap)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) { const int t = list[i]; S.done[t] = 0; S.nsweeps[t] = 0; S.cap_sweeps[t] = cap; }
}

// deadline drain of the one-launch-per-sweep path: the sweep cap of every unfinished tour := the sweeps it has
// completed, so that the next launch applies the pending move and stops (refinment.c:17-26: a sweep that ran is applied)
__global__ void k_cap_now(Tours S, int slot0, int count)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count && !S.done[slot0 + i]) S.cap_sweeps[slot0 + i] = S.nsweeps[slot0 + i];
}

#include "tspgpu_lds2opt.inc"
#include "tspgpu_lds2opt_win.inc"
#include "tspgpu_str2opt.inc"
#include "tspgpu_em.inc"
#include "tspgpu_oropt.inc"
#include "tspgpu_multi2opt.inc"
#include "tspgpu_nl2opt.inc"
#include "tspgpu_ornl.inc"
#include "tspgpu_nl3opt.inc"
#include "tspgpu_looks_dl.inc"
#include "tspgpu_greedy.inc"
#include "tspgpu_nlbatch.inc"
#include "tspgpu_nlbatch_dl.inc"
#include "tspgpu_nlvns.inc"
#include "tspgpu_hk.inc"

// ===========================================================================
// host side
// ===========================================================================
struct GraphEntry { int slot0, ntours, tabu, K; hipGraphExec_t exec; };

// ---- the memory of a context, by its four lifetimes ---------------------------------------------------------
// A group frees what it holds when it is reset and when the context is deleted.  Tours, Fused, M2Buf, NlBuf and HistBuf stay
// what the kernels take by value, structs of raw pointers; each has ONE table of rows (tspgpu_mem.h) or a tuple of owners
// next to it, and allocation, fill, copy and free all go through that.
#include "tspgpu_hipmem.h"
using tspmem::Row; using tspmem::Rows;
#define MEM_GROUP __attribute__((visibility("hidden")))     // (see tspgpu_mem.h)

struct MEM_GROUP ContextMem {             // until tspgpu_destroy: allocated on first use, grown or replaced in place
    DevBuf<int> d_flags;
    DevBuf<double2> d_pts;      // replaced by tspgpu_set_points
    DevBuf<int2> d_ipts;        // ceil_int(): the coordinates as integers relative to the bounding box's corner (k_sweep_otf8<KIND_CEIL_INT>)
    DevBuf<double2> d_spts;     // gathered successor points (ensure_spts)
    PinBuf<int> h_ord;          // pinned staging of load_path
    DevBuf<double> d_trace;     // tabu / VNS cost trace
    HistBuf hist{nullptr, nullptr, nullptr, 0};     // (a view the resident descent advances; the owners hold the arrays)
    DevBuf<int> hist_a, hist_b; DevBuf<double> hist_d;
    DevBuf<unsigned long long> d_stamps;
    DevBuf<u64> d_lp_slots; PinBuf<int> h_lp;       // LDS-resident descent: exchange slots, the control words behind them
    DevBuf<u16> d_lp_tmat;                          // ... [n][n] the matrix in tour order (the TM instantiations of k_lds2opt; filled by every launch)
    DevBuf<int> d_lp_best;      // tabu walk / VNS: the best tour by array cell [ld], its direction and flag [2]
    DevBuf<int> d_vns_rand;     // VNS: the caller's rand() values of a launch
    DevBuf<OrCtl> d_or;         // control block of the single-tour Or-opt
    DevBuf<M2Ctl> d_m2;         // ... of the parallel-move 2-opt
};

struct MEM_GROUP InstanceMem {            // of one n: new_instance drops it
    // parallel-move 2-opt (tspgpu_multi2opt.inc): the candidate arrays of the slot a descent runs on, on first use
    M2Buf m2{};
    // batched neighbour-list descent (tspgpu_nlbatch.inc): the candidate arrays and a control block per slot of a range of nlb_cap
    // slots; all of them allocated at the first batched call, or none
    M2Buf nlb{};
    NlbCtl *d_nlb_ctl = nullptr;
    int nlb_cap = 0;
    // ... with don't-look bits (tspgpu_nlbatch_dl.inc): a queue [n] and a look block per slot of a range of nlbq_cap slots, at the
    // first batched call with looks; both, or none.  They go where the candidate arrays go
    int *d_nlb_queue = nullptr;
    LookCtl *d_nlb_look = nullptr;
    int nlbq_cap = 0;
    // neighbour-list VNS (tspgpu_nlvns.inc): per walk a second order array, the incumbent and a control block, for nlv_cap walks;
    // the walks' number blocks and trace rows of the call in hand.  All of them, or none
    int *d_nlv_ord = nullptr, *d_nlv_best = nullptr;
    NlvCtl *d_nlv_ctl = nullptr;
    int nlv_cap = 0;
    DevBuf<int> d_nlv_rand; DevBuf<double> d_nlv_trace;
    // uniform grid over the points for the grid NN (k_nn_grid): built on the host in tspgpu_set_points
    DevBuf<double2> d_gxy; DevBuf<int> d_gidx, d_gpos, d_cstart, d_gcell;
    DevBuf<unsigned> d_knn;     // [n][NN_K] neighbour lists of k_nn_grid's KNN form (built at the first single-tour NN)
    int grid_G = 0; bool grid_ok = false;
    // don't-look bits (tspgpu_looks_dl.inc): the queue of looked units [n] and the control block of a phase with looks; both, with
    // the slots' sets (SlotMem::d_awake), at the first call of "Don't-look bits", or none
    int *d_lq = nullptr;
    LookCtl *d_look = nullptr;

    // greedy-edge construction (tspgpu_greedy.inc): best keys, adjacency, degrees, other_end, accept flags, the free list, the
    // rank buffers and the control block, 80 n bytes: all of them at the first construction, or none; dropped with the lists
    GeBuf ge{};
    Rows ge_rows(size_t n)
    {
        return {{&ge.bw, n * 8}, {&ge.be, n * 8}, {&ge.adj, n * 8}, {&ge.deg, n * 4}, {&ge.oe, n * 4}, {&ge.acc, n * 4}, {&ge.fl, n * 4},
                {&ge.nxt, n * 16}, {&ge.dist, n * 16}, {&ge.ctl, sizeof(GeCtl), 0, 0}};
    }
    void drop_greedy() { tspmem::free_rows<HipMem>(ge_rows(0)); }

    // Held-Karp lower bound (tspgpu_hk.inc): multipliers and pi*, labels, hooks, the nodes' and the components' best keys, degrees,
    // the tree's edges and the control block, 68 n bytes (+ 1.3 KB of slack behind the arrays the scan reads in vectors): all of
    // them at the first 1-tree, or none; dropped with the instance
    HkBuf hk{};
    Rows hk_rows(size_t n)
    {
        const size_t slack = 64;    // the scan reads pi[] and comp[] in vectors up to ld
        return {{&hk.pi, n * 8, slack * 8, 0}, {&hk.pibest, n * 8, slack * 8, 0}, {&hk.comp, n * 4, slack * 4, 0}, {&hk.up, n * 4}, {&hk.bw, n * 8},
                {&hk.be, n * 8}, {&hk.cw, n * 8}, {&hk.ce, n * 8}, {&hk.deg, n * 4}, {&hk.edges, n * 8}, {&hk.ctl, sizeof(HkCtl), 0, 0}};
    }
    void drop_hk() { tspmem::free_rows<HipMem>(hk_rows(0)); }

    Rows look_ctx_rows(size_t n) { return {{&d_lq, n * 4}, {&d_look, sizeof(LookCtl), 0, 0}}; }
    void drop_look_ctx() { tspmem::free_rows<HipMem>(look_ctx_rows(0)); }
    static Rows m2_rows(M2Buf &B, size_t n)
    {
        return {{&B.raw_d, n * 8}, {&B.raw_b, n * 4}, {&B.d, n * 8}, {&B.a, n * 4}, {&B.b, n * 4}, {&B.i, n * 4}, {&B.j, n * 4}, {&B.acc, n * 4}};
    }
    Rows nlb_rows(size_t n) { Rows r = m2_rows(nlb, n); r.push_back({&d_nlb_ctl, sizeof(NlbCtl)}); return r; }     // per slot
    Rows nlv_rows(size_t n) { return {{&d_nlv_ord, n * 4}, {&d_nlv_best, n * 4}, {&d_nlv_ctl, sizeof(NlvCtl)}}; }           // per walk
    void drop_nlv() { tspmem::free_rows<HipMem>(nlv_rows(0)); nlv_cap = 0; tspmem::reset_all(d_nlv_rand, d_nlv_trace); }
    Rows nlbq_rows(size_t n) { return {{&d_nlb_queue, n * 4}, {&d_nlb_look, sizeof(LookCtl)}}; }                           // per slot
    void drop_nlbq() { tspmem::free_rows<HipMem>(nlbq_rows(0)); nlbq_cap = 0; }
    void drop_nlb() { tspmem::free_rows<HipMem>(nlb_rows(0)); nlb_cap = 0; drop_nlbq(); drop_nlv(); }
    void drop_grid() { tspmem::reset_all(d_gxy, d_gidx, d_gpos, d_cstart, d_gcell, d_knn); grid_G = 0; grid_ok = false; }
    void reset() { tspmem::free_rows<HipMem>(m2_rows(m2, 0)); drop_look_ctx(); drop_greedy(); drop_hk(); drop_nlb(); drop_grid(); }
    ~InstanceMem() { reset(); }
};

struct MEM_GROUP CostMem {                // of one cost source: free_matrix drops it
    DevBuf<void> d_mat;         // [n][ld] cells of the kind in `elem`; empty in matrix-free mode
    // neighbour-list 2-opt (tspgpu_nl2opt.inc): the lists of the cost source in place (tspgpu_neighbours_build)
    NlBuf nl{};
    DevBuf<int> nl_node; DevBuf<double> nl_w;
    void drop_nl() { tspmem::reset_all(nl_node, nl_w); nl = NlBuf{}; }
    void reset() { drop_nl(); d_mat.reset(); }
};

struct MEM_GROUP SlotMem {                // of one slot capacity: ensure_tours replaces it as a whole, a new instance drops it
    int tcap = 0;
    Tours S{};
    int *d_starts = nullptr, *d_caps = nullptr;
    int *h_status = nullptr;    // pinned: done[tcap] then nsweeps[tcap]
    double *h_costs = nullptr;  // pinned [tcap]
    OrCtl *d_or_ctl = nullptr;  // Or-opt over a batch of tours: one control block per slot
    // the list of slots a launch of a batched descent works on (device, and its pinned staging): [tcap], either family's
    int *d_live = nullptr, *h_live = nullptr;
    // tabu, sized by n: allocated with the first slots and kept when they grow
    int *d_tabu_list = nullptr, *d_best_succ = nullptr;
    TabuState *d_tabu = nullptr;
    Fused F{};                  // fused path state (allocated on first use, capacity fcap)
    int fcap = 0;
    // don't-look bits: awake[slot][family][n] bytes for lcap slots (0: not allocated), grown with the slots; new slots are all awake
    unsigned char *d_awake = nullptr;
    int lcap = 0;
    Rows look_rows(size_t n) { return {{&d_awake, 3 * n, 0, 1, true}}; }
    void drop_looks() { tspmem::free_rows<HipMem>(look_rows(0)); lcap = 0; }

    // per slot; new slots are zero-filled (no sweep cap: 0xff) and the old ones copied
    Rows tour_rows(size_t n, size_t pstride)
    {
        const size_t slack = 64;    // vector reads of the last tour's tail (load_run)
        const int none = Row::NO_FILL; const bool keep = true, pinned = true;
        return {{&S.ord, n * 4, slack * 4, 0, keep}, {&S.pos, n * 4, slack * 4, 0, keep}, {&S.succ, n * 4, slack * 4, 0, keep},
                {&S.dpos, n * 8, slack * 8, 0, keep}, {&S.dnb, n * 8, slack * 8, 0, keep},
                {&S.dir, 4, 0, 0, keep}, {&S.cost, 8, 0, 0, keep}, {&S.last_delta, 8, 0, 0, keep}, {&S.done, 4, 0, 0, keep},
                {&S.nsweeps, 4, 0, 0, keep}, {&S.cap_sweeps, 4, 0, 0xff, keep}, {&S.status, 4, 0, 0, keep},
                {&S.partial, pstride * sizeof(Partial)},
                {&d_starts, 4}, {&d_caps, 4},
                {&d_tabu_list, 0, (n + 64) * 4},    // + slack: the sweeps read it with 16-byte vectors up to ld
                {&d_best_succ, 0, n * 4}, {&d_tabu, 0, sizeof(TabuState)},
                {&h_status, 4 * 2, 0, none, !keep, pinned}, {&h_costs, 8, 0, none, !keep, pinned},
                {&d_or_ctl, sizeof(OrCtl)},         // (armed at the start of every batched Or-opt phase)
                {&d_live, 4}, {&h_live, 4, 0, none, !keep, pinned}};
    }
    Rows fused_rows(size_t n, size_t pstride)
    {
        const size_t slack = 64;
        Rows r;
        for (int p = 0; p < 2; p++)
            r.insert(r.end(), {{&F.ord[p], n * 4, slack * 4}, {&F.pos[p], n * 4, slack * 4, 0}, {&F.nl[p], n * 4, slack * 4, 0},
                               {&F.nr[p], n * 4, slack * 4, 0}, {&F.dl[p], n * 8, slack * 8, 0}, {&F.dr[p], n * 8, slack * 8, 0},
                               {&F.dir[p], 4}, {&F.k[p], 4}, {&F.stop[p], 4}, {&F.cost[p], 8}, {&F.partial[p], pstride * sizeof(Partial)}});
        r.insert(r.end(), {{&F.cur, 4}, {&F.bestkey, 4 * 8},
                           {&F.payload[0], pstride * 16 * 4}, {&F.payload[1], pstride * 16 * 4}});      // 16 ints per workgroup record
        return r;
    }
    void drop_fused() { tspmem::free_rows<HipMem>(fused_rows(0, 0)); fcap = 0; }
    void reset() { tspmem::free_rows<HipMem>(tour_rows(0, 0)); drop_fused(); drop_looks(); S.pstride = 0; tcap = 0; }
    ~SlotMem() { reset(); }
};

struct M2Counters { long sweeps = 0, moves = 0, max_k = 0; };    // what tspgpu_info keeps of a parallel-move family's last call

struct tspgpu_ctx : ContextMem, InstanceMem, CostMem, SlotMem {
    int device = 0;
    hipStream_t stream = nullptr;
    int cus = 256;
    size_t lds_max = 65536;
    std::string err;

    // options
    int opt_elem = TSPGPU_ELEM_AUTO, opt_kernel = 0, opt_batch = 32, opt_wgs = 0, opt_hist = 0, opt_graph = 1,
        opt_timing = 0, opt_block = 0, opt_max_tours = 1024, opt_sweep_cap = -1;

    // instance
    int n = 0, ld = 0, kind = TSPGPU_EUC_2D;
    bool have_points = false, have_costs = false, symmetric = true;
    bool built = false;      // the matrix (or the matrix-free mode) comes from tspgpu_build_costs, not from a caller
    int elem = 0; // TSPGPU_ELEM_F64 / _I32 / _U16 in use
    bool otf = false;        // matrix-free: weights recomputed from d_pts
    int opt_otf = 0;         // 0 auto, 1 force matrix-free, 2 never
    int grid_max_occ = 0;
    double grid_x0 = 0, grid_y0 = 0, grid_cell = 1, grid_inv = 0, grid_eps = 0;
    int opt_nn = 0;          // 0 auto, 1 matrix / strided kernels, 2 grid kernel
    double cost_bound = 0;   // upper bound of any entry the uploaded points can produce
    bool int_coords = false; // every coordinate an integer below 2^25 in magnitude
    bool ceil_int() const { return kind == TSPGPU_CEIL_2D && int_coords && cost_bound < 4194304.0; }   // edge_w<KIND_CEIL_INT> applies

    // tours
    std::vector<unsigned char> slot_valid;   // [tcap] host side: the slot holds a complete tour state
    // don't-look bits: 1 = every node of the slot is awake in all three sets, whatever d_awake holds (a loaded slot, and any
    // slot a call outside "Don't-look bits" may have rewritten)
    std::vector<unsigned char> look_all;     // [tcap] host side
    hipEvent_t ev_ord = nullptr; bool ord_pending = false;   // guards the reuse of h_ord

    // launch plan (tspgpu_plan.h): kernel 0 = none; make_plan assigns it whole, drop_plan forgets it
    plan::Sweep plan;
    int opt_depth = 0, opt_ablate = 0, opt_stamps = 0;
    int opt_pipe2 = 1;          // 1 = the two-edge streaming form (pipe_stream2) where four rows fit LDS, 0 = never

    // LDS-resident descent (k_lds2opt): exchange slots + control words, allocated on first use
    int opt_persist = 1;       // 0 never, 1 where it applies (uint16 cells, one tour, n <= 4096, a whole idle chip), 2 or fail
    int opt_persist_edges = 0; // tour edges per workgroup (0 = auto)
    int opt_build_tile = 0;     // probe hook 92: 64 = the 64 x 64 tiles at every size
    int opt_build = 0;          // K1 for integer cells: 0 one triangle + transposed store (k_build_costs_tri), 1 every cell computed (k_build_costs_int)
    int opt_persist_window = 0; // 0 auto (half-window rows where whole rows do not fit the chip's LDS), 1 always, 2 never
    bool lp_window = false;    // ... and it was the half-window form (k_lds2opt_w)
    bool lp_handed = false;    // run_persist began a descent and handed the rest to the per-sweep path
    long lp_sweeps = 0;        // sweeps run by the launches of the last LDS-resident descent / walk
    int vns_mode = 0;          // the last tspgpu_vns_search: 1 resident throughout, 2 host kicks throughout, 3 resident launches first,
                               // then (the grid lost its co-residency) host kicks
    long opt_lp_hello = 200000; // rendezvous limit in 10 ns ticks
    int opt_lp_poll_sleep = 0;  // probe hook 95
    int opt_vns_launch_k = 65536;   // VNS iterations a launch may complete (test hook 94 lowers it to force relaunches)
    int opt_lp_fail_at = 0;     // test hook 96: the next N RE-launches of a descent (deadline runs relaunch per sweep budget) fail their rendezvous
    int vns_launch_nrand = 0;   // VNS: the caller's rand() values of a launch
    relaunch::Gate lp_gate;     // the grid did not come up co-resident: the next descents keep to the one-launch-per-sweep path
    bool lp_used = false;      // the last descent ran in k_lds2opt
    // streamed persistent descent (k_str2opt): single tours past the LDS-resident sizes, uint16 cells
    int opt_stream = 1;        // 0 never, 1 where it applies (uint16 cells, one tour, n past k_lds2opt_w, a whole idle chip), 2 or fail
    bool sp_used = false;      // the last descent ran in k_str2opt
    int opt_sp_nch = 0;        // probe hook 93
    int opt_otf_early = 0;         // hook 91: 0 automatic, 1 the early-out kernel for every matrix-free sweep, 2 never
    bool lp_shaped = false;    // the last LDS-resident descent ran in a shaped instantiation of k_lds2opt
    int opt_lp_generic = 0;    // undocumented (option 89): 1 = never a shaped instantiation
    bool lp_tmat = false;      // ... and it fetched moved rows from the tour-ordered copy (a TM instantiation)
    int opt_lp_no_tmat = 0;    // undocumented (option 88): 1 = the shaped instantiation that reloads moved rows from the matrix
    bool lp_packed = false;    // the last LDS-resident descent / tabu walk / VNS walk ran the packed 16-bit loop (pk in run_persist)
    bool max16k = false;       // every off-diagonal cell <= 16383 (packed 16-bit deltas cannot overflow)
    bool max8k = false;        // ... <= 8190 (the tabu form of the packed loop: a poisoned pair must exceed every valid delta)

    // Extra Mileage (tspgpu_em.inc)
    int opt_em_form = 0;       // 0 (default) and 2 one launch pair per step; 1 the one-launch form, or fail with code 8
    int em_form = 0;           // how the last construction ran: 1 resident, 2 per step
    long em_stale = 0, em_steps = 0;   // stale rescans and insertions of the last construction

    // Or-opt (tspgpu_oropt.inc)
    int or_batch_R = 0;        // positions per sweep workgroup in the first Or-opt round of the last batched descent
    // ... in matrix-free mode (k_oropt_sweep_otf): single tours only
    int opt_or_otf = 0;        // TSPGPU_OPT_OR_MATRIX_FREE: 0 refuse Or-opt in matrix-free mode (code 12), 1 run it from the points
    int opt_or_otf_early = 0;  // hook 90: 0 automatic, 1 the early-out form for every matrix-free Or-opt sweep, 2 never
    int or_otf_form = 0;       // how the last matrix-free Or-opt sweep ran: 0 none, 1 every candidate, 2 with the early-out
    int or_otf_R = 0;          // its tour positions per workgroup

    // the parallel-move families (M2Family): the last call's sweeps, moves and largest sweep (a descent: over its rounds or phases)
    M2Counters m2_count, nl_count, ornl_count, nl3_count;

    // neighbour-list 2-opt (tspgpu_nl2opt.inc)
    bool nl_dropped = false;   // a new cost source took the lists away (the refusal says so)
    long nl_polish_sweeps = 0; // the polish of the last neighbour-list phase
    // neighbour-list Or-opt (tspgpu_ornl.inc)
    int ornl_rounds = 0;       // rounds of the last tspgpu_local_search_nl
    // neighbour-list 3-opt (tspgpu_nl3opt.inc): the width asked for and W = min(width, K') in effect, and the 3-opt phases of
    // the last tspgpu_local_search_nl3
    int nl3_width = 0, nl3_w = 0;
    int nl3_phases = 0;
    // don't-look bits (tspgpu_looks_dl.inc): units looked at, full sweeps and the largest sweep that was not full of the last call
    long dl_looked = 0, dl_full = 0, dl_max_q = 0;
    long nlb_dl_looked = 0, nlb_dl_full = 0, nlb_dl_max_q = 0;  // the last batched descent with looks: sums and the maximum over its tours
    // greedy-edge construction (tspgpu_greedy.inc): the last one's rounds per phase, phase-1 edges, free nodes entering phase 2
    long ge_rounds1 = 0, ge_rounds2 = 0, ge_edges1 = 0, ge_free = 0;
    // Held-Karp lower bound (tspgpu_hk.inc): Boruvka rounds of the last 1-tree; iterations, reason and final h of the last ascent;
    // the LDS bytes per workgroup of the last 1-tree's scan (0: comp[] and pi[] came through L2)
    long hk_rounds = 0, hk_iters = 0, hk_reason = 0, hk_h = 0, hk_lds = 0;
    // batched neighbour-list descent (tspgpu_nlbatch.inc)
    long nlb_tours = 0, nlb_launches = 0, nlb_max_live = 0;     // the last batched descent: tours, sweeps launched, most tours in one
    long nlb_w3 = 0, nlb_three_sweeps = 0, nlb_three_moves = 0, nlb_three_max_k = 0;    // ... its 3-opt width in effect (0: none), 3-opt sweeps and
                                                                                        // moves over the tours, most moves of one tour's 3-opt sweep
    // neighbour-list VNS (tspgpu_nlvns.inc): the last call's walks, iterations completed, sweep rounds, most walks live in one, dry walks
    long nlv_walks = 0, nlv_iterations = 0, nlv_rounds = 0, nlv_max_live = 0, nlv_dry = 0;

    int opt_fused = 1;         // 1 = one launch per sweep where applicable

    std::vector<GraphEntry> graphs;
    std::vector<const void *> max_lds_fns;     // kernels whose maximum dynamic LDS is set already (ensure_max_lds)

    // timing
    std::vector<hipEvent_t> ev;
    double sweep_ms_total = 0; long sweep_launches = 0;
};

static int fail(tspgpu_ctx *c, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (c) c->err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(ctx, E_INTERNAL, "%s -> %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

static void drop_graphs(tspgpu_ctx *ctx)
{
    for (auto &g : ctx->graphs) hipGraphExecDestroy(g.exec);
    ctx->graphs.clear();
}

// no plan, and no captured launches of one (the other fields keep the last plan's values: tspgpu_info shows them until the next)
static void drop_plan(tspgpu_ctx *ctx) { ctx->plan.kernel = 0; drop_graphs(ctx); }

// what the plans read of the context (tspgpu_plan.h)
static plan::In plan_in(const tspgpu_ctx *ctx)
{
    plan::In in;
    in.cus = ctx->cus; in.lds_max = ctx->lds_max;
    in.n = ctx->n; in.ld = ctx->ld; in.elem = ctx->elem;
    in.otf = ctx->otf; in.symmetric = ctx->symmetric; in.has_matrix = ctx->d_mat.p != nullptr;
    in.int_points = ctx->ceil_int() && ctx->d_ipts.p != nullptr; in.cost_bound = ctx->cost_bound;
    in.opt_kernel = ctx->opt_kernel; in.opt_block = ctx->opt_block; in.opt_wgs = ctx->opt_wgs; in.opt_depth = ctx->opt_depth;
    in.opt_pipe2 = ctx->opt_pipe2; in.opt_ablate = ctx->opt_ablate; in.opt_otf_early = ctx->opt_otf_early;
    in.opt_persist_edges = ctx->opt_persist_edges; in.opt_persist_window = ctx->opt_persist_window; in.opt_sp_nch = ctx->opt_sp_nch;
    return in;
}

static void free_matrix(tspgpu_ctx *ctx)
{
    if (ctx->nl.K) ctx->nl_dropped = true;  // the neighbour lists belong to the old costs
    ctx->drop_greedy();                     // (the construction's scratch goes with them)
    ctx->CostMem::reset();
    ctx->have_costs = false;
    ctx->or_otf_form = ctx->or_otf_R = 0;
    std::fill(ctx->slot_valid.begin(), ctx->slot_valid.end(), 0);   // the slots' edge costs belong to the old matrix
    drop_graphs(ctx);
}

// room for `count` elements in a buffer whose address captured launches hold
template <class BUF> static int reserve_captured(tspgpu_ctx *ctx, BUF &buf, size_t count)
{
    if (count <= buf.n) return E_OK;
    drop_graphs(ctx);
    HIP_TRY(buf.reserve(count));
    return E_OK;
}

// Tour slots [0, want).  Growing keeps the contents of the slots that exist (a tour loaded into slot 0 survives a
// later tspgpu_tour_nn(20) or a multi-start); new slots are zero-filled and marked invalid until something is
// loaded / built / copied into them (slot_valid: the slot entry points answer FAILED_PRECONDITION otherwise).
// All or none: a failed allocation leaves the capacity, every array, the fused state and the captured graphs as they were.
static int ensure_tours(tspgpu_ctx *ctx, int want)
{
    if (want <= ctx->tcap) return E_OK;
    want = std::max(want, 16);
    const int pstride = std::max(MAX_WGS_PER_TOUR, (ctx->n + 7) / 8 + 8); // the matrix-free sweep runs n/8 workgroups per tour
    // (the awake sets first, where they exist: if the slots then fail to grow, the sets merely have room to spare)
    if (ctx->lcap && ctx->lcap < want) {
        HIP_TRY(tspmem::grow(HipMem{ctx->stream}, ctx->look_rows((size_t)ctx->n), (size_t)ctx->lcap, (size_t)want));
        ctx->lcap = want;
    }
    HIP_TRY(tspmem::grow(HipMem{ctx->stream}, ctx->tour_rows((size_t)ctx->n, (size_t)pstride), (size_t)ctx->tcap, (size_t)want));
    ctx->S.pstride = pstride;
    if (ctx->tcap) {
        ctx->drop_fused();        // sized by the slot count; only live inside a run
        drop_graphs(ctx);         // captured launches hold the old pointers
    }
    ctx->tcap = want;
    ctx->slot_valid.resize((size_t)want, 0);
    ctx->look_all.resize((size_t)want, 1);
    return E_OK;
}

// don't-look bits: the slots' tours were, or may have been, rewritten outside "Don't-look bits": every node is awake
static void wake_slots(tspgpu_ctx *ctx, int slot0, int count)
{
    for (int i = slot0; i < slot0 + count && i < (int)ctx->look_all.size(); i++) ctx->look_all[i] = 1;
}

static void mark_slots(tspgpu_ctx *ctx, int slot0, int count, bool valid)
{
    for (int i = slot0; i < slot0 + count && i < (int)ctx->slot_valid.size(); i++) ctx->slot_valid[i] = valid ? 1 : 0;
    wake_slots(ctx, slot0, count);
}

// a slot entry point was handed `slot`: it must exist and hold a tour
static int need_slot(tspgpu_ctx *ctx, int slot)
{
    if (slot < 0) return fail(ctx, E_INVALID, "slot %d is negative", slot);
    // (the slot array grows on demand and a new instance starts it empty: a slot past its end is a slot nothing was put into)
    if (slot >= ctx->tcap || !ctx->slot_valid[slot]) return fail(ctx, E_PRECOND, "slot %d holds no tour (load, build or copy one into it first)", slot);
    return E_OK;
}

// the slot list of the next launches of a batched descent: staged in pinned memory, so the stream must have drained the
// previous list first
static int set_live(tspgpu_ctx *ctx, const std::vector<int> &list)
{
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(ctx->h_live, list.data(), list.size() * 4);
    HIP_TRY(hipMemcpyAsync(ctx->d_live, ctx->h_live, list.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    return E_OK;
}

static int new_instance(tspgpu_ctx *ctx, int n)
{
    if (n < 4) return fail(ctx, E_INVALID, "need at least 4 nodes, got %d", n);
    if (n > 131072) return fail(ctx, E_INVALID, "n = %d: at most 131072 nodes", n);
    free_matrix(ctx);
    ctx->SlotMem::reset();
    ctx->InstanceMem::reset(); // (the grid is the old points': tspgpu_set_points builds the new one)
    ctx->slot_valid.clear();
    ctx->look_all.clear();
    drop_graphs(ctx);
    ctx->grid_max_occ = 0;
    ctx->n = n;
    ctx->ld = (n + 31) & ~31; // rows 128-byte aligned for both element kinds
    ctx->have_points = false;
    ctx->symmetric = true;
    return E_OK;
}

using plan::MATRIX_MAX_N;
using plan::elem_size;

// run `...` with T bound to the storage type of `elem`
#define ELEM_SWITCH(elem, T, ...)                                             \
    do {                                                                      \
        if ((elem) == TSPGPU_ELEM_F64) { typedef double T; __VA_ARGS__; }     \
        else if ((elem) == TSPGPU_ELEM_I32) { typedef int T; __VA_ARGS__; }   \
        else { typedef u16 T; __VA_ARGS__; }                                  \
    } while (0)

// f(kind, pts, spts) for the point kind of a matrix-free instance: `kind` a compile-time constant (kind()), pts the points and
// spts the gathered successor points, typed for it -- the int2 points of ceil_int() where they exist, as launch_sweep
template <typename F> static void kind_switch(const tspgpu_ctx *ctx, F &&f)
{
    double2 *const pts = ctx->d_pts, *const spts = ctx->d_spts;
    if (ctx->ceil_int() && ctx->d_ipts) f(std::integral_constant<int, KIND_CEIL_INT>{}, ctx->d_ipts.p, reinterpret_cast<int2 *>(spts));
    else if (ctx->kind == TSPGPU_EUC_2D) f(std::integral_constant<int, TSPGPU_EUC_2D>{}, pts, spts);
    else if (ctx->kind == TSPGPU_ATT) f(std::integral_constant<int, TSPGPU_ATT>{}, pts, spts);
    else f(std::integral_constant<int, TSPGPU_CEIL_2D>{}, pts, spts);
}

// one launch from whichever cost source the context has: K<T>(S, mat, n, ld, ...) or K_otf<KIND>(S, pts, n, ...)
#define LAUNCH_BY_COST(K, grid, block, ...)                                                                                               \
    do {                                                                                                                                  \
        if (ctx->otf) kind_switch(ctx, [&](auto kind, auto *pts, auto *) {                                                                \
            hipLaunchKernelGGL((K##_otf<kind()>), grid, block, 0, ctx->stream, ctx->S, pts, ctx->n, __VA_ARGS__); });                      \
        else ELEM_SWITCH(ctx->elem, T, hipLaunchKernelGGL((K<T>), grid, block, 0, ctx->stream, ctx->S, (const T *)ctx->d_mat.p, ctx->n,  \
                                                          ctx->ld, __VA_ARGS__));                                                         \
    } while (0)

// room for `points` gathered successor points
static int ensure_spts(tspgpu_ctx *ctx, size_t points)
{
    HIP_TRY(ctx->d_spts.reserve(points));
    return E_OK;
}

// the kernel `fn` may use all of a workgroup's LDS as dynamic LDS: set at the first launch of each kernel
static int ensure_max_lds(tspgpu_ctx *ctx, const void *fn)
{
    std::vector<const void *> &seen = ctx->max_lds_fns;
    if (std::find(seen.begin(), seen.end(), fn) != seen.end()) return E_OK;
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ctx->lds_max));
    seen.push_back(fn);
    return E_OK;
}

// at least `count` timing events in ctx->ev
static int ensure_events(tspgpu_ctx *ctx, int count)
{
    while ((int)ctx->ev.size() < count) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); ctx->ev.push_back(e); }
    return E_OK;
}

// K iterations of body(i) as one graph launch: captured the first time the key (slot0, ntours, tabu, K) is seen, then replayed
template <typename B> static int replay_graph(tspgpu_ctx *ctx, int slot0, int ntours, int tabu, int K, B &&body)
{
    hipGraphExec_t exec = nullptr;
    for (auto &g : ctx->graphs)
        if (g.slot0 == slot0 && g.ntours == ntours && g.tabu == tabu && g.K == K) exec = g.exec;
    if (!exec) {
        hipGraph_t graph;
        HIP_TRY(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
        int rc = E_OK;
        for (int i = 0; i < K && !rc; i++) rc = body(i);
        hipError_t ce = hipStreamEndCapture(ctx->stream, &graph);
        if (rc) return rc;
        if (ce != hipSuccess) return fail(ctx, E_INTERNAL, "graph capture failed: %s", hipGetErrorString(ce));
        HIP_TRY(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        hipGraphDestroy(graph);
        ctx->graphs.push_back({slot0, ntours, tabu, K, exec});
    }
    HIP_TRY(hipGraphLaunch(exec, ctx->stream));
    return E_OK;
}

// a control block to the device / `count` of them back, the stream drained (the host copy may sit on the caller's stack)
template <typename C> static int ctl_put(tspgpu_ctx *ctx, C *dev, const C &host)
{
    HIP_TRY(hipMemcpyAsync(dev, &host, sizeof(C), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return E_OK;
}
template <typename C> static int ctl_get(tspgpu_ctx *ctx, C *host, const C *dev, size_t count = 1)
{
    HIP_TRY(hipMemcpyAsync(host, dev, count * sizeof(C), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return E_OK;
}

// the mean time in ms of `reps` calls of body() on the engine's stream, behind one call of warm(); either returns a code, and
// any failure ends the measurement with it.  The events are destroyed on every way out
template <typename W, typename B> static int time_launches(tspgpu_ctx *ctx, int reps, W &&warm, B &&body, float *ms_mean)
{
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float ms = 0;
    auto timed = [&]() -> int {
        int rc;
        HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
        if ((rc = warm())) return rc;
        HIP_TRY(hipEventRecord(e0, ctx->stream));
        for (int i = 0; i < reps; i++) if ((rc = body())) return rc;
        HIP_TRY(hipEventRecord(e1, ctx->stream));
        HIP_TRY(hipEventSynchronize(e1));
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        return E_OK;
    };
    const int rc = timed();
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    if (!rc) *ms_mean = ms / reps;
    return rc;
}

using plan::SweepGeom;     // geometry of a candidate sweep (plan::sweep_geom: or_plan, m2_plan)

// --------------------------------------------------------------- launch plan
template <typename T, int NCH, int D, bool TABU> static const void *pipe_fn() { return (const void *)k_sweep_pipe<T, NCH, D, TABU>; }

// The selectors below name the kernels; WHICH (elem, nch) exist is plan::has_pipe2 / has_pipe / has_res / has_fused
// (tspgpu_plan.h), which every selector asks first and which the plan asks too.
// depth 9 = the two-edge form (pipe_stream2, four LDS row buffers): symmetric matrices, plain 2-opt, nch <= 3
static const void *pipe2_kernel(int elem, int nch)
{
    if (!plan::has_pipe2(elem, nch)) return nullptr;
    const void *fn = nullptr;
    ELEM_SWITCH(elem, T, fn = nch == 1 ? pipe_fn<T, 1, 9, false>() : pipe_fn<T, 2, 9, false>());
    if (nch == 3) fn = pipe_fn<u16, 3, 9, false>();
    return fn;
}

static const void *pipe_kernel(int elem, int nch, int depth, bool tabu)
{
    if (!plan::has_pipe(elem, nch)) return nullptr;
#define PK(T, N, DD) (tabu ? pipe_fn<T, N, DD, true>() : pipe_fn<T, N, DD, false>())
    if (elem == TSPGPU_ELEM_F64) {
        switch (nch) {
        case 1: return depth == 8 ? PK(double, 1, 8) : depth == 4 ? PK(double, 1, 4) : PK(double, 1, 2);
        case 2: return depth == 4 ? PK(double, 2, 4) : PK(double, 2, 2);
        case 4: return PK(double, 4, 2);
        }
    } else if (elem == TSPGPU_ELEM_I32) {
        switch (nch) {
        case 1: return depth == 8 ? PK(int, 1, 8) : depth == 4 ? PK(int, 1, 4) : PK(int, 1, 2);
        case 2: return depth == 4 ? PK(int, 2, 4) : PK(int, 2, 2);
        case 4: return PK(int, 4, 2);
        }
    } else {
        switch (nch) {
        case 1: return depth >= 4 ? PK(u16, 1, 4) : PK(u16, 1, 2);
        case 2: return depth >= 4 ? PK(u16, 2, 4) : PK(u16, 2, 2);
        case 3: return PK(u16, 3, 2);
        case 4: return PK(u16, 4, 2);
        }
    }
#undef PK
    return nullptr;
}

template <typename T, int NCH, bool TABU> static const void *res_fn() { return (const void *)k_sweep_res<T, NCH, 8, TABU>; }
static const void *res_kernel(int elem, int nch, bool tabu)
{
    if (!plan::has_res(elem, nch)) return nullptr;
    const void *fn = nullptr;
    ELEM_SWITCH(elem, T, fn = nch == 1 ? (tabu ? res_fn<T, 1, true>() : res_fn<T, 1, false>())
                                       : (tabu ? res_fn<T, 2, true>() : res_fn<T, 2, false>()));
    return fn;
}

template <typename T, int NCH, int D> static const void *fused_fn() { return (const void *)k_sweep_fused<T, NCH, 8, D>; }
// kernel 3: resident rows (nch 1, 2); kernel 2: streamed rows (nch 1, 2) -- two edges per barrier interval over four
// LDS row buffers (pipe_stream2) when `pipe2`, else one edge per barrier over three (pipe_stream, register depth 2)
static const void *fused_kernel(int elem, int nch, int kernel, bool pipe2)
{
    if (!plan::has_fused(elem, nch, kernel)) return nullptr;
    const void *fn = nullptr;
    if (kernel == 3) ELEM_SWITCH(elem, T, fn = nch == 1 ? fused_fn<T, 1, 0>() : fused_fn<T, 2, 0>());
    else {
        // (three uint16 chunks per thread, n > 16 384: the fused prologue no longer fits the register
        // budget next to the per-b state -- measured 1.7x slower than sweep + apply on d18512)
        // rows in flight (4 = one pair, 5 = two): measured at n=4096 -- f64 30.9 us with one pair, 33.0 with two (already at
        // 5.6 TB/s of the ~6.1 TB/s a CU's load path sustains; more requests only queue); int32 20.9 / 20.5
        if (pipe2 && elem == TSPGPU_ELEM_U16) fn = nch == 1 ? fused_fn<u16, 1, 5>() : fused_fn<u16, 2, 4>();
        else if (pipe2 && elem == TSPGPU_ELEM_F64) fn = nch == 1 ? fused_fn<double, 1, 4>() : fused_fn<double, 2, 4>();
        else if (pipe2) fn = nch == 1 ? fused_fn<int, 1, 5>() : fused_fn<int, 2, 5>();
        else ELEM_SWITCH(elem, T, fn = nch == 1 ? fused_fn<T, 1, 2>() : fused_fn<T, 2, 2>());
    }
    return fn;
}

static const void *simple_kernel(int elem, bool tabu)
{
    const void *fn = nullptr;
    ELEM_SWITCH(elem, T, fn = tabu ? (const void *)k_sweep_simple<T, true> : (const void *)k_sweep_simple<T, false>);
    return fn;
}

using plan::pow2_ceil;

// The plan for `ntours` tours in flight (plan::decide: kernel variant, block size, workgroups per tour), with the dynamic-LDS
// caps of its kernels raised.  `early`: plan::otf_early's answer.  A refusal leaves the plan the context had
static int make_plan(tspgpu_ctx *ctx, int ntours, bool early)
{
    const int n = ctx->n;
    const size_t row = (size_t)ctx->ld * elem_size(ctx->elem);
    if (const int rc = ctx->otf ? ensure_spts(ctx, (size_t)ntours * n) : (int)E_OK) return rc;    // matrix-free: every tour's gathered points
    const plan::Sweep s = plan::decide(plan_in(ctx), ntours, early, [&](plan::Kernel k, int bt, size_t lds) {
        const void *fn = k.kernel == 2 ? pipe_kernel(ctx->elem, k.nch, k.depth, false) : simple_kernel(ctx->elem, false);
        int api = 0; // registers count too: ask the runtime for this very kernel
        if (fn && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess &&
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&api, fn, bt, lds) == hipSuccess && api > 0)
            return api;
        return 0;
    });
    switch (s.refused) {
    case plan::Refusal::NONE: break;
    case plan::Refusal::RES_ROWS: return fail(ctx, E_EXHAUSTED, "resident sweep: rows of %zu B do not fit", row);
    case plan::Refusal::PIPE_ROWS: return fail(ctx, E_EXHAUSTED, "pipelined sweep: 3 rows of %zu B do not fit %zu B of LDS", row, ctx->lds_max);
    case plan::Refusal::WGS: return fail(ctx, E_EXHAUSTED, "resident sweep: %d workgroups per tour exceed %d", s.G, MAX_WGS_PER_TOUR);
    case plan::Refusal::ROW: return fail(ctx, E_EXHAUSTED, "matrix mode needs one %zu-byte row in LDS (max %zu): n=%d too large", row, ctx->lds_max, n);
    case plan::Refusal::MATRIX_N: return fail(ctx, E_EXHAUSTED, "n=%d exceeds the matrix-mode limit", n);
    }
    if (ctx->otf) {
        if (s.G > ctx->S.pstride) return fail(ctx, E_INTERNAL, "partial stride %d < %d workgroups", ctx->S.pstride, s.G);
        ctx->plan = s;
        return E_OK;
    }
    if (s.pipe2_sweep)
        HIP_TRY(hipFuncSetAttribute(pipe2_kernel(ctx->elem, s.NCH), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(s.lds + row)));
    // raise the dynamic-LDS cap of the kernels we are going to launch
    if (const void *ff = fused_kernel(ctx->elem, s.NCH, s.kernel, s.pipe2))
        HIP_TRY(hipFuncSetAttribute(ff, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.lds_fused));
    for (int tabu = 0; tabu < 2; tabu++) {
        const void *fn = s.kernel == 3 ? res_kernel(ctx->elem, s.NCH, tabu)
                       : s.kernel == 2 ? pipe_kernel(ctx->elem, s.NCH, s.D, tabu) : simple_kernel(ctx->elem, tabu);
        if (!fn) return fail(ctx, E_INTERNAL, "no kernel instance for nch=%d", s.NCH);
        const size_t need = tabu ? plan::tabu_lds(s, n) : s.lds;
        if (need > ctx->lds_max) continue;      // (tabu only, s.tabu_fits: plain 2-opt must not fail for the tabu variant's sake)
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need));
    }
    ctx->plan = s;
    return E_OK;
}

// g0 / gcount: the workgroups (runs) to launch; gcount < 0 = all of them (a sharded sweep launches a part)
static int launch_sweep(tspgpu_ctx *ctx, int slot0, int ntours, bool tabu, int g0 = 0, int gcount = -1)
{
    SweepArgs A;
    memset(&A, 0, sizeof A);
    A.S = ctx->S;
    A.mat = ctx->d_mat;
    A.n = ctx->n; A.ld = ctx->ld; A.slot0 = slot0; A.P = ctx->plan.P;
    A.g0 = g0;
    const int G = gcount < 0 ? ctx->plan.G : gcount;
    A.symmetric = ctx->symmetric ? 1 : 0;
    A.ablate = ctx->opt_ablate;
    A.stamps = ctx->opt_stamps ? ctx->d_stamps : nullptr;
    A.pts = ctx->d_pts; A.spts = ctx->d_spts; A.kind = ctx->kind;
    A.tabu_list = ctx->d_tabu_list; A.tabu = ctx->d_tabu;
    if (ctx->plan.kernel == 4) {
        const int n = ctx->n;
        const bool otf8 = plan::otf8(ctx->cost_bound, n);
        if (otf8 && ctx->ceil_int() && ctx->d_ipts) {      // (the int2 successors' points take the front half of the double2 buffer)
            A.ipts = ctx->d_ipts; A.ispts = reinterpret_cast<const int2 *>(ctx->d_spts.p);
            hipLaunchKernelGGL(k_gather_ispts, dim3((n + 255) / 256, ntours), dim3(256), 0, ctx->stream, ctx->S, n, slot0, ctx->d_ipts, reinterpret_cast<int2 *>(ctx->d_spts.p));
        } else
            hipLaunchKernelGGL(k_gather_spts, dim3((n + 255) / 256, ntours), dim3(256), 0, ctx->stream, ctx->S, n, slot0, ctx->d_pts, ctx->d_spts);
        HIP_TRY(hipGetLastError());
        const void *fo = tabu ? (const void *)k_sweep_otf<true> : (const void *)k_sweep_otf<false>;
        if (otf8) {
            const int kind = ctx->ceil_int() ? KIND_CEIL_INT : ctx->kind;
#define OTF8(K) (tabu ? (const void *)k_sweep_otf8<K, true> : ctx->plan.otf_early ? (const void *)k_sweep_otf8<K, false, true> : (const void *)k_sweep_otf8<K, false>)
            // plain 2-opt: with the exact early-out and runs of 64 edges (option 99 = 3: without it, the full evaluation of every
            // pair -- diagnostics, tools/otf_rate.py)
            fo = kind == TSPGPU_EUC_2D ? OTF8(TSPGPU_EUC_2D) : kind == TSPGPU_ATT ? OTF8(TSPGPU_ATT)
               : kind == KIND_CEIL_INT ? OTF8(KIND_CEIL_INT) : OTF8(TSPGPU_CEIL_2D);
#undef OTF8
        }
        void *ao[] = {&A};
        HIP_TRY(hipLaunchKernel(fo, dim3(G, ntours), dim3(256), ao, 0, ctx->stream));
        return E_OK;
    }
    const void *fn = ctx->plan.kernel == 3 ? res_kernel(ctx->elem, ctx->plan.NCH, tabu)
                   : ctx->plan.kernel == 2 ? pipe_kernel(ctx->elem, ctx->plan.NCH, ctx->plan.D, tabu) : simple_kernel(ctx->elem, tabu);
    // (the two-edge streaming form replaces the pipelined kernel below when it applies)
    // tabu: n + 32 verdict bytes behind everything else in the dynamic LDS
    if (tabu && ctx->plan.kernel != 1 && !ctx->plan.tabu_fits)
        return fail(ctx, E_EXHAUSTED, "tabu sweep: the rows leave no room for %d verdict bytes in LDS (use TSPGPU_OPT_KERNEL=1 or the matrix-free mode)", ctx->n + 32);
    A.tabu_lds = (int)((ctx->plan.lds + 15) & ~(size_t)15);
    size_t lds = tabu && ctx->plan.kernel != 1 ? (size_t)A.tabu_lds + ctx->n + 32 : ctx->plan.lds;
    if (ctx->plan.kernel == 2 && ctx->plan.pipe2_sweep && !tabu && ctx->symmetric) {
        fn = pipe2_kernel(ctx->elem, ctx->plan.NCH);
        lds = ctx->plan.lds + (size_t)ctx->ld * elem_size(ctx->elem);
    }
    void *args[] = {&A};
    HIP_TRY(hipLaunchKernel(fn, dim3(G, ntours), dim3(ctx->plan.BT), args, lds, ctx->stream));
    return E_OK;
}

// partials of one tour := {the given move, nothing else}: what k_apply then applies (sharded sweeps)
__global__ void k_set_move(Tours S, int slot, int G, double d, u64 key)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    Partial o;
    o.d = g == 0 ? d : 0.0;
    o.key = g == 0 ? key : 0;
    S.partial[(size_t)slot * S.pstride + g] = o;
}

static int launch_apply(tspgpu_ctx *ctx, int slot0, int ntours, bool tabu, bool resident_tabu)
{
    ApplyArgs A;
    A.S = ctx->S;
    A.mat = ctx->d_mat;
    A.n = ctx->n; A.ld = ctx->ld; A.slot0 = slot0; A.G = ctx->plan.G;
    A.symmetric = ctx->symmetric ? 1 : 0;
    A.pts = ctx->d_pts; A.kind = ctx->kind;
    A.tabu_list = ctx->d_tabu_list; A.tabu = ctx->d_tabu;
    A.best_succ = ctx->d_best_succ; A.trace = resident_tabu ? ctx->d_trace : nullptr;
    A.hist = ctx->hist;
    const int BT = std::min(1024, std::max(64, pow2_ceil(ctx->n / 4)));
    const void *fn = nullptr;
    ELEM_SWITCH(ctx->elem, T, fn = tabu ? (const void *)k_apply<T, true> : (const void *)k_apply<T, false>);
    void *args[] = {&A};
    HIP_TRY(hipLaunchKernel(fn, dim3(ntours), dim3(BT), args, 0, ctx->stream));
    return E_OK;
}

static double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// the entry points' time limit as a point in time (< 0: none), and what they answer when it passed
static double deadline_of(double time_left_s) { return time_left_s >= 0 ? now_s() + time_left_s : -1; }
static int done_code(bool late) { return late ? E_DEADLINE : E_OK; }

static int ensure_fused(tspgpu_ctx *ctx)
{
    if (ctx->fcap >= ctx->tcap) return E_OK;
    HIP_TRY(tspmem::grow(HipMem{ctx->stream}, ctx->fused_rows((size_t)ctx->n, (size_t)ctx->S.pstride), 0, (size_t)ctx->tcap));
    ctx->fcap = ctx->tcap;
    return E_OK;
}

static int launch_fused(tspgpu_ctx *ctx, int slot0, int ntours, int parity)
{
    SweepArgs A;
    memset(&A, 0, sizeof A);
    A.S = ctx->S;
    A.mat = ctx->d_mat;
    A.n = ctx->n; A.ld = ctx->ld; A.slot0 = slot0; A.P = ctx->plan.P;
    A.symmetric = 1;
    A.ablate = ctx->opt_ablate;
    A.stamps = ctx->opt_stamps ? ctx->d_stamps : nullptr;
    A.pts = ctx->d_pts; A.spts = nullptr; A.kind = ctx->kind;
    A.F = ctx->F; A.parity = parity; A.hist = ctx->hist;
    const void *fn = fused_kernel(ctx->elem, ctx->plan.NCH, ctx->plan.kernel, ctx->plan.pipe2);
    if (!fn) return fail(ctx, E_INTERNAL, "no one-launch-per-sweep instance for kernel %d, %d chunks", ctx->plan.kernel, ctx->plan.NCH);
    void *args[] = {&A};
    HIP_TRY(hipLaunchKernel(fn, dim3(ctx->plan.G, ntours), dim3(ctx->plan.BT), args, ctx->plan.lds_fused, ctx->stream));
    return E_OK;
}

// Rough duration of one sweep iteration over `ntours` tours before anything has been measured (rows at ~4 TB/s
// plus the fixed launch chain): only used to decide how early the deadline logic leaves the batched mode.
static double est_iter_s(const tspgpu_ctx *ctx, int ntours)
{
    const double n = ctx->n;
    if (ctx->otf) return ntours * (20e-6 + n * n / 2 / 5e11);
    return ntours * (12e-6 + n * ctx->ld * (double)elem_size(ctx->elem) / 4e12);
}

// One launch per sweep (k_sweep_fused): begin, batches of an even number of launches with
// alternating parity (replayed as a hipGraph), end.
//
// Deadline (refinment.c:17-24 polls before every sweep): while more than three batches' worth of time is left the
// batches run pipelined against the host; after that single launches, one host poll each; once the time is up the
// sweep that already ran is applied (k_cap_now + two launches), so the tour, its cost, the sweep count and the move
// history returned are those of one and the same state, at most one sweep past the deadline.
static int run_fused(tspgpu_ctx *ctx, int slot0, int ntours, double time_left_s, bool *deadline_hit)
{
    int rc = ensure_fused(ctx);
    if (rc) return rc;
    const int n = ctx->n;
    const bool f64 = ctx->elem == TSPGPU_ELEM_F64;
    const dim3 grid1((n + 255) / 256, ntours);
    const bool pk = ctx->elem == TSPGPU_ELEM_U16;
    const double t_end = deadline_of(time_left_s);
    if (t_end >= 0 && time_left_s <= 0) { if (deadline_hit) *deadline_hit = true; return E_OK; }   // not one sweep
    if (f64) hipLaunchKernelGGL((k_fused_begin<double, false>), grid1, dim3(256), 0, ctx->stream, ctx->S, ctx->F, n, slot0);
    else if (pk) hipLaunchKernelGGL((k_fused_begin<int, true>), grid1, dim3(256), 0, ctx->stream, ctx->S, ctx->F, n, slot0);
    else hipLaunchKernelGGL((k_fused_begin<int, false>), grid1, dim3(256), 0, ctx->stream, ctx->S, ctx->F, n, slot0);
    HIP_TRY(hipGetLastError());
    const int K = std::max(2, ctx->opt_batch & ~1);
    long issued = 0;      // launches so far; the next one writes parity issued & 1
    bool late = false;
    auto launch_eager = [&](int cnt) -> int {
        for (int i = 0; i < cnt; i++) {
            const int rc = launch_fused(ctx, slot0, ntours, (int)(issued & 1));
            if (rc) return rc;
            issued++;
        }
        return E_OK;
    };
    // one batch = K launches (a replayed hipGraph; `issued` is even whenever this runs) + the copy of the `done` words
    auto issue_batch = [&](int *h_done) -> int {
        int rc = E_OK;
        if (ctx->opt_graph) {
            // (key 2: neither the plain nor the tabu pairs of run_sweeps_plain)
            if ((rc = replay_graph(ctx, slot0, ntours, 2, K, [&](int i) { return launch_fused(ctx, slot0, ntours, i & 1); }))) return rc;
            issued += K;
        } else if ((rc = launch_eager(K))) return rc;
        if (ctx->opt_timing) HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
        HIP_TRY(hipMemcpyAsync(h_done, ctx->S.done + slot0, (size_t)ntours * 4, hipMemcpyDeviceToHost, ctx->stream));
        return E_OK;
    };
    auto all_done = [&](const int *h_done) {
        for (int i = 0; i < ntours; i++) if (!h_done[i]) return false;
        return true;
    };
    bool finished = false;
    bool careful = t_end >= 0 && time_left_s < 3.0 * K * est_iter_s(ctx, ntours);
    if (ctx->opt_timing) {
        for (;;) {
            // timing mode: one event pair around the whole batch (the launches of a batch run back to
            // back, so batch time / K is the mean launch duration); only batches in which every launch
            // swept are counted
            if ((rc = ensure_events(ctx, 2))) return rc;
            const long before = issued;
            HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
            if ((rc = issue_batch(ctx->h_status))) return rc;
            HIP_TRY(hipMemcpyAsync(ctx->h_status + ctx->tcap, ctx->S.nsweeps + slot0, (size_t)ntours * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            {
                int live = 0; // launches 0 .. nsweeps-1 swept (launch nsweeps only found the tour finished)
                for (int i = 0; i < ntours; i++) live = std::max(live, ctx->h_status[ctx->tcap + i]);
                if (before + K <= live) {
                    float ms = 0;
                    HIP_TRY(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
                    ctx->sweep_ms_total += ms; ctx->sweep_launches += K;
                }
            }
            if (all_done(ctx->h_status)) { finished = true; break; }
            if (t_end >= 0 && now_s() >= t_end) { late = true; break; }
        }
    } else if (!careful) {
        // Pipelined: the next batch is in the stream before the host looks at the previous one's
        // `done` words, so the device never waits for the host (a graph launch + a sync cost
        // ~20 us per batch otherwise); the price is one batch of immediately-returning launches
        // after the tour has finished.
        if ((rc = ensure_events(ctx, 4))) return rc;
        int *buf[2] = {ctx->h_status, ctx->h_status + ctx->tcap};
        if ((rc = issue_batch(buf[0]))) return rc;
        HIP_TRY(hipEventRecord(ctx->ev[2], ctx->stream));
        double t_prev = now_s(), batch_dt = 0;
        for (int cur = 0;; cur ^= 1) {
            if ((rc = issue_batch(buf[cur ^ 1]))) return rc;
            HIP_TRY(hipEventRecord(ctx->ev[2 + (cur ^ 1)], ctx->stream));
            HIP_TRY(hipEventSynchronize(ctx->ev[2 + cur]));
            if (all_done(buf[cur])) { finished = true; break; }
            if (t_end >= 0) {
                const double now = now_s();
                batch_dt = batch_dt == 0 ? now - t_prev : 0.5 * (batch_dt + now - t_prev);
                t_prev = now;
                if (now >= t_end || t_end - now < 3.0 * batch_dt) {
                    // leave the batched mode: wait for the batch in flight, then poll per launch
                    HIP_TRY(hipEventSynchronize(ctx->ev[2 + (cur ^ 1)]));
                    if (all_done(buf[cur ^ 1])) finished = true;
                    careful = true;
                    break;
                }
            }
        }
    }
    if (careful && !finished && !late) {
        for (;;) {
            if (now_s() >= t_end) { late = true; break; }
            if ((rc = launch_eager(1))) return rc;
            HIP_TRY(hipMemcpyAsync(ctx->h_status, ctx->S.done + slot0, (size_t)ntours * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            if (all_done(ctx->h_status)) { finished = true; break; }
        }
    }
    if (late) {
        if (deadline_hit) *deadline_hit = true;
        if (issued > 0) {
            // apply the move of the last sweep that ran: cap := sweeps completed, then one launch applies it and raises
            // `stop`, the next one raises `done` (a tour whose last sweep found nothing finishes the ordinary way)
            hipLaunchKernelGGL(k_cap_now, dim3((ntours + 63) / 64), dim3(64), 0, ctx->stream, ctx->S, slot0, ntours);
            HIP_TRY(hipGetLastError());
            if ((rc = launch_eager(2))) return rc;
        }
    }
    const int last_parity = (int)((issued + 1) & 1);   // parity written by the last launch (moot once `done` is up)
    if (f64) hipLaunchKernelGGL((k_fused_end<double, false>), grid1, dim3(256), 0, ctx->stream, ctx->S, ctx->F, n, slot0, last_parity);
    else if (pk) hipLaunchKernelGGL((k_fused_end<int, true>), grid1, dim3(256), 0, ctx->stream, ctx->S, ctx->F, n, slot0, last_parity);
    else hipLaunchKernelGGL((k_fused_end<int, false>), grid1, dim3(256), 0, ctx->stream, ctx->S, ctx->F, n, slot0, last_parity);
    HIP_TRY(hipGetLastError());
    return E_OK;
}

// The shaped instantiations of k_lds2opt (plain packed descent, n == nl): the one place that lists them.
// tmat: the form that fetches moved rows from the tour-ordered copy (PersistArgs::tmat, n * n cells)
// clocked: the instantiation that carries the phase clocks (option 98); production runs the one without
template <int NLC, int EC> static const void *lp_shaped_of(bool tmat, bool clocked)
{
    if (clocked) return tmat ? (const void *)k_lds2opt<true, false, false, NLC, EC, true, true> : (const void *)k_lds2opt<true, false, false, NLC, EC, false, true>;
    return tmat ? (const void *)k_lds2opt<true, false, false, NLC, EC, true> : (const void *)k_lds2opt<true, false, false, NLC, EC>;
}
static const void *lp_shaped_fn(int n, int E, bool tmat, bool clocked)
{
    if (n == 4096 && E == 16) return lp_shaped_of<4096, 16>(tmat, clocked);
    if (n == 1024 && E == 4) return lp_shaped_of<1024, 4>(tmat, clocked);
    return nullptr;
}

// ---- the one-launch descents: run_persist and run_pstream around relaunch::drive (tspgpu_relaunch.h) ----------------------
static_assert((int)relaunch::INTERNAL == (int)E_INTERNAL && (int)relaunch::GO_ON == (int)E_OK, "the driver's codes are the engine's");
// wanted: always, or where nothing else was chosen (TSPGPU_OPT_KERNEL / _FUSED keep to that choice)
static bool resident_wanted(const tspgpu_ctx *ctx) { return ctx->opt_persist == 2 || (ctx->opt_persist == 1 && ctx->opt_kernel == 0 && ctx->opt_fused == 1); }

// For a launch of W workgroups: their exchange slots and the control words behind them zeroed (one memset for both), and
// the fields that PersistArgs and StreamArgs have in common.
template <typename ARGS> static int resident_args(tspgpu_ctx *ctx, ARGS &A, int slot, int W, int budget, bool first)
{
    HIP_TRY(hipMemsetAsync(ctx->d_lp_slots, 0, (size_t)2 * W * 64 + 64, ctx->stream));
    memset(&A, 0, sizeof A);
    A.S = ctx->S; A.mat = (const u16 *)ctx->d_mat.p; A.n = ctx->n; A.ld = ctx->ld; A.slot = slot; A.budget = budget;
    A.slots = ctx->d_lp_slots; A.ctl = reinterpret_cast<int *>(ctx->d_lp_slots + (size_t)2 * W * 8); A.hist = ctx->hist;
    A.hello_ticks = ctx->opt_lp_hello;   // 2 ms (test hook 97: negative = workgroup 0 withholds its record for that long)
    if (ctx->opt_lp_fail_at > 0 && !first) { ctx->opt_lp_fail_at--; A.hello_ticks = -5000; }   // test hook 96: the next N relaunches fail their rendezvous
    A.spin_ticks = 100000000;            // 1 s
    A.poll_sleep = ctx->opt_lp_poll_sleep; A.stamps = ctx->opt_stamps ? ctx->d_stamps : nullptr;
    return E_OK;
}

// One launch between its timing events; back in ctx->h_lp the control words ([1] status, [2] sweeps run) and at [8] the double
// `also`; the stream drained.  relaunch::drive's launch callable: the two errors that the driver makes of it are worded here.
template <typename ARGS>
static int launch_resident(tspgpu_ctx *ctx, const char *what, const void *fn, int W, int block, size_t lds, ARGS &A, bool first, int &status, int &sweeps, const double *also = nullptr)
{
    void *args[] = {&A};
    if (ctx->opt_timing) { const int rc = ensure_events(ctx, 2); if (rc) return rc; }
    if (ctx->opt_timing) HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
    const hipError_t le = hipLaunchKernel(fn, dim3(W), dim3(block), args, lds, ctx->stream);
    if (le != hipSuccess) {                     // (e.g. a device that does not grant 160 KiB of LDS to one workgroup)
        (void)hipGetLastError();
        if (!first) fail(ctx, E_INTERNAL, "%s: launch failed: %s", what, hipGetErrorString(le));
        return status = relaunch::REFUSED, E_OK;
    }
    if (ctx->opt_timing) HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->h_lp, A.ctl, 32, hipMemcpyDeviceToHost, ctx->stream));
    if (also) HIP_TRY(hipMemcpyAsync(ctx->h_lp + 8, also, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    status = ctx->h_lp[1]; sweeps = ctx->h_lp[2];
    if (status == LP_ST_RUNNING) fail(ctx, E_INTERNAL, "%s: no status written (after %d sweeps)", what, sweeps);
    return E_OK;
}

// A launch completed: the time between its events goes to the sweep statistics; a descent is over at a local optimum or at
// its sweep cap, a launch that used up its budget is followed by another.
static int descent_completed(tspgpu_ctx *ctx, int status, int sd)
{
    if (ctx->opt_timing && sd > 0) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        ctx->sweep_ms_total += ms; ctx->sweep_launches += sd;
    }
    return status == LP_ST_OPTIMUM || status == LP_ST_CAPPED ? relaunch::STOP : relaunch::GO_ON;
}
static int hand_over(bool) { return relaunch::HAND_OVER; }

// What relaunch::drive answered, for the context and the caller.  *ran stays false where the one-launch-per-sweep path has to
// take over; lp_handed then tells whether from the start or from the tour the last completed launch wrote back.
static int resident_result(tspgpu_ctx *ctx, const relaunch::Result &r, bool *deadline_hit, bool *ran)
{
    ctx->lp_sweeps = r.sweeps;
    if (!r.code && !r.ran) ctx->lp_handed = r.handed;
    if (r.late && deadline_hit) *deadline_hit = true;
    *ran = r.ran;
    return r.code;
}

struct PersistTabu { int k, tenure, t_min, t_max, up; double best; };
// mh_VNS's loop in the LDS-resident kernels (tspgpu_lds_vns.inc): in/out state of tspgpu_vns_search across launches
struct PersistVns {
    int k;                  // iterations asked for in all
    int it;                 // iterations completed
    int phase;              // 1: the next launch resumes in the kick phase of iteration `it`
    const int *h_rand;      // the caller's rand() values
    long nrand, used;       // ... how many there are, how many have been consumed
    double best;            // cost of the incumbent
    double *h_trace;        // cost of every local optimum from iteration it_entry on, or nullptr
    bool need_rand;         // out: stopped in front of a kick phase for want of numbers
    int it_entry;           // `it` when the call was entered
};

// *ran = false: nothing was touched (does not apply, or the grid did not come up co-resident), or -- lp_handed -- the grid
// lost its co-residency after the first launch (another context took CUs): the slot holds the consistent tour the last
// completed launch wrote back and *time_left_io the time that is left.  Either way the caller takes the one-launch-per-sweep
// path.  Every launch leaves a consistent tour (the sweep that ran is applied, refinment.c:17-26).
static int run_persist(tspgpu_ctx *ctx, int slot, double *time_left_io, bool *deadline_hit, bool *ran, const PersistTabu *tabu = nullptr,
                       PersistVns *vns = nullptr)
{
    *ran = false;
    const double time_left_s = time_left_io ? *time_left_io : -1.0;
    const plan::Resident R = plan::resident(plan_in(ctx), tabu != nullptr);
    if (R.form == plan::Form::NONE) return E_OK;
    const int E = R.E, W = R.W, Ws = R.Ws, nstage = R.nstage;
    const size_t lds = R.lds;
    const bool win = R.form == plan::Form::WINDOW;
    if (ctx->lp_gate.skip_this()) return E_OK;
    HIP_TRY(ctx->d_lp_slots.reserve(((size_t)2 * LP_BT * 64 + 64) / 8));   // exchange slots, then the control words
    HIP_TRY(ctx->h_lp.reserve(16));
    if (tabu || vns) HIP_TRY(ctx->d_lp_best.reserve((size_t)ctx->ld + 16));
    const int pk = (tabu ? ctx->max8k : ctx->max16k) ? 1 : 0;
    void (*const fns[2][3][2])(PersistArgs) = {     // [half-window rows][plain descent, tabu walk, VNS loop][packed deltas]
        {{k_lds2opt<false, false>, k_lds2opt<true, false>}, {k_lds2opt<false, true>, k_lds2opt<true, true>}, {k_lds2opt<false, false, true>, k_lds2opt<true, false, true>}},
        {{k_lds2opt_w<false, false>, k_lds2opt_w<true, false>}, {k_lds2opt_w<false, true>, k_lds2opt_w<true, true>}, {k_lds2opt_w<false, false, true>, k_lds2opt_w<true, false, true>}}};
    // (E comes from the device's compute units: 16 / 4 on a whole MI355X; with fewer CUs E is larger, no shape is listed and
    // the generic kernel runs -- tspgpu_info 61 tells)
    const bool shaped = !win && !tabu && !vns && pk && !ctx->opt_lp_generic && lp_shaped_fn(ctx->n, E, false, false);
    // the tour-ordered copy where a shaped form runs; without the memory for it the shaped form that needs none
    bool tm = shaped && !ctx->opt_lp_no_tmat;
    if (tm && ctx->d_lp_tmat.reserve((size_t)ctx->n * ctx->n) != hipSuccess) { (void)hipGetLastError(); tm = false; }
    const void *const sfn = shaped ? lp_shaped_fn(ctx->n, E, tm, ctx->opt_stamps != 0) : nullptr;
    const void *const fn = sfn ? sfn : (const void *)fns[win][tabu ? 1 : vns ? 2 : 0][pk];
    if (const int rc = ensure_max_lds(ctx, fn)) return rc;
    const double t_end = deadline_of(time_left_s);
    if (t_end >= 0 && time_left_s <= 0) { if (deadline_hit) *deadline_hit = true; *ran = true; ctx->lp_used = true; ctx->lp_window = win; ctx->lp_shaped = false; ctx->lp_tmat = false; ctx->lp_packed = pk != 0; return E_OK; }
    if (vns) vns->need_rand = false;
    // one launch: fill(A) queues what the walk needs in front of it and completes the arguments
    auto launch = [&](int budget, bool first, int &status, int &sd, auto &&fill, const double *also = nullptr) -> int {
        PersistArgs A;
        int rc = resident_args(ctx, A, slot, W, budget, first);
        A.E = E; A.nl = (ctx->n + 7) & ~7; A.Ws = Ws; A.nstage = nstage; A.tmat = tm ? ctx->d_lp_tmat.p : nullptr;
        if (!rc) rc = fill(A);
        return rc ? rc : launch_resident(ctx, "LDS-resident descent", fn, W, win ? LW_BT : LP_BT, lds, A, first, status, sd, also);
    };
    // the walks keep their best tour by array cell, every workgroup its own cells (d_lp_best), and its cost in the tabu state
    auto best_cost = [&]() { return reinterpret_cast<double *>(reinterpret_cast<char *>(ctx->d_tabu) + offsetof(TabuState, best_cost)); };
    auto walk_fill = [&](PersistArgs &A, double best0) -> int {
        HIP_TRY(hipMemsetAsync(ctx->d_lp_best + ctx->ld, 0, 8, ctx->stream));
        A.best0 = best0; A.best_ord = ctx->d_lp_best; A.best_dir = ctx->d_lp_best + ctx->ld; A.best_out = best_cost();
        return E_OK;
    };
    // A walk's launch completed: its best tour becomes the successor array.  Only now -- a launch that lost its grid half
    // way leaves a MIXTURE of old and new cells in best_ord (the workgroups that passed the last exchange wrote theirs, the
    // one that timed out did not), and d_best_succ must keep the last good launch's tour for the hand-over
    auto walk_completed = [&](int status, int sd) -> int {
        hipLaunchKernelGGL(k_lds_best_succ, dim3((ctx->n + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_lp_best, ctx->d_lp_best + ctx->ld, ctx->d_best_succ, ctx->n);
        HIP_TRY(hipGetLastError());
        return descent_completed(ctx, status, sd);
    };
    relaunch::Result r;
    if (tabu) {
        auto fill = [&](PersistArgs &A) -> int {
            A.tabu_k = tabu->k; A.tenure0 = tabu->tenure; A.t_min = tabu->t_min; A.t_max = tabu->t_max; A.up0 = tabu->up;
            A.budget = -1; A.trace = ctx->d_trace;
            return walk_fill(A, tabu->best);
        };
        r = relaunch::drive(ctx->lp_gate, now_s, t_end, 8e-6, time_left_io, [&](int budget, bool first, int &st, int &sd) { return launch(budget, first, st, sd, fill); },
                            walk_completed, [&](bool first) -> int {
                                return first ? (int)relaunch::HAND_OVER : fail(ctx, E_INTERNAL, "LDS-resident tabu walk: exchange lost after %d iterations", ctx->h_lp[2]); });
    } else if (vns) {
        auto fill = [&](PersistArgs &A) -> int {
            int rc = walk_fill(A, vns->best);
            if (rc) return rc;
            // this launch: at most 65536 iterations, the numbers they can be expected to need (a kick phase draws 1 + 3 per
            // kick + the rejected ones, 8 on average; the kernel stops in front of a kick phase it cannot finish)
            A.vns_k = std::min(vns->k - vns->it, ctx->opt_vns_launch_k);
            const long want = std::min<long>(vns->nrand - vns->used, 32L * A.vns_k + 1024);
            if (want > 0) HIP_TRY(ctx->d_vns_rand.reserve((size_t)want + 64));
            if (want > 0) HIP_TRY(hipMemcpyAsync(ctx->d_vns_rand, vns->h_rand + vns->used, (size_t)want * 4, hipMemcpyHostToDevice, ctx->stream));
            if (vns->h_trace && (rc = reserve_captured(ctx, ctx->d_trace, (size_t)A.vns_k))) return rc;
            ctx->vns_launch_nrand = (int)want;
            A.vns_it0 = vns->it; A.vns_phase = vns->phase; A.vns_rand = ctx->d_vns_rand; A.vns_nrand = (int)want; A.vns_state = A.ctl + 4;
            A.trace = vns->h_trace ? ctx->d_trace : nullptr;
            return E_OK;
        };
        auto completed = [&](int status, int sd) -> int {
            const int next = walk_completed(status, sd);
            if (next > 0) return next;
            // what the launch completed: iterations, numbers, the incumbent's cost, the local optima's costs
            const int it1 = ctx->h_lp[4];
            if (vns->h_trace && it1 > vns->it) {
                HIP_TRY(hipMemcpyAsync(vns->h_trace + (vns->it - vns->it_entry), ctx->d_trace, (size_t)(it1 - vns->it) * 8, hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(hipStreamSynchronize(ctx->stream));
            }
            vns->it = it1; vns->used += ctx->h_lp[5]; vns->phase = ctx->h_lp[6];
            memcpy(&vns->best, ctx->h_lp + 8, 8);
            if (status == LP_ST_NEED_RAND) {    // out of numbers: of all the caller gave, or only of this launch's window
                vns->need_rand = vns->used + ctx->vns_launch_nrand - ctx->h_lp[5] >= vns->nrand;
                return vns->need_rand ? relaunch::STOP : relaunch::GO_ON;
            }
            if (status == LP_ST_VNS_DONE) return vns->it >= vns->k ? relaunch::STOP : relaunch::GO_ON;   // (a launch completes at most 65536 iterations)
            return next;
        };
        r = relaunch::drive(ctx->lp_gate, now_s, t_end, 8e-6, time_left_io,
                            [&](int budget, bool first, int &st, int &sd) { return launch(budget, first, st, sd, fill, best_cost()); }, completed, hand_over);
    } else
        r = relaunch::drive(ctx->lp_gate, now_s, t_end, 8e-6, time_left_io,
                            [&](int budget, bool first, int &st, int &sd) { return launch(budget, first, st, sd, [](PersistArgs &) -> int { return E_OK; }); },
                            [&](int status, int sd) { return descent_completed(ctx, status, sd); }, hand_over);
    if (const int rc = resident_result(ctx, r, deadline_hit, ran); rc || !*ran) return rc;
    ctx->lp_used = true; ctx->lp_window = win; ctx->lp_shaped = sfn != nullptr; ctx->lp_tmat = tm; ctx->lp_packed = pk != 0;
    return E_OK;
}

// *ran, *time_left_io and the deadline as run_persist.
static int run_pstream(tspgpu_ctx *ctx, int slot, double *time_left_io, bool *deadline_hit, bool *ran)
{
    *ran = false;
    const double time_left_s = time_left_io ? *time_left_io : -1.0;
    const plan::Stream SP = plan::stream(plan_in(ctx));
    if (!SP.fits) return E_OK;
    const int P = SP.P, W = SP.W, BT = SP.BT, NCH = SP.NCH;
    const size_t lds = SP.lds;
    if (ctx->lp_gate.skip_this()) return E_OK;
    HIP_TRY(ctx->d_lp_slots.reserve(((size_t)2 * LP_BT * 64 + 64) / 8));
    HIP_TRY(ctx->h_lp.reserve(16));
    // (the register budget follows the block: 768 threads leave 170 registers a thread, 512 leave 256)
    const void *fn = NCH == 1 ? (BT <= 768 ? (const void *)k_str2opt<1, 768> : (const void *)k_str2opt<1, 1024>)
                              : (BT <= 512 ? (const void *)k_str2opt<2, 512> : (const void *)k_str2opt<2, 1024>);
    if (const int rc = ensure_max_lds(ctx, fn)) return rc;
    const double t_end = deadline_of(time_left_s);
    if (t_end >= 0 && time_left_s <= 0) { if (deadline_hit) *deadline_hit = true; *ran = true; ctx->sp_used = true; return E_OK; }
    const double sweep_s = 2e-9 * (double)ctx->n * ctx->n / 5.0e3 + 5e-6;     // first guess: the rows at 5 TB/s + the exchange
    const relaunch::Result r = relaunch::drive(ctx->lp_gate, now_s, t_end, sweep_s, time_left_io, [&](int budget, bool first, int &status, int &sd) -> int {
        StreamArgs A;
        const int rc = resident_args(ctx, A, slot, W, budget, first);
        A.P = P; A.ablate = ctx->opt_ablate;
        return rc ? rc : launch_resident(ctx, "streamed persistent descent", fn, W, BT, lds, A, first, status, sd);
    }, [&](int status, int sd) { return descent_completed(ctx, status, sd); }, hand_over);
    if (const int rc = resident_result(ctx, r, deadline_hit, ran); rc || !*ran) return rc;
    ctx->sp_used = true;
    return E_OK;
}

// Run (sweep, apply) pairs on slots [slot0, slot0+ntours) until every tour is
// done, `max_iters` pairs were issued (tabu), or the deadline passed (checked before every batch; the batches
// shrink to single iterations once fewer than three batches' worth of time is left, refinment.c:17-24).
__global__ void k_rebase(Tours S, int slot, int delta)     // sweep counter and cap of a slot shifted by delta (see run_sweeps)
{
    S.nsweeps[slot] += delta;
    if (S.cap_sweeps[slot] >= 0) S.cap_sweeps[slot] += delta;
}

static int run_sweeps_plain(tspgpu_ctx *ctx, int slot0, int ntours, bool tabu, long max_iters, double time_left_s, bool *deadline_hit);

// the launch plan for `ntours` tours in flight, plain 2-opt or tabu (the matrix-free sweep's run length follows the variant:
// plan::otf_early)
static int ensure_plan(tspgpu_ctx *ctx, int ntours, bool tabu)
{
    const bool early = plan::otf_early(plan_in(ctx), tabu);
    if (ctx->plan.T != ntours || ctx->plan.kernel == 0 || (ctx->otf && ctx->plan.otf_early != early)) {
        int rc = make_plan(ctx, ntours, early);
        if (rc) return rc;
        drop_graphs(ctx);
    }
    return E_OK;
}

// A one-launch descent began and lost its grid (another context took CUs): the slot holds the tour its last completed
// launch wrote back.  The per-sweep kernels count their sweeps from 0: run them on a rebased counter / cap / history and shift
// everything back afterwards.
static int run_rebased(tspgpu_ctx *ctx, int slot0, long max_iters, double time_left_s, bool *deadline_hit)
{
    int base = 0;
    HIP_TRY(hipMemcpyAsync(&base, ctx->S.nsweeps + slot0, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const HistBuf keep = ctx->hist;
    const int hb = std::min(base, keep.cap);
    if (keep.cap > 0) { ctx->hist.a += hb; ctx->hist.b += hb; ctx->hist.d += hb; ctx->hist.cap -= hb; }
    drop_graphs(ctx);
    hipLaunchKernelGGL(k_rebase, dim3(1), dim3(1), 0, ctx->stream, ctx->S, slot0, -base);
    int rc2 = run_sweeps_plain(ctx, slot0, 1, false, max_iters, time_left_s, deadline_hit);
    hipLaunchKernelGGL(k_rebase, dim3(1), dim3(1), 0, ctx->stream, ctx->S, slot0, base);
    if (!rc2 && hipGetLastError() != hipSuccess) rc2 = fail(ctx, E_INTERNAL, "k_rebase launch failed");
    ctx->hist = keep;
    drop_graphs(ctx);
    return rc2;
}

static int run_sweeps(tspgpu_ctx *ctx, int slot0, int ntours, bool tabu, long max_iters, double time_left_s,
                      bool *deadline_hit)
{
    if (deadline_hit) *deadline_hit = false;
    {
        const int rc = ensure_plan(ctx, ntours, tabu);
        if (rc) return rc;
    }
    // One launch per sweep pays in the latency-bound regime (a few tours in flight: the apply
    // launch is ~30 % of an iteration); in a large batch the separate apply launch serves every
    // tour at once and the leaner sweep wins (measured 7.0e11 vs 5.0e11 evals/s at 64 tours).
    // "how the last descent ran" (tspgpu_info 15, 20, 21, 24): all of it is this call's, whichever branch below returns
    ctx->lp_used = false;
    ctx->sp_used = false;
    ctx->lp_handed = false;
    if (!tabu && ntours == 1 && resident_wanted(ctx)) {
        bool ran = false;
        const int rc = run_persist(ctx, slot0, &time_left_s, deadline_hit, &ran);     // (half way handed over: time_left_s = what is left)
        if (rc) return rc;
        if (ran) return E_OK;
        if (ctx->lp_handed) return run_rebased(ctx, slot0, max_iters, time_left_s, deadline_hit);
        if (ctx->opt_persist == 2) return fail(ctx, E_EXHAUSTED, "the LDS-resident descent does not apply (uint16 cells, n in [64, ~5400], one idle chip)");
    }
    bool stream = !tabu && ntours == 1 && ctx->opt_stream == 2;
    if (!tabu && ntours == 1 && ctx->opt_stream == 1 && resident_wanted(ctx)) {      // (PERSIST = 2 does not get here)
        // automatic: where the LDS-resident kernels do not take the instance
        // (one 16-byte vector per thread: n <= 8192; with two the kernel is at the register limit and the one-launch-per-sweep
        // kernel is faster: n = 12288 65.6 vs 56.5 us per sweep)
        stream = ctx->ld / 8 <= 1024 && plan::resident(plan_in(ctx), false).form == plan::Form::NONE;
    }
    if (stream) {
        ctx->lp_handed = false;
        bool ran = false;
        const int rc = run_pstream(ctx, slot0, &time_left_s, deadline_hit, &ran);
        if (rc) return rc;
        if (ran) return E_OK;
        if (ctx->lp_handed) return run_rebased(ctx, slot0, max_iters, time_left_s, deadline_hit);
        if (ctx->opt_stream == 2) return fail(ctx, E_EXHAUSTED, "the streamed persistent descent does not apply (uint16 cells, n in [1024, 16384), one idle chip)");
    }
    return run_sweeps_plain(ctx, slot0, ntours, tabu, max_iters, time_left_s, deadline_hit);
}

static int run_sweeps_plain(tspgpu_ctx *ctx, int slot0, int ntours, bool tabu, long max_iters, double time_left_s, bool *deadline_hit)
{
    if (!tabu && ctx->symmetric && fused_kernel(ctx->elem, ctx->plan.NCH, ctx->plan.kernel, ctx->plan.pipe2) &&
        (ctx->opt_fused == 2 || (ctx->opt_fused == 1 && ntours <= 4)))
        return run_fused(ctx, slot0, ntours, time_left_s, deadline_hit);
    const double t_end = deadline_of(time_left_s);
    const int K = std::max(1, ctx->opt_batch);
    long issued = 0;
    double iter_dt = est_iter_s(ctx, ntours);   // seconds per (sweep, apply) pair: estimate, then measured
    for (;;) {
        int todo = K;
        if (max_iters >= 0) todo = (int)std::min<long>(K, max_iters - issued);
        if (todo <= 0) break;
        double t_batch = 0;
        if (t_end >= 0) {
            t_batch = now_s();
            if (t_batch >= t_end) { if (deadline_hit) *deadline_hit = true; break; }
            if (t_end - t_batch < 3.0 * K * iter_dt) todo = 1;
        }
        const bool use_graph = ctx->opt_graph && !ctx->opt_timing && todo == K;
        if (use_graph) {
            const int rc = replay_graph(ctx, slot0, ntours, (int)tabu, K, [&](int) {
                const int r = launch_sweep(ctx, slot0, ntours, tabu);
                return r ? r : launch_apply(ctx, slot0, ntours, tabu, tabu);
            });
            if (rc) return rc;
        } else {
            if (ctx->opt_timing) { const int rc = ensure_events(ctx, 2 * K); if (rc) return rc; }
            for (int i = 0; i < todo; i++) {
                if (ctx->opt_timing) HIP_TRY(hipEventRecord(ctx->ev[2 * i], ctx->stream));
                int rc = launch_sweep(ctx, slot0, ntours, tabu);
                if (rc) return rc;
                if (ctx->opt_timing) HIP_TRY(hipEventRecord(ctx->ev[2 * i + 1], ctx->stream));
                rc = launch_apply(ctx, slot0, ntours, tabu, tabu);
                if (rc) return rc;
            }
        }
        HIP_TRY(hipMemcpyAsync(ctx->h_status, ctx->S.done + slot0, (size_t)ntours * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (ctx->opt_timing)
            HIP_TRY(hipMemcpyAsync(ctx->h_status + ctx->tcap, ctx->S.nsweeps + slot0, (size_t)ntours * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (t_end >= 0) iter_dt = (now_s() - t_batch) / todo;
        if (ctx->opt_timing) {
            // count only launches that did work: once every tour is done a sweep exits at once
            int live = 0;
            for (int i = 0; i < ntours; i++) live = std::max(live, ctx->h_status[ctx->tcap + i]);
            for (int i = 0; i < todo && issued + i < live; i++) {
                float ms = 0;
                HIP_TRY(hipEventElapsedTime(&ms, ctx->ev[2 * i], ctx->ev[2 * i + 1]));
                ctx->sweep_ms_total += ms; ctx->sweep_launches++;
            }
        }
        issued += todo;
        bool all = true;
        for (int i = 0; i < ntours; i++) if (!ctx->h_status[i]) { all = false; break; }
        if (all) break;
    }
    return E_OK;
}

// host: successor array -> visiting order from node 0; validates the cycle
static int succ_to_order(tspgpu_ctx *ctx, const int *path, std::vector<int> &ord)
{
    const int n = ctx->n;
    ord.resize(n);
    std::vector<unsigned char> seen(n, 0);
    int v = 0;
    for (int p = 0; p < n; p++) {
        if (v < 0 || v >= n || seen[v]) return fail(ctx, E_INVALID, "path is not a single n-cycle");
        seen[v] = 1; ord[p] = v; v = path[v];
    }
    if (v != 0) return fail(ctx, E_INVALID, "path is not a single n-cycle");
    return E_OK;
}

static int init_slots(tspgpu_ctx *ctx, int slot0, int ntours, int cap)
{
    const int n = ctx->n;
    int *caps = nullptr;
    if (cap >= 0) {
        std::vector<int> h(ntours, cap);
        HIP_TRY(hipMemcpyAsync(ctx->d_caps, h.data(), (size_t)ntours * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream)); // h goes out of scope
        caps = ctx->d_caps;
    }
    const int BT = std::min(1024, std::max(64, pow2_ceil(n / 4)));
    ELEM_SWITCH(ctx->elem, T, hipLaunchKernelGGL((k_tour_init<T>), dim3(ntours), dim3(BT), 0, ctx->stream, ctx->S,
                                                 (const T *)ctx->d_mat.p, n, ctx->ld, slot0, caps, ctx->d_pts, ctx->kind));
    HIP_TRY(hipGetLastError());
    return E_OK;
}

static int need_costs(tspgpu_ctx *ctx)
{
    if (!ctx->have_costs) return fail(ctx, E_PRECOND, "no cost matrix: call tspgpu_build_costs or tspgpu_set_costs first");
    return E_OK;
}

static int load_path(tspgpu_ctx *ctx, int slot, const int *path, int cap)
{
    std::vector<int> ord;
    int rc = succ_to_order(ctx, path, ord);
    if (rc) return rc;
    rc = ensure_tours(ctx, std::max(slot + 1, 1));
    if (rc) return rc;
    // through a pinned buffer of the context: the copy is asynchronous and the call does not wait for it (an event guards
    // the buffer's reuse) -- one host synchronisation less per descent (~15 us; a VNS iteration is ~5 sweeps)
    const size_t n = (size_t)ctx->n;
    if (ctx->h_ord.n < n) {
        if (ctx->h_ord) HIP_TRY(hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx->h_ord.reserve(n));
        if (!ctx->ev_ord) HIP_TRY(hipEventCreateWithFlags(&ctx->ev_ord, hipEventDisableTiming));
        ctx->ord_pending = false;
    }
    if (ctx->ord_pending) { HIP_TRY(hipEventSynchronize(ctx->ev_ord)); ctx->ord_pending = false; }
    memcpy(ctx->h_ord, ord.data(), n * 4);
    HIP_TRY(hipMemcpyAsync(ctx->S.ord + (size_t)slot * n, ctx->h_ord, n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev_ord, ctx->stream));
    ctx->ord_pending = true;
    if ((rc = init_slots(ctx, slot, 1, cap))) return rc;
    mark_slots(ctx, slot, 1, true);
    return E_OK;
}

static int store_path(tspgpu_ctx *ctx, int slot, int *path, double *cost, double *last_delta)
{
    const int n = ctx->n;
    if (path) HIP_TRY(hipMemcpyAsync(path, ctx->S.succ + (size_t)slot * n, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (cost) HIP_TRY(hipMemcpyAsync(cost, ctx->S.cost + slot, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (last_delta) HIP_TRY(hipMemcpyAsync(last_delta, ctx->S.last_delta + slot, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return E_OK;
}

// Uniform grid over the points (k_nn_grid): G x G square cells over the bounding box, about three points per cell
// of the box's area (refined while a cell holds more than 32 and the cell table stays O(n)), cells row-major, points
// counting-sorted by cell.  Instances the grid cannot spread (more than 256 points in one cell: massive duplicates)
// keep the matrix / strided kernels.
static int build_grid(tspgpu_ctx *ctx, const double *xy, int n, double x0, double x1, double y0, double y1)
{
    ctx->drop_grid();
    const double w = x1 - x0, h = y1 - y0, extent = std::max(w, h);
    if (!(extent >= 0) || !std::isfinite(extent)) return E_OK;        // NaN / inf coordinates: no grid
    int G = 1;
    double cell = 1.0;
    std::vector<int> cid(n), cnt;
    int max_occ = n;
    if (extent > 0) {
        const double area = std::max(w, extent * 1e-3) * std::max(h, extent * 1e-3);
        cell = std::sqrt(area * 3.0 / n);
        for (int round = 0; round < 4; round++) {
            G = (int)std::min(4096.0, std::max(1.0, std::ceil(extent / cell)));
            while ((double)G * G > 64.0 * n + 4096.0) G = G * 3 / 4;
            cell = extent / G * (1.0 + 1e-12);
            const double inv = 1.0 / cell;
            cnt.assign((size_t)G * G, 0);
            max_occ = 0;
            for (int i = 0; i < n; i++) {
                const int cx = std::min(G - 1, std::max(0, (int)((xy[2 * i] - x0) * inv)));
                const int cy = std::min(G - 1, std::max(0, (int)((xy[2 * i + 1] - y0) * inv)));
                cid[i] = cy * G + cx;
                max_occ = std::max(max_occ, ++cnt[cid[i]]);
            }
            if (max_occ <= 32 || (double)(2 * G) * (2 * G) > 64.0 * n + 4096.0 || G >= 2048) break;
            cell *= 0.5;
        }
    } else {
        cnt.assign(1, n);
        std::fill(cid.begin(), cid.end(), 0);
    }
    ctx->grid_max_occ = max_occ;
    if (max_occ > 256) return E_OK;
    const size_t C = (size_t)G * G;
    std::vector<int> cstart(C + 1, 0), gidx(n), gpos(n);
    for (size_t c = 0; c < C; c++) cstart[c + 1] = cstart[c] + cnt[c];
    std::vector<int> fill(cstart.begin(), cstart.end() - 1);
    for (int i = 0; i < n; i++) { const int p = fill[cid[i]]++; gidx[p] = i; gpos[i] = p; }   // node order inside a cell
    std::vector<double> gxy((size_t)2 * n);
    std::vector<int> gcell(n);
    for (int p = 0; p < n; p++) {
        gxy[2 * p] = xy[2 * gidx[p]]; gxy[2 * p + 1] = xy[2 * gidx[p] + 1];
        const int c = cid[gidx[p]];
        gcell[p] = (c % G) | ((c / G) << 16);
    }
    HIP_TRY(tspmem::alloc_all<HipMem>({{&ctx->d_gxy, (size_t)n}, {&ctx->d_gidx, (size_t)n}, {&ctx->d_gpos, (size_t)n},
                                       {&ctx->d_cstart, C + 1}, {&ctx->d_gcell, (size_t)n}}));
    HIP_TRY(hipMemcpy(ctx->d_gcell, gcell.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ctx->d_gxy, gxy.data(), (size_t)n * sizeof(double2), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ctx->d_gidx, gidx.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ctx->d_gpos, gpos.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ctx->d_cstart, cstart.data(), (C + 1) * 4, hipMemcpyHostToDevice));
    ctx->grid_G = G; ctx->grid_x0 = x0; ctx->grid_y0 = y0; ctx->grid_cell = cell; ctx->grid_inv = extent > 0 ? 1.0 / cell : 0.0;
    ctx->grid_eps = 1e-7 * cell + 1e-9 * (std::fabs(x0) + std::fabs(x1) + std::fabs(y0) + std::fabs(y1) + extent);
    ctx->grid_ok = true;
    return E_OK;
}

template <int KIND> static const void *nn_grid_fn(bool lds_pts, bool lds_cs, bool key32, int knn = 0)
{
    if (knn == 1) return (const void *)k_nn_grid<KIND, true, true, true, 1>;
    if (knn == 2 && key32) return lds_cs ? (const void *)k_nn_grid<KIND, false, true, true, 2> : (const void *)k_nn_grid<KIND, false, false, true, 2>;
    if (knn == 2) return lds_cs ? (const void *)k_nn_grid<KIND, false, true, false, 2> : (const void *)k_nn_grid<KIND, false, false, false, 2>;
    if (lds_pts && lds_cs) return key32 ? (const void *)k_nn_grid<KIND, true, true, true> : (const void *)k_nn_grid<KIND, true, true, false>;
    if (lds_pts) return (const void *)k_nn_grid<KIND, true, false, false>;
    return lds_cs ? (const void *)k_nn_grid<KIND, false, true, false> : (const void *)k_nn_grid<KIND, false, false, false>;
}

// NN tours from h_starts into ord[] / cost[] of slots [slot0, slot0+count).  The slots are NOT complete tour states
// afterwards (init_slots derives pos / succ / edge costs); they are marked invalid here and valid again by the callers
// that run init_slots.  Fails with INVALID_ARGUMENT when a tour could not be completed (an unvisited node without an
// admissible edge: NOT_CONNECTED entries) -- the reference ends with an invalid tour there (heuristics.c:266-272).
static int launch_nn(tspgpu_ctx *ctx, int slot0, const int *h_starts, int count)
{
    const int n = ctx->n;
    for (int i = 0; i < count; i++)
        if (h_starts[i] < 0 || h_starts[i] >= n) return fail(ctx, E_UNAVAILABLE, "starting node %d not in [0,%d)", h_starts[i], n);
    mark_slots(ctx, slot0, count, false);
    HIP_TRY(hipMemcpyAsync(ctx->d_starts, h_starts, (size_t)count * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    bool launched = false;
    // weights that come from the points (built matrix or matrix-free, integer weights below 2^27): the grid kernel
    if (ctx->built && ctx->grid_ok && ctx->opt_nn != 1 && ctx->cost_bound < 134217728.0) {
        GridArgs A;
        A.S = ctx->S; A.n = n; A.slot0 = slot0; A.starts = ctx->d_starts;
        A.gxy = ctx->d_gxy; A.gidx = ctx->d_gidx; A.gcell = ctx->d_gcell; A.gpos = ctx->d_gpos; A.cstart = ctx->d_cstart;
        A.G = ctx->grid_G; A.cell = ctx->grid_cell; A.eps = ctx->grid_eps;
        const size_t nwords = ((size_t)n + 31) / 32, ncs = (size_t)ctx->grid_G * ctx->grid_G + 1;
        size_t lds = ((nwords + 3) & ~(size_t)3) * 4 + NN_TAIL * 4;
        const bool lc = ncs * 4 <= 48 * 1024;
        if (lc) lds += ((ncs + 3) & ~(size_t)3) * 4;
        // a single tour (or a handful) is latency-bound: points, node ids and cells in LDS; batches keep the LDS for occupancy
        const bool lp = count <= ctx->cus && lds + (size_t)n * 24 + 64 <= ctx->lds_max;
        if (lp) lds += (size_t)n * 24;
        const bool key32 = ctx->cost_bound < 32767.0 && n <= 131072;      // (weight << 17 | node) in one 32-bit word, below the "none" key
        const int kind = ctx->ceil_int() ? KIND_CEIL_INT : ctx->kind;
        // ... and, where they fit beside them, the 3 nearest neighbours of every point (built once per instance)
        // (in LDS for a single tour; batches and tours whose points do not fit LDS read them from global memory)
        // (weights past the 32-bit key -- pla85900 -- keep the 64-bit candidate scan but take the lists from global memory as well:
        // a listed neighbour's weight is below 2^15 by construction)
        const int knn = ctx->opt_nn == 3 || n > 131072 ? 0 : !key32 ? (lp ? 0 : 2)
                      : (lp && lc && lds + (size_t)n * NN_K * 4 <= ctx->lds_max) ? 1 : !lp ? 2 : 0;
        A.knn = nullptr;
        if (knn) {
            if (!ctx->d_knn) {
                HIP_TRY(ctx->d_knn.alloc((size_t)n * NN_K));
                const dim3 g((n + 255) / 256), b(256);
                if (kind == TSPGPU_EUC_2D) hipLaunchKernelGGL((k_knn_build<TSPGPU_EUC_2D>), g, b, 0, ctx->stream, A, ctx->d_knn);
                else if (kind == TSPGPU_ATT) hipLaunchKernelGGL((k_knn_build<TSPGPU_ATT>), g, b, 0, ctx->stream, A, ctx->d_knn);
                else if (kind == KIND_CEIL_INT) hipLaunchKernelGGL((k_knn_build<KIND_CEIL_INT>), g, b, 0, ctx->stream, A, ctx->d_knn);
                else hipLaunchKernelGGL((k_knn_build<TSPGPU_CEIL_2D>), g, b, 0, ctx->stream, A, ctx->d_knn);
                HIP_TRY(hipGetLastError());
            }
            A.knn = ctx->d_knn;
            if (knn == 1) lds += (size_t)n * NN_K * 4;
        }
        const void *fn = kind == TSPGPU_EUC_2D ? nn_grid_fn<TSPGPU_EUC_2D>(lp, lc, key32, knn) : kind == TSPGPU_ATT ? nn_grid_fn<TSPGPU_ATT>(lp, lc, key32, knn)
                       : kind == KIND_CEIL_INT ? nn_grid_fn<KIND_CEIL_INT>(lp, lc, key32, knn) : nn_grid_fn<TSPGPU_CEIL_2D>(lp, lc, key32, knn);
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        void *args[] = {&A};
        HIP_TRY(hipLaunchKernel(fn, dim3(count), dim3(64), args, lds, ctx->stream));
        launched = true;
    }
    if (!launched && ctx->d_mat && !ctx->otf) {
        // matrix mode: vector row reads, one or two 16-byte vectors per thread where n allows
        const int V = 16 / (int)elem_size(ctx->elem), nvec = ctx->ld / V;
        int BT = std::min(1024, std::max(64, (nvec + 63) & ~63));
        if ((nvec + BT - 1) / BT <= 16) {
            ELEM_SWITCH(ctx->elem, T, hipLaunchKernelGGL((k_nn_vec<T>), dim3(count), dim3(BT), 0, ctx->stream, ctx->S,
                                                         (const T *)ctx->d_mat.p, n, ctx->ld, slot0, ctx->d_starts));
            HIP_TRY(hipGetLastError());
            launched = true;
        }
    }
    if (!launched) {
        int BT = std::min(1024, std::max(64, pow2_ceil(n / 4)));
        while ((long)BT * 128 < n && BT < 1024) BT *= 2; // register visited mask: n <= 128*BT
        if ((long)BT * 128 < n) return fail(ctx, E_EXHAUSTED, "nn kernel supports n <= 131072");
        ELEM_SWITCH(ctx->elem, T, hipLaunchKernelGGL((k_nn<T>), dim3(count), dim3(BT), 0, ctx->stream, ctx->S,
                                                     (const T *)ctx->d_mat.p, n, ctx->ld, slot0, ctx->d_starts, ctx->d_pts, ctx->kind));
        HIP_TRY(hipGetLastError());
    }
    // Only a caller matrix can hold NOT_CONNECTED off the diagonal; built matrices never leave a tour open.
    if (!ctx->built) {
        HIP_TRY(hipMemcpyAsync(ctx->h_status, ctx->S.status + slot0, (size_t)count * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < count; i++)
            if (ctx->h_status[i])
                return fail(ctx, E_INVALID, "nearest-neighbour tour from start %d is incomplete: a node has no admissible edge left (NOT_CONNECTED entries)", h_starts[i]);
    }
    return E_OK;
}

// ---- what the entry points of every move family share ------------------------------------------------------------------

// (what a descent did on one tour, and its way to the caller's arrays: Descent, DescentOut, descent_out of tspgpu_descent.h)

// Host tour in, host tour out, for an entry point that has checked its arguments: the family's check, the tour into slot 0
// (load_path recomputes its cost, refinment.c:6-9; keep_cost: the caller's running cost instead, as ref_2opt_once),
// body(&late), the tour and its cost back.
template <typename B> static int with_host_tour(tspgpu_ctx *ctx, int *path, double *cost, bool keep_cost, int (*check)(tspgpu_ctx *), B &&body)
{
    hipSetDevice(ctx->device);
    int rc = check(ctx);
    if (rc) return rc;
    if ((rc = load_path(ctx, 0, path, -1))) return rc;
    if (keep_cost) HIP_TRY(hipMemcpyAsync(ctx->S.cost, cost, 8, hipMemcpyHostToDevice, ctx->stream));
    bool late = false;
    if ((rc = body(&late))) return rc;
    if ((rc = store_path(ctx, 0, path, cost, nullptr))) return rc;
    return done_code(late);
}

// the same on a slot that must hold a tour: the family's check, the slot's, body(&late).  keeps_looks: the body keeps the
// slot's awake sets itself ("Don't-look bits"); after any other body every node is awake
template <typename B> static int with_slot(tspgpu_ctx *ctx, int slot, int (*check)(tspgpu_ctx *), B &&body, bool keeps_looks = false)
{
    hipSetDevice(ctx->device);
    int rc = check(ctx);
    if (rc) return rc;
    if ((rc = need_slot(ctx, slot))) return rc;
    if (!keeps_looks) wake_slots(ctx, slot, 1);
    bool late = false;
    if ((rc = body(&late))) return rc;
    return done_code(late);
}

struct MultiStart {
    Descent total;          // summed over every start that was processed
    int m_last = 0;         // tours of the last chunk processed: they are still in slots 0 .. m_last - 1
};

// The multi-start of every family: the start list (nullptr: nodes 0 .. nstarts - 1) in chunks of TSPGPU_OPT_MAX_TOURS tours.
// Per chunk of m: the nearest-neighbour tours into slots 0 .. m - 1, their edge costs with sweep cap `cap`,
// descend(m, time left, &late, Descent[m]) -- the family's descent over those slots, the only thing a family supplies --, the
// costs back, the incumbent's tour stored.  A chunk in which the deadline strikes is the last one; it still counts.
template <typename F>
static int multistart(tspgpu_ctx *ctx, const int *starts, int nstarts, double time_left_s, int cap, int *best_path, double *best_cost,
                      int *best_start, double *costs_out, MultiStart *out, F &&descend)
{
    const double t_end = deadline_of(time_left_s);
    const int chunk = std::min(nstarts, ctx->opt_max_tours);
    int rc = ensure_tours(ctx, chunk);
    if (rc) return rc;
    double best = DBL_MAX; int arg = -1;
    bool late = false;
    std::vector<int> hs(chunk);
    std::vector<Descent> D(chunk);
    for (int base = 0; base < nstarts && !late; base += chunk) {
        const int m = std::min(chunk, nstarts - base);
        for (int i = 0; i < m; i++) hs[i] = starts ? starts[base + i] : base + i;
        if ((rc = launch_nn(ctx, 0, hs.data(), m))) return rc;
        if ((rc = init_slots(ctx, 0, m, cap))) return rc;
        mark_slots(ctx, 0, m, true);
        const double left = t_end >= 0 ? std::max(0.0, t_end - now_s()) : -1;
        if ((rc = descend(m, left, &late, D.data()))) return rc;
        HIP_TRY(hipMemcpyAsync(ctx->h_costs, ctx->S.cost, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        int win = -1;
        for (int i = 0; i < m; i++) {
            out->total += D[i];
            if (costs_out) costs_out[base + i] = ctx->h_costs[i];
            if (ctx->h_costs[i] < best) { best = ctx->h_costs[i]; win = i; }    // strict <, tsp.c:671: ties to the earliest entry
        }
        if (win >= 0) {
            arg = hs[win];
            if ((rc = store_path(ctx, win, best_path, nullptr, nullptr))) return rc;
        }
        out->m_last = m;
    }
    *best_cost = best; *best_start = arg;
    return done_code(late);
}

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

int tspgpu_device_count(void)
{
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

int tspgpu_create(int device, tspgpu_ctx **out)
{
    if (!out) return E_INVALID;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return E_UNAVAILABLE;
    if (device < 0 || device >= count) return E_INVALID;
    tspgpu_ctx *ctx = new tspgpu_ctx();
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess) { delete ctx; return E_UNAVAILABLE; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { delete ctx; return E_UNAVAILABLE; }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        // the code object is gfx950-only; say so instead of failing at first launch
        fprintf(stderr, "tspgpu: device %d is %s, this library is built for gfx950\n", device, prop.gcnArchName);
        delete ctx; return E_UNAVAILABLE;
    }
    ctx->cus = prop.multiProcessorCount;
    // gfx950: 160 KiB of LDS per CU, and one workgroup may take all of it
    // (MI355X_MICROARCH.md, register files / LDS); the generic attribute still says 64 KiB.
    ctx->lds_max = 160 * 1024;
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return E_INTERNAL; }
    if (ctx->d_flags.alloc(16) != hipSuccess) { delete ctx; return E_INTERNAL; }
    *out = ctx;
    return E_OK;
}

void tspgpu_destroy(tspgpu_ctx *ctx)
{
    if (!ctx) return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    if (ctx->ev_ord) hipEventDestroy(ctx->ev_ord);
    for (auto e : ctx->ev) hipEventDestroy(e);
    drop_graphs(ctx);
    const hipStream_t stream = ctx->stream;
    delete ctx;                 // every group frees what it holds, before the stream it was filled on goes
    hipStreamDestroy(stream);
}

const char *tspgpu_last_error(const tspgpu_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int tspgpu_set_option(tspgpu_ctx *ctx, int option, long value)
{
    if (!ctx) return E_INVALID;
    hipSetDevice(ctx->device);
    switch (option) {
    case TSPGPU_OPT_ELEM: if (value < 0 || value > 3) return fail(ctx, E_INVALID, "bad element kind"); ctx->opt_elem = (int)value; break;
    case TSPGPU_OPT_KERNEL: if (value < 0 || value > 3) return fail(ctx, E_INVALID, "bad kernel id"); ctx->opt_kernel = (int)value; drop_plan(ctx); break;
    case TSPGPU_OPT_BATCH: if (value < 1 || value > 4096) return fail(ctx, E_INVALID, "bad batch"); ctx->opt_batch = (int)value; drop_graphs(ctx); break;
    case TSPGPU_OPT_WGS_PER_TOUR: if (value < 0 || value > MAX_WGS_PER_TOUR) return fail(ctx, E_INVALID, "bad wgs"); ctx->opt_wgs = (int)value; drop_plan(ctx); break;
    case TSPGPU_OPT_HISTORY: {
        if (value < 0 || value > (1 << 22)) return fail(ctx, E_INVALID, "bad history size");
        drop_graphs(ctx);       // (captured launches hold the old arrays: they go first, so a failure below leaves "no history")
        tspmem::reset_all(ctx->hist_a, ctx->hist_b, ctx->hist_d);
        ctx->hist = HistBuf{nullptr, nullptr, nullptr, 0}; ctx->opt_hist = 0;
        if (value > 0) {
            HIP_TRY(tspmem::alloc_all<HipMem>({{&ctx->hist_a, (size_t)value}, {&ctx->hist_b, (size_t)value}, {&ctx->hist_d, (size_t)value}}));
            ctx->hist = HistBuf{ctx->hist_a, ctx->hist_b, ctx->hist_d, (int)value};
        }
        ctx->opt_hist = (int)value;
        break;
    }
    case TSPGPU_OPT_GRAPH: ctx->opt_graph = value ? 1 : 0; break;
    case TSPGPU_OPT_TIMING: ctx->opt_timing = value ? 1 : 0; break;
    case TSPGPU_OPT_BLOCK: if (value < 0 || value > 1024) return fail(ctx, E_INVALID, "bad block"); ctx->opt_block = (int)value; drop_plan(ctx); break;
    case TSPGPU_OPT_DEPTH: if (value < 0 || value > 8) return fail(ctx, E_INVALID, "bad depth"); ctx->opt_depth = (int)value; drop_plan(ctx); break;
    case 99: ctx->opt_ablate = (int)value; drop_graphs(ctx); break; // undocumented: kernel ablation for profiling
    case 88: ctx->opt_lp_no_tmat = value ? 1 : 0; break; // undocumented: the shaped k_lds2opt that reloads moved rows from the matrix, not from the tour-ordered copy (tests)
    case 89: ctx->opt_lp_generic = value ? 1 : 0; break; // undocumented: the generic k_lds2opt where a shaped instantiation exists (tests)
    case 90: ctx->opt_or_otf_early = value == 1 || value == 2 ? (int)value : 0; break; // undocumented: see or_otf_early()
    case 91: ctx->opt_otf_early = value == 1 || value == 2 ? (int)value : 0; drop_plan(ctx); break; // undocumented: see plan::otf_early()
    case 92: ctx->opt_build_tile = (int)value; break; // undocumented: tile of the triangle build (tools/build_probe.py)
    case 93: ctx->opt_sp_nch = value == 1 || value == 2 ? (int)value : 0; break; // undocumented: vectors per thread of k_str2opt (tools/stream_probe.py)
    case 94: ctx->opt_vns_launch_k = value > 0 ? (int)std::min<long>(value, 65536) : 65536; break; // undocumented: VNS iterations per launch (tests)
    case 95: ctx->opt_lp_poll_sleep = (int)value; break; // undocumented: s_sleep(1) repetitions between polls of the exchange slots (tools/persist_probe.py)
    case 96: ctx->opt_lp_fail_at = (int)value; break; // undocumented: see opt_lp_fail_at (tests)
    case 97: ctx->opt_lp_hello = value ? value : 200000; ctx->lp_gate.rearm(); break; // undocumented: rendezvous limit of k_lds2opt (tests)
    case 98: // undocumented: per-workgroup phase stamps of the pipelined sweep (single tour)
        ctx->opt_stamps = value ? 1 : 0; drop_graphs(ctx);
        if (value) HIP_TRY(ctx->d_stamps.reserve((size_t)MAX_WGS_PER_TOUR * 64));
        if (value) HIP_TRY(hipMemset(ctx->d_stamps, 0, (size_t)MAX_WGS_PER_TOUR * 64 * 8));
        break;
    case TSPGPU_OPT_MATRIX_FREE: if (value < 0 || value > 2) return fail(ctx, E_INVALID, "bad matrix-free mode"); ctx->opt_otf = (int)value; break;
    case TSPGPU_OPT_FUSED: if (value < 0 || value > 2) return fail(ctx, E_INVALID, "bad fused mode"); ctx->opt_fused = (int)value; break;
    case TSPGPU_OPT_MAX_TOURS: if (value < 1 || value > (1 << 20)) return fail(ctx, E_INVALID, "bad max tours"); ctx->opt_max_tours = (int)value; break;
    case TSPGPU_OPT_PERSIST: if (value < 0 || value > 2) return fail(ctx, E_INVALID, "bad persist mode"); ctx->opt_persist = (int)value; ctx->lp_gate.rearm(); break;
    case TSPGPU_OPT_STREAM_PERSIST: if (value < 0 || value > 2) return fail(ctx, E_INVALID, "bad stream-persist mode"); ctx->opt_stream = (int)value; ctx->lp_gate.rearm(); break;
    case TSPGPU_OPT_PERSIST_EDGES: if (value < 0 || value > LW_EMAX) return fail(ctx, E_INVALID, "edges per workgroup: 0 (auto) .. %d", LW_EMAX); ctx->opt_persist_edges = (int)value; break;
    case TSPGPU_OPT_BUILD_KERNEL: if (value < 0 || value > 1) return fail(ctx, E_INVALID, "bad build kernel"); ctx->opt_build = (int)value; break;
    case TSPGPU_OPT_PERSIST_WINDOW: if (value < 0 || value > 2) return fail(ctx, E_INVALID, "bad window mode"); ctx->opt_persist_window = (int)value; break;
    case TSPGPU_OPT_PIPE2: if (value < 0 || value > 1) return fail(ctx, E_INVALID, "bad pipe2 mode"); ctx->opt_pipe2 = (int)value; drop_plan(ctx); break;
    case TSPGPU_OPT_NN_KERNEL: if (value < 0 || value > 3) return fail(ctx, E_INVALID, "bad NN kernel id"); ctx->opt_nn = (int)value; break;
    case TSPGPU_OPT_EM_FORM: if (value < 0 || value > 2) return fail(ctx, E_INVALID, "bad Extra Mileage form"); ctx->opt_em_form = (int)value; break;
    case TSPGPU_OPT_OR_MATRIX_FREE: if (value < 0 || value > 1) return fail(ctx, E_INVALID, "bad matrix-free Or-opt mode"); ctx->opt_or_otf = (int)value; break;
    case TSPGPU_OPT_SWEEP_CAP: if (value < -1 || value > INT_MAX) return fail(ctx, E_INVALID, "bad sweep cap"); ctx->opt_sweep_cap = (int)value; break;
    default: return fail(ctx, E_INVALID, "unknown option %d", option);
    }
    return E_OK;
}

static int or_single_R(const tspgpu_ctx *ctx);      // (tspgpu_oropt.inc's driver, below)
static int or_single_geom(const tspgpu_ctx *ctx, bool nch);
static int m2_geom(const tspgpu_ctx *ctx, int what);       // (tspgpu_multi2opt.inc's driver, below)

long tspgpu_info(const tspgpu_ctx *ctx, int what)
{
    if (!ctx) return -1;
    switch (what) {
    case 0: return ctx->n;
    case 1: return ctx->ld;
    case 2: return ctx->elem;
    case 3: return ctx->plan.kernel;
    case 4: return ctx->plan.G;
    case 5: return (long)ctx->plan.lds;
    case 6: return ctx->plan.BT;
    case 7: return ctx->symmetric ? 1 : 0;
    case 8: return ctx->cus;
    case 9: return ctx->plan.D;
    case 10: return ctx->otf ? 1 : 0;
    case 11: return (ctx->symmetric && ctx->opt_fused && fused_kernel(ctx->elem, ctx->plan.NCH, ctx->plan.kernel, ctx->plan.pipe2)) ? 1 : 0;
    case 14: return (ctx->plan.pipe2 || ctx->plan.pipe2_sweep) ? 1 : 0;
    case 15: return ctx->lp_used ? 1 : 0;
    case 16: case 17: case 18: case 19: {    // geometry of the LDS-resident descent (0: it does not apply to the instance)
        const plan::Resident R = plan::resident(plan_in(ctx), false);
        return what == 16 ? R.W : what == 17 ? R.E : what == 18 ? (long)R.lds : R.Ws;
    }
    case 20: return ctx->lp_used && ctx->lp_window ? 1 : 0;
    case 21: return ctx->lp_handed ? 1 : 0;
    case 22: return ctx->lp_sweeps;
    case 23: return ctx->vns_mode;
    case 24: return ctx->sp_used ? 1 : 0;
    case 25:   // the matrix-free sweep kernel of the current plan (see launch_sweep)
        if (!ctx->otf || ctx->plan.kernel != 4) return 0;
        return !plan::otf8(ctx->cost_bound, ctx->n) ? 1 : ctx->plan.otf_early ? 3 : 2;
    case 26: return ctx->have_points && ctx->ceil_int() ? 1 : 0;   // CEIL_2D weights by the integer ceil-sqrt (edge_w<KIND_CEIL_INT>)
    case 27: return ctx->em_form;
    case 28: return ctx->em_stale;
    case 29: return ctx->em_steps;
    case 30: return ctx->or_batch_R;
    case 31: return or_single_R(ctx);
    case 32: return or_single_geom(ctx, false);
    case 33: return or_single_geom(ctx, true);
    case 34: return ctx->or_otf_form;
    case 35: return ctx->or_otf_R;
    case 36: return ctx->m2_count.sweeps;
    case 37: return ctx->m2_count.moves;
    case 38: return ctx->m2_count.max_k;
    case 39: return m2_geom(ctx, 0);
    case 40: return m2_geom(ctx, 1);
    case 41: return m2_geom(ctx, 2);
    case 42: return ctx->nl.K;
    case 43: return ctx->nl_count.sweeps;
    case 44: return ctx->nl_count.moves;
    case 45: return ctx->nl_polish_sweeps;
    case 46: return NL_NODES;
    case 47: return ctx->ornl_count.sweeps;
    case 48: return ctx->ornl_count.moves;
    case 49: return ctx->ornl_count.max_k;
    case 50: return ctx->ornl_rounds;
    case 51: return ORNL_STARTS;
    case 52: return ctx->nlb_tours;
    case 53: return ctx->nlb_launches;
    case 54: return ctx->nlb_max_live;
    case 56: return ctx->nlv_walks;
    case 57: return ctx->nlv_iterations;
    case 58: return ctx->nlv_rounds;
    case 59: return ctx->nlv_max_live;
    case 60: return ctx->nlv_dry;
    case 61: return ctx->lp_used && ctx->lp_shaped ? 1 : 0;
    case 62: return ctx->nl3_w;
    case 63: return ctx->nl3_count.sweeps;
    case 64: return ctx->nl3_count.moves;
    case 65: return ctx->nl3_count.max_k;
    case 66: return ctx->nl3_phases;
    case 67: return NL3_NODES;
    case 68: return ctx->lp_used && ctx->lp_shaped && ctx->lp_tmat ? 1 : 0;
    case 69: return ctx->lp_used && ctx->lp_packed ? 1 : 0;
    case 70: return ctx->dl_looked;
    case 71: return ctx->dl_full;
    case 72: return ctx->dl_max_q;
    case 73: return (long)LOOK_WGS_PER_CU * ctx->cus;
    case 74: return ctx->ge_rounds1;
    case 75: return ctx->ge_rounds2;
    case 76: return ctx->ge_edges1;
    case 77: return ctx->ge_free;
    case 78: return ctx->nlb_w3;
    case 79: return ctx->nlb_three_sweeps;
    case 80: return ctx->nlb_three_moves;
    case 81: return ctx->nlb_three_max_k;
    case 82: return ctx->nlb_dl_looked;
    case 83: return ctx->nlb_dl_full;
    case 84: return ctx->nlb_dl_max_q;
    case 86: return ctx->hk_rounds;
    case 87: return ctx->hk_iters;
    case 88: return ctx->hk_reason;
    case 89: return ctx->hk_h;
    case 90: return HK_ROWS;
    case 91: return ctx->hk_lds;
    case 85: return ctx->have_costs && ctx->n >= 8 ? std::min(NLB_QSWEEP_WGS, (ctx->n + ORNL_STARTS - 1) / ORNL_STARTS) : 0;
    case 55: return ctx->have_costs && ctx->symmetric && ctx->n >= 8 ? (ctx->n + ORNL_STARTS - 1) / ORNL_STARTS : 0;
    case 12: return (ctx->built && ctx->grid_ok && ctx->opt_nn != 1 && ctx->cost_bound < 134217728.0) ? ctx->grid_G : 0;
    case 13: return ctx->grid_max_occ;
    }
    return -1;
}

int tspgpu_set_points(tspgpu_ctx *ctx, const double *xy, int n, int edge_weight_type)
{
    if (!ctx || !xy) return fail(ctx, E_INVALID, "null argument");
    if (edge_weight_type < 0 || edge_weight_type > 2) return fail(ctx, E_INVALID, "unknown edge weight type %d", edge_weight_type);
    hipSetDevice(ctx->device);
    int rc = new_instance(ctx, n);
    if (rc) return rc;
    HIP_TRY(ctx->d_pts.alloc((size_t)n));
    HIP_TRY(hipMemcpy(ctx->d_pts, xy, (size_t)n * sizeof(double2), hipMemcpyHostToDevice));
    ctx->kind = edge_weight_type;
    ctx->have_points = true;
    double x0 = xy[0], x1 = xy[0], y0 = xy[1], y1 = xy[1];
    ctx->int_coords = true;
    for (int i = 0; i < 2 * n; i++)
        if (!(std::fabs(xy[i]) < 33554432.0) || xy[i] != std::floor(xy[i])) { ctx->int_coords = false; break; }
    for (int i = 1; i < n; i++) {
        x0 = std::min(x0, xy[2 * i]); x1 = std::max(x1, xy[2 * i]);
        y0 = std::min(y0, xy[2 * i + 1]); y1 = std::max(y1, xy[2 * i + 1]);
    }
    const double diag = std::sqrt((x1 - x0) * (x1 - x0) + (y1 - y0) * (y1 - y0));
    ctx->cost_bound = (edge_weight_type == TSPGPU_ATT ? diag / std::sqrt(10.0) : diag) + 2.0;
    ctx->d_ipts.reset();
    if (ctx->ceil_int()) {
        std::vector<int> ip((size_t)2 * n);
        for (int i = 0; i < n; i++) { ip[2 * i] = (int)(xy[2 * i] - x0); ip[2 * i + 1] = (int)(xy[2 * i + 1] - y0); }
        HIP_TRY(ctx->d_ipts.alloc((size_t)n));
        HIP_TRY(hipMemcpy(ctx->d_ipts, ip.data(), (size_t)n * sizeof(int2), hipMemcpyHostToDevice));
    }
    return build_grid(ctx, xy, n, x0, x1, y0, y1);
}

static int launch_build(tspgpu_ctx *ctx)
{
    const int n = ctx->n, ld = ctx->ld;
    if (ctx->elem == TSPGPU_ELEM_F64) {
        dim3 grid((ld / 2 + 255) / 256, n);
        hipLaunchKernelGGL((k_build_costs<double>), grid, dim3(256), 0, ctx->stream, ctx->d_pts, n, ld, ctx->kind, (double *)ctx->d_mat.p);
    } else {
        const int kind = ctx->ceil_int() ? KIND_CEIL_INT : ctx->kind;
        // one triangle + transposed store (k_build_costs_tri); TSPGPU_OPT_BUILD_KERNEL = 1 keeps the full-matrix form
        const int NT = (n + TRI - 1) / TRI;
        // (uint16 cells only: with int32 cells the 64-byte row segments of the transposed tiles store slower than the
        // arithmetic they save -- measured 27.5 vs 16.7 us at n=4096, tools/build_probe.py)
        const bool tri = ctx->opt_build == 0 && ctx->elem == TSPGPU_ELEM_U16 && n >= 2 * TRI && NT <= 2047;
        const bool f32r = kind == TSPGPU_EUC_2D && ctx->cost_bound < 4.0e6;      // (every root below 2^22)
        // 128 x 128 tiles (256-byte row segments in both halves) from n = 8192 up: measured (tools/build_probe.py) n = 16384 123 vs
        // 131 us, but n = 4096 15.4 vs 11.8 us -- 528 workgroups of four times the arithmetic fill the chip worse than 2080
        const bool big = tri && ctx->opt_build_tile != 64 && (n >= 8192 || (ctx->opt_build_tile == 128 && n >= 1024));
        const int NTB = (n + TRIB - 1) / TRIB;
#define BUILD_INT(T, K) do { if (big && f32r && K == TSPGPU_EUC_2D) hipLaunchKernelGGL((k_build_costs_tri128<T, TSPGPU_EUC_2D, true>), dim3(NTB * (NTB + 1) / 2), dim3(256), 0, ctx->stream, ctx->d_pts, n, ld, NTB, (T *)ctx->d_mat.p); \
                             else if (big) hipLaunchKernelGGL((k_build_costs_tri128<T, K, false>), dim3(NTB * (NTB + 1) / 2), dim3(256), 0, ctx->stream, ctx->d_pts, n, ld, NTB, (T *)ctx->d_mat.p); \
                             else if (tri && f32r && K == TSPGPU_EUC_2D) hipLaunchKernelGGL((k_build_costs_tri<T, TSPGPU_EUC_2D, true>), dim3(NT * (NT + 1) / 2), dim3(256), 0, ctx->stream, ctx->d_pts, n, ld, NT, (T *)ctx->d_mat.p); \
                             else if (tri) hipLaunchKernelGGL((k_build_costs_tri<T, K, false>), dim3(NT * (NT + 1) / 2), dim3(256), 0, ctx->stream, ctx->d_pts, n, ld, NT, (T *)ctx->d_mat.p); \
                             else hipLaunchKernelGGL((k_build_costs_int<T, K>), dim3((ld / (16 / (int)sizeof(T)) + 255) / 256, (n + BUILD_ROWS - 1) / BUILD_ROWS), dim3(256), 0, ctx->stream, \
                                                     ctx->d_pts, n, ld, (T *)ctx->d_mat.p); } while (0)
#define BUILD_KIND(T) do { if (kind == TSPGPU_EUC_2D) BUILD_INT(T, TSPGPU_EUC_2D); else if (kind == TSPGPU_ATT) BUILD_INT(T, TSPGPU_ATT); \
                           else if (kind == KIND_CEIL_INT) BUILD_INT(T, KIND_CEIL_INT); else BUILD_INT(T, TSPGPU_CEIL_2D); } while (0)
        if (ctx->elem == TSPGPU_ELEM_I32) BUILD_KIND(int); else BUILD_KIND(u16);
#undef BUILD_KIND
#undef BUILD_INT
    }
    HIP_TRY(hipGetLastError());
    return E_OK;
}

int tspgpu_build_costs(tspgpu_ctx *ctx, double *host_out)
{
    if (!ctx) return E_INVALID;
    hipSetDevice(ctx->device);
    if (!ctx->have_points) return fail(ctx, E_PRECOND, "no points: call tspgpu_set_points first");
    free_matrix(ctx);
    const size_t cells = (size_t)ctx->n * ctx->ld;
    // every supported edge-weight kind yields integers: AUTO = the narrowest exact storage.
    // cost_bound (from the bounding box of the points) decides whether 16 bits are enough.
    const bool fits16 = ctx->cost_bound <= 65534.0, fits32 = ctx->cost_bound < 134217728.0;
    if (ctx->opt_elem == TSPGPU_ELEM_U16 && !fits16) return fail(ctx, E_INVALID, "uint16 storage requested but costs may reach %.0f", ctx->cost_bound);
    if (ctx->opt_elem == TSPGPU_ELEM_I32 && !fits32) return fail(ctx, E_INVALID, "int32 storage requested but costs may reach %.0f", ctx->cost_bound);
    if (ctx->opt_elem != TSPGPU_ELEM_AUTO) ctx->elem = ctx->opt_elem;
    else ctx->elem = fits16 ? TSPGPU_ELEM_U16 : fits32 ? TSPGPU_ELEM_I32 : TSPGPU_ELEM_F64;
    // matrix-free when asked for, when one matrix row cannot sit in LDS (every matrix sweep
    // gathers c[succ a][succ b] from an LDS row) -- e.g. pla85900: 343 KB per int32 row --, or when n
    // is past the matrix sweeps' 16-bit labels (a uint16 row of up to ~80 900 cells still fits LDS)
    const bool row_fits = (size_t)ctx->ld * elem_size(ctx->elem) + 2048 <= ctx->lds_max;
    const bool labels_fit = ctx->n <= MATRIX_MAX_N;
    ctx->otf = ctx->opt_otf == 1 || (ctx->opt_otf == 0 && (!row_fits || !labels_fit));
    if (ctx->otf) {
        if (!fits32) return fail(ctx, E_EXHAUSTED, "matrix-free mode needs integer costs below 2^27 (bound %.0f)", ctx->cost_bound);
        if (host_out) return fail(ctx, E_INVALID, "matrix-free mode: there is no n x n matrix to copy out (n = %d)", ctx->n);
        ctx->elem = TSPGPU_ELEM_I32;   // integer deltas; no cells are stored
        ctx->symmetric = true;
        ctx->have_costs = true;
        ctx->built = true;
        drop_plan(ctx);
        return E_OK;
    }
    if (!row_fits) return fail(ctx, E_EXHAUSTED, "n = %d: a matrix row does not fit LDS and matrix-free mode is disabled", ctx->n);
    if (!labels_fit) return fail(ctx, E_EXHAUSTED, "n = %d exceeds the matrix-mode limit of %d nodes and matrix-free mode is disabled", ctx->n, MATRIX_MAX_N);
    HIP_TRY(ctx->d_mat.alloc(cells * elem_size(ctx->elem)));
    int rc = launch_build(ctx);
    if (rc) return rc;
    ctx->symmetric = true; // Euclidean
    ctx->max16k = ctx->cost_bound <= 16383.0;
    ctx->max8k = ctx->cost_bound <= 8190.0;
    ctx->have_costs = true;
    ctx->built = true;
    drop_plan(ctx);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (host_out) return tspgpu_get_costs(ctx, host_out);
    return E_OK;
}

int tspgpu_set_costs(tspgpu_ctx *ctx, const double *host_costs, int n)
{
    if (!ctx || !host_costs) return fail(ctx, E_INVALID, "null argument");
    hipSetDevice(ctx->device);
    if (n != ctx->n || !ctx->n) {
        int rc = new_instance(ctx, n);
        if (rc) return rc;
    } else {
        free_matrix(ctx);
    }
    ctx->otf = false;
    ctx->built = false;
    const int ld = ctx->ld;
    const size_t cells = (size_t)n * ld;
    DevBuf<void> owner;          // the matrix as doubles: it becomes the matrix where that is the cell type
    HIP_TRY(owner.alloc(cells * 8));
    double *const stage = static_cast<double *>(owner.p);
    HIP_TRY(hipMemsetAsync(stage, 0, cells * 8, ctx->stream));
    HIP_TRY(hipMemcpy2DAsync(stage, (size_t)ld * 8, host_costs, (size_t)n * 8, (size_t)n * 8, n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(ctx->d_flags, 0, 32, ctx->stream));
    hipLaunchKernelGGL(k_inspect, dim3((n + 255) / 256, n), dim3(256), 0, ctx->stream, stage, n, ld, ctx->d_flags);
    HIP_TRY(hipGetLastError());
    int flags[5] = {0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(flags, ctx->d_flags, 20, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const bool integral = flags[0] == 0, fits16 = flags[2] == 0;
    ctx->max16k = fits16 && flags[3] == 0;
    ctx->max8k = fits16 && flags[4] == 0;
    ctx->symmetric = flags[1] == 0;
    if ((ctx->opt_elem == TSPGPU_ELEM_I32 && !integral) || (ctx->opt_elem == TSPGPU_ELEM_U16 && !fits16)) {
        return fail(ctx, E_INVALID, "integer storage requested but the matrix is not representable (int32: integers in [-1, 2^27); uint16: integers in [0, 65534] with a -1 diagonal)");
    }
    if (ctx->opt_elem != TSPGPU_ELEM_AUTO) ctx->elem = ctx->opt_elem;
    else ctx->elem = fits16 ? TSPGPU_ELEM_U16 : integral ? TSPGPU_ELEM_I32 : TSPGPU_ELEM_F64;
    if (ctx->elem == TSPGPU_ELEM_F64) {
        ctx->d_mat = std::move(owner);
    } else {
        HIP_TRY(ctx->d_mat.alloc(cells * elem_size(ctx->elem)));
        if (ctx->elem == TSPGPU_ELEM_I32)
            hipLaunchKernelGGL((k_from_f64<int>), dim3((ld + 255) / 256, n), dim3(256), 0, ctx->stream, stage, n, ld, (int *)ctx->d_mat.p);
        else
            hipLaunchKernelGGL((k_from_f64<u16>), dim3((ld + 255) / 256, n), dim3(256), 0, ctx->stream, stage, n, ld, (u16 *)ctx->d_mat.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    ctx->have_costs = true;
    drop_plan(ctx);
    return E_OK;
}

int tspgpu_get_costs(tspgpu_ctx *ctx, double *host_out)
{
    if (!ctx || !host_out) return fail(ctx, E_INVALID, "null argument");
    hipSetDevice(ctx->device);
    int rc = need_costs(ctx);
    if (rc) return rc;
    if (ctx->otf) return fail(ctx, E_PRECOND, "matrix-free mode: no matrix is held");
    const int n = ctx->n, ld = ctx->ld;
    const double *src = (const double *)ctx->d_mat.p;
    DevBuf<double> tmp;
    if (ctx->elem != TSPGPU_ELEM_F64) {
        HIP_TRY(tmp.alloc((size_t)n * ld));
        if (ctx->elem == TSPGPU_ELEM_I32)
            hipLaunchKernelGGL((k_to_f64<int>), dim3((ld + 255) / 256, n), dim3(256), 0, ctx->stream, (const int *)ctx->d_mat.p, n, ld, tmp);
        else
            hipLaunchKernelGGL((k_to_f64<u16>), dim3((ld + 255) / 256, n), dim3(256), 0, ctx->stream, (const u16 *)ctx->d_mat.p, n, ld, tmp);
        src = tmp;
    }
    HIP_TRY(hipMemcpy2DAsync(host_out, (size_t)n * 8, src, (size_t)ld * 8, (size_t)n * 8, n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return E_OK;
}

int tspgpu_nn_tour(tspgpu_ctx *ctx, int start, int *path, double *cost)
{
    if (!ctx || !path || !cost) return fail(ctx, E_INVALID, "null argument");
    hipSetDevice(ctx->device);
    int rc = need_costs(ctx);
    if (rc) return rc;
    if (start < 0 || start >= ctx->n) return fail(ctx, E_UNAVAILABLE, "starting node not correct"); // heuristics.c:223-226
    if ((rc = ensure_tours(ctx, 1))) return rc;
    if ((rc = launch_nn(ctx, 0, &start, 1))) return rc;
    double nn_cost = 0;
    HIP_TRY(hipMemcpyAsync(&nn_cost, ctx->S.cost, 8, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = init_slots(ctx, 0, 1, -1))) return rc; // derives succ[]
    mark_slots(ctx, 0, 1, true);
    if ((rc = store_path(ctx, 0, path, nullptr, nullptr))) return rc;
    *cost = nn_cost; // the running sum of heuristics.c:276,281, not the node-order recompute
    return E_OK;
}

int tspgpu_tour_load(tspgpu_ctx *ctx, int slot, const int *path)
{
    if (!ctx || !path || slot < 0) return fail(ctx, E_INVALID, "bad argument");
    hipSetDevice(ctx->device);
    int rc = need_costs(ctx);
    if (rc) return rc;
    return load_path(ctx, slot, path, -1);
}

int tspgpu_tour_nn(tspgpu_ctx *ctx, int slot, int start)
{
    if (!ctx || slot < 0) return fail(ctx, E_INVALID, "bad argument");
    hipSetDevice(ctx->device);
    int rc = need_costs(ctx);
    if (rc) return rc;
    if ((rc = ensure_tours(ctx, slot + 1))) return rc;
    if ((rc = launch_nn(ctx, slot, &start, 1))) return rc;
    if ((rc = init_slots(ctx, slot, 1, -1))) return rc;
    mark_slots(ctx, slot, 1, true);
    return E_OK;
}

int tspgpu_tour_copy(tspgpu_ctx *ctx, int dst, int src)
{
    if (!ctx || dst < 0) return fail(ctx, E_INVALID, "bad slot");
    hipSetDevice(ctx->device);
    int rc = need_slot(ctx, src);
    if (rc) return rc;
    if ((rc = ensure_tours(ctx, dst + 1))) return rc;
    hipLaunchKernelGGL(k_copy_tour, dim3(std::max(1, ctx->n / 256)), dim3(256), 0, ctx->stream, ctx->S, ctx->n, dst, src);
    HIP_TRY(hipGetLastError());
    const bool src_all = ctx->look_all[src] != 0;
    mark_slots(ctx, dst, 1, true);
    if (!src_all) {                         // the awake sets travel with the tour (d_awake exists: something cleared the flag)
        const size_t bytes = 3 * (size_t)ctx->n;
        if (dst != src)
            HIP_TRY(hipMemcpyAsync(ctx->d_awake + dst * bytes, ctx->d_awake + src * bytes, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        ctx->look_all[dst] = 0;
    }
    return E_OK;
}

int tspgpu_tour_two_opt(tspgpu_ctx *ctx, int slot, long max_sweeps, double time_left_s, long *sweeps)
{
    if (!ctx) return E_INVALID;
    hipSetDevice(ctx->device);
    int rc = need_costs(ctx);
    if (rc) return rc;
    if ((rc = need_slot(ctx, slot))) return rc;
    wake_slots(ctx, slot, 1);
    hipLaunchKernelGGL(k_rearm, dim3(1), dim3(64), 0, ctx->stream, ctx->S, slot, 1, (int)std::min<long>(max_sweeps, INT_MAX));
    HIP_TRY(hipGetLastError());
    bool late = false;
    if ((rc = run_sweeps(ctx, slot, 1, false, -1, time_left_s, &late))) return rc;
    if (sweeps) {
        int ns = 0;   // on the engine's stream: it is non-blocking, a null-stream copy would not order after it
        HIP_TRY(hipMemcpyAsync(&ns, ctx->S.nsweeps + slot, 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        *sweeps = ns;
    }
    return late ? E_DEADLINE : E_OK;
}

int tspgpu_tour_store(tspgpu_ctx *ctx, int slot, int *path, double *cost, double *last_delta)
{
    if (!ctx) return E_INVALID;
    hipSetDevice(ctx->device);
    int rc = need_slot(ctx, slot);
    if (rc) return rc;
    return store_path(ctx, slot, path, cost, last_delta);
}

int tspgpu_two_opt_once(tspgpu_ctx *ctx, int *path, double *cost, double *delta)
{
    if (!ctx || !path || !cost) return fail(ctx, E_INVALID, "null argument");
    hipSetDevice(ctx->device);
    int rc = need_costs(ctx);
    if (rc) return rc;
    if ((rc = load_path(ctx, 0, path, 1))) return rc;
    // ref_2opt_once trusts the caller's running cost (refinment.c:83): keep it
    HIP_TRY(hipMemcpyAsync(ctx->S.cost, cost, 8, hipMemcpyHostToDevice, ctx->stream));
    const int save_graph = ctx->opt_graph;
    ctx->opt_graph = 0;
    rc = run_sweeps(ctx, 0, 1, false, 1, -1, nullptr);
    ctx->opt_graph = save_graph;
    if (rc) return rc;
    double d = 0;
    if ((rc = store_path(ctx, 0, path, cost, &d))) return rc;
    if (delta) *delta = d;
    return E_OK;
}

int tspgpu_two_opt(tspgpu_ctx *ctx, int *path, double *cost, double time_left_s, long *sweeps)
{
    if (!ctx || !path || !cost) return fail(ctx, E_INVALID, "null argument");
    hipSetDevice(ctx->device);
    int rc = need_costs(ctx);
    if (rc) return rc;
    if ((rc = load_path(ctx, 0, path, -1))) return rc;
    bool late = false;
    if ((rc = run_sweeps(ctx, 0, 1, false, -1, time_left_s, &late))) return rc;
    // (the sweep count rides on store_path's synchronisation: pinned word, engine's stream)
    if (sweeps) HIP_TRY(hipMemcpyAsync(ctx->h_status, ctx->S.nsweeps, 4, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = store_path(ctx, 0, path, cost, nullptr))) return rc;
    if (sweeps) *sweeps = ctx->h_status[0];
    return late ? E_DEADLINE : E_OK;
}

static int tabu_prepare(tspgpu_ctx *ctx, const int *tabu_list, int tenure, int iter, int t_min, int t_max, int up,
                        int resident, double best_cost)
{
    TabuState ts;
    ts.iter = iter; ts.tenure = tenure; ts.t_min = t_min; ts.t_max = t_max; ts.up = up; ts.resident = resident;
    ts.best_cost = best_cost;
    HIP_TRY(hipMemcpyAsync(ctx->d_tabu, &ts, sizeof ts, hipMemcpyHostToDevice, ctx->stream));
    if (tabu_list) HIP_TRY(hipMemcpyAsync(ctx->d_tabu_list, tabu_list, (size_t)ctx->n * 4, hipMemcpyHostToDevice, ctx->stream));
    else HIP_TRY(hipMemsetAsync(ctx->d_tabu_list, 0xff, (size_t)ctx->n * 4, ctx->stream)); // all -1
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return E_OK;
}

int tspgpu_tabu_move(tspgpu_ctx *ctx, int *path, double *cost, int *tabu_list, int tenure, int iter)
{
    if (!ctx || !path || !cost || !tabu_list) return fail(ctx, E_INVALID, "null argument");
    hipSetDevice(ctx->device);
    int rc = need_costs(ctx);
    if (rc) return rc;
    if ((rc = load_path(ctx, 0, path, 1))) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->S.cost, cost, 8, hipMemcpyHostToDevice, ctx->stream)); // running cost, metaheuristic.c:233
    if ((rc = tabu_prepare(ctx, tabu_list, tenure, iter, INT_MIN, INT_MAX, 1, 0, 0.0))) return rc;
    const int save_graph = ctx->opt_graph;
    ctx->opt_graph = 0;
    rc = run_sweeps(ctx, 0, 1, true, 1, -1, nullptr);
    ctx->opt_graph = save_graph;
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(tabu_list, ctx->d_tabu_list, (size_t)ctx->n * 4, hipMemcpyDeviceToHost, ctx->stream));
    return store_path(ctx, 0, path, cost, nullptr);
}

int tspgpu_tabu_search(tspgpu_ctx *ctx, int *path, double *cost, int k, int *best_path, double *best_cost, double *trace)
{
    if (!ctx || !path || !cost || !best_path || !best_cost || k < 0) return fail(ctx, E_INVALID, "bad argument");
    hipSetDevice(ctx->device);
    int rc = need_costs(ctx);
    if (rc) return rc;
    const int n = ctx->n;
    if ((rc = load_path(ctx, 0, path, k))) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->S.cost, cost, 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->d_best_succ, path, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = reserve_captured(ctx, ctx->d_trace, (size_t)k))) return rc;
    // tabu_init (metaheuristic.c:65-84) then the first policy step (:126-143 -> :40-59)
    int tenure = (int)(0.125 * n + 1), t_max = (int)(0.25 * n), t_min = (int)(0.125 * n), up = 1;
    if (tenure == t_max || tenure == t_min) up = !up;
    tenure += up ? 1 : -1;
    if ((rc = tabu_prepare(ctx, nullptr, tenure, 0, t_min, t_max, up, 1, *cost))) return rc;
    bool ran = false;
    ctx->lp_used = false;
    if (k > 0 && ctx->symmetric && resident_wanted(ctx)) {
        // the whole walk in one launch, matrix and ages in LDS (k_lds2opt<., true>) where it applies
        const PersistTabu pt = {k, tenure, t_min, t_max, up, *cost};
        if ((rc = run_persist(ctx, 0, nullptr, nullptr, &ran, &pt))) return rc;
        if (!ran && ctx->opt_persist == 2) return fail(ctx, E_EXHAUSTED, "the LDS-resident tabu walk does not apply (uint16 cells, n in [64, ~5400], one idle chip)");
    }
    if (k > 0 && !ran && (rc = run_sweeps(ctx, 0, 1, true, k, -1, nullptr))) return rc;
    if (trace && k > 0) HIP_TRY(hipMemcpyAsync(trace, ctx->d_trace, (size_t)k * 8, hipMemcpyDeviceToHost, ctx->stream));
    TabuState ts;
    HIP_TRY(hipMemcpyAsync(&ts, ctx->d_tabu, sizeof ts, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(best_path, ctx->d_best_succ, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = store_path(ctx, 0, path, cost, nullptr))) return rc;
    *best_cost = ts.best_cost;
    return E_OK;
}

// host side of vns_kick (metaheuristic.c:344-409, :490-500) for the non-resident path of tspgpu_vns_search: the same
// draws, the same rejection rule, the same unwrapped probes as tspgpu_lds_vns.inc
static bool vns_kick_host(std::vector<int> &succ, std::vector<int> &tour, const int *rv, long nrand, long &cur)
{
    const int n = (int)succ.size();
    for (int p = 0, v = 0; p < n; p++, v = succ[v]) tour[p] = v;
    auto at = [&](int p) { return p < 0 ? 0 : p >= n ? ((n & 3) == 2 ? -2 : 0) : tour[p]; };
    int pick[3];
    for (int i = 0; i < 3; i++) {
        int r = -1;
        while (r < 0) {
            if (cur >= nrand) return false;
            r = (int)((unsigned)rv[cur++] % (unsigned)n);
            for (int j = 0; j < i; j++)
                if (r == pick[j] || r == at(pick[j] - 1) || r == at(pick[j] + 1)) { r = -1; break; }
        }
        pick[i] = r;
        for (int j = i; j > 0 && pick[j] < pick[j - 1]; j--) std::swap(pick[j], pick[j - 1]);
    }
    const int a = tour[pick[0]], sa = tour[(pick[0] + 1) % n], b = tour[pick[1]], sb = tour[(pick[1] + 1) % n],
              c = tour[pick[2]], sc = tour[(pick[2] + 1) % n];
    succ[a] = sb; succ[c] = sa; succ[b] = sc;
    return true;
}

int tspgpu_vns_search(tspgpu_ctx *ctx, int *path, double *cost, int k, double time_left_s, const int *rand_values, long nrand,
                      long *consumed, int *iterations, int *kick_pending, int *best_path, double *best_cost, double *trace)
{
    if (!ctx || !path || !cost || !best_path || !best_cost || !iterations || !kick_pending || !consumed || k < 0 || nrand < 0 ||
        (nrand > 0 && !rand_values) || *iterations < 0 || *iterations > k)
        return fail(ctx, E_INVALID, "bad argument");
    hipSetDevice(ctx->device);
    int rc = need_costs(ctx);
    if (rc) return rc;
    const int n = ctx->n;
    *consumed = 0;
    if (*iterations >= k) return E_OK;
    const double t_end = deadline_of(time_left_s);
    if ((rc = load_path(ctx, 0, path, -1))) return rc;              // (recomputes the cost: refinment.c:6-9)
    bool resident_done = false;
    ctx->lp_used = false;
    PersistVns pv = {k, *iterations, *kick_pending ? 1 : 0, rand_values, nrand, 0, *best_cost, trace, false, *iterations};
    bool late = false;
    if (ctx->symmetric && resident_wanted(ctx)) {
        HIP_TRY(hipMemcpyAsync(ctx->d_best_succ, best_path, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
        double left = t_end >= 0 ? std::max(0.0, t_end - now_s()) : -1.0;
        bool ran = false;
        ctx->lp_handed = false;
        if ((rc = run_persist(ctx, 0, &left, &late, &ran, nullptr, &pv))) return rc;
        resident_done = ran;
        if (!ran && ctx->opt_persist == 2) return fail(ctx, E_EXHAUSTED, "the LDS-resident VNS loop does not apply (uint16 cells, n in [64, ~5400], one idle chip)");
        // the incumbent as far as the resident launches got (all of the walk; or, when the grid lost its co-residency half
        // way, up to the last launch that completed: the slot then holds that launch's tour and the loop below goes on from it)
        HIP_TRY(hipMemcpyAsync(best_path, ctx->d_best_succ, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (!ran && (rc = store_path(ctx, 0, path, cost, nullptr))) return rc;
    }
    ctx->vns_mode = resident_done ? 1 : pv.it > pv.it_entry ? 3 : 2;
    if (!resident_done) {
        // one local search per iteration on the device (whatever kernels the instance takes), kicks on the host
        std::vector<int> succ(path, path + n), tour(n), before(n);
        long cur = pv.used;                        // (numbers the resident launches consumed before the grid was lost)
        while (pv.it < k) {
            if (t_end >= 0 && now_s() >= t_end) { late = true; break; }
            if (!pv.phase) {
                if ((rc = load_path(ctx, 0, succ.data(), -1))) return rc;
                bool l2 = false;
                if ((rc = run_sweeps(ctx, 0, 1, false, -1, t_end >= 0 ? std::max(0.0, t_end - now_s()) : -1.0, &l2))) return rc;
                double c = 0;
                if ((rc = store_path(ctx, 0, succ.data(), &c, nullptr))) return rc;
                if (c < pv.best) { pv.best = c; memcpy(best_path, succ.data(), (size_t)n * 4); }
                if (trace) trace[pv.it - pv.it_entry] = c;
                *cost = c;
            }
            const long cur0 = cur;
            before = succ;
            bool dry = cur >= nrand;
            if (!dry) {
                const int kicks = rand_values[cur++] % 9 - 2;
                for (int j = 0; j < kicks && !dry; j++) dry = !vns_kick_host(succ, tour, rand_values, nrand, cur);
            }
            if (dry) { succ = before; cur = cur0; pv.phase = 1; pv.need_rand = true; break; }
            pv.phase = 0; pv.it++;
        }
        pv.used = cur;
        memcpy(path, succ.data(), (size_t)n * 4);
    } else {
        if ((rc = store_path(ctx, 0, path, cost, nullptr))) return rc;
    }
    *iterations = pv.it; *kick_pending = pv.phase; *consumed = pv.used; *best_cost = pv.best;
    if (pv.need_rand) return fail(ctx, E_EXHAUSTED, "the random numbers ran out in front of the kicks of iteration %d: call again with more", pv.it);
    return late ? E_DEADLINE : E_OK;
}

int tspgpu_nn_all_timed(tspgpu_ctx *ctx, const int *starts, int nstarts, double time_left_s, int *best_path, double *best_cost,
                        int *best_start, int *done_starts)
{
    if (!ctx || !best_path || !best_cost || !best_start || nstarts <= 0) return fail(ctx, E_INVALID, "bad argument");
    hipSetDevice(ctx->device);
    int rc = need_costs(ctx);
    if (rc) return rc;
    const double t0 = now_s();
    const double t_end = time_left_s >= 0 ? t0 + time_left_s : -1;
    // NN tours in flight: one wave per start, and a step is a dependent chain of ~1.3 us whatever else runs -- the chip takes
    // 13-16 waves per CU (the visited bits of a tour in LDS) where the multi-start default of 1024 tours leaves 4: 4096 starts
    // per launch while the slots stay below 12 GB and the caller has not set TSPGPU_OPT_MAX_TOURS itself
    // (pla85900 All-NN, 85 900 tours: 10.5 -> 6.0 s)
    int want = ctx->opt_max_tours;
    if (want == 1024 && (size_t)4096 * 28 * (size_t)ctx->n <= ((size_t)12 << 30)) want = 4096;
    const int cap = std::min(nstarts, want);
    if ((rc = ensure_tours(ctx, cap))) return rc;
    double best = DBL_MAX; int arg = -1;
    std::vector<int> hs(cap);
    // under a deadline: first one start per CU, then batches of about a quarter of the time left
    // (at most ~0.5 s) at the rate measured so far; the reference checks before every start
    int chunk = t_end >= 0 ? std::min(cap, std::max(1, ctx->cus)) : cap;
    int base = 0;
    bool late = false;
    while (base < nstarts) {
        if (t_end >= 0 && now_s() >= t_end) { late = true; break; }
        const int m = std::min(chunk, nstarts - base);
        for (int i = 0; i < m; i++) hs[i] = starts ? starts[base + i] : base + i;
        if ((rc = launch_nn(ctx, 0, hs.data(), m))) return rc;
        HIP_TRY(hipMemcpyAsync(ctx->h_costs, ctx->S.cost, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        int win = -1;
        for (int i = 0; i < m; i++) if (ctx->h_costs[i] < best) { best = ctx->h_costs[i]; win = i; } // strict <, heuristics.c:58
        if (win >= 0) {
            arg = hs[win];
            if ((rc = init_slots(ctx, win, 1, -1))) return rc;
            mark_slots(ctx, win, 1, true);
            if ((rc = store_path(ctx, win, best_path, nullptr, nullptr))) return rc;
        }
        base += m;
        if (t_end >= 0) {
            const double now = now_s(), rate = base / std::max(now - t0, 1e-6);     // starts per second
            const double budget = std::min(0.5, std::max(0.0, t_end - now) / 4);
            chunk = (int)std::min<double>(cap, std::max<double>(std::min(cap, ctx->cus), rate * budget));
        }
    }
    *best_cost = best; *best_start = arg;
    if (done_starts) *done_starts = base;
    return late ? E_DEADLINE : E_OK;
}

int tspgpu_nn_all(tspgpu_ctx *ctx, const int *starts, int nstarts, int *best_path, double *best_cost, int *best_start)
{
    return tspgpu_nn_all_timed(ctx, starts, nstarts, -1.0, best_path, best_cost, best_start, nullptr);
}

int tspgpu_multistart_nn_2opt(tspgpu_ctx *ctx, const int *starts, int nstarts, double time_left_s, int *best_path,
                              double *best_cost, int *best_start, long *total_sweeps, int *last_path, double *last_cost)
{
    if (!ctx || !best_path || !best_cost || !best_start || nstarts <= 0) return fail(ctx, E_INVALID, "bad argument");
    hipSetDevice(ctx->device);
    int rc = need_costs(ctx);
    if (rc) return rc;
    // a chunk's sweep counts ride on the loop's cost readback: copied into the sweep-count half of the pinned status words (the
    // next chunk's NN launch may reuse the first half), added up in front of the next chunk's descent and behind the last one
    long sweeps = 0;
    int pending = 0;
    auto add_pending = [&] { for (int i = 0; i < pending; i++) sweeps += ctx->h_status[ctx->tcap + i]; pending = 0; };
    MultiStart ms;
    rc = multistart(ctx, starts, nstarts, time_left_s, ctx->opt_sweep_cap, best_path, best_cost, best_start, nullptr, &ms,
                    [&](int m, double left, bool *late, Descent *) {
                        add_pending();
                        const int e = run_sweeps(ctx, 0, m, false, -1, left, late);
                        if (e) return e;
                        HIP_TRY(hipMemcpyAsync(ctx->h_status + ctx->tcap, ctx->S.nsweeps, (size_t)m * 4, hipMemcpyDeviceToHost, ctx->stream));
                        pending = m;
                        return (int)E_OK;
                    });
    if (rc && rc != E_DEADLINE) return rc;
    add_pending();
    // what h_Greedy_2opt_mod_costs leaves in *solution: the tour of the last start it processed -- the last
    // one of the list, or of the chunk in which the deadline struck (always a valid tour, heuristics.c:118-149)
    if (last_path) {
        const int e = store_path(ctx, ms.m_last - 1, last_path, last_cost, nullptr);
        if (e) return e;
    }
    if (total_sweeps) *total_sweeps = sweeps;
    return rc;
}

int tspgpu_tour_sweep_part(tspgpu_ctx *ctx, int slot, int part, int nparts, double *delta, int *a, int *b)
{
    if (!ctx || !delta || !a || !b || nparts <= 0 || part < 0 || part >= nparts)
        return fail(ctx, E_INVALID, "bad argument");
    hipSetDevice(ctx->device);
    int rc = need_costs(ctx);
    if (rc) return rc;
    if ((rc = need_slot(ctx, slot))) return rc;
    if (!ctx->symmetric) return fail(ctx, E_PRECOND, "a sharded sweep needs a symmetric matrix (both orientations of a pair live in different parts otherwise)");
    if ((rc = ensure_plan(ctx, 1, false))) return rc;
    const int G = ctx->plan.G;
    const int g_lo = (int)((long)part * G / nparts), g_hi = (int)((long)(part + 1) * G / nparts);
    *delta = 0.0; *a = 0; *b = 0;
    if (g_hi <= g_lo) return E_OK;
    hipLaunchKernelGGL(k_reopen, dim3(1), dim3(1), 0, ctx->stream, ctx->S, slot);     // (a finished slot's sweep would leave its partials as they were)
    if ((rc = launch_sweep(ctx, slot, 1, false, g_lo, g_hi - g_lo))) return rc;
    std::vector<Partial> h((size_t)(g_hi - g_lo));
    HIP_TRY(hipMemcpyAsync(h.data(), ctx->S.partial + (size_t)slot * ctx->S.pstride + g_lo, h.size() * sizeof(Partial),
                           hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    double d = 0.0;
    u64 key = 0;
    for (const Partial &q : h)
        if (q.d < d || (q.d == d && q.key < key)) { d = q.d; key = q.key; }     // (delta, a, b): the reference's order
    if (d < TWO_OPT_EPS) { *delta = d; *a = (int)(key >> 32); *b = (int)(key & 0xffffffffu); }
    return E_OK;
}

int tspgpu_tour_apply_move(tspgpu_ctx *ctx, int slot, int a, int b, double delta)
{
    if (!ctx) return E_INVALID;
    const int n = ctx->n;
    if (a < 0 || b < 0 || a >= n || b >= n) return fail(ctx, E_INVALID, "move (%d,%d) outside [0,%d)", a, b, n);
    hipSetDevice(ctx->device);
    int rc = need_costs(ctx);
    if (rc) return rc;
    if ((rc = need_slot(ctx, slot))) return rc;
    wake_slots(ctx, slot, 1);
    if ((rc = ensure_plan(ctx, 1, false))) return rc;
    const int G = ctx->plan.G;
    const u64 key = delta < TWO_OPT_EPS ? (a < b ? ((u64)(unsigned)a << 32) | (unsigned)b : ((u64)(unsigned)b << 32) | (unsigned)a) : 0;
    hipLaunchKernelGGL(k_reopen, dim3(1), dim3(1), 0, ctx->stream, ctx->S, slot);     // (k_apply leaves a finished slot alone)
    hipLaunchKernelGGL(k_set_move, dim3((G + 255) / 256), dim3(256), 0, ctx->stream, ctx->S, slot, G, delta < TWO_OPT_EPS ? delta : 0.0, key);
    HIP_TRY(hipGetLastError());
    if ((rc = launch_apply(ctx, slot, 1, false, false))) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return E_OK;
}

int tspgpu_time_sweep(tspgpu_ctx *ctx, int slot, int reps, float *ms_mean)
{
    if (!ctx || !ms_mean || reps <= 0) return fail(ctx, E_INVALID, "bad argument");
    hipSetDevice(ctx->device);
    int rc = need_costs(ctx);
    if (rc) return rc;
    if ((rc = need_slot(ctx, slot))) return rc;
    if ((rc = ensure_plan(ctx, 1, false))) return rc;
    hipLaunchKernelGGL(k_rearm, dim3(1), dim3(64), 0, ctx->stream, ctx->S, slot, 1, -1);
    auto sweep = [&] { return launch_sweep(ctx, slot, 1, false); };
    return time_launches(ctx, reps, sweep, sweep, ms_mean);
}

int tspgpu_time_build(tspgpu_ctx *ctx, int reps, float *ms_mean)
{
    if (!ctx || !ms_mean || reps <= 0) return fail(ctx, E_INVALID, "bad argument");
    hipSetDevice(ctx->device);
    int rc = need_costs(ctx);
    if (rc) return rc;
    if (!ctx->have_points) return fail(ctx, E_PRECOND, "no points");
    if (ctx->otf) { *ms_mean = 0; return E_OK; }
    auto build = [&] { return launch_build(ctx); };
    return time_launches(ctx, reps, build, build, ms_mean);
}

int tspgpu_timing_read(tspgpu_ctx *ctx, double *sweep_ms_total, long *sweep_launches, int reset)
{
    if (!ctx) return E_INVALID;
    if (sweep_ms_total) *sweep_ms_total = ctx->sweep_ms_total;
    if (sweep_launches) *sweep_launches = ctx->sweep_launches;
    if (reset) { ctx->sweep_ms_total = 0; ctx->sweep_launches = 0; }
    return E_OK;
}

int tspgpu_debug_stamps(tspgpu_ctx *ctx, unsigned long long *out, int capacity_words)
{
    if (!ctx || !out || !ctx->d_stamps) return fail(ctx, E_PRECOND, "stamps not enabled");
    hipSetDevice(ctx->device);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const size_t words = std::min<size_t>((size_t)capacity_words, (size_t)MAX_WGS_PER_TOUR * 64);
    HIP_TRY(hipMemcpy(out, ctx->d_stamps, words * 8, hipMemcpyDeviceToHost));
    return E_OK;
}

int tspgpu_debug_tmat(tspgpu_ctx *ctx, unsigned short *out, size_t cells)
{
    if (!ctx || !out) return fail(ctx, E_INVALID, "null argument");
    if (!ctx->d_lp_tmat) return fail(ctx, E_PRECOND, "no tour-ordered copy was kept");
    hipSetDevice(ctx->device);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(out, ctx->d_lp_tmat, std::min(cells, ctx->d_lp_tmat.n) * sizeof(u16), hipMemcpyDeviceToHost));
    return E_OK;
}

int tspgpu_history(tspgpu_ctx *ctx, int *a, int *b, double *delta, int capacity, int *count)
{
    if (!ctx || !count) return fail(ctx, E_INVALID, "null argument");
    hipSetDevice(ctx->device);
    int ns = 0;
    if (ctx->tcap > 0) {
        HIP_TRY(hipMemcpyAsync(&ns, ctx->S.nsweeps, 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    int m = std::min(std::min(ns, ctx->hist.cap), capacity);
    if (m > 0) {
        if (a) HIP_TRY(hipMemcpyAsync(a, ctx->hist.a, (size_t)m * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (b) HIP_TRY(hipMemcpyAsync(b, ctx->hist.b, (size_t)m * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (delta) HIP_TRY(hipMemcpyAsync(delta, ctx->hist.d, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    *count = m;
    return E_OK;
}

} // extern "C"

// ---- Extra Mileage (tspgpu_em.inc) -----------------------------------------------------------------------------------

// run `...` with WF bound to the weight functor of the context's matrix / matrix-free kind
#define EM_WF_SWITCH(ctx, WF, ...)                                                                        \
    do {                                                                                                  \
        if ((ctx)->otf) {                                                                                 \
            if ((ctx)->kind == TSPGPU_EUC_2D) { typedef EmPts<TSPGPU_EUC_2D> WF; __VA_ARGS__; }          \
            else if ((ctx)->kind == TSPGPU_ATT) { typedef EmPts<TSPGPU_ATT> WF; __VA_ARGS__; }           \
            else { typedef EmPts<TSPGPU_CEIL_2D> WF; __VA_ARGS__; }                                       \
        } else if ((ctx)->elem == TSPGPU_ELEM_F64) { typedef EmMat<double> WF; __VA_ARGS__; }             \
        else if ((ctx)->elem == TSPGPU_ELEM_I32) { typedef EmMat<int> WF; __VA_ARGS__; }                  \
        else { typedef EmMat<u16> WF; __VA_ARGS__; }                                                      \
    } while (0)

// the held weights are integers in [0, 2^27) off the diagonal (every delta and key then is an exact integer)
static int em_check(tspgpu_ctx *ctx)
{
    int rc = need_costs(ctx);
    if (rc) return rc;
    if (ctx->built) {
        if (!(ctx->cost_bound < 134217728.0)) return fail(ctx, E_PRECOND, "Extra Mileage needs integer costs below 2^27 (bound %.0f)", ctx->cost_bound);
        return E_OK;
    }
    const int n = ctx->n, ld = ctx->ld;
    HIP_TRY(hipMemsetAsync(ctx->d_flags, 0, 4, ctx->stream));
    const dim3 grid((n + 255) / 256, n);
    if (ctx->elem == TSPGPU_ELEM_F64) hipLaunchKernelGGL((k_em_check<double>), grid, dim3(256), 0, ctx->stream, (const double *)ctx->d_mat.p, n, ld, ctx->d_flags);
    else if (ctx->elem == TSPGPU_ELEM_I32) hipLaunchKernelGGL((k_em_check<int>), grid, dim3(256), 0, ctx->stream, (const int *)ctx->d_mat.p, n, ld, ctx->d_flags);
    else hipLaunchKernelGGL((k_em_check<u16>), grid, dim3(256), 0, ctx->stream, (const u16 *)ctx->d_mat.p, n, ld, ctx->d_flags);
    HIP_TRY(hipGetLastError());
    int flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, ctx->d_flags, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (flag) return fail(ctx, E_PRECOND, "Extra Mileage needs every off-diagonal cost an integer in [0, 2^27)");
    return E_OK;
}

static EmArgs em_args(const tspgpu_ctx *ctx)
{
    EmArgs A;
    memset(&A, 0, sizeof A);
    A.mat = ctx->d_mat; A.pts = ctx->d_pts; A.ld = ctx->ld; A.n = ctx->n; A.sym = ctx->symmetric;
    return A;
}

extern "C" {

int tspgpu_farthest_pair(tspgpu_ctx *ctx, int *a, int *b, double *cost)
{
    if (!ctx || !a || !b || !cost) return fail(ctx, E_INVALID, "null argument");
    hipSetDevice(ctx->device);
    int rc = em_check(ctx);
    if (rc) return rc;
    DevBuf<u64> d_key;
    u64 key = 0;
    HIP_TRY(d_key.alloc(1));
    EmArgs A = em_args(ctx);
    HIP_TRY(hipMemsetAsync(d_key, 0, 8, ctx->stream));
    EM_WF_SWITCH(ctx, WF, hipLaunchKernelGGL((k_em_farthest<WF>), dim3(ctx->n), dim3(EM_BT), 0, ctx->stream, A, d_key.p));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&key, d_key, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const u64 lin = ~key & EM_FMASK, n = (u64)ctx->n;
    *a = (int)(lin / n); *b = (int)(lin % n);
    *cost = (double)(key >> 35);
    return E_OK;
}

int tspgpu_extra_mileage(tspgpu_ctx *ctx, int a, int b, double time_left_s, int *path, double *cost)
{
    if (!ctx || !path || !cost) return fail(ctx, E_INVALID, "null argument");
    hipSetDevice(ctx->device);
    int rc = em_check(ctx);
    if (rc) return rc;
    const int n = ctx->n;
    if (a < 0 || a >= n || b < 0 || b >= n || a == b) return fail(ctx, E_INVALID, "starting pair (%d, %d) is not two distinct nodes of [0, %d)", a, b, n);
    if (time_left_s >= 0 && time_left_s <= 0) return fail(ctx, E_DEADLINE, "time limit exceeded before the first insertion");
    // one allocation: control block | skey[n] | eu, ev, ec, succ [n] | stale [3][n]
    const size_t N = (size_t)n, bytes = sizeof(EmCtl) + N * 8 + N * 4 * 4 + N * 4 * 3;
    DevBuf<unsigned char> mem;
    HIP_TRY(mem.alloc(bytes));
    EmArgs A = em_args(ctx);
    A.ctl = reinterpret_cast<EmCtl *>(mem.p);
    A.skey = reinterpret_cast<u64 *>(mem + sizeof(EmCtl));
    A.eu = reinterpret_cast<int *>(mem + sizeof(EmCtl) + N * 8);
    A.ev = A.eu + N; A.ec = A.ev + N; A.succ = A.ec + N; A.stale = A.succ + N;
    A.limit = time_left_s < 0 ? -1 : (long long)(time_left_s * 1e8);
    A.hello = ctx->opt_lp_hello;            // 2 ms
    A.spin = 100000000;                     // 1 s
    const int W = ctx->cus;
    EmCtl C;
    memset(&C, 0, sizeof C);
    auto run = [&](bool resident) -> int {
        HIP_TRY(hipMemsetAsync(A.ctl, 0, sizeof(EmCtl), ctx->stream));
        if (resident) {
            EM_WF_SWITCH(ctx, WF, hipLaunchKernelGGL((k_em_resident<WF>), dim3(W), dim3(EM_BT), 0, ctx->stream, A, a, b));
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&C, A.ctl, sizeof C, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            return E_OK;
        }
        EM_WF_SWITCH(ctx, WF, hipLaunchKernelGGL((k_em_init<WF>), dim3(W), dim3(EM_BT), 0, ctx->stream, A, a, b));
        HIP_TRY(hipGetLastError());
        // every step's two launches back to back; the host looks at the stop word once per chunk of steps
        for (int s0 = 0; s0 <= n - 3; s0 += 2048) {
            for (int s = s0; s <= n - 3 && s < s0 + 2048; s++) {
                EM_WF_SWITCH(ctx, WF, hipLaunchKernelGGL((k_em_a<WF>), dim3(W), dim3(EM_BT), 0, ctx->stream, A, s));
                if (s < n - 3) EM_WF_SWITCH(ctx, WF, hipLaunchKernelGGL((k_em_b<WF>), dim3(W), dim3(EM_BT), 0, ctx->stream, A, s));
            }
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&C, A.ctl, sizeof C, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            if (C.stop) break;
        }
        return E_OK;
    };
    const int form = ctx->opt_em_form == 1 ? 1 : 2;    // (measured: the per-step form is faster)
    rc = run(form == 1);
    if (!rc && C.status == EM_ST_BROKEN) rc = fail(ctx, E_INTERNAL, "Extra Mileage: a step found no candidate (after %d insertions)", C.steps);
    if (!rc && C.status != EM_ST_OK)
        rc = fail(ctx, E_EXHAUSTED, "Extra Mileage: the resident grid of %d workgroups %s", W,
                  C.status == EM_ST_NO_RENDEZVOUS ? "did not come up co-resident" : "lost its co-residency");
    if (!rc) {
        ctx->em_form = form; ctx->em_stale = C.stale; ctx->em_steps = C.steps;
        if (C.stop) rc = fail(ctx, E_DEADLINE, "time limit exceeded after %d of %d insertions", C.steps, n - 2);
        else if (C.steps != n - 2) rc = fail(ctx, E_INTERNAL, "Extra Mileage ended after %d of %d insertions", C.steps, n - 2);
        else {
            HIP_TRY(hipMemcpyAsync(path, A.succ, N * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            *cost = 2.0 * (double)C.cab + (double)C.dsum;     // heuristics.c:184 then :362, exact in integers
        }
    }
    return rc;
}

} // extern "C"

// ---- Or-opt and the 2-opt + Or-opt descent (tspgpu_oropt.inc) -------------------------------------------------------

// largest n the Or-opt sweep takes with cells of `esz` bytes: four rows of ld cells and OR_EXTRA bytes in one workgroup's LDS
static int or_max_n(const tspgpu_ctx *ctx, size_t esz) { return (int)((ctx->lds_max - OR_EXTRA) / (4 * esz)) & ~31; }

// batch: the entry points over several slots, which matrix-free mode refuses whatever TSPGPU_OPT_OR_MATRIX_FREE says
static int or_check(tspgpu_ctx *ctx, bool batch)
{
    int rc = need_costs(ctx);
    if (rc) return rc;
    if (ctx->otf && (batch || !ctx->opt_or_otf))
        return fail(ctx, E_UNIMPL, "Or-opt needs the resident cost matrix: it is not implemented in matrix-free mode");
    if (ctx->n < 8) return fail(ctx, E_INVALID, "Or-opt needs at least 8 nodes, got %d", ctx->n);
    if (ctx->otf) {     // from the points: symmetric by construction, costs below 2^27, n <= 131 072 (new_instance), no row in LDS
        if ((rc = ensure_spts(ctx, (size_t)ctx->n))) return rc;     // sized as make_plan sizes them for one tour
    } else {
        if (!ctx->symmetric) return fail(ctx, E_PRECOND, "Or-opt needs a symmetric cost matrix");
        const int lim = or_max_n(ctx, elem_size(ctx->elem));
        if (ctx->ld > lim)
            return fail(ctx, E_EXHAUSTED, "Or-opt keeps four matrix rows in LDS: n = %d is past the limit of %d nodes for %d-byte cells",
                        ctx->n, lim, (int)elem_size(ctx->elem));
    }
    HIP_TRY(ctx->d_or.reserve(1));
    return E_OK;
}

static int or_check(tspgpu_ctx *ctx) { return or_check(ctx, false); }

template <typename T> static const void *or_sweep_fn(int nch)
{
    return nch == 1 ? (const void *)k_oropt_sweep<T, 1> : nch == 2 ? (const void *)k_oropt_sweep<T, 2> : (const void *)k_oropt_sweep<T, 3>;
}

// the form of a matrix-free Or-opt sweep (hook 90).  Automatic is the full form: the early-out form is chosen only where
// tools/oropt_otf_rate.py has measured it faster, and no such measurement is recorded yet
static bool or_otf_early(const tspgpu_ctx *ctx) { return ctx->opt_or_otf_early == 1; }

// four rows in LDS, at most three vectors per thread and row below every LDS limit, R at least 2 and the partial slots of a tour
static SweepGeom or_plan(const tspgpu_ctx *ctx)
{
    const int rmin = std::max(2, (ctx->n + MAX_WGS_PER_TOUR - 1) / MAX_WGS_PER_TOUR);
    SweepGeom P = plan::sweep_geom(plan_in(ctx), 4, OR_EXTRA, rmin, OR_RMAX, {1, 2, 3}, OR_OTF_RUN);
    if (!ctx->otf) ELEM_SWITCH(ctx->elem, T, P.fn = or_sweep_fn<T>(P.NCH));
    return P;
}

static int or_single_R(const tspgpu_ctx *ctx) { return ctx->have_costs && !ctx->otf && ctx->n >= 8 ? or_plan(ctx).R : 0; }
// threads per sweep workgroup, or -- nch -- 16-byte vectors per thread and row, of the same plan (0 where or_single_R is 0)
static int or_single_geom(const tspgpu_ctx *ctx, bool nch)
{
    if (!or_single_R(ctx)) return 0;
    const SweepGeom P = or_plan(ctx);
    return nch ? P.NCH : P.BT;
}

// spts := the points of the successors in `slot`, unless *stop (a control block's, on the device) says the descent is over
static int launch_spts_gather(tspgpu_ctx *ctx, int slot, const int *stop)
{
    const int n = ctx->n;
    kind_switch(ctx, [&](auto kind, auto *pts, auto *spts) {
        hipLaunchKernelGGL((k_spts_gather<typename OrPt<kind()>::type>), dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->S, n, slot,
                           pts, spts, stop);
    });
    HIP_TRY(hipGetLastError());
    return E_OK;
}

// matrix-free mode: the gather of the successors' points (it must see the tour the previous apply left), then the sweep
static int or_launch_sweep_otf(tspgpu_ctx *ctx, int slot, const SweepGeom &P, bool gather)
{
    const int n = ctx->n;
    const bool early = or_otf_early(ctx);
    const OrCtl *ctl = ctx->d_or;
    if (gather) {
        const int rc = launch_spts_gather(ctx, slot, &ctl->stop);
        if (rc) return rc;
    }
    kind_switch(ctx, [&](auto kind, auto *pts, auto *spts) {
        if (early) hipLaunchKernelGGL((k_oropt_sweep_otf<kind(), true>), dim3(P.W), dim3(P.BT), 0, ctx->stream, ctx->S, pts, spts, n, slot, ctl);
        else hipLaunchKernelGGL((k_oropt_sweep_otf<kind(), false>), dim3(P.W), dim3(P.BT), 0, ctx->stream, ctx->S, pts, spts, n, slot, ctl);
    });
    HIP_TRY(hipGetLastError());
    ctx->or_otf_form = early ? 2 : 1;
    ctx->or_otf_R = P.R;
    return E_OK;
}

static int or_launch_sweep(tspgpu_ctx *ctx, int slot, const SweepGeom &P, bool gather = true)
{
    if (ctx->otf) return or_launch_sweep_otf(ctx, slot, P, gather);
    const int rc = ensure_max_lds(ctx, P.fn);
    if (rc) return rc;
#define OR_SWEEP(T, N) hipLaunchKernelGGL((k_oropt_sweep<T, N>), dim3(P.W), dim3(P.BT), P.lds, ctx->stream, ctx->S, (const T *)ctx->d_mat.p, \
                                          ctx->n, ctx->ld, slot, P.R, (const OrCtl *)ctx->d_or)
    ELEM_SWITCH(ctx->elem, T, { if (P.NCH == 1) OR_SWEEP(T, 1); else if (P.NCH == 2) OR_SWEEP(T, 2); else OR_SWEEP(T, 3); });
#undef OR_SWEEP
    HIP_TRY(hipGetLastError());
    return E_OK;
}

static int or_launch_apply(tspgpu_ctx *ctx, int slot, const SweepGeom &P)
{
    const int BT = std::min(1024, std::max(64, pow2_ceil(ctx->n / 8)));
    LAUNCH_BY_COST(k_oropt_apply, dim3(1), dim3(BT), slot, P.W, ctx->d_or);
    HIP_TRY(hipGetLastError());
    return E_OK;
}

// Or-opt moves on `slot` until a sweep finds nothing improving, max_moves (< 0: no cap) are applied or t_end (< 0: none) passes;
// one sweep launch and one apply launch per move (matrix-free mode: gather, sweep, apply), eight of them between looks at the
// control block (one under a deadline)
static int or_run(tspgpu_ctx *ctx, int slot, long max_moves, double t_end, long *moves, bool *late, OrCtl *last)
{
    OrCtl C;
    memset(&C, 0, sizeof C);
    C.move[0] = C.move[1] = C.move[2] = C.move[3] = -1;
    C.budget = max_moves;
    if (late) *late = false;
    if (moves) *moves = 0;
    if (last) *last = C;
    if (max_moves == 0) return E_OK;
    int rc = ctl_put(ctx, ctx->d_or.p, C);
    if (rc) return rc;
    const SweepGeom P = or_plan(ctx);
    const looks::Result r = looks::drive(
        now_s, t_end, 8,
        [&] { const int e = or_launch_sweep(ctx, slot, P); return e ? e : or_launch_apply(ctx, slot, P); },
        [&] { const int e = ctl_get(ctx, &C, ctx->d_or.p); return e ? e : C.stop ? (int)looks::STOP : (int)looks::GO_ON; });
    if (r.code) return r.code;
    if (late) *late = r.late;
    if (r.late && (rc = ctl_get(ctx, &C, ctx->d_or.p))) return rc;      // (as m2_run: every round under a deadline has its look, so C stands)
    if (moves) *moves = (long)C.moves;
    if (last) *last = C;
    return E_OK;
}

// the descent of tspgpu_local_search on a slot: { 2-opt to its local optimum; Or-opt until nothing improves } until Or-opt applies nothing
static int or_descent(tspgpu_ctx *ctx, int slot, double time_left_s, Descent *out, bool *late)
{
    const double t_end = deadline_of(time_left_s);
    Descent D;
    int rc = E_OK;
    *late = false;
    for (;;) {
        double left = -1;
        if (t_end >= 0 && (left = t_end - now_s()) <= 0) { *late = true; break; }
        hipLaunchKernelGGL(k_rearm, dim3(1), dim3(64), 0, ctx->stream, ctx->S, slot, 1, -1);
        HIP_TRY(hipGetLastError());
        if ((rc = run_sweeps(ctx, slot, 1, false, -1, left, late))) break;
        int ns = 0;
        HIP_TRY(hipMemcpyAsync(&ns, ctx->S.nsweeps + slot, 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        D.tw += ns; D.nr++;
        if (*late) break;
        long m = 0;
        if ((rc = or_run(ctx, slot, -1, t_end, &m, late, nullptr))) break;
        D.om += m;
        if (*late || m == 0) break;
    }
    *out = D;
    return rc;
}

// ---- the same descent over a batch of slots ----

template <typename T> static const void *or_sweep_batch_fn(int nch)
{
    return nch == 1 ? (const void *)k_oropt_sweep_batch<T, 1> : nch == 2 ? (const void *)k_oropt_sweep_batch<T, 2>
                                                                         : (const void *)k_oropt_sweep_batch<T, 3>;
}

// or_plan sizes R so that ONE tour's workgroups fill the chip; with `live` tours in flight fewer workgroups per tour do, and a
// workgroup of R positions streams R + 2 rows: the largest R at which live * W still gives every CU two workgroups (one to
// compute while the other waits at its barrier), never below the single-tour R
static SweepGeom or_plan_batch(const tspgpu_ctx *ctx, int live)
{
    SweepGeom P = or_plan(ctx);
    const int n = ctx->n;
    const long target = (long)ctx->cus * std::min(P.occ, 2);
    for (int R = OR_RMAX; R > P.R; R--)
        if ((long)live * ((n + R - 1) / R) >= target) { P.R = R; break; }
    P.W = (n + P.R - 1) / P.R;
    ELEM_SWITCH(ctx->elem, T, P.fn = or_sweep_batch_fn<T>(P.NCH));
    return P;
}

// one Or-opt round on the first `live` slots of the list: a sweep launch and an apply launch (grid rows in runs of 65 535)
static int or_launch_round(tspgpu_ctx *ctx, int live, const SweepGeom &P)
{
    const int rc = ensure_max_lds(ctx, P.fn);
    if (rc) return rc;
    for (int off = 0; off < live; off += 65535) {
        const int rows = std::min(65535, live - off);
        const int *list = ctx->d_live + off;
#define OR_SWEEP(T, N) hipLaunchKernelGGL((k_oropt_sweep_batch<T, N>), dim3(P.W, rows), dim3(P.BT), P.lds, ctx->stream, ctx->S, \
                                          (const T *)ctx->d_mat.p, ctx->n, ctx->ld, list, P.R, (const OrCtl *)ctx->d_or_ctl)
        ELEM_SWITCH(ctx->elem, T, { if (P.NCH == 1) OR_SWEEP(T, 1); else if (P.NCH == 2) OR_SWEEP(T, 2); else OR_SWEEP(T, 3); });
#undef OR_SWEEP
        HIP_TRY(hipGetLastError());
    }
    const int BT = std::min(1024, std::max(64, pow2_ceil(ctx->n / 8)));
    ELEM_SWITCH(ctx->elem, T, hipLaunchKernelGGL((k_oropt_apply_batch<T>), dim3(live), dim3(BT), 0, ctx->stream, ctx->S, (const T *)ctx->d_mat.p,
                                                 ctx->n, ctx->ld, (const int *)ctx->d_live, P.W, ctx->d_or_ctl));
    HIP_TRY(hipGetLastError());
    return E_OK;
}

// or_descent on the slots slot0 .. slot0 + count - 1 at once; every tour goes through exactly the sequence or_descent runs on it.
// A tour is LIVE until one of its Or-opt phases applies nothing.  Per round: the live tours are re-armed (k_rearm_list: a
// finished tour keeps done = 1 and is skipped by the sweep kernels, so it runs no extra sweep) and run_sweeps takes the whole
// range to the 2-opt optimum; then Or-opt rounds -- one sweep and one apply launch for all tours still in the phase -- with the
// control blocks read back every 8 rounds (every round under a deadline) and the list rebuilt from them.
// D: per-slot 2-opt sweeps, Or-opt moves and 2-opt descents, [count].
static int or_descent_batch(tspgpu_ctx *ctx, int slot0, int count, double time_left_s, Descent *D, bool *late)
{
    const double t_end = deadline_of(time_left_s);
    std::vector<int> live(count), act;
    std::vector<OrCtl> hc(count);
    for (int i = 0; i < count; i++) { live[i] = slot0 + i; D[i] = Descent{}; }
    *late = false;
    ctx->or_batch_R = 0;
    int rc;
    auto read_ctl = [&] { return ctl_get(ctx, hc.data(), ctx->d_or_ctl + slot0, (size_t)count); };
    while (!live.empty()) {
        double left = -1;
        if (t_end >= 0 && (left = t_end - now_s()) <= 0) { *late = true; break; }
        const int nl = (int)live.size();
        if ((rc = set_live(ctx, live))) return rc;
        hipLaunchKernelGGL(k_rearm_list, dim3((nl + 255) / 256), dim3(256), 0, ctx->stream, ctx->S, (const int *)ctx->d_live, nl, -1);
        HIP_TRY(hipGetLastError());
        if ((rc = run_sweeps(ctx, slot0, count, false, -1, left, late))) return rc;
        HIP_TRY(hipMemcpyAsync(ctx->h_status, ctx->S.nsweeps + slot0, (size_t)count * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (int t : live) { D[t - slot0].tw += ctx->h_status[t - slot0]; D[t - slot0].nr++; }
        if (*late) break;
        // the Or-opt phase of the live tours (the list uploaded above is still theirs)
        hipLaunchKernelGGL(k_or_arm, dim3((nl + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_or_ctl, (const int *)ctx->d_live, nl);
        HIP_TRY(hipGetLastError());
        act = live;             // d_live holds `act`, and only set_live writes it: a list that did not shrink is not uploaded again
        SweepGeom P{};
        const looks::Result r = looks::drive_live(
            now_s, t_end, 8, act,
            [&](int len) { P = or_plan_batch(ctx, len); if (!ctx->or_batch_R) ctx->or_batch_R = P.R; },
            [&](int len) { return or_launch_round(ctx, len, P); }, read_ctl, [&](int t) { return hc[t - slot0].stop != 0; },
            [&](const std::vector<int> &list) { return set_live(ctx, list); });
        if (r.code) return r.code;
        *late = r.late;
        if (*late && (rc = read_ctl())) return rc;
        size_t k = 0;
        for (int t : live) {
            const long m = (long)hc[t - slot0].moves;
            D[t - slot0].om += m;
            if (m > 0) live[k++] = t;
        }
        live.resize(k);
        if (*late) break;
    }
    return E_OK;
}

// the argument checks of the batched entry points: the slots exist and hold tours
static int or_batch_args(tspgpu_ctx *ctx, int slot0, int count, bool rewrites = true)
{
    if (slot0 < 0 || count <= 0 || slot0 > INT_MAX - count) return fail(ctx, E_INVALID, "bad slot range: slot0 %d, count %d", slot0, count);
    for (int i = 0; i < count; i++) {
        const int rc = need_slot(ctx, slot0 + i);
        if (rc) return rc;
    }
    if (rewrites) wake_slots(ctx, slot0, count);    // (a batched descent rewrites them; one with looks keeps the sets itself)
    return E_OK;
}

extern "C" {

int tspgpu_tours_local_search(tspgpu_ctx *ctx, int slot0, int count, double time_left_s, long *two_opt_sweeps, long *or_moves, int *rounds)
{
    if (!ctx) return E_UNAVAILABLE;
    hipSetDevice(ctx->device);
    int rc = or_check(ctx, true);
    if (rc) return rc;
    if ((rc = or_batch_args(ctx, slot0, count))) return rc;
    std::vector<Descent> D(count);
    bool late = false;
    if ((rc = or_descent_batch(ctx, slot0, count, time_left_s, D.data(), &late))) return rc;
    descent_out(D.data(), count, DescentOut{two_opt_sweeps, nullptr, nullptr, or_moves, rounds});
    return done_code(late);
}

int tspgpu_multistart_local_search(tspgpu_ctx *ctx, const int *starts, int nstarts, double time_left_s, int *best_path, double *best_cost,
                                   int *best_start, long *total_two_opt_sweeps, long *total_or_moves, double *costs_out)
{
    if (!ctx) return E_UNAVAILABLE;
    if (!best_path || !best_cost || !best_start || nstarts <= 0) return fail(ctx, E_INVALID, "bad argument");
    hipSetDevice(ctx->device);
    int rc = or_check(ctx, true);
    if (rc) return rc;
    if (ctx->opt_sweep_cap != -1)
        return fail(ctx, E_INVALID, "TSPGPU_OPT_SWEEP_CAP = %d: the 2-opt + Or-opt descent runs every 2-opt phase to its local optimum", ctx->opt_sweep_cap);
    MultiStart ms;
    rc = multistart(ctx, starts, nstarts, time_left_s, -1, best_path, best_cost, best_start, costs_out, &ms,
                    [&](int m, double left, bool *late, Descent *D) { return or_descent_batch(ctx, 0, m, left, D, late); });
    if (rc && rc != E_DEADLINE) return rc;
    descent_out(&ms.total, 1, DescentOut{total_two_opt_sweeps, nullptr, nullptr, total_or_moves});
    return rc;
}

int tspgpu_tour_or_opt(tspgpu_ctx *ctx, int slot, long max_moves, double time_left_s, long *moves)
{
    if (!ctx) return E_UNAVAILABLE;
    return with_slot(ctx, slot, or_check, [&](bool *late) { return or_run(ctx, slot, max_moves, deadline_of(time_left_s), moves, late, nullptr); });
}

int tspgpu_tour_local_search(tspgpu_ctx *ctx, int slot, double time_left_s, long *two_opt_sweeps, long *or_moves, int *rounds)
{
    if (!ctx) return E_UNAVAILABLE;
    return with_slot(ctx, slot, or_check, [&](bool *late) {
        Descent D;
        const int rc = or_descent(ctx, slot, time_left_s, &D, late);
        descent_out(&D, 1, DescentOut{two_opt_sweeps, nullptr, nullptr, or_moves, rounds});
        return rc;
    });
}

int tspgpu_time_or_sweep(tspgpu_ctx *ctx, int slot, int reps, float *ms_mean)
{
    if (!ctx) return E_UNAVAILABLE;
    if (!ms_mean || reps <= 0) return fail(ctx, E_INVALID, "bad argument");
    hipSetDevice(ctx->device);
    int rc = or_check(ctx);
    if (rc) return rc;
    if ((rc = need_slot(ctx, slot))) return rc;
    HIP_TRY(hipMemsetAsync(ctx->d_or, 0, sizeof(OrCtl), ctx->stream));
    const SweepGeom P = or_plan(ctx);
    // warm: in matrix-free mode with its gather; the timed launches are the sweep kernel alone
    return time_launches(ctx, reps, [&] { return or_launch_sweep(ctx, slot, P); }, [&] { return or_launch_sweep(ctx, slot, P, false); }, ms_mean);
}

int tspgpu_or_opt_once(tspgpu_ctx *ctx, int *path, double *cost, double *delta, int move[4])
{
    if (!ctx) return E_UNAVAILABLE;
    if (!path || !cost) return fail(ctx, E_INVALID, "null argument");
    OrCtl C;
    const int rc = with_host_tour(ctx, path, cost, true, or_check, [&](bool *) { return or_run(ctx, 0, 1, -1, nullptr, nullptr, &C); });
    if (rc) return rc;
    if (delta) *delta = C.applied ? C.d : 0.0;
    if (move) for (int i = 0; i < 4; i++) move[i] = C.applied ? C.move[i] : -1;
    return E_OK;
}

int tspgpu_or_opt(tspgpu_ctx *ctx, int *path, double *cost, double time_left_s, long *moves)
{
    if (!ctx) return E_UNAVAILABLE;
    if (!path || !cost) return fail(ctx, E_INVALID, "null argument");
    return with_host_tour(ctx, path, cost, true, or_check,
                          [&](bool *late) { return or_run(ctx, 0, -1, deadline_of(time_left_s), moves, late, nullptr); });
}

int tspgpu_local_search(tspgpu_ctx *ctx, int *path, double *cost, double time_left_s, long *two_opt_sweeps, long *or_moves, int *rounds)
{
    if (!ctx) return E_UNAVAILABLE;
    if (!path || !cost) return fail(ctx, E_INVALID, "null argument");
    return with_host_tour(ctx, path, cost, false, or_check, [&](bool *late) {
        Descent D;
        const int rc = or_descent(ctx, 0, time_left_s, &D, late);
        descent_out(&D, 1, DescentOut{two_opt_sweeps, nullptr, nullptr, or_moves, rounds});
        return rc;
    });
}

} // extern "C"

// ---- parallel-move 2-opt (tspgpu_multi2opt.inc) ------------------------------------------------------------------------

static int m2_check(tspgpu_ctx *ctx)
{
    int rc = need_costs(ctx);
    if (rc) return rc;
    const int n = ctx->n;
    if (n < 5) return fail(ctx, E_INVALID, "parallel-move 2-opt needs at least 5 nodes, got %d", n);
    if (!ctx->symmetric) return fail(ctx, E_PRECOND, "parallel-move 2-opt needs a symmetric cost matrix");
    if (!ctx->otf && (size_t)ctx->ld * elem_size(ctx->elem) + M2_EXTRA > ctx->lds_max)     // (the matrix 2-opt's own limit: tspgpu_build_costs)
        return fail(ctx, E_EXHAUSTED, "n = %d: a matrix row of %d-byte cells does not fit LDS (at most %d nodes)", n,
                    (int)elem_size(ctx->elem), (int)((ctx->lds_max - M2_EXTRA) / elem_size(ctx->elem)) & ~31);
    if (ctx->otf && (rc = ensure_spts(ctx, (size_t)n))) return rc;     // sized as make_plan sizes them for one tour
    HIP_TRY(ctx->d_m2.reserve(1));
    // all eight or none: a later call must not find half of them
    if (!ctx->m2.raw_d) HIP_TRY(tspmem::grow(HipMem{ctx->stream}, ctx->m2_rows(ctx->m2, (size_t)n), 0, 1));
    return E_OK;
}

template <typename T> static const void *m2_sweep_fn(int nch)
{
    return nch == 1 ? (const void *)k_m2_sweep<T, 1> : nch == 2 ? (const void *)k_m2_sweep<T, 2>
         : nch == 4 ? (const void *)k_m2_sweep<T, 4> : (const void *)k_m2_sweep<T, 10>;
}

// one row in LDS; the vectors per thread and row are the template's 1, 2, 4 or 10 (a row fits LDS -- need_costs --, 10 240
// vectors at most)
static SweepGeom m2_plan(const tspgpu_ctx *ctx)
{
    SweepGeom P = plan::sweep_geom(plan_in(ctx), 1, M2_EXTRA, M2_RMIN, M2_RMAX, {1, 2, 4, 10}, M2_OTF_RUN);
    if (!ctx->otf) ELEM_SWITCH(ctx->elem, T, P.fn = m2_sweep_fn<T>(P.NCH));
    return P;
}

// what = 0 / 1 / 2: positions per workgroup / threads per workgroup / 16-byte vectors per thread and row of the candidate sweep
// (0: no symmetric costs of >= 5 nodes; the vectors also in matrix-free mode)
static int m2_geom(const tspgpu_ctx *ctx, int what)
{
    if (!ctx->have_costs || !ctx->symmetric || ctx->n < 5) return 0;
    const SweepGeom P = m2_plan(ctx);
    return what == 0 ? P.R : what == 1 ? P.BT : P.NCH;
}

// the host's copy of a sweep's compacted list, as far as a family's `put` reads it.  The names are the device buffers': a, b the
// candidate as M2Buf holds it; i, j the two ends of its range (for the 3-opt: the rule's i and k); jk what k_nl3_describe left
// in raw_b, the 3-opt's middle position and kind as j << 2 | kind
struct M2Moves { std::vector<int> a, b, i, j, jk; };

// A parallel-move family: where the candidates of a sweep come from and what an accepted one is.  The drivers below (m2_run,
// m2_once, m2_time) know a family only through this; the four instances stand behind their families' launch functions
struct M2Family {
    int (*check)(tspgpu_ctx *);
    int (*sweep)(tspgpu_ctx *, int slot, const SweepGeom &P, bool gather);      // the candidate sweep (P, gather: the full family's)
    void (*compact)(tspgpu_ctx *, int slot);                                    // the launch of its compaction
    int (*apply)(tspgpu_ctx *, int slot);
    int ints;                                                                   // ints per move in the caller's `moves` array
    int (*describe)(tspgpu_ctx *, size_t m, M2Moves &L);    // queues what `put` needs beyond a and b, while the tour still stands (or null)
    void (*put)(int *out, const M2Moves &L, int x);         // candidate x into the caller's array
    M2Counters tspgpu_ctx::*count;
    long tspgpu_ctx::*voids;                                // a descent's counter that a new run of the family takes back to 0 (or null)
    // "Don't-look bits" (null / -1: the family has none): its set, the queue pass over its window with the queued sweep behind
    // it, and the wake pass that goes between the selection and the apply
    int look_set = -1;
    int (*qsweep)(tspgpu_ctx *, int slot, const LookBuf &K, int closing) = nullptr;
    int (*wake)(tspgpu_ctx *, int slot, const LookBuf &K) = nullptr;
};

// every b of every node (k_m2_sweep; matrix-free mode: behind the gather of the successors' points)
static int m2_sweep_full(tspgpu_ctx *ctx, int slot, const SweepGeom &P, bool gather)
{
    const int n = ctx->n;
    const M2Ctl *ctl = ctx->d_m2;
    int rc;
    if (ctx->otf) {
        if (gather && (rc = launch_spts_gather(ctx, slot, &ctl->stop))) return rc;
        kind_switch(ctx, [&](auto kind, auto *pts, auto *spts) {
            hipLaunchKernelGGL((k_m2_sweep_otf<kind()>), dim3(P.W), dim3(P.BT), 0, ctx->stream, ctx->S, pts, spts, n, slot, ctx->m2, ctl);
        });
    } else {
        if ((rc = ensure_max_lds(ctx, P.fn))) return rc;
#define M2_SWEEP(T, N) hipLaunchKernelGGL((k_m2_sweep<T, N>), dim3(P.W), dim3(P.BT), P.lds, ctx->stream, ctx->S, (const T *)ctx->d_mat.p, \
                                          n, ctx->ld, slot, P.R, ctx->m2, ctl)
        ELEM_SWITCH(ctx->elem, T, { if (P.NCH == 1) M2_SWEEP(T, 1); else if (P.NCH == 2) M2_SWEEP(T, 2);
                                    else if (P.NCH == 4) M2_SWEEP(T, 4); else M2_SWEEP(T, 10); });
#undef M2_SWEEP
    }
    return E_OK;
}

static void m2_compact_pairs(tspgpu_ctx *ctx, int slot)
{
    hipLaunchKernelGGL(k_m2_compact, dim3(1), dim3(1024), 0, ctx->stream, ctx->S, ctx->n, slot, ctx->m2, ctx->d_m2);
}

static int m2_apply_pairs(tspgpu_ctx *ctx, int slot)
{
    const int G = std::min(M2_APPLY_WGS, (ctx->n + 1) / 2);
    LAUNCH_BY_COST(k_m2_apply, dim3(G), dim3(256), slot, ctx->m2, ctx->d_m2);
    HIP_TRY(hipGetLastError());
    return E_OK;
}

static void m2_put_pair(int *out, const M2Moves &L, int x) { out[0] = L.a[x]; out[1] = L.b[x]; }

static const M2Family M2_FULL = {m2_check, m2_sweep_full, m2_compact_pairs, m2_apply_pairs, 2, nullptr, m2_put_pair, &tspgpu_ctx::m2_count, nullptr};

// the candidate sweep and the selection of one sweep; K: the queue pass over the family's window and the queued sweep instead
static int m2_launch_select(tspgpu_ctx *ctx, int slot, const SweepGeom &P, bool gather, const M2Family &F, const LookBuf *K = nullptr,
                            int closing = 0)
{
    const int rc = K ? F.qsweep(ctx, slot, *K, closing) : F.sweep(ctx, slot, P, gather);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    F.compact(ctx, slot);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_m2_select, dim3((ctx->n + 255) / 256), dim3(256), 0, ctx->stream, ctx->m2, (const M2Ctl *)ctx->d_m2);
    HIP_TRY(hipGetLastError());
    return E_OK;
}

// the control block of a run := nothing done yet, `budget` sweeps allowed (< 0: no cap); the slot's sweep counter and flag re-armed
static int m2_arm(tspgpu_ctx *ctx, int slot, long budget)
{
    M2Ctl C;
    memset(&C, 0, sizeof C);
    C.budget = budget;
    const int rc = ctl_put(ctx, ctx->d_m2.p, C);
    if (rc) return rc;
    hipLaunchKernelGGL(k_rearm, dim3(1), dim3(64), 0, ctx->stream, ctx->S, slot, 1, -1);
    HIP_TRY(hipGetLastError());
    return E_OK;
}

static void m2_record(tspgpu_ctx *ctx, const M2Ctl &C, const M2Family &F)
{
    ctx->*F.count = M2Counters{(long)C.sweeps, (long)C.moves, (long)C.max_k};
    if (F.voids) ctx->*F.voids = 0;
}

// what a phase with looks ("Don't-look bits") counts beyond its sweeps and moves; a phase with looks is m2_run with an M2Looks
struct DlCount {
    long looked = 0, full = 0, max_q = 0;
    void operator+=(const DlCount &d) { looked += d.looked; full += d.full; max_q = std::max(max_q, d.max_q); }
};
struct M2Looks { int closing; DlCount *dl; };
static int look_buf(tspgpu_ctx *ctx, int slot, bool sets, LookBuf *K);

// sweeps on `slot` until one accepts nothing, max_sweeps (< 0: no cap) have run or t_end (< 0: none) passes; per sweep the
// launches of m2_launch_select and the family's apply, four sweeps between looks at the control block (looks::drive).
// lk: the phase with looks of the family: the queue pass in front of the sweep and the wake pass in front of the apply, and
// the host decides at its look what a stopped phase does next (looks::after_stop); *lk->dl: totals over the phase
static int m2_run(tspgpu_ctx *ctx, int slot, long max_sweeps, double t_end, long *sweeps, long *moves, bool *late, const M2Family &F,
                  const M2Looks *lk = nullptr)
{
    M2Ctl C;
    LookCtl LC;
    memset(&C, 0, sizeof C);
    memset(&LC, 0, sizeof LC);
    *late = false;
    if (lk) *lk->dl = DlCount{};
    if (sweeps) *sweeps = 0;
    if (moves) *moves = 0;
    m2_record(ctx, C, F);
    if (max_sweeps == 0) return E_OK;
    LookBuf K{};
    int rc;
    if (lk) {
        if ((rc = look_buf(ctx, slot, true, &K))) return rc;
        HIP_TRY(hipMemsetAsync(ctx->d_look, 0, sizeof(LookCtl), ctx->stream));
    }
    if ((rc = m2_arm(ctx, slot, max_sweeps))) return rc;
    const SweepGeom P = m2_plan(ctx);
    const int n = ctx->n;
    const looks::Result r = looks::drive(
        now_s, t_end, 4,
        [&]() -> int {
            int e = m2_launch_select(ctx, slot, P, true, F, lk ? &K : nullptr, lk ? lk->closing : 0);
            if (e) return e;
            if (lk && (e = F.wake(ctx, slot, K))) return e;
            return F.apply(ctx, slot);
        },
        [&]() -> int {
            int e = ctl_get(ctx, &C, ctx->d_m2.p);
            if (e) return e;
            if (!C.stop) return (int)looks::GO_ON;
            if (!lk) return (int)looks::STOP;
            if ((e = ctl_get(ctx, &LC, (const LookCtl *)ctx->d_look))) return e;
            const looks::AfterStop next = looks::after_stop(lk->closing != 0, C.sweeps, C.last_k, LC.last_q, n, C.budget);
            if (next == looks::AfterStop::END) return (int)looks::STOP;
            HIP_TRY(hipMemsetAsync(K.awake + (size_t)F.look_set * n, 1, (size_t)n, ctx->stream));
            if (next == looks::AfterStop::WAKE_END) return (int)looks::STOP;
            HIP_TRY(hipMemsetAsync(&ctx->d_m2.p->stop, 0, sizeof(int), ctx->stream));
            return (int)looks::GO_ON;
        });
    if (r.code) return r.code;
    *late = r.late;
    if (r.late && (rc = ctl_get(ctx, &C, ctx->d_m2.p))) return rc;
    if (lk && (rc = ctl_get(ctx, &LC, (const LookCtl *)ctx->d_look))) return rc;
    if (sweeps) *sweeps = (long)C.sweeps;
    if (moves) *moves = (long)C.moves;
    if (lk) *lk->dl = DlCount{(long)LC.looked, (long)LC.full, (long)LC.max_q};
    m2_record(ctx, C, F);
    return E_OK;
}

extern "C" {

int tspgpu_tour_two_opt_multi(tspgpu_ctx *ctx, int slot, long max_sweeps, double time_left_s, long *sweeps, long *moves)
{
    if (!ctx) return E_UNAVAILABLE;
    return with_slot(ctx, slot, m2_check,
                     [&](bool *late) { return m2_run(ctx, slot, max_sweeps, deadline_of(time_left_s), sweeps, moves, late, M2_FULL); });
}

int tspgpu_two_opt_multi(tspgpu_ctx *ctx, int *path, double *cost, double time_left_s, long *sweeps, long *moves)
{
    if (!ctx) return E_UNAVAILABLE;
    if (!path || !cost) return fail(ctx, E_INVALID, "null argument");
    return with_host_tour(ctx, path, cost, false, m2_check,
                          [&](bool *late) { return m2_run(ctx, 0, -1, deadline_of(time_left_s), sweeps, moves, late, M2_FULL); });
}

} // extern "C"

// one sweep of family F on a host tour, `F.ints` ints per move in `moves` (tspgpu_two_opt_multi_once, tspgpu_two_opt_nl_once,
// tspgpu_or_opt_nl_once, tspgpu_three_opt_nl_once)
static int m2_once(tspgpu_ctx *ctx, int *path, double *cost, int *nmoves, int *moves, double *deltas, int cap, const M2Family &F)
{
    if (!ctx) return E_UNAVAILABLE;
    if (!path || !cost || cap < 0 || (cap > 0 && (!moves || !deltas))) return fail(ctx, E_INVALID, "bad argument");
    hipSetDevice(ctx->device);
    int rc = F.check(ctx);
    if (rc) return rc;
    if ((rc = load_path(ctx, 0, path, -1))) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->S.cost, cost, 8, hipMemcpyHostToDevice, ctx->stream));     // the caller's running cost, as ref_2opt_once
    if ((rc = m2_arm(ctx, 0, 1))) return rc;
    if ((rc = m2_launch_select(ctx, 0, m2_plan(ctx), true, F))) return rc;
    // the accepted list comes back before anything is applied: a list longer than `cap` leaves the tour as it is
    M2Ctl C;
    if ((rc = ctl_get(ctx, &C, ctx->d_m2.p))) return rc;
    const size_t m = (size_t)C.m;
    M2Moves L;
    L.a.resize(m); L.b.resize(m);
    std::vector<int> acc(m);
    std::vector<double> d(m);
    if (m) {
        if (F.describe && (rc = F.describe(ctx, m, L))) return rc;
        HIP_TRY(hipMemcpyAsync(acc.data(), ctx->m2.acc, m * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(L.a.data(), ctx->m2.a, m * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(L.b.data(), ctx->m2.b, m * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d.data(), ctx->m2.d, m * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    std::vector<int> idx;
    for (size_t x = 0; x < m; x++) if (acc[x]) idx.push_back((int)x);
    if ((int)idx.size() > cap)
        return fail(ctx, E_EXHAUSTED, "the sweep accepts %d moves, the caller's arrays hold %d: nothing was applied", (int)idx.size(), cap);
    std::sort(idx.begin(), idx.end(), [&](int x, int y) {
        if (d[x] != d[y]) return d[x] < d[y];
        const int lx = std::min(L.a[x], L.b[x]), ly = std::min(L.a[y], L.b[y]);
        return lx != ly ? lx < ly : std::max(L.a[x], L.b[x]) < std::max(L.a[y], L.b[y]);
    });
    for (size_t k = 0; k < idx.size(); k++) {
        deltas[k] = d[idx[k]];
        F.put(moves + (size_t)F.ints * k, L, idx[k]);
    }
    if (nmoves) *nmoves = (int)idx.size();
    if ((rc = F.apply(ctx, 0))) return rc;
    if ((rc = store_path(ctx, 0, path, cost, nullptr))) return rc;
    if ((rc = ctl_get(ctx, &C, ctx->d_m2.p))) return rc;
    m2_record(ctx, C, F);
    return E_OK;
}

// the candidate sweep and the selection `reps` times, nothing applied (tspgpu_time_multi_sweep, tspgpu_time_nl_sweep,
// tspgpu_time_or_nl_sweep, tspgpu_time_three_nl_sweep)
static int m2_time(tspgpu_ctx *ctx, int slot, int reps, float *ms_mean, const M2Family &F)
{
    if (!ctx) return E_UNAVAILABLE;
    if (!ms_mean || reps <= 0) return fail(ctx, E_INVALID, "bad argument");
    hipSetDevice(ctx->device);
    int rc = F.check(ctx);
    if (rc) return rc;
    if ((rc = need_slot(ctx, slot))) return rc;
    HIP_TRY(hipMemsetAsync(ctx->d_m2, 0, sizeof(M2Ctl), ctx->stream));
    const SweepGeom P = m2_plan(ctx);
    // warm: in matrix-free mode with its gather; the timed launches go without
    return time_launches(ctx, reps, [&] { return m2_launch_select(ctx, slot, P, true, F); },
                         [&] { return m2_launch_select(ctx, slot, P, false, F); }, ms_mean);
}

extern "C" {

int tspgpu_two_opt_multi_once(tspgpu_ctx *ctx, int *path, double *cost, int *nmoves, int *moves_ab, double *deltas, int cap)
{
    return m2_once(ctx, path, cost, nmoves, moves_ab, deltas, cap, M2_FULL);
}

int tspgpu_time_multi_sweep(tspgpu_ctx *ctx, int slot, int reps, float *ms_mean)
{
    return m2_time(ctx, slot, reps, ms_mean, M2_FULL);
}

} // extern "C"

// ---- neighbour-list 2-opt (tspgpu_nl2opt.inc) --------------------------------------------------------------------------

// everything the parallel-move descent needs (the polish runs it on the same slot), and the lists
static int nl_check(tspgpu_ctx *ctx)
{
    const int rc = m2_check(ctx);
    if (rc) return rc;
    if (!ctx->nl.K)
        return fail(ctx, E_PRECOND, ctx->nl_dropped ? "the neighbour lists were invalidated by a new cost source: call tspgpu_neighbours_build again"
                                                    : "no neighbour lists: call tspgpu_neighbours_build first");
    return E_OK;
}

static int nl_launch_sweep(tspgpu_ctx *ctx, int slot, const SweepGeom &, bool)
{
    const dim3 grid((ctx->n + NL_NODES - 1) / NL_NODES), block(NL_NODES * 32);
    LAUNCH_BY_COST(k_nl_sweep, grid, block, slot, ctx->nl, ctx->m2, (const M2Ctl *)ctx->d_m2);
    HIP_TRY(hipGetLastError());
    return E_OK;
}

// "Don't-look bits": the workgroups of a queued sweep with `per_wg` units each, and of the wake pass: fixed from n and the chip
static dim3 look_grid(const tspgpu_ctx *ctx, int per_wg)
{
    return dim3((unsigned)std::max(1, std::min((ctx->n + per_wg - 1) / per_wg, LOOK_WGS_PER_CU * ctx->cus)));
}

// the queue pass of family F over a window of FWD positions behind the unit
template <int F, int FWD> static int look_launch_queue(tspgpu_ctx *ctx, int slot, const LookBuf &K, int closing)
{
    hipLaunchKernelGGL((k_look_queue<F, FWD>), dim3(1), dim3(1024), 0, ctx->stream, ctx->S, ctx->n, slot, K, ctx->m2, (M2Ctl *)ctx->d_m2, closing);
    HIP_TRY(hipGetLastError());
    return E_OK;
}

template <int F> static int look_launch_wake(tspgpu_ctx *ctx, int slot, const LookBuf &K)
{
    hipLaunchKernelGGL((k_look_wake<F>), look_grid(ctx, 256), dim3(256), 0, ctx->stream, ctx->S, ctx->n, slot, ctx->nl, K, ctx->m2,
                       (const M2Ctl *)ctx->d_m2);
    HIP_TRY(hipGetLastError());
    return E_OK;
}

static int nl_launch_qsweep(tspgpu_ctx *ctx, int slot, const LookBuf &K, int closing)
{
    const int rc = look_launch_queue<0, 0>(ctx, slot, K, closing);
    if (rc) return rc;
    LAUNCH_BY_COST(k_nl_qsweep, look_grid(ctx, NL_NODES), dim3(NL_NODES * 32), slot, ctx->nl, ctx->m2, (const M2Ctl *)ctx->d_m2, K);
    HIP_TRY(hipGetLastError());
    return E_OK;
}

// the lists' 2-opt pairs: compaction, apply and move layout are the full family's.  (A phase's polish is counted behind it,
// tspgpu_two_opt_nl: until then the phase has none)
static const M2Family M2_NL = {nl_check, nl_launch_sweep, m2_compact_pairs, m2_apply_pairs, 2, nullptr, m2_put_pair, &tspgpu_ctx::nl_count,
                               &tspgpu_ctx::nl_polish_sweeps, 0, nl_launch_qsweep, look_launch_wake<0>};

extern "C" {

int tspgpu_neighbours_build(tspgpu_ctx *ctx, int K)
{
    if (!ctx) return E_UNAVAILABLE;
    hipSetDevice(ctx->device);
    if (K == 0) { ctx->drop_nl(); ctx->drop_greedy(); ctx->nl_dropped = false; return E_OK; }
    if (K < 0 || K > NL_KMAX) return fail(ctx, E_INVALID, "neighbour lists hold 1 to %d nodes, got K = %d", NL_KMAX, K);
    int rc = need_costs(ctx);
    if (rc) return rc;
    if (!ctx->symmetric) return fail(ctx, E_PRECOND, "neighbour lists need a symmetric cost matrix");
    const int n = ctx->n, Kp = std::min(K, n - 1);
    ctx->drop_nl();             // a build that fails leaves no lists
    ctx->nl_dropped = false;
    DevBuf<int> node;
    DevBuf<double> w;
    HIP_TRY(tspmem::alloc_all<HipMem>({{&node, (size_t)n * Kp}, {&w, (size_t)n * Kp}}));
    const NlBuf L{Kp, node, w};
    const dim3 grid((n + NL_BUILD_ROWS - 1) / NL_BUILD_ROWS), block(NL_BUILD_ROWS * 64);
    if (ctx->otf)
        kind_switch(ctx, [&](auto kind, auto *pts, auto *) { hipLaunchKernelGGL((k_nl_build_otf<kind()>), grid, block, 0, ctx->stream, pts, n, L); });
    else
        ELEM_SWITCH(ctx->elem, T, hipLaunchKernelGGL((k_nl_build<T>), grid, block, 0, ctx->stream, (const T *)ctx->d_mat.p, n, ctx->ld, L));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->nl_node = std::move(node); ctx->nl_w = std::move(w);
    ctx->nl = L;
    return E_OK;
}

int tspgpu_neighbours_get(tspgpu_ctx *ctx, int *nodes, double *weights)
{
    if (!ctx) return E_UNAVAILABLE;
    if (!nodes) return fail(ctx, E_INVALID, "null argument");
    hipSetDevice(ctx->device);
    int rc = need_costs(ctx);
    if (rc) return rc;
    if (!ctx->nl.K) return nl_check(ctx);   // (the refusal's text)
    const size_t cnt = (size_t)ctx->n * ctx->nl.K;
    HIP_TRY(hipMemcpyAsync(nodes, ctx->nl.node, cnt * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (!weights) return E_OK;
    if (ctx->elem == TSPGPU_ELEM_F64) {
        HIP_TRY(hipMemcpyAsync(weights, ctx->nl.w, cnt * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    } else {                                // integer modes keep 4-byte weights
        std::vector<int> w(cnt);
        HIP_TRY(hipMemcpyAsync(w.data(), ctx->nl.w, cnt * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < cnt; i++) weights[i] = (double)w[i];
    }
    return E_OK;
}

int tspgpu_two_opt_nl_once(tspgpu_ctx *ctx, int *path, double *cost, int *nmoves, int *moves_ab, double *deltas, int cap)
{
    return m2_once(ctx, path, cost, nmoves, moves_ab, deltas, cap, M2_NL);
}

int tspgpu_tour_two_opt_nl(tspgpu_ctx *ctx, int slot, long max_sweeps, double time_left_s, long *sweeps, long *moves)
{
    if (!ctx) return E_UNAVAILABLE;
    return with_slot(ctx, slot, nl_check,
                     [&](bool *late) { return m2_run(ctx, slot, max_sweeps, deadline_of(time_left_s), sweeps, moves, late, M2_NL); });
}

int tspgpu_two_opt_nl(tspgpu_ctx *ctx, int *path, double *cost, double time_left_s, int polish,
                      long *sweeps, long *moves, long *polish_sweeps, long *polish_moves)
{
    if (!ctx) return E_UNAVAILABLE;
    if (!path || !cost) return fail(ctx, E_INVALID, "null argument");
    return with_host_tour(ctx, path, cost, false, nl_check, [&](bool *late) {
        const double t_end = deadline_of(time_left_s);
        long ps = 0, pm = 0;
        ctx->nl_polish_sweeps = 0;
        int rc = m2_run(ctx, 0, -1, t_end, sweeps, moves, late, M2_NL);
        if (rc) return rc;
        if (polish && !*late) {                 // the parallel-move descent goes on from the slot as it stands
            if ((rc = m2_run(ctx, 0, -1, t_end, &ps, &pm, late, M2_FULL))) return rc;
            ctx->nl_polish_sweeps = ps;
        }
        if (polish_sweeps) *polish_sweeps = ps;
        if (polish_moves) *polish_moves = pm;
        return (int)E_OK;
    });
}

int tspgpu_time_nl_sweep(tspgpu_ctx *ctx, int slot, int reps, float *ms_mean)
{
    return m2_time(ctx, slot, reps, ms_mean, M2_NL);
}

} // extern "C"

// ---- neighbour-list Or-opt and the descent over the lists (tspgpu_ornl.inc) ---------------------------------------------

// what the neighbour-list 2-opt needs (the descent alternates with it on the same slot), and Or-opt's eight nodes.  No row in
// LDS beyond the parallel-move limit, and no TSPGPU_OPT_OR_MATRIX_FREE: the costs come from the lists and single gathers
static int ornl_check(tspgpu_ctx *ctx)
{
    const int rc = need_costs(ctx);
    if (rc) return rc;
    if (ctx->n < 8) return fail(ctx, E_INVALID, "neighbour-list Or-opt needs at least 8 nodes, got %d", ctx->n);
    return nl_check(ctx);
}

static int ornl_launch_sweep(tspgpu_ctx *ctx, int slot, const SweepGeom &, bool)
{
    const dim3 grid((ctx->n + ORNL_STARTS - 1) / ORNL_STARTS), block(ORNL_STARTS * 64);
    LAUNCH_BY_COST(k_ornl_sweep, grid, block, slot, ctx->nl, ctx->m2, (const M2Ctl *)ctx->d_m2);
    HIP_TRY(hipGetLastError());
    return E_OK;
}

static int ornl_launch_qsweep(tspgpu_ctx *ctx, int slot, const LookBuf &K, int closing)
{
    const int rc = look_launch_queue<1, 2>(ctx, slot, K, closing);     // a changed edge (t, x) reaches the units whose segments end in t
    if (rc) return rc;
    LAUNCH_BY_COST(k_ornl_qsweep, look_grid(ctx, ORNL_STARTS), dim3(ORNL_STARTS * 64), slot, ctx->nl, ctx->m2, (const M2Ctl *)ctx->d_m2, K);
    HIP_TRY(hipGetLastError());
    return E_OK;
}

static int ornl_launch_apply(tspgpu_ctx *ctx, int slot)
{
    const int G = std::min(M2_APPLY_WGS, (ctx->n + 1) / 2);
    LAUNCH_BY_COST(k_ornl_apply, dim3(G), dim3(ORNL_APPLY_BT), slot, ctx->m2, ctx->d_m2);
    HIP_TRY(hipGetLastError());
    return E_OK;
}

static void ornl_launch_compact(tspgpu_ctx *ctx, int slot)
{
    hipLaunchKernelGGL(k_ornl_compact, dim3(1), dim3(1024), 0, ctx->stream, ctx->S, ctx->n, slot, ctx->m2, ctx->d_m2);
}

// s, L, q, rev of a = s < b = the packed (L, q, rev): m2_once's order (delta, a, b) is (delta, s, L, q, rev)
static void ornl_put(int *out, const M2Moves &L, int x)
{
    const int b = L.b[x];
    out[0] = L.a[x]; out[1] = b >> ORNL_LSHIFT; out[2] = (b >> 1) & (int)OR_QM; out[3] = b & 1;
}

static const M2Family M2_ORNL = {ornl_check, ornl_launch_sweep, ornl_launch_compact, ornl_launch_apply, 4, nullptr, ornl_put, &tspgpu_ctx::ornl_count,
                                 nullptr, 1, ornl_launch_qsweep, look_launch_wake<1>};

extern "C" {

int tspgpu_or_opt_nl_once(tspgpu_ctx *ctx, int *path, double *cost, int *nmoves, int *moves, double *deltas, int cap)
{
    return m2_once(ctx, path, cost, nmoves, moves, deltas, cap, M2_ORNL);
}

int tspgpu_or_opt_nl(tspgpu_ctx *ctx, int *path, double *cost, double time_left_s, long *sweeps, long *moves)
{
    if (!ctx) return E_UNAVAILABLE;
    if (!path || !cost) return fail(ctx, E_INVALID, "null argument");
    return with_host_tour(ctx, path, cost, true, ornl_check,
                          [&](bool *late) { return m2_run(ctx, 0, -1, deadline_of(time_left_s), sweeps, moves, late, M2_ORNL); });
}

int tspgpu_tour_or_opt_nl(tspgpu_ctx *ctx, int slot, long max_sweeps, double time_left_s, long *sweeps, long *moves)
{
    if (!ctx) return E_UNAVAILABLE;
    return with_slot(ctx, slot, ornl_check,
                     [&](bool *late) { return m2_run(ctx, slot, max_sweeps, deadline_of(time_left_s), sweeps, moves, late, M2_ORNL); });
}

int tspgpu_time_or_nl_sweep(tspgpu_ctx *ctx, int slot, int reps, float *ms_mean)
{
    return m2_time(ctx, slot, reps, ms_mean, M2_ORNL);
}

} // extern "C"

// ---- neighbour-list 3-opt and the descent with a 3-opt phase (tspgpu_nl3opt.inc) -----------------------------------------

// what the neighbour-list Or-opt needs (the descent runs its alternation on the same slot), and a width of 1 .. 16: W is the
// part of every list the chains are drawn from
static int nl3_check(tspgpu_ctx *ctx)
{
    if (ctx->nl3_width < 1 || ctx->nl3_width > NL_KMAX)
        return fail(ctx, E_INVALID, "neighbour-list 3-opt takes a width of 1 to %d list entries, got %d", NL_KMAX, ctx->nl3_width);
    const int rc = ornl_check(ctx);
    if (rc) return rc;
    ctx->nl3_w = std::min(ctx->nl3_width, ctx->nl.K);
    return E_OK;
}

static int nl3_launch_sweep(tspgpu_ctx *ctx, int slot, const SweepGeom &, bool)
{
    const dim3 grid((ctx->n + NL3_NODES - 1) / NL3_NODES), block(NL3_NODES * 64);
    LAUNCH_BY_COST(k_nl3_sweep, grid, block, slot, ctx->nl, ctx->nl3_w, ctx->m2, (const M2Ctl *)ctx->d_m2);
    HIP_TRY(hipGetLastError());
    return E_OK;
}

static int nl3_launch_qsweep(tspgpu_ctx *ctx, int slot, const LookBuf &K, int closing)
{
    const int rc = look_launch_queue<2, 0>(ctx, slot, K, closing);
    if (rc) return rc;
    LAUNCH_BY_COST(k_nl3_qsweep, look_grid(ctx, NL3_NODES), dim3(NL3_NODES * 64), slot, ctx->nl, ctx->nl3_w, ctx->m2, (const M2Ctl *)ctx->d_m2, K);
    HIP_TRY(hipGetLastError());
    return E_OK;
}

static int nl3_launch_apply(tspgpu_ctx *ctx, int slot)
{
    const int G = std::min(M2_APPLY_WGS, (ctx->n + 2) / 3);     // a range holds three positions at least
    LAUNCH_BY_COST(k_nl3_apply, dim3(G), dim3(NL3_APPLY_BT), slot, ctx->nl, ctx->m2, ctx->d_m2);
    HIP_TRY(hipGetLastError());
    return E_OK;
}

static void nl3_launch_compact(tspgpu_ctx *ctx, int slot)
{
    hipLaunchKernelGGL(k_nl3_compact, dim3(1), dim3(1024), 0, ctx->stream, ctx->S, ctx->n, slot, ctx->nl, ctx->m2, ctx->d_m2);
}

// the range and (j, kind) of every candidate of slot 0, while the tour still stands
static int nl3_describe(tspgpu_ctx *ctx, size_t m, M2Moves &L)
{
    L.i.resize(m); L.j.resize(m); L.jk.resize(m);
    hipLaunchKernelGGL(k_nl3_describe, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, ctx->S, ctx->n, 0, ctx->nl, ctx->m2, ctx->d_m2);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(L.i.data(), ctx->m2.i, m * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(L.j.data(), ctx->m2.j, m * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(L.jk.data(), ctx->m2.raw_b, m * 4, hipMemcpyDeviceToHost, ctx->stream));
    return E_OK;
}

// i, j, k, kind of a = t1 < b = the code: m2_once's order (delta, a, b) is (delta, t1, code)
static void nl3_put(int *out, const M2Moves &L, int x)
{
    out[0] = L.i[x]; out[1] = L.jk[x] >> 2; out[2] = L.j[x]; out[3] = L.jk[x] & 3;
}

static const M2Family M2_NL3 = {nl3_check, nl3_launch_sweep, nl3_launch_compact, nl3_launch_apply, 4, nl3_describe, nl3_put, &tspgpu_ctx::nl3_count,
                                nullptr, 2, nl3_launch_qsweep, look_launch_wake<2>};

extern "C" {

int tspgpu_three_opt_nl_once(tspgpu_ctx *ctx, int width, int *path, double *cost, int *nmoves, int *moves, double *deltas, int cap)
{
    if (!ctx) return E_UNAVAILABLE;
    ctx->nl3_width = width;
    return m2_once(ctx, path, cost, nmoves, moves, deltas, cap, M2_NL3);
}

int tspgpu_three_opt_nl(tspgpu_ctx *ctx, int width, int *path, double *cost, double time_left_s, long *sweeps, long *moves)
{
    if (!ctx) return E_UNAVAILABLE;
    if (!path || !cost) return fail(ctx, E_INVALID, "null argument");
    ctx->nl3_width = width;
    return with_host_tour(ctx, path, cost, true, nl3_check,
                          [&](bool *late) { return m2_run(ctx, 0, -1, deadline_of(time_left_s), sweeps, moves, late, M2_NL3); });
}

int tspgpu_tour_three_opt_nl(tspgpu_ctx *ctx, int slot, int width, long max_sweeps, double time_left_s, long *sweeps, long *moves)
{
    if (!ctx) return E_UNAVAILABLE;
    ctx->nl3_width = width;
    return with_slot(ctx, slot, nl3_check,
                     [&](bool *late) { return m2_run(ctx, slot, max_sweeps, deadline_of(time_left_s), sweeps, moves, late, M2_NL3); });
}

int tspgpu_time_three_nl_sweep(tspgpu_ctx *ctx, int slot, int width, int reps, float *ms_mean)
{
    if (!ctx) return E_UNAVAILABLE;
    ctx->nl3_width = width;
    return m2_time(ctx, slot, reps, ms_mean, M2_NL3);
}

} // extern "C"

// ---- don't-look bits for the neighbour-list families, and the kick on a slot (tspgpu_looks_dl.inc) --------------------------

// The queue and the control block (by n) and the slots' awake sets (3 n bytes per slot): all of them at the first call of
// "Don't-look bits", or none.  They go where the M2Buf and the slot arrays go (InstanceMem, SlotMem) and grow with the slots
static int ensure_looks(tspgpu_ctx *ctx)
{
    const size_t n = (size_t)ctx->n;
    const bool fresh = !ctx->d_lq;
    if (fresh) HIP_TRY(tspmem::grow(HipMem{ctx->stream}, ctx->look_ctx_rows(n), 0, 1));
    if (!ctx->lcap) {
        const hipError_t e = tspmem::grow(HipMem{ctx->stream}, ctx->look_rows(n), 0, (size_t)ctx->tcap);
        if (e != hipSuccess) {
            if (fresh) ctx->drop_look_ctx();
            return fail(ctx, E_INTERNAL, "the awake sets of %d slots: %s", ctx->tcap, hipGetErrorString(e));
        }
        ctx->lcap = ctx->tcap;
    }
    return E_OK;
}

// the look state of a slot that holds a tour; a slot flagged "all awake" has its sets filled first (sets != 0), so that the
// device arrays are what counts from here on
static int look_buf(tspgpu_ctx *ctx, int slot, bool sets, LookBuf *K)
{
    const int rc = ensure_looks(ctx);
    if (rc) return rc;
    const size_t n = (size_t)ctx->n;
    *K = LookBuf{ctx->d_awake + (size_t)slot * 3 * n, ctx->d_lq, ctx->d_look};
    if (sets && ctx->look_all[slot]) {
        HIP_TRY(hipMemsetAsync(K->awake, 1, 3 * n, ctx->stream));
        ctx->look_all[slot] = 0;
    }
    return E_OK;
}

static void dl_record(tspgpu_ctx *ctx, const DlCount &dl) { ctx->dl_looked = dl.looked; ctx->dl_full = dl.full; ctx->dl_max_q = dl.max_q; }

// a single phase with looks on a slot (tspgpu_tour_two_opt_nl_dl, _or_opt_nl_dl, _three_opt_nl_dl)
static int dl_phase(tspgpu_ctx *ctx, int slot, int closing, long max_sweeps, double time_left_s, long *sweeps, long *moves, long *looked,
                    const M2Family &F)
{
    return with_slot(ctx, slot, F.check, [&](bool *late) {
        DlCount dl;
        const M2Looks lk{closing, &dl};
        const int rc = m2_run(ctx, slot, max_sweeps, deadline_of(time_left_s), sweeps, moves, late, F, &lk);
        if (rc) return rc;
        dl_record(ctx, dl);
        if (looked) *looked = dl.looked;
        return (int)E_OK;
    }, true);
}

// a width of 0 .. 16; 0: the checks of the descent without a 3-opt phase
static int dl_descent_check(tspgpu_ctx *ctx)
{
    if (ctx->nl3_width == 0) return ornl_check(ctx);
    return nl3_check(ctx);
}

// ---- the descent over the neighbour lists behind its entry points: plain, with a 3-opt phase, with looks --------------------

// the looks mode of a batched descent: off, or "Batched don't-look bits" with its `closing`
struct NlbMode { bool looks = false; int closing = 0; };

// which descent an entry point asks for: tspgpu_*_nl (nl_plain), tspgpu_*_nl3 (nl_three), tspgpu_*_nl3_dl (nl_looks)
struct NlSpec {
    int (*check)(tspgpu_ctx *);
    int width;              // the caller's
    bool keep;              // ... goes into ctx->nl3_width; the plain forms leave that as it is
    bool looks;             // every phase is a phase with looks
    int closing;
    // the width of the 3-opt phase once `check` has passed, 0: the descent has none
    int w3(const tspgpu_ctx *ctx) const { return looks ? (width ? ctx->nl3_w : 0) : keep ? ctx->nl3_w : 0; }
    NlbMode mode() const { return NlbMode{looks, closing}; }
};
static NlSpec nl_plain() { return NlSpec{ornl_check, 0, false, false, 0}; }
static NlSpec nl_three(int width) { return NlSpec{nl3_check, width, true, false, 0}; }
static NlSpec nl_looks(int width, int closing) { return NlSpec{dl_descent_check, width, true, true, closing}; }

// what stands in front of the device and the family's check: the forms with looks refuse a width out of range; the width is kept
static int nl_admit(tspgpu_ctx *ctx, const NlSpec &S)
{
    if (S.looks && (S.width < 0 || S.width > NL_KMAX))
        return fail(ctx, E_INVALID, "the descent with looks takes a width of 0 to %d list entries, got %d", NL_KMAX, S.width);
    if (S.keep) ctx->nl3_width = S.width;
    return E_OK;
}

// The descent on a slot: descent::alternate over m2_run, every phase without a cap.  The counters of "Neighbour-list Or-opt"
// hold the totals; those of "Neighbour-list 3-opt" too where the descent has the phase (with looks and no phase the sweep
// counters are 0 and the phase count stands).  Counters and `out` are written whatever the answer
static int nl_descent(tspgpu_ctx *ctx, int slot, const NlSpec &S, double time_left_s, const DescentOut &out, bool *late)
{
    static const M2Family *const family[3] = {&M2_NL, &M2_ORNL, &M2_NL3};
    const double t_end = deadline_of(time_left_s);
    const int w3 = S.w3(ctx);
    Descent D;
    descent::Peaks P;
    DlCount total;
    if (S.looks) ctx->nl3_count = M2Counters{};
    const int rc = descent::alternate(
        w3,
        [&](descent::Family f, long *sweeps, long *moves, bool *phase_late) {
            DlCount dl;
            const M2Looks lk{S.closing, &dl};
            const int e = m2_run(ctx, slot, -1, t_end, sweeps, moves, phase_late, *family[f], S.looks ? &lk : nullptr);
            if (!e) total += dl;
            return e;
        },
        [&](descent::Family f) { return (ctx->*family[f]->count).max_k; }, &D, &P, late);
    ctx->ornl_count = M2Counters{D.os, D.om, P.k[descent::OR_OPT]}; ctx->ornl_rounds = D.nr;
    if (w3) { ctx->nl3_count = M2Counters{D.hs, D.hm, P.k[descent::THREE_OPT]}; ctx->nl3_phases = D.np; }
    if (S.looks) { D.lk = total.looked; D.lf = total.full; dl_record(ctx, total); }
    descent_out(&D, 1, out);
    return rc;
}

// ... of a host tour
static int nl_search_host(tspgpu_ctx *ctx, const NlSpec &S, int *path, double *cost, double time_left_s, const DescentOut &out)
{
    if (!path || !cost) return fail(ctx, E_INVALID, "null argument");
    const int rc = nl_admit(ctx, S);
    if (rc) return rc;
    return with_host_tour(ctx, path, cost, false, S.check, [&](bool *late) { return nl_descent(ctx, 0, S, time_left_s, out, late); });
}

// ... of the tour in a slot; with looks from the slot's awake sets as they stand
static int nl_search_slot(tspgpu_ctx *ctx, const NlSpec &S, int slot, double time_left_s, const DescentOut &out)
{
    const int rc = nl_admit(ctx, S);
    if (rc) return rc;
    return with_slot(ctx, slot, S.check, [&](bool *late) { return nl_descent(ctx, slot, S, time_left_s, out, late); }, S.looks);
}

static int kick_check(tspgpu_ctx *ctx)
{
    const int rc = need_costs(ctx);
    if (rc) return rc;
    if (ctx->n < 8) return fail(ctx, E_INVALID, "a kick needs at least 8 nodes, got %d", ctx->n);
    if (!ctx->symmetric) return fail(ctx, E_PRECOND, "a kick needs a symmetric cost matrix");
    return E_OK;
}

// the slot entry points of the awake sets: a context, costs, a tour in the slot
static int look_slot_check(tspgpu_ctx *ctx) { return need_costs(ctx); }

extern "C" {

int tspgpu_tour_wake(tspgpu_ctx *ctx, int slot, const int *nodes, int count)
{
    if (!ctx) return E_UNAVAILABLE;
    if (count > 0 && !nodes) return fail(ctx, E_INVALID, "null argument");
    return with_slot(ctx, slot, look_slot_check, [&](bool *) {
        for (int x = 0; x < count; x++)
            if (nodes[x] < 0 || nodes[x] >= ctx->n) return fail(ctx, E_INVALID, "node %d outside 0 .. %d: nothing was changed", nodes[x], ctx->n - 1);
        LookBuf K;
        int rc = look_buf(ctx, slot, count >= 0, &K);
        if (rc) return rc;
        if (count < 0) { wake_slots(ctx, slot, 1); return (int)E_OK; }
        if (count == 0) return (int)E_OK;
        DevBuf<int> d_nodes;
        HIP_TRY(d_nodes.alloc((size_t)count));
        HIP_TRY(hipMemcpyAsync(d_nodes, nodes, (size_t)count * 4, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_look_set, dim3((unsigned)std::min(256, (count + 255) / 256)), dim3(256), 0, ctx->stream, K.awake, ctx->n,
                           (const int *)d_nodes, count);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(ctx->stream));     // (d_nodes and the caller's array are free again)
        return (int)E_OK;
    }, true);
}

int tspgpu_tour_sleep(tspgpu_ctx *ctx, int slot)
{
    if (!ctx) return E_UNAVAILABLE;
    return with_slot(ctx, slot, look_slot_check, [&](bool *) {
        LookBuf K;
        const int rc = look_buf(ctx, slot, false, &K);
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(K.awake, 0, 3 * (size_t)ctx->n, ctx->stream));
        ctx->look_all[slot] = 0;
        return (int)E_OK;
    }, true);
}

int tspgpu_tour_awake(tspgpu_ctx *ctx, int slot, int family, unsigned char *out, int *count)
{
    if (!ctx) return E_UNAVAILABLE;
    if (family < 0 || family > 2) return fail(ctx, E_INVALID, "family %d: 0 the 2-opt, 1 Or-opt, 2 the 3-opt", family);
    return with_slot(ctx, slot, look_slot_check, [&](bool *) {
        LookBuf K;
        const int rc = look_buf(ctx, slot, false, &K);
        if (rc) return rc;
        const size_t n = (size_t)ctx->n;
        std::vector<unsigned char> h(n, 1);
        if (!ctx->look_all[slot]) {
            HIP_TRY(hipMemcpyAsync(h.data(), K.awake + (size_t)family * n, n, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
        }
        int c = 0;
        for (size_t v = 0; v < n; v++) { c += h[v] != 0; if (out) out[v] = h[v] != 0; }
        if (count) *count = c;
        return (int)E_OK;
    }, true);
}

int tspgpu_tour_kick(tspgpu_ctx *ctx, int slot, int i, int j, int k)
{
    if (!ctx) return E_UNAVAILABLE;
    return with_slot(ctx, slot, kick_check, [&](bool *) {
        if (!(0 <= i && i < j && j < k && k <= ctx->n - 1))
            return fail(ctx, E_INVALID, "a kick takes edge positions 0 <= i < j < k <= n - 1, got %d, %d, %d (n = %d)", i, j, k, ctx->n);
        LookBuf K;
        const int rc = look_buf(ctx, slot, false, &K);
        if (rc) return rc;
        unsigned char *awake = ctx->look_all[slot] ? nullptr : K.awake;    // (all awake: the six nodes are awake already)
        LAUNCH_BY_COST(k_tour_kick, dim3(1), dim3(256), slot, i, j, k, awake);
        HIP_TRY(hipGetLastError());
        return (int)E_OK;
    }, true);
}

int tspgpu_tour_two_opt_nl_dl(tspgpu_ctx *ctx, int slot, int closing, long max_sweeps, double time_left_s, long *sweeps, long *moves, long *looked)
{
    if (!ctx) return E_UNAVAILABLE;
    return dl_phase(ctx, slot, closing, max_sweeps, time_left_s, sweeps, moves, looked, M2_NL);
}

int tspgpu_tour_or_opt_nl_dl(tspgpu_ctx *ctx, int slot, int closing, long max_sweeps, double time_left_s, long *sweeps, long *moves, long *looked)
{
    if (!ctx) return E_UNAVAILABLE;
    return dl_phase(ctx, slot, closing, max_sweeps, time_left_s, sweeps, moves, looked, M2_ORNL);
}

int tspgpu_tour_three_opt_nl_dl(tspgpu_ctx *ctx, int slot, int width, int closing, long max_sweeps, double time_left_s, long *sweeps, long *moves,
                                long *looked)
{
    if (!ctx) return E_UNAVAILABLE;
    ctx->nl3_width = width;
    return dl_phase(ctx, slot, closing, max_sweeps, time_left_s, sweeps, moves, looked, M2_NL3);
}

int tspgpu_tour_local_search_nl3_dl(tspgpu_ctx *ctx, int slot, int width, int closing, double time_left_s, long *two_opt_sweeps, long *two_opt_moves,
                                    long *or_sweeps, long *or_moves, int *rounds, long *three_sweeps, long *three_moves, int *three_phases,
                                    long *looked, long *full_sweeps)
{
    if (!ctx) return E_UNAVAILABLE;
    return nl_search_slot(ctx, nl_looks(width, closing), slot, time_left_s,
                          DescentOut{two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, rounds, three_sweeps, three_moves, three_phases, looked,
                                     full_sweeps});
}

int tspgpu_local_search_nl3_dl(tspgpu_ctx *ctx, int width, int closing, int *path, double *cost, double time_left_s, long *two_opt_sweeps,
                               long *two_opt_moves, long *or_sweeps, long *or_moves, int *rounds, long *three_sweeps, long *three_moves,
                               int *three_phases, long *looked, long *full_sweeps)
{
    if (!ctx) return E_UNAVAILABLE;
    return nl_search_host(ctx, nl_looks(width, closing), path, cost, time_left_s,
                          DescentOut{two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, rounds, three_sweeps, three_moves, three_phases, looked,
                                     full_sweeps});
}

int tspgpu_local_search_nl(tspgpu_ctx *ctx, int *path, double *cost, double time_left_s, long *two_opt_sweeps, long *two_opt_moves,
                           long *or_sweeps, long *or_moves, int *rounds)
{
    if (!ctx) return E_UNAVAILABLE;
    return nl_search_host(ctx, nl_plain(), path, cost, time_left_s, DescentOut{two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, rounds});
}

int tspgpu_tour_local_search_nl(tspgpu_ctx *ctx, int slot, double time_left_s, long *two_opt_sweeps, long *two_opt_moves,
                                long *or_sweeps, long *or_moves, int *rounds)
{
    if (!ctx) return E_UNAVAILABLE;
    return nl_search_slot(ctx, nl_plain(), slot, time_left_s, DescentOut{two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, rounds});
}

int tspgpu_local_search_nl3(tspgpu_ctx *ctx, int width, int *path, double *cost, double time_left_s, long *two_opt_sweeps, long *two_opt_moves,
                            long *or_sweeps, long *or_moves, int *rounds, long *three_sweeps, long *three_moves, int *three_phases)
{
    if (!ctx) return E_UNAVAILABLE;
    return nl_search_host(ctx, nl_three(width), path, cost, time_left_s,
                          DescentOut{two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, rounds, three_sweeps, three_moves, three_phases});
}

int tspgpu_tour_local_search_nl3(tspgpu_ctx *ctx, int slot, int width, double time_left_s, long *two_opt_sweeps, long *two_opt_moves,
                                 long *or_sweeps, long *or_moves, int *rounds, long *three_sweeps, long *three_moves, int *three_phases)
{
    if (!ctx) return E_UNAVAILABLE;
    return nl_search_slot(ctx, nl_three(width), slot, time_left_s,
                          DescentOut{two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, rounds, three_sweeps, three_moves, three_phases});
}

} // extern "C"

// ---- greedy-edge construction over the neighbour lists (tspgpu_greedy.inc) ---------------------------------------------------

// the preconditions of "Neighbour-list 2-opt" without its row-in-LDS limit: no kernel here holds a matrix row
static int greedy_check(tspgpu_ctx *ctx)
{
    const int rc = need_costs(ctx);
    if (rc) return rc;
    if (ctx->n < 5) return fail(ctx, E_INVALID, "the greedy-edge construction needs at least 5 nodes, got %d", ctx->n);
    if (!ctx->symmetric) return fail(ctx, E_PRECOND, "the greedy-edge construction needs a symmetric cost matrix");
    if (!ctx->nl.K)
        return fail(ctx, E_PRECOND, ctx->nl_dropped ? "the neighbour lists were invalidated by a new cost source: call tspgpu_neighbours_build again"
                                                    : "no neighbour lists: call tspgpu_neighbours_build first");
    return E_OK;
}

// rounds of one phase in batches of GE_ROUNDS_PER_LOOK behind one another on the stream; the host reads the control block per
// batch.  A phase has at most n - 1 rounds that accept an edge and one that does not
constexpr int GE_ROUNDS_PER_LOOK = 16;

template <typename R> static int greedy_phase(tspgpu_ctx *ctx, int ph, GeCtl *C, R &&round)
{
    int r = 0;
    const looks::Result res = looks::drive(
        now_s, -1.0, GE_ROUNDS_PER_LOOK,
        [&]() -> int {
            const int rc = round(r);
            r++;
            return rc;
        },
        [&]() -> int {
            const int rc = ctl_get(ctx, C, (const GeCtl *)ctx->ge.ctl);
            if (rc) return rc;
            if (C->done[ph]) return (int)looks::STOP;
            if (r > ctx->n + GE_ROUNDS_PER_LOOK) return fail(ctx, E_INTERNAL, "greedy-edge phase %d did not end within %d rounds", ph + 1, r);
            return (int)looks::GO_ON;
        });
    return res.code;
}

// the greedy-edge tour of the cost source in place into `slot` (checked, and the slot array grown, by the caller)
static int greedy_build(tspgpu_ctx *ctx, int slot)
{
    const int n = ctx->n;
    if (!ctx->ge.ctl) HIP_TRY(tspmem::grow(HipMem{ctx->stream}, ctx->ge_rows((size_t)n), 0, 1));
    const GeBuf G = ctx->ge;
    const NlBuf L = ctx->nl;
    const dim3 nodes((n + GE_BT - 1) / GE_BT), darts((2 * n + GE_BT - 1) / GE_BT), block(GE_BT);
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemsetAsync(G.ctl, 0, sizeof(GeCtl), st));
    hipLaunchKernelGGL(k_ge_init, nodes, block, 0, st, G, n);
    HIP_TRY(hipGetLastError());
    GeCtl C;
    memset(&C, 0, sizeof C);
    const bool f64 = ctx->elem == TSPGPU_ELEM_F64;
    int rc = greedy_phase(ctx, 0, &C, [&](int r) -> int {
        if (f64) {
            hipLaunchKernelGGL((k_ge_p1<double, 0>), nodes, block, 0, st, G, L, n);
            hipLaunchKernelGGL((k_ge_p1<double, 1>), nodes, block, 0, st, G, L, n);
        } else {
            hipLaunchKernelGGL((k_ge_p1<int, 0>), nodes, block, 0, st, G, L, n);
            hipLaunchKernelGGL((k_ge_p1<int, 1>), nodes, block, 0, st, G, L, n);
        }
        hipLaunchKernelGGL(k_ge_accept, nodes, block, 0, st, G, n, 0, r & 1);
        hipLaunchKernelGGL(k_ge_link, nodes, block, 0, st, G, n, 0, r);
        HIP_TRY(hipGetLastError());
        return E_OK;
    });
    if (rc) return rc;
    const dim3 scan((unsigned)std::max(1, std::min((n + 3) / 4, 4 * ctx->cus)));    // a wave per free node, striding
    rc = greedy_phase(ctx, 1, &C, [&](int r) -> int {
        hipLaunchKernelGGL(k_ge_p2_compact, nodes, block, 0, st, G, n, r & 1);
        ELEM_SWITCH(ctx->elem, T, hipLaunchKernelGGL((k_ge_p2_best<T>), scan, block, 0, st, G, (const T *)ctx->d_mat.p, ctx->d_pts, ctx->kind,
                                                     ctx->ld, n, r & 1));
        hipLaunchKernelGGL(k_ge_accept, nodes, block, 0, st, G, n, 1, r & 1);
        hipLaunchKernelGGL(k_ge_link, nodes, block, 0, st, G, n, 1, r);
        HIP_TRY(hipGetLastError());
        return E_OK;
    });
    if (rc) return rc;
    if (C.edges[0] + C.edges[1] != (unsigned)(n - 1))
        return fail(ctx, E_INTERNAL, "the greedy-edge construction ended with %u edges of %d", C.edges[0] + C.edges[1], n - 1);
    ctx->ge_rounds1 = C.rounds[0]; ctx->ge_rounds2 = C.rounds[1]; ctx->ge_edges1 = C.edges[0]; ctx->ge_free = C.free_in;
    // the order: close the path, rank the darts (ceil(log2 n) jumps between the two halves of the rank buffers), write ord[]
    hipLaunchKernelGGL(k_ge_close, nodes, block, 0, st, G, n);
    hipLaunchKernelGGL(k_ge_rank_init, darts, block, 0, st, G, n);
    int cur = 0;
    for (int reach = 1; reach < n; reach *= 2, cur ^= 1)
        hipLaunchKernelGGL(k_ge_rank_jump, darts, block, 0, st, G.nxt + (size_t)cur * 2 * n, G.dist + (size_t)cur * 2 * n,
                           G.nxt + (size_t)(cur ^ 1) * 2 * n, G.dist + (size_t)(cur ^ 1) * 2 * n, 2 * n);
    hipLaunchKernelGGL(k_ge_rank_out, darts, block, 0, st, G, G.nxt + (size_t)cur * 2 * n, G.dist + (size_t)cur * 2 * n, ctx->S, slot, n);
    HIP_TRY(hipGetLastError());
    if ((rc = init_slots(ctx, slot, 1, -1))) return rc;
    mark_slots(ctx, slot, 1, true);
    return E_OK;
}

extern "C" {

int tspgpu_tour_greedy(tspgpu_ctx *ctx, int slot)
{
    if (!ctx) return E_UNAVAILABLE;
    if (slot < 0) return fail(ctx, E_INVALID, "bad slot %d", slot);
    hipSetDevice(ctx->device);
    int rc = greedy_check(ctx);
    if (rc) return rc;
    if ((rc = ensure_tours(ctx, slot + 1))) return rc;
    return greedy_build(ctx, slot);
}

int tspgpu_greedy_tour(tspgpu_ctx *ctx, int *path, double *cost)
{
    if (!ctx) return E_UNAVAILABLE;
    if (!path || !cost) return fail(ctx, E_INVALID, "null argument");
    hipSetDevice(ctx->device);
    int rc = greedy_check(ctx);
    if (rc) return rc;
    if ((rc = ensure_tours(ctx, 1))) return rc;
    if ((rc = greedy_build(ctx, 0))) return rc;
    return store_path(ctx, 0, path, cost, nullptr);
}

} // extern "C"

// ---- Held-Karp lower bound (tspgpu_hk.inc) ---------------------------------------------------------------------------------

static int hk_check(tspgpu_ctx *ctx)
{
    const int rc = need_costs(ctx);
    if (rc) return rc;
    if (ctx->n < 5) return fail(ctx, E_INVALID, "the Held-Karp bound needs at least 5 nodes, got %d", ctx->n);
    if (!ctx->symmetric) return fail(ctx, E_PRECOND, "the Held-Karp bound needs a symmetric cost matrix");
    if (!ctx->otf && ctx->elem == TSPGPU_ELEM_F64) return fail(ctx, E_UNIMPL, "the Held-Karp bound needs integer costs (uint16 / int32 cells or matrix-free mode), not f64 cells");
    return E_OK;
}

static int hk_pi_check(tspgpu_ctx *ctx, const long *pi)
{
    if (pi)
        for (int v = 0; v < ctx->n; v++)
            if (pi[v] > HK_PI_MAX || pi[v] < -HK_PI_MAX) return fail(ctx, E_INVALID, "multiplier %d is %ld: at most 2^45 in magnitude", v, pi[v]);
    return E_OK;
}

// the state (all or none) and the multipliers in place: pi, or zeros
static int hk_begin(tspgpu_ctx *ctx, const long *pi)
{
    const size_t n = (size_t)ctx->n;
    if (!ctx->hk.ctl) {
        const Rows rows = ctx->hk_rows(n);
        const hipError_t e = tspmem::grow(HipMem{ctx->stream}, rows, 0, 1);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(ctx, E_EXHAUSTED, "the Held-Karp bound needs %zu bytes of device memory for %d nodes (%s)", tspmem::rows_bytes(rows, 1), ctx->n,
                        hipGetErrorString(e));
        }
    }
    static_assert(sizeof(long) == sizeof(long long), "the ABI's long is 64 bits");
    if (pi) HIP_TRY(hipMemcpyAsync(ctx->hk.pi, pi, n * 8, hipMemcpyHostToDevice, ctx->stream));
    else HIP_TRY(hipMemsetAsync(ctx->hk.pi, 0, n * 8, ctx->stream));
    return E_OK;
}

static int hk_rounds_max(int n)
{
    int r = 0;
    while ((1 << r) < n - 1) r++;
    return std::max(r, 1);
}

// one 1-tree of the multipliers in place, enqueued: init, node 0's edges, the maximal number of rounds
static int hk_enqueue_tree(tspgpu_ctx *ctx)
{
    const int n = ctx->n, ld = ctx->ld;
    const HkBuf H = ctx->hk;
    hipStream_t st = ctx->stream;
    const dim3 nodes((n + HK_BT - 1) / HK_BT), block(HK_BT), rows((n - 1 + HK_ROWS - 1) / HK_ROWS), wave_rows(HK_ROWS * 64);
    const bool stage = (size_t)12 * ld <= 65536;
    const size_t lds = stage ? (size_t)12 * ld : 0;
    const bool i32 = ctx->elem == TSPGPU_ELEM_I32;
    ctx->hk_lds = (long)lds;
    hipLaunchKernelGGL(k_hk_init, nodes, block, 0, st, H, n);
    if (ctx->otf) kind_switch(ctx, [&](auto kind, auto *pts, auto *) { hipLaunchKernelGGL((k_hk_zero_otf<kind()>), dim3(1), block, 0, st, H, pts, n); });
    else if (i32) hipLaunchKernelGGL((k_hk_zero<int>), dim3(1), block, 0, st, H, (const int *)ctx->d_mat.p, n, ld);
    else hipLaunchKernelGGL((k_hk_zero<u16>), dim3(1), block, 0, st, H, (const u16 *)ctx->d_mat.p, n, ld);
    for (int r = 0, R = hk_rounds_max(n); r < R; r++) {
        if (ctx->otf)
            kind_switch(ctx, [&](auto kind, auto *pts, auto *) {
                if (stage) hipLaunchKernelGGL((k_hk_scan_otf<kind(), true>), rows, wave_rows, lds, st, H, pts, n, ld);
                else hipLaunchKernelGGL((k_hk_scan_otf<kind(), false>), rows, wave_rows, 0, st, H, pts, n, ld);
            });
        else if (i32) {
            if (stage) hipLaunchKernelGGL((k_hk_scan<int, true>), rows, wave_rows, lds, st, H, (const int *)ctx->d_mat.p, n, ld);
            else hipLaunchKernelGGL((k_hk_scan<int, false>), rows, wave_rows, 0, st, H, (const int *)ctx->d_mat.p, n, ld);
        } else {
            if (stage) hipLaunchKernelGGL((k_hk_scan<u16, true>), rows, wave_rows, lds, st, H, (const u16 *)ctx->d_mat.p, n, ld);
            else hipLaunchKernelGGL((k_hk_scan<u16, false>), rows, wave_rows, 0, st, H, (const u16 *)ctx->d_mat.p, n, ld);
        }
        hipLaunchKernelGGL(k_hk_cmin, nodes, block, 0, st, H, n);
        hipLaunchKernelGGL(k_hk_hook, nodes, block, 0, st, H, n);
        hipLaunchKernelGGL(k_hk_flat, nodes, block, 0, st, H, n);
    }
    HIP_TRY(hipGetLastError());
    return E_OK;
}

static long long hk_ceil_div(long long x) { return x >= 0 ? (x + HK_S - 1) / HK_S : -((-x) / HK_S); }

// the tree's edges from the device, ascending by pair
static int hk_fetch_edges(tspgpu_ctx *ctx, std::vector<u64> &e)
{
    e.resize((size_t)ctx->n);
    HIP_TRY(hipMemcpyAsync(e.data(), ctx->hk.edges, e.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::sort(e.begin(), e.end());
    for (const u64 x : e)
        if ((unsigned)(x >> 32) >= (unsigned)x || (unsigned)x >= (unsigned)ctx->n) return fail(ctx, E_INTERNAL, "the 1-tree holds an edge that is none");
    return E_OK;
}

extern "C" {

int tspgpu_one_tree(tspgpu_ctx *ctx, const long *pi, int *edges, int *degree, long *weight)
{
    if (!ctx) return E_UNAVAILABLE;
    if (!weight) return fail(ctx, E_INVALID, "null argument");
    hipSetDevice(ctx->device);
    int rc = hk_check(ctx);
    if (rc || (rc = hk_pi_check(ctx, pi)) || (rc = hk_begin(ctx, pi))) return rc;
    const int n = ctx->n;
    HkCtl C;
    memset(&C, 0, sizeof C);
    HIP_TRY(hipMemcpyAsync(ctx->hk.ctl, &C, sizeof C, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = hk_enqueue_tree(ctx)) || (rc = ctl_get(ctx, &C, (const HkCtl *)ctx->hk.ctl))) return rc;
    if (!C.done || C.err || C.nedges != (unsigned)(n - 2))
        return fail(ctx, E_INTERNAL, "the 1-tree ended with %u tree edges of %d (%d rounds)", C.nedges, n - 2, C.rounds);
    ctx->hk_rounds = C.rounds;
    long long spi = 0;
    if (pi) for (int v = 0; v < n; v++) spi += pi[v];
    if (edges) {
        std::vector<u64> e;
        if ((rc = hk_fetch_edges(ctx, e))) return rc;
        for (int k = 0; k < n; k++) { edges[2 * k] = (int)(e[k] >> 32); edges[2 * k + 1] = (int)(unsigned)e[k]; }
    }
    if (degree) HIP_TRY(hipMemcpy(degree, ctx->hk.deg, (size_t)n * 4, hipMemcpyDeviceToHost));
    *weight = (long)(C.wsum - 2 * spi);
    return E_OK;
}

int tspgpu_lower_bound(tspgpu_ctx *ctx, double upper, int iters, int patience, double time_left_s, const long *pi_in, double *bound,
                       long *pi_out, int *path, int *iters_done, int *reason)
{
    if (!ctx) return E_UNAVAILABLE;
    if (!bound || !iters_done || !reason) return fail(ctx, E_INVALID, "null argument");
    hipSetDevice(ctx->device);
    int rc = hk_check(ctx);
    if (rc) return rc;
    if (!(upper >= 0) || upper != std::floor(upper) || !(upper * (double)HK_S < 1099511627776.0))
        return fail(ctx, E_INVALID, "the upper bound %g is not an integer in [0, 2^40 / 128)", upper);
    if (iters < 1 || patience < 1) return fail(ctx, E_INVALID, "iters = %d, patience = %d: both at least 1", iters, patience);
    if ((rc = hk_pi_check(ctx, pi_in)) || (rc = hk_begin(ctx, pi_in))) return rc;
    const int n = ctx->n;
    const double t_end = deadline_of(time_left_s);
    HkCtl C;
    memset(&C, 0, sizeof C);
    C.ubs = HK_S * (long long)upper; C.patience = patience;
    HIP_TRY(hipMemcpyAsync(ctx->hk.ctl, &C, sizeof C, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->hk.pibest, ctx->hk.pi, (size_t)n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    // batches of TSPGPU_OPT_BATCH iterations behind one another on the stream; the host looks at the control block per batch
    const int batch = std::max(1, ctx->opt_batch);
    bool late = false;
    for (int queued = 0; queued < iters && !C.stop && !late;) {
        const int k = std::min(batch, iters - queued);
        for (int i = 0; i < k; i++) {
            if ((rc = hk_enqueue_tree(ctx))) return rc;
            hipLaunchKernelGGL(k_hk_step, dim3(1), dim3(HK_STEP_BT), 0, ctx->stream, ctx->hk, n);
        }
        HIP_TRY(hipGetLastError());
        queued += k;
        if ((rc = ctl_get(ctx, &C, (const HkCtl *)ctx->hk.ctl))) return rc;
        late = t_end >= 0 && queued < iters && !C.stop && now_s() >= t_end;
    }
    if (C.stop == 7 || !C.have_best) return fail(ctx, E_INTERNAL, "a 1-tree of the ascent did not complete (iteration %d, %u tree edges of %d)", C.iters, C.nedges, n - 2);
    const int why = C.stop ? C.stop - 1 : late ? 4 : 0;
    ctx->hk_rounds = C.rounds; ctx->hk_iters = C.iters; ctx->hk_reason = why; ctx->hk_h = C.h;
    if (why == 1 && path) {                 // the tree in hand is a tour: from node 0 towards its smaller neighbour
        std::vector<u64> e;
        if ((rc = hk_fetch_edges(ctx, e))) return rc;
        std::vector<int> adj(2 * (size_t)n, -1), cnt((size_t)n, 0);
        for (const u64 x : e) {
            const int a = (int)(x >> 32), b = (int)(unsigned)x;
            if (cnt[a] >= 2 || cnt[b] >= 2) return fail(ctx, E_INTERNAL, "the 1-tree of reason 1 is no tour");
            adj[2 * a + cnt[a]++] = b; adj[2 * b + cnt[b]++] = a;
        }
        std::vector<int> succ((size_t)n, -1);
        int prev = 0, v = std::min(adj[0], adj[1]);
        succ[0] = v;
        for (int k = 1; k < n; k++) {
            const int next = adj[2 * v] == prev ? adj[2 * v + 1] : adj[2 * v];
            if ((unsigned)next >= (unsigned)n || succ[v] >= 0) return fail(ctx, E_INTERNAL, "the 1-tree of reason 1 is no tour");
            succ[v] = next; prev = v; v = next;
        }
        if (v != 0) return fail(ctx, E_INTERNAL, "the 1-tree of reason 1 is no tour");
        memcpy(path, succ.data(), (size_t)n * sizeof(int));
    }
    if (pi_out) HIP_TRY(hipMemcpy(pi_out, ctx->hk.pibest, (size_t)n * 8, hipMemcpyDeviceToHost));
    *bound = (double)hk_ceil_div(C.best);
    *iters_done = C.iters; *reason = why;
    return done_code(why == 4);
}

} // extern "C"

// ---- batched neighbour-list descent (tspgpu_nlbatch.inc) ---------------------------------------------------------------

// the candidate arrays (40 bytes per node and slot) and a control block per slot for a range of `count` slots
static int nlb_ensure(tspgpu_ctx *ctx, int count)
{
    if (count <= ctx->nlb_cap) return E_OK;
    ctx->drop_nlb();
    const Rows rows = ctx->nlb_rows((size_t)ctx->n);
    const size_t total = tspmem::rows_bytes(rows, (size_t)count);
    const hipError_t e = tspmem::grow(HipMem{ctx->stream}, rows, 0, (size_t)count);
    if (e != hipSuccess) {                  // all or none: a later call must not find half of them
        (void)hipGetLastError();
        return fail(ctx, E_EXHAUSTED, "the batched neighbour-list descent needs %zu bytes of device memory for %d tours of %d nodes (%s)",
                    total, count, ctx->n, hipGetErrorString(e));
    }
    ctx->nlb_cap = count;
    return E_OK;
}

// the memory of a batched descent with looks (NlbMode) beyond nlb_ensure's: the slots' sets (ensure_looks), and a queue of n nodes and a look block per slot of the range
static int nlbq_ensure(tspgpu_ctx *ctx, int count)
{
    int rc = ensure_looks(ctx);
    if (rc) return rc;
    if (count <= ctx->nlbq_cap) return E_OK;
    ctx->drop_nlbq();
    const Rows rows = ctx->nlbq_rows((size_t)ctx->n);
    const hipError_t e = tspmem::grow(HipMem{ctx->stream}, rows, 0, (size_t)count);
    if (e != hipSuccess) {                  // all or none
        (void)hipGetLastError();
        return fail(ctx, E_EXHAUSTED, "the batched descent with don't-look bits needs %zu bytes of device memory for the queues of %d tours of %d nodes (%s)",
                    tspmem::rows_bytes(rows, (size_t)count), count, ctx->n, hipGetErrorString(e));
    }
    ctx->nlbq_cap = count;
    return E_OK;
}

// the sets of the slots slot0 .. slot0 + count - 1 as the device arrays: flagged slots ("every node is awake") are filled
static int nlb_fill_flagged(tspgpu_ctx *ctx, int slot0, int count)
{
    const size_t bytes = 3 * (size_t)ctx->n;
    for (int i = slot0; i < slot0 + count;) {
        if (!ctx->look_all[i]) { i++; continue; }
        int j = i;
        while (j < slot0 + count && ctx->look_all[j]) ctx->look_all[j++] = 0;
        HIP_TRY(hipMemsetAsync(ctx->d_awake + (size_t)i * bytes, 1, (size_t)(j - i) * bytes, ctx->stream));
        i = j;
    }
    return E_OK;
}

// one sweep of every tour of the first `live` slots of the list: the four launches (six with looks: the queue pass in front
// of the sweep, the wake pass in front of the apply), grid rows in runs of at most 65 535.
// THREE: the instantiations with the 3-opt phase, at width w3
template <bool THREE>
static int nlb_launch_sweep_as(tspgpu_ctx *ctx, int slot0, int live, int w3, const NlbMode &M)
{
    const int n = ctx->n, W = (n + ORNL_STARTS - 1) / ORNL_STARTS, G = std::min(NLB_APPLY_WGS, (n + 1) / 2);
    NlbCtl *ctl = ctx->d_nlb_ctl;
    const NlbLooks Q{ctx->d_awake, ctx->d_nlb_queue, ctx->d_nlb_look, M.closing};
    const int run = std::max(1, std::min(65535, (1 << 23) / W));    // (a grid holds fewer than 2^32 threads)
    for (int off = 0; off < live; off += run) {
        const unsigned rows = (unsigned)std::min(run, live - off);
        const int *list = ctx->d_live + off;
        if (M.looks) {
            const int QW = std::min(NLB_QSWEEP_WGS, W);
            hipLaunchKernelGGL(k_nlb_queue<THREE>, dim3(rows), dim3(1024), 0, ctx->stream, ctx->S, n, list, slot0, ctx->nlb, ctl, Q);
            HIP_TRY(hipGetLastError());
            if (ctx->otf)
                kind_switch(ctx, [&](auto kind, auto *pts, auto *) {
                    hipLaunchKernelGGL((k_nlb_qsweep_otf<kind(), THREE>), dim3(QW, rows), dim3(256), 0, ctx->stream, ctx->S, pts, n, list, slot0,
                                       ctx->nl, ctx->nlb, (const NlbCtl *)ctl, w3, Q);
                });
            else
                ELEM_SWITCH(ctx->elem, T, hipLaunchKernelGGL((k_nlb_qsweep<T, THREE>), dim3(QW, rows), dim3(256), 0, ctx->stream, ctx->S,
                                                             (const T *)ctx->d_mat.p, n, ctx->ld, list, slot0, ctx->nl, ctx->nlb,
                                                             (const NlbCtl *)ctl, w3, Q));
        } else if (ctx->otf)
            kind_switch(ctx, [&](auto kind, auto *pts, auto *) {
                hipLaunchKernelGGL((k_nlb_sweep_otf<kind(), THREE>), dim3(W, rows), dim3(256), 0, ctx->stream, ctx->S, pts, n, list, slot0, ctx->nl,
                                   ctx->nlb, (const NlbCtl *)ctl, w3);
            });
        else
            ELEM_SWITCH(ctx->elem, T, hipLaunchKernelGGL((k_nlb_sweep<T, THREE>), dim3(W, rows), dim3(256), 0, ctx->stream, ctx->S,
                                                         (const T *)ctx->d_mat.p, n, ctx->ld, list, slot0, ctx->nl, ctx->nlb, (const NlbCtl *)ctl, w3));
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_nlb_compact<THREE>, dim3(1, rows), dim3(1024), 0, ctx->stream, ctx->S, n, list, slot0, ctx->nlb, ctl, ctx->nl);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_nlb_select, dim3((n + 255) / 256, rows), dim3(256), 0, ctx->stream, n, list, slot0, ctx->nlb, (const NlbCtl *)ctl);
        HIP_TRY(hipGetLastError());
        if (M.looks) {
            hipLaunchKernelGGL(k_nlb_wake<THREE>, dim3(NLB_WAKE_WGS, rows), dim3(256), 0, ctx->stream, ctx->S, n, list, slot0, ctx->nl, ctx->nlb,
                               (const NlbCtl *)ctl, Q);
            HIP_TRY(hipGetLastError());
            if (ctx->otf)
                kind_switch(ctx, [&](auto kind, auto *pts, auto *) {
                    hipLaunchKernelGGL((k_nlb_apply_dl_otf<kind(), THREE>), dim3(G, rows), dim3(256), 0, ctx->stream, ctx->S, pts, n, list, slot0,
                                       ctx->nlb, ctl, ctx->nl, Q);
                });
            else
                ELEM_SWITCH(ctx->elem, T, hipLaunchKernelGGL((k_nlb_apply_dl<T, THREE>), dim3(G, rows), dim3(256), 0, ctx->stream, ctx->S,
                                                             (const T *)ctx->d_mat.p, n, ctx->ld, list, slot0, ctx->nlb, ctl, ctx->nl, Q));
        } else if (ctx->otf)
            kind_switch(ctx, [&](auto kind, auto *pts, auto *) {
                hipLaunchKernelGGL((k_nlb_apply_otf<kind(), THREE>), dim3(G, rows), dim3(256), 0, ctx->stream, ctx->S, pts, n, list, slot0, ctx->nlb,
                                   ctl, ctx->nl);
            });
        else
            ELEM_SWITCH(ctx->elem, T, hipLaunchKernelGGL((k_nlb_apply<T, THREE>), dim3(G, rows), dim3(256), 0, ctx->stream, ctx->S,
                                                         (const T *)ctx->d_mat.p, n, ctx->ld, list, slot0, ctx->nlb, ctl, ctx->nl));
        HIP_TRY(hipGetLastError());
    }
    return E_OK;
}

// w3: the width of the 3-opt phase, 0: the descent has none
static int nlb_launch_sweep(tspgpu_ctx *ctx, int slot0, int live, int w3, const NlbMode &M = NlbMode{})
{
    return w3 > 0 ? nlb_launch_sweep_as<true>(ctx, slot0, live, w3, M) : nlb_launch_sweep_as<false>(ctx, slot0, live, 0, M);
}

// the look blocks of the first `count` places of a range into D (lk, lf) and the context's totals
static int nlb_looks_out(tspgpu_ctx *ctx, int count, Descent *D)
{
    std::vector<LookCtl> hl((size_t)count);
    const int rc = ctl_get(ctx, hl.data(), (const LookCtl *)ctx->d_nlb_look, (size_t)count);
    if (rc) return rc;
    ctx->nlb_dl_looked = ctx->nlb_dl_full = ctx->nlb_dl_max_q = 0;
    for (int i = 0; i < count; i++) {
        if (D) { D[i].lk = (long)hl[i].looked; D[i].lf = (long)hl[i].full; }
        ctx->nlb_dl_looked += (long)hl[i].looked; ctx->nlb_dl_full += (long)hl[i].full;
        ctx->nlb_dl_max_q = std::max(ctx->nlb_dl_max_q, (long)hl[i].max_q);
    }
    return E_OK;
}

// nl_descent's rule (w3 > 0: with the 3-opt phase at that width) on the slots slot0 .. slot0 + count - 1 at once.  The control blocks are
// armed (2-opt phase, round 1) and the slots re-armed as m2_arm does; then sweeps of all live tours -- four between looks at
// the control blocks, one under a deadline, as m2_run -- and the tours whose descent has ended leave the list.  D: per-slot
// counters, [count]
// M.looks: every phase is a phase with looks, from the slots' sets as they stand (flagged slots: every node awake)
static int nlb_descent(tspgpu_ctx *ctx, int slot0, int count, int w3, double time_left_s, Descent *D, bool *late, const NlbMode &M = NlbMode{})
{
    const double t_end = deadline_of(time_left_s);
    *late = false;
    ctx->nlb_tours = count; ctx->nlb_launches = 0; ctx->nlb_max_live = 0;
    ctx->nlb_w3 = w3; ctx->nlb_three_sweeps = ctx->nlb_three_moves = ctx->nlb_three_max_k = 0;
    int rc = nlb_ensure(ctx, count);
    if (rc) return rc;
    if (M.looks) {
        if ((rc = nlbq_ensure(ctx, count))) return rc;
        if ((rc = nlb_fill_flagged(ctx, slot0, count))) return rc;
        HIP_TRY(hipMemsetAsync(ctx->d_nlb_look, 0, (size_t)count * sizeof(LookCtl), ctx->stream));
    }
    std::vector<NlbCtl> hc((size_t)count);
    memset(hc.data(), 0, hc.size() * sizeof(NlbCtl));
    for (NlbCtl &c : hc) c.rounds = 1;
    HIP_TRY(hipMemcpyAsync(ctx->d_nlb_ctl, hc.data(), hc.size() * sizeof(NlbCtl), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_rearm, dim3((count + 255) / 256), dim3(256), 0, ctx->stream, ctx->S, slot0, count, -1);
    HIP_TRY(hipGetLastError());
    std::vector<int> live((size_t)count);
    for (int i = 0; i < count; i++) live[i] = slot0 + i;
    if ((rc = set_live(ctx, live))) return rc;
    const looks::Result r = looks::drive_live(
        now_s, t_end, 4, live, [](int) {},
        [&](int len) { const int e = nlb_launch_sweep(ctx, slot0, len, w3, M); ctx->nlb_launches += !e; return e; },
        [&] { return ctl_get(ctx, hc.data(), ctx->d_nlb_ctl, (size_t)count); }, [&](int t) { return hc[t - slot0].stop != 0; },
        [&](const std::vector<int> &list) { return set_live(ctx, list); });
    ctx->nlb_max_live = r.max_live;
    if (r.code) return r.code;
    *late = r.late;
    for (int i = 0; i < count; i++) {
        D[i].tw = (long)hc[i].two_opt_sweeps; D[i].tm = (long)hc[i].two_opt_moves;
        D[i].os = (long)hc[i].or_sweeps; D[i].om = (long)hc[i].or_moves; D[i].nr = hc[i].rounds;
        D[i].hs = (long)hc[i].three_sweeps; D[i].hm = (long)hc[i].three_moves; D[i].np = hc[i].three_phases;
        ctx->nlb_three_sweeps += D[i].hs; ctx->nlb_three_moves += D[i].hm;
        ctx->nlb_three_max_k = std::max(ctx->nlb_three_max_k, (long)hc[i].three_max_k);
    }
    if (M.looks && (rc = nlb_looks_out(ctx, count, D))) return rc;
    return E_OK;
}

// the range of a batched descent over the lists, behind the family's check: count slots from slot0, each with a tour
static int nlb_range(tspgpu_ctx *ctx, int slot0, int count, bool rewrites = true)
{
    if (slot0 < 0 || count <= 0 || count > ctx->tcap || slot0 > ctx->tcap - count)      // (the range first: a slot past the end is no slot without a tour)
        return fail(ctx, E_INVALID, "bad slot range: slot0 %d, count %d of %d slots", slot0, count, ctx->tcap);
    return or_batch_args(ctx, slot0, count, rewrites);
}

static int nlb_no_cap(tspgpu_ctx *ctx)
{
    if (ctx->opt_sweep_cap != -1)
        return fail(ctx, E_INVALID, "TSPGPU_OPT_SWEEP_CAP = %d: the descent over the neighbour lists runs every phase to its end", ctx->opt_sweep_cap);
    return E_OK;
}

// the batched descent on the slots slot0 .. slot0 + count - 1 (tspgpu_tours_local_search_nl, _nl3, _nl3_dl)
static int nl_search_tours(tspgpu_ctx *ctx, const NlSpec &S, int slot0, int count, double time_left_s, const DescentOut &out)
{
    int rc = nl_admit(ctx, S);
    if (rc) return rc;
    hipSetDevice(ctx->device);
    if ((rc = S.check(ctx))) return rc;
    if ((rc = nlb_range(ctx, slot0, count, !S.looks))) return rc;
    std::vector<Descent> D(count);
    bool late = false;
    if ((rc = nlb_descent(ctx, slot0, count, S.w3(ctx), time_left_s, D.data(), &late, S.mode()))) return rc;
    descent_out(D.data(), count, out);
    return done_code(late);
}

// the multi-start with it (tspgpu_multistart_local_search_nl, _nl3, _nl3_dl); total: sums over every start processed
static int nl_multistart(tspgpu_ctx *ctx, const NlSpec &S, const int *starts, int nstarts, double time_left_s, int *best_path, double *best_cost,
                         int *best_start, const DescentOut &total, double *costs_out)
{
    if (!best_path || !best_cost || !best_start || nstarts <= 0) return fail(ctx, E_INVALID, "bad argument");
    int rc = nl_admit(ctx, S);
    if (rc) return rc;
    hipSetDevice(ctx->device);
    if ((rc = S.check(ctx))) return rc;
    if ((rc = nlb_no_cap(ctx))) return rc;
    const int w3 = S.w3(ctx);
    MultiStart ms;
    rc = multistart(ctx, starts, nstarts, time_left_s, -1, best_path, best_cost, best_start, costs_out, &ms,
                    [&](int m, double left, bool *late, Descent *D) { return nlb_descent(ctx, 0, m, w3, left, D, late, S.mode()); });
    if (rc && rc != E_DEADLINE) return rc;
    descent_out(&ms.total, 1, total);
    return rc;
}

extern "C" {

int tspgpu_tours_local_search_nl(tspgpu_ctx *ctx, int slot0, int count, double time_left_s, long *two_opt_sweeps, long *two_opt_moves,
                                 long *or_sweeps, long *or_moves, int *rounds)
{
    if (!ctx) return E_UNAVAILABLE;
    return nl_search_tours(ctx, nl_plain(), slot0, count, time_left_s, DescentOut{two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, rounds});
}

int tspgpu_tours_local_search_nl3(tspgpu_ctx *ctx, int slot0, int count, int width, double time_left_s, long *two_opt_sweeps, long *two_opt_moves,
                                  long *or_sweeps, long *or_moves, int *rounds, long *three_sweeps, long *three_moves, int *three_phases)
{
    if (!ctx) return E_UNAVAILABLE;
    return nl_search_tours(ctx, nl_three(width), slot0, count, time_left_s,
                           DescentOut{two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, rounds, three_sweeps, three_moves, three_phases});
}

int tspgpu_tours_local_search_nl3_dl(tspgpu_ctx *ctx, int slot0, int count, int width, int closing, double time_left_s, long *two_opt_sweeps,
                                     long *two_opt_moves, long *or_sweeps, long *or_moves, int *rounds, long *three_sweeps, long *three_moves,
                                     int *three_phases, long *looked, long *full_sweeps)
{
    if (!ctx) return E_UNAVAILABLE;
    return nl_search_tours(ctx, nl_looks(width, closing), slot0, count, time_left_s,
                           DescentOut{two_opt_sweeps, two_opt_moves, or_sweeps, or_moves, rounds, three_sweeps, three_moves, three_phases, looked,
                                      full_sweeps});
}

int tspgpu_multistart_local_search_nl(tspgpu_ctx *ctx, const int *starts, int nstarts, double time_left_s, int *best_path, double *best_cost,
                                      int *best_start, long *total_two_opt_sweeps, long *total_two_opt_moves, long *total_or_sweeps,
                                      long *total_or_moves, double *costs_out)
{
    if (!ctx) return E_UNAVAILABLE;
    return nl_multistart(ctx, nl_plain(), starts, nstarts, time_left_s, best_path, best_cost, best_start,
                         DescentOut{total_two_opt_sweeps, total_two_opt_moves, total_or_sweeps, total_or_moves}, costs_out);
}

int tspgpu_multistart_local_search_nl3(tspgpu_ctx *ctx, int width, const int *starts, int nstarts, double time_left_s, int *best_path,
                                       double *best_cost, int *best_start, long *total_two_opt_sweeps, long *total_two_opt_moves,
                                       long *total_or_sweeps, long *total_or_moves, long *total_three_sweeps, long *total_three_moves,
                                       double *costs_out)
{
    if (!ctx) return E_UNAVAILABLE;
    return nl_multistart(ctx, nl_three(width), starts, nstarts, time_left_s, best_path, best_cost, best_start,
                         DescentOut{total_two_opt_sweeps, total_two_opt_moves, total_or_sweeps, total_or_moves, nullptr, total_three_sweeps,
                                    total_three_moves},
                         costs_out);
}

int tspgpu_multistart_local_search_nl3_dl(tspgpu_ctx *ctx, int width, int closing, const int *starts, int nstarts, double time_left_s,
                                          int *best_path, double *best_cost, int *best_start, long *total_two_opt_sweeps,
                                          long *total_two_opt_moves, long *total_or_sweeps, long *total_or_moves, long *total_three_sweeps,
                                          long *total_three_moves, long *total_looked, long *total_full_sweeps, double *costs_out)
{
    if (!ctx) return E_UNAVAILABLE;
    return nl_multistart(ctx, nl_looks(width, closing), starts, nstarts, time_left_s, best_path, best_cost, best_start,
                         DescentOut{total_two_opt_sweeps, total_two_opt_moves, total_or_sweeps, total_or_moves, nullptr, total_three_sweeps,
                                    total_three_moves, nullptr, total_looked, total_full_sweeps},
                         costs_out);
}

} // extern "C"

// ---- neighbour-list VNS (tspgpu_nlvns.inc) -----------------------------------------------------------------------------

// per walk beyond the batched descent's: two int arrays of n and a control block; nrand numbers; k trace cells.  All or none
static int nlv_ensure(tspgpu_ctx *ctx, int walks, long nrand, int k)
{
    const size_t n = (size_t)ctx->n, nr = (size_t)walks * (size_t)nrand, nt = (size_t)walks * (size_t)k;
    const Rows rows = ctx->nlv_rows(n);
    hipError_t e = hipSuccess;
    if (walks > ctx->nlv_cap) {
        ctx->drop_nlv();
        if ((e = tspmem::grow(HipMem{ctx->stream}, rows, 0, (size_t)walks)) == hipSuccess) ctx->nlv_cap = walks;
    }
    if (e == hipSuccess) e = ctx->d_nlv_rand.reserve(std::max<size_t>(nr, 1));
    if (e == hipSuccess) e = ctx->d_nlv_trace.reserve(std::max<size_t>(nt, 1));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ctx->drop_nlv();
        return fail(ctx, E_EXHAUSTED, "the neighbour-list VNS needs %zu bytes of device memory for %d walks of %d nodes, %ld numbers and %d iterations each (%s)",
                    tspmem::rows_bytes(rows, (size_t)walks) + nr * 4 + nt * 8, walks, ctx->n, nrand, k, hipGetErrorString(e));
    }
    return E_OK;
}

static int nlv_launch_step(tspgpu_ctx *ctx, int live, bool trace, bool looks)
{
    const int n = ctx->n;
    for (int off = 0; off < live; off += 65535 * 16) {      // (a grid of 1024-thread workgroups holds fewer than 2^32 threads)
        const unsigned wgs = (unsigned)std::min(65535 * 16, live - off);
#define NLV_STEP(DL)                                                                                                                      \
    ELEM_SWITCH(ctx->elem, T, hipLaunchKernelGGL((k_nlv_step<T, DL>), dim3(wgs), dim3(1024), 0, ctx->stream, ctx->S, (const T *)ctx->d_mat.p, n,  \
                                                 ctx->ld, (const int *)(ctx->d_live + off), 0, ctx->nlb, ctx->d_nlb_ctl, ctx->d_nlv_ctl,       \
                                                 ctx->d_nlv_ord, ctx->d_nlv_best, (const int *)ctx->d_nlv_rand.p,                              \
                                                 trace ? ctx->d_nlv_trace.p : nullptr, (const double2 *)ctx->d_pts.p, ctx->kind,               \
                                                 DL ? ctx->d_awake : nullptr))
        if (looks) NLV_STEP(true);
        else NLV_STEP(false);
#undef NLV_STEP
        HIP_TRY(hipGetLastError());
    }
    return E_OK;
}

// the walks on slots 0 .. walks-1: upload, arm, sweep rounds of five launches (the four of the batched descent and the step)
// -- four rounds between looks at the control blocks, one under a deadline, as nlb_descent --, download
static int nlv_walks(tspgpu_ctx *ctx, int w3, int walks, int k, double time_left_s, int *paths, double *costs, const int *rand_values, long nrand,
                     long *consumed, int *iterations, int *kick_pending, int *best_paths, double *best_costs, double *trace, long *totals,
                     const NlbMode &M = NlbMode{})
{
    const double t_end = deadline_of(time_left_s);
    const size_t n = (size_t)ctx->n, W = (size_t)walks;
    int rc;
    // every path is an n-cycle, or nothing is run
    std::vector<int> ords(W * n), ord;
    for (size_t w = 0; w < W; w++) {
        if ((rc = succ_to_order(ctx, paths + w * n, ord))) return fail(ctx, E_INVALID, "paths[%zu] is not a single n-cycle", w);
        memcpy(ords.data() + w * n, ord.data(), n * 4);
    }
    if ((rc = ensure_tours(ctx, walks))) return rc;
    if ((rc = nlb_ensure(ctx, walks))) return rc;
    if ((rc = nlv_ensure(ctx, walks, nrand, k))) return rc;
    if (M.looks && (rc = nlbq_ensure(ctx, walks))) return rc;
    ctx->nlv_walks = walks; ctx->nlv_iterations = ctx->nlv_rounds = ctx->nlv_max_live = ctx->nlv_dry = 0;

    std::vector<NlbCtl> hc(W);
    std::vector<NlvCtl> hv(W);
    memset(hc.data(), 0, W * sizeof(NlbCtl));
    memset(hv.data(), 0, W * sizeof(NlvCtl));
    std::vector<int> live;
    for (size_t w = 0; w < W; w++) {
        const bool finished = iterations[w] >= k, resume = !finished && kick_pending[w] != 0;
        hv[w].it = iterations[w]; hv[w].k = k; hv[w].halt = finished ? 1 : 0;
        hv[w].kick_pending = resume ? 1 : 0; hv[w].resume = resume ? 1 : 0;
        hv[w].nrand = nrand; hv[w].best = best_costs[w];
        hc[w].stop = finished || resume ? 1 : 0;            // a walk in front of a kick phase skips its descent
        hc[w].rounds = finished || resume ? 0 : 1;
        if (!finished) live.push_back((int)w);
    }
    HIP_TRY(hipMemcpyAsync(ctx->S.ord, ords.data(), W * n * 4, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = init_slots(ctx, 0, walks, -1))) return rc;    // (recomputes the cost: refinment.c:6-9)
    mark_slots(ctx, 0, walks, true);
    if (M.looks) {                          // a walk in front of a descent starts all awake; the step writes the sets behind every kick phase
        if ((rc = nlb_fill_flagged(ctx, 0, walks))) return rc;
        HIP_TRY(hipMemsetAsync(ctx->d_nlb_look, 0, W * sizeof(LookCtl), ctx->stream));
    }
    HIP_TRY(hipMemcpyAsync(ctx->d_nlv_best, best_paths, W * n * 4, hipMemcpyHostToDevice, ctx->stream));
    if (nrand > 0) HIP_TRY(hipMemcpyAsync(ctx->d_nlv_rand.p, rand_values, W * (size_t)nrand * 4, hipMemcpyHostToDevice, ctx->stream));
    if (trace && k > 0) HIP_TRY(hipMemsetAsync(ctx->d_nlv_trace.p, 0xff, W * (size_t)k * 8, ctx->stream));     // (NaN: a cell not written)
    HIP_TRY(hipMemcpyAsync(ctx->d_nlb_ctl, hc.data(), W * sizeof(NlbCtl), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->d_nlv_ctl, hv.data(), W * sizeof(NlvCtl), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));             // (the copies read pageable memory of this call)

    if (!live.empty() && (rc = set_live(ctx, live))) return rc;
    const looks::Result r = looks::drive_live(
        now_s, t_end, 4, live, [](int) {},
        [&](int len) {
            int e = nlb_launch_sweep(ctx, 0, len, w3, M);
            if (!e && !(e = nlv_launch_step(ctx, len, trace != nullptr, M.looks))) ctx->nlv_rounds++;
            return e;
        },
        [&] { return ctl_get(ctx, hv.data(), ctx->d_nlv_ctl, W); }, [&](int w) { return hv[w].halt != 0; },
        [&](const std::vector<int> &list) { return set_live(ctx, list); });
    ctx->nlv_max_live = r.max_live;
    if (r.code) return r.code;
    const bool late = r.late;

    std::vector<double> tr(trace ? W * (size_t)k : 0);
    HIP_TRY(hipMemcpyAsync(hc.data(), ctx->d_nlb_ctl, W * sizeof(NlbCtl), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(hv.data(), ctx->d_nlv_ctl, W * sizeof(NlvCtl), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(paths, ctx->S.succ, W * n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(costs, ctx->S.cost, W * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(best_paths, ctx->d_nlv_best, W * n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (!tr.empty()) HIP_TRY(hipMemcpyAsync(tr.data(), ctx->d_nlv_trace.p, tr.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::vector<Descent> DL(M.looks ? W : 0);
    if (M.looks && (rc = nlb_looks_out(ctx, walks, DL.data()))) return rc;
    for (size_t w = 0; w < W; w++) {
        ctx->nlv_iterations += hv[w].it - iterations[w];
        if (hv[w].halt == 2) ctx->nlv_dry++;
        iterations[w] = hv[w].it; kick_pending[w] = hv[w].kick_pending; best_costs[w] = hv[w].best; consumed[w] = (long)hv[w].cursor;
        for (size_t i = 0; i < tr.size() / W; i++)
            if (tr[w * k + i] == tr[w * k + i]) trace[w * k + i] = tr[w * k + i];
        if (totals) {
            long *o = totals + (M.looks ? 11 : w3 > 0 ? 9 : 6) * w;
            o[0] = (long)hc[w].two_opt_sweeps; o[1] = (long)hc[w].two_opt_moves; o[2] = (long)hc[w].or_sweeps; o[3] = (long)hc[w].or_moves;
            o[4] = hc[w].rounds; o[5] = (long)hv[w].kicks;
            if (w3 > 0 || M.looks) { o[6] = (long)hc[w].three_sweeps; o[7] = (long)hc[w].three_moves; o[8] = hc[w].three_phases; }
            if (M.looks) { o[9] = DL[w].lk; o[10] = DL[w].lf; }
        }
    }
    if (late) return E_DEADLINE;
    if (ctx->nlv_dry)
        return fail(ctx, E_EXHAUSTED, "the random numbers of %ld of %d walks ran out in front of a kick phase: call again with more for them",
                    ctx->nlv_dry, walks);
    return E_OK;
}

// the walks behind their argument checks (tspgpu_vns_walks_nl, _nl3, _nl3_dl)
static int nl_walks(tspgpu_ctx *ctx, const NlSpec &S, int walks, int k, double time_left_s, int *paths, double *costs, const int *rand_values,
                    long nrand, long *consumed, int *iterations, int *kick_pending, int *best_paths, double *best_costs, double *trace,
                    long *totals)
{
    if (walks <= 0 || k < 0 || nrand < 0 || !paths || !costs || !consumed || !iterations || !kick_pending || !best_paths || !best_costs ||
        (nrand > 0 && !rand_values))
        return fail(ctx, E_INVALID, "bad argument");
    int rc = nl_admit(ctx, S);
    if (rc) return rc;
    hipSetDevice(ctx->device);
    if ((rc = S.check(ctx))) return rc;
    for (int w = 0; w < walks; w++)
        if (iterations[w] < 0 || iterations[w] > k) return fail(ctx, E_INVALID, "iterations[%d] = %d is outside [0, %d]", w, iterations[w], k);
    return nlv_walks(ctx, S.w3(ctx), walks, k, time_left_s, paths, costs, rand_values, nrand, consumed, iterations, kick_pending, best_paths,
                     best_costs, trace, totals, S.mode());
}

extern "C" {

int tspgpu_vns_walks_nl(tspgpu_ctx *ctx, int walks, int k, double time_left_s, int *paths, double *costs, const int *rand_values, long nrand,
                        long *consumed, int *iterations, int *kick_pending, int *best_paths, double *best_costs, double *trace, long *totals)
{
    if (!ctx) return E_UNAVAILABLE;
    return nl_walks(ctx, nl_plain(), walks, k, time_left_s, paths, costs, rand_values, nrand, consumed, iterations, kick_pending, best_paths,
                    best_costs, trace, totals);
}

int tspgpu_vns_walks_nl3(tspgpu_ctx *ctx, int width, int walks, int k, double time_left_s, int *paths, double *costs, const int *rand_values,
                         long nrand, long *consumed, int *iterations, int *kick_pending, int *best_paths, double *best_costs, double *trace,
                         long *totals)
{
    if (!ctx) return E_UNAVAILABLE;
    return nl_walks(ctx, nl_three(width), walks, k, time_left_s, paths, costs, rand_values, nrand, consumed, iterations, kick_pending, best_paths,
                    best_costs, trace, totals);
}

int tspgpu_vns_walks_nl3_dl(tspgpu_ctx *ctx, int width, int closing, int walks, int k, double time_left_s, int *paths, double *costs,
                            const int *rand_values, long nrand, long *consumed, int *iterations, int *kick_pending, int *best_paths,
                            double *best_costs, double *trace, long *totals)
{
    if (!ctx) return E_UNAVAILABLE;
    return nl_walks(ctx, nl_looks(width, closing), walks, k, time_left_s, paths, costs, rand_values, nrand, consumed, iterations, kick_pending,
                    best_paths, best_costs, trace, totals);
}

} // extern "C"
