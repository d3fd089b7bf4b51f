// ---------------------------------------------------------------------------
// tmat: the tour-ordered copy of the matrix that the shaped k_lds2opt keeps in device memory (tspgpu_lds2opt.inc, TM).
//     tmat[x][q] = c[x][ord q]           (row of node x, indexed by array cell q; the cell of x itself poisoned)
// A move reverses the array cells [lo, lo + M) (mod n, n a power of two, 2 <= M <= n/2).  A workgroup that gets a node it
// did not hold reads that node's row from tmat -- still in the order before the move -- and applies the reversal on the way
// in; the workgroup that holds a node behind the move rewrites the 8-cell chunks of its row that overlap the range.
// This file is the index arithmetic of both, shared by the kernel and by the CPU model (tests/lds_tmat_main.cpp): plain
// integers, no HIP types.
// ---------------------------------------------------------------------------
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TMAT_HD __host__ __device__
#else
#define TMAT_HD
#endif

namespace lds_tmat {

// is array cell q inside the reversed range?
TMAT_HD inline bool in_range(int q, int lo, int M, int n) { return ((q - lo) & (n - 1)) < M; }

// the cell of the row BEFORE the move that cell q of the row AFTER the move takes its value from
TMAT_HD inline int src_cell(int q, int lo, int M, int n) { return in_range(q, lo, M, n) ? (2 * lo + M - 1 - q) & (n - 1) : q; }

// How the aligned chunk of 8 cells that begins at q0 is fetched:
//   SAME      all eight cells outside the range: the 8 cells from `start` (== q0), as they are
//   MIRROR    all eight inside and the mirrored run does not cross the array end: the 8 cells from `start`
//             (any 2-byte boundary), their order reversed
//   CELLWISE  mixed, or the mirrored run crosses the array end: cell by cell through src_cell
enum { SAME = 0, MIRROR = 1, CELLWISE = 2 };
TMAT_HD inline int chunk_class(int q0, int lo, int M, int n, int &start)
{
    const int d0 = (q0 - lo) & (n - 1);                 // the chunk's cells lie d0 .. d0 + 7 behind lo (mod n)
    start = q0;
    if (d0 >= M && d0 + 7 < n) return SAME;             // (d0 + 7 >= n: the chunk's tail wraps into the range's head)
    if (d0 + 7 < M) {
        const int a = (2 * lo + M - 1 - (q0 + 7)) & (n - 1);
        if (a + 8 <= n) { start = a; return MIRROR; }
    }
    return CELLWISE;
}

// Every CELLWISE chunk of a row is one of these three (a chunk listed here may be of another class: fetching it cell by
// cell is right for any chunk): the chunk of the range's first cell, of the first cell behind it, and of the cell whose
// source is cell 0 (the only place where a mirrored run can cross the array end).
TMAT_HD inline void cellwise_chunks(int lo, int M, int n, int c[3])
{
    c[0] = lo >> 3;
    c[1] = ((lo + M) & (n - 1)) >> 3;
    c[2] = ((2 * lo + M - 1) & (n - 1)) >> 3;
}

// The write-back behind a move: wb_count aligned chunks from chunk wb_first on, wrapping at n / 8 chunks, cover the range.
TMAT_HD inline int wb_first(int lo) { return lo >> 3; }
TMAT_HD inline int wb_count(int lo, int M) { return ((lo & 7) + M + 7) >> 3; }

// The packed evaluation of the shaped kernels: two 16-bit deltas a register, carried with a bias of 0x8000 a half so that
// x + y - w[k] is ONE 32-bit three-operand add.  With every operand <= 16383 a half of x + y + pk_bias(wk) lies in
// [16385, 65534] -- no carry into the upper half -- and, w[m] taken off half by half, in [2, 65534]; the unsigned order of
// the biased halves is the signed order of the deltas, and XOR PK_BIAS gives the deltas themselves.
constexpr unsigned PK_BIAS = 0x80008000u;
TMAT_HD inline unsigned pk_bias(unsigned wk) { return PK_BIAS - (wk | wk << 16); }                   // wk <= 16383
TMAT_HD inline unsigned pk_biased(unsigned x, unsigned y, unsigned b) { return x + y + b; }          // packed x, y; b = pk_bias(wk)

}   // namespace lds_tmat
