// bilu4_solve.hpp — the level-scheduled triangular solves of the 4x4-block ILU preconditioner, x = U^-1 L^-1 b: what
// MatSolve_SeqBAIJ_4 computes (src/kernels/baij4_solve.c:4-93; natural ordering, the diagonal blocks stored INVERTED).
//
// The factor lies level-major on the device (bilu4_plan.hpp): for each sweep the rows of a dependency level are contiguous, so a
// level is one contiguous stream of blocks; `perm` maps a position back to its block row.  Lane layout of spmv_bcsr4: four lanes
// per block row, lane q owns row 4*i + q and reads its four coefficients of a block as two 16-byte loads (the quad reads the
// block's 128 bytes contiguously); the t / x block of the block column is gathered through L2.  One block of look-ahead:
// a level is a few MB at most, so a lane lives for (blocks per row) x (L2 latency) and the loop is written to keep the next
// block's loads in flight while the current chain runs.
//
// Arithmetic (fixed, include/mi355_spmv.h): per block p = fma(a3,t3, fma(a2,t2, fma(a1,t1, a0*t0))), then ONE rounded s - p,
// blocks in ascending column order; the backward sweep ends with x = Dinv . s, one chain from a rounded product per entry.
// A row's result is one fixed sequence of roundings whatever the schedule, the folding or the alignment of the vectors.
//
// Stored type: the kernels are templates over the type the VALUES are stored in, as bilu4_sweep is (bilu4_sweep.hpp) — the device
// factor's doubles (mi_bilu4_solve*), or the opt-in single-precision copy of them (mi_bilu4spx_*: v32 = (double)(float)v for L, U
// and the inverted diagonal blocks).  Pattern, vectors, look-ahead and arithmetic are the same; a float row of a block is ONE
// 16-byte load, widened exactly in registers where the chain takes it, so the result is the exact solve of the rounded factor.
// The type is the VIEW's (Bilu4SweepViewT<T>), not a second kernel argument beside it as in bilu4_sweep: with the values in an
// argument of their own the compiler's kernel-resource-usage report for the double backward kernels changes (bilu4_level and
// bilu4_level_wide: 22 SGPRs become 18), and an existing kernel stays the kernel it is.  This way the double instantiations take
// the argument they always took and their report is unchanged.  The float instantiations (gfx950, the same report, forward /
// backward, either alignment, no scratch, 8 waves per SIMD): bilu4_level 40 / 44 VGPRs and 18 / 22 SGPRs, bilu4_folded 44 / 48 and
// 26 / 26 — the double kernels' numbers: one block of look-ahead holds too little for the narrower type to show.
//
// The vector x carries t between the sweeps and between the levels.  It is read with plain vector loads and is deliberately
// NOT const __restrict__: inside the folded kernel other waves of the workgroup write it between two barriers.
#pragma once
#include "spmv_kernels.hpp"

namespace mi355 {

// T: the type the values are stored in.  Bilu4SweepView, the view of the device factor's own doubles, is what every kernel took
// before there was a second type and is the same kernel argument as before; Bilu4SweepViewT<float> carries the arrays of the
// single-precision copy in the same two places (Bilu4SweepVals<float>, bilu4_sweep.hpp) and the SAME pattern arrays.
template <class T>
struct Bilu4SweepViewT {
    const int* perm;    // [nb] position -> block row
    const int* ptr;     // [nb + 1] by position: first off-diagonal block of the row in this sweep
    const int* col;     // block columns, ascending per row
    const T* val;       // 16 per block, row-major
    const T* dinv;      // backward sweep: [16 * nb] by position, the inverted diagonal blocks; forward: null
    const int* lev_ptr; // [nlev + 1] first position of each level
};
using Bilu4SweepView = Bilu4SweepViewT<double>;

// the four entries of block j of v; AL: v is 16-byte aligned
template <bool AL>
__device__ __forceinline__ void bilu4_load4(const double* v, unsigned j, double (&t)[4])
{
    if (AL) {
        const double2* p = reinterpret_cast<const double2*>(v + 4 * (size_t)j);
        const double2 a = p[0], b = p[1];
        t[0] = a.x, t[1] = a.y, t[2] = b.x, t[3] = b.y;
    } else {
        const double* p = v + 4 * (size_t)j;
        t[0] = p[0], t[1] = p[1], t[2] = p[2], t[3] = p[3];
    }
}

__device__ __forceinline__ double bilu4_chain(double2 c01, double2 c23, const double (&t)[4])
{
    double p = __dmul_rn(c01.x, t[0]);
    p = fma(c01.y, t[1], p);
    p = fma(c23.x, t[2], p);
    return fma(c23.y, t[3], p);
}

// a quad lane's row of one block as it lies in registers between its load and its chain: two 16-byte loads of doubles, or ONE of
// floats, widened (exactly) only where the chain takes it, so that a stage of a pipeline holds half the registers
template <class T>
struct Bilu4CoefRow;
template <>
struct Bilu4CoefRow<double> {
    double2 a01, a23;
    __device__ __forceinline__ void load(const double* p)
    {
        const double2* r = reinterpret_cast<const double2*>(p);
        a01 = r[0];
        a23 = r[1];
    }
    __device__ __forceinline__ double2 c01() const { return a01; }
    __device__ __forceinline__ double2 c23() const { return a23; }
};
template <>
struct Bilu4CoefRow<float> {
    float4 a;
    __device__ __forceinline__ void load(const float* p) { a = *reinterpret_cast<const float4*>(p); }
    __device__ __forceinline__ double2 c01() const { return make_double2((double)a.x, (double)a.y); }
    __device__ __forceinline__ double2 c23() const { return make_double2((double)a.z, (double)a.w); }
};

// the end of a backward row: Dinv_pos . s, the quad's four entries of s exchanged
template <class T>
__device__ __forceinline__ double bilu4_sweep_dinv(const T* dinv, int pos, int q, double s)
{
    const double sv[4] = {quad_bcast<0>(s), quad_bcast<1>(s), quad_bcast<2>(s), quad_bcast<3>(s)};
    Bilu4CoefRow<T> d;
    d.load(dinv + 16 * (size_t)pos + 4 * q);
    return bilu4_chain(d.c01(), d.c23(), sv);
}

// one block row of one sweep, by the quad's lane q; pos < number of rows.  BWD: src == x (t lies there), else src == b.  The
// value of entry q of block row `row`: every kernel of the solve stores exactly this.
template <bool BWD, bool AL, class T>
__device__ __forceinline__ double bilu4_row_value(const Bilu4SweepViewT<T>& V, int pos, int row, int q, const double* src, const double* x)
{
    const int ia0 = V.ptr[pos], ia1 = V.ptr[pos + 1];
    double s = src[4 * (size_t)row + q];
    if (ia0 < ia1) {
        const int last = ia1 - 1;
        const T* cq = V.val + 4 * q;
        Bilu4CoefRow<T> a;
        a.load(cq + 16 * (size_t)ia0);
        double t[4];
        bilu4_load4<AL>(x, (unsigned)V.col[ia0], t);
        unsigned cn = (unsigned)V.col[min(ia0 + 1, last)];
        for (int ia = ia0; ia < ia1; ia++) {
            const double2 c01 = a.c01(), c23 = a.c23();
            const double u[4] = {t[0], t[1], t[2], t[3]};
            // the next block (clamped to the row's last: loads are unconditional) while this one's chain runs
            const int nb = min(ia + 1, last);
            a.load(cq + 16 * (size_t)nb);
            bilu4_load4<AL>(x, cn, t);
            cn = (unsigned)V.col[min(ia + 2, last)];
            s = __dsub_rn(s, bilu4_chain(c01, c23, u));
        }
    }
    if (BWD) s = bilu4_sweep_dinv(V.dinv, pos, q, s);
    return s;
}

template <bool BWD, bool AL, class T>
__device__ __forceinline__ void bilu4_row(const Bilu4SweepViewT<T>& V, int pos, int q, const double* src, double* x)
{
    const int row = V.perm[pos];
    x[4 * (size_t)row + q] = bilu4_row_value<BWD, AL>(V, pos, row, q, src, x);
}

// one level: positions [p0, p1), 64 block rows per workgroup
template <bool BWD, bool AL, class T>
__global__ __launch_bounds__(kWG) void bilu4_level(Bilu4SweepViewT<T> V, int p0, int p1, const double* src, double* x)
{
    const int g = blockIdx.x * kWG + threadIdx.x;
    const int pos = p0 + (g >> 2);
    if (pos >= p1) return; // whole quads leave together
    bilu4_row<BWD, AL>(V, pos, g & 3, src, x);
}

// a run of narrow levels [l0, l1) (each fewer than 64 block rows) in ONE workgroup: a workgroup barrier between levels.  The
// barrier orders the quads' stores to x before the next level's loads of it (same CU, same L1, write-through).
template <bool BWD, bool AL, class T>
__global__ __launch_bounds__(kWG) void bilu4_folded(Bilu4SweepViewT<T> V, int l0, int l1, const double* src, double* x)
{
    const int slot = threadIdx.x >> 2, q = threadIdx.x & 3;
    for (int l = l0; l < l1; l++) {
        const int pos = V.lev_ptr[l] + slot;
        if (pos < V.lev_ptr[l + 1]) bilu4_row<BWD, AL>(V, pos, q, src, x);
        __threadfence_block();
        __syncthreads();
    }
}

} // namespace mi355
