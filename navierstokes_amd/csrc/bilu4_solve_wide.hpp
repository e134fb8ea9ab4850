// bilu4_solve_wide.hpp — the exact solve's kernel for WIDE levels, used by ordered handles only (mi_bilu4_create_ordered).
//
// bilu4_level (bilu4_solve.hpp) keeps one block of look-ahead: written for the natural order's short levels, where a lane lives
// for (blocks per row) x (L2 latency) and nothing more is worth holding.  Under a multicolour ordering a level is a colour: tens
// of thousands of independent rows, a contiguous stream of blocks as long as a triangle's share — the shape of a Jacobi sweep.
// This kernel computes the positions [p0, p1) of one level with the software pipeline of bilu4_sweep (bilu4_sweep.hpp):
// coefficients and gathered x blocks P deep, block columns one round ahead, indices clamped to the row's last block,
// unconditional loads.  (The loop is restated here, not shared with bilu4_sweep: with the loop in a common __device__ function the
// compiler's resource report for both double kernels changes from 130 / 134 VGPRs and 3 waves per SIMD to 124 / 128 and 4 — other
// code, with the same bits.  Measured, profiles/NOTES.md R18.1: the double sweeps at counts 3 and 4 are then 1.9 % and 1.7 %
// SLOWER on fe_matrix(24) at fill 1 (41.98 -> 42.76 and 54.38 -> 55.33 us), beyond the run-to-run range, and 2.8 % and 3.0 %
// faster on fe_matrix(68) at fill 0; this kernel 0.8 % faster on the coloured fe_matrix(68).  Not taken: one case is slower.)
//
// Arithmetic: bilu4_row_value's sequence of roundings exactly — blocks ascending, bilu4_chain, one rounded subtraction, backward
// the Dinv chain — so every bit equals bilu4_level's, and which of the two kernels a launch takes cannot change a result.
//
// x is updated in place and therefore NOT __restrict__: the rows of one level only read rows of finished levels (earlier
// launches on the stream), and a lane stores its entry after all its loads.  x is always the ordered handle's own vector, hence
// 16-byte aligned: there is no scalar-load form (the caller's alignment ends at the boundary kernels, bilu4_order_kernels.hpp).
//
// Registers at P = 4 (gfx950, the compiler's kernel-resource-usage report): 130 VGPRs forward, 134 backward, no scratch — 3 waves
// per SIMD, what the double bilu4_sweep it restates gets.  The float instantiation (mi_bilu4spx_*, the single-precision copy of the
// values: Bilu4SweepViewT<float>) at P = 4: 124 VGPRs forward, 128 backward, 18 / 22 SGPRs, no scratch — 4 waves per SIMD, what the
// float bilu4_sweep gets.
#pragma once
#include "bilu4_sweep.hpp"

namespace mi355 {

// An unfolded level of an ordered handle takes this kernel from this many block rows on (MI355_BILU_WIDE_MIN=<rows> at create
// overrides it).  By measurement (profiles/NOTES.md R15.1): the wide kernel was the faster one at every width that was timed, down
// to levels of 64 to 255 block rows (fe_matrix(24) at fill 1), so the threshold is the narrowest level that is not folded.
constexpr int kBiluWideMin = kBiluRowsPerWG;

// P of the float instantiation, a constant of its own: a stage holds 4 VGPRs of coefficients instead of 8, as in the f32 sweeps.
// 4 and 8 were compared by building each (-DMI355_BILU_WIDE_DEPTH_F32=n) and timing both on the GPU (profiles/NOTES.md R16.1): 8 was
// slower on every matrix timed (its report: 100 / 104 VGPRs, 4 waves per SIMD — fewer registers than at 4 for twice the stages; why
// was not analysed).
#ifndef MI355_BILU_WIDE_DEPTH_F32
#define MI355_BILU_WIDE_DEPTH_F32 kBiluSweepDepthF32
#endif
constexpr int kBiluWideDepthF32 = MI355_BILU_WIDE_DEPTH_F32;

template <bool BWD, int P, class T>
__global__ __launch_bounds__(kWG) void bilu4_level_wide(Bilu4SweepViewT<T> V, int p0, int p1, const double* src, double* x)
{
    const int g = blockIdx.x * kWG + threadIdx.x;
    const int pos = p0 + (g >> 2), q = g & 3;
    if (pos >= p1) return; // whole quads leave together
    const int row = V.perm[pos];
    const int ia0 = V.ptr[pos], ia1 = V.ptr[pos + 1];
    double s = src[4 * (size_t)row + q];
    if (ia0 < ia1) {
        const int last = ia1 - 1;
        const unsigned* ucol = reinterpret_cast<const unsigned*>(V.col);
        const T* cq = V.val + 4 * q;
        Bilu4CoefRow<T> a[P];
        double t[P][4];
        unsigned cn[P]; // columns of blocks ia+P+k
#pragma unroll
        for (int k = 0; k < P; k++) {
            const int blk = min(ia0 + k, last);
            a[k].load(cq + 16 * (size_t)blk);
            cn[k] = ucol[blk];
        }
#pragma unroll
        for (int k = 0; k < P; k++) bilu4_load4<true>(x, cn[k], t[k]);
#pragma unroll
        for (int k = 0; k < P; k++) cn[k] = ucol[min(ia0 + P + k, last)];
        for (int ia = ia0; ia < ia1; ia += P) {
#pragma unroll
            for (int k = 0; k < P; k++) {
                const double2 c01 = a[k].c01(), c23 = a[k].c23();
                const double u[4] = {t[k][0], t[k][1], t[k][2], t[k][3]};
                // refill stage k with block ia+k+P (its column arrived a round ago), then ask for the column of block ia+k+2P
                const int nx = min(ia + k + P, last);
                a[k].load(cq + 16 * (size_t)nx);
                bilu4_load4<true>(x, cn[k], t[k]);
                cn[k] = ucol[min(ia + k + 2 * P, last)];
                if (ia + k < ia1) s = __dsub_rn(s, bilu4_chain(c01, c23, u));
            }
        }
    }
    if (BWD) s = bilu4_sweep_dinv(V.dinv, pos, q, s);
    x[4 * (size_t)row + q] = s;
}

} // namespace mi355
