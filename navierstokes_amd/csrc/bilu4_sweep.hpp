// bilu4_sweep.hpp — the block ILU factor applied by a FIXED number of Jacobi sweeps per triangle (the truncated Neumann series;
// Anzt, Chow, Dongarra, "Iterative sparse triangular solves for preconditioning", Euro-Par 2015) instead of the exact,
// level-scheduled solve of bilu4_solve.hpp.  Definition (include/mi355_spmv.h, mi_bilu4sw_*):
//   forward   t^0 = b;               t^{k+1}_i = b_i - sum_{j<i} L_ij t^k_j                  k < sf
//   diagonal  x^0_i = Dinv_i . t^{sf}_i
//   backward  x^{k+1}_i = Dinv_i . (t^{sf}_i - sum_{j>i} U_ij x^k_j)                         k < sb
// Every sweep computes ALL rows from the previous iterate: one launch over the positions [0, nb) of the sweep's level-major copy
// (the same Bilu4SweepView the exact solve reads: values a refactor writes are picked up with no extra step), shaped like the
// blocked product and bound by bandwidth, not by the dependency chain.
//
// Arithmetic: a row's sequence of roundings is bilu4_row_value's — blocks in ascending column order, per block bilu4_chain, then
// ONE rounded subtraction; the backward row ends with Dinv . s, one chain per entry.  A row of dependency level l (counted from 0)
// therefore holds the exact solve's bits after l sweeps, and nlev - 1 sweeps return the exact solve bit for bit.
//
// Memory: the source vector (b or t) is read at the row, the old iterate is gathered by block column, the new iterate is another
// vector: nothing is updated in place, so the old iterate is const __restrict__ (in bilu4_level it cannot be).  src may be out (the
// caller's x == b with no forward sweep: each lane reads its own entry before it writes it), so those two are plain pointers.
// The exact solve keeps one block of look-ahead, written for short levels bound by latency; this kernel streams a whole triangle
// and takes the software pipeline of spmv_bcsr4 (spmv_kernels.hpp): coefficients and gathered blocks P deep, block columns one
// round ahead, indices clamped to the row's last block, unconditional loads.
#pragma once
#include "bilu4_solve.hpp"

namespace mi355 {

// P of the launches, by measurement (profiles/NOTES.md R8.2): from kBcsrDepth = 2, fe_matrix(68) at fill 0, 4 sweeps per triangle,
// P = 1 640 us, 2 625, 3 638, 4 612; fe_matrix(24) at fill 1: 78.9, 56.1, 53.8, 52.9 — the rows of ONE triangle are half as long as
// the product's, so a lane's few blocks are all in flight at P = 4 and the 134 VGPRs (3 waves per SIMD) cost less than they buy.
// (The depths were compared through a run-time switch that the library no longer has: the depth is this constant.)
constexpr int kBiluSweepDepth = 4;

// one sweep: out_i = src_i - sum_k A_ik old_{col k} over the off-diagonal blocks of the view (BWD: then Dinv_i . that)
template <bool BWD, bool AL, int P>
__global__ __launch_bounds__(kWG) void bilu4_sweep(Bilu4SweepView V, int nb, const double* src, const double* __restrict__ old, double* out)
{
    const int g = blockIdx.x * kWG + threadIdx.x;
    const int pos = g >> 2, q = g & 3;
    if (pos >= nb) return; // whole quads leave together
    const int row = V.perm[pos];
    const int ia0 = V.ptr[pos], ia1 = V.ptr[pos + 1];
    double s = src[4 * (size_t)row + q];
    if (ia0 < ia1) {
        const int last = ia1 - 1;
        const unsigned* ucol = reinterpret_cast<const unsigned*>(V.col);
        const double* cq = V.val + 4 * q;
        double2 a01[P], a23[P];
        double t[P][4];
        unsigned cn[P]; // columns of blocks ia+P+k
#pragma unroll
        for (int k = 0; k < P; k++) {
            const int blk = min(ia0 + k, last);
            const double2* r = reinterpret_cast<const double2*>(cq + 16 * (size_t)blk);
            a01[k] = r[0];
            a23[k] = r[1];
            cn[k] = ucol[blk];
        }
#pragma unroll
        for (int k = 0; k < P; k++) bilu4_load4<AL>(old, cn[k], t[k]);
#pragma unroll
        for (int k = 0; k < P; k++) cn[k] = ucol[min(ia0 + P + k, last)];
        for (int ia = ia0; ia < ia1; ia += P) {
#pragma unroll
            for (int k = 0; k < P; k++) {
                const double2 c01 = a01[k], c23 = a23[k];
                const double u[4] = {t[k][0], t[k][1], t[k][2], t[k][3]};
                // refill stage k with block ia+k+P (its column arrived a round ago), then ask for the column of block ia+k+2P
                const int nx = min(ia + k + P, last);
                const double2* nr = reinterpret_cast<const double2*>(cq + 16 * (size_t)nx);
                a01[k] = nr[0];
                a23[k] = nr[1];
                bilu4_load4<AL>(old, cn[k], t[k]);
                cn[k] = ucol[min(ia + k + 2 * P, last)];
                if (ia + k < ia1) s = __dsub_rn(s, bilu4_chain(c01, c23, u));
            }
        }
    }
    if (BWD) {
        const double sv[4] = {quad_bcast<0>(s), quad_bcast<1>(s), quad_bcast<2>(s), quad_bcast<3>(s)};
        const double2* d = reinterpret_cast<const double2*>(V.dinv + 16 * (size_t)pos + 4 * q);
        s = bilu4_chain(d[0], d[1], sv);
    }
    out[4 * (size_t)row + q] = s;
}

// the diagonal pass x^0_i = Dinv_i . t_i over the backward view: the end of the backward row, without its blocks.  t may be x0.
__global__ __launch_bounds__(kWG) void bilu4_sweep_diag(Bilu4SweepView V, int nb, const double* t, double* x0)
{
    const int g = blockIdx.x * kWG + threadIdx.x;
    const int pos = g >> 2, q = g & 3;
    if (pos >= nb) return;
    const int row = V.perm[pos];
    const double s = t[4 * (size_t)row + q];
    const double sv[4] = {quad_bcast<0>(s), quad_bcast<1>(s), quad_bcast<2>(s), quad_bcast<3>(s)};
    const double2* d = reinterpret_cast<const double2*>(V.dinv + 16 * (size_t)pos + 4 * q);
    x0[4 * (size_t)row + q] = bilu4_chain(d[0], d[1], sv);
}

} // namespace mi355
