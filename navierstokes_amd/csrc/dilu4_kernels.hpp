// dilu4_kernels.hpp — the three triangular sweeps of the block DILU preconditioner applied with Eisenstat's trick (mi_dilu4_*,
// include/mi355_spmv.h): with B = L + D + U, pivots E and M = (E + L) E^-1 (E + U), the split-preconditioned operator
// A^ = (E + L)^-1 B (E + U)^-1 E is one backward and one forward sweep over B's OWN off-diagonal blocks, and no product.
//
// ONE row template over the three forms (in: the vector a row reads only its own entries of; g: the vector the sweep gathers
// finished rows from and stores its row into):
//   kDiluToHat    forward,  g = b^:  a = 0; a_q += chain(L_ij row q, b^_j) over the L blocks ascending; s_q = r_iq - a_q;
//                                     b^_iq = chain(Einv_i row q, s)
//   kDiluFromHat  backward, g = x:   a = 0; a_q += chain(U_ij row q, x_j) over the U blocks ascending; c_q = chain(Einv_i row q, a);
//                                     x_iq = u_iq - c_q
//   kDiluApply    forward,  g = y:   a_q = chain(K_i row q, t_i); a_q += chain(L_ij row q, y_j); c_q = chain(Einv_i row q, a);
//                                     y_iq = u_iq - c_q; w_iq = t_iq + y_iq — the final add is the row's epilogue, not a pass
// chain(a, t) = fma(a3,t3, fma(a2,t2, fma(a1,t1, a0*t0))) (bilu4_chain); every += and every - is ONE rounded operation.  A row is
// therefore one fixed sequence of roundings whatever the schedule, the folding or the alignment.
//
// Lane layout of bilu4_solve.hpp: four lanes per block row, lane q owns entry q and reads its row of a block as two 16-byte
// loads; the quad exchanges its four values through DPP (quad_bcast) for the Einv chain.  The off-diagonal blocks lie level-major
// (the rows of a level contiguous), Einv and K by block row.
// The block loop is the four-deep software pipeline of bilu4_level_wide (bilu4_solve_wide.hpp): coefficients and gathered blocks
// P deep, block columns one round ahead, indices clamped to the row's last block, unconditional loads.  It is RESTATED here, not
// shared: bilu4_solve_wide.hpp explains that moving that loop into a common function changes the resource report of the kernels
// that have it, and an existing kernel stays the kernel it is.  This file only uses the load / chain primitives of bilu4_solve.hpp.
// An unfolded level is one launch of dilu4_level, 64 block rows per workgroup; a folded run (Bilu4Launch::folded) is one workgroup
// of dilu4_folded with a workgroup barrier per level, as bilu4_folded.
//
// g is updated in place and read by other rows, so it is NOT __restrict__ (inside the folded kernel other waves write it between
// two barriers).  `in` and `out` may be the same vector, and `in` may be g (mi_dilu4_to_hat_dev in place): a lane reads its own
// entry of `in` before it stores anything, and no other lane reads or writes that entry of `in`.
// AL: g is 16-byte aligned (the handle's own vectors always; a caller's vector needs 8 bytes only).
//
// The compiler's kernel-resource-usage report (gfx950, -O3; to_hat / from_hat / apply_hat; the same for either AL; no scratch, no
// LDS, 4 waves per SIMD throughout):
//   dilu4_level   VGPRs 122 / 122 / 124, SGPRs 24 / 24 / 30
//   dilu4_folded  VGPRs 124 / 124 / 118, SGPRs 34 / 34 / 32
#pragma once
#include "bilu4_solve.hpp"

namespace mi355 {

enum { kDiluToHat = 0, kDiluFromHat = 1, kDiluApply = 2 };
constexpr int kDiluDepth = 4; // stages of the block loop's pipeline: bilu4_level_wide's

// one sweep's level-major copy of B's off-diagonal blocks, and the per-block-row pivots
struct Dilu4View {
    const int* perm;    // [nb] position -> block row
    const int* ptr;     // [nb + 1] by position: first off-diagonal block of the row in this sweep
    const int* col;     // block columns, ascending per row
    const double* val;  // 16 per block, row-major
    const double* einv; // [16 nb] by block row
    const double* kmat; // [16 nb] by block row: K = 2E - D
    const int* lev_ptr; // [nlev + 1] first position of each level
};

// entry q of chain(Mat_row . v), v = the quad's four values
__device__ __forceinline__ double dilu4_quad_chain(const double* mat, int row, int q, double v)
{
    const double sv[4] = {quad_bcast<0>(v), quad_bcast<1>(v), quad_bcast<2>(v), quad_bcast<3>(v)};
    Bilu4CoefRow<double> d;
    d.load(mat + 16 * (size_t)row + 4 * q);
    return bilu4_chain(d.c01(), d.c23(), sv);
}

// one block row of one sweep, by the quad's lane q; pos < number of rows.  t, out: kDiluApply only.
template <int FORM, bool AL>
__device__ __forceinline__ void dilu4_row(const Dilu4View& V, int pos, int q, const double* in, double* g, const double* t, double* out)
{
    constexpr int P = kDiluDepth;
    const int row = V.perm[pos];
    const int ia0 = V.ptr[pos], ia1 = V.ptr[pos + 1];
    const double mine = in[4 * (size_t)row + q];
    double tq = 0.0, a = 0.0;
    if (FORM == kDiluApply) {
        double ti[4];
        bilu4_load4<true>(t, (unsigned)row, ti);
        tq = t[4 * (size_t)row + q]; // (not ti[q]: a register array is never indexed at run time)
        Bilu4CoefRow<double> k;
        k.load(V.kmat + 16 * (size_t)row + 4 * q);
        a = bilu4_chain(k.c01(), k.c23(), ti);
    }
    if (ia0 < ia1) {
        const int last = ia1 - 1;
        const unsigned* ucol = reinterpret_cast<const unsigned*>(V.col);
        const double* cq = V.val + 4 * q;
        Bilu4CoefRow<double> c[P];
        double x[P][4];
        unsigned cn[P]; // columns of blocks ia+P+k
#pragma unroll
        for (int k = 0; k < P; k++) {
            const int blk = min(ia0 + k, last);
            c[k].load(cq + 16 * (size_t)blk);
            cn[k] = ucol[blk];
        }
#pragma unroll
        for (int k = 0; k < P; k++) bilu4_load4<AL>(g, cn[k], x[k]);
#pragma unroll
        for (int k = 0; k < P; k++) cn[k] = ucol[min(ia0 + P + k, last)];
        for (int ia = ia0; ia < ia1; ia += P) {
#pragma unroll
            for (int k = 0; k < P; k++) {
                const double2 c01 = c[k].c01(), c23 = c[k].c23();
                const double u[4] = {x[k][0], x[k][1], x[k][2], x[k][3]};
                // refill stage k with block ia+k+P (its column arrived a round ago), then ask for the column of block ia+k+2P
                const int nx = min(ia + k + P, last);
                c[k].load(cq + 16 * (size_t)nx);
                bilu4_load4<AL>(g, cn[k], x[k]);
                cn[k] = ucol[min(ia + k + 2 * P, last)];
                if (ia + k < ia1) a = __dadd_rn(a, bilu4_chain(c01, c23, u));
            }
        }
    }
    const size_t at = 4 * (size_t)row + q;
    if (FORM == kDiluToHat) {
        g[at] = dilu4_quad_chain(V.einv, row, q, __dsub_rn(mine, a));
    } else {
        const double y = __dsub_rn(mine, dilu4_quad_chain(V.einv, row, q, a));
        g[at] = y;
        if (FORM == kDiluApply) out[at] = __dadd_rn(tq, y);
    }
}

// one unfolded level: positions [p0, p1), 64 block rows per workgroup
template <int FORM, bool AL>
__global__ __launch_bounds__(kWG) void dilu4_level(Dilu4View V, int p0, int p1, const double* in, double* g, const double* t, double* out)
{
    const int gid = blockIdx.x * kWG + threadIdx.x;
    const int pos = p0 + (gid >> 2);
    if (pos >= p1) return; // whole quads leave together
    dilu4_row<FORM, AL>(V, pos, gid & 3, in, g, t, out);
}

// a run of narrow levels [l0, l1) (each fewer than 64 block rows) in ONE workgroup: a workgroup barrier between levels orders the
// quads' stores to g before the next level's loads of it (same CU, same L1, write-through), as in bilu4_folded
template <int FORM, bool AL>
__global__ __launch_bounds__(kWG) void dilu4_folded(Dilu4View V, int l0, int l1, const double* in, double* g, const double* t, double* out)
{
    const int slot = threadIdx.x >> 2, q = threadIdx.x & 3;
    for (int l = l0; l < l1; l++) {
        const int pos = V.lev_ptr[l] + slot;
        if (pos < V.lev_ptr[l + 1]) dilu4_row<FORM, AL>(V, pos, q, in, g, t, out);
        __threadfence_block();
        __syncthreads();
    }
}

} // namespace mi355
