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
//
// Stored type: the kernel is a template over the type the VALUES are stored in — the device factor's doubles (mi_bilu4sw_*) or the
// opt-in single-precision copy of them (mi_bilu4sp_*; the conversion kernel that writes it is at the end of this file).  Pattern,
// vectors, pipeline and arithmetic are the same: a float row of a block is one 16-byte load, widened exactly in registers.
#pragma once
#include "bilu4_solve.hpp"

namespace mi355 {

// P of the launches, by measurement (profiles/NOTES.md R8.2): from kBcsrDepth = 2, fe_matrix(68) at fill 0, 4 sweeps per triangle,
// P = 1 640 us, 2 625, 3 638, 4 612; fe_matrix(24) at fill 1: 78.9, 56.1, 53.8, 52.9 — the rows of ONE triangle are half as long as
// the product's, so a lane's few blocks are all in flight at P = 4 and the 134 VGPRs (3 waves per SIMD) cost less than they buy.
// (The depths were compared through a run-time switch that the library no longer has: the depth is this constant.)
constexpr int kBiluSweepDepth = 4;
// ... and over the single-precision copy of the values (mi_bilu4sp_*): a stage holds 4 VGPRs of coefficients instead of 8.  4 and 8
// were compared by building each (-DMI355_BILU_SWEEP_DEPTH_F32=n) and timing both on the GPU: profiles/NOTES.md R11.1.
#ifndef MI355_BILU_SWEEP_DEPTH_F32
#define MI355_BILU_SWEEP_DEPTH_F32 4
#endif
constexpr int kBiluSweepDepthF32 = MI355_BILU_SWEEP_DEPTH_F32;

// The values a sweep streams, in the type they are STORED in: the device factor itself (double), or its single-precision copy
// (float, mi_bilu4sp_*: v32 = (double)(float)v, round to nearest even, subnormals kept).  Pattern, positions and vectors are the
// view's and double either way; the arithmetic is bilu4_chain in double on the widened values.  (A lane's row of a block in
// registers, Bilu4CoefRow<T>, and the end of a backward row, bilu4_sweep_dinv<T>: bilu4_solve.hpp, shared with the exact solve.)
template <class T>
struct Bilu4SweepVals {
    const T* val;  // 16 per block, row-major, in the view's block order
    const T* dinv; // backward sweep: [16 * nb] by position; forward: null
};

// one sweep: out_i = src_i - sum_k A_ik old_{col k} over the off-diagonal blocks of the view (BWD: then Dinv_i . that)
template <bool BWD, bool AL, int P, class T>
__global__ __launch_bounds__(kWG) void bilu4_sweep(Bilu4SweepView V, Bilu4SweepVals<T> A, int nb, const double* src, const double* __restrict__ old, double* out)
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
        const T* cq = A.val + 4 * q;
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
        for (int k = 0; k < P; k++) bilu4_load4<AL>(old, cn[k], t[k]);
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
                bilu4_load4<AL>(old, cn[k], t[k]);
                cn[k] = ucol[min(ia + k + 2 * P, last)];
                if (ia + k < ia1) s = __dsub_rn(s, bilu4_chain(c01, c23, u));
            }
        }
    }
    if (BWD) s = bilu4_sweep_dinv(A.dinv, pos, q, s);
    out[4 * (size_t)row + q] = s;
}

// the diagonal pass x^0_i = Dinv_i . t_i over the backward view: the end of the backward row, without its blocks.  t may be x0.
template <class T>
__global__ __launch_bounds__(kWG) void bilu4_sweep_diag(Bilu4SweepView V, const T* dinv, int nb, const double* t, double* x0)
{
    const int g = blockIdx.x * kWG + threadIdx.x;
    const int pos = g >> 2, q = g & 3;
    if (pos >= nb) return;
    const int row = V.perm[pos];
    x0[4 * (size_t)row + q] = bilu4_sweep_dinv(dinv, pos, q, t[4 * (size_t)row + q]);
}

// ---------------------------------------------------------------- the single-precision copy (mi_bilu4sp_*)
// What a conversion leaves behind for mi_bilu4sp_status: how many values were finite as double and are not as float, and the smallest
// block row that holds one.
constexpr int kBiluSpNoRow = 0x7fffffff;
struct Bilu4SpRecord {
    unsigned long long overflowed;
    int row;
};

// the three arrays of the level-major factor a conversion walks, as one range of ROWS OF BLOCKS (4 values, one lane each):
// [0, end[0]) the L blocks, [end[0], end[1]) the U blocks, [end[1], end[2]) the inverted diagonal blocks by backward position
struct Bilu4SpConvert {
    const double* src[3];
    float* dst[3];
    long long end[3];
    const int* ptr[2];  // forward, backward: [nb + 1] by position, to name the block row of an overflow
    const int* perm[2]; // position -> block row
    int nb;
    Bilu4SpRecord* rec;
};

__global__ void bilu4sp_reset(Bilu4SpRecord* rec)
{
    rec->overflowed = 0;
    rec->row = kBiluSpNoRow;
}

// dst = (float)src, round to nearest even, for every value of the factor; one lane per row of a block: two 16-byte loads, one
// 16-byte store.  The rare overflow looks its block row up (a binary search of the position pointers) and reports it.
__global__ __launch_bounds__(kWG) void bilu4sp_convert(Bilu4SpConvert C)
{
    const long long g = (long long)blockIdx.x * kWG + threadIdx.x;
    if (g >= C.end[2]) return;
    const int part = g < C.end[0] ? 0 : g < C.end[1] ? 1 : 2;
    const long long r = g - (part ? C.end[part - 1] : 0); // row r & 3 of block r >> 2 of its array
    const double2* p = reinterpret_cast<const double2*>(C.src[part] + 4 * r);
    const double2 v01 = p[0], v23 = p[1];
    const double v[4] = {v01.x, v01.y, v23.x, v23.y};
    const float4 f = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
    reinterpret_cast<float4*>(C.dst[part])[r] = f;
    const float w[4] = {f.x, f.y, f.z, f.w};
    int bad = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) bad += (isfinite(v[k]) && !isfinite(w[k])) ? 1 : 0;
    if (bad) {
        const long long blk = r >> 2;
        int pos;
        if (part == 2) {
            pos = (int)blk;
        } else { // the last position whose first block is <= blk (positions without blocks repeat the pointer: skipped)
            const int* ptr = C.ptr[part];
            int lo = 0, hi = C.nb; // ptr[lo] <= blk < ptr[hi]
            while (hi - lo > 1) {
                const int mid = lo + (hi - lo) / 2;
                if (ptr[mid] <= blk) lo = mid; else hi = mid;
            }
            pos = lo;
        }
        atomicAdd(&C.rec->overflowed, (unsigned long long)bad);
        atomicMin(&C.rec->row, C.perm[part == 0 ? 0 : 1][pos]);
    }
}

} // namespace mi355
