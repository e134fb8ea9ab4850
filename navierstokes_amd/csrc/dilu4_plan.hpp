// dilu4_plan.hpp — host side of the 4x4-block DILU preconditioner applied with Eisenstat's trick (mi_dilu4_*, include/mi355_spmv.h):
// the values of B in the factor's numbering and the pivots E, their inverses and K = 2E - D.  Plain C++ (no HIP), like
// bilu4_plan.hpp, whose pattern, levels, folding rule, 4x4 primitives, block intake (bilu4_block_in) and level loop
// (bilu4_for_level_rows) it reuses; the ordering is bilu4_order.hpp's.
//
// B = Q A Q^T = L + D + U (strict block triangles, block diagonal), NO fill: the pattern is B's own, so Bilu4Pattern at fill 0 lists
// B's blocks in B's order and block k of the pattern is block k of the permuted matrix.  M = (E + L) E^-1 (E + U).
//
// PIVOTS (part of the interface, restated by tests/dilu4_model.py), block rows i ascending:
//   E_i = D_i;  for every j < i ascending with BOTH blocks (i, j) and (j, i) in the pattern: T = B_ij . Einv_j, P = T . B_ji (each a
//   4x4 product of sixteen chains, bilu4_matmul), E_i = E_i - P, one rounded subtraction per entry;
//   Einv_i = bilu4_invert(E_i) (Gauss-Jordan without pivoting, a pivot below 1e-12 refused);
//   K_i = (2 E_i) - D_i per entry: an exact doubling, then one rounded subtraction.
// Row i needs Einv_j only of rows j it has an L block to: rows of one forward dependency level are independent.
// Compiled with floating-point contraction OFF, as bilu4_plan.hpp is.
#pragma once
#include "bilu4_order.hpp"
#include "bilu4_plan.hpp"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace mi355 {

// the caller's values into B's block order, row-major; src: null, or the caller's index of every block of B (bilu4_order.hpp)
inline void dilu4_values(long long nblocks, const double* coef, bool colmajor, const int* src, double* val)
{
    for (long long k = 0; k < nblocks; k++) bilu4_block_in(coef + 16 * (size_t)(src ? src[k] : k), colmajor, val + 16 * (size_t)k);
}

// Einv_i and K_i of block row i (16 doubles each, by block row); false: a refused pivot in this row
static inline bool dilu4_pivot_row(const Bilu4Pattern& P, int i, const double* val, double* einv, double* kmat)
{
    const double* d = val + 16 * (size_t)P.diag[i];
    double* e = einv + 16 * (size_t)i;
    std::memcpy(e, d, sizeof(double) * 16);
    double t[16], p[16];
    for (int k = P.ptr[i]; k < P.diag[i]; k++) {
        const int j = P.col[k];
        // block (j, i): among row j's U columns, which ascend
        const int* u0 = P.col.data() + P.diag[j] + 1;
        const int* u1 = P.col.data() + P.ptr[j + 1];
        const int* at = std::lower_bound(u0, u1, i);
        if (at == u1 || *at != i) continue; // no block (j, i): the term is skipped
        bilu4_matmul(val + 16 * (size_t)k, einv + 16 * (size_t)j, t);
        bilu4_matmul(t, val + 16 * (size_t)(at - P.col.data()), p);
        for (int x = 0; x < 16; x++) e[x] = e[x] - p[x];
    }
    double* km = kmat + 16 * (size_t)i;
    for (int x = 0; x < 16; x++) {
        const double twice = 2.0 * e[x];
        km[x] = twice - d[x];
    }
    return bilu4_invert(e);
}

// All pivots over the forward schedule F, by bilu4_for_level_rows: the bits do not depend on the thread count.  Returns -1, or the
// lowest block row (B's numbering) whose pivot was refused; rows behind it are then not meaningful.
inline int dilu4_pivots(const Bilu4Pattern& P, const Bilu4Sweep& F, const double* val, int threads, double* einv, double* kmat)
{
    return bilu4_for_level_rows(F, threads, [&](int i, int) { return dilu4_pivot_row(P, i, val, einv, kmat); });
}

} // namespace mi355
