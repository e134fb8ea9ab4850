// dilu4_plan.hpp — host side of the 4x4-block DILU preconditioner applied with Eisenstat's trick (mi_dilu4_*, include/mi355_spmv.h):
// the values of B in the factor's numbering, the pivots E, their inverses and K = 2E - D, and the pattern-only plan of the same
// pivots on the device (Dilu4DevPlan, at the end; kernels in dilu4_factor.hpp).  Plain C++ (no HIP), like bilu4_plan.hpp, whose pattern, levels, folding rule, 4x4 primitives, block intake (bilu4_block_in) and level loop
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

// ---------------------------------------------------------------- the device refactor's plan (mi_dilu4dev_*)
// Pattern-only tables of the pivots on the GPU (dilu4_factor.hpp), built once per handle, in the manner of Bilu4DevPlan.  The
// device state is four arrays: B's L blocks in the forward sweep's order, its U blocks in the backward sweep's order (the
// level-major copies the sweeps read), and Einv and K by block row.  A block of B is named by ONE index ("home") into
// L | U | one diagonal block per block row; the diagonal block of row i is what both Einv_i and K_i start from.
constexpr int kDiluDevFixedLaunches = 1; // launches of a device refactor besides the forward sweep's: the one that scatters

struct Dilu4DevPlan {
    long long nL = 0, nU = 0;  // blocks of the L and of the U array
    std::vector<int> fpos;     // [nb] block row -> its position in the forward order (the refusal rule)
    std::vector<int> gather;   // [nL + nU + nb] by home: the block of the CALLER's matrix that lands there (no fill: never -1)
    std::vector<int> mate;     // [nL] per L block (i, j) in the forward order: the place of block (j, i) in the U array, or -1 when
                               // the pattern has none (the term is skipped) — what dilu4_pivot_row finds by std::lower_bound
    long long pivot_pairs = 0; // entries of mate that are not -1: the updates E_i -= (L_ij Einv_j) U_ji of one refactor
    long long bytes() const { return (long long)sizeof(int) * (long long)(fpos.size() + gather.size() + mate.size() + 1); } // + the refusal word
};

// (a_ptr, a_col: the pattern the schedule was made on, which at fill 0 is S.pat's own; src: null, or the caller's index of every
// block of it, bilu4_order.hpp)
inline void dilu4dev_plan(const Bilu4Schedule& S, const int* a_ptr, const int* a_col, Dilu4DevPlan* D, const int* src = nullptr)
{
    const Bilu4Pattern& P = S.pat;
    const int nb = P.nb;
    D->fpos.assign(nb, 0);
    for (int q = 0; q < nb; q++) D->fpos[S.sweep[0].perm[q]] = q;
    // home of every block of the pattern: the level-major copies list a row's blocks in the pattern's order
    std::vector<int> home((size_t)P.nblocks());
    long long n = 0;
    for (int b = 0; b < 2; b++) {
        for (int q = 0; q < nb; q++) {
            const auto [k0, k1] = P.offdiag(S.sweep[b].perm[q], b == 1);
            for (int k = k0; k < k1; k++) home[k] = (int)n++;
        }
        (b ? D->nU : D->nL) = n - (b ? D->nL : 0);
    }
    for (int i = 0; i < nb; i++) home[P.diag[i]] = (int)(n + i);
    D->gather.assign((size_t)P.nblocks(), -1);
    for (int i = 0; i < nb; i++) {
        int k = P.ptr[i]; // both column lists ascend; without fill they are the same list
        for (int a = a_ptr[i]; a < a_ptr[i + 1]; a++) {
            while (P.col[k] != a_col[a]) k++;
            D->gather[home[k]] = src ? src[a] : a;
        }
    }
    D->mate.assign((size_t)D->nL, -1);
    D->pivot_pairs = 0;
    for (int i = 0; i < nb; i++)
        for (int k = P.ptr[i]; k < P.diag[i]; k++) {
            const int j = P.col[k];
            const int* u0 = P.col.data() + P.diag[j] + 1; // block (j, i): among row j's U columns, which ascend
            const int* u1 = P.col.data() + P.ptr[j + 1];
            const int* at = std::lower_bound(u0, u1, i);
            if (at == u1 || *at != i) continue;
            D->mate[home[k]] = home[at - P.col.data()] - (int)D->nL;
            D->pivot_pairs++;
        }
}

// What the kernels rely on, replayed against the pattern WITHOUT the tables the planner built on the way (block coordinates come
// from the two level-major orders themselves; presence from a linear scan): every home gathered exactly once and from the block
// that belongs there, every mate the block (j, i) of its L block (i, j), every -1 truly absent, fpos the inverse of the forward
// order.  Empty string, or the first violation.
inline std::string dilu4dev_check(const Bilu4Schedule& S, const Dilu4DevPlan& D, const int* src = nullptr)
{
    const Bilu4Pattern& P = S.pat;
    const int nb = P.nb;
    const long long total = P.nblocks();
    if ((long long)D.gather.size() != total || (long long)D.mate.size() != D.nL || (int)D.fpos.size() != nb || D.nL + D.nU + nb != total)
        return "table sizes disagree";
    for (int q = 0; q < nb; q++)
        if (D.fpos[S.sweep[0].perm[q]] != q) return "fpos is not the inverse of the forward order at position " + std::to_string(q);
    // the level-major arrays, block by block: (row, column, the pattern's index)
    std::vector<int> row[2], col[2], at[2];
    for (int b = 0; b < 2; b++)
        for (int q = 0; q < nb; q++) {
            const int i = S.sweep[b].perm[q];
            const auto [k0, k1] = P.offdiag(i, b == 1);
            for (int k = k0; k < k1; k++) row[b].push_back(i), col[b].push_back(P.col[k]), at[b].push_back(k);
        }
    if ((long long)row[0].size() != D.nL || (long long)row[1].size() != D.nU) return "the triangles' block counts disagree with the pattern";
    std::vector<char> seen((size_t)total, 0);
    for (long long h = 0; h < total; h++) {
        const long long k = h < D.nL ? at[0][h] : h < D.nL + D.nU ? at[1][h - D.nL] : P.diag[h - D.nL - D.nU];
        const long long want = src ? src[k] : k;
        if (D.gather[h] != want) return "home " + std::to_string(h) + " gathers block " + std::to_string(D.gather[h]) + ", not " + std::to_string(want);
        if (D.gather[h] < 0 || D.gather[h] >= total || seen[D.gather[h]]++) return "block " + std::to_string(D.gather[h]) + " is gathered twice or out of range (home " + std::to_string(h) + ")";
    }
    long long pairs = 0;
    for (long long k = 0; k < D.nL; k++) {
        const int i = row[0][k], j = col[0][k], m = D.mate[k];
        if (m >= 0) {
            if (m >= D.nU || row[1][m] != j || col[1][m] != i)
                return "L block " + std::to_string(k) + " (" + std::to_string(i) + ", " + std::to_string(j) + ") is mated to U block " + std::to_string(m) + ", which is not (" +
                       std::to_string(j) + ", " + std::to_string(i) + ")";
            pairs++;
        } else {
            if (m != -1) return "L block " + std::to_string(k) + " has mate " + std::to_string(m);
            for (int kk = P.diag[j] + 1; kk < P.ptr[j + 1]; kk++)
                if (P.col[kk] == i) return "L block " + std::to_string(k) + " (" + std::to_string(i) + ", " + std::to_string(j) + ") has no mate, but the pattern has block (" + std::to_string(j) + ", " + std::to_string(i) + ")";
        }
    }
    if (pairs != D.pivot_pairs) return "pivot_pairs is " + std::to_string(D.pivot_pairs) + ", the mates count " + std::to_string(pairs);
    return std::string();
}

} // namespace mi355
