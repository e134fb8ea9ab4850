// dilu4_factor.hpp — the pivots of the 4x4-block DILU preconditioner on the GPU (mi_dilu4dev_refactor): what a Newton step
// recomputes before every linear solve (src/solve_newton.c:1245-1265), from block values that already lie on the device, written in
// place into the arrays the three sweeps read (dilu4_kernels.hpp): B's two triangles level-major, Einv and K by block row.  Bit for
// bit the host computation of dilu4_plan.hpp ("PIVOTS" there, dilu4_pivot_row operation for operation): E_i = D_i; for the row's L
// blocks (i, j) in ascending column that have a block (j, i): T = L_ij . Einv_j, P = T . U_ji, every entry one chain from a rounded
// product (bilu4_matmul), E_i = E_i - P one rounded subtraction per entry; K_i = (2 E_i) - D_i; Einv_i by the Gauss-Jordan inverse
// of bilu4_plan.hpp with its 1e-12 refusal.  An L block without a mate is skipped; there is NO all-zero-block skip (the host has
// none).  Compiled with -ffp-contract=off.
//
// Schedule: the forward sweep's — a row needs Einv of the rows it has an L block to and nothing else.  A wide level is one launch,
// a run of narrow levels one launch of one workgroup with a barrier between levels (Bilu4Launch::folded, the one rule), after ONE
// launch that scatters the caller's values to every block of L | U, to Einv_i and K_i (both start as D_i, so that no third array
// is needed) and resets the refusal word.
//
// Lane layout of bilu4_factor.hpp: SIXTEEN lanes per block row; lane e = 4r + c owns entry (r, c) of E_i, K_i and of every block of
// its row.  A lane only ever reads back from its own row what it wrote itself (Einv_i and K_i start as D_i, written by the scatter
// launch, and are stored once), so program order suffices inside a row.  The row of L_ij or of T that a product needs comes from
// the 16-lane group by cross-lane moves (the idiom of bilu4f_row, restated); the inversion runs in registers.  Einv_j of another
// row was written by an earlier launch or, in a folded run, by other waves of the workgroup before a barrier: Einv is read with
// plain loads and is deliberately NOT const __restrict__.  L and U are written by the scatter launch only.
//
// The block loop: the two products of one block do not depend on the previous block, only the subtraction chain does.  The
// operands of block k+1 (its own entry of L, a column of Einv_j and of U_ji) are loaded while block k is multiplied, and the
// indices they need (column, mate) one block further ahead, so that no load waits for an index.  Indices are clamped to the row's
// last block and an absent mate reads U block 0 (every array has at least one block), so all loads are unconditional; an unmated
// block's product is computed and dropped by a select, which keeps the 16-lane groups of a wave in step.
//
// Refused pivot, the rule of bilu4_factor.hpp: the refusing group does atomicMin on *bad with B's block row.  The host stops after
// the first LEVEL with a refusal and reports the lowest row of that level; here a launch does nothing when *bad names a row of an
// EARLIER launch (fpos[*bad] < the launch's first position — a row of the launch's own levels must not stop its peers, or a lower
// row of the same level could go unreported), and a folded run leaves at the barrier that ends a level with a refusal.
//
// The compiler's kernel-resource-usage report (gfx950, -O3, -ffp-contract=off; scratch 0 in all three):
//   dilu4f_gather  VGPRs 10, SGPRs 22, no LDS, 8 waves per SIMD
//   dilu4f_level   VGPRs 59, SGPRs 30, no LDS, 8 waves per SIMD
//   dilu4f_folded  VGPRs 67, SGPRs 68, LDS 256 bytes (the barrier's vote), 7 waves per SIMD (it runs as one workgroup of 16 waves)
#pragma once
#include "spmv_kernels.hpp"
#include "bilu4_plan.hpp"

namespace mi355 {

// (bilu4_factor.hpp's two constants, restated: that file defines kernels and belongs to one translation unit)
constexpr int kDiluBadNone = 0x7fffffff;  // *bad: no pivot refused
constexpr int kDiluFactorFoldedWG = 1024; // threads of the folded kernel: 16 lanes for each of up to 63 block rows

struct Dilu4FactorView {
    const int* fperm;   // [nb] forward position -> block row
    const int* fptr;    // [nb + 1] by forward position: the row's first L block
    const int* fcol;    // [nL] column of every L block
    const int* lev_ptr; // forward levels
    const int* fpos;    // [nb] block row -> forward position
    const int* mate;    // [nL] see Dilu4DevPlan
    double* L;          // level-major triangles (forward / backward order)
    double* U;
    double* einv;       // [16 nb] by block row
    double* kmat;       // [16 nb] by block row
    int nL, nU;
    int* bad;
};

// scatter in one pass: 16 lanes per home, every block of L | U written once and D_i into Einv_i and K_i; also resets *bad
__global__ __launch_bounds__(kWG) void dilu4f_gather(Dilu4FactorView V, const int* __restrict__ gather, long long total,
                                                     const double* __restrict__ coef, int colmajor)
{
    const long long g = (long long)blockIdx.x * kWG + threadIdx.x;
    if (g == 0) *V.bad = kDiluBadNone;
    const long long h = g >> 4;
    if (h >= total) return;
    const int e = (int)(g & 15);
    const double v = coef[16 * (size_t)gather[h] + (colmajor ? 4 * (e & 3) + (e >> 2) : e)];
    if (h < V.nL) {
        V.L[16 * (size_t)h + e] = v;
    } else if (h < (long long)V.nL + V.nU) {
        V.U[16 * (size_t)(h - V.nL) + e] = v;
    } else {
        const size_t at = 16 * (size_t)(h - V.nL - V.nU) + e;
        V.einv[at] = v;
        V.kmat[at] = v;
    }
}

// what a lane holds of one L block (i, j) and its partners: its own entry of L_ij, column c of Einv_j and of U_ji
struct Dilu4fStage {
    double w, a0, a1, a2, a3, u0, u1, u2, u3;
    __device__ __forceinline__ void load(const Dilu4FactorView& V, int lk, int j, int m, int e)
    {
        const int c = e & 3;
        w = V.L[16 * (size_t)lk + e];
        const double* ap = V.einv + 16 * (size_t)j + c;
        a0 = ap[0], a1 = ap[4], a2 = ap[8], a3 = ap[12];
        const double* up = V.U + 16 * (size_t)max(m, 0) + c;
        u0 = up[0], u1 = up[4], u2 = up[8], u3 = up[12];
    }
};

// one block row by its 16-lane group (e: the lane's entry); false: its pivot was refused.  All 16 lanes run it together.
__device__ __forceinline__ bool dilu4f_row(const Dilu4FactorView& V, int q, int e)
{
    const int r4 = e & 12, c = e & 3;
    const int i = V.fperm[q];
    const int k0 = V.fptr[q], k1 = V.fptr[q + 1];
    double* ei = V.einv + 16 * (size_t)i + e;
    double* ki = V.kmat + 16 * (size_t)i + e;
    double a = *ei;       // E_i, from D_i
    const double d = *ki; // D_i
    if (k0 < k1) {
        const int last = k1 - 1;
        // data one block ahead, its indices two
        int m = V.mate[k0];
        Dilu4fStage nx;
        nx.load(V, k0, V.fcol[k0], m, e);
        int kn = min(k0 + 1, last);
        int jn = V.fcol[kn], mn = V.mate[kn];
        for (int lk = k0; lk < k1; lk++) {
            const Dilu4fStage s = nx;
            const int mc = m;
            nx.load(V, kn, jn, mn, e);
            m = mn;
            kn = min(lk + 2, last);
            jn = V.fcol[kn], mn = V.mate[kn];
            double t = __dmul_rn(__shfl(s.w, r4, 16), s.a0);
            t = fma(__shfl(s.w, r4 + 1, 16), s.a1, t);
            t = fma(__shfl(s.w, r4 + 2, 16), s.a2, t);
            t = fma(__shfl(s.w, r4 + 3, 16), s.a3, t);
            double p = __dmul_rn(__shfl(t, r4, 16), s.u0);
            p = fma(__shfl(t, r4 + 1, 16), s.u1, p);
            p = fma(__shfl(t, r4 + 2, 16), s.u2, p);
            p = fma(__shfl(t, r4 + 3, 16), s.u3, p);
            const double less = __dsub_rn(a, p);
            a = mc < 0 ? a : less; // no block (j, i): the term is skipped
        }
    }
    *ki = __dsub_rn(__dmul_rn(2.0, a), d);
    // E_i inverted in registers (bilu4f_row's inversion, restated)
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double dk = __shfl(a, 5 * k, 16);
        if (fabs(dk) < kBiluPivotMin) {
            ok = false;
            break;
        }
        const double piv = __ddiv_rn(1.0, dk);
        if (e == 5 * k) a = 1.0;
        if (r4 == 4 * k) a = __dmul_rn(a, piv);
        const double f = __shfl(a, r4 + k, 16);      // a[r][k], before it is zeroed
        const double akc = __shfl(a, 4 * k + c, 16); // a[k][c], scaled
        if (r4 != 4 * k) a = __dsub_rn(c == k ? 0.0 : a, __dmul_rn(f, akc));
    }
    *ei = a;
    if (!ok && e == 0) {
        atomicMin(V.bad, i);
        __threadfence();
    }
    return ok;
}

// does *bad name a row that an earlier launch refused?
__device__ __forceinline__ bool dilu4f_stopped(const Dilu4FactorView& V, int p0)
{
    const int b = __hip_atomic_load(V.bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return b != kDiluBadNone && V.fpos[b] < p0;
}

// one wide level: forward positions [p0, p1), 16 block rows per workgroup
__global__ __launch_bounds__(kWG) void dilu4f_level(Dilu4FactorView V, int p0, int p1)
{
    if (dilu4f_stopped(V, p0)) return;
    const long long g = (long long)blockIdx.x * kWG + threadIdx.x;
    const long long q = p0 + (g >> 4);
    if (q >= p1) return; // whole groups leave together
    dilu4f_row(V, (int)q, (int)(g & 15));
}

// a run of narrow levels [l0, l1) in ONE workgroup; the barrier orders a level's stores before the next level's loads (same CU)
// and carries the refusal vote
__global__ __launch_bounds__(kDiluFactorFoldedWG) void dilu4f_folded(Dilu4FactorView V, int l0, int l1)
{
    if (dilu4f_stopped(V, V.lev_ptr[l0])) return; // the same answer in every thread: this workgroup's own rows lie at >= p0
    const int slot = threadIdx.x >> 4, e = threadIdx.x & 15;
    for (int l = l0; l < l1; l++) {
        const int q = V.lev_ptr[l] + slot;
        int refused = 0;
        if (q < V.lev_ptr[l + 1]) refused = !dilu4f_row(V, q, e);
        __threadfence_block();
        const int stop = __syncthreads_or(refused);
        __threadfence_block(); // the vote's barrier fences the LDS only: nothing of the next level is loaded ahead of it
        if (stop) return;
    }
}

} // namespace mi355
