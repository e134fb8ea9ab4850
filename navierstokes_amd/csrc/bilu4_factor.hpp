// bilu4_factor.hpp — the numeric 4x4-block ILU(k) factorisation on the GPU (mi_bilu4dev_refactor): the IKJ factorisation that
// PETSc performs for the reference, in the row loop src/kernels/baij4_factor_avx2.c:114-170 is laid out as (that file is not run by
// the reference — nothing installs it — and does not compute it: its line 141 drops L . Dinv), written in place into the level-major
// device copies the solve reads (bilu4_solve.hpp).  Bit for bit the host factorisation of bilu4_plan.hpp ("ARITHMETIC" there): every product
// entry one chain from a rounded product, every update one rounded subtraction, pivots in ascending column order, an L block
// whose 16 entries all == 0.0 at its turn skipped, the Gauss-Jordan inverse in the order fixed there (rounded product, then
// rounded subtraction; 1/d a correctly rounded division; |d| < 1e-12 refused).  Compiled with -ffp-contract=off.
//
// Schedule: the forward sweep's — a row needs the finished rows of its L columns and nothing else.  A wide level is one launch,
// a run of narrow levels one launch of one workgroup with a barrier between levels.
//
// Lane layout: SIXTEEN lanes per block row; lane e = 4r + c owns entry (r, c) of every block of its row.  A lane therefore only
// ever reads back from its own row what it wrote itself, so program order suffices inside a row and nothing is fenced between
// pivots.  The row of w or of m that a product needs comes from the 16-lane group by cross-lane moves; the all-zero test is a
// vote over the group; the inversion runs in registers.  Another row's Dinv and U blocks were written by an earlier launch or,
// in a folded run, by other waves of the workgroup before a barrier: the factor arrays are read with plain loads and are
// deliberately NOT const __restrict__.
//
// Refused pivot: the refusing group does atomicMin on *bad with its block row.  The host stops after the first LEVEL with a
// refusal and reports the lowest row of that level; here a launch does nothing when *bad names a row of an EARLIER launch
// (fpos[*bad] < the launch's first position — a row of the launch's own levels must not stop its peers, or a lower row of the
// same level could go unreported), and a folded run leaves at the barrier that ends a level with a refusal.
#pragma once
#include "spmv_kernels.hpp"
#include "bilu4_plan.hpp"

namespace mi355 {

constexpr int kBiluBadNone = 0x7fffffff;  // *bad: no pivot refused
constexpr int kBiluFactorFoldedWG = 1024; // threads of the folded factor kernel: 16 lanes for each of up to 63 block rows

struct Bilu4FactorView {
    const int* fperm;         // [nb] forward position -> block row
    const int* fptr;          // [nb + 1] by forward position: the row's first L block
    const int* fcol;          // [nL] pivot column of every L block
    const int* bptr;          // [nb + 1] by backward position: the row's first U block
    const int* lev_ptr;       // forward levels
    const int* fpos;          // [nb] block row -> forward position
    const int* bpos;          // [nb] block row -> backward position
    const long long* upd_ptr; // [nL + 1]
    const int* upd;           // homes (index into L | U | D) or -1, see Bilu4DevPlan
    double* L;
    double* U;
    double* D;
    int nL, nU;
    int* bad;
};

__device__ __forceinline__ double* bilu4f_home(const Bilu4FactorView& V, int h)
{
    return h < V.nL ? V.L + 16 * (size_t)h : h < V.nL + V.nU ? V.U + 16 * (size_t)(h - V.nL) : V.D + 16 * (size_t)(h - V.nL - V.nU);
}

// clear and scatter in one pass over the factor: 16 lanes per block, every block of L | U | D written once; also resets *bad
__global__ __launch_bounds__(kWG) void bilu4f_gather(Bilu4FactorView V, const int* __restrict__ gather, long long total,
                                                     const double* __restrict__ coef, int colmajor)
{
    const long long g = (long long)blockIdx.x * kWG + threadIdx.x;
    if (g == 0) *V.bad = kBiluBadNone;
    const long long h = g >> 4;
    if (h >= total) return;
    const int e = (int)(g & 15);
    const int src = gather[h];
    const double v = src < 0 ? 0.0 : coef[16 * (size_t)src + (colmajor ? 4 * (e & 3) + (e >> 2) : e)];
    bilu4f_home(V, (int)h)[e] = v;
}

// one block row by its 16-lane group (e: the lane's entry); false: its pivot was refused.  All 16 lanes run it together.
__device__ __forceinline__ bool bilu4f_row(const Bilu4FactorView& V, int q, int e)
{
    const int r4 = e & 12, c = e & 3;
    const int shift = threadIdx.x & 48; // the group's place in its wave
    const int i = V.fperm[q];
    for (int lk = V.fptr[q]; lk < V.fptr[q + 1]; lk++) {
        double* wk = V.L + 16 * (size_t)lk + e;
        const double w = *wk;
        // !(all 16 == 0.0): a NaN is not zero, -0.0 is
        if (((__ballot(w != 0.0) >> shift) & 0xffffull) == 0) continue;
        const int bp = V.bpos[V.fcol[lk]];
        const double* dp = V.D + 16 * (size_t)bp + c;
        double m = __dmul_rn(__shfl(w, r4, 16), dp[0]);
        m = fma(__shfl(w, r4 + 1, 16), dp[4], m);
        m = fma(__shfl(w, r4 + 2, 16), dp[8], m);
        m = fma(__shfl(w, r4 + 3, 16), dp[12], m);
        *wk = m;
        const int u0 = V.bptr[bp], u1 = V.bptr[bp + 1];
        if (u0 == u1) continue;
        const double m0 = __shfl(m, r4, 16), m1 = __shfl(m, r4 + 1, 16), m2 = __shfl(m, r4 + 2, 16), m3 = __shfl(m, r4 + 3, 16);
        const int* at = V.upd + V.upd_ptr[lk];
        const double* uc = V.U + c;
        const int last = u1 - 1;
        // one block of look-ahead: row p is finished, so its U blocks never alias what this row stores
        int h = at[0];
        const double* un = uc + 16 * (size_t)u0;
        double b0 = un[0], b1 = un[4], b2 = un[8], b3 = un[12];
        for (int kk = u0; kk < u1; kk++) {
            const int hc = h;
            const double c0 = b0, c1 = b1, c2 = b2, c3 = b3;
            const int nx = min(kk + 1, last);
            h = at[nx - u0];
            un = uc + 16 * (size_t)nx;
            b0 = un[0], b1 = un[4], b2 = un[8], b3 = un[12];
            if (hc < 0) continue;
            double pr = __dmul_rn(m0, c0);
            pr = fma(m1, c1, pr);
            pr = fma(m2, c2, pr);
            pr = fma(m3, c3, pr);
            double* t = bilu4f_home(V, hc) + e;
            *t = __dsub_rn(*t, pr);
        }
    }
    // the diagonal block, inverted in registers
    double* di = V.D + 16 * (size_t)V.bpos[i] + e;
    double a = *di;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double d = __shfl(a, 5 * k, 16);
        if (fabs(d) < kBiluPivotMin) {
            ok = false;
            break;
        }
        const double piv = __ddiv_rn(1.0, d);
        if (e == 5 * k) a = 1.0;
        if (r4 == 4 * k) a = __dmul_rn(a, piv);
        const double f = __shfl(a, r4 + k, 16);    // a[r][k], before it is zeroed
        const double akc = __shfl(a, 4 * k + c, 16); // a[k][c], scaled
        if (r4 != 4 * k) a = __dsub_rn(c == k ? 0.0 : a, __dmul_rn(f, akc));
    }
    *di = a;
    if (!ok && e == 0) {
        atomicMin(V.bad, i);
        __threadfence();
    }
    return ok;
}

// does *bad name a row that an earlier launch refused?
__device__ __forceinline__ bool bilu4f_stopped(const Bilu4FactorView& V, int p0)
{
    const int b = __hip_atomic_load(V.bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return b != kBiluBadNone && V.fpos[b] < p0;
}

// one wide level: forward positions [p0, p1), 16 block rows per workgroup
__global__ __launch_bounds__(kWG) void bilu4f_level(Bilu4FactorView V, int p0, int p1)
{
    if (bilu4f_stopped(V, p0)) return;
    const long long g = (long long)blockIdx.x * kWG + threadIdx.x;
    const long long q = p0 + (g >> 4);
    if (q >= p1) return; // whole groups leave together
    bilu4f_row(V, (int)q, (int)(g & 15));
}

// a run of narrow levels [l0, l1) in ONE workgroup; the barrier orders a level's stores before the next level's loads (same CU)
// and carries the refusal vote
__global__ __launch_bounds__(kBiluFactorFoldedWG) void bilu4f_folded(Bilu4FactorView V, int l0, int l1)
{
    if (bilu4f_stopped(V, V.lev_ptr[l0])) return; // the same answer in every thread: this workgroup's own rows lie at >= p0
    const int slot = threadIdx.x >> 4, e = threadIdx.x & 15;
    for (int l = l0; l < l1; l++) {
        const int q = V.lev_ptr[l] + slot;
        int refused = 0;
        if (q < V.lev_ptr[l + 1]) refused = !bilu4f_row(V, q, e);
        __threadfence_block();
        const int stop = __syncthreads_or(refused);
        __threadfence_block(); // the vote's barrier fences the LDS only: nothing of the next level is loaded ahead of it
        if (stop) return;
    }
}

} // namespace mi355
