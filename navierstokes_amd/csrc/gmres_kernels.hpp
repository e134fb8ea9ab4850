// gmres_kernels.hpp — the device side of mi_gmres_* (capi_gmres.hip) that the library did not have yet: the residual of a cycle's
// start with the first stage of its norm in one pass, and the small least-squares problem of restarted GMRES (Givens rotations,
// the residual recurrence, the back-substitution) as one-workgroup kernels, so that a cycle never needs the host for arithmetic;
// and round_f32_kernel, which normalises, rounds and stores a vector of the single-precision basis (MI_BASIS_F32) in one pass.
// For a cycle enqueued whole (mi_gmres_cycle_dev, mi_gmres_plan_*) the counted steps are a device-side value: the step kernel stops
// counting at maxiter, gmres_backsolve_counted reads k from the record and gmres_update_x updates x only when a step was counted.
// The ARITHMETIC below is part of the interface (include/mi355_spmv.h, mi_gmres_*; tests/gmres_dev_model.py restates
// it in numpy scalars): every product and every sum of the small problem is rounded on its own, nothing is contracted into an fma.
#pragma once
#include "blas1_kernels.hpp"
#include "blas1_multi.hpp"
#include "gmres_record.hpp"

namespace mi355 {

// ---- the small state of a solve, in device memory (doubles; m = restart) --------------------------------------------------------
//   [0, 8)                 the 64-byte record the host reads back (GmresRecord)
//   [8, 8 + m)             hcyc: the history entry of every counted step of the current cycle
//   then  hraw [m (m + 2)] raw Gram-Schmidt columns, mi_krylov_basis_cgs_dev's layout: column k at k (m + 2), the norm at j = k + 1
//         R    [m m]       the rotated columns, column-major: R_jk at j + k m
//         cs, sn [m] each, g [m + 1], y [m], then two scalars: ||b|| as mi_norm2_dev wrote it, the cycle's ||r0||
// (GmresRecord, kGmresMetAtStart and kGmresRecDoubles: gmres_record.hpp, shared with the host loop of gmres_drive.hpp)

struct GmresSmall {
    int m;
    double* base;
    __host__ __device__ GmresRecord* rec() const { return reinterpret_cast<GmresRecord*>(base); }
    __host__ __device__ double* hcyc() const { return base + kGmresRecDoubles; }
    __host__ __device__ double* hraw() const { return hcyc() + m; }
    __host__ __device__ double* R() const { return hraw() + (size_t)m * (m + 2); }
    __host__ __device__ double* cs() const { return R() + (size_t)m * m; }
    __host__ __device__ double* sn() const { return cs() + m; }
    __host__ __device__ double* g() const { return sn() + m; }
    __host__ __device__ double* y() const { return g() + m + 1; }
    __host__ __device__ double* bnorm() const { return y() + m; }
    __host__ __device__ double* beta() const { return bnorm() + 1; }
    static size_t doubles(int m) { return kGmresRecDoubles + (size_t)m + (size_t)m * (m + 2) + (size_t)m * m + 4 * (size_t)m + 1 + 2; }
};

// r = b - w (one rounded subtraction per entry) and the stage-1 partials of r . r in reduce_stage1<0>'s geometry: the same segments,
// the same lane chain s = fma(r, r, s) over the same pairs, the 16-byte and the 8-byte path — reduce_stage2<1> over the partials
// yields the bits of mi_norm2_dev(r).  One pass in place of copy + AXPY + the norm's first stage.
template <bool NT>
__global__ __launch_bounds__(kRedWG) void gmres_residual(int n, int seg, const double* __restrict__ b, const double* __restrict__ w,
                                                         double* __restrict__ r, double* __restrict__ partial)
{
    __shared__ double s_part[4];
    const long long lo = (long long)blockIdx.x * seg;
    const long long hi = (lo + seg < n) ? lo + seg : n;
    double s = 0.0;
    const bool aligned = (((uintptr_t)b | (uintptr_t)w | (uintptr_t)r) & 15) == 0;
    if (aligned) {
        for (long long i = lo + 2 * threadIdx.x; i + 1 < hi; i += 2 * kRedWG) {
            const double2 bv = ld2_stream<NT>(b + i);
            const double2 wv = ld2_stream<NT>(w + i);
            d2v_ rv;
            rv.x = __dsub_rn(bv.x, wv.x);
            rv.y = __dsub_rn(bv.y, wv.y);
            s = fma(rv.x, rv.x, s);
            s = fma(rv.y, rv.y, s);
            if (NT) __builtin_nontemporal_store(rv, reinterpret_cast<d2v_*>(r + i));
            else *reinterpret_cast<d2v_*>(r + i) = rv;
        }
    } else { // 8-byte-aligned bases: the same pairs in the same order through scalar accesses
        for (long long i = lo + 2 * threadIdx.x; i + 1 < hi; i += 2 * kRedWG) {
            const double r0 = __dsub_rn(ld1_stream<NT>(b + i), ld1_stream<NT>(w + i));
            const double r1 = __dsub_rn(ld1_stream<NT>(b + i + 1), ld1_stream<NT>(w + i + 1));
            s = fma(r0, r0, s);
            s = fma(r1, r1, s);
            if (NT) {
                __builtin_nontemporal_store(r0, r + i);
                __builtin_nontemporal_store(r1, r + i + 1);
            } else {
                r[i] = r0;
                r[i + 1] = r1;
            }
        }
    }
    // odd tail element of the segment (only the last segment can have one)
    if (((hi - lo) & 1) && threadIdx.x == 0) {
        const double rv = __dsub_rn(b[hi - 1], w[hi - 1]);
        s = fma(rv, rv, s);
        r[hi - 1] = rv;
    }
    const double t = block_sum(s, s_part);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// The float basis (MI_BASIS_F32; mi_round_f32_dev): out32[i] = round32(x[i] / *div) — the IEEE division (DIV) and the conversion,
// to nearest even, subnormals kept, beyond the float range +-Inf — and out64[i] = widen(out32[i]) where out64 is given, in one pass:
// what div_by_scalar_kernel is to the double basis, with the stored vector and the one the next product reads written together.
// Elementwise, so the bits do not depend on the path: pairs (16-byte load, 8-byte and 16-byte store) where the three bases allow
// them, else scalars.  out64 may be x itself (every element is read before it is written, by the same lane).
template <bool DIV>
__global__ __launch_bounds__(256) void round_f32_kernel(int n, const double* x, const double* __restrict__ div, float* __restrict__ out32,
                                                        double* out64)
{
    const double q = DIV ? div[0] : 1.0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool pairs = ((((uintptr_t)x | (uintptr_t)out64) & 15) | ((uintptr_t)out32 & 7)) == 0;
    if (pairs) {
        const long long n2 = n >> 1;
        for (long long i = t; i < n2; i += stride) {
            const double2 v = reinterpret_cast<const double2*>(x)[i];
            f2v_ f;
            f.x = (float)(DIV ? __ddiv_rn(v.x, q) : v.x);
            f.y = (float)(DIV ? __ddiv_rn(v.y, q) : v.y);
            reinterpret_cast<f2v_*>(out32)[i] = f;
            if (out64) reinterpret_cast<double2*>(out64)[i] = make_double2((double)f.x, (double)f.y);
        }
        if ((n & 1) && t == 0) {
            const float f = (float)(DIV ? __ddiv_rn(x[n - 1], q) : x[n - 1]);
            out32[n - 1] = f;
            if (out64) out64[n - 1] = (double)f;
        }
    } else {
        for (long long i = t; i < n; i += stride) {
            const float f = (float)(DIV ? __ddiv_rn(x[i], q) : x[i]);
            out32[i] = f;
            if (out64) out64[i] = (double)f;
        }
    }
}

// The start of a cycle, behind the residual's norm (one thread): beta and ||b|| into the record, g_0 = beta, the cycle's step count
// cleared, and the three reasons a solve ends at a cycle's start, in mpk.GMRES's order: beta / bnorm <= rtol, its >= maxiter, beta not
// finite.  first: the start of a solve (its = 0, and ||b|| = 0 becomes 1).
static __global__ __launch_bounds__(64) void gmres_cycle_begin(GmresSmall S, int first, double rtol, int maxiter)
{
#pragma clang fp contract(off) // every operator below is one rounded operation: nothing is fused (the __d*_rn intrinsics would be
                               // inlined with their own header's setting and fused all the same)
    if (threadIdx.x) return;
    GmresRecord* rec = S.rec();
    const double beta = S.beta()[0];
    double bn = S.bnorm()[0];
    if (first) {
        if (bn == 0.0) bn = 1.0;
        rec->its = 0;
        rec->bnorm = bn;
    } else {
        bn = rec->bnorm;
    }
    const double rel = (beta / bn);
    int reason = 0;
    if (rel <= rtol) reason = rec->its == 0 ? kGmresMetAtStart : 1;
    else if (rec->its >= maxiter) reason = 2;
    else if (!isfinite(beta)) reason = 4;
    rec->k = 0;
    rec->reason = reason;
    rec->beta = beta;
    rec->rel0 = rel;
    if (first) rec->last = rel;
    S.g()[0] = beta;
}

// Step k of the small problem, behind the step's Gram-Schmidt (one wave; lane 0 walks the rotation chain, which is serial by nature;
// the lanes move the column): the rotations 0..k-1 applied to a copy of raw column k, the new rotation, R's column, g, the history
// entry, the stopping rule.  FROZEN STATE: once the record holds a reason every later launch of the cycle returns at once.  A step
// at its >= maxiter returns at once too and writes no reason: a cycle enqueued whole (mi_gmres_cycle_dev) cannot be clipped by the
// host, and mi_gmres_solve_dev, which clips its batches, never launches such a step.
static __global__ __launch_bounds__(64) void gmres_hess_step(GmresSmall S, int k, double rtol, int maxiter)
{
#pragma clang fp contract(off) // every operator below is one rounded operation: nothing is fused (the __d*_rn intrinsics would be
                               // inlined with their own header's setting and fused all the same)
    __shared__ double c[kMultiMax + 2], s_cs[kMultiMax], s_sn[kMultiMax];
    GmresRecord* rec = S.rec();
    if (rec->reason != 0 || rec->its >= maxiter) return; // (uniform: every lane reads the same words, and nothing below writes them before the barrier)
    const int m = S.m, lane = threadIdx.x;
    const double* col = S.hraw() + (size_t)k * (m + 2);
    for (int j = lane; j <= k + 1; j += 64) c[j] = col[j];
    for (int j = lane; j < k; j += 64) s_cs[j] = S.cs()[j], s_sn[j] = S.sn()[j];
    __syncthreads();
    __shared__ int s_ok;
    if (lane == 0) {
        for (int j = 0; j < k; j++) {
            const double t = s_cs[j] * c[j] + s_sn[j] * c[j + 1];
            c[j + 1] = (-s_sn[j]) * c[j] + s_cs[j] * c[j + 1];
            c[j] = t;
        }
        const double nrm = c[k + 1];
        const double rho = sqrt(c[k] * c[k] + nrm * nrm);
        if (rho == 0.0 || !isfinite(rho)) {
            rec->reason = 4; // the step is not counted
            s_ok = 0;
        } else {
            const double csk = c[k] / rho, snk = nrm / rho;
            S.cs()[k] = csk;
            S.sn()[k] = snk;
            c[k] = rho;
            double* g = S.g();
            const double gk = g[k];
            const double gn = (-snk) * gk;
            g[k + 1] = gn;
            g[k] = csk * gk;
            const double h = fabs(gn) / rec->bnorm;
            S.hcyc()[k] = h;
            rec->last = h;
            rec->its += 1;
            rec->k = k + 1;
            if (h <= rtol) rec->reason = 1;
            else if (nrm == 0.0) rec->reason = 3;
            s_ok = 1;
        }
    }
    __syncthreads();
    if (s_ok)
        for (int j = lane; j <= k; j += 64) S.R()[j + (size_t)k * m] = c[j];
}

// The end of a cycle of k counted steps (one workgroup; the rows are serial by nature): R y = g by back-substitution, for
// i = k-1 .. 0: s = g_i, s = s - R_ij y_j for j = i+1 .. k-1 ascending, y_i = s / R_ii — each product, each difference and the
// division rounded once.  y stays in device memory: mi_maxpy_dev reads it there.
__device__ __forceinline__ void gmres_backsolve_body(const GmresSmall& S, int k)
{
#pragma clang fp contract(off) // every operator below is one rounded operation: nothing is fused (the __d*_rn intrinsics would be
                               // inlined with their own header's setting and fused all the same)
    __shared__ double sR[kMultiMax * kMultiMax], sy[kMultiMax];
    const int m = S.m;
    for (int e = threadIdx.x; e < k * k; e += blockDim.x) {
        const int j = e / k, i = e - j * k; // column j, row i
        sR[i + j * k] = S.R()[i + (size_t)j * m];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double* g = S.g();
        for (int i = k - 1; i >= 0; i--) {
            double s = g[i];
            for (int j = i + 1; j < k; j++) s = s - sR[i + j * k] * sy[j];
            sy[i] = (s / sR[i + i * k]);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < k; i += blockDim.x) S.y()[i] = sy[i];
}

static __global__ __launch_bounds__(256) void gmres_backsolve(GmresSmall S, int k)
{
    gmres_backsolve_body(S, k);
}

// ... with k read from the record (the end of a cycle enqueued whole: only the device knows how many steps were counted).  k == 0
// writes nothing.
static __global__ __launch_bounds__(256) void gmres_backsolve_counted(GmresSmall S)
{
    int k = S.rec()->k; // (uniform; nothing in this launch writes the record)
    k = k < 0 ? 0 : (k > S.m ? S.m : k);
    gmres_backsolve_body(S, k);
}

// x_i = fma(1, z_i, x_i), mi_axpy_dev's arithmetic, only when the cycle counted a step (rec->k > 0): with k == 0 the cycle's end
// leaves every bit of x alone, as the host-driven solve does by not launching the update.
static __global__ __launch_bounds__(256) void gmres_update_x(int n, const GmresRecord* __restrict__ rec, const double* __restrict__ z,
                                                             double* __restrict__ x)
{
    if (rec->k <= 0) return; // (uniform)
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if ((((uintptr_t)z | (uintptr_t)x) & 15) == 0) {
        const long long n2 = n >> 1;
        for (long long i = t; i < n2; i += stride) {
            const double2 zv = reinterpret_cast<const double2*>(z)[i];
            double2 xv = reinterpret_cast<double2*>(x)[i];
            xv.x = fma(1.0, zv.x, xv.x);
            xv.y = fma(1.0, zv.y, xv.y);
            reinterpret_cast<double2*>(x)[i] = xv;
        }
        if ((n & 1) && t == 0) x[n - 1] = fma(1.0, z[n - 1], x[n - 1]);
    } else {
        for (long long i = t; i < n; i += stride) x[i] = fma(1.0, z[i], x[i]);
    }
}

} // namespace mi355
