// blas1_multi.hpp — the vector half of one GMRES iteration against a whole basis at once: VecMDot / VecMAXPY of the reference's
// solver (src/solve_newton.c:1265, inside KSPSolve) and the classical Gram-Schmidt pass built from them.  blas1_kernels.hpp's
// sweep (mgs_step_kernel) reads y once per basis vector, 32 bytes per element and vector in m + 1 launches; here y is read once
// per TILE basis vectors: 8 (TILE + 1) / TILE bytes per element and vector for the dots, 8 (TILE + 2) / TILE for the update.
//
// Nothing here has a summation tree of its own.  Segments, lane pairs, block_sum and finish_sum are those of reduce_stage1 /
// reduce_stage2, every column keeps a private accumulator, and the update is a per-element fma chain in basis order, so that
//   column j of mdot_stage1's partials  ==  reduce_stage1<0>'s partials of (y, v_j)
//   maxpy_kernel's y                    ==  m successive axpy_kernel launches
//   maxpy_kernel<.., NORM>'s partials   ==  reduce_stage1<0>'s partials of (y_new, y_new)
// bit for bit, whatever TILE, the alignment, the stream or the non-temporal choice: the oracle's models of dot, norm2 and axpy
// (oracle/cpu_ref.c) describe these kernels as they stand.
//
// FLOAT BASIS (mi_*_f32_dev; include/mi355_spmv.h, MI_BASIS_F32): the same kernels with T = float for the basis vectors.  A lane
// takes its pair of basis entries with ONE 8-byte load where the double kernel takes 16 bytes, widens it in registers (exact) and
// goes on as above: y, the accumulators and every fma are double, so the float instantiation on V32 has the bits of the double
// instantiation on widen(V32).  A float pair is 8-byte aligned whenever its vector is (the host checks that), whatever y's
// alignment: both y paths load it the same way.
#pragma once
#include "blas1_kernels.hpp"

namespace mi355 {

constexpr int kMultiMax = 64; // basis vectors per call (= the bound of mi_krylov_basis_dev's s)

// The basis pointers of one call, by value in the kernel arguments: no device-side table, nothing allocated or copied per call,
// safe under stream capture.  Workgroups of chunk c (blockIdx.y, or `first` / TILE) use v[c * TILE ...].
template <typename T>
struct MultiVecT {
    const T* v[kMultiMax];
};
using MultiVec = MultiVecT<double>;
using MultiVecF32 = MultiVecT<float>;

typedef float f2v_ __attribute__((ext_vector_type(2)));
// One lane's pair of basis entries as doubles.  double: 16 bytes on the aligned path, two scalar loads on the other; float: one
// 8-byte load on either path, widened exactly.
template <bool NT, bool ALIGNED>
__device__ __forceinline__ double2 ld_pair(const double* p)
{
    if (ALIGNED) return ld2_stream<NT>(p);
    return make_double2(ld1_stream<NT>(p), ld1_stream<NT>(p + 1));
}
template <bool NT, bool ALIGNED>
__device__ __forceinline__ double2 ld_pair(const float* p)
{
    const f2v_ v = NT ? __builtin_nontemporal_load(reinterpret_cast<const f2v_*>(p)) : *reinterpret_cast<const f2v_*>(p);
    return make_double2((double)v.x, (double)v.y);
}
// what a basis vector's address adds to the test for the 16-byte path: a float vector's nothing (y alone decides)
__device__ __forceinline__ uintptr_t align_bits(const double* p) { return (uintptr_t)p; }
__device__ __forceinline__ uintptr_t align_bits(const float*) { return 0; }

template <bool NT>
__device__ __forceinline__ void st2_stream(double* p, double2 v)
{
    if (NT) {
        d2v_ w;
        w.x = v.x;
        w.y = v.y;
        __builtin_nontemporal_store(w, reinterpret_cast<d2v_*>(p));
    } else {
        *reinterpret_cast<double2*>(p) = v;
    }
}
template <bool NT>
__device__ __forceinline__ void st1_stream(double* p, double v)
{
    if (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// CNT dots y . v[j] over this workgroup's segment: reduce_stage1<0>'s loop with one accumulator per column.
template <int CNT, bool NT, typename T>
__device__ __forceinline__ void mdot_body(int n, int seg, const double* __restrict__ y, const MultiVecT<T>& B, int first,
                                          double* __restrict__ partial, double* s_part)
{
    const long long lo = (long long)blockIdx.x * seg;
    const long long hi = (lo + seg < n) ? lo + seg : n;
    const T* v[CNT];
    double acc[CNT];
    uintptr_t bits = (uintptr_t)y;
#pragma unroll
    for (int j = 0; j < CNT; j++) {
        v[j] = B.v[first + j];
        acc[j] = 0.0;
        bits |= align_bits(v[j]);
    }
    if ((bits & 15) == 0) {
        for (long long i = lo + 2 * threadIdx.x; i + 1 < hi; i += 2 * kRedWG) {
            double2 vv[CNT];
            const double2 yv = ld2_stream<NT>(y + i);
#pragma unroll
            for (int j = 0; j < CNT; j++) vv[j] = ld_pair<NT, true>(v[j] + i); // every load of the iteration is in flight before the first fma
#pragma unroll
            for (int j = 0; j < CNT; j++) {
                acc[j] = fma(yv.x, vv[j].x, acc[j]);
                acc[j] = fma(yv.y, vv[j].y, acc[j]);
            }
        }
    } else { // a base that is only 8-byte aligned: the same pairs in the same order through scalar loads
        for (long long i = lo + 2 * threadIdx.x; i + 1 < hi; i += 2 * kRedWG) {
            double v0[CNT], v1[CNT];
            const double y0 = ld1_stream<NT>(y + i), y1 = ld1_stream<NT>(y + i + 1);
#pragma unroll
            for (int j = 0; j < CNT; j++) {
                const double2 p = ld_pair<NT, false>(v[j] + i);
                v0[j] = p.x;
                v1[j] = p.y;
            }
#pragma unroll
            for (int j = 0; j < CNT; j++) {
                acc[j] = fma(y0, v0[j], acc[j]);
                acc[j] = fma(y1, v1[j], acc[j]);
            }
        }
    }
    // odd tail element of the segment (only the last segment can have one)
    if (((hi - lo) & 1) && threadIdx.x == 0) {
        const double yv = y[hi - 1];
#pragma unroll
        for (int j = 0; j < CNT; j++) acc[j] = fma(yv, (double)v[j][hi - 1], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < CNT; j++) {
        const double t = block_sum(acc[j], s_part);
        if (threadIdx.x == 0) partial[(size_t)(first + j) * kMaxPartials + blockIdx.x] = t;
    }
}

// the body compiled for the chunk's vector count (uniform): no predicated loads, no dead columns
template <int C, bool NT, typename T>
__device__ __forceinline__ void mdot_dispatch(int cnt, int n, int seg, const double* y, const MultiVecT<T>& B, int first, double* partial,
                                              double* s_part)
{
    if (cnt == C) mdot_body<C, NT, T>(n, seg, y, B, first, partial, s_part);
    else if constexpr (C > 1) mdot_dispatch<C - 1, NT, T>(cnt, n, seg, y, B, first, partial, s_part);
}

// partial[j * kMaxPartials + g] = (y . v_j) over segment g, for the m vectors of B in chunks of TILE: grid (np, chunks), the
// geometry of reduce_stage1 in x.  y is read once per chunk.
template <int TILE, bool NT, typename T>
__global__ __launch_bounds__(kRedWG) void mdot_stage1(int n, int seg, int m, const double* __restrict__ y, const MultiVecT<T> B,
                                                      double* __restrict__ partial)
{
    __shared__ double s_part[4];
    const int first = blockIdx.y * TILE;
    const int cnt = (m - first < TILE) ? m - first : TILE;
    mdot_dispatch<TILE, NT, T>(cnt, n, seg, y, B, first, partial, s_part);
}

// One workgroup per column: the finishing tree of reduce_stage2<0> over that column's partials.  accum != nullptr: also
// accum[j] = accum[j] + dots[j], ONE rounded add (the Hessenberg entry of a second Gram-Schmidt pass).
static __global__ __launch_bounds__(kRedWG) void mdot_stage2(int np, const double* __restrict__ partial, double* __restrict__ dots,
                                                      double* __restrict__ accum)
{
    __shared__ double s_part[4];
    const int j = blockIdx.x;
    const double t = finish_sum(np, partial + (size_t)j * kMaxPartials, s_part);
    if (threadIdx.x == 0) {
        dots[j] = t;
        if (accum) accum[j] = accum[j] + t;
    }
}

// y[i] <- fma(a_{CNT-1}, v_{CNT-1}[i], ... fma(a_0, v_0[i], y[i])) over this workgroup's segment; NORM: the segment's partial
// of sum y_new^2 in reduce_stage1's order.
template <int CNT, bool NT, bool NORM, typename T>
__device__ __forceinline__ void maxpy_body(int n, int seg, const double* __restrict__ coef, int negate, const MultiVecT<T>& B, int first,
                                           double* y, double* __restrict__ partial, double* s_part)
{
    const long long lo = (long long)blockIdx.x * seg;
    const long long hi = (lo + seg < n) ? lo + seg : n;
    const T* v[CNT];
    double a[CNT];
    uintptr_t bits = (uintptr_t)y;
#pragma unroll
    for (int j = 0; j < CNT; j++) {
        v[j] = B.v[first + j];
        const double c = coef[first + j];
        a[j] = negate ? -c : c;
        bits |= align_bits(v[j]);
    }
    double s = 0.0;
    if ((bits & 15) == 0) {
        for (long long i = lo + 2 * threadIdx.x; i + 1 < hi; i += 2 * kRedWG) {
            double2 vv[CNT];
            double2 t = ld2_stream<NT>(y + i);
#pragma unroll
            for (int j = 0; j < CNT; j++) vv[j] = ld_pair<NT, true>(v[j] + i);
#pragma unroll
            for (int j = 0; j < CNT; j++) {
                t.x = fma(a[j], vv[j].x, t.x);
                t.y = fma(a[j], vv[j].y, t.y);
            }
            st2_stream<NT>(y + i, t);
            if (NORM) {
                s = fma(t.x, t.x, s);
                s = fma(t.y, t.y, s);
            }
        }
    } else {
        for (long long i = lo + 2 * threadIdx.x; i + 1 < hi; i += 2 * kRedWG) {
            double v0[CNT], v1[CNT];
            double t0 = ld1_stream<NT>(y + i), t1 = ld1_stream<NT>(y + i + 1);
#pragma unroll
            for (int j = 0; j < CNT; j++) {
                const double2 p = ld_pair<NT, false>(v[j] + i);
                v0[j] = p.x;
                v1[j] = p.y;
            }
#pragma unroll
            for (int j = 0; j < CNT; j++) {
                t0 = fma(a[j], v0[j], t0);
                t1 = fma(a[j], v1[j], t1);
            }
            st1_stream<NT>(y + i, t0);
            st1_stream<NT>(y + i + 1, t1);
            if (NORM) {
                s = fma(t0, t0, s);
                s = fma(t1, t1, s);
            }
        }
    }
    if (((hi - lo) & 1) && threadIdx.x == 0) {
        double t = y[hi - 1];
#pragma unroll
        for (int j = 0; j < CNT; j++) t = fma(a[j], (double)v[j][hi - 1], t);
        y[hi - 1] = t;
        if (NORM) s = fma(t, t, s);
    }
    if (NORM) {
        const double p = block_sum(s, s_part);
        if (threadIdx.x == 0) partial[blockIdx.x] = p;
    }
}

template <int C, bool NT, bool NORM, typename T>
__device__ __forceinline__ void maxpy_dispatch(int cnt, int n, int seg, const double* coef, int negate, const MultiVecT<T>& B, int first,
                                               double* y, double* partial, double* s_part)
{
    if (cnt == C) maxpy_body<C, NT, NORM, T>(n, seg, coef, negate, B, first, y, partial, s_part);
    else if constexpr (C > 1) maxpy_dispatch<C - 1, NT, NORM, T>(cnt, n, seg, coef, negate, B, first, y, partial, s_part);
}

// One chunk of cnt <= TILE vectors, B.v[first ...] with coef[first ...] (device memory: no host round trip after the dots):
// grid np, the geometry of reduce_stage1.  A longer basis is one launch per chunk, the chain continued from the stored y (a
// store and a reload are exact).  NORM (the last chunk): partial[g] as reduce_stage1<0> would write for (y_new, y_new), so that
// reduce_stage2<1> gives mi_norm2_dev's bits without reading y again.
template <int TILE, bool NT, bool NORM, typename T>
__global__ __launch_bounds__(kRedWG) void maxpy_kernel(int n, int seg, int first, int cnt, const double* __restrict__ coef, int negate,
                                                       const MultiVecT<T> B, double* y, double* __restrict__ partial)
{
    __shared__ double s_part[4];
    maxpy_dispatch<TILE, NT, NORM, T>(cnt, n, seg, coef, negate, B, first, y, partial, s_part);
}

// The same chunk with the vector count in DEVICE memory (mi_maxpy_upto*_dev: the update of a captured GMRES cycle, whose counted
// steps only the device knows): c = *count clamped to [0, m], and this launch takes the vectors first .. min(first + TILE, c) - 1.
// The host always launches ceil(m / TILE) chunks; one that starts at or past c returns at once (uniform: every lane reads the same
// word) and has loaded no vector, no coefficient and no y.  What runs is maxpy_kernel's body on maxpy_kernel's geometry, so y has
// the bits of mi_maxpy*_dev(n, c, ..) and is not touched at all when c == 0.
template <int TILE, bool NT, typename T>
__global__ __launch_bounds__(kRedWG) void maxpy_upto_kernel(int n, int seg, int first, int m, const int* __restrict__ count,
                                                            const double* __restrict__ coef, int negate, const MultiVecT<T> B, double* y)
{
    __shared__ double s_part[4];
    int c = count[0];
    c = c < 0 ? 0 : (c > m ? m : c);
    const int cnt = (c - first < TILE) ? c - first : TILE;
    if (cnt <= 0) return;
    maxpy_dispatch<TILE, NT, false, T>(cnt, n, seg, coef, negate, B, first, y, nullptr, s_part);
}

} // namespace mi355
