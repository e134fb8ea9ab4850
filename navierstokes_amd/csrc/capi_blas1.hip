// capi_blas1.hip: dot, AXPY, orthogonalize, Gram-Schmidt sweep, norms — part of libmi355spmv.so (see capi_internal.hpp for the layout of the library).
// Built for gfx950 only; no CPU fallback anywhere: every compute entry point needs a HIP device.
#include "capi_internal.hpp"
#include "blas1_kernels.hpp"
#include "blas1_multi.hpp"
#include "gmres_kernels.hpp"

// Reduction workspace: partials of the two-stage reductions, one per (device, stream) so that
// reductions enqueued on different streams (or by different rank threads of one process) never share
// partials.  In units of K = kMaxPartials doubles: [0, 2K) the two partial arrays of a reduction (or the
// ping-pong pair of the Gram-Schmidt sweep, or the norm partials of mi_maxpy_dev), [2K, 4K) spare,
// [4K, 68K) one partial array per column of mi_mdot_dev, then kMultiMax doubles for the second-pass
// dots of mi_cgs_dev.  548 KB per stream that ever reduced; a destroyed stream's slot is simply reused
// if the runtime hands the same handle out again.
static std::map<std::pair<int, hipStream_t>, double*> g_ws;
constexpr size_t kWsMdot = 4 * (size_t)kMaxPartials;                         // the columns' partials
constexpr size_t kWsDots2 = kWsMdot + (size_t)kMultiMax * kMaxPartials;      // mi_cgs_dev: dots of the second pass
constexpr size_t kWsDoubles = kWsDots2 + kMultiMax + 8;

int get_ws(hipStream_t s, double** out)
{
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_mu);
    double*& w = g_ws[std::make_pair(dev, s)];
    if (!w) HIP_TRY(hipMalloc(&w, sizeof(double) * kWsDoubles));
    *out = w;
    return MI_OK;
}

// ---------------------------------------------------------------- BLAS-1
// large vectors are streamed past the caches (blas1_kernels.hpp); MI355_BLAS1_NT=0|1 forces the choice
static bool blas1_nt(int n)
{
    static const int forced = getenv("MI355_BLAS1_NT") ? atoi(getenv("MI355_BLAS1_NT")) : -1;
    return forced >= 0 ? forced != 0 : n >= kBlas1NtMin;
}

static int red_geometry(int n, int* np, int* seg)
{
    // segments of a multiple of 2*kRedWG elements, at most kMaxPartials of them
    long long s = ((long long)n + kMaxPartials - 1) / kMaxPartials;
    const int q = 2 * kRedWG;
    s = ((s + q - 1) / q) * q;
    if (s < q) s = q;
    *seg = (int)s;
    *np = (int)(((long long)n + s - 1) / s);
    if (*np < 1) *np = 1;
    return MI_OK;
}

template <int MODE, int FIN>
static int reduce_dev(int n, const double* a, const double* b, double* d_out, hipStream_t s)
{
    CHECK_ARG(n >= 0, "negative n");
    CHECK_ARG(d_out && (n == 0 || (a && b)), "null vector");
    double* ws = nullptr;
    int rc = get_ws(s, &ws);
    if (rc) return rc;
    int np, seg;
    red_geometry(n, &np, &seg);
    pick([&](auto NT) { hipLaunchKernelGGL((reduce_stage1<MODE, NT()>), dim3(np), dim3(kRedWG), 0, s, n, seg, a, b, ws, ws + kMaxPartials); }, blas1_nt(n));
    hipLaunchKernelGGL((reduce_stage2<FIN>), dim3(1), dim3(kRedWG), 0, s, np, ws, ws + kMaxPartials, d_out);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_dot_dev(int n, const double* d_x, const double* d_y, double* d_out, mi_stream_t s)
{
    return reduce_dev<0, 0>(n, d_x, d_y, d_out, (hipStream_t)s);
}

extern "C" int mi_norm2_dev(int n, const double* d_x, double* d_out, mi_stream_t s)
{
    return reduce_dev<0, 1>(n, d_x, d_x, d_out, (hipStream_t)s);
}

extern "C" int mi_rel_error_dev(int n, const double* d_ref, const double* d_test, double* d_out, mi_stream_t s)
{
    return reduce_dev<1, 2>(n, d_ref, d_test, d_out, (hipStream_t)s);
}

// r = b - w and ||r||_2 into d_out: the residual at the start of a GMRES cycle (gmres_kernels.hpp) in two launches, the norm with
// the bits of mi_norm2_dev(r).  n > 0, arguments checked by the caller (capi_gmres.hip)
int residual_norm_dev(int n, const double* d_b, const double* d_w, double* d_r, double* d_out, hipStream_t s)
{
    double* ws = nullptr;
    int rc = get_ws(s, &ws);
    if (rc) return rc;
    int np, seg;
    red_geometry(n, &np, &seg);
    pick([&](auto NT) { hipLaunchKernelGGL((gmres_residual<NT()>), dim3(np), dim3(kRedWG), 0, s, n, seg, d_b, d_w, d_r, ws); }, blas1_nt(n));
    hipLaunchKernelGGL((reduce_stage2<1>), dim3(1), dim3(kRedWG), 0, s, np, ws, ws + kMaxPartials, d_out);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_axpy_dev(int n, double a, const double* d_x, double* d_y, mi_stream_t s)
{
    CHECK_ARG(n >= 0, "negative n");
    CHECK_ARG(n == 0 || (d_x && d_y), "null vector");
    if (n == 0) return MI_OK;
    hipLaunchKernelGGL(axpy_kernel, dim3(launch_grid(n / 2, 256, 2048, 1)), dim3(256), 0, (hipStream_t)s, n, a, d_x, d_y);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_orthogonalize_dev(int n, const double* d_b, const double* d_x1, double* d_x3, double alpha,
                                    double* d_beta_out, mi_stream_t s_)
{
    CHECK_ARG(d_beta_out, "null beta");
    CHECK_ARG(n >= 0, "negative n");
    hipStream_t s = (hipStream_t)s_;
    if (n == 0) return reduce_dev<0, 0>(n, d_b, d_x1, d_beta_out, s); // beta = 0
    CHECK_ARG(d_b && d_x1 && d_x3, "null vector");
    // two kernels: per-workgroup partials of b.x1, then the update, whose workgroups each finish the dot themselves
    double* ws = nullptr;
    int rc = get_ws(s, &ws);
    if (rc) return rc;
    int np, seg;
    red_geometry(n, &np, &seg);
    const int grid = launch_grid(n, kRedWG, 2048);
    pick([&](auto NT) {
        hipLaunchKernelGGL((reduce_stage1<0, NT()>), dim3(np), dim3(kRedWG), 0, s, n, seg, d_b, d_x1, ws, ws + kMaxPartials);
        hipLaunchKernelGGL(ortho_update_kernel<NT()>, dim3(grid), dim3(kRedWG), 0, s, n, alpha, np, ws, d_beta_out, d_b, d_x1, d_x3);
    }, blas1_nt(n));
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

// the update of a distributed orthogonalize on one rank's slice: beta = sum of the ranks' partial dots in rank order (capi_dist.hip)
int ortho_update_from_parts(int n, int nparts, const double* parts, double alpha, const double* d_b, const double* d_x1, double* d_x3, double* d_beta_out,
                            hipStream_t s)
{
    CHECK_ARG(n >= 0 && nparts >= 1 && nparts <= 64 && parts, "bad argument");
    CHECK_ARG(n == 0 || (d_b && d_x1 && d_x3), "null vector");
    const int grid = launch_grid(n, kRedWG, 2048, 1);
    pick([&](auto NT) { hipLaunchKernelGGL(ortho_update_ranks_kernel<NT()>, dim3(grid), dim3(kRedWG), 0, s, n, alpha, nparts, parts, d_beta_out, d_b, d_x1, d_x3); }, blas1_nt(n));
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

// ---- product + dot in one pass (the f-4 pipeline SpMV -> dot + AXPY -> SpMV, mpk/SpMVmulti.cpp:563-569) -------------------
// y = A x with the partial sums of b . y accumulated in the product's epilogue where the launch can carry it (the LEAN ring
// kernel: ring_dot_eligible), else product and dot as separate launches — the same API either way.  *np = partials written to ws.
static int spmv_with_dot_partials(mi_csr_t A, const double* d_x, double* d_y, const double* d_b, hipStream_t s, double* ws, int* np)
{
    int rc;
    if (ring_dot_eligible(A)) {
        RingDot dt{d_b, ws};
        if ((rc = launch_spmv(A, d_x, d_y, s, true, nullptr, &dt))) return rc;
        *np = A->ring.wgs;
        return MI_OK;
    }
    if ((rc = launch_spmv(A, d_x, d_y, s))) return rc;
    int seg;
    red_geometry(A->n, np, &seg);
    pick([&](auto NT) { hipLaunchKernelGGL((reduce_stage1<0, NT()>), dim3(*np), dim3(kRedWG), 0, s, A->n, seg, d_b, d_y, ws, ws + kMaxPartials); }, blas1_nt(A->n));
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_csr_dot_epilogue_info(mi_csr_t A, int* in_epilogue)
{
    CHECK_ARG(A && in_epilogue, "null argument");
    *in_epilogue = ring_dot_eligible(A) ? 1 : 0;
    return MI_OK;
}

// what the ring kernel's DOT instantiation walks (spmv_ring.hpp): workgroup size, the blocks of each logical workgroup's run
// and the rows of each block — enough to restate its summation tree on the host
extern "C" int mi_csr_dot_epilogue_layout(mi_csr_t A, int* threads, int* wgs, int* nblk, int* run_first_block, int* block_row0,
                                          int* block_rows, int cap_runs, int cap_blocks)
{
    CHECK_ARG(A && threads && wgs && nblk, "null argument");
    if (!ring_dot_eligible(A)) return fail(MI_ERR_STATE, "this handle's launch does not carry the dot epilogue");
    const RingTable& R = A->ring;
    *threads = R.cfg.threads;
    *wgs = R.wgs;
    *nblk = R.nblk;
    if (!run_first_block && !block_row0 && !block_rows) return MI_OK;
    CHECK_ARG(cap_runs >= R.wgs + 1 && cap_blocks >= R.nblk, "arrays too short: need wgs + 1 run entries and nblk block entries");
    std::vector<int> rng((size_t)2 * R.wgs);
    if (R.uniform) {
        for (int g = 0; g < R.wgs; g++) {
            rng[2 * g] = std::min(R.nblk, g * R.bpw);
            rng[2 * g + 1] = std::min(R.nblk, (g + 1) * R.bpw);
        }
    } else {
        HIP_TRY(hipMemcpy(rng.data(), R.d_rng, sizeof(int) * rng.size(), hipMemcpyDeviceToHost));
    }
    for (int g = 0; g < R.wgs; g++) // the runs tile the blocks in order: one start per run and the end of the last
        if (rng[2 * g] != (g ? rng[2 * g - 1] : 0) || rng[2 * g + 1] < rng[2 * g])
            return fail(MI_ERR_STATE, "ring runs are not consecutive");
    if (R.wgs && rng[2 * R.wgs - 1] != R.nblk) return fail(MI_ERR_STATE, "ring runs do not cover every block");
    if (run_first_block) {
        for (int g = 0; g < R.wgs; g++) run_first_block[g] = rng[2 * g];
        run_first_block[R.wgs] = R.nblk;
    }
    if (block_row0 || block_rows) {
        std::vector<int> plan((size_t)8 * R.nblk);
        if (R.nblk) HIP_TRY(hipMemcpy(plan.data(), R.d_plan, sizeof(int) * plan.size(), hipMemcpyDeviceToHost));
        for (int b = 0; b < R.nblk; b++) {
            if (block_row0) block_row0[b] = plan[(size_t)8 * b];
            if (block_rows) block_rows[b] = plan[(size_t)8 * b + 2];
        }
    }
    return MI_OK;
}

extern "C" int mi_spmv_dot_dev(mi_csr_t A, const double* d_x, double* d_y, const double* d_b, double* d_beta_out, mi_stream_t s_)
{
    CHECK_ARG(A, "null handle");
    CHECK_ARG(d_beta_out, "null beta");
    CHECK_ARG(!A->mapped, "needs an unmapped matrix (b is indexed like y)");
    hipStream_t s = (hipStream_t)s_;
    if (A->n == 0) return reduce_dev<0, 0>(0, d_b, d_y, d_beta_out, s);
    CHECK_ARG(d_x && d_y && d_b, "null vector");
    double* ws = nullptr;
    int rc = get_ws(s, &ws), np = 0;
    if (rc) return rc;
    if ((rc = spmv_with_dot_partials(A, d_x, d_y, d_b, s, ws, &np))) return rc;
    hipLaunchKernelGGL((reduce_stage2<0>), dim3(1), dim3(kRedWG), 0, s, np, ws, ws + kMaxPartials, d_beta_out);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_spmv_orthogonalize_dev(mi_csr_t A, const double* d_x, double* d_x1, const double* d_b, double* d_x3, double alpha,
                                         double* d_beta_out, mi_stream_t s_)
{
    CHECK_ARG(A, "null handle");
    CHECK_ARG(d_beta_out, "null beta");
    CHECK_ARG(!A->mapped, "needs an unmapped matrix (b is indexed like y)");
    hipStream_t s = (hipStream_t)s_;
    const int n = A->n;
    if (n == 0) return reduce_dev<0, 0>(0, d_b, d_x1, d_beta_out, s);
    CHECK_ARG(d_x && d_x1 && d_b && d_x3, "null vector");
    double* ws = nullptr;
    int rc = get_ws(s, &ws), np = 0;
    if (rc) return rc;
    if ((rc = spmv_with_dot_partials(A, d_x, d_x1, d_b, s, ws, &np))) return rc;
    const int grid = launch_grid(n, kRedWG, 2048);
    pick([&](auto NT) { hipLaunchKernelGGL(ortho_update_kernel<NT()>, dim3(grid), dim3(kRedWG), 0, s, n, alpha, np, ws, d_beta_out, d_b, d_x1, d_x3); }, blas1_nt(n));
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_orthonormalize_against_basis_dev(int n, int m, const double* const* d_basis, double* d_y, double* d_dots,
                                                    mi_stream_t s_)
{
    CHECK_ARG(n >= 0 && m >= 0, "negative size");
    if (m == 0) return MI_OK;
    CHECK_ARG(d_basis && d_dots, "null basis / dots");
    hipStream_t s = (hipStream_t)s_;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_dots, 0, sizeof(double) * (size_t)m, s));
        return MI_OK;
    }
    CHECK_ARG(d_y, "null y");
    for (int j = 0; j < m; j++) CHECK_ARG(d_basis[j], "null basis vector");
    double* ws = nullptr;
    int rc = get_ws(s, &ws);
    if (rc) return rc;
    int np, seg;
    red_geometry(n, &np, &seg);
    double* part[2] = {ws, ws + kMaxPartials};
    // dot of the first vector, then one launch per vector: finish dot j, update y, partials of dot j+1
    pick([&](auto NT) {
        hipLaunchKernelGGL((reduce_stage1<0, NT()>), dim3(np), dim3(kRedWG), 0, s, n, seg, d_y, d_basis[0], part[0], part[1]);
        for (int j = 0; j < m; j++) {
            const double* vn = j + 1 < m ? d_basis[j + 1] : nullptr;
            hipLaunchKernelGGL(mgs_step_kernel<NT()>, dim3(np), dim3(kRedWG), 0, s, n, seg, np, part[j & 1], d_dots + j, d_basis[j], vn, d_y, part[(j + 1) & 1]);
        }
    }, blas1_nt(n));
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

// ---------------------------------------------------------------- VecMDot / VecMAXPY / classical Gram-Schmidt (blas1_multi.hpp)
// basis vectors per pass over y: a compile-time set {4, 8, 16}; the default is what tools/bench_orth.py measured fastest
// (profiles/NOTES.md), MI355_MDOT_TILE=4|8|16 forces another compiled value (the bits do not depend on it; other values are ignored)
#ifndef MI355_MDOT_TILE_DEFAULT
#define MI355_MDOT_TILE_DEFAULT 8
#endif
static int mdot_tile()
{
    static const int t = [] {
        const int e = getenv("MI355_MDOT_TILE") ? atoi(getenv("MI355_MDOT_TILE")) : 0;
        return (e == 4 || e == 8 || e == 16) ? e : MI355_MDOT_TILE_DEFAULT;
    }();
    return t;
}

// the float basis (mi_*_f32_dev): 8 or 16 vectors per pass; MI355_MDOT_TILE_F32=8|16 forces the other compiled value (the bits do not
// depend on it).  The default is what tools/bench_orth.py --basis f32 measured fastest (profiles/NOTES.md R13.1)
#ifndef MI355_MDOT_TILE_F32_DEFAULT
#define MI355_MDOT_TILE_F32_DEFAULT 8
#endif
static int mdot_tile_f32()
{
    static const int t = [] {
        const int e = getenv("MI355_MDOT_TILE_F32") ? atoi(getenv("MI355_MDOT_TILE_F32")) : 0;
        return (e == 8 || e == 16) ? e : MI355_MDOT_TILE_F32_DEFAULT;
    }();
    return t;
}
// fn(TILE) with the compiled tile of a basis of T: {4, 8, 16} for doubles, {8, 16} for floats (tile 4 is not instantiated for them)
template <typename T, class Fn>
static void with_multi_tile(Fn&& fn)
{
    if constexpr (sizeof(T) == 8) pick_int<4, 16, 8>(mdot_tile(), fn);
    else pick_int<16, 8>(mdot_tile_f32(), fn);
}

// the argument rules shared by mi_mdot_dev / mi_maxpy_dev / mi_cgs_dev and their float-basis twins; nothing here touches the device
template <typename T>
static int multi_check(int n, int m, const T* const* basis, const double* y)
{
    CHECK_ARG(n >= 0, "negative n");
    CHECK_ARG(m >= 0 && m <= kMultiMax, "m must be in 0..64");
    CHECK_ARG(m == 0 || basis, "null basis");
    if (n == 0) return MI_OK;
    CHECK_ARG(y, "null y");
    for (int j = 0; j < m; j++) {
        CHECK_ARG(basis[j], "null basis vector");
        CHECK_ARG((const void*)basis[j] != (const void*)y, "y is one of the basis vectors");
        if (sizeof(T) == 4) CHECK_ARG(((uintptr_t)basis[j] & 7) == 0, "a float basis vector is not 8-byte aligned (the kernels load pairs)");
    }
    return MI_OK;
}

// dots[j] = y . v_j (and accum[j] += dots[j] when accum is given); n > 0, m > 0, arguments checked
template <typename T>
static int mdot_run(int n, int m, const MultiVecT<T>& B, const double* y, double* d_dots, double* d_accum, double* ws, hipStream_t s)
{
    int np, seg;
    red_geometry(n, &np, &seg);
    const bool nt = blas1_nt(n);
    with_multi_tile<T>([&](auto TILE) {
        const dim3 grid(np, (m + TILE() - 1) / TILE());
        pick([&](auto NT) { hipLaunchKernelGGL((mdot_stage1<TILE(), NT(), T>), grid, dim3(kRedWG), 0, s, n, seg, m, y, B, ws + kWsMdot); }, nt);
    });
    hipLaunchKernelGGL(mdot_stage2, dim3(m), dim3(kRedWG), 0, s, np, ws + kWsMdot, d_dots, d_accum);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

// y <- y + sum a_j v_j and, when d_norm_out is given, the norm of the new y from the last chunk's partials; n > 0, m > 0
template <typename T>
static int maxpy_run(int n, int m, const double* d_coef, int negate, const MultiVecT<T>& B, double* y, double* d_norm_out, double* ws,
                     hipStream_t s)
{
    int np, seg;
    red_geometry(n, &np, &seg);
    const bool nt = blas1_nt(n), norm = d_norm_out != nullptr;
    with_multi_tile<T>([&](auto TILE) {
        for (int first = 0; first < m; first += TILE()) { // one chunk per launch: each continues the chain from the stored y
            const int cnt = std::min(TILE(), m - first);
            pick([&](auto NT, auto LAST) {
                hipLaunchKernelGGL((maxpy_kernel<TILE(), NT(), LAST(), T>), dim3(np), dim3(kRedWG), 0, s, n, seg, first, cnt, d_coef, negate, B, y, ws);
            }, nt, norm && first + TILE() >= m);
        }
    });
    if (norm) hipLaunchKernelGGL((reduce_stage2<1>), dim3(1), dim3(kRedWG), 0, s, np, ws, ws + kMaxPartials, d_norm_out);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

template <typename T>
static MultiVecT<T> multi_vec(int m, const T* const* basis)
{
    MultiVecT<T> B;
    for (int j = 0; j < kMultiMax; j++) B.v[j] = j < m ? basis[j] : nullptr;
    return B;
}

// mi_mdot_dev / mi_maxpy_dev / mi_cgs_dev and their float-basis twins: one body each, T the basis's element type
template <typename T>
static int mdot_dev(int n, int m, const T* const* d_basis, const double* d_y, double* d_dots, mi_stream_t s_)
{
    int rc = multi_check(n, m, d_basis, d_y);
    if (rc) return rc;
    if (m == 0) return MI_OK;
    CHECK_ARG(d_dots, "null dots");
    hipStream_t s = (hipStream_t)s_;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_dots, 0, sizeof(double) * (size_t)m, s));
        return MI_OK;
    }
    double* ws = nullptr;
    if ((rc = get_ws(s, &ws))) return rc;
    return mdot_run(n, m, multi_vec(m, d_basis), d_y, d_dots, nullptr, ws, s);
}

template <typename T>
static int maxpy_dev(int n, int m, const double* d_coef, int negate, const T* const* d_basis, double* d_y, double* d_norm_out, mi_stream_t s_)
{
    int rc = multi_check(n, m, d_basis, d_y);
    if (rc) return rc;
    CHECK_ARG(m == 0 || d_coef, "null coefficients");
    hipStream_t s = (hipStream_t)s_;
    if (m == 0 || n == 0) // nothing to update; the norm of y as it stands (0 for an empty vector)
        return d_norm_out ? mi_norm2_dev(n, d_y, d_norm_out, s_) : MI_OK;
    double* ws = nullptr;
    if ((rc = get_ws(s, &ws))) return rc;
    return maxpy_run(n, m, d_coef, negate, multi_vec(m, d_basis), d_y, d_norm_out, ws, s);
}

// mi_maxpy_upto_dev and its float-basis twin: mi_maxpy*_dev's geometry and tile, the count read by the kernels
template <typename T>
static int maxpy_upto_dev(int n, int m, const int* d_count, const double* d_coef, int negate, const T* const* d_basis, double* d_y, mi_stream_t s_)
{
    int rc = multi_check(n, m, d_basis, d_y);
    if (rc) return rc;
    CHECK_ARG(d_count, "null count");
    CHECK_ARG(m == 0 || d_coef, "null coefficients");
    if (m == 0 || n == 0) return MI_OK;
    hipStream_t s = (hipStream_t)s_;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev)); // (MI_ERR_NODEVICE without a GPU; no norm, so no workspace: nothing is allocated, on any stream)
    int np, seg;
    red_geometry(n, &np, &seg);
    const bool nt = blas1_nt(n);
    const MultiVecT<T> B = multi_vec(m, d_basis);
    with_multi_tile<T>([&](auto TILE) {
        for (int first = 0; first < m; first += TILE()) // every chunk of the m vectors, whatever the count will be: the kernel decides
            pick([&](auto NT) { hipLaunchKernelGGL((maxpy_upto_kernel<TILE(), NT(), T>), dim3(np), dim3(kRedWG), 0, s, n, seg, first, m, d_count, d_coef, negate, B, d_y); }, nt);
    });
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

template <typename T>
static int cgs_dev(int n, int m, const T* const* d_basis, double* d_y, int passes, double* d_h, double* d_norm, mi_stream_t s_)
{
    int rc = multi_check(n, m, d_basis, d_y);
    if (rc) return rc;
    CHECK_ARG(passes == 1 || passes == 2, "passes must be 1 or 2");
    CHECK_ARG(d_norm && (m == 0 || d_h), "null h / norm");
    hipStream_t s = (hipStream_t)s_;
    if (n == 0 && m) HIP_TRY(hipMemsetAsync(d_h, 0, sizeof(double) * (size_t)m, s));
    if (m == 0 || n == 0) return mi_norm2_dev(n, d_y, d_norm, s_);
    double* ws = nullptr;
    if ((rc = get_ws(s, &ws))) return rc;
    const MultiVecT<T> B = multi_vec(m, d_basis);
    // per pass: every dot against the SAME y, then one update with the negated dots; the norm rides on the last update
    if ((rc = mdot_run(n, m, B, d_y, d_h, nullptr, ws, s))) return rc;
    if ((rc = maxpy_run(n, m, d_h, 1, B, d_y, passes == 1 ? d_norm : nullptr, ws, s))) return rc;
    if (passes == 2) {
        double* d2 = ws + kWsDots2;
        if ((rc = mdot_run(n, m, B, d_y, d2, d_h, ws, s))) return rc; // h_j = h_j + d2_j, one rounded add
        if ((rc = maxpy_run(n, m, d2, 1, B, d_y, d_norm, ws, s))) return rc;
    }
    return MI_OK;
}

extern "C" int mi_mdot_dev(int n, int m, const double* const* d_basis, const double* d_y, double* d_dots, mi_stream_t s)
{
    return mdot_dev(n, m, d_basis, d_y, d_dots, s);
}

extern "C" int mi_maxpy_dev(int n, int m, const double* d_coef, int negate, const double* const* d_basis, double* d_y,
                            double* d_norm_out, mi_stream_t s)
{
    return maxpy_dev(n, m, d_coef, negate, d_basis, d_y, d_norm_out, s);
}

extern "C" int mi_cgs_dev(int n, int m, const double* const* d_basis, double* d_y, int passes, double* d_h, double* d_norm,
                          mi_stream_t s)
{
    return cgs_dev(n, m, d_basis, d_y, passes, d_h, d_norm, s);
}

extern "C" int mi_mdot_f32_dev(int n, int m, const float* const* d_basis, const double* d_y, double* d_dots, mi_stream_t s)
{
    return mdot_dev(n, m, d_basis, d_y, d_dots, s);
}

extern "C" int mi_maxpy_f32_dev(int n, int m, const double* d_coef, int negate, const float* const* d_basis, double* d_y,
                                double* d_norm_out, mi_stream_t s)
{
    return maxpy_dev(n, m, d_coef, negate, d_basis, d_y, d_norm_out, s);
}

extern "C" int mi_maxpy_upto_dev(int n, int m, const int* d_count, const double* d_coef, int negate, const double* const* d_basis, double* d_y,
                                 mi_stream_t s)
{
    return maxpy_upto_dev(n, m, d_count, d_coef, negate, d_basis, d_y, s);
}

extern "C" int mi_maxpy_upto_f32_dev(int n, int m, const int* d_count, const double* d_coef, int negate, const float* const* d_basis, double* d_y,
                                     mi_stream_t s)
{
    return maxpy_upto_dev(n, m, d_count, d_coef, negate, d_basis, d_y, s);
}

extern "C" int mi_cgs_f32_dev(int n, int m, const float* const* d_basis, double* d_y, int passes, double* d_h, double* d_norm,
                              mi_stream_t s)
{
    return cgs_dev(n, m, d_basis, d_y, passes, d_h, d_norm, s);
}

// out32 = round32(x / *d_div), out64 = widen(out32) (gmres_kernels.hpp): one launch, nothing allocated, capturable
extern "C" int mi_round_f32_dev(int n, const double* d_x, const double* d_div, float* d_out32, double* d_out64, mi_stream_t s)
{
    CHECK_ARG(n >= 0, "negative n");
    if (n == 0) return MI_OK;
    CHECK_ARG(d_x && d_out32, "null vector");
    CHECK_ARG(((uintptr_t)d_out32 & 3) == 0 && (((uintptr_t)d_x | (uintptr_t)d_out64) & 7) == 0, "a misaligned vector");
    CHECK_ARG((const void*)d_out32 != (const void*)d_x && (const void*)d_out32 != (const void*)d_out64, "out32 is one of the double vectors");
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev)); // (MI_ERR_NODEVICE without a GPU, like the entry points that need the workspace)
    const int grid = launch_grid(n / 2, 256, 2048, 1);
    pick([&](auto DIV) { hipLaunchKernelGGL(round_f32_kernel<DIV()>, dim3(grid), dim3(256), 0, (hipStream_t)s, n, d_x, d_div, d_out32, d_out64); }, d_div != nullptr);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_gather_dev(int m, const int* d_idx, const double* d_src, double* d_dst, mi_stream_t s)
{
    CHECK_ARG(m >= 0, "negative m");
    if (m == 0) return MI_OK;
    CHECK_ARG(d_idx && d_src && d_dst, "null pointer");
    hipLaunchKernelGGL(gather_kernel, dim3(launch_grid(m, 256, 2048)), dim3(256), 0, (hipStream_t)s, m, d_idx, d_src, d_dst);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_dot(int n, const double* x, const double* y, double* out)
{
    CHECK_ARG(n >= 0 && out && (n == 0 || (x && y)), "bad argument");
    int rc = need_device();
    if (rc) return rc;
    Scratch S;
    double *dx, *dy, *dout;
    if ((rc = S.up(x, n, &dx)) || (rc = S.up(y, n, &dy)) || (rc = S.up(nullptr, 1, &dout))) return rc;
    if ((rc = mi_dot_dev(n, dx, dy, dout, nullptr))) return rc;
    HIP_TRY(hipMemcpy(out, dout, sizeof(double), hipMemcpyDeviceToHost));
    return MI_OK;
}

extern "C" int mi_norm2(int n, const double* x, double* out)
{
    CHECK_ARG(n >= 0 && out && (n == 0 || x), "bad argument");
    int rc = need_device();
    if (rc) return rc;
    Scratch S;
    double *dx, *dout;
    if ((rc = S.up(x, n, &dx)) || (rc = S.up(nullptr, 1, &dout))) return rc;
    if ((rc = mi_norm2_dev(n, dx, dout, nullptr))) return rc;
    HIP_TRY(hipMemcpy(out, dout, sizeof(double), hipMemcpyDeviceToHost));
    return MI_OK;
}

extern "C" int mi_rel_error(int n, const double* ref, const double* test, double* out)
{
    CHECK_ARG(n >= 0 && out && (n == 0 || (ref && test)), "bad argument");
    int rc = need_device();
    if (rc) return rc;
    Scratch S;
    double *da, *db, *dout;
    if ((rc = S.up(ref, n, &da)) || (rc = S.up(test, n, &db)) || (rc = S.up(nullptr, 1, &dout))) return rc;
    if ((rc = mi_rel_error_dev(n, da, db, dout, nullptr))) return rc;
    HIP_TRY(hipMemcpy(out, dout, sizeof(double), hipMemcpyDeviceToHost));
    return MI_OK;
}

extern "C" int mi_axpy(int n, double a, const double* x, double* y)
{
    CHECK_ARG(n >= 0 && (n == 0 || (x && y)), "bad argument");
    int rc = need_device();
    if (rc) return rc;
    Scratch S;
    double *dx, *dy;
    if ((rc = S.up(x, n, &dx)) || (rc = S.up(y, n, &dy))) return rc;
    if ((rc = mi_axpy_dev(n, a, dx, dy, nullptr))) return rc;
    if (n) HIP_TRY(hipMemcpy(y, dy, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    return MI_OK;
}

extern "C" int mi_orthogonalize(int n, const double* b, const double* x1, double* x3, double alpha, double* beta_out)
{
    CHECK_ARG(n >= 0 && (n == 0 || (b && x1 && x3)), "bad argument");
    int rc = need_device();
    if (rc) return rc;
    Scratch S;
    double *db, *dx1, *dx3, *dbeta;
    if ((rc = S.up(b, n, &db)) || (rc = S.up(x1, n, &dx1)) || (rc = S.up(nullptr, n, &dx3)) || (rc = S.up(nullptr, 1, &dbeta)))
        return rc;
    if ((rc = mi_orthogonalize_dev(n, db, dx1, dx3, alpha, dbeta, nullptr))) return rc;
    if (n) HIP_TRY(hipMemcpy(x3, dx3, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    double beta = 0.0;
    HIP_TRY(hipMemcpy(&beta, dbeta, sizeof(double), hipMemcpyDeviceToHost));
    if (beta_out) *beta_out = beta;
    return MI_OK;
}

extern "C" int mi_orthonormalize_against_basis(int n, int m, const double* const* basis, double* y, double* dots_out)
{
    CHECK_ARG(n >= 0 && m >= 0 && (m == 0 || basis) && (n == 0 || y), "bad argument");
    int rc = need_device();
    if (rc) return rc;
    if (m == 0) return MI_OK;
    Scratch S;
    std::vector<const double*> dv((size_t)m);
    double *dy = nullptr, *dd = nullptr;
    for (int j = 0; j < m; j++) {
        CHECK_ARG(n == 0 || basis[j], "null basis vector");
        double* p = nullptr;
        if ((rc = S.up(basis[j], n, &p))) return rc;
        dv[j] = p;
    }
    if ((rc = S.up(y, n, &dy)) || (rc = S.up(nullptr, m, &dd))) return rc;
    if ((rc = mi_orthonormalize_against_basis_dev(n, m, dv.data(), dy, dd, nullptr))) return rc;
    if (n) HIP_TRY(hipMemcpy(y, dy, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    if (dots_out) HIP_TRY(hipMemcpy(dots_out, dd, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost));
    else HIP_TRY(hipDeviceSynchronize());
    return MI_OK;
}

extern "C" int mi_mdot(int n, int m, const double* const* basis, const double* y, double* dots)
{
    int rc = multi_check(n, m, basis, y);
    if (rc) return rc;
    CHECK_ARG(m == 0 || dots, "null dots");
    if ((rc = need_device())) return rc;
    if (m == 0) return MI_OK;
    Scratch S;
    std::vector<const double*> dv((size_t)m);
    double *dy = nullptr, *dd = nullptr;
    for (int j = 0; j < m; j++) {
        double* p = nullptr;
        if ((rc = S.up(n ? basis[j] : nullptr, n, &p))) return rc;
        dv[j] = p;
    }
    if ((rc = S.up(y, n, &dy)) || (rc = S.up(nullptr, m, &dd))) return rc;
    if ((rc = mi_mdot_dev(n, m, dv.data(), dy, dd, nullptr))) return rc;
    HIP_TRY(hipMemcpy(dots, dd, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost));
    return MI_OK;
}

extern "C" int mi_maxpy(int n, int m, const double* coef, int negate, const double* const* basis, double* y)
{
    int rc = multi_check(n, m, basis, y);
    if (rc) return rc;
    CHECK_ARG(m == 0 || coef, "null coefficients");
    if ((rc = need_device())) return rc;
    if (m == 0 || n == 0) return MI_OK;
    Scratch S;
    std::vector<const double*> dv((size_t)m);
    double *dy = nullptr, *dc = nullptr;
    for (int j = 0; j < m; j++) {
        double* p = nullptr;
        if ((rc = S.up(basis[j], n, &p))) return rc;
        dv[j] = p;
    }
    if ((rc = S.up(y, n, &dy)) || (rc = S.up(coef, m, &dc))) return rc;
    if ((rc = mi_maxpy_dev(n, m, dc, negate, dv.data(), dy, nullptr, nullptr))) return rc;
    HIP_TRY(hipMemcpy(y, dy, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    return MI_OK;
}

// ---------------------------------------------------------------- permutations of a relabelled handle (reorder.hpp)
// x into a reordered handle's numbering (whole nodes at a time when nodes were moved and x allows 16-byte accesses)
int gather_perm(mi_csr_t A, const double* d_x, double* d_xp, hipStream_t s)
{
    if (A->reorder_block == 4 && (((uintptr_t)d_x | (uintptr_t)d_xp) & 15) == 0) {
        const int nn = A->n / 4;
        hipLaunchKernelGGL(gather_nodes_kernel, dim3(launch_grid(nn, 256, 4096)), dim3(256), 0, s, nn, A->d_iperm, d_x, d_xp);
        HIP_TRY(hipGetLastError());
        return MI_OK;
    }
    return mi_gather_dev(A->n, A->d_iperm, d_x, d_xp, (mi_stream_t)s);
}


// dst[idx[i]] = src[i]
__global__ __launch_bounds__(256) void scatter_kernel(int m, const int* __restrict__ idx, const double* __restrict__ src,
                                                      double* __restrict__ dst)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) dst[idx[i]] = src[i];
}

// a vector in a reordered handle's numbering back into the caller's: dst[iperm[r']] = src[r']
int scatter_perm(mi_csr_t A, const double* d_src, double* d_dst, hipStream_t s)
{
    hipLaunchKernelGGL(scatter_kernel, dim3(launch_grid(A->n, 256, 2048)), dim3(256), 0, s, A->n, A->d_iperm, d_src, d_dst);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}
