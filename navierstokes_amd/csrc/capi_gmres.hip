// capi_gmres.hip: mi_gmres_* — right-preconditioned restarted GMRES with a whole cycle enqueued on the device (include/mi355_spmv.h,
// DESIGN.md 4.6) — part of libmi355spmv.so (see capi_internal.hpp for the layout of the library).  The vector work is the library's
// own entry points (the products, mi_bilu4*_solve_dev, mi_cgs_dev, mi_maxpy_dev, mi_axpy_dev); what is new on the device is
// gmres_kernels.hpp.  A handle created with MI_BASIS_F32 stores its Krylov basis in float: the same loop with mi_cgs_f32_dev /
// mi_maxpy_f32_dev / mi_round_f32_dev, and a converged recurrence confirmed by the next cycle's start.  At the end of the file: a
// whole cycle with no read-back (mi_gmres_cycle_dev: the counted steps stay on the device) and the solve as replayed graphs
// (mi_gmres_plan_*), both with the bits of mi_gmres_solve_dev.  Built for gfx950 only; no CPU fallback: every entry point that computes needs a HIP device.
#include "capi_internal.hpp"
#include "gmres_kernels.hpp"

#include <set>

struct mi_gmres_s {
    int device = 0;
    int n = 0, m = 0;       // rows; restart
    long long ldv = 0;      // n rounded up to even: every row of V is 16-byte aligned
    int basis = MI_BASIS_F64;
    long long ldv32 = 0;    // MI_BASIS_F32: n rounded up to a multiple of 4: every row of V32 is 16-byte aligned
    mi_csr_t A_csr = nullptr;       // the operator: one of the two (not owned)
    mi_bcsr4_t A_bcsr = nullptr;
    mi_bilu4_t F = nullptr;         // the preconditioner (not owned), or null
    int pc_kind = MI_GMRES_PC_EXACT, sf = 0, sb = 0;
    DevArray<double> V;             // (m + 1) rows of ldv (MI_BASIS_F64 only)
    DevArray<float> V32;            // (m + 1) rows of ldv32 (MI_BASIS_F32 only), and q: widen(the newest row), what the next product reads
    DevArray<double> q;
    DevArray<double> w, z;          // the two work vectors
    DevArray<double> small;         // GmresSmall (gmres_kernels.hpp)
    DevArray<double> hb, hx;        // b and x of the host-pointer solve, allocated by its first call
    PinnedArray<double> slot[2];    // read-back slots: the record and the cycle's history entries
    OwnedEvent ev[2];
    std::vector<const double*> Vptr; // the rows of V, as mi_cgs_dev / mi_maxpy_dev take them
    std::vector<const float*> V32ptr; // the rows of V32, as mi_cgs_f32_dev / mi_maxpy_f32_dev take them
    int refused_last = 0;           // MI_BASIS_F32: claims of the recurrence that the next cycle's true residual did not confirm
    int next_slot = 0;
    int last_k = 0;                 // the last cycle: its counted steps and its ||r0||
    double last_beta = 0.0;
    int readbacks_last = 0, launches_last = 0, wasted_last = 0;
    unsigned gen = 0;               // bumped by every mi_gmres_set_*: a plan (mi_gmres_plan_*) made before it is stale
    std::set<hipStream_t> prepared; // streams mi_gmres_prepare_stream has seen since the operator was set
    GmresSmall S() const { return GmresSmall{m, small.get()}; }
    double* row(int k) const { return V.get() + (size_t)k * ldv; }
    float* row32(int k) const { return V32.get() + (size_t)k * ldv32; }
    bool f32() const { return basis == MI_BASIS_F32; }
    // freed in the order of allocation
    ~mi_gmres_s() { V = {}, V32 = {}, q = {}, w = {}, z = {}, small = {}, hb = {}, hx = {}; }
};

constexpr size_t kGmresSlotDoubles = kGmresRecDoubles + kMultiMax;

extern "C" int mi_gmres_create(int n, int restart, mi_gmres_t* out)
{
    return mi_gmres_create_ex(n, restart, MI_BASIS_F64, out);
}

extern "C" int mi_gmres_create_ex(int n, int restart, int basis, mi_gmres_t* out)
{
    CHECK_ARG(out, "null output handle");
    *out = nullptr;
    CHECK_ARG(n >= 1, "n must be at least 1");
    CHECK_ARG(restart >= 1 && restart <= kMultiMax, "restart must be in 1..64");
    CHECK_ARG(basis == MI_BASIS_F64 || basis == MI_BASIS_F32, "unknown basis (MI_BASIS_F64 or MI_BASIS_F32)");
    int rc = need_device();
    if (rc) return rc;
    std::unique_ptr<mi_gmres_s> G(new (std::nothrow) mi_gmres_s);
    if (!G) return fail(MI_ERR_ALLOC, "out of host memory");
    HIP_TRY(hipGetDevice(&G->device));
    G->n = n, G->m = restart, G->ldv = (long long)n + (n & 1);
    G->basis = basis, G->ldv32 = ((long long)n + 3) / 4 * 4;
    if (G->f32()) {
        if ((rc = dev_alloc(G->V32, (size_t)(restart + 1) * G->ldv32)) || (rc = dev_alloc(G->q, (size_t)G->ldv))) return rc;
    } else if ((rc = dev_alloc(G->V, (size_t)(restart + 1) * G->ldv))) {
        return rc;
    }
    if ((rc = dev_alloc(G->w, (size_t)G->ldv)) || (rc = dev_alloc(G->z, (size_t)G->ldv)) ||
        (rc = dev_zeros(G->small, GmresSmall::doubles(restart))))
        return rc;
    for (int i = 0; i < 2; i++) {
        HIP_TRY_AS("hipHostMalloc", G->slot[i].alloc(kGmresSlotDoubles));
        if ((rc = dev_create(G->ev[i], hipEventDisableTiming))) return rc;
    }
    for (int k = 0; k <= restart; k++) {
        if (G->f32()) G->V32ptr.push_back(G->row32(k));
        else G->Vptr.push_back(G->row(k));
    }
    *out = G.release();
    return MI_OK;
}

extern "C" int mi_gmres_destroy(mi_gmres_t G)
{
    if (!G) return MI_OK;
    (void)hipDeviceSynchronize(); // a copy into a pinned slot may still be in flight behind the last solve
    delete G;
    return MI_OK;
}

extern "C" int mi_gmres_set_operator_csr(mi_gmres_t G, mi_csr_t A)
{
    CHECK_ARG(G && A, "null handle");
    CHECK_ARG(A->n == A->ncols && !A->mapped, "the operator must be a square, unmapped matrix");
    CHECK_ARG(A->n == G->n, "the operator's row count is not the solver's n");
    G->A_csr = A, G->A_bcsr = nullptr;
    G->gen++, G->prepared.clear();
    return MI_OK;
}

extern "C" int mi_gmres_set_operator_bcsr4(mi_gmres_t G, mi_bcsr4_t A)
{
    CHECK_ARG(G && A, "null handle");
    CHECK_ARG(A->nbrows == A->nbcols, "the operator must be square");
    CHECK_ARG(4LL * A->nbrows == G->n, "the operator's row count (4 nbrows) is not the solver's n");
    G->A_bcsr = A, G->A_csr = nullptr;
    G->gen++, G->prepared.clear();
    return MI_OK;
}

extern "C" int mi_gmres_set_precond(mi_gmres_t G, mi_bilu4_t F, int kind, int sweeps_fwd, int sweeps_bwd)
{
    CHECK_ARG(G, "null handle");
    if (!F) {
        G->F = nullptr;
        G->gen++;
        return MI_OK;
    }
    CHECK_ARG(kind == MI_GMRES_PC_EXACT || kind == MI_GMRES_PC_SWEEPS || kind == MI_GMRES_PC_SWEEPS_F32, "unknown preconditioner kind");
    CHECK_ARG(kind == MI_GMRES_PC_EXACT || (sweeps_fwd >= 0 && sweeps_bwd >= 0), "negative sweep count");
    int nb = 0, rc;
    if ((rc = mi_bilu4_info(F, &nb, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))) return rc;
    CHECK_ARG(4LL * nb == G->n, "the preconditioner's row count (4 nbrows) is not the solver's n");
    // everything a solve would otherwise allocate on first use
    if (kind == MI_GMRES_PC_SWEEPS && (rc = mi_bilu4sw_prepare(F))) return rc;
    if (kind == MI_GMRES_PC_SWEEPS_F32 && (rc = mi_bilu4sp_prepare(F))) return rc;
    G->F = F, G->pc_kind = kind, G->sf = sweeps_fwd, G->sb = sweeps_bwd;
    G->gen++;
    return MI_OK;
}

static int gmres_mult(mi_gmres_s* G, const double* x, double* y, mi_stream_t s)
{
    return G->A_csr ? mi_spmv_dev(G->A_csr, x, y, s) : mi_bcsr4_spmv_dev(G->A_bcsr, x, y, s);
}

// out += sum y_j V_j over the k counted steps of the cycle (the basis as stored)
static int gmres_combine(mi_gmres_s* G, int k, double* out, mi_stream_t s)
{
    const GmresSmall S = G->S();
    return G->f32() ? mi_maxpy_f32_dev(G->n, k, S.y(), 0, G->V32ptr.data(), out, nullptr, s)
                    : mi_maxpy_dev(G->n, k, S.y(), 0, G->Vptr.data(), out, nullptr, s);
}

static int gmres_precond(mi_gmres_s* G, const double* in, double* out, mi_stream_t s)
{
    switch (G->pc_kind) {
    case MI_GMRES_PC_SWEEPS: return mi_bilu4sw_solve_dev(G->F, in, out, G->sf, G->sb, s);
    case MI_GMRES_PC_SWEEPS_F32: return mi_bilu4sp_solve_dev(G->F, in, out, G->sf, G->sb, s);
    default: return mi_bilu4_solve_dev(G->F, in, out, s);
    }
}

// step k of a cycle, enqueued: w = A M^-1 V_k straight into row k + 1, CGS2 in place with the raw column where the small problem
// reads it, the small problem, the division
static int gmres_enqueue_step(mi_gmres_s* G, int k, double rtol, int maxiter, int grid, hipStream_t st)
{
    const GmresSmall S = G->S();
    mi_stream_t s = (mi_stream_t)st;
    double* next = G->row(k + 1);
    double* col = S.hraw() + (size_t)k * (G->m + 2);
    int rc;
    if (G->F) {
        if ((rc = gmres_precond(G, G->row(k), G->z, s)) || (rc = gmres_mult(G, G->z, next, s))) return rc;
        G->launches_last++;
    } else if ((rc = gmres_mult(G, G->row(k), next, s))) {
        return rc;
    }
    if ((rc = mi_cgs_dev(G->n, k + 1, G->Vptr.data(), next, 2, col, col + k + 1, s))) return rc;
    hipLaunchKernelGGL(gmres_hess_step, dim3(1), dim3(64), 0, st, S, k, rtol, maxiter);
    hipLaunchKernelGGL(div_by_scalar_kernel, dim3(grid), dim3(256), 0, st, G->n, col + k + 1, next);
    G->launches_last += 4;
    return MI_OK;
}

// the same step with the float basis: w = A M^-1 q into a work vector (q = widen(V32_k), the STORED vector), CGS2 of w against
// V32_0..V32_k, the small problem unchanged, then V32_{k+1} = round32(w / nrm) and q = widen(V32_{k+1}) in one launch
static int gmres_enqueue_step_f32(mi_gmres_s* G, int k, double rtol, int maxiter, hipStream_t st)
{
    const GmresSmall S = G->S();
    mi_stream_t s = (mi_stream_t)st;
    double* col = S.hraw() + (size_t)k * (G->m + 2);
    int rc;
    if (G->F) {
        if ((rc = gmres_precond(G, G->q, G->z, s)) || (rc = gmres_mult(G, G->z, G->w, s))) return rc;
        G->launches_last++;
    } else if ((rc = gmres_mult(G, G->q, G->w, s))) {
        return rc;
    }
    if ((rc = mi_cgs_f32_dev(G->n, k + 1, G->V32ptr.data(), G->w, 2, col, col + k + 1, s))) return rc;
    hipLaunchKernelGGL(gmres_hess_step, dim3(1), dim3(64), 0, st, S, k, rtol, maxiter);
    if ((rc = mi_round_f32_dev(G->n, G->w, col + k + 1, G->row32(k + 1), G->q, s))) return rc;
    G->launches_last += 4;
    return MI_OK;
}

extern "C" int mi_gmres_solve_dev(mi_gmres_t G, const double* d_b, double* d_x, double rtol, int maxiter, int check_every, int* iterations,
                                  int* reason_out, double* history, mi_stream_t s)
{
    CHECK_ARG(check_every >= 1, "check_every must be at least 1");
    CHECK_ARG(maxiter >= 0, "negative maxiter");
    CHECK_ARG(G, "null handle");
    CHECK_ARG(d_b && d_x, "null vector");
    if (!G->A_csr && !G->A_bcsr) return fail(MI_ERR_STATE, "mi_gmres_solve_dev: no operator set (mi_gmres_set_operator_*)");
    hipStream_t st = (hipStream_t)s;
    if (stream_is_capturing(st)) return fail(MI_ERR_STATE, "mi_gmres_solve_dev: the stream is capturing and a solve reads back (it cannot be captured)");
    const int n = G->n, m = G->m;
    const GmresSmall S = G->S();
    int grid = (n + 255) / 256;
    if (grid > 2048) grid = 2048;
    G->readbacks_last = G->launches_last = G->wasted_last = G->refused_last = 0;
    const bool f32 = G->f32();
    bool claimed = false; // MI_BASIS_F32: the last cycle froze with reason 1 and this cycle's start has to confirm it
    G->last_k = 0;
    int its = 0, reason = 0, rc;
    bool first = true;
    for (;;) {
        // ---- the start of a cycle: r = b - A x into row 0, its norm, the record, V_0 = r / beta (the float basis: r into a work
        // vector, then V32_0 = round32(r / beta) and q = widen(V32_0))
        if ((rc = gmres_mult(G, d_x, G->w, s)) || (rc = residual_norm_dev(n, d_b, G->w, f32 ? G->z.get() : G->row(0), S.beta(), st))) return rc;
        if (first && (rc = mi_norm2_dev(n, d_b, S.bnorm(), s))) return rc;
        hipLaunchKernelGGL(gmres_cycle_begin, dim3(1), dim3(64), 0, st, S, first ? 1 : 0, rtol, maxiter);
        if (f32) {
            if ((rc = mi_round_f32_dev(n, G->z, S.beta(), G->row32(0), G->q, s))) return rc;
        } else {
            hipLaunchKernelGGL(div_by_scalar_kernel, dim3(grid), dim3(256), 0, st, n, S.beta(), G->row(0));
        }
        HIP_TRY(hipGetLastError());
        G->launches_last += first ? 6 : 5;
        // ---- batches of steps; behind each the record and the cycle's history go to a pinned slot, and the host looks at a batch's
        // slot only after the NEXT batch is enqueued
        GmresRecord rec{};
        int k_enq = 0, pending = -1;
        for (;;) {
            int cur = -1;
            const int room = std::min(m - k_enq, maxiter - its - k_enq);
            if (room > 0 || pending < 0) { // (room == 0 with nothing pending: maxiter == 0, the record alone)
                // (a cycle's first batch is one step short: a solve that ends at the cycle's start, which only this batch's record
                // tells, has then wasted 2 check_every - 1 steps at most, like one that freezes inside a batch)
                const int nb = std::min(pending < 0 ? check_every - 1 : check_every, std::max(room, 0));
                for (int j = 0; j < nb; j++)
                    if ((rc = f32 ? gmres_enqueue_step_f32(G, k_enq + j, rtol, maxiter, st) : gmres_enqueue_step(G, k_enq + j, rtol, maxiter, grid, st))) return rc;
                k_enq += nb;
                cur = G->next_slot;
                G->next_slot ^= 1;
                HIP_TRY(hipMemcpyAsync(G->slot[cur], S.base, sizeof(double) * (kGmresRecDoubles + (size_t)k_enq), hipMemcpyDeviceToHost, st));
                HIP_TRY(hipEventRecord(G->ev[cur], st));
            }
            if (pending >= 0) {
                HIP_TRY(hipEventSynchronize(G->ev[pending]));
                G->readbacks_last++;
                memcpy(&rec, G->slot[pending], sizeof(rec));
                if (history) {
                    if (first) history[0] = rec.rel0;
                    for (int j = 0; j < rec.k; j++) history[its + 1 + j] = G->slot[pending][kGmresRecDoubles + j];
                }
                if (rec.reason != 0 || cur < 0) break; // frozen (what is enqueued behind it is wasted), or the cycle's last batch
            }
            pending = cur;
        }
        G->wasted_last += k_enq - rec.k;
        its = rec.its;
        G->last_k = rec.k, G->last_beta = rec.beta;
        // ---- the end of a cycle: y on the device, then x += M^-1 (V y)
        if (rec.k > 0) {
            hipLaunchKernelGGL(gmres_backsolve, dim3(1), dim3(256), 0, st, S, rec.k);
            HIP_TRY(hipGetLastError());
            if (G->F) {
                HIP_TRY(hipMemsetAsync(G->w, 0, sizeof(double) * (size_t)n, st));
                if ((rc = gmres_combine(G, rec.k, G->w, s)) || (rc = gmres_precond(G, G->w, G->z, s)) ||
                    (rc = mi_axpy_dev(n, 1.0, G->z, d_x, s)))
                    return rc;
                G->launches_last += 5;
            } else {
                if ((rc = gmres_combine(G, rec.k, d_x, s))) return rc;
                G->launches_last += 2;
            }
        }
        reason = rec.reason == kGmresMetAtStart ? 0 : rec.reason;
        // the float basis: the recurrence is exact only to float rounding of the basis, so a step's reason 1 (rec.k > 0) is a CLAIM:
        // the update above has run, and the next cycle's start — the true residual — confirms it (reason 1 with k = 0) or not
        if (claimed && !(rec.reason == 1 && rec.k == 0)) G->refused_last++;
        claimed = f32 && rec.reason == 1 && rec.k > 0;
        if (claimed) {
            first = false;
            continue;
        }
        if (rec.reason != 0) break;
        if (its >= maxiter) {
            reason = 2;
            break;
        }
        first = false;
    }
    if (iterations) *iterations = its;
    if (reason_out) *reason_out = reason;
    return MI_OK;
}

extern "C" int mi_gmres_solve(mi_gmres_t G, const double* b, double* x, double rtol, int maxiter, int check_every, int* iterations, int* reason,
                              double* history)
{
    CHECK_ARG(check_every >= 1, "check_every must be at least 1");
    CHECK_ARG(maxiter >= 0, "negative maxiter");
    CHECK_ARG(G, "null handle");
    CHECK_ARG(b && x, "null vector");
    int rc;
    if (!G->hb && ((rc = dev_alloc(G->hb, (size_t)G->ldv)) || (rc = dev_alloc(G->hx, (size_t)G->ldv)))) return rc;
    const size_t bytes = sizeof(double) * (size_t)G->n;
    HIP_TRY(hipMemcpy(G->hb, b, bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(G->hx, x, bytes, hipMemcpyHostToDevice));
    if ((rc = mi_gmres_solve_dev(G, G->hb, G->hx, rtol, maxiter, check_every, iterations, reason, history, nullptr))) return rc;
    HIP_TRY(hipMemcpy(x, G->hx, bytes, hipMemcpyDeviceToHost));
    return MI_OK;
}

extern "C" int mi_gmres_fetch_cycle(mi_gmres_t G, int* k, double* hraw, double* y, double* beta)
{
    CHECK_ARG(G, "null handle");
    const int m = G->m, kk = G->last_k;
    const GmresSmall S = G->S();
    if (k) *k = kk;
    if (beta) *beta = G->last_beta;
    if (hraw || y) HIP_TRY(hipDeviceSynchronize());
    if (hraw) { // columns past the last counted step were never used: reported as zeros (as the places past a column's norm are)
        memset(hraw, 0, sizeof(double) * (size_t)m * (m + 2));
        if (kk) HIP_TRY(hipMemcpy(hraw, S.hraw(), sizeof(double) * (size_t)kk * (m + 2), hipMemcpyDeviceToHost));
    }
    if (y) {
        memset(y, 0, sizeof(double) * (size_t)m);
        if (kk) HIP_TRY(hipMemcpy(y, S.y(), sizeof(double) * (size_t)kk, hipMemcpyDeviceToHost));
    }
    return MI_OK;
}

// V, or V32 and q
static long long gmres_basis_bytes(const mi_gmres_s* G)
{
    return G->f32() ? 4LL * (G->m + 1) * G->ldv32 + 8LL * G->ldv : 8LL * (G->m + 1) * G->ldv;
}

extern "C" int mi_gmres_basis_info(mi_gmres_t G, int* basis, long long* basis_bytes, int* refused_last)
{
    CHECK_ARG(G, "null handle");
    if (basis) *basis = G->basis;
    if (basis_bytes) *basis_bytes = gmres_basis_bytes(G);
    if (refused_last) *refused_last = G->refused_last;
    return MI_OK;
}

extern "C" int mi_gmres_info(mi_gmres_t G, int* restart, long long* device_bytes, int* readbacks_last, int* launches_last, int* wasted_steps_last)
{
    CHECK_ARG(G, "null handle");
    if (restart) *restart = G->m;
    if (device_bytes) // what the handle owns: the basis (gmres_basis_bytes), the two work vectors, the small state, b and x of the host form
        *device_bytes = gmres_basis_bytes(G) + (long long)sizeof(double) * (2 * G->ldv + (long long)GmresSmall::doubles(G->m) + (G->hb ? 2 * G->ldv : 0));
    if (readbacks_last) *readbacks_last = G->readbacks_last;
    if (launches_last) *launches_last = G->launches_last;
    if (wasted_steps_last) *wasted_steps_last = G->wasted_last;
    return MI_OK;
}

// ---------------------------------------------------------------- a cycle with no read-back, and the solve as replayed graphs
// (include/mi355_spmv.h, "capturable GMRES")

// the start of a cycle, enqueued: the launches of mi_gmres_solve_dev's own cycle start (whose host loop keeps them inline)
static int gmres_enqueue_start(mi_gmres_s* G, const double* d_b, double* d_x, bool first, double rtol, int maxiter, int grid, hipStream_t st)
{
    const GmresSmall S = G->S();
    mi_stream_t s = (mi_stream_t)st;
    const int n = G->n;
    const bool f32 = G->f32();
    int rc;
    if ((rc = gmres_mult(G, d_x, G->w, s)) || (rc = residual_norm_dev(n, d_b, G->w, f32 ? G->z.get() : G->row(0), S.beta(), st))) return rc;
    if (first && (rc = mi_norm2_dev(n, d_b, S.bnorm(), s))) return rc;
    hipLaunchKernelGGL(gmres_cycle_begin, dim3(1), dim3(64), 0, st, S, first ? 1 : 0, rtol, maxiter);
    if (f32) {
        if ((rc = mi_round_f32_dev(n, G->z, S.beta(), G->row32(0), G->q, s))) return rc;
    } else {
        hipLaunchKernelGGL(div_by_scalar_kernel, dim3(grid), dim3(256), 0, st, n, S.beta(), G->row(0));
    }
    HIP_TRY(hipGetLastError());
    G->launches_last += first ? 6 : 5;
    return MI_OK;
}

static int gmres_grid(int n)
{
    const int grid = (n + 255) / 256;
    return grid > 2048 ? 2048 : grid;
}

// the end of a cycle, enqueued, with the counted steps k where only the device has them (the record): y, then x += M^-1 (V y) over
// the first k vectors; k == 0 changes no bit of x
static int gmres_enqueue_end(mi_gmres_s* G, double* d_x, hipStream_t st)
{
    const GmresSmall S = G->S();
    mi_stream_t s = (mi_stream_t)st;
    const int n = G->n, m = G->m;
    const int* d_k = &S.rec()->k;
    int rc;
    hipLaunchKernelGGL(gmres_backsolve_counted, dim3(1), dim3(256), 0, st, S);
    HIP_TRY(hipGetLastError());
    double* out = G->F ? G->w.get() : d_x;
    if (G->F) HIP_TRY(hipMemsetAsync(G->w, 0, sizeof(double) * (size_t)n, st));
    if ((rc = G->f32() ? mi_maxpy_upto_f32_dev(n, m, d_k, S.y(), 0, G->V32ptr.data(), out, s)
                       : mi_maxpy_upto_dev(n, m, d_k, S.y(), 0, G->Vptr.data(), out, s)))
        return rc;
    if (G->F) {
        if ((rc = gmres_precond(G, G->w, G->z, s))) return rc;
        int grid = (n / 2 + 255) / 256;
        grid = grid < 1 ? 1 : (grid > 2048 ? 2048 : grid);
        hipLaunchKernelGGL(gmres_update_x, dim3(grid), dim3(256), 0, st, n, S.rec(), G->z, d_x);
        HIP_TRY(hipGetLastError());
    }
    return MI_OK;
}

static int gmres_enqueue_steps(mi_gmres_s* G, int k0, int k1, double rtol, int maxiter, hipStream_t st)
{
    const int grid = gmres_grid(G->n);
    for (int k = k0; k < k1; k++)
        if (const int rc = G->f32() ? gmres_enqueue_step_f32(G, k, rtol, maxiter, st) : gmres_enqueue_step(G, k, rtol, maxiter, grid, st)) return rc;
    return MI_OK;
}

extern "C" int mi_gmres_prepare_stream(mi_gmres_t G, mi_stream_t s)
{
    CHECK_ARG(G, "null handle");
    if (!G->A_csr && !G->A_bcsr) return fail(MI_ERR_STATE, "mi_gmres_prepare_stream: no operator set (mi_gmres_set_operator_*)");
    hipStream_t st = (hipStream_t)s;
    if (stream_is_capturing(st)) return fail(MI_ERR_STATE, "mi_gmres_prepare_stream: the stream is capturing (preparing allocates: call it before the capture)");
    if (G->prepared.count(st)) return MI_OK;
    double* ws = nullptr;
    int rc;
    // the reduction workspace of (device, s), and whatever the operator allocates at its first product on s (a relabelled handle's
    // gather buffer): a throwaway product on the work vectors, which every cycle overwrites before it reads them
    if ((rc = get_ws(st, &ws)) || (rc = gmres_mult(G, G->z, G->w, s))) return rc;
    G->prepared.insert(st);
    return MI_OK;
}

extern "C" int mi_gmres_cycle_dev(mi_gmres_t G, const double* d_b, double* d_x, int first, double rtol, int maxiter, mi_stream_t s)
{
    CHECK_ARG(maxiter >= 0, "negative maxiter");
    CHECK_ARG(G, "null handle");
    CHECK_ARG(d_b && d_x, "null vector");
    if (!G->A_csr && !G->A_bcsr) return fail(MI_ERR_STATE, "mi_gmres_cycle_dev: no operator set (mi_gmres_set_operator_*)");
    hipStream_t st = (hipStream_t)s;
    if (stream_is_capturing(st) && !G->prepared.count(st))
        return fail(MI_ERR_STATE, "mi_gmres_cycle_dev: the stream is capturing and was not prepared (mi_gmres_prepare_stream allocates: call it before the capture)");
    int rc;
    if ((rc = gmres_enqueue_start(G, d_b, d_x, first != 0, rtol, maxiter, gmres_grid(G->n), st)) ||
        (rc = gmres_enqueue_steps(G, 0, G->m, rtol, maxiter, st)) || (rc = gmres_enqueue_end(G, d_x, st)))
        return rc;
    return MI_OK;
}

// the record and the cycle's history entries into a pinned slot behind st, and the event that says so
static int gmres_enqueue_readback(mi_gmres_s* G, int entries, int* slot, hipStream_t st)
{
    const int cur = G->next_slot;
    G->next_slot ^= 1;
    HIP_TRY(hipMemcpyAsync(G->slot[cur], G->S().base, sizeof(double) * (kGmresRecDoubles + (size_t)entries), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(G->ev[cur], st));
    *slot = cur;
    return MI_OK;
}

extern "C" int mi_gmres_state(mi_gmres_t G, mi_stream_t s, int* its, int* k, int* done, int* reason, double* last, double* beta,
                              double* history_cycle)
{
    CHECK_ARG(G, "null handle");
    hipStream_t st = (hipStream_t)s;
    if (stream_is_capturing(st)) return fail(MI_ERR_STATE, "mi_gmres_state: the stream is capturing and the state is read back (it cannot be captured)");
    int cur = 0, rc;
    if ((rc = gmres_enqueue_readback(G, G->m, &cur, st))) return rc;
    HIP_TRY(hipEventSynchronize(G->ev[cur]));
    GmresRecord rec{};
    memcpy(&rec, G->slot[cur], sizeof(rec));
    G->last_k = rec.k, G->last_beta = rec.beta; // (what mi_gmres_fetch_cycle reports)
    if (its) *its = rec.its;
    if (k) *k = rec.k;
    if (done) *done = rec.reason != 0;
    if (reason) *reason = rec.reason == kGmresMetAtStart ? 0 : rec.reason;
    if (last) *last = rec.last;
    if (beta) *beta = rec.beta;
    if (history_cycle)
        for (int j = 0; j < G->m; j++) history_cycle[j] = j < rec.k ? G->slot[cur][kGmresRecDoubles + j] : 0.0;
    return MI_OK;
}

struct mi_gmres_plan_s {
    mi_gmres_s* G = nullptr;
    unsigned gen = 0;
    const double* d_b = nullptr;
    double* d_x = nullptr;
    double rtol = 0.0;
    int maxiter = 0, segment = 0, nseg = 0;
    OwnedStream cap; // the private stream the graphs were captured on (nothing ever runs on it but the preparing product)
    // [0] the start of a solve, [1] the start of a later cycle, [2 .. 2 + nseg) the segments, [2 + nseg] the cycle's end
    std::vector<hipGraph_t> graph;
    std::vector<hipGraphExec_t> exec;
    int replays_last = 0, readbacks_last = 0, wasted_last = 0;
    ~mi_gmres_plan_s()
    {
        for (hipGraphExec_t e : exec) (void)hipGraphExecDestroy(e);
        for (hipGraph_t g : graph) (void)hipGraphDestroy(g);
    }
};

// one graph out of what `enqueue` puts on the private stream; thread-local capture mode: what other threads do meanwhile is their own
template <class F>
static int plan_capture(mi_gmres_plan_s* P, F&& enqueue)
{
    hipStream_t st = P->cap;
    HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue(st);
    const std::string why = g_err; // (ending the capture must not replace the reason)
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(st, &g);
    if (rc || e != hipSuccess) {
        if (g) (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        return rc ? fail(rc, why) : hip_fail(e, "hipStreamEndCapture");
    }
    P->graph.push_back(g);
    hipGraphExec_t x = nullptr;
    HIP_TRY(hipGraphInstantiate(&x, g, nullptr, nullptr, 0));
    P->exec.push_back(x);
    return MI_OK;
}

extern "C" int mi_gmres_plan_create(mi_gmres_t G, const double* d_b, double* d_x, double rtol, int maxiter, int segment, mi_gmres_plan_t* out)
{
    CHECK_ARG(out, "null output handle");
    *out = nullptr;
    CHECK_ARG(segment >= 1, "segment must be at least 1");
    CHECK_ARG(maxiter >= 0, "negative maxiter");
    CHECK_ARG(G, "null handle");
    CHECK_ARG(d_b && d_x, "null vector");
    if (!G->A_csr && !G->A_bcsr) return fail(MI_ERR_STATE, "mi_gmres_plan_create: no operator set (mi_gmres_set_operator_*)");
    std::unique_ptr<mi_gmres_plan_s> P(new (std::nothrow) mi_gmres_plan_s);
    if (!P) return fail(MI_ERR_ALLOC, "out of host memory");
    const int m = G->m;
    P->G = G, P->gen = G->gen, P->d_b = d_b, P->d_x = d_x, P->rtol = rtol, P->maxiter = maxiter;
    P->segment = std::min(segment, m), P->nseg = (m + P->segment - 1) / P->segment;
    int rc;
    if ((rc = dev_create(P->cap, hipStreamNonBlocking)) || (rc = mi_gmres_prepare_stream(G, (mi_stream_t)(hipStream_t)P->cap))) return rc;
    HIP_TRY(hipStreamSynchronize(P->cap)); // the preparing product wrote the work vectors: over before anything else uses them
    const int launches = G->launches_last; // (the enqueue helpers count for mi_gmres_info, which describes the last mi_gmres_solve_dev)
    const int grid = gmres_grid(G->n);
    for (int first = 1; first >= 0 && !rc; first--)
        rc = plan_capture(P.get(), [&](hipStream_t st) { return gmres_enqueue_start(G, d_b, d_x, first != 0, rtol, maxiter, grid, st); });
    for (int j = 0; j < P->nseg && !rc; j++)
        rc = plan_capture(P.get(), [&](hipStream_t st) { return gmres_enqueue_steps(G, j * P->segment, std::min(m, (j + 1) * P->segment), rtol, maxiter, st); });
    if (!rc) rc = plan_capture(P.get(), [&](hipStream_t st) { return gmres_enqueue_end(G, d_x, st); });
    G->launches_last = launches;
    if (rc) return rc;
    *out = P.release();
    return MI_OK;
}

extern "C" int mi_gmres_plan_solve(mi_gmres_plan_t P, int* iterations, int* reason_out, double* history, mi_stream_t s)
{
    CHECK_ARG(P, "null handle");
    mi_gmres_s* G = P->G;
    if (P->gen != G->gen) return fail(MI_ERR_STATE, "mi_gmres_plan_solve: the solver's operator or preconditioner was set again after the plan was made (make a new plan)");
    hipStream_t st = (hipStream_t)s;
    if (stream_is_capturing(st)) return fail(MI_ERR_STATE, "mi_gmres_plan_solve: the stream is capturing and a solve reads back (capture mi_gmres_cycle_dev instead)");
    const int m = G->m, maxiter = P->maxiter, nseg = P->nseg;
    const bool f32 = G->f32();
    auto replay = [&](int g) {
        P->replays_last++;
        return hipGraphLaunch(P->exec[(size_t)g], st);
    };
    P->replays_last = P->readbacks_last = P->wasted_last = 0;
    G->refused_last = 0, G->last_k = 0;
    bool claimed = false, first = true;
    int its = 0, reason = 0, rc;
    for (;;) {
        HIP_TRY_AS("hipGraphLaunch", replay(first ? 0 : 1));
        // mi_gmres_solve_dev's loop with the segments as batches (the first batch of a cycle: no step, the record of its start)
        GmresRecord rec{};
        int k_enq = 0, seg = 0, pending = -1, rec_slot = -1;
        for (;;) {
            int cur = -1;
            const int room = std::min(m - k_enq, maxiter - its - k_enq);
            if (pending < 0 || room > 0) {
                if (pending >= 0) {
                    HIP_TRY_AS("hipGraphLaunch", replay(2 + seg));
                    k_enq = std::min(m, (seg + 1) * P->segment), seg++;
                }
                if ((rc = gmres_enqueue_readback(G, k_enq, &cur, st))) return rc;
            }
            if (pending >= 0) {
                HIP_TRY(hipEventSynchronize(G->ev[pending]));
                P->readbacks_last++;
                rec_slot = pending;
                memcpy(&rec, G->slot[pending], sizeof(rec));
                if (rec.reason != 0 || cur < 0) break; // frozen (what is enqueued behind it is wasted), or nothing more to enqueue
            }
            pending = cur;
        }
        if (history) {
            if (first) history[0] = rec.rel0;
            for (int j = 0; j < rec.k; j++) history[its + 1 + j] = G->slot[rec_slot][kGmresRecDoubles + j];
        }
        P->wasted_last += k_enq - rec.k;
        its = rec.its;
        G->last_k = rec.k, G->last_beta = rec.beta;
        if (rec.k > 0) HIP_TRY_AS("hipGraphLaunch", replay(2 + nseg)); // (with k == 0 the end would change nothing: not launched, as in mi_gmres_solve_dev)
        // the end of a solve, the reasons and the float basis's claim / confirm: mi_gmres_solve_dev's
        reason = rec.reason == kGmresMetAtStart ? 0 : rec.reason;
        if (claimed && !(rec.reason == 1 && rec.k == 0)) G->refused_last++;
        claimed = f32 && rec.reason == 1 && rec.k > 0;
        if (claimed) {
            first = false;
            continue;
        }
        if (rec.reason != 0) break;
        if (its >= maxiter) {
            reason = 2;
            break;
        }
        first = false;
    }
    if (iterations) *iterations = its;
    if (reason_out) *reason_out = reason;
    return MI_OK;
}

extern "C" int mi_gmres_plan_info(mi_gmres_plan_t P, int* graphs, int* segment, int* replays_last, int* readbacks_last, int* wasted_steps_last)
{
    CHECK_ARG(P, "null handle");
    if (graphs) *graphs = (int)P->exec.size();
    if (segment) *segment = P->segment;
    if (replays_last) *replays_last = P->replays_last;
    if (readbacks_last) *readbacks_last = P->readbacks_last;
    if (wasted_steps_last) *wasted_steps_last = P->wasted_last;
    return MI_OK;
}

extern "C" int mi_gmres_plan_destroy(mi_gmres_plan_t P)
{
    if (!P) return MI_OK;
    (void)hipDeviceSynchronize(); // a replay may still be in flight behind the last solve
    delete P;
    return MI_OK;
}
