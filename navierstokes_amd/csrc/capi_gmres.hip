// capi_gmres.hip: mi_gmres_* — right-preconditioned restarted GMRES with a whole cycle enqueued on the device (include/mi355_spmv.h,
// DESIGN.md 4.6) — part of libmi355spmv.so (see capi_internal.hpp for the layout of the library).  The vector work is the library's
// own entry points (the products, mi_bilu4*_solve_dev, mi_cgs_dev, mi_maxpy_dev, mi_axpy_dev); what is new on the device is
// gmres_kernels.hpp.  A handle created with MI_BASIS_F32 stores its Krylov basis in float: the same loop with mi_cgs_f32_dev /
// mi_maxpy_f32_dev / mi_round_f32_dev, and a converged recurrence confirmed by the next cycle's start.  At the end of the file: a
// whole cycle with no read-back (mi_gmres_cycle_dev: the counted steps stay on the device) and the solve as replayed graphs
// (mi_gmres_plan_*), both with the bits of mi_gmres_solve_dev.  The host loop of both solves is gmres_drive.hpp's.  Built for gfx950 only; no CPU fallback: every entry point that computes needs a HIP device.
#include "capi_internal.hpp"
#include "gmres_drive.hpp"
#include "gmres_kernels.hpp"

#include <set>

struct mi_gmres_s {
    int device = 0;
    int n = 0, m = 0;       // rows; restart
    long long ldv = 0;      // n rounded up to even: every row of V is 16-byte aligned
    int basis = MI_BASIS_F64;
    long long ldv32 = 0;    // MI_BASIS_F32: n rounded up to a multiple of 4: every row of V32 is 16-byte aligned
    mi_csr_t A_csr = nullptr;       // the operator: one of these (not owned)
    mi_bcsr4_t A_bcsr = nullptr;
    mi_dilu4_t A_dilu = nullptr;    // ... or the split-preconditioned operator of a block DILU handle (mi_gmres_set_operator_dilu4)
    mi_bilu4_t F = nullptr;         // the preconditioner (not owned), or null
    Bilu4Apply pc{false, false, 0, 0}; // how F is applied (mi_gmres_set_precond*)
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
    G->A_csr = A, G->A_bcsr = nullptr, G->A_dilu = nullptr;
    G->gen++, G->prepared.clear();
    return MI_OK;
}

extern "C" int mi_gmres_set_operator_bcsr4(mi_gmres_t G, mi_bcsr4_t A)
{
    CHECK_ARG(G && A, "null handle");
    CHECK_ARG(A->nbrows == A->nbcols, "the operator must be square");
    CHECK_ARG(4LL * A->nbrows == G->n, "the operator's row count (4 nbrows) is not the solver's n");
    G->A_bcsr = A, G->A_csr = nullptr, G->A_dilu = nullptr;
    G->gen++, G->prepared.clear();
    return MI_OK;
}

extern "C" int mi_gmres_set_operator_dilu4(mi_gmres_t G, mi_dilu4_t E)
{
    CHECK_ARG(G && E, "null handle");
    int nb = 0, rc;
    if ((rc = mi_dilu4_info(E, &nb, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))) return rc;
    CHECK_ARG(4LL * nb == G->n, "the operator's row count (4 nbrows) is not the solver's n");
    if (G->F) return fail(MI_ERR_STATE, "mi_gmres_set_operator_dilu4: a preconditioner is set; the DILU operator has its preconditioner inside (mi_gmres_set_precond(G, NULL, ..) first)");
    G->A_dilu = E, G->A_csr = nullptr, G->A_bcsr = nullptr;
    G->gen++, G->prepared.clear();
    return MI_OK;
}

// MI_GMRES_PC_* -> how the factor is applied: what makes a kind valid, and what decides which prepare it needs
static const Bilu4Apply kGmresPc[] = {{false, false, 0, 0}, {true, false, 0, 0}, {true, true, 0, 0}, {false, true, 0, 0}}; // EXACT, SWEEPS, SWEEPS_F32, EXACT_F32
static_assert(MI_GMRES_PC_EXACT == 0 && MI_GMRES_PC_SWEEPS == 1 && MI_GMRES_PC_SWEEPS_F32 == 2 && MI_GMRES_PC_EXACT_F32 == 3, "kGmresPc is indexed by kind");

// kind and counts are checked first (with a preconditioner they are wrong whatever the solver is), then the handle
extern "C" int mi_gmres_set_precond_ex(mi_gmres_t G, mi_bilu4_t F, int kind, int sweeps_fwd, int sweeps_bwd)
{
    const bool known = kind >= 0 && kind < (int)(sizeof(kGmresPc) / sizeof(kGmresPc[0]));
    CHECK_ARG(!F || known, "unknown preconditioner kind");
    Bilu4Apply how = kGmresPc[known ? kind : 0];
    how.sf = sweeps_fwd, how.sb = sweeps_bwd;
    CHECK_ARG(!F || !how.sweeps || (sweeps_fwd >= 0 && sweeps_bwd >= 0), "negative sweep count");
    CHECK_ARG(G, "null handle");
    if (!F) {
        G->F = nullptr;
        G->gen++;
        return MI_OK;
    }
    if (G->A_dilu) return fail(MI_ERR_STATE, "mi_gmres_set_precond: the operator is a DILU handle's, which has its preconditioner inside");
    int nb = 0, rc;
    if ((rc = mi_bilu4_info(F, &nb, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))) return rc;
    CHECK_ARG(4LL * nb == G->n, "the preconditioner's row count (4 nbrows) is not the solver's n");
    if ((rc = bilu4_apply_prepare(F, how))) return rc; // everything a solve would otherwise allocate on first use
    G->F = F, G->pc = how;
    G->gen++;
    return MI_OK;
}

// the kinds it has always taken (0..2), refused in the order it has always refused: the handle first
extern "C" int mi_gmres_set_precond(mi_gmres_t G, mi_bilu4_t F, int kind, int sweeps_fwd, int sweeps_bwd)
{
    CHECK_ARG(G, "null handle");
    CHECK_ARG(!F || (kind >= MI_GMRES_PC_EXACT && kind <= MI_GMRES_PC_SWEEPS_F32), "unknown preconditioner kind");
    return mi_gmres_set_precond_ex(G, F, kind, sweeps_fwd, sweeps_bwd);
}

static int gmres_mult(mi_gmres_s* G, const double* x, double* y, mi_stream_t s)
{
    if (G->A_dilu) return mi_dilu4_apply_hat_dev(G->A_dilu, x, y, s);
    return G->A_csr ? mi_spmv_dev(G->A_csr, x, y, s) : mi_bcsr4_spmv_dev(G->A_bcsr, x, y, s);
}

constexpr int kCountedOnDevice = -1; // in place of a cycle's counted steps k: only the record has them

// out += sum y_j V_j over the k counted steps of the cycle (the basis as stored); kCountedOnDevice: over the record's k
static int gmres_combine(mi_gmres_s* G, int k, double* out, mi_stream_t s)
{
    const GmresSmall S = G->S();
    if (k == kCountedOnDevice)
        return G->f32() ? mi_maxpy_upto_f32_dev(G->n, G->m, &S.rec()->k, S.y(), 0, G->V32ptr.data(), out, s)
                        : mi_maxpy_upto_dev(G->n, G->m, &S.rec()->k, S.y(), 0, G->Vptr.data(), out, s);
    return G->f32() ? mi_maxpy_f32_dev(G->n, k, S.y(), 0, G->V32ptr.data(), out, nullptr, s)
                    : mi_maxpy_dev(G->n, k, S.y(), 0, G->Vptr.data(), out, nullptr, s);
}

static int gmres_precond(mi_gmres_s* G, const double* in, double* out, mi_stream_t s) { return bilu4_apply_dev(G->F, G->pc, in, out, (hipStream_t)s); }

static int gmres_need_operator(const mi_gmres_s* G, const char* who)
{
    return G->A_csr || G->A_bcsr || G->A_dilu ? MI_OK : fail(MI_ERR_STATE, std::string(who) + ": no operator set (mi_gmres_set_operator_*)");
}

// The enqueue helpers add what they enqueued to `launches`, by the rule of mi_gmres_info (kernels of this file and library calls, each
// counted once); only mi_gmres_solve_dev keeps the sum.

// the start of a cycle, enqueued: r = b - A x into row 0, its norm, the record, V_0 = r / beta (the float basis: r into a work
// vector, then V32_0 = round32(r / beta) and q = widen(V32_0))
static int gmres_enqueue_start(mi_gmres_s* G, const double* d_b, double* d_x, bool first, double rtol, int maxiter, hipStream_t st, int& launches)
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
        hipLaunchKernelGGL(div_by_scalar_kernel, dim3(launch_grid(n, 256, 2048, 1)), dim3(256), 0, st, n, S.beta(), G->row(0));
    }
    HIP_TRY(hipGetLastError());
    launches += first ? 6 : 5;
    return MI_OK;
}

// step k of a cycle, enqueued: w = A M^-1 v, CGS2 of w in place with the raw column where the small problem reads it, the small
// problem, the division.  The double basis: v = V_k and w is row k + 1 itself.  The float basis: v = q = widen(V32_k), the STORED
// vector, w a work vector, CGS2 against V32_0..V32_k, and V32_{k+1} = round32(w / nrm) with q = widen(V32_{k+1}) in one launch
static int gmres_enqueue_step(mi_gmres_s* G, int k, double rtol, int maxiter, hipStream_t st, int& launches)
{
    const GmresSmall S = G->S();
    mi_stream_t s = (mi_stream_t)st;
    const bool f32 = G->f32();
    const double* v = f32 ? G->q.get() : G->row(k);
    double* w = f32 ? G->w.get() : G->row(k + 1);
    double* col = S.hraw() + (size_t)k * (G->m + 2);
    int rc;
    if (G->F && (rc = gmres_precond(G, v, G->z, s))) return rc;
    if ((rc = gmres_mult(G, G->F ? G->z.get() : v, w, s))) return rc;
    if ((rc = f32 ? mi_cgs_f32_dev(G->n, k + 1, G->V32ptr.data(), w, 2, col, col + k + 1, s)
                  : mi_cgs_dev(G->n, k + 1, G->Vptr.data(), w, 2, col, col + k + 1, s)))
        return rc;
    hipLaunchKernelGGL(gmres_hess_step, dim3(1), dim3(64), 0, st, S, k, rtol, maxiter);
    if (f32) {
        if ((rc = mi_round_f32_dev(G->n, w, col + k + 1, G->row32(k + 1), G->q, s))) return rc;
    } else {
        hipLaunchKernelGGL(div_by_scalar_kernel, dim3(launch_grid(G->n, 256, 2048, 1)), dim3(256), 0, st, G->n, col + k + 1, w);
    }
    launches += G->F ? 5 : 4;
    return MI_OK;
}

static int gmres_enqueue_steps(mi_gmres_s* G, int k0, int k1, double rtol, int maxiter, hipStream_t st, int& launches)
{
    for (int k = k0; k < k1; k++)
        if (const int rc = gmres_enqueue_step(G, k, rtol, maxiter, st, launches)) return rc;
    return MI_OK;
}

// the end of a cycle, enqueued: y on the device, then x += M^-1 (V y) over the first k vectors.  k from the host (k > 0), or
// kCountedOnDevice: the back-substitution and the update read the record, and k == 0 changes no bit of x
static int gmres_enqueue_end(mi_gmres_s* G, double* d_x, int k, hipStream_t st, int& launches)
{
    const GmresSmall S = G->S();
    mi_stream_t s = (mi_stream_t)st;
    const int n = G->n;
    int rc;
    if (k == kCountedOnDevice) hipLaunchKernelGGL(gmres_backsolve_counted, dim3(1), dim3(256), 0, st, S);
    else hipLaunchKernelGGL(gmres_backsolve, dim3(1), dim3(256), 0, st, S, k);
    HIP_TRY(hipGetLastError());
    if (G->F) HIP_TRY(hipMemsetAsync(G->w, 0, sizeof(double) * (size_t)n, st));
    if ((rc = gmres_combine(G, k, G->F ? G->w.get() : d_x, s))) return rc;
    if (G->F) {
        if ((rc = gmres_precond(G, G->w, G->z, s))) return rc;
        if (k == kCountedOnDevice) {
            hipLaunchKernelGGL(gmres_update_x, dim3(launch_grid(n / 2, 256, 2048, 1)), dim3(256), 0, st, n, S.rec(), G->z, d_x);
            HIP_TRY(hipGetLastError());
        } else if ((rc = mi_axpy_dev(n, 1.0, G->z, d_x, s))) {
            return rc;
        }
    }
    launches += G->F ? 5 : 2;
    return MI_OK;
}

// what both solves' backends (gmres_drive.hpp) and mi_gmres_state do with the two pinned slots, behind st
struct GmresSlots {
    mi_gmres_s* G;
    hipStream_t st;
    // the record and the cycle's history entries into the next slot, and the event that says so
    int readback(int entries, int* slot)
    {
        const int cur = *slot = G->next_slot;
        G->next_slot ^= 1;
        HIP_TRY(hipMemcpyAsync(G->slot[cur], G->S().base, sizeof(double) * (kGmresRecDoubles + (size_t)entries), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(G->ev[cur], st));
        return MI_OK;
    }
    int wait(int slot, GmresRecord* rec, const double** entries)
    {
        HIP_TRY(hipEventSynchronize(G->ev[slot]));
        memcpy(rec, G->slot[slot], sizeof(*rec));
        *entries = G->slot[slot] + kGmresRecDoubles;
        return MI_OK;
    }
};

// mi_gmres_solve_dev to gmres_drive: launches with the host's k, batches of check_every steps
struct GmresEager : GmresSlots {
    const double* d_b;
    double* d_x;
    double rtol;
    int maxiter, check_every;
    int launches = 0;
    int start(bool first) { return gmres_enqueue_start(G, d_b, d_x, first, rtol, maxiter, st, launches); }
    int batch(int& k_enq, int room, bool first_batch)
    {
        const int k0 = k_enq;
        k_enq = gmres_eager_batch(k0, room, first_batch, check_every);
        return gmres_enqueue_steps(G, k0, k_enq, rtol, maxiter, st, launches);
    }
    int end(int k) { return gmres_enqueue_end(G, d_x, k, st, launches); }
};

extern "C" int mi_gmres_solve_dev(mi_gmres_t G, const double* d_b, double* d_x, double rtol, int maxiter, int check_every, int* iterations,
                                  int* reason_out, double* history, mi_stream_t s)
{
    CHECK_ARG(check_every >= 1, "check_every must be at least 1");
    CHECK_ARG(maxiter >= 0, "negative maxiter");
    CHECK_ARG(G, "null handle");
    CHECK_ARG(d_b && d_x, "null vector");
    if (const int rc = gmres_need_operator(G, "mi_gmres_solve_dev")) return rc;
    hipStream_t st = (hipStream_t)s;
    if (stream_is_capturing(st)) return fail(MI_ERR_STATE, "mi_gmres_solve_dev: the stream is capturing and a solve reads back (it cannot be captured)");
    GmresEager B{{G, st}, d_b, d_x, rtol, maxiter, check_every};
    GmresOutcome out;
    out.last_beta = G->last_beta;
    const int rc = gmres_drive(B, G->m, maxiter, G->f32(), history, out);
    G->readbacks_last = out.readbacks, G->launches_last = B.launches, G->wasted_last = out.wasted, G->refused_last = out.refused;
    G->last_k = out.last_k, G->last_beta = out.last_beta;
    if (rc) return rc;
    if (iterations) *iterations = out.its;
    if (reason_out) *reason_out = out.reason;
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

extern "C" int mi_gmres_prepare_stream(mi_gmres_t G, mi_stream_t s)
{
    CHECK_ARG(G, "null handle");
    int rc;
    if ((rc = gmres_need_operator(G, "mi_gmres_prepare_stream"))) return rc;
    hipStream_t st = (hipStream_t)s;
    if (stream_is_capturing(st)) return fail(MI_ERR_STATE, "mi_gmres_prepare_stream: the stream is capturing (preparing allocates: call it before the capture)");
    if (G->prepared.count(st)) return MI_OK;
    double* ws = nullptr;
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
    int rc, launches = 0; // (not kept: mi_gmres_info describes the last mi_gmres_solve_dev)
    if ((rc = gmres_need_operator(G, "mi_gmres_cycle_dev"))) return rc;
    hipStream_t st = (hipStream_t)s;
    if (stream_is_capturing(st) && !G->prepared.count(st))
        return fail(MI_ERR_STATE, "mi_gmres_cycle_dev: the stream is capturing and was not prepared (mi_gmres_prepare_stream allocates: call it before the capture)");
    if ((rc = gmres_enqueue_start(G, d_b, d_x, first != 0, rtol, maxiter, st, launches)) ||
        (rc = gmres_enqueue_steps(G, 0, G->m, rtol, maxiter, st, launches)) || (rc = gmres_enqueue_end(G, d_x, kCountedOnDevice, st, launches)))
        return rc;
    return MI_OK;
}

extern "C" int mi_gmres_state(mi_gmres_t G, mi_stream_t s, int* its, int* k, int* done, int* reason, double* last, double* beta,
                              double* history_cycle)
{
    CHECK_ARG(G, "null handle");
    hipStream_t st = (hipStream_t)s;
    if (stream_is_capturing(st)) return fail(MI_ERR_STATE, "mi_gmres_state: the stream is capturing and the state is read back (it cannot be captured)");
    GmresSlots io{G, st};
    GmresRecord rec{};
    const double* entries = nullptr;
    int cur = 0, rc, why = 0;
    if ((rc = io.readback(G->m, &cur)) || (rc = io.wait(cur, &rec, &entries))) return rc;
    const bool is_done = gmres_decode(rec, &why);
    G->last_k = rec.k, G->last_beta = rec.beta; // (what mi_gmres_fetch_cycle reports)
    if (its) *its = rec.its;
    if (k) *k = rec.k;
    if (done) *done = is_done;
    if (reason) *reason = why;
    if (last) *last = rec.last;
    if (beta) *beta = rec.beta;
    if (history_cycle)
        for (int j = 0; j < G->m; j++) history_cycle[j] = j < rec.k ? entries[j] : 0.0;
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
    int rc, launches = 0; // (not kept: mi_gmres_info describes the last mi_gmres_solve_dev)
    if ((rc = gmres_need_operator(G, "mi_gmres_plan_create"))) return rc;
    std::unique_ptr<mi_gmres_plan_s> P(new (std::nothrow) mi_gmres_plan_s);
    if (!P) return fail(MI_ERR_ALLOC, "out of host memory");
    const int m = G->m;
    P->G = G, P->gen = G->gen, P->d_b = d_b, P->d_x = d_x, P->rtol = rtol, P->maxiter = maxiter;
    P->segment = std::min(segment, m), P->nseg = (m + P->segment - 1) / P->segment;
    if ((rc = dev_create(P->cap, hipStreamNonBlocking)) || (rc = mi_gmres_prepare_stream(G, (mi_stream_t)(hipStream_t)P->cap))) return rc;
    HIP_TRY(hipStreamSynchronize(P->cap)); // the preparing product wrote the work vectors: over before anything else uses them
    for (int first = 1; first >= 0 && !rc; first--)
        rc = plan_capture(P.get(), [&](hipStream_t st) { return gmres_enqueue_start(G, d_b, d_x, first != 0, rtol, maxiter, st, launches); });
    for (int j = 0; j < P->nseg && !rc; j++)
        rc = plan_capture(P.get(), [&](hipStream_t st) { return gmres_enqueue_steps(G, j * P->segment, std::min(m, (j + 1) * P->segment), rtol, maxiter, st, launches); });
    if (!rc) rc = plan_capture(P.get(), [&](hipStream_t st) { return gmres_enqueue_end(G, d_x, kCountedOnDevice, st, launches); });
    if (rc) return rc;
    *out = P.release();
    return MI_OK;
}

// mi_gmres_plan_solve to gmres_drive: every launch is a replayed graph, the segments are the batches
struct GmresPlanned : GmresSlots {
    mi_gmres_plan_s* P;
    int replay(int g)
    {
        P->replays_last++;
        HIP_TRY_AS("hipGraphLaunch", hipGraphLaunch(P->exec[(size_t)g], st));
        return MI_OK;
    }
    int start(bool first) { return replay(first ? 0 : 1); }
    int batch(int& k_enq, int, bool first_batch)
    {
        int seg;
        k_enq = gmres_plan_batch(k_enq, G->m, first_batch, P->segment, &seg);
        return seg < 0 ? MI_OK : replay(2 + seg);
    }
    int end(int) { return replay(2 + P->nseg); } // (the graph reads k from the record)
};

extern "C" int mi_gmres_plan_solve(mi_gmres_plan_t P, int* iterations, int* reason_out, double* history, mi_stream_t s)
{
    CHECK_ARG(P, "null handle");
    mi_gmres_s* G = P->G;
    if (P->gen != G->gen) return fail(MI_ERR_STATE, "mi_gmres_plan_solve: the solver's operator or preconditioner was set again after the plan was made (make a new plan)");
    hipStream_t st = (hipStream_t)s;
    if (stream_is_capturing(st)) return fail(MI_ERR_STATE, "mi_gmres_plan_solve: the stream is capturing and a solve reads back (capture mi_gmres_cycle_dev instead)");
    GmresPlanned B{{G, st}, P};
    GmresOutcome out;
    out.last_beta = G->last_beta;
    P->replays_last = 0;
    const int rc = gmres_drive(B, G->m, P->maxiter, G->f32(), history, out);
    P->readbacks_last = out.readbacks, P->wasted_last = out.wasted;
    G->refused_last = out.refused, G->last_k = out.last_k, G->last_beta = out.last_beta;
    if (rc) return rc;
    if (iterations) *iterations = out.its;
    if (reason_out) *reason_out = out.reason;
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
