// capi_dilu.hip: the 4x4-block DILU preconditioner applied with Eisenstat's trick, mi_dilu4_* — part of libmi355spmv.so (see
// capi_internal.hpp for the layout of the library).  Pivots on the host (dilu4_plan.hpp) or, into the same device arrays, on the
// GPU level by level from values that lie on the device (mi_dilu4dev_*, dilu4_factor.hpp); the three sweeps on the GPU
// (dilu4_kernels.hpp), one launch per (folded) dependency level of the schedule bilu4_plan.hpp computes on the pattern of B.
// Everything a DILU handle has in common with a block ILU handle is capi_bilu_common.hpp's: the argument rules, the host part of
// the handle (ordering, pattern, schedule), the level-major copy of the two triangles, the guard, the steps of a refactor and the
// gather and scatter that bracket every call on an ordered handle (MI_BILU_ORDER_COLOUR).  This file holds what is DILU's own.
// No CPU fallback: the sweeps and the device refactor need a HIP device; create_host, refactor, fetch, info and the plan probe need none.
#include "capi_bilu_common.hpp"
#include "dilu4_plan.hpp"
#include "dilu4_kernels.hpp"
#include "dilu4_factor.hpp"

// the device refactor (mi_dilu4dev_prepare): pattern-only tables, see Dilu4DevPlan
struct Dilu4DevTables {
    bool prepared = false;
    long long nL = 0, nU = 0, plan_bytes = 0;
    DevArray<int> fpos, gather, mate, bad;
};

struct mi_dilu4_s : Bilu4Handle { // sched: fill 0, the pattern is B's own
    std::vector<double> val;        // B's values, B's block order, row-major
    std::vector<double> einv, kmat; // [16 nb] by B's block row
    DevArray<double> d_einv, d_kmat;
    DevArray<double> d_t, d_y;      // the work vectors of apply_hat, B's numbering
    DevArray<double> d_v;           // ordered: the vector every call passes through, B's numbering
    Dilu4DevTables dev;
    ~mi_dilu4_s() { dev = {}, d_v = {}, d_perm = {}, d_y = {}, d_t = {}, d_kmat = {}, d_einv = {}; } // newest first, then the order the handle has always been freed in; the two triangles follow
    Dilu4View view(int b) const { return Dilu4View{lev[b].perm, lev[b].ptr, lev[b].col, lev[b].val, d_einv, d_kmat, lev[b].lev_ptr}; }
    Dilu4FactorView factor_view() const
    {
        return Dilu4FactorView{lev[0].perm, lev[0].ptr, lev[0].col, lev[0].lev_ptr, dev.fpos, dev.mate, lev[0].val, lev[1].val, d_einv, d_kmat, (int)dev.nL, (int)dev.nU, dev.bad};
    }
    long long device_bytes() const
    {
        if (device < 0 || pat().nb == 0) return 0;
        const long long nb = pat().nb, offd = (long long)(lev[0].blocks() + lev[1].blocks());
        long long n = offd * (long long)(16 * sizeof(double) + sizeof(int));                                                // blocks and their columns
        n += 2 * (2 * nb + 1) * (long long)sizeof(int) + (long long)sizeof(int) * (sched.sweep[0].nlev() + sched.sweep[1].nlev() + 2); // perm, ptr, lev_ptr
        n += 2 * 16 * nb * (long long)sizeof(double);                                                                       // Einv, K
        n += 2 * 4 * nb * (long long)sizeof(double);                                                                        // t, y
        if (ord.on()) n += nb * (long long)sizeof(int) + 4 * nb * (long long)sizeof(double);
        return n;
    }
};

constexpr BiluHostOnly kDiluHostOnly{MI_ERR_STATE, ": a host-only handle (mi_dilu4_create_host) has no device copy"};

static int dilu_zero_pivot(int row)
{
    return fail(MI_ERR_ARG, "mi_dilu4: zero pivot (|d| < 1e-12) in the pivot block E of block row " + std::to_string(row));
}

// B's values and the pivots from the caller's coef
static int dilu_factor(mi_dilu4_s* E, const double* coef, int layout)
{
    const auto t0 = std::chrono::steady_clock::now();
    dilu4_values(E->pat().nblocks(), coef, layout == MI_BLOCK_COLMAJOR, E->ord.src_or_null(), E->val.data());
    const int bad = dilu4_pivots(E->pat(), E->sched.sweep[0], E->val.data(), bilu_threads(), E->einv.data(), E->kmat.data());
    E->factor_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return bad >= 0 ? dilu_zero_pivot(E->ord.caller_row(bad)) : MI_OK;
}

// the host values to the device copies: both triangles level-major, Einv and K by block row
static int dilu_upload_values(mi_dilu4_s* E)
{
    if (const int rc = bilu_move_offdiag(E, E->val.data(), true)) return rc;
    HIP_TRY(hipMemcpy(E->d_einv, E->einv.data(), sizeof(double) * E->einv.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(E->d_kmat, E->kmat.data(), sizeof(double) * E->kmat.size(), hipMemcpyHostToDevice));
    return MI_OK;
}

static int dilu_create(int nbrows, const int* ptrow, const int* indcol, const double* coef, int layout, int ordering, bool device, mi_dilu4_t* out)
{
    int rc;
    if ((rc = bilu_check_create("mi_dilu4: ", nbrows, ptrow, indcol, coef, layout, 0, ordering, out))) return rc;
    if (device && (rc = need_device())) return rc;
    std::unique_ptr<mi_dilu4_s> E(new (std::nothrow) mi_dilu4_s);
    if (!E) return fail(MI_ERR_ALLOC, "host allocation failed");
    if ((rc = bilu_plan_host(E.get(), nbrows, ptrow, indcol, 0, ordering, "mi_dilu4_create"))) return rc;
    E->val.assign(16 * (size_t)E->pat().nblocks(), 0.0);
    E->einv.assign(16 * (size_t)nbrows, 0.0);
    E->kmat.assign(16 * (size_t)nbrows, 0.0);
    if ((rc = dilu_factor(E.get(), coef, layout))) return rc;
    if (device && nbrows > 0) {
        HIP_TRY(hipGetDevice(&E->device));
        const size_t n = 4 * (size_t)nbrows;
        if ((rc = bilu_upload_pattern(E.get())) || (rc = dev_alloc(E->d_einv, 16 * (size_t)nbrows)) || (rc = dev_alloc(E->d_kmat, 16 * (size_t)nbrows)) ||
            (rc = dilu_upload_values(E.get())) || (rc = dev_zeros(E->d_t, n)) || (rc = dev_zeros(E->d_y, n)))
            return rc;
        if (E->ord.on() && ((rc = dev_upload(E->d_perm, E->ord.perm, 1)) || (rc = dev_zeros(E->d_v, n)))) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr)); // (the zeroed vectors, before the first call on the caller's stream)
    } else if (device) {
        E->device = 0; // an empty matrix: every call on it is a no-op
    }
    *out = E.release();
    return MI_OK;
}

extern "C" int mi_dilu4_create(int nbrows, const int* ptrow, const int* indcol, const double* coef, int layout, int ordering, mi_dilu4_t* out)
{
    return dilu_create(nbrows, ptrow, indcol, coef, layout, ordering, true, out);
}

extern "C" int mi_dilu4_create_host(int nbrows, const int* ptrow, const int* indcol, const double* coef, int layout, int ordering, mi_dilu4_t* out)
{
    return dilu_create(nbrows, ptrow, indcol, coef, layout, ordering, false, out);
}

extern "C" int mi_dilu4_destroy(mi_dilu4_t E)
{
    delete E;
    return MI_OK;
}

extern "C" int mi_dilu4_refactor(mi_dilu4_t E, const double* coef, int layout)
{
    return bilu_refactor(E, coef, layout, [&] { return dilu_factor(E, coef, layout); }, [&] { return dilu_upload_values(E); });
}

extern "C" int mi_dilu4_fetch(mi_dilu4_t E, double* einv, double* k)
{
    CHECK_ARG(E, "null handle");
    for (int i = 0; i < E->pat().nb; i++) { // the caller's block row i is B's row perm[i]
        const size_t from = 16 * (size_t)(E->ord.on() ? E->ord.perm[i] : i);
        if (einv) memcpy(einv + 16 * (size_t)i, &E->einv[from], sizeof(double) * 16);
        if (k) memcpy(k + 16 * (size_t)i, &E->kmat[from], sizeof(double) * 16);
    }
    return MI_OK;
}

extern "C" int mi_dilu4_info(mi_dilu4_t E, int* nbrows, long long* nblocks, int* ordering, int* ncolours, int* fwd_levels, int* bwd_levels,
                             int* launches, double* factor_seconds, long long* device_bytes, int* perm)
{
    CHECK_ARG(E, "null handle");
    const Bilu4Sweep* S = E->sched.sweep;
    if (nbrows) *nbrows = E->pat().nb;
    if (nblocks) *nblocks = E->pat().nblocks();
    if (ordering) *ordering = E->ord.ordering;
    if (ncolours) *ncolours = E->ord.ncolours;
    if (fwd_levels) *fwd_levels = S[0].nlev();
    if (bwd_levels) *bwd_levels = S[1].nlev();
    if (launches) *launches = S[0].nlaunch() + S[1].nlaunch() + (E->ord.on() ? kBiluOrderLaunches : 0);
    if (factor_seconds) *factor_seconds = E->factor_seconds;
    if (device_bytes) *device_bytes = E->device_bytes();
    for (int i = 0; perm && i < E->pat().nb; i++) perm[i] = E->ord.on() ? E->ord.perm[i] : i;
    return MI_OK;
}

// ---------------------------------------------------------------- mi_dilu4dev_*: the pivots on the GPU
// the plan of a schedule, checked (dilu4dev_check) before anything relies on it; who: the entry point, for the message
static int dilu_dev_plan(const Bilu4Handle* H, const char* who, Dilu4DevPlan* D)
{
    dilu4dev_plan(H->sched, H->a_ptr.data(), H->a_col.data(), D, H->ord.src_or_null());
    const std::string bad = dilu4dev_check(H->sched, *D, H->ord.src_or_null());
    if (!bad.empty()) return fail(MI_ERR_STATE, std::string(who) + ": " + bad);
    return MI_OK;
}

extern "C" int mi_dilu4dev_plan_probe(int nbrows, const int* ptrow, const int* indcol, int ordering, long long* pivot_pairs, int* launches, long long* plan_bytes)
{
    CHECK_ARG(!bilu_bad_ordering(ordering), bilu_bad_ordering(ordering));
    int rc;
    if ((rc = bilu_check_args("mi_dilu4: ", nbrows, ptrow, indcol, 0))) return rc;
    Bilu4Handle H; // the host part only: nothing of it reaches a device
    Dilu4DevPlan D;
    if ((rc = bilu_plan_host(&H, nbrows, ptrow, indcol, 0, ordering, "mi_dilu4dev_plan_probe")) || (rc = dilu_dev_plan(&H, "mi_dilu4dev_plan_probe", &D))) return rc;
    if (pivot_pairs) *pivot_pairs = D.pivot_pairs;
    if (launches) *launches = H.sched.sweep[0].nlaunch() + kDiluDevFixedLaunches;
    if (plan_bytes) *plan_bytes = D.bytes();
    return MI_OK;
}

extern "C" int mi_dilu4dev_prepare(mi_dilu4_t E)
{
    if (const int rc = bilu_guard(E, "mi_dilu4dev_prepare", kDiluHostOnly); rc != kBiluGo) return rc;
    if (E->dev.prepared) return MI_OK;
    Dilu4DevPlan D;
    int rc;
    if ((rc = dilu_dev_plan(E, "mi_dilu4dev_prepare", &D))) return rc;
    Dilu4DevTables T; // moves into the handle once it is complete; a failure on the way frees what there is
    if ((rc = dev_upload(T.fpos, D.fpos, 1)) || (rc = dev_upload(T.gather, D.gather, 1)) || (rc = dev_upload(T.mate, D.mate, 1)) ||
        (rc = dev_upload(T.bad, std::vector<int>(1, kDiluBadNone), 1)))
        return rc;
    T.nL = D.nL, T.nU = D.nU, T.plan_bytes = D.bytes();
    T.prepared = true;
    E->dev = std::move(T);
    return MI_OK;
}

extern "C" int mi_dilu4dev_refactor(mi_dilu4_t E, const double* d_coef, int layout, mi_stream_t s)
{
    if (const int rc = bilu_guard(E, "mi_dilu4dev_refactor", kDiluHostOnly, bilu_bad_layout(layout), d_coef ? nullptr : "null coef"); rc != kBiluGo) return rc;
    int rc;
    if (!E->dev.prepared && (rc = mi_dilu4dev_prepare(E))) return rc;
    hipStream_t st = (hipStream_t)s;
    const Dilu4FactorView V = E->factor_view();
    const long long total = E->pat().nblocks();
    hipLaunchKernelGGL(dilu4f_gather, dim3((unsigned)((total * 16 + kWG - 1) / kWG)), dim3(kWG), 0, st, V, E->dev.gather, total, d_coef, (int)(layout == MI_BLOCK_COLMAJOR));
    const Bilu4Sweep& S = E->sched.sweep[0]; // the pivots follow the forward sweep's launches
    for (int a = 0; a < S.nlaunch(); a++) {
        const Bilu4Launch L = S.launch(a);
        if (L.folded()) {
            hipLaunchKernelGGL(dilu4f_folded, dim3(1), dim3(kDiluFactorFoldedWG), 0, st, V, L.l0, L.l1);
        } else {
            const int grid = (int)(((long long)(L.p1 - L.p0) * 16 + kWG - 1) / kWG);
            hipLaunchKernelGGL(dilu4f_level, dim3(grid), dim3(kWG), 0, st, V, L.p0, L.p1);
        }
    }
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_dilu4dev_status(mi_dilu4_t E, int* bad_row)
{
    if (E && bad_row) *bad_row = -1;
    if (const int rc = bilu_guard(E, "mi_dilu4dev_status", kDiluHostOnly); rc != kBiluGo) return rc;
    if (!E->dev.prepared) return MI_OK; // no device refactor yet
    HIP_TRY(hipDeviceSynchronize());
    int bad = kDiluBadNone;
    HIP_TRY(hipMemcpy(&bad, E->dev.bad, sizeof(int), hipMemcpyDeviceToHost));
    if (bad == kDiluBadNone) return MI_OK;
    bad = E->ord.caller_row(bad);
    if (bad_row) *bad_row = bad;
    return dilu_zero_pivot(bad);
}

// the device's triangles, Einv and K into the host copies; B's diagonal blocks are not kept on the device (Einv and K start from
// them), so those of the host's val stay as the last host refactor left them — nothing reads them but that refactor, which rewrites them
extern "C" int mi_dilu4dev_fetch(mi_dilu4_t E)
{
    if (const int rc = bilu_guard(E, "mi_dilu4dev_fetch", kDiluHostOnly); rc != kBiluGo) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (const int rc = bilu_move_offdiag(E, E->val.data(), false)) return rc;
    HIP_TRY(hipMemcpy(E->einv.data(), E->d_einv, sizeof(double) * E->einv.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(E->kmat.data(), E->d_kmat, sizeof(double) * E->kmat.size(), hipMemcpyDeviceToHost));
    return MI_OK;
}

extern "C" int mi_dilu4dev_info(mi_dilu4_t E, int* prepared, int* launches, long long* plan_bytes)
{
    CHECK_ARG(E, "null handle");
    if (prepared) *prepared = E->dev.prepared ? 1 : 0;
    if (launches) *launches = E->sched.sweep[0].nlaunch() + kDiluDevFixedLaunches;
    if (plan_bytes) *plan_bytes = E->dev.plan_bytes;
    return MI_OK;
}

// ---------------------------------------------------------------- the sweeps
// one sweep of form FORM over its schedule: one launch per (folded) level (Bilu4Launch::folded, the one rule)
template <int FORM, bool AL>
static void dilu_sweep_launch(const mi_dilu4_s* E, const double* in, double* g, const double* t, double* out, hipStream_t s)
{
    constexpr int b = FORM == kDiluFromHat ? 1 : 0;
    const Bilu4Sweep& S = E->sched.sweep[b];
    const Dilu4View V = E->view(b);
    for (int a = 0; a < S.nlaunch(); a++) {
        const Bilu4Launch L = S.launch(a);
        if (L.folded()) {
            hipLaunchKernelGGL((dilu4_folded<FORM, AL>), dim3(1), dim3(kWG), 0, s, V, L.l0, L.l1, in, g, t, out);
        } else {
            const int grid = (L.p1 - L.p0 + kBiluRowsPerWG - 1) / kBiluRowsPerWG;
            hipLaunchKernelGGL((dilu4_level<FORM, AL>), dim3(grid), dim3(kWG), 0, s, V, L.p0, L.p1, in, g, t, out);
        }
    }
}

template <int FORM>
static void dilu_sweep(const mi_dilu4_s* E, const double* in, double* g, const double* t, double* out, hipStream_t s)
{
    bilu_by_alignment(g, [&](auto al) { dilu_sweep_launch<FORM, decltype(al)::value>(E, in, g, t, out, s); return 0; });
}

// a device entry point: the guard, then inner(in, out) in B's numbering — on the caller's own vectors in natural order, on the
// handle's vector, in place, on an ordered handle (bilu_in_order)
template <class Fn>
static int dilu_entry(mi_dilu4_s* E, const char* name, const double* d_in, double* d_out, hipStream_t s, Fn&& inner)
{
    if (const int rc = bilu_guard(E, name, kDiluHostOnly, nullptr, d_in && d_out ? nullptr : "null vector"); rc != kBiluGo) return rc;
    return bilu_in_order(E, d_in, d_out, E->d_v, E->d_v, s, [&](const double* in, double* out) -> int {
        inner(in, out);
        HIP_TRY(hipGetLastError());
        return MI_OK;
    });
}

extern "C" int mi_dilu4_to_hat_dev(mi_dilu4_t E, const double* d_r, double* d_bhat, mi_stream_t s)
{
    return dilu_entry(E, "mi_dilu4_to_hat_dev", d_r, d_bhat, (hipStream_t)s, [&](const double* in, double* out) { dilu_sweep<kDiluToHat>(E, in, out, nullptr, nullptr, (hipStream_t)s); });
}

extern "C" int mi_dilu4_from_hat_dev(mi_dilu4_t E, const double* d_u, double* d_x, mi_stream_t s)
{
    return dilu_entry(E, "mi_dilu4_from_hat_dev", d_u, d_x, (hipStream_t)s, [&](const double* in, double* out) { dilu_sweep<kDiluFromHat>(E, in, out, nullptr, nullptr, (hipStream_t)s); });
}

extern "C" int mi_dilu4_apply_hat_dev(mi_dilu4_t E, const double* d_u, double* d_w, mi_stream_t s)
{
    return dilu_entry(E, "mi_dilu4_apply_hat_dev", d_u, d_w, (hipStream_t)s, [&](const double* in, double* out) {
        dilu_sweep<kDiluFromHat>(E, in, E->d_t, nullptr, nullptr, (hipStream_t)s);
        dilu_sweep<kDiluApply>(E, in, E->d_y, E->d_t, out, (hipStream_t)s);
    });
}
