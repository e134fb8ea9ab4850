// capi_dilu.hip: the 4x4-block DILU preconditioner applied with Eisenstat's trick, mi_dilu4_* — part of libmi355spmv.so (see
// capi_internal.hpp for the layout of the library).  Pivots on the host (dilu4_plan.hpp); the three sweeps on the GPU
// (dilu4_kernels.hpp), one launch per (folded) dependency level of the schedule bilu4_plan.hpp computes on the pattern of B.
// An ordered handle (MI_BILU_ORDER_COLOUR, bilu4_order.hpp) brackets every call with the gather and the scatter of ordered block ILU
// handles (bilu4_order_kernels.hpp).  No CPU fallback: the sweeps need a HIP device; create_host, refactor, fetch and info need none.
#include "capi_internal.hpp"
#include "dilu4_plan.hpp"
#include "dilu4_kernels.hpp"
#include "bilu4_order_kernels.hpp"

#include <thread>

// the level-major copy of one sweep's off-diagonal blocks
struct Dilu4DevSweep {
    DevArray<int> perm, ptr, col;
    DevArray<double> val;
    DevArray<int> lev_ptr;
    std::vector<long long> src; // per device block: its place in the host copy of B's values
    size_t blocks() const { return src.size(); }
};

struct mi_dilu4_s {
    int device = -1; // -1: host-only handle (mi_dilu4_create_host)
    Bilu4Order ord;
    std::vector<int> a_ptr, a_col; // B's pattern: the caller's, or the permuted one, whose blocks ord.src maps back to the caller's
    Bilu4Schedule sched;           // fill 0: the pattern is B's own
    std::vector<double> val;       // B's values, B's block order, row-major
    std::vector<double> einv, kmat; // [16 nb] by B's block row
    double factor_seconds = 0.0;
    Dilu4DevSweep lev[2];          // forward (L), backward (U)
    DevArray<double> d_einv, d_kmat;
    DevArray<double> d_t, d_y;     // the work vectors of apply_hat, B's numbering
    DevArray<int> d_perm;          // ordered: the caller's block row -> B's
    DevArray<double> d_v;          // ordered: the vector every call passes through, B's numbering
    const Bilu4Pattern& pat() const { return sched.pat; }
    Dilu4View view(int b) const { return Dilu4View{lev[b].perm, lev[b].ptr, lev[b].col, lev[b].val, d_einv, d_kmat, lev[b].lev_ptr}; }
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

static int dilu_threads()
{
    const char* e = getenv("MI355_BILU_THREADS");
    if (e && atoi(e) > 0) return atoi(e);
    const unsigned hw = std::thread::hardware_concurrency();
    return (int)std::max(1u, std::min(hw, 16u));
}

static const char* dilu_bad_layout(int layout) { return layout == MI_BLOCK_ROWMAJOR || layout == MI_BLOCK_COLMAJOR ? nullptr : "unknown block layout"; }

// B's values and the pivots from the caller's coef
static int dilu_factor(mi_dilu4_s* E, const double* coef, int layout)
{
    const auto t0 = std::chrono::steady_clock::now();
    dilu4_values(E->pat().nblocks(), coef, layout == MI_BLOCK_COLMAJOR, E->ord.src_or_null(), E->val.data());
    const int bad = dilu4_pivots(E->pat(), E->sched.sweep[0], E->val.data(), dilu_threads(), E->einv.data(), E->kmat.data());
    E->factor_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (bad >= 0) return fail(MI_ERR_ARG, "mi_dilu4: zero pivot (|d| < 1e-12) in the pivot block E of block row " + std::to_string(E->ord.caller_row(bad)));
    return MI_OK;
}

static int dilu_upload_pattern(const mi_dilu4_s* E, int b, Dilu4DevSweep* D)
{
    const Bilu4Pattern& P = E->pat();
    const Bilu4Sweep& S = E->sched.sweep[b];
    std::vector<int> ptr(P.nb + 1, 0), col;
    D->src.clear();
    for (int q = 0; q < P.nb; q++) {
        const auto [k0, k1] = P.offdiag(S.perm[q], b == 1);
        for (int k = k0; k < k1; k++) {
            col.push_back(P.col[k]);
            D->src.push_back(k);
        }
        ptr[q + 1] = (int)col.size();
    }
    int rc;
    if ((rc = dev_upload(D->perm, S.perm, 1)) || (rc = dev_upload(D->ptr, ptr, 1)) || (rc = dev_upload(D->col, col, 1)) ||
        (rc = dev_alloc(D->val, 16 * std::max<size_t>(col.size(), 1))) || (rc = dev_upload(D->lev_ptr, S.lev_ptr, 1)))
        return rc;
    return MI_OK;
}

// the host values to the device copies: both triangles level-major, Einv and K by block row
static int dilu_upload_values(mi_dilu4_s* E)
{
    std::vector<double> v;
    for (int b = 0; b < 2; b++) {
        const Dilu4DevSweep& D = E->lev[b];
        if (!D.blocks()) continue;
        v.resize(16 * D.blocks());
        for (size_t k = 0; k < D.blocks(); k++) memcpy(&v[16 * k], &E->val[16 * (size_t)D.src[k]], sizeof(double) * 16);
        HIP_TRY(hipMemcpy(D.val, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy(E->d_einv, E->einv.data(), sizeof(double) * E->einv.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(E->d_kmat, E->kmat.data(), sizeof(double) * E->kmat.size(), hipMemcpyHostToDevice));
    return MI_OK;
}

static int dilu_create(int nbrows, const int* ptrow, const int* indcol, const double* coef, int layout, int ordering, bool device, mi_dilu4_t* out)
{
    CHECK_ARG(out, "null output handle");
    *out = nullptr;
    CHECK_ARG(!dilu_bad_layout(layout), dilu_bad_layout(layout));
    CHECK_ARG(ordering == MI_BILU_ORDER_NATURAL || ordering == MI_BILU_ORDER_COLOUR, "unknown ordering (0: natural, 1: multicolour)");
    CHECK_ARG(nbrows >= 0, "negative nbrows");
    if (nbrows > 0) {
        CHECK_ARG(ptrow, "null ptrow");
        CHECK_ARG(ptrow[nbrows] <= 0 || indcol, "null indcol");
        const std::string why = bilu4_check_pattern(nbrows, ptrow, indcol);
        if (!why.empty()) return fail(MI_ERR_ARG, "mi_dilu4: " + why);
        CHECK_ARG(coef, "null coef");
    }
    int rc;
    if (device && (rc = need_device())) return rc;
    std::unique_ptr<mi_dilu4_s> E(new (std::nothrow) mi_dilu4_s);
    if (!E) return fail(MI_ERR_ALLOC, "host allocation failed");
    if (nbrows == 0) {
        E->ord.ordering = ordering; // (an empty matrix: no tables, but the handle says what it was asked for)
        E->a_ptr.assign(1, 0);
    } else if (ordering != MI_BILU_ORDER_NATURAL) {
        bilu4_colour(nbrows, ptrow, indcol, &E->ord);
        const std::string bad = bilu4_order_check(nbrows, ptrow, indcol, E->ord);
        if (!bad.empty()) return fail(MI_ERR_STATE, "mi_dilu4_create: " + bad);
        bilu4_permute_pattern(nbrows, ptrow, indcol, &E->ord, &E->a_ptr, &E->a_col);
    } else {
        E->a_ptr.assign(ptrow, ptrow + nbrows + 1);
        E->a_col.assign(indcol, indcol + ptrow[nbrows]);
    }
    bilu4_schedule(nbrows, E->a_ptr.data(), E->a_col.data(), 0, &E->sched);
    E->val.assign(16 * (size_t)E->pat().nblocks(), 0.0);
    E->einv.assign(16 * (size_t)nbrows, 0.0);
    E->kmat.assign(16 * (size_t)nbrows, 0.0);
    if ((rc = dilu_factor(E.get(), coef, layout))) return rc;
    if (device && nbrows > 0) {
        HIP_TRY(hipGetDevice(&E->device));
        const size_t n = 4 * (size_t)nbrows;
        if ((rc = dilu_upload_pattern(E.get(), 0, &E->lev[0])) || (rc = dilu_upload_pattern(E.get(), 1, &E->lev[1])) ||
            (rc = dev_alloc(E->d_einv, 16 * (size_t)nbrows)) || (rc = dev_alloc(E->d_kmat, 16 * (size_t)nbrows)) || (rc = dilu_upload_values(E.get())) ||
            (rc = dev_zeros(E->d_t, n)) || (rc = dev_zeros(E->d_y, n)))
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
    CHECK_ARG(E, "null handle");
    CHECK_ARG(!dilu_bad_layout(layout), dilu_bad_layout(layout));
    if (E->pat().nb == 0) return MI_OK;
    CHECK_ARG(coef, "null coef");
    int rc = dilu_factor(E, coef, layout);
    if (rc || E->device < 0) return rc;
    // sweeps already enqueued read the old values: wait for them, then replace (as mi_bilu4_refactor)
    HIP_TRY(hipDeviceSynchronize());
    return dilu_upload_values(E);
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
    if (launches) *launches = S[0].nlaunch() + S[1].nlaunch() + (E->ord.on() ? 2 : 0);
    if (factor_seconds) *factor_seconds = E->factor_seconds;
    if (device_bytes) *device_bytes = E->device_bytes();
    for (int i = 0; perm && i < E->pat().nb; i++) perm[i] = E->ord.on() ? E->ord.perm[i] : i;
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
    pick([&](auto al) { dilu_sweep_launch<FORM, decltype(al)::value>(E, in, g, t, out, s); return 0; }, (((uintptr_t)g) & 15) == 0);
}

// the two boundary launches of an ordered handle: the caller's vector into B's numbering, and back
template <bool IN>
static void dilu_order_move(const mi_dilu4_s* E, const double* from, double* to, const double* user, hipStream_t s)
{
    const int nb = E->pat().nb;
    pick([&](auto al) {
        constexpr bool AL = decltype(al)::value;
        const int grid = launch_grid((long long)nb * kBiluOrderLanes<AL>, kWG, INT_MAX, 1);
        hipLaunchKernelGGL((bilu4_order_move<IN, AL>), dim3(grid), dim3(kWG), 0, s, E->d_perm, nb, from, to);
        return 0;
    }, (((uintptr_t)user) & 15) == 0);
}

// what every device entry point begins with; kDiluGo: go on
constexpr int kDiluGo = -1;
static int dilu_guard(const mi_dilu4_s* E, const char* name, const void* d_in, const void* d_out)
{
    CHECK_ARG(E, "null handle");
    if (E->pat().nb == 0) return MI_OK;
    CHECK_ARG(d_in && d_out, "null vector");
    if (E->device < 0) return fail(MI_ERR_STATE, std::string(name) + ": a host-only handle (mi_dilu4_create_host) has no device copy");
    return kDiluGo;
}

// op 1 or 2 (FORM) in the caller's numbering: natural order on the caller's own vectors (out is the sweep's gathered vector),
// ordered in place on the handle's vector between a gather and a scatter
template <int FORM>
static int dilu_one_sweep(mi_dilu4_s* E, const double* d_in, double* d_out, hipStream_t s)
{
    if (!E->ord.on()) {
        dilu_sweep<FORM>(E, d_in, d_out, nullptr, nullptr, s);
    } else {
        dilu_order_move<true>(E, d_in, E->d_v, d_in, s);
        dilu_sweep<FORM>(E, E->d_v, E->d_v, nullptr, nullptr, s);
        dilu_order_move<false>(E, E->d_v, d_out, d_out, s);
    }
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_dilu4_to_hat_dev(mi_dilu4_t E, const double* d_r, double* d_bhat, mi_stream_t s)
{
    if (const int rc = dilu_guard(E, "mi_dilu4_to_hat_dev", d_r, d_bhat); rc != kDiluGo) return rc;
    return dilu_one_sweep<kDiluToHat>(E, d_r, d_bhat, (hipStream_t)s);
}

extern "C" int mi_dilu4_from_hat_dev(mi_dilu4_t E, const double* d_u, double* d_x, mi_stream_t s)
{
    if (const int rc = dilu_guard(E, "mi_dilu4_from_hat_dev", d_u, d_x); rc != kDiluGo) return rc;
    return dilu_one_sweep<kDiluFromHat>(E, d_u, d_x, (hipStream_t)s);
}

extern "C" int mi_dilu4_apply_hat_dev(mi_dilu4_t E, const double* d_u, double* d_w, mi_stream_t s)
{
    if (const int rc = dilu_guard(E, "mi_dilu4_apply_hat_dev", d_u, d_w); rc != kDiluGo) return rc;
    hipStream_t st = (hipStream_t)s;
    if (!E->ord.on()) {
        dilu_sweep<kDiluFromHat>(E, d_u, E->d_t, nullptr, nullptr, st);
        dilu_sweep<kDiluApply>(E, d_u, E->d_y, E->d_t, d_w, st);
    } else {
        dilu_order_move<true>(E, d_u, E->d_v, d_u, st);
        dilu_sweep<kDiluFromHat>(E, E->d_v, E->d_t, nullptr, nullptr, st);
        dilu_sweep<kDiluApply>(E, E->d_v, E->d_y, E->d_t, E->d_v, st);
        dilu_order_move<false>(E, E->d_v, d_w, d_w, st);
    }
    HIP_TRY(hipGetLastError());
    return MI_OK;
}
