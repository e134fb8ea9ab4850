// capi_ilu.hip: the 4x4-block ILU(k) preconditioner, mi_bilu4_* — part of libmi355spmv.so (see capi_internal.hpp for the layout of
// the library).  Factored on the host (bilu4_plan.hpp), solved on the GPU by one launch per (folded) dependency level
// (bilu4_solve.hpp) or, where the handle was told so (mi_bilu4_set_solve_form), by ONE launch of persistent workgroups
// (bilu4_solve_one.hpp, mi_bilu4one_*); mi_bilu4dev_* refactors on the GPU, into the same device copies, level by level
// (bilu4_factor.hpp).
// No CPU fallback: the solve and the device refactor need a HIP device; the planning and host factorisation entry points need none.
#include "capi_internal.hpp"
#include "bilu4_plan.hpp"
#include "bilu4_solve.hpp"
#include "bilu4_solve_one.hpp"
#include "bilu4_factor.hpp"

struct Bilu4DevSweep {
    int* perm = nullptr;
    int* ptr = nullptr;
    int* col = nullptr;
    double* val = nullptr;
    double* dinv = nullptr;
    int* lev_ptr = nullptr;
    std::vector<long long> src; // per device block: its place in the host factor (refactor re-gathers through it)
    void release()
    {
        dfree(perm), dfree(ptr), dfree(col), dfree(val), dfree(dinv), dfree(lev_ptr);
        perm = ptr = col = lev_ptr = nullptr;
        val = dinv = nullptr;
    }
    Bilu4SweepView view() const { return Bilu4SweepView{perm, ptr, col, val, dinv, lev_ptr}; }
};

// the one-launch solve's tables of one sweep on the device (Bilu4OneSweep)
struct Bilu4OneDev {
    int* chunk_pos = nullptr;
    int* chunk_lev = nullptr;
    int* dep_ptr = nullptr;
    int* dep = nullptr;
    unsigned* flags = nullptr;
    int nchunks = 0;
    void release()
    {
        dfree(chunk_pos), dfree(chunk_lev), dfree(dep_ptr), dfree(dep), dfree(flags);
        chunk_pos = chunk_lev = dep_ptr = dep = nullptr;
        flags = nullptr;
    }
    Bilu4OneTab tab() const { return Bilu4OneTab{chunk_pos, chunk_lev, dep_ptr, dep, flags, nchunks}; }
};

struct mi_bilu4_s {
    int device = -1; // -1: host-only handle (mi_bilu4_create_host)
    int fill = 0;
    std::vector<int> a_ptr, a_col; // the matrix's pattern (refactor scatters new values through it)
    Bilu4Pattern pat;
    std::vector<double> val;       // host factor, row order, row-major blocks
    Bilu4Sweep fwd, bwd;
    Bilu4DevSweep dfwd, dbwd;
    double factor_seconds = 0.0;
    double us_form[2] = {0.0, 0.0}; // [0] one launch per level, measured at create; [1] one launch, once mi_bilu4_set_solve_form(F, -1) has measured it
    double* d_b = nullptr;          // scratch of the host-pointer solve
    double* d_x = nullptr;
    // the device refactor (mi_bilu4dev_prepare): pattern-only tables, see Bilu4DevPlan
    bool dev_prepared = false;
    long long dev_nL = 0, dev_nU = 0, dev_plan_bytes = 0;
    int* d_fpos = nullptr;
    int* d_bpos = nullptr;
    int* d_gather = nullptr;
    int* d_upd = nullptr;
    long long* d_upd_ptr = nullptr;
    int* d_bad = nullptr;
    // the one-launch solve (mi_bilu4one_prepare): chunks, dependency lists, flags, see Bilu4OnePlan
    int form = MI_BILU_FORM_LEVELS;
    int one_state = 0; // 0: not prepared; 1: prepared; -1: not eligible (one_why)
    std::string one_why;
    int one_wgs = 0, one_nchunks[2] = {0, 0}, one_max_deps[2] = {0, 0};
    long long one_plan_bytes = 0;
    Bilu4OneDev one[2];
    unsigned* d_one_counter = nullptr;
    unsigned* h_one_giveups = nullptr; // host-mapped, sticky
    unsigned* d_one_giveups = nullptr;
    unsigned one_epoch = 0;
};

static int bilu_threads()
{
    const char* e = getenv("MI355_BILU_THREADS");
    if (e && atoi(e) > 0) return atoi(e);
    const unsigned hw = std::thread::hardware_concurrency();
    return (int)std::max(1u, std::min(hw, 16u));
}

static int bilu_check_args(int nbrows, const int* ptrow, const int* indcol, int fill)
{
    CHECK_ARG(nbrows >= 0, "negative nbrows");
    CHECK_ARG(fill >= 0, "fill must be >= 0");
    if (nbrows == 0) return MI_OK;
    CHECK_ARG(ptrow, "null ptrow");
    CHECK_ARG(ptrow[nbrows] <= 0 || indcol, "null indcol");
    const std::string why = bilu4_check_pattern(nbrows, ptrow, indcol);
    if (!why.empty()) return fail(MI_ERR_ARG, "mi_bilu4: " + why);
    return MI_OK;
}

static int bilu_factor(mi_bilu4_s* F, const double* coef, int layout)
{
    const auto t0 = std::chrono::steady_clock::now();
    const int bad = bilu4_factor(F->pat, F->fwd, F->a_ptr.data(), F->a_col.data(), coef, layout == MI_BLOCK_COLMAJOR, bilu_threads(), F->val.data());
    F->factor_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (bad >= 0) return fail(MI_ERR_ARG, "mi_bilu4: zero pivot (|d| < 1e-12) in the diagonal block of block row " + std::to_string(bad));
    return MI_OK;
}

// the level-major copy of one sweep
static int bilu_upload_pattern(const mi_bilu4_s* F, bool backward, Bilu4DevSweep* D)
{
    const Bilu4Pattern& P = F->pat;
    const Bilu4Sweep& S = backward ? F->bwd : F->fwd;
    const int nb = P.nb;
    std::vector<int> ptr(nb + 1, 0), col;
    D->src.clear();
    for (int q = 0; q < nb; q++) {
        const int i = S.perm[q];
        const int k0 = backward ? P.diag[i] + 1 : P.ptr[i], k1 = backward ? P.ptr[i + 1] : P.diag[i];
        for (int k = k0; k < k1; k++) {
            col.push_back(P.col[k]);
            D->src.push_back(k);
        }
        ptr[q + 1] = (int)col.size();
    }
    const size_t nblk = col.size();
    HIP_TRY(hipMalloc(&D->perm, sizeof(int) * nb));
    HIP_TRY(hipMalloc(&D->ptr, sizeof(int) * (nb + 1)));
    HIP_TRY(hipMalloc(&D->col, sizeof(int) * std::max<size_t>(nblk, 1)));
    HIP_TRY(hipMalloc(&D->val, sizeof(double) * 16 * std::max<size_t>(nblk, 1)));
    HIP_TRY(hipMalloc(&D->lev_ptr, sizeof(int) * S.lev_ptr.size()));
    if (backward) HIP_TRY(hipMalloc(&D->dinv, sizeof(double) * 16 * nb));
    HIP_TRY(hipMemcpy(D->perm, S.perm.data(), sizeof(int) * nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(D->ptr, ptr.data(), sizeof(int) * (nb + 1), hipMemcpyHostToDevice));
    if (nblk) HIP_TRY(hipMemcpy(D->col, col.data(), sizeof(int) * nblk, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(D->lev_ptr, S.lev_ptr.data(), sizeof(int) * S.lev_ptr.size(), hipMemcpyHostToDevice));
    return MI_OK;
}

static int bilu_upload_values(const mi_bilu4_s* F, bool backward, Bilu4DevSweep* D)
{
    const int nb = F->pat.nb;
    std::vector<double> v(16 * std::max<size_t>(D->src.size(), 1));
    for (size_t b = 0; b < D->src.size(); b++) memcpy(&v[16 * b], &F->val[16 * (size_t)D->src[b]], sizeof(double) * 16);
    if (!D->src.empty()) HIP_TRY(hipMemcpy(D->val, v.data(), sizeof(double) * 16 * D->src.size(), hipMemcpyHostToDevice));
    if (backward) {
        v.resize(16 * (size_t)nb);
        for (int q = 0; q < nb; q++) memcpy(&v[16 * (size_t)q], &F->val[16 * (size_t)F->pat.diag[F->bwd.perm[q]]], sizeof(double) * 16);
        HIP_TRY(hipMemcpy(D->dinv, v.data(), sizeof(double) * 16 * nb, hipMemcpyHostToDevice));
    }
    return MI_OK;
}

template <bool BWD, bool AL>
static void bilu_sweep_launch(const Bilu4Sweep& S, const Bilu4SweepView& V, const double* src, double* x, hipStream_t s)
{
    for (int a = 0; a < S.nlaunch(); a++) {
        const int l0 = S.launch_ptr[a], l1 = S.launch_ptr[a + 1];
        const int p0 = S.lev_ptr[l0], p1 = S.lev_ptr[l1];
        if (l1 - l0 > 1 || p1 - p0 < kBiluRowsPerWG) {
            hipLaunchKernelGGL((bilu4_folded<BWD, AL>), dim3(1), dim3(kWG), 0, s, V, l0, l1, src, x);
        } else {
            const int grid = (p1 - p0 + kBiluRowsPerWG - 1) / kBiluRowsPerWG;
            hipLaunchKernelGGL((bilu4_level<BWD, AL>), dim3(grid), dim3(kWG), 0, s, V, p0, p1, src, x);
        }
    }
}

// form A: one launch per (folded) level, forward then backward, on the caller's stream; nothing allocated or synchronised
static int bilu_solve_launch(mi_bilu4_s* F, const double* d_b, double* d_x, hipStream_t s)
{
    const Bilu4SweepView vf = F->dfwd.view(), vb = F->dbwd.view();
    if ((((uintptr_t)d_x) & 15) == 0) {
        bilu_sweep_launch<false, true>(F->fwd, vf, d_b, d_x, s);
        bilu_sweep_launch<true, true>(F->bwd, vb, d_x, d_x, s);
    } else {
        bilu_sweep_launch<false, false>(F->fwd, vf, d_b, d_x, s);
        bilu_sweep_launch<true, false>(F->bwd, vb, d_x, d_x, s);
    }
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

static const char* const kOneGaveUp =
    "mi_bilu4: a hand-off wait of the one-launch solve gave up (workgroups of the grid were not all resident: another kernel held CUs); "
    "results since then are invalid — call mi_bilu4_set_solve_form(F, 0) to clear this and solve level by level";

static bool bilu_one_gave_up(const mi_bilu4_s* F) { return F->h_one_giveups && __atomic_load_n(F->h_one_giveups, __ATOMIC_ACQUIRE) != 0; }

template <bool AL>
static hipError_t bilu_one_launch_t(const mi_bilu4_s* F, const Bilu4OneArgs& A, const double* d_b, double* d_x, hipStream_t s, bool query, int* max_blocks)
{
    auto kern = bilu4_solve_one<AL>;
    if (query) return hipOccupancyMaxActiveBlocksPerMultiprocessor(max_blocks, kern, kWG, 0);
    hipLaunchKernelGGL(kern, dim3(F->one_wgs), dim3(kWG), 0, s, F->dfwd.view(), F->dbwd.view(), A, d_b, d_x);
    return hipGetLastError();
}

// form 1: both sweeps in one launch of F->one_wgs persistent workgroups.  ONE solve at a time per handle: the epoch is per handle.
static int bilu_solve_one_launch(mi_bilu4_s* F, const double* d_b, double* d_x, hipStream_t s)
{
    Bilu4OneArgs A{};
    A.fwd = F->one[0].tab();
    A.bwd = F->one[1].tab();
    A.epoch = ++F->one_epoch; // flags are never cleared: this solve's are the ones that carry its epoch
    A.counter = F->d_one_counter;
    A.giveups = F->d_one_giveups;
    static const unsigned spin_max = 1u << (getenv("MI355_BILU_ONE_SPIN_LOG2") ? std::max(8, std::min(30, atoi(getenv("MI355_BILU_ONE_SPIN_LOG2")))) : 21);
    A.spin_max = spin_max;
    const hipError_t e = (((uintptr_t)d_x) & 15) == 0 ? bilu_one_launch_t<true>(F, A, d_b, d_x, s, false, nullptr) : bilu_one_launch_t<false>(F, A, d_b, d_x, s, false, nullptr);
    if (e != hipSuccess) return fail(MI_ERR_HIP, std::string("one-launch ILU solve: ") + hipGetErrorString(e));
    return MI_OK;
}

// what mi_bilu4_solve* enqueue: the handle's form — except under stream capture, where the level-by-level form is recorded (the
// one-launch form's epoch is a kernel argument: a replayed graph would present it again and every wait would pass at once)
static int bilu_solve_any(mi_bilu4_s* F, const double* d_b, double* d_x, hipStream_t s)
{
    if (bilu_one_gave_up(F)) return fail(MI_ERR_HIP, kOneGaveUp);
    if (F->form == MI_BILU_FORM_ONE && !stream_is_capturing(s)) return bilu_solve_one_launch(F, d_b, d_x, s);
    return bilu_solve_launch(F, d_b, d_x, s);
}

static void bilu_one_release(mi_bilu4_s* F)
{
    F->one[0].release();
    F->one[1].release();
    dfree(F->d_one_counter);
    if (F->h_one_giveups) (void)hipHostFree(F->h_one_giveups);
    F->d_one_counter = F->h_one_giveups = F->d_one_giveups = nullptr;
}

static void bilu_free(mi_bilu4_s* F)
{
    if (!F) return;
    bilu_one_release(F);
    F->dfwd.release();
    F->dbwd.release();
    dfree(F->d_b);
    dfree(F->d_x);
    dfree(F->d_fpos), dfree(F->d_bpos), dfree(F->d_gather), dfree(F->d_upd), dfree(F->d_upd_ptr), dfree(F->d_bad);
    delete F;
}

static int bilu_create(int nbrows, const int* ptrow, const int* indcol, const double* coef, int layout, int fill, bool device, mi_bilu4_t* out)
{
    CHECK_ARG(out, "null output handle");
    *out = nullptr;
    CHECK_ARG(layout == MI_BLOCK_ROWMAJOR || layout == MI_BLOCK_COLMAJOR, "unknown block layout");
    int rc = bilu_check_args(nbrows, ptrow, indcol, fill);
    if (rc) return rc;
    CHECK_ARG(nbrows == 0 || coef, "null coef");
    if (const char* e = getenv("MI355_BILU_FORM")) {
        CHECK_ARG(!strcmp(e, "0") || !strcmp(e, "1"), "MI355_BILU_FORM must be 0 or 1");
        if (!strcmp(e, "1"))
            return fail(MI_ERR_UNSUPPORTED, "MI355_BILU_FORM=1: the one-launch form of the solve is not built in this version (form 0: one launch per level)");
    }
    if (device && (rc = need_device())) return rc;
    mi_bilu4_s* F = new (std::nothrow) mi_bilu4_s;
    if (!F) return fail(MI_ERR_ALLOC, "host allocation failed");
    F->fill = fill;
    if (nbrows > 0) {
        F->a_ptr.assign(ptrow, ptrow + nbrows + 1);
        F->a_col.assign(indcol, indcol + ptrow[nbrows]);
    } else {
        F->a_ptr.assign(1, 0);
    }
    bilu4_symbolic(nbrows, F->a_ptr.data(), F->a_col.data(), fill, &F->pat);
    bilu4_sweep(F->pat, false, &F->fwd);
    bilu4_sweep(F->pat, true, &F->bwd);
    F->val.assign(16 * (size_t)F->pat.nblocks(), 0.0);
    if ((rc = bilu_factor(F, coef, layout))) {
        bilu_free(F);
        return rc;
    }
    if (device && nbrows > 0) {
        auto up = [&]() -> int {
            HIP_TRY(hipGetDevice(&F->device));
            int r;
            if ((r = bilu_upload_pattern(F, false, &F->dfwd)) || (r = bilu_upload_pattern(F, true, &F->dbwd))) return r;
            if ((r = bilu_upload_values(F, false, &F->dfwd)) || (r = bilu_upload_values(F, true, &F->dbwd))) return r;
            HIP_TRY(hipMalloc(&F->d_b, sizeof(double) * 4 * nbrows));
            HIP_TRY(hipMalloc(&F->d_x, sizeof(double) * 4 * nbrows));
            HIP_TRY(hipMemset(F->d_b, 0, sizeof(double) * 4 * nbrows));
            // the solve's time, through the library's one timing helper (zero right-hand side: the time does not depend on values)
            LaunchTimer T(nullptr);
            if ((r = T.init())) return r;
            if ((r = T.time(2, 5, [&] { return bilu_solve_launch(F, F->d_b, F->d_x, nullptr); }, &F->us_form[0]))) return r;
            return MI_OK;
        };
        if ((rc = up())) {
            bilu_free(F);
            return rc;
        }
    } else if (device) {
        F->device = 0; // an empty matrix: every call on it is a no-op
    }
    *out = F;
    return MI_OK;
}

extern "C" int mi_bilu4_create(int nbrows, const int* ptrow, const int* indcol, const double* coef, int layout, int fill, mi_bilu4_t* out)
{
    return bilu_create(nbrows, ptrow, indcol, coef, layout, fill, true, out);
}

extern "C" int mi_bilu4_create_host(int nbrows, const int* ptrow, const int* indcol, const double* coef, int layout, int fill, mi_bilu4_t* out)
{
    return bilu_create(nbrows, ptrow, indcol, coef, layout, fill, false, out);
}

extern "C" int mi_bilu4_destroy(mi_bilu4_t F)
{
    bilu_free(F);
    return MI_OK;
}

extern "C" int mi_bilu4_refactor(mi_bilu4_t F, const double* coef, int layout)
{
    CHECK_ARG(F, "null handle");
    CHECK_ARG(layout == MI_BLOCK_ROWMAJOR || layout == MI_BLOCK_COLMAJOR, "unknown block layout");
    if (F->pat.nb == 0) return MI_OK;
    CHECK_ARG(coef, "null coef");
    int rc = bilu_factor(F, coef, layout);
    if (rc) return rc;
    if (F->device < 0) return MI_OK;
    // solves already enqueued read the old values: wait for them, then replace (a Newton step refactors between solves)
    HIP_TRY(hipDeviceSynchronize());
    if ((rc = bilu_upload_values(F, false, &F->dfwd)) || (rc = bilu_upload_values(F, true, &F->dbwd))) return rc;
    return MI_OK;
}

extern "C" int mi_bilu4_solve_dev(mi_bilu4_t F, const double* d_b, double* d_x, mi_stream_t s)
{
    CHECK_ARG(F, "null handle");
    if (F->pat.nb == 0) return MI_OK;
    CHECK_ARG(d_b && d_x, "null vector");
    if (F->device < 0) return fail(MI_ERR_STATE, "mi_bilu4_solve: a host-only handle (mi_bilu4_create_host) has no device factor");
    return bilu_solve_any(F, d_b, d_x, (hipStream_t)s);
}

extern "C" int mi_bilu4_solve(mi_bilu4_t F, const double* b, double* x)
{
    CHECK_ARG(F, "null handle");
    if (F->pat.nb == 0) return MI_OK;
    CHECK_ARG(b && x, "null vector");
    if (F->device < 0) return fail(MI_ERR_STATE, "mi_bilu4_solve: a host-only handle (mi_bilu4_create_host) has no device factor");
    const size_t bytes = sizeof(double) * 4 * (size_t)F->pat.nb;
    HIP_TRY(hipMemcpy(F->d_b, b, bytes, hipMemcpyHostToDevice));
    int rc = bilu_solve_any(F, F->d_b, F->d_x, nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(x, F->d_x, bytes, hipMemcpyDeviceToHost));
    return MI_OK;
}

extern "C" int mi_bilu4_info(mi_bilu4_t F, int* nbrows, long long* nblocks, int* fwd_levels, int* bwd_levels, int* launches, int* form,
                             double us[2], double* factor_seconds, long long* factor_bytes)
{
    CHECK_ARG(F, "null handle");
    if (nbrows) *nbrows = F->pat.nb;
    if (nblocks) *nblocks = F->pat.nblocks();
    if (fwd_levels) *fwd_levels = F->fwd.nlev();
    if (bwd_levels) *bwd_levels = F->bwd.nlev();
    if (launches) *launches = F->form == MI_BILU_FORM_ONE ? 1 : F->fwd.nlaunch() + F->bwd.nlaunch();
    if (form) *form = F->form;
    if (us) us[0] = F->us_form[0], us[1] = F->us_form[1];
    if (factor_seconds) *factor_seconds = F->factor_seconds;
    if (factor_bytes) *factor_bytes = F->pat.nblocks() * (long long)(16 * sizeof(double) + sizeof(int)) + (long long)F->pat.nb * 4 * (long long)sizeof(int);
    return MI_OK;
}

extern "C" int mi_bilu4_factor_host(mi_bilu4_t F, int* ptr, int* col, int* diag, double* val, long long cap_blocks)
{
    CHECK_ARG(F, "null handle");
    const long long nblk = F->pat.nblocks();
    CHECK_ARG(cap_blocks >= nblk || (!col && !val), "arrays too short: need mi_bilu4_info's nblocks entries");
    const int nb = F->pat.nb;
    if (ptr && nb) memcpy(ptr, F->pat.ptr.data(), sizeof(int) * (nb + 1));
    if (ptr && !nb) ptr[0] = 0;
    if (col && nblk) memcpy(col, F->pat.col.data(), sizeof(int) * nblk);
    if (diag && nb) memcpy(diag, F->pat.diag.data(), sizeof(int) * nb);
    if (val && nblk) memcpy(val, F->val.data(), sizeof(double) * 16 * nblk);
    return MI_OK;
}

extern "C" int mi_bilu4_plan_probe(int nbrows, const int* ptrow, const int* indcol, int fill, long long* nblocks, int* fwd_levels,
                                   int* bwd_levels, int* fwd_launches, int* bwd_launches, int* fwd_sizes, int* bwd_sizes, int cap_levels)
{
    int rc = bilu_check_args(nbrows, ptrow, indcol, fill);
    if (rc) return rc;
    Bilu4Pattern P;
    Bilu4Sweep Fw, Bw;
    bilu4_symbolic(nbrows, ptrow, indcol, fill, &P);
    bilu4_sweep(P, false, &Fw);
    bilu4_sweep(P, true, &Bw);
    if (nblocks) *nblocks = P.nblocks();
    if (fwd_levels) *fwd_levels = Fw.nlev();
    if (bwd_levels) *bwd_levels = Bw.nlev();
    if (fwd_launches) *fwd_launches = Fw.nlaunch();
    if (bwd_launches) *bwd_launches = Bw.nlaunch();
    CHECK_ARG((!fwd_sizes || cap_levels >= Fw.nlev()) && (!bwd_sizes || cap_levels >= Bw.nlev()), "level-size arrays too short");
    if (fwd_sizes)
        for (int l = 0; l < Fw.nlev(); l++) fwd_sizes[l] = Fw.lev_ptr[l + 1] - Fw.lev_ptr[l];
    if (bwd_sizes)
        for (int l = 0; l < Bw.nlev(); l++) bwd_sizes[l] = Bw.lev_ptr[l + 1] - Bw.lev_ptr[l];
    return MI_OK;
}

// ---------------------------------------------------------------- mi_bilu4dev_*: the numeric factorisation on the GPU
static const char* const kHostOnlyDev = ": a host-only handle (mi_bilu4_create_host) has no device factor";

extern "C" int mi_bilu4dev_plan_probe(int nbrows, const int* ptrow, const int* indcol, int fill, long long* update_pairs, int* launches,
                                      long long* plan_bytes)
{
    int rc = bilu_check_args(nbrows, ptrow, indcol, fill);
    if (rc) return rc;
    Bilu4Pattern P;
    Bilu4Sweep Fw, Bw;
    Bilu4DevPlan D;
    bilu4_symbolic(nbrows, ptrow, indcol, fill, &P);
    bilu4_sweep(P, false, &Fw);
    bilu4_sweep(P, true, &Bw);
    bilu4dev_plan(P, Fw, Bw, ptrow, indcol, &D);
    if (update_pairs) *update_pairs = D.update_pairs;
    if (launches) *launches = Fw.nlaunch() + kBiluDevFixedLaunches;
    if (plan_bytes) *plan_bytes = D.bytes();
    return MI_OK;
}

template <class T>
static int bilu_dev_table(const std::vector<T>& h, T** d)
{
    HIP_TRY(hipMalloc(d, sizeof(T) * std::max<size_t>(h.size(), 1)));
    if (!h.empty()) HIP_TRY(hipMemcpy(*d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
    return MI_OK;
}

extern "C" int mi_bilu4dev_prepare(mi_bilu4_t F)
{
    CHECK_ARG(F, "null handle");
    if (F->pat.nb == 0) return MI_OK;
    if (F->device < 0) return fail(MI_ERR_STATE, std::string("mi_bilu4dev_prepare") + kHostOnlyDev);
    if (F->dev_prepared) return MI_OK;
    Bilu4DevPlan D;
    bilu4dev_plan(F->pat, F->fwd, F->bwd, F->a_ptr.data(), F->a_col.data(), &D);
    auto up = [&]() -> int {
        int rc;
        if ((rc = bilu_dev_table(D.fpos, &F->d_fpos)) || (rc = bilu_dev_table(D.bpos, &F->d_bpos)) || (rc = bilu_dev_table(D.gather, &F->d_gather)) ||
            (rc = bilu_dev_table(D.upd, &F->d_upd)) || (rc = bilu_dev_table(D.upd_ptr, &F->d_upd_ptr)))
            return rc;
        if (!F->d_bad) HIP_TRY(hipMalloc(&F->d_bad, sizeof(int)));
        const int none = kBiluBadNone;
        HIP_TRY(hipMemcpy(F->d_bad, &none, sizeof(int), hipMemcpyHostToDevice));
        return MI_OK;
    };
    if (int rc = up()) {
        dfree(F->d_fpos), dfree(F->d_bpos), dfree(F->d_gather), dfree(F->d_upd), dfree(F->d_upd_ptr);
        F->d_fpos = F->d_bpos = F->d_gather = F->d_upd = nullptr;
        F->d_upd_ptr = nullptr;
        return rc;
    }
    F->dev_nL = D.nL, F->dev_nU = D.nU, F->dev_plan_bytes = D.bytes();
    F->dev_prepared = true;
    return MI_OK;
}

extern "C" int mi_bilu4dev_refactor(mi_bilu4_t F, const double* d_coef, int layout, mi_stream_t s)
{
    CHECK_ARG(F, "null handle");
    CHECK_ARG(layout == MI_BLOCK_ROWMAJOR || layout == MI_BLOCK_COLMAJOR, "unknown block layout");
    if (F->pat.nb == 0) return MI_OK;
    CHECK_ARG(d_coef, "null coef");
    if (F->device < 0) return fail(MI_ERR_STATE, std::string("mi_bilu4dev_refactor") + kHostOnlyDev);
    int rc;
    if (!F->dev_prepared && (rc = mi_bilu4dev_prepare(F))) return rc;
    hipStream_t st = (hipStream_t)s;
    const Bilu4FactorView V{F->dfwd.perm, F->dfwd.ptr, F->dfwd.col, F->dbwd.ptr, F->dfwd.lev_ptr, F->d_fpos, F->d_bpos, F->d_upd_ptr, F->d_upd,
                            F->dfwd.val, F->dbwd.val, F->dbwd.dinv, (int)F->dev_nL, (int)F->dev_nU, F->d_bad};
    const long long total = F->pat.nblocks();
    hipLaunchKernelGGL(bilu4f_gather, dim3((unsigned)((total * 16 + kWG - 1) / kWG)), dim3(kWG), 0, st, V, F->d_gather, total, d_coef,
                       (int)(layout == MI_BLOCK_COLMAJOR));
    const Bilu4Sweep& S = F->fwd;
    for (int a = 0; a < S.nlaunch(); a++) {
        const int l0 = S.launch_ptr[a], l1 = S.launch_ptr[a + 1];
        const int p0 = S.lev_ptr[l0], p1 = S.lev_ptr[l1];
        if (l1 - l0 > 1 || p1 - p0 < kBiluRowsPerWG) {
            hipLaunchKernelGGL(bilu4f_folded, dim3(1), dim3(kBiluFactorFoldedWG), 0, st, V, l0, l1);
        } else {
            const int grid = (int)(((long long)(p1 - p0) * 16 + kWG - 1) / kWG);
            hipLaunchKernelGGL(bilu4f_level, dim3(grid), dim3(kWG), 0, st, V, p0, p1);
        }
    }
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_bilu4dev_status(mi_bilu4_t F, int* bad_row)
{
    CHECK_ARG(F, "null handle");
    if (bad_row) *bad_row = -1;
    if (F->pat.nb == 0) return MI_OK;
    if (F->device < 0) return fail(MI_ERR_STATE, std::string("mi_bilu4dev_status") + kHostOnlyDev);
    if (!F->dev_prepared) return MI_OK; // no device refactor yet
    HIP_TRY(hipDeviceSynchronize());
    int bad = kBiluBadNone;
    HIP_TRY(hipMemcpy(&bad, F->d_bad, sizeof(int), hipMemcpyDeviceToHost));
    if (bad == kBiluBadNone) return MI_OK;
    if (bad_row) *bad_row = bad;
    return fail(MI_ERR_ARG, "mi_bilu4: zero pivot (|d| < 1e-12) in the diagonal block of block row " + std::to_string(bad));
}

extern "C" int mi_bilu4dev_fetch(mi_bilu4_t F)
{
    CHECK_ARG(F, "null handle");
    if (F->pat.nb == 0) return MI_OK;
    if (F->device < 0) return fail(MI_ERR_STATE, std::string("mi_bilu4dev_fetch") + kHostOnlyDev);
    HIP_TRY(hipDeviceSynchronize());
    const int nb = F->pat.nb;
    std::vector<double> v;
    for (const Bilu4DevSweep* D : {&F->dfwd, &F->dbwd}) {
        if (D->src.empty()) continue;
        v.resize(16 * D->src.size());
        HIP_TRY(hipMemcpy(v.data(), D->val, sizeof(double) * v.size(), hipMemcpyDeviceToHost));
        for (size_t b = 0; b < D->src.size(); b++) memcpy(&F->val[16 * (size_t)D->src[b]], &v[16 * b], sizeof(double) * 16);
    }
    v.resize(16 * (size_t)nb);
    HIP_TRY(hipMemcpy(v.data(), F->dbwd.dinv, sizeof(double) * v.size(), hipMemcpyDeviceToHost));
    for (int q = 0; q < nb; q++) memcpy(&F->val[16 * (size_t)F->pat.diag[F->bwd.perm[q]]], &v[16 * (size_t)q], sizeof(double) * 16);
    return MI_OK;
}

extern "C" int mi_bilu4dev_info(mi_bilu4_t F, int* prepared, int* launches, long long* plan_bytes)
{
    CHECK_ARG(F, "null handle");
    if (prepared) *prepared = F->dev_prepared ? 1 : 0;
    if (launches) *launches = F->fwd.nlaunch() + kBiluDevFixedLaunches;
    if (plan_bytes) *plan_bytes = F->dev_plan_bytes;
    return MI_OK;
}

// ---------------------------------------------------------------- mi_bilu4one_*: both sweeps of the solve in one launch
extern "C" int mi_bilu4one_plan_probe(int nbrows, const int* ptrow, const int* indcol, int fill, int workgroups, int* eligible, int nchunks[2],
                                      int max_deps[2], long long* plan_bytes, int* const chunk_pos[2], int* const chunk_lev[2],
                                      int* const dep_ptr[2], int* const dep[2])
{
    int rc = bilu_check_args(nbrows, ptrow, indcol, fill);
    if (rc) return rc;
    CHECK_ARG(workgroups >= 0, "negative workgroups");
    Bilu4Pattern P;
    Bilu4Sweep S[2];
    Bilu4OnePlan O;
    bilu4_symbolic(nbrows, ptrow, indcol, fill, &P);
    bilu4_sweep(P, false, &S[0]);
    bilu4_sweep(P, true, &S[1]);
    bilu4one_plan(P, S[0], S[1], &O);
    for (int b = 0; b < 2; b++) {
        const std::string bad = bilu4one_check(P, S[b], b == 1, O.sweep[b], workgroups ? workgroups : kBiluOnePlanFor);
        if (!bad.empty()) return fail(MI_ERR_STATE, "mi_bilu4one_plan_probe: " + bad);
    }
    auto copy = [](const std::vector<int>& v, int* const out[2], int b) {
        if (out && out[b] && !v.empty()) memcpy(out[b], v.data(), sizeof(int) * v.size());
    };
    for (int b = 0; b < 2; b++) {
        const Bilu4OneSweep& W = O.sweep[b];
        if (nchunks) nchunks[b] = W.nchunks();
        if (max_deps) max_deps[b] = W.max_deps;
        copy(W.chunk_pos, chunk_pos, b), copy(W.chunk_lev, chunk_lev, b), copy(W.dep_ptr, dep_ptr, b), copy(W.dep, dep, b);
    }
    if (plan_bytes) *plan_bytes = O.bytes();
    if (eligible) *eligible = O.eligible() ? 1 : 0;
    if (!O.eligible()) g_err = "mi_bilu4one: not eligible: " + O.why_not();
    return MI_OK;
}

static int bilu_one_not_eligible(mi_bilu4_s* F, const std::string& why)
{
    bilu_one_release(F);
    F->one_state = -1;
    F->one_why = "mi_bilu4one: not eligible: " + why;
    return fail(MI_ERR_UNSUPPORTED, F->one_why);
}

extern "C" int mi_bilu4one_prepare(mi_bilu4_t F)
{
    CHECK_ARG(F, "null handle");
    if (F->pat.nb == 0) return MI_OK;
    if (F->device < 0) return fail(MI_ERR_STATE, std::string("mi_bilu4one_prepare") + kHostOnlyDev);
    if (F->one_state == 1) return MI_OK;
    if (F->one_state < 0) return fail(MI_ERR_UNSUPPORTED, F->one_why);
    Bilu4OnePlan O;
    bilu4one_plan(F->pat, F->fwd, F->bwd, &O);
    for (int b = 0; b < 2; b++) F->one_nchunks[b] = O.sweep[b].nchunks(), F->one_max_deps[b] = O.sweep[b].max_deps;
    if (!O.eligible()) return bilu_one_not_eligible(F, O.why_not());
    // every workgroup of the grid must be resident at once (a waiting workgroup keeps its slot)
    int per_cu[2] = {0, 0}, dev = 0, cus = 0;
    Bilu4OneArgs dummy{};
    HIP_TRY(bilu_one_launch_t<true>(F, dummy, nullptr, nullptr, nullptr, true, &per_cu[0]));
    HIP_TRY(bilu_one_launch_t<false>(F, dummy, nullptr, nullptr, nullptr, true, &per_cu[1]));
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const long long resident = (long long)std::min(per_cu[0], per_cu[1]) * cus;
    if (resident < 1) return bilu_one_not_eligible(F, "the occupancy query leaves no workgroup of the one-launch kernel resident");
    long long G = std::min<long long>(cus, std::max(F->one_nchunks[0], F->one_nchunks[1]));
    if (const char* e = getenv("MI355_BILU_ONE_WGS")) {
        CHECK_ARG(atoi(e) >= 1, "MI355_BILU_ONE_WGS must be >= 1");
        G = atoi(e);
    }
    G = std::max<long long>(1, std::min(G, resident));
    // (the plan is replayed for the grid it will run on: a stall here would be a hang there)
    for (int b = 0; b < 2; b++) {
        const std::string bad = bilu4one_check(F->pat, b ? F->bwd : F->fwd, b == 1, O.sweep[b], (int)G);
        if (!bad.empty()) return fail(MI_ERR_STATE, "mi_bilu4one_prepare: " + bad);
    }
    auto up = [&]() -> int {
        int rc;
        for (int b = 0; b < 2; b++) {
            Bilu4OneDev& D = F->one[b];
            const Bilu4OneSweep& W = O.sweep[b];
            if ((rc = bilu_dev_table(W.chunk_pos, &D.chunk_pos)) || (rc = bilu_dev_table(W.chunk_lev, &D.chunk_lev)) ||
                (rc = bilu_dev_table(W.dep_ptr, &D.dep_ptr)) || (rc = bilu_dev_table(W.dep, &D.dep)))
                return rc;
            D.nchunks = W.nchunks();
            const size_t bytes = sizeof(unsigned) * kBiluOneFlagStride * (size_t)std::max(D.nchunks, 1);
            HIP_TRY(hipMalloc(&D.flags, bytes));
            HIP_TRY(hipMemset(D.flags, 0, bytes));
        }
        HIP_TRY(hipMalloc(&F->d_one_counter, sizeof(unsigned) * kBiluOneFlagStride));
        HIP_TRY(hipMemset(F->d_one_counter, 0, sizeof(unsigned) * kBiluOneFlagStride));
        HIP_TRY(hipHostMalloc((void**)&F->h_one_giveups, sizeof(unsigned), hipHostMallocMapped));
        *F->h_one_giveups = 0;
        HIP_TRY(hipHostGetDevicePointer((void**)&F->d_one_giveups, F->h_one_giveups, 0));
        HIP_TRY(hipStreamSynchronize(nullptr)); // (the zeroed flags, before the first solve on the caller's stream reads them)
        return MI_OK;
    };
    if (int rc = up()) {
        bilu_one_release(F);
        return rc;
    }
    F->one_wgs = (int)G;
    F->one_epoch = 0;
    F->one_plan_bytes = O.bytes();
    F->one_state = 1;
    return MI_OK;
}

// a wait gave up: some workgroups left early, so flags and counter no longer add up — start again from zero
static int bilu_one_reset(mi_bilu4_s* F)
{
    HIP_TRY(hipDeviceSynchronize());
    for (int b = 0; b < 2; b++) HIP_TRY(hipMemset(F->one[b].flags, 0, sizeof(unsigned) * kBiluOneFlagStride * (size_t)std::max(F->one[b].nchunks, 1)));
    HIP_TRY(hipMemset(F->d_one_counter, 0, sizeof(unsigned) * kBiluOneFlagStride));
    HIP_TRY(hipDeviceSynchronize());
    F->one_epoch = 0;
    __atomic_store_n(F->h_one_giveups, 0u, __ATOMIC_RELEASE);
    return MI_OK;
}

extern "C" int mi_bilu4_set_solve_form(mi_bilu4_t F, int form)
{
    CHECK_ARG(F, "null handle");
    CHECK_ARG(form == MI_BILU_FORM_LEVELS || form == MI_BILU_FORM_ONE || form == MI_BILU_FORM_AUTO, "unknown solve form (0: one launch per level, 1: one launch, -1: measure and choose)");
    if (F->pat.nb == 0) return MI_OK;
    if (F->device < 0) return fail(MI_ERR_STATE, std::string("mi_bilu4_set_solve_form") + kHostOnlyDev);
    int rc;
    if (form == MI_BILU_FORM_LEVELS) {
        F->form = MI_BILU_FORM_LEVELS;
        if (bilu_one_gave_up(F) && (rc = bilu_one_reset(F))) return rc;
        return MI_OK;
    }
    if ((rc = mi_bilu4one_prepare(F))) {
        if (rc == MI_ERR_UNSUPPORTED) F->form = MI_BILU_FORM_LEVELS;
        return rc == MI_ERR_UNSUPPORTED && form == MI_BILU_FORM_AUTO ? MI_OK : rc;
    }
    if (bilu_one_gave_up(F)) return fail(MI_ERR_HIP, kOneGaveUp);
    if (form == MI_BILU_FORM_ONE) {
        F->form = MI_BILU_FORM_ONE;
        return MI_OK;
    }
    // auto: both forms give the same bits, so time each on the handle's own scratch vectors, two interleaved rounds, and keep the
    // one-launch form only if it measured below 0.98 of the other and no wait gave up (the rule of the one-launch powers step)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemset(F->d_b, 0, sizeof(double) * 4 * (size_t)F->pat.nb));
    LaunchTimer T(nullptr);
    if ((rc = T.init())) return rc;
    double us[2] = {0.0, 0.0};
    for (int round = 0; round < 2; round++)
        for (int f = 0; f < 2; f++) {
            double t = 0.0;
            if ((rc = T.time(2, 5, [&] { return f ? bilu_solve_one_launch(F, F->d_b, F->d_x, nullptr) : bilu_solve_launch(F, F->d_b, F->d_x, nullptr); }, &t))) return rc;
            us[f] = min_measured(us[f], t);
            if (f == 1 && bilu_one_gave_up(F)) round = 2; // every further launch would spin its whole budget again
        }
    F->us_form[0] = us[0], F->us_form[1] = us[1];
    const bool gave_up = bilu_one_gave_up(F);
    if (gave_up && (rc = bilu_one_reset(F))) return rc; // (measured on scratch vectors: nothing of the caller's is invalid)
    F->form = (!gave_up && us[1] > 0 && us[1] < 0.98 * us[0]) ? MI_BILU_FORM_ONE : MI_BILU_FORM_LEVELS;
    return MI_OK;
}

extern "C" int mi_bilu4one_status(mi_bilu4_t F)
{
    CHECK_ARG(F, "null handle");
    if (F->pat.nb == 0) return MI_OK;
    if (F->device < 0) return fail(MI_ERR_STATE, std::string("mi_bilu4one_status") + kHostOnlyDev);
    if (bilu_one_gave_up(F)) return fail(MI_ERR_HIP, kOneGaveUp);
    return MI_OK;
}

extern "C" int mi_bilu4one_info(mi_bilu4_t F, int* prepared, int* eligible, int* workgroups, int nchunks[2], int max_deps[2], long long* plan_bytes)
{
    CHECK_ARG(F, "null handle");
    if (prepared) *prepared = F->one_state == 1;
    if (eligible) *eligible = F->one_state == 1;
    if (workgroups) *workgroups = F->one_state == 1 ? F->one_wgs : 0;
    for (int b = 0; b < 2; b++) {
        if (nchunks) nchunks[b] = F->one_nchunks[b];
        if (max_deps) max_deps[b] = F->one_max_deps[b];
    }
    if (plan_bytes) *plan_bytes = F->one_state == 1 ? F->one_plan_bytes : 0;
    return MI_OK;
}
