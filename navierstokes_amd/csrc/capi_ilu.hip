// capi_ilu.hip: the 4x4-block ILU(k) preconditioner, mi_bilu4_* — part of libmi355spmv.so (see capi_internal.hpp for the layout of
// the library).  Factored on the host (bilu4_plan.hpp) or, into the same device copies, on the GPU level by level (mi_bilu4dev_*,
// bilu4_factor.hpp).  Applied on the GPU in one of four ways, a Bilu4Apply each, through ONE path (bilu_apply, at the end of the
// file): exactly — one launch per (folded) dependency level (bilu4_solve.hpp) or, where the handle was told so
// (mi_bilu4_set_solve_form), one launch of persistent workgroups (bilu4_solve_one.hpp, mi_bilu4one_*) — or by a fixed number of
// Jacobi sweeps per triangle, one launch per sweep (mi_bilu4sw_*, bilu4_sweep.hpp); either over the factor's doubles or over an
// opt-in single-precision copy of its values (mi_bilu4sp_* the sweeps, mi_bilu4spx_* the exact solve), which every entry point
// that writes the factor keeps current.  mi_bilu4_create_ordered puts a multicolour ordering behind the handle (bilu4_order.hpp):
// the factor is then that of the permuted matrix, every solve is bracketed by a gather and a scatter (bilu_in_order, the one
// place), and wide unfolded levels take bilu4_level_wide (bilu4_solve_wide.hpp).
// What the handle has in common with a block DILU handle (capi_dilu.hip) is capi_bilu_common.hpp's: the argument rules, the host
// part of the handle (ordering, pattern, schedule), the level-major device copy and how values move into it, the guard, the steps
// of a refactor, and bilu_in_order.
// No CPU fallback: the solve and the device refactor need a HIP device; the planning and host factorisation entry points need none.
#include "capi_bilu_common.hpp"
#include "bilu4_solve.hpp"
#include "bilu4_solve_one.hpp"
#include "bilu4_factor.hpp"
#include "bilu4_sweep.hpp"
#include "bilu4_solve_wide.hpp"

// (ownership: DevArray and the floor of one entry, capi_bilu_common.hpp; the give-up word is a MappedWord)

static Bilu4SweepView bilu_view(const Bilu4DevSweep& D) { return Bilu4SweepView{D.perm, D.ptr, D.col, D.val, D.dinv, D.lev_ptr}; }

// the device refactor (mi_bilu4dev_prepare): pattern-only tables, see Bilu4DevPlan
struct Bilu4DevTables {
    bool prepared = false;
    long long nL = 0, nU = 0, plan_bytes = 0;
    DevArray<int> fpos, bpos, gather, upd;
    DevArray<long long> upd_ptr;
    DevArray<int> bad;
};

// the one-launch solve (mi_bilu4one_prepare): chunks, dependency lists, flags, see Bilu4OnePlan
struct Bilu4OneTables {
    struct Sweep {
        DevArray<int> chunk_pos, chunk_lev, dep_ptr, dep;
        DevArray<unsigned> flags;
        int nchunks = 0;
        size_t nflags() const { return kBiluOneFlagStride * (size_t)std::max(nchunks, 1); }
        Bilu4OneTab tab() const { return Bilu4OneTab{chunk_pos, chunk_lev, dep_ptr, dep, flags, nchunks}; }
    };
    int state = 0; // 0: not prepared; 1: prepared; -1: not eligible (why)
    std::string why;
    int wgs = 0, nchunks[2] = {0, 0}, max_deps[2] = {0, 0};
    long long plan_bytes = 0;
    Sweep sweep[2];
    DevArray<unsigned> counter;
    MappedWord giveups;
    unsigned epoch = 0;
};

// the sweep solve (mi_bilu4sw_prepare): its three work vectors — the forward iterates alternate between w[0] and w[1], the one
// that does not end up holding t and w[2] carry the backward iterates
struct Bilu4SweepWork {
    bool prepared = false;
    int launches_last = 0;
    DevArray<double> w[3];
};

// the single-precision copy of the level-major values (mi_bilu4sp_prepare): L blocks, U blocks, inverted diagonal blocks, in the
// order of lev[0].val, lev[1].val and lev[1].dinv; rec: what the last conversion found (Bilu4SpRecord).  The sweeps (mi_bilu4sp_*)
// and the exact solve (mi_bilu4spx_*) both stream it; exact_*: launches of the last exact solve over it, and those that were wide
struct Bilu4SpCopy {
    bool prepared = false;
    int convert_launches = 0, launches_last = 0;
    int exact_launches_last = 0, exact_wide_last = 0;
    DevArray<float> val[2], dinv;
    DevArray<Bilu4SpRecord> rec;
};

// what an ordered handle (mi_bilu4_create_ordered) owns on the device besides the numbering (d_perm): the two vectors in it that every
// solve passes through — allocated at create, so that a solve allocates nothing and stays capturable; hence one solve at a time per handle
struct Bilu4OrderDev {
    DevArray<double> b, x; // [4 nb] right-hand side and solution in the factor's numbering
    int wide_min = 0;      // block rows from which an unfolded level takes bilu4_level_wide; 0: never (natural order)
};

struct mi_bilu4_s : Bilu4Handle { // a_ptr, a_col: the pattern that is factored (refactor scatters new values through it)
    int fill = 0;
    std::vector<double> val;       // host factor, row order, row-major blocks
    double us_form[2] = {0.0, 0.0}; // [0] one launch per level, measured at create; [1] one launch, once mi_bilu4_set_solve_form(F, -1) has measured it
    int form = MI_BILU_FORM_LEVELS;
    DevArray<double> d_b, d_x;     // scratch of the host-pointer solve
    Bilu4DevTables dev;
    Bilu4OneTables one;
    Bilu4SweepWork sw;
    Bilu4SpCopy sp;
    Bilu4OrderDev ordd;
    ~mi_bilu4_s() { d_perm = {}, ordd = {}, sp = {}, sw = {}, one = {}, lev[0] = {}, lev[1] = {}, d_b = {}, d_x = {}, dev = {}; } // the order the handle has always been freed in (newest first)
    Bilu4FactorView factor_view() const
    {
        return Bilu4FactorView{lev[0].perm, lev[0].ptr, lev[0].col, lev[1].ptr, lev[0].lev_ptr, dev.fpos, dev.bpos, dev.upd_ptr, dev.upd,
                               lev[0].val, lev[1].val, lev[1].dinv, (int)dev.nL, (int)dev.nU, dev.bad};
    }
};

// what a host-only handle gets: MI_ERR_STATE, but MI_ERR_NODEVICE from everything about sweeps and the single-precision copy
constexpr BiluHostOnly kHostOnlyDev{MI_ERR_STATE, ": a host-only handle (mi_bilu4_create_host) has no device factor"};
constexpr BiluHostOnly kHostOnlySweep{MI_ERR_NODEVICE, ": a host-only handle (mi_bilu4_create_host) has no device factor, and the sweep solve has no CPU fallback"};

static int bilu_zero_pivot(int row)
{
    return fail(MI_ERR_ARG, "mi_bilu4: zero pivot (|d| < 1e-12) in the diagonal block of block row " + std::to_string(row));
}

static int bilu_factor(mi_bilu4_s* F, const double* coef, int layout)
{
    const auto t0 = std::chrono::steady_clock::now();
    const int bad = bilu4_factor(F->pat(), F->sched.sweep[0], F->a_ptr.data(), F->a_col.data(), coef, layout == MI_BLOCK_COLMAJOR, bilu_threads(), F->val.data(),
                                 F->ord.src_or_null());
    F->factor_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return bad >= 0 ? bilu_zero_pivot(F->ord.caller_row(bad)) : MI_OK;
}

// THE ONE LISTING of the factor's three level-major value arrays — the L blocks, the U blocks, the inverted diagonal blocks by
// backward position: fn(doubles, floats, blocks, host_block) for each in that order, where floats is the array's place in the
// single-precision copy S (the handle's, or one still being built) and host_block(k) the place of its block k in the host factor
template <class Fn>
static int bilu_each_values(const mi_bilu4_s* F, Bilu4SpCopy& S, Fn&& fn)
{
    for (int b = 0; b < 2; b++) {
        const Bilu4DevSweep& D = F->lev[b];
        if (const int rc = fn((double*)D.val, S.val[b], D.src.size(), [&](size_t k) { return D.src[k]; })) return rc;
    }
    return fn((double*)F->lev[1].dinv, S.dinv, (size_t)F->pat().nb, [&](size_t q) { return F->pat().diag[F->sched.sweep[1].perm[q]]; });
}

// the values between the host factor and the level-major device copies, to the device (create, mi_bilu4_refactor) or back
// (mi_bilu4dev_fetch)
static int bilu_move_values(mi_bilu4_s* F, bool to_device)
{
    std::vector<double> v;
    return bilu_each_values(F, F->sp, [&](double* dev, DevArray<float>&, size_t n, auto&& host_block) { return bilu_move_blocks(dev, n, F->val.data(), host_block, to_device, v); });
}

// does launch L take the wide-level kernel?  wide_min: the handle's (0 on a natural-order handle: never)
static bool bilu_wide(const Bilu4Launch& L, int wide_min) { return wide_min > 0 && !L.folded() && L.p1 - L.p0 >= wide_min; }

// D: the sweep's level-major copy; A: its values in the type they are streamed in — D's own doubles, or the single-precision copy
// (mi_bilu4spx_*), which take D's places in the view the kernels are handed
template <bool BWD, bool AL, class T>
static void bilu_sweep_launch(const Bilu4Sweep& S, const Bilu4SweepView& D, const Bilu4SweepVals<T>& A, const double* src, double* x, int wide_min, hipStream_t s)
{
    const Bilu4SweepViewT<T> V{D.perm, D.ptr, D.col, A.val, A.dinv, D.lev_ptr};
    constexpr int P = std::is_same<T, float>::value ? kBiluWideDepthF32 : kBiluSweepDepth;
    for (int a = 0; a < S.nlaunch(); a++) {
        const Bilu4Launch L = S.launch(a);
        if (L.folded()) {
            hipLaunchKernelGGL((bilu4_folded<BWD, AL, T>), dim3(1), dim3(kWG), 0, s, V, L.l0, L.l1, src, x);
            continue;
        }
        const int grid = (L.p1 - L.p0 + kBiluRowsPerWG - 1) / kBiluRowsPerWG;
        if constexpr (AL) { // (the wide kernel runs on an ordered handle's own vectors only: always aligned)
            if (bilu_wide(L, wide_min)) {
                hipLaunchKernelGGL((bilu4_level_wide<BWD, P, T>), dim3(grid), dim3(kWG), 0, s, V, L.p0, L.p1, src, x);
                continue;
            }
        }
        hipLaunchKernelGGL((bilu4_level<BWD, AL, T>), dim3(grid), dim3(kWG), 0, s, V, L.p0, L.p1, src, x);
    }
}

// launches of one exact solve in form 0 that take the wide-level kernel
static int bilu_wide_launches(const mi_bilu4_s* F)
{
    int n = 0;
    for (const Bilu4Sweep& S : F->sched.sweep)
        for (int a = 0; a < S.nlaunch(); a++) n += bilu_wide(S.launch(a), F->ordd.wide_min);
    return n;
}

// form A: one launch per (folded) level, forward then backward, on the caller's stream; nothing allocated or synchronised
// Lv, Uv: the values of the two triangles in the type they are streamed in (the factor's own, or its single-precision copy)
template <class T>
static int bilu_solve_launch(mi_bilu4_s* F, const Bilu4SweepVals<T>& Lv, const Bilu4SweepVals<T>& Uv, const double* d_b, double* d_x, hipStream_t s)
{
    bilu_by_alignment(d_x, [&](auto al) {
        bilu_sweep_launch<false, decltype(al)::value>(F->sched.sweep[0], bilu_view(F->lev[0]), Lv, d_b, d_x, F->ordd.wide_min, s);
        bilu_sweep_launch<true, decltype(al)::value>(F->sched.sweep[1], bilu_view(F->lev[1]), Uv, d_x, d_x, F->ordd.wide_min, s);
    });
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

static int bilu_solve_launch(mi_bilu4_s* F, const double* d_b, double* d_x, hipStream_t s)
{
    return bilu_solve_launch<double>(F, {F->lev[0].val, nullptr}, {F->lev[1].val, F->lev[1].dinv}, d_b, d_x, s);
}

static const char* const kOneGaveUp =
    "mi_bilu4: a hand-off wait of the one-launch solve gave up (workgroups of the grid were not all resident: another kernel held CUs); "
    "results since then are invalid — call mi_bilu4_set_solve_form(F, 0) to clear this and solve level by level";

static bool bilu_one_gave_up(const mi_bilu4_s* F) { return F->one.giveups.host && __atomic_load_n(F->one.giveups.host.get(), __ATOMIC_ACQUIRE) != 0; }

template <bool AL>
static hipError_t bilu_one_launch_t(const mi_bilu4_s* F, const Bilu4OneArgs& A, const double* d_b, double* d_x, hipStream_t s, bool query, int* max_blocks)
{
    auto kern = bilu4_solve_one<AL>;
    if (query) return hipOccupancyMaxActiveBlocksPerMultiprocessor(max_blocks, kern, kWG, 0);
    hipLaunchKernelGGL(kern, dim3(F->one.wgs), dim3(kWG), 0, s, bilu_view(F->lev[0]), bilu_view(F->lev[1]), A, d_b, d_x);
    return hipGetLastError();
}

// form 1: both sweeps in one launch of F->one.wgs persistent workgroups.  ONE solve at a time per handle: the epoch is per handle.
static int bilu_solve_one_launch(mi_bilu4_s* F, const double* d_b, double* d_x, hipStream_t s)
{
    Bilu4OneArgs A{};
    A.fwd = F->one.sweep[0].tab();
    A.bwd = F->one.sweep[1].tab();
    A.epoch = ++F->one.epoch; // flags are never cleared: this solve's are the ones that carry its epoch
    A.counter = F->one.counter;
    A.giveups = F->one.giveups.dev;
    static const unsigned spin_max = 1u << (getenv("MI355_BILU_ONE_SPIN_LOG2") ? std::max(8, std::min(30, atoi(getenv("MI355_BILU_ONE_SPIN_LOG2")))) : 21);
    A.spin_max = spin_max;
    const hipError_t e = bilu_by_alignment(d_x, [&](auto al) { return bilu_one_launch_t<decltype(al)::value>(F, A, d_b, d_x, s, false, nullptr); });
    if (e != hipSuccess) return fail(MI_ERR_HIP, std::string("one-launch ILU solve: ") + hipGetErrorString(e));
    return MI_OK;
}

// The single-precision copy written from the level-major factor as it lies on the device now, on stream s: two launches (the record
// of mi_bilu4sp_status cleared, then the values), nothing allocated or synchronised.  S: the copy to write — the handle's, or the
// one mi_bilu4sp_prepare is still building.
static int bilu_sp_convert(const mi_bilu4_s* F, Bilu4SpCopy& S, hipStream_t s)
{
    Bilu4SpConvert C{};
    long long end = 0;
    int a = 0;
    bilu_each_values(F, S, [&](const double* src, DevArray<float>& dst, size_t blocks, auto&&) {
        C.src[a] = src, C.dst[a] = dst, C.end[a] = (end += 4 * (long long)blocks);
        a++;
        return MI_OK;
    });
    for (int b = 0; b < 2; b++) C.ptr[b] = F->lev[b].ptr, C.perm[b] = F->lev[b].perm;
    C.nb = F->pat().nb;
    C.rec = S.rec;
    hipLaunchKernelGGL(bilu4sp_reset, dim3(1), dim3(1), 0, s, C.rec);
    hipLaunchKernelGGL(bilu4sp_convert, dim3((unsigned)((end + kWG - 1) / kWG)), dim3(kWG), 0, s, C);
    HIP_TRY(hipGetLastError());
    S.convert_launches++;
    return MI_OK;
}

static int bilu_create(int nbrows, const int* ptrow, const int* indcol, const double* coef, int layout, int fill, int ordering, bool device, mi_bilu4_t* out)
{
    int rc;
    if ((rc = bilu_check_create("mi_bilu4: ", nbrows, ptrow, indcol, coef, layout, fill, ordering, out))) return rc;
    if (const char* e = getenv("MI355_BILU_FORM")) {
        CHECK_ARG(!strcmp(e, "0") || !strcmp(e, "1"), "MI355_BILU_FORM must be 0 or 1");
        if (!strcmp(e, "1"))
            return fail(MI_ERR_UNSUPPORTED, "MI355_BILU_FORM=1: the one-launch form of the solve is not built at create: it is chosen per handle, with mi_bilu4_set_solve_form (every handle starts in form 0: one launch per level)");
    }
    if (device && (rc = need_device())) return rc;
    std::unique_ptr<mi_bilu4_s> F(new (std::nothrow) mi_bilu4_s);
    if (!F) return fail(MI_ERR_ALLOC, "host allocation failed");
    F->fill = fill;
    if ((rc = bilu_plan_host(F.get(), nbrows, ptrow, indcol, fill, ordering, "mi_bilu4_create_ordered"))) return rc;
    if (nbrows > 0 && F->ord.on()) {
        F->ordd.wide_min = kBiluWideMin;
        if (const char* e = getenv("MI355_BILU_WIDE_MIN")) {
            CHECK_ARG(atoi(e) >= 1, "MI355_BILU_WIDE_MIN must be >= 1 (block rows)");
            F->ordd.wide_min = atoi(e);
        }
    }
    F->val.assign(16 * (size_t)F->pat().nblocks(), 0.0);
    if ((rc = bilu_factor(F.get(), coef, layout))) return rc;
    if (device && nbrows > 0) {
        HIP_TRY(hipGetDevice(&F->device));
        if ((rc = bilu_upload_pattern(F.get())) || (rc = dev_alloc(F->lev[1].dinv, 16 * (size_t)nbrows, 1)) || (rc = bilu_move_values(F.get(), true)) ||
            (rc = dev_alloc(F->d_b, 4 * (size_t)nbrows, 1)) || (rc = dev_alloc(F->d_x, 4 * (size_t)nbrows, 1)))
            return rc;
        if (F->ord.on() && ((rc = dev_upload(F->d_perm, F->ord.perm, 1)) || (rc = dev_alloc(F->ordd.b, 4 * (size_t)nbrows, 1)) || (rc = dev_alloc(F->ordd.x, 4 * (size_t)nbrows, 1))))
            return rc;
        HIP_TRY(hipMemset(F->d_b, 0, sizeof(double) * 4 * nbrows));
        // the solve's time, through the library's one timing helper (zero right-hand side: the time does not depend on values)
        LaunchTimer T(nullptr);
        if ((rc = T.init())) return rc;
        if ((rc = T.time(2, 5, [&] { return bilu_solve_launch(F.get(), F->d_b, F->d_x, nullptr); }, &F->us_form[0]))) return rc;
    } else if (device) {
        F->device = 0; // an empty matrix: every call on it is a no-op
    }
    *out = F.release();
    return MI_OK;
}

extern "C" int mi_bilu4_create(int nbrows, const int* ptrow, const int* indcol, const double* coef, int layout, int fill, mi_bilu4_t* out)
{
    return bilu_create(nbrows, ptrow, indcol, coef, layout, fill, MI_BILU_ORDER_NATURAL, true, out);
}

extern "C" int mi_bilu4_create_host(int nbrows, const int* ptrow, const int* indcol, const double* coef, int layout, int fill, mi_bilu4_t* out)
{
    return bilu_create(nbrows, ptrow, indcol, coef, layout, fill, MI_BILU_ORDER_NATURAL, false, out);
}

extern "C" int mi_bilu4_create_ordered(int nbrows, const int* ptrow, const int* indcol, const double* coef, int layout, int fill, int ordering, mi_bilu4_t* out)
{
    return bilu_create(nbrows, ptrow, indcol, coef, layout, fill, ordering, true, out);
}

extern "C" int mi_bilu4_create_host_ordered(int nbrows, const int* ptrow, const int* indcol, const double* coef, int layout, int fill, int ordering, mi_bilu4_t* out)
{
    return bilu_create(nbrows, ptrow, indcol, coef, layout, fill, ordering, false, out);
}

extern "C" int mi_bilu4_order_info(mi_bilu4_t F, int* ordering, int* ncolours, int* wide_launches, int* perm)
{
    CHECK_ARG(F, "null handle");
    if (ordering) *ordering = F->ord.ordering;
    if (ncolours) *ncolours = F->ord.ncolours;
    if (wide_launches) *wide_launches = bilu_wide_launches(F);
    for (int i = 0; perm && i < F->pat().nb; i++) perm[i] = F->ord.on() ? F->ord.perm[i] : i;
    return MI_OK;
}

extern "C" int mi_bilu4_order_probe(int nbrows, const int* ptrow, const int* indcol, int ordering, int* perm, int* ncolours, int* colour_sizes, int cap)
{
    CHECK_ARG(!bilu_bad_ordering(ordering), bilu_bad_ordering(ordering));
    int rc = bilu_check_args("mi_bilu4: ", nbrows, ptrow, indcol, 0);
    if (rc) return rc;
    Bilu4Order O;
    if ((rc = bilu_order(nbrows, ptrow, indcol, ordering, "mi_bilu4_order_probe", &O))) return rc;
    if (ncolours) *ncolours = O.ncolours;
    CHECK_ARG(!colour_sizes || cap >= O.ncolours, "colour-size array too short");
    for (int i = 0; perm && i < nbrows; i++) perm[i] = O.on() ? O.perm[i] : i;
    for (int c = 0; colour_sizes && c < O.ncolours; c++) colour_sizes[c] = O.colour_ptr[c + 1] - O.colour_ptr[c];
    return MI_OK;
}

extern "C" int mi_bilu4_destroy(mi_bilu4_t F)
{
    delete F;
    return MI_OK;
}

extern "C" int mi_bilu4_refactor(mi_bilu4_t F, const double* coef, int layout)
{
    return bilu_refactor(F, coef, layout, [&] { return bilu_factor(F, coef, layout); }, [&]() -> int {
        int rc;
        if ((rc = bilu_move_values(F, true)) || !F->sp.prepared) return rc;
        // the single-precision copy follows the factor before the call returns
        if ((rc = bilu_sp_convert(F, F->sp, nullptr))) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        return MI_OK;
    });
}

extern "C" int mi_bilu4_info(mi_bilu4_t F, int* nbrows, long long* nblocks, int* fwd_levels, int* bwd_levels, int* launches, int* form,
                             double us[2], double* factor_seconds, long long* factor_bytes)
{
    CHECK_ARG(F, "null handle");
    const Bilu4Sweep* S = F->sched.sweep;
    if (nbrows) *nbrows = F->pat().nb;
    if (nblocks) *nblocks = F->pat().nblocks();
    if (fwd_levels) *fwd_levels = S[0].nlev();
    if (bwd_levels) *bwd_levels = S[1].nlev();
    if (launches) *launches = (F->form == MI_BILU_FORM_ONE ? 1 : S[0].nlaunch() + S[1].nlaunch()) + (F->ord.on() ? kBiluOrderLaunches : 0);
    if (form) *form = F->form;
    if (us) us[0] = F->us_form[0], us[1] = F->us_form[1];
    if (factor_seconds) *factor_seconds = F->factor_seconds;
    if (factor_bytes) *factor_bytes = F->pat().nblocks() * (long long)(16 * sizeof(double) + sizeof(int)) + (long long)F->pat().nb * 4 * (long long)sizeof(int);
    return MI_OK;
}

extern "C" int mi_bilu4_factor_host(mi_bilu4_t F, int* ptr, int* col, int* diag, double* val, long long cap_blocks)
{
    CHECK_ARG(F, "null handle");
    const Bilu4Pattern& P = F->pat();
    const long long nblk = P.nblocks();
    CHECK_ARG(cap_blocks >= nblk || (!col && !val), "arrays too short: need mi_bilu4_info's nblocks entries");
    const int nb = P.nb;
    if (ptr && nb) memcpy(ptr, P.ptr.data(), sizeof(int) * (nb + 1));
    if (ptr && !nb) ptr[0] = 0;
    if (col && nblk) memcpy(col, P.col.data(), sizeof(int) * nblk);
    if (diag && nb) memcpy(diag, P.diag.data(), sizeof(int) * nb);
    if (val && nblk) memcpy(val, F->val.data(), sizeof(double) * 16 * nblk);
    return MI_OK;
}

extern "C" int mi_bilu4_plan_probe(int nbrows, const int* ptrow, const int* indcol, int fill, long long* nblocks, int* fwd_levels,
                                   int* bwd_levels, int* fwd_launches, int* bwd_launches, int* fwd_sizes, int* bwd_sizes, int cap_levels)
{
    int rc = bilu_check_args("mi_bilu4: ", nbrows, ptrow, indcol, fill);
    if (rc) return rc;
    Bilu4Schedule S;
    bilu4_schedule(nbrows, ptrow, indcol, fill, &S);
    int* const levels[2] = {fwd_levels, bwd_levels};
    int* const launches[2] = {fwd_launches, bwd_launches};
    int* const sizes[2] = {fwd_sizes, bwd_sizes};
    if (nblocks) *nblocks = S.pat.nblocks();
    for (int b = 0; b < 2; b++) {
        if (levels[b]) *levels[b] = S.sweep[b].nlev();
        if (launches[b]) *launches[b] = S.sweep[b].nlaunch();
    }
    CHECK_ARG((!fwd_sizes || cap_levels >= S.sweep[0].nlev()) && (!bwd_sizes || cap_levels >= S.sweep[1].nlev()), "level-size arrays too short");
    for (int b = 0; b < 2; b++)
        for (int l = 0; sizes[b] && l < S.sweep[b].nlev(); l++) sizes[b][l] = S.sweep[b].lev_ptr[l + 1] - S.sweep[b].lev_ptr[l];
    return MI_OK;
}

// ---------------------------------------------------------------- mi_bilu4dev_*: the numeric factorisation on the GPU
extern "C" int mi_bilu4dev_plan_probe(int nbrows, const int* ptrow, const int* indcol, int fill, long long* update_pairs, int* launches,
                                      long long* plan_bytes)
{
    int rc = bilu_check_args("mi_bilu4: ", nbrows, ptrow, indcol, fill);
    if (rc) return rc;
    Bilu4Schedule S;
    Bilu4DevPlan D;
    bilu4_schedule(nbrows, ptrow, indcol, fill, &S);
    bilu4dev_plan(S, ptrow, indcol, &D);
    if (update_pairs) *update_pairs = D.update_pairs;
    if (launches) *launches = S.sweep[0].nlaunch() + kBiluDevFixedLaunches;
    if (plan_bytes) *plan_bytes = D.bytes();
    return MI_OK;
}

extern "C" int mi_bilu4dev_prepare(mi_bilu4_t F)
{
    if (const int rc = bilu_guard(F, "mi_bilu4dev_prepare", kHostOnlyDev); rc != kBiluGo) return rc;
    if (F->dev.prepared) return MI_OK;
    Bilu4DevPlan D;
    bilu4dev_plan(F->sched, F->a_ptr.data(), F->a_col.data(), &D, F->ord.src_or_null());
    Bilu4DevTables T; // moves into the handle once it is complete; a failure on the way frees what there is
    int rc;
    if ((rc = dev_upload(T.fpos, D.fpos, 1)) || (rc = dev_upload(T.bpos, D.bpos, 1)) || (rc = dev_upload(T.gather, D.gather, 1)) || (rc = dev_upload(T.upd, D.upd, 1)) ||
        (rc = dev_upload(T.upd_ptr, D.upd_ptr, 1)) || (rc = dev_upload(T.bad, std::vector<int>(1, kBiluBadNone), 1)))
        return rc;
    T.nL = D.nL, T.nU = D.nU, T.plan_bytes = D.bytes();
    T.prepared = true;
    F->dev = std::move(T);
    return MI_OK;
}

extern "C" int mi_bilu4dev_refactor(mi_bilu4_t F, const double* d_coef, int layout, mi_stream_t s)
{
    if (const int rc = bilu_guard(F, "mi_bilu4dev_refactor", kHostOnlyDev, bilu_bad_layout(layout), d_coef ? nullptr : "null coef"); rc != kBiluGo) return rc;
    int rc;
    if (!F->dev.prepared && (rc = mi_bilu4dev_prepare(F))) return rc;
    hipStream_t st = (hipStream_t)s;
    const Bilu4FactorView V = F->factor_view();
    const long long total = F->pat().nblocks();
    hipLaunchKernelGGL(bilu4f_gather, dim3((unsigned)((total * 16 + kWG - 1) / kWG)), dim3(kWG), 0, st, V, F->dev.gather, total, d_coef,
                       (int)(layout == MI_BLOCK_COLMAJOR));
    const Bilu4Sweep& S = F->sched.sweep[0]; // the factor follows the forward sweep's launches
    for (int a = 0; a < S.nlaunch(); a++) {
        const Bilu4Launch L = S.launch(a);
        if (L.folded()) {
            hipLaunchKernelGGL(bilu4f_folded, dim3(1), dim3(kBiluFactorFoldedWG), 0, st, V, L.l0, L.l1);
        } else {
            const int grid = (int)(((long long)(L.p1 - L.p0) * 16 + kWG - 1) / kWG);
            hipLaunchKernelGGL(bilu4f_level, dim3(grid), dim3(kWG), 0, st, V, L.p0, L.p1);
        }
    }
    HIP_TRY(hipGetLastError());
    return F->sp.prepared ? bilu_sp_convert(F, F->sp, st) : MI_OK; // behind the factorisation, on the same stream (and in the same graph)
}

extern "C" int mi_bilu4dev_status(mi_bilu4_t F, int* bad_row)
{
    if (F && bad_row) *bad_row = -1;
    if (const int rc = bilu_guard(F, "mi_bilu4dev_status", kHostOnlyDev); rc != kBiluGo) return rc;
    if (!F->dev.prepared) return MI_OK; // no device refactor yet
    HIP_TRY(hipDeviceSynchronize());
    int bad = kBiluBadNone;
    HIP_TRY(hipMemcpy(&bad, F->dev.bad, sizeof(int), hipMemcpyDeviceToHost));
    if (bad == kBiluBadNone) return MI_OK;
    bad = F->ord.caller_row(bad);
    if (bad_row) *bad_row = bad;
    return bilu_zero_pivot(bad);
}

extern "C" int mi_bilu4dev_fetch(mi_bilu4_t F)
{
    if (const int rc = bilu_guard(F, "mi_bilu4dev_fetch", kHostOnlyDev); rc != kBiluGo) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return bilu_move_values(F, false);
}

extern "C" int mi_bilu4dev_info(mi_bilu4_t F, int* prepared, int* launches, long long* plan_bytes)
{
    CHECK_ARG(F, "null handle");
    if (prepared) *prepared = F->dev.prepared ? 1 : 0;
    if (launches) *launches = F->sched.sweep[0].nlaunch() + kBiluDevFixedLaunches;
    if (plan_bytes) *plan_bytes = F->dev.plan_bytes;
    return MI_OK;
}

// ---------------------------------------------------------------- mi_bilu4one_*: both sweeps of the solve in one launch
// the plan replayed for G workgroups, both sweeps; who: the entry point, for the message
static int bilu_one_replay(const Bilu4Schedule& S, const Bilu4OnePlan& O, int G, const char* who)
{
    for (int b = 0; b < 2; b++) {
        const std::string bad = bilu4one_check(S, b, O.sweep[b], G);
        if (!bad.empty()) return fail(MI_ERR_STATE, std::string(who) + ": " + bad);
    }
    return MI_OK;
}

extern "C" int mi_bilu4one_plan_probe(int nbrows, const int* ptrow, const int* indcol, int fill, int workgroups, int* eligible, int nchunks[2],
                                      int max_deps[2], long long* plan_bytes, int* const chunk_pos[2], int* const chunk_lev[2],
                                      int* const dep_ptr[2], int* const dep[2])
{
    int rc = bilu_check_args("mi_bilu4: ", nbrows, ptrow, indcol, fill);
    if (rc) return rc;
    CHECK_ARG(workgroups >= 0, "negative workgroups");
    Bilu4Schedule S;
    Bilu4OnePlan O;
    bilu4_schedule(nbrows, ptrow, indcol, fill, &S);
    bilu4one_plan(S, &O);
    if ((rc = bilu_one_replay(S, O, workgroups ? workgroups : kBiluOnePlanFor, "mi_bilu4one_plan_probe"))) return rc;
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

extern "C" int mi_bilu4one_prepare(mi_bilu4_t F)
{
    if (const int rc = bilu_guard(F, "mi_bilu4one_prepare", kHostOnlyDev); rc != kBiluGo) return rc;
    if (F->one.state == 1) return MI_OK;
    if (F->one.state < 0) return fail(MI_ERR_UNSUPPORTED, F->one.why);
    Bilu4OnePlan O;
    bilu4one_plan(F->sched, &O);
    Bilu4OneTables T; // moves into the handle when it is complete or refused for good; any other failure on the way frees what there is
    for (int b = 0; b < 2; b++) T.nchunks[b] = O.sweep[b].nchunks(), T.max_deps[b] = O.sweep[b].max_deps;
    auto not_eligible = [&](const std::string& why) {
        T.state = -1;
        T.why = "mi_bilu4one: not eligible: " + why;
        F->one = std::move(T);
        return fail(MI_ERR_UNSUPPORTED, F->one.why);
    };
    if (!O.eligible()) return not_eligible(O.why_not());
    // every workgroup of the grid must be resident at once (a waiting workgroup keeps its slot)
    int per_cu[2] = {0, 0}, dev = 0, cus = 0;
    Bilu4OneArgs dummy{};
    HIP_TRY(bilu_one_launch_t<true>(F, dummy, nullptr, nullptr, nullptr, true, &per_cu[0]));
    HIP_TRY(bilu_one_launch_t<false>(F, dummy, nullptr, nullptr, nullptr, true, &per_cu[1]));
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const long long resident = (long long)std::min(per_cu[0], per_cu[1]) * cus;
    if (resident < 1) return not_eligible("the occupancy query leaves no workgroup of the one-launch kernel resident");
    long long G = std::min<long long>(cus, std::max(T.nchunks[0], T.nchunks[1]));
    if (const char* e = getenv("MI355_BILU_ONE_WGS")) {
        CHECK_ARG(atoi(e) >= 1, "MI355_BILU_ONE_WGS must be >= 1");
        G = atoi(e);
    }
    G = std::max<long long>(1, std::min(G, resident));
    // (the plan is replayed for the grid it will run on: a stall here would be a hang there)
    int rc;
    if ((rc = bilu_one_replay(F->sched, O, (int)G, "mi_bilu4one_prepare"))) return rc;
    for (int b = 0; b < 2; b++) {
        Bilu4OneTables::Sweep& D = T.sweep[b];
        const Bilu4OneSweep& W = O.sweep[b];
        D.nchunks = W.nchunks();
        if ((rc = dev_upload(D.chunk_pos, W.chunk_pos, 1)) || (rc = dev_upload(D.chunk_lev, W.chunk_lev, 1)) || (rc = dev_upload(D.dep_ptr, W.dep_ptr, 1)) ||
            (rc = dev_upload(D.dep, W.dep, 1)) || (rc = dev_zeros(D.flags, D.nflags())))
            return rc;
    }
    if ((rc = dev_zeros(T.counter, kBiluOneFlagStride)) || (rc = dev_alloc(T.giveups))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr)); // (the zeroed flags, before the first solve on the caller's stream reads them)
    T.wgs = (int)G;
    T.plan_bytes = O.bytes();
    T.state = 1;
    F->one = std::move(T);
    return MI_OK;
}

// a wait gave up: some workgroups left early, so flags and counter no longer add up — start again from zero
static int bilu_one_reset(mi_bilu4_s* F)
{
    HIP_TRY(hipDeviceSynchronize());
    for (const Bilu4OneTables::Sweep& D : F->one.sweep) HIP_TRY(hipMemset(D.flags, 0, sizeof(unsigned) * D.nflags()));
    HIP_TRY(hipMemset(F->one.counter, 0, sizeof(unsigned) * kBiluOneFlagStride));
    HIP_TRY(hipDeviceSynchronize());
    F->one.epoch = 0;
    __atomic_store_n(F->one.giveups.host.get(), 0u, __ATOMIC_RELEASE);
    return MI_OK;
}

extern "C" int mi_bilu4_set_solve_form(mi_bilu4_t F, int form)
{
    const bool known = form == MI_BILU_FORM_LEVELS || form == MI_BILU_FORM_ONE || form == MI_BILU_FORM_AUTO;
    if (const int rc = bilu_guard(F, "mi_bilu4_set_solve_form", kHostOnlyDev, known ? nullptr : "unknown solve form (0: one launch per level, 1: one launch, -1: measure and choose)"); rc != kBiluGo)
        return rc;
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
    HIP_TRY(hipMemset(F->d_b, 0, sizeof(double) * 4 * (size_t)F->pat().nb));
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
    if (const int rc = bilu_guard(F, "mi_bilu4one_status", kHostOnlyDev); rc != kBiluGo) return rc;
    if (bilu_one_gave_up(F)) return fail(MI_ERR_HIP, kOneGaveUp);
    return MI_OK;
}

extern "C" int mi_bilu4one_info(mi_bilu4_t F, int* prepared, int* eligible, int* workgroups, int nchunks[2], int max_deps[2], long long* plan_bytes)
{
    CHECK_ARG(F, "null handle");
    const Bilu4OneTables& T = F->one;
    if (prepared) *prepared = T.state == 1;
    if (eligible) *eligible = T.state == 1;
    if (workgroups) *workgroups = T.state == 1 ? T.wgs : 0;
    for (int b = 0; b < 2; b++) {
        if (nchunks) nchunks[b] = T.nchunks[b];
        if (max_deps) max_deps[b] = T.max_deps[b];
    }
    if (plan_bytes) *plan_bytes = T.state == 1 ? T.plan_bytes : 0;
    return MI_OK;
}

// ---------------------------------------------------------------- mi_bilu4sw_*: the factor applied by fixed Jacobi sweeps
static const char* bilu_sw_bad_counts(int sf, int sb) { return sf < 0 || sb < 0 ? "negative sweep count" : nullptr; }

// levels - 1 of sweep b: the count at which the sweeps have reached the exact solve's bits, where counts are clamped
static int bilu_sw_max(const mi_bilu4_s* F, int b) { return std::max(F->sched.sweep[b].nlev() - 1, 0); }

static dim3 bilu_sw_grid(int nb) { return dim3((unsigned)((nb + kBiluRowsPerWG - 1) / kBiluRowsPerWG)); }

// one sweep; AL by the vector that is gathered (the work vectors are aligned, b need not be)
template <bool BWD, class T>
static void bilu_sw_launch(const Bilu4SweepView& V, const Bilu4SweepVals<T>& A, int nb, const double* src, const double* old, double* out, hipStream_t s)
{
    constexpr int P = std::is_same<T, float>::value ? kBiluSweepDepthF32 : kBiluSweepDepth;
    bilu_by_alignment(old, [&](auto al) {
        hipLaunchKernelGGL((bilu4_sweep<BWD, decltype(al)::value, P, T>), bilu_sw_grid(nb), dim3(kWG), 0, s, V, A, nb, src, old, out);
        return 0;
    });
}

// sf forward sweeps, the diagonal pass, sb backward sweeps, on the caller's stream: launches only.  d_b is read by every forward
// sweep and never written unless it is d_x; d_x is written by the LAST launch only, when d_b is no longer needed.
// Lv, Uv: the values of the two triangles in the type they are streamed in (the factor's own, or its single-precision copy);
// *launches_last: the count of the precision that was asked for.
template <class T>
static int bilu_sw_solve_launch(mi_bilu4_s* F, const Bilu4SweepVals<T>& Lv, const Bilu4SweepVals<T>& Uv, int* launches_last, const double* d_b, double* d_x, int sf, int sb,
                                hipStream_t s)
{
    static_assert(kBiluRowsPerWG * 4 == kWG, "four lanes per block row");
    const int nb = F->pat().nb;
    sf = std::min(sf, bilu_sw_max(F, 0));
    sb = std::min(sb, bilu_sw_max(F, 1));
    double* const w[3] = {F->sw.w[0], F->sw.w[1], F->sw.w[2]};
    const Bilu4SweepView L = bilu_view(F->lev[0]), U = bilu_view(F->lev[1]);
    const double* t = d_b; // t^0
    for (int k = 0; k < sf; k++) {
        bilu_sw_launch<false>(L, Lv, nb, d_b, t, w[k & 1], s);
        t = w[k & 1];
    }
    double* const pong[2] = {t == w[0] ? w[1] : w[0], w[2]}; // free of t, whichever vector holds it
    double* x = sb == 0 ? d_x : pong[0];
    hipLaunchKernelGGL(bilu4_sweep_diag<T>, bilu_sw_grid(nb), dim3(kWG), 0, s, U, Uv.dinv, nb, t, x);
    for (int k = 0; k < sb; k++) {
        double* const out = k == sb - 1 ? d_x : pong[(k + 1) & 1];
        bilu_sw_launch<true>(U, Uv, nb, t, x, out, s);
        x = out;
    }
    HIP_TRY(hipGetLastError());
    *launches_last = sf + 1 + sb;
    return MI_OK;
}

extern "C" int mi_bilu4sw_prepare(mi_bilu4_t F)
{
    if (const int rc = bilu_guard(F, "mi_bilu4sw_prepare", kHostOnlySweep); rc != kBiluGo) return rc;
    if (F->sw.prepared) return MI_OK;
    Bilu4SweepWork W; // moves into the handle once it is complete; a failure on the way frees what there is
    for (DevArray<double>& v : W.w) // (uninitialised: every sweep writes all rows of its output before anything reads them)
        if (const int rc = dev_alloc(v, 4 * (size_t)F->pat().nb, 1)) return rc;
    W.prepared = true;
    F->sw = std::move(W);
    return MI_OK;
}

extern "C" int mi_bilu4sw_info(mi_bilu4_t F, int* prepared, int* max_fwd, int* max_bwd, int* launches_last, long long* work_bytes)
{
    CHECK_ARG(F, "null handle");
    if (prepared) *prepared = F->sw.prepared ? 1 : 0;
    if (max_fwd) *max_fwd = bilu_sw_max(F, 0);
    if (max_bwd) *max_bwd = bilu_sw_max(F, 1);
    if (launches_last) *launches_last = F->sw.launches_last;
    if (work_bytes) *work_bytes = F->sw.prepared ? 3LL * 4 * F->pat().nb * (long long)sizeof(double) : 0;
    return MI_OK;
}

// ---------------------------------------------------------------- mi_bilu4sp_*: the sweeps over a single-precision copy of the values
extern "C" int mi_bilu4sp_prepare(mi_bilu4_t F)
{
    if (const int rc = bilu_guard(F, "mi_bilu4sp_prepare", kHostOnlySweep); rc != kBiluGo) return rc;
    if (F->sp.prepared) return MI_OK;
    Bilu4SpCopy S; // moves into the handle once it is complete; a failure on the way frees what there is
    int rc;
    if ((rc = bilu_each_values(F, S, [](const double*, DevArray<float>& copy, size_t blocks, auto&&) { return dev_alloc(copy, 16 * std::max<size_t>(blocks, 1)); })) ||
        (rc = dev_alloc(S.rec, 1)))
        return rc;
    // the factor as it is now: behind everything that was enqueued to write it, and finished before the first solve on any stream
    HIP_TRY(hipDeviceSynchronize());
    if ((rc = bilu_sp_convert(F, S, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if ((rc = mi_bilu4sw_prepare(F))) return rc; // the same three work vectors
    S.prepared = true;
    F->sp = std::move(S);
    return MI_OK;
}

extern "C" int mi_bilu4sp_status(mi_bilu4_t F, int* bad_block_row, long long* overflowed)
{
    if (F && bad_block_row) *bad_block_row = -1;
    if (F && overflowed) *overflowed = 0;
    if (const int rc = bilu_guard(F, "mi_bilu4sp_status", kHostOnlySweep); rc != kBiluGo) return rc;
    if (!F->sp.prepared) return MI_OK; // no copy yet
    HIP_TRY(hipDeviceSynchronize());
    Bilu4SpRecord R{};
    HIP_TRY(hipMemcpy(&R, F->sp.rec, sizeof(R), hipMemcpyDeviceToHost));
    if (R.overflowed == 0) return MI_OK;
    R.row = F->ord.caller_row(R.row);
    if (bad_block_row) *bad_block_row = R.row;
    if (overflowed) *overflowed = (long long)R.overflowed;
    return fail(MI_ERR_ARG, "mi_bilu4sp: " + std::to_string(R.overflowed) + " finite value(s) of the factor are beyond the range of float and are Inf in the single-precision copy; the first in block row " +
                                std::to_string(R.row));
}

extern "C" int mi_bilu4sp_fetch(mi_bilu4_t F, float* val, long long cap_blocks)
{
    if (const int rc = bilu_guard(F, "mi_bilu4sp_fetch", kHostOnlySweep, nullptr, val ? nullptr : "null val"); rc != kBiluGo) return rc;
    CHECK_ARG(cap_blocks >= F->pat().nblocks(), "array too short: need mi_bilu4_info's nblocks blocks of 16 floats");
    if (!F->sp.prepared) return fail(MI_ERR_STATE, "mi_bilu4sp_fetch: the handle is not prepared (mi_bilu4sp_prepare)");
    HIP_TRY(hipDeviceSynchronize());
    // as bilu_move_values brings the double factor back: each level-major block to its place in the host factor's order
    std::vector<float> v;
    return bilu_each_values(F, F->sp, [&](const double*, DevArray<float>& copy, size_t n, auto&& host_block) -> int {
        if (!n) return MI_OK;
        v.resize(16 * n);
        HIP_TRY(hipMemcpy(v.data(), copy, sizeof(float) * v.size(), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < n; k++) memcpy(val + 16 * (size_t)host_block(k), &v[16 * k], sizeof(float) * 16);
        return MI_OK;
    });
}

extern "C" int mi_bilu4sp_info(mi_bilu4_t F, int* prepared, int* convert_launches, int* launches_last, long long* copy_bytes)
{
    CHECK_ARG(F, "null handle");
    if (prepared) *prepared = F->sp.prepared ? 1 : 0;
    if (convert_launches) *convert_launches = F->sp.convert_launches;
    if (launches_last) *launches_last = F->sp.launches_last;
    if (copy_bytes) *copy_bytes = F->sp.prepared ? (long long)(16 * sizeof(float)) * F->pat().nblocks() : 0;
    return MI_OK;
}

// ---------------------------------------------------------------- the one apply path: every solve entry point, and GMRES's step
// A way of applying the factor is a Bilu4Apply (capi_internal.hpp); what differs between the four is this table's row and the
// launcher bilu_apply picks.  The exact solve over the single-precision copy (mi_bilu4spx_*) is that of mi_bilu4_solve* with the
// float instantiations of the same kernels — always level by level: the one-launch form is not a template over the stored type.
struct Bilu4Way {
    const char *name_dev, *name_host; // as the two entry points report themselves
    BiluHostOnly host_only;
    int (*prepare)(mi_bilu4_t);       // what a first solve needs made (null: nothing) ...
    const char* unprepared_capturing; // ... and cannot make while the stream is capturing
};
static const Bilu4Way kBiluWays[2][2] = { // [sweeps][f32]
    {{"mi_bilu4_solve", "mi_bilu4_solve", kHostOnlyDev, nullptr, nullptr},
     {"mi_bilu4spx_solve_dev", "mi_bilu4spx_solve", kHostOnlySweep, mi_bilu4sp_prepare,
      "mi_bilu4spx_solve_dev: the handle is not prepared and the stream is capturing (mi_bilu4sp_prepare allocates and converts: call it before the capture)"}},
    {{"mi_bilu4sw_solve_dev", "mi_bilu4sw_solve", kHostOnlySweep, mi_bilu4sw_prepare,
      "mi_bilu4sw_solve_dev: the handle is not prepared and the stream is capturing (mi_bilu4sw_prepare allocates: call it before the capture)"},
     {"mi_bilu4sp_solve_dev", "mi_bilu4sp_solve", kHostOnlySweep, mi_bilu4sp_prepare,
      "mi_bilu4sp_solve_dev: the handle is not prepared and the stream is capturing (mi_bilu4sp_prepare allocates and converts: call it before the capture)"}},
};
static const Bilu4Way& bilu_way(const Bilu4Apply& how) { return kBiluWays[how.sweeps][how.f32]; }

int bilu4_apply_prepare(mi_bilu4_t F, const Bilu4Apply& how) { return bilu_way(how).prepare ? bilu_way(how).prepare(F) : MI_OK; }

static int bilu_ensure(mi_bilu4_s* F, const Bilu4Apply& how, hipStream_t s)
{
    const Bilu4Way& W = bilu_way(how);
    if (!W.prepare || (how.f32 ? F->sp.prepared : F->sw.prepared)) return MI_OK;
    if (stream_is_capturing(s)) return fail(MI_ERR_STATE, W.unprepared_capturing);
    return W.prepare(F);
}

// d_x = the factor applied to d_b, enqueued on s.  The exact solve in double takes the handle's form — except under stream capture,
// where the level-by-level form is recorded (the one-launch form's epoch is a kernel argument: a replayed graph would present it
// again and every wait would pass at once) — and is the one way that refuses once a hand-off wait has given up.
static int bilu_apply(mi_bilu4_s* F, const Bilu4Apply& how, const double* d_b, double* d_x, hipStream_t s)
{
    if (!how.sweeps && !how.f32 && bilu_one_gave_up(F)) return fail(MI_ERR_HIP, kOneGaveUp);
    if (const int rc = bilu_ensure(F, how, s)) return rc;
    const Bilu4SweepVals<double> L64{F->lev[0].val, nullptr}, U64{F->lev[1].val, F->lev[1].dinv};
    const Bilu4SweepVals<float> L32{F->sp.val[0], nullptr}, U32{F->sp.val[1], F->sp.dinv};
    const int rc = bilu_in_order(F, d_b, d_x, F->ordd.b, F->ordd.x, s, [&](const double* b, double* x) {
        if (how.sweeps)
            return how.f32 ? bilu_sw_solve_launch(F, L32, U32, &F->sp.launches_last, b, x, how.sf, how.sb, s)
                           : bilu_sw_solve_launch(F, L64, U64, &F->sw.launches_last, b, x, how.sf, how.sb, s);
        if (how.f32) return bilu_solve_launch(F, L32, U32, b, x, s);
        if (F->form == MI_BILU_FORM_ONE && !stream_is_capturing(s)) return bilu_solve_one_launch(F, b, x, s);
        return bilu_solve_launch(F, L64, U64, b, x, s);
    });
    if (rc || how.sweeps || !how.f32) return rc;
    F->sp.exact_launches_last = F->sched.sweep[0].nlaunch() + F->sched.sweep[1].nlaunch() + (F->ord.on() ? kBiluOrderLaunches : 0);
    F->sp.exact_wide_last = bilu_wide_launches(F);
    return MI_OK;
}

// the host-pointer form: through the handle's two scratch vectors, on the null stream
static int bilu_apply_host(mi_bilu4_s* F, const Bilu4Apply& how, const double* b, double* x)
{
    const size_t bytes = sizeof(double) * 4 * (size_t)F->pat().nb;
    HIP_TRY(hipMemcpy(F->d_b, b, bytes, hipMemcpyHostToDevice));
    if (const int rc = bilu_apply(F, how, F->d_b, F->d_x, nullptr)) return rc;
    HIP_TRY(hipMemcpy(x, F->d_x, bytes, hipMemcpyDeviceToHost));
    return MI_OK;
}

// a solve entry point: its family's guard, then the one path.  host: b and x are host pointers (and s is not looked at)
static int bilu_solve_entry(mi_bilu4_s* F, const Bilu4Apply& how, bool host, const double* b, double* x, hipStream_t s)
{
    const Bilu4Way& W = bilu_way(how);
    const char* const bad_counts = how.sweeps ? bilu_sw_bad_counts(how.sf, how.sb) : nullptr;
    if (const int rc = bilu_guard(F, host ? W.name_host : W.name_dev, W.host_only, bad_counts, b && x ? nullptr : "null vector"); rc != kBiluGo) return rc;
    return host ? bilu_apply_host(F, how, b, x) : bilu_apply(F, how, b, x, s);
}

int bilu4_apply_dev(mi_bilu4_t F, const Bilu4Apply& how, const double* d_b, double* d_x, hipStream_t s) { return bilu_solve_entry(F, how, false, d_b, d_x, s); }

extern "C" int mi_bilu4_solve_dev(mi_bilu4_t F, const double* d_b, double* d_x, mi_stream_t s) { return bilu_solve_entry(F, {false, false, 0, 0}, false, d_b, d_x, (hipStream_t)s); }

extern "C" int mi_bilu4_solve(mi_bilu4_t F, const double* b, double* x) { return bilu_solve_entry(F, {false, false, 0, 0}, true, b, x, nullptr); }

extern "C" int mi_bilu4sw_solve_dev(mi_bilu4_t F, const double* d_b, double* d_x, int sweeps_fwd, int sweeps_bwd, mi_stream_t s)
{
    return bilu_solve_entry(F, {true, false, sweeps_fwd, sweeps_bwd}, false, d_b, d_x, (hipStream_t)s);
}

extern "C" int mi_bilu4sw_solve(mi_bilu4_t F, const double* b, double* x, int sweeps_fwd, int sweeps_bwd)
{
    return bilu_solve_entry(F, {true, false, sweeps_fwd, sweeps_bwd}, true, b, x, nullptr);
}

extern "C" int mi_bilu4sp_solve_dev(mi_bilu4_t F, const double* d_b, double* d_x, int sweeps_fwd, int sweeps_bwd, mi_stream_t s)
{
    return bilu_solve_entry(F, {true, true, sweeps_fwd, sweeps_bwd}, false, d_b, d_x, (hipStream_t)s);
}

extern "C" int mi_bilu4sp_solve(mi_bilu4_t F, const double* b, double* x, int sweeps_fwd, int sweeps_bwd)
{
    return bilu_solve_entry(F, {true, true, sweeps_fwd, sweeps_bwd}, true, b, x, nullptr);
}

extern "C" int mi_bilu4spx_solve_dev(mi_bilu4_t F, const double* d_b, double* d_x, mi_stream_t s) { return bilu_solve_entry(F, {false, true, 0, 0}, false, d_b, d_x, (hipStream_t)s); }

extern "C" int mi_bilu4spx_solve(mi_bilu4_t F, const double* b, double* x) { return bilu_solve_entry(F, {false, true, 0, 0}, true, b, x, nullptr); }

extern "C" int mi_bilu4spx_info(mi_bilu4_t F, int* launches_last, int* wide_launches_last)
{
    CHECK_ARG(F, "null handle");
    if (launches_last) *launches_last = F->sp.exact_launches_last;
    if (wide_launches_last) *wide_launches_last = F->sp.exact_wide_last;
    return MI_OK;
}
