// capi_bcsr.hip: BCSR 4x4 handles and products, multi-vector products, Krylov basis — part of libmi355spmv.so (see capi_internal.hpp for the layout of the library).
// Built for gfx950 only; no CPU fallback anywhere: every compute entry point needs a HIP device.
#include "capi_internal.hpp"
#include "blas1_kernels.hpp"
#include "spmv_bcsr_sell.hpp"
#include "spmm_tile_plan.hpp"
#include "bcsr4_tile_plan.hpp"

static int sell_fill(mi_bcsr4_t A, hipStream_t s);

// ---------------------------------------------------------------- BCSR 4x4
// The forms of a blocked handle timed against each other on a scratch pair (x = 0: timing does not depend on the values): two rounds
// of 3 + 8 launches per form, select(c) putting form c in place; us[c] = the faster round, 0 where the measurement failed (it never
// wins).  false: no room for the pair, nothing measured.
template <class Select>
static bool bcsr4_race(mi_bcsr4_t A, int ncand, Select select, double* us)
{
    LaunchTimer tm;
    ScratchPair sp;
    if (sp.alloc(4 * (size_t)std::max(A->nbcols, 1), 4 * (size_t)std::max(A->nbrows, 1)) != MI_OK || tm.init() != MI_OK) return false;
    std::vector<char> failed((size_t)ncand, 0);
    for (int round = 0; round < 2; round++)
        for (int c = 0; c < ncand; c++) {
            if (failed[c]) continue;
            select(c);
            double t = 0.0;
            if (tm.time(3, 8, [&] { return launch_bcsr4(A, sp.x, sp.y, nullptr, false); }, &t) == MI_OK) us[c] = min_measured(us[c], t);
            else failed[c] = 1;
        }
    for (int c = 0; c < ncand; c++)
        if (failed[c]) us[c] = 0.0;
    return true;
}

// The x tile per workgroup (spmv_bcsr4_tile): the distinct block columns of each group of 64 block rows, and every block's
// position in its group's list.  Built when no group needs more than the tile holds; then both kernels are timed and the
// faster is kept (MI355_BCSR_TILE=0 never builds it, =1 takes it unmeasured).
static int build_bcsr4_tile(mi_bcsr4_t A, const int* ptrow, const int* indcol)
{
    const long long nb = A->nblocks;
    if (nb < kBtileMinBlocks || env_is("MI355_BCSR_TILE", "0")) return MI_OK;
    Bcsr4TileListsHost H; // the lists themselves: bcsr4_tile_plan.hpp (host only; mi_bcsr4_tile_probe below reports the same call)
    build_bcsr4_tile_lists(A->nbrows, ptrow, indcol, kWG / 4, kBtileNodes, H);
    if (!H.built) return MI_OK;
    Bcsr4TileLists T;
    HIP_TRY(T.ptr.alloc(H.wg_ptr.size()));
    HIP_TRY(T.nodes.alloc(H.nodes.size()));
    HIP_TRY(T.slots.alloc(H.slots.size()));
    HIP_TRY(T.ptr.fill(H.wg_ptr));
    HIP_TRY(T.nodes.fill(H.nodes));
    HIP_TRY(T.slots.fill(H.slots));
    A->tl = std::move(T);
    if (env_is("MI355_BCSR_TILE", "1")) A->use_tile = true;
    else if (!env_is("MI355_SPMV_AUTOTUNE", "0") && nb >= 100000) {
        double us[2] = {0, 0};
        if (bcsr4_race(A, 2, [&](int c) { A->use_tile = c == 1; }, us)) {
            A->tune_us_plain = us[0];
            A->tune_us_tile = us[1];
            A->use_tile = us[1] > 0 && us[1] < us[0];
        }
    }
    return MI_OK;
}

// host-only: the list-building half of build_bcsr4_tile for this block pattern — would the handle hold the x tile, and how full is it
extern "C" int mi_bcsr4_tile_probe(int nbrows, const int* ptrow, const int* indcol, int* would_build, int* groups, int* max_nodes, int* groups_at_cap)
{
    CHECK_ARG(nbrows >= 0 && ptrow && ptrow[0] == 0, "bad argument");
    for (int i = 0; i < nbrows; i++) CHECK_ARG(ptrow[i] <= ptrow[i + 1], "ptrow must be non-decreasing");
    const long long nb = ptrow[nbrows];
    CHECK_ARG(nb == 0 || indcol, "indcol is null");
    for (long long k = 0; k < nb; k++) CHECK_ARG(indcol[k] >= 0, "negative block column");
    Bcsr4TileListsHost H;
    build_bcsr4_tile_lists(nbrows, ptrow, indcol, kWG / 4, kBtileNodes, H);
    if (would_build) *would_build = H.built;
    if (groups) *groups = H.groups;
    if (max_nodes) *max_nodes = H.max_nodes;
    if (groups_at_cap) *groups_at_cap = H.groups_at_cap;
    return MI_OK;
}

// The sliced copy (spmv_bcsr_sell.hpp): 16 block rows per slice, one contiguous stream per persistent wave.  MI_OK without it when
// there is no room for a second copy of the block values: the row-per-quad kernels serve the handle, as build_sstream does for the
// scalar format — a create that worked without the sliced copy must not fail because of it.
static int build_bcsr4_sell(mi_bcsr4_t A, const int* ptrow, const int* indcol)
{
    SellPlanHost P, P2;
    build_sell_plan(A->nbrows, ptrow, indcol, 1024, P);
    build_sell_wave_ranges(P, 2048, P2.wrng, P2.nwaves);
    Bcsr4Sliced S;
    hipError_t e;
    if ((e = S.val.alloc((size_t)(P.nsteps + kSellPadSteps) * kSellStepDoubles)) != hipSuccess || (e = S.col.alloc(P.col.size())) != hipSuccess ||
        (e = S.sptr.alloc(P.sptr.size())) != hipSuccess || (e = S.wrng.alloc(P.wrng.size())) != hipSuccess || (e = S.wrng2.upload(P2.wrng)) != hipSuccess ||
        (e = hipMemset(S.val + (size_t)P.nsteps * kSellStepDoubles, 0, sizeof(double) * (size_t)kSellPadSteps * kSellStepDoubles)) != hipSuccess ||
        (e = S.col.fill(P.col)) != hipSuccess || (e = S.sptr.fill(P.sptr)) != hipSuccess || (e = S.wrng.fill(P.wrng)) != hipSuccess) {
        (void)hipGetLastError();
        S = {};
        return e == hipErrorOutOfMemory ? MI_OK : fail(MI_ERR_HIP, std::string("bcsr4 sliced copy: ") + hipGetErrorString(e));
    }
    A->sell = std::move(S);
    A->sell_nslices = P.nslices;
    A->sell_nwaves = P.nwaves;
    A->sell_nwaves2 = P2.nwaves;
    A->sell_nsteps = P.nsteps;
    // filled HERE and refilled where the block values change (mi_bcsr4_update_values*), on that call's stream — never lazily in
    // front of a product: a product captured into a HIP graph holds only the product's node
    return sell_fill(A, nullptr);
}

// which form mi_bcsr4_spmv* launches once the sliced copy is there: the fastest of the row-per-quad choice and the four sliced variants
static void choose_bcsr4_sell_form(mi_bcsr4_t A, bool forced)
{
    if (const char* fe = getenv("MI355_BCSR_SELL_FORM")) A->sell_form = std::max(0, std::min(3, atoi(fe))); // tests: one variant, unmeasured
    else if (forced) A->sell_form = 0;
    else if (env_is("MI355_SPMV_AUTOTUNE", "0")) A->sell_form = 0; // no measurement: the sliced, non-temporal form for matrices of this size
    else {
        double us[5] = {0, 0, 0, 0, 0}; // [0] the row-per-quad choice made above, [1..4] the sliced variants
        if (!bcsr4_race(A, 5, [&](int c) { A->sell_form = c - 1; }, us)) return;
        int best = 0;
        for (int c = 1; c < 5; c++) {
            A->tune_us_sell[c - 1] = us[c];
            if (better(us[c], us[best])) best = c;
        }
        if (A->tune_us_plain <= 0 && A->tune_us_tile <= 0) A->tune_us_plain = us[0];
        A->sell_form = best - 1;
    }
}

extern "C" int mi_bcsr4_create(int nbrows, int nbcols, const int* ptrow, const int* indcol, const double* coef,
                               mi_bcsr4_t* out)
{
    CHECK_ARG(out, "out is null");
    *out = nullptr;
    CHECK_ARG(nbrows >= 0 && nbcols >= 0 && ptrow && ptrow[0] == 0, "bad argument");
    for (int i = 0; i < nbrows; i++) CHECK_ARG(ptrow[i] <= ptrow[i + 1], "ptrow must be non-decreasing");
    const long long nb = ptrow[nbrows];
    CHECK_ARG(nb == 0 || (indcol && coef), "indcol/coef is null");
    for (long long k = 0; k < nb; k++) CHECK_ARG(indcol[k] >= 0 && indcol[k] < nbcols, "block column outside [0, nbcols)");
    int rc = need_device();
    if (rc) return rc;
    // destroyed on every early return below, released to the caller on success
    std::unique_ptr<mi_bcsr4_s> owner(new (std::nothrow) mi_bcsr4_s());
    mi_bcsr4_t A = owner.get();
    if (!A) return fail(MI_ERR_ALLOC, "host allocation failed");
    A->nbrows = nbrows;
    A->nbcols = nbcols;
    A->nblocks = nb;
    HIP_TRY(hipGetDevice(&A->device));
    HIP_TRY(A->d_ptrow.alloc((size_t)nbrows + 1));
    HIP_TRY(A->d_indcol.alloc((size_t)nb + 1));
    HIP_TRY(A->d_coef.alloc(16 * ((size_t)nb + 1)));
    HIP_TRY(A->d_ptrow.fill(ptrow, (size_t)nbrows + 1));
    HIP_TRY(A->d_indcol.fill(indcol, (size_t)nb));
    HIP_TRY(A->d_coef.fill(coef, 16 * (size_t)nb));
    for (int s0 = 0; s0 < nbrows; s0 += kSellRows) // values of the longest slice of 16 block rows (bcsr4_refresh_kernel picks its LDS buffer by it)
        A->max_slice_vals = std::max(A->max_slice_vals, 16 * (ptrow[std::min(nbrows, s0 + kSellRows)] - ptrow[s0]));
    if ((rc = build_bcsr4_tile(A, ptrow, indcol))) return rc;
    // The sliced copy: built for matrices large enough to stream (MI355_BCSR_SELL=0 never, =1 always and unmeasured with D = 4,
    // non-temporal); its four variants are timed against the row-per-quad kernels above and the fastest of all is what
    // mi_bcsr4_spmv* launches.  Costs a second copy of the block values on the device (+0.9 % padding on the FE matrix).
    // Never for a matrix without block columns (forced only: it has no blocks): the sliced kernels read x at node 0 for every padding
    // place, and every slice of such a matrix is one padding step — 32 bytes of an x that has no elements.
    const bool forced = env_is("MI355_BCSR_SELL", "1");
    if (!env_is("MI355_BCSR_SELL", "0") && (forced || nb >= 100000) && nbcols > 0 && nbcols < (1 << 30)) {
        if ((rc = build_bcsr4_sell(A, ptrow, indcol))) return rc;
        if (A->sell.val) choose_bcsr4_sell_form(A, forced);
    }
    // the handle is complete on return (the sliced values are filled on the null stream, which a non-blocking stream does not wait for)
    if (hipError_t e = hipStreamSynchronize(nullptr)) return fail(MI_ERR_HIP, std::string("mi_bcsr4_create: ") + hipGetErrorString(e));
    *out = owner.release();
    return MI_OK;
}

// (re)fill the sliced copy from the row-major blocks, on stream s
static int sell_fill(mi_bcsr4_t A, hipStream_t s)
{
    const int grid = std::max(1, std::min(A->sell_nslices, 8192));
    hipLaunchKernelGGL(bcsr4_to_sell_kernel, dim3((unsigned)grid), dim3(64), 0, s, A->sell_nslices, A->nbrows, A->d_ptrow, A->d_coef, A->sell.sptr, A->sell.val);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

// fn(CAP, grid) for a refresh kernel: the slice capacity it is compiled for, by the handle's largest slice, and its grid.
// 4096: 32 KB of LDS, four workgroups per CU (the FE rows of 56-60: 3 584-3 840 values per slice); 0: no LDS staging
template <class Fn>
static void by_slice_cap(const mi_bcsr4_s* A, int nslices, Fn&& fn)
{
    const int grid = std::max(1, std::min(nslices, 2048));
    const int cap = A->max_slice_vals <= 4096 ? 4096 : (A->max_slice_vals <= 16384 ? 16384 : 0);
    pick_int<4096, 16384, 0>(cap, [&](auto CAP) { fn(CAP, (unsigned)(CAP() == 16384 ? std::min(grid, 256) : grid)); });
}

// the blocked copy of a CSR handle from that handle's (new) CSR values, d_src — and, when d_csr_out is given, the handle's CSR value
// array — in one pass (bcsr4_refresh_kernel); every copy the blocked kernels read is current when this returns (in stream order)
int bcsr4_refresh_from_csr(mi_bcsr4_s* A, const int* d_csr_ptrow, const double* d_src, double* d_csr_out, hipStream_t s)
{
    if (!A || A->nbrows == 0) return MI_OK;
    const int nslices = (A->nbrows + kSellRows - 1) / kSellRows;
    const int* sptr = A->sell.val ? A->sell.sptr : nullptr;
    double* sv = A->sell.val;
    by_slice_cap(A, nslices, [&](auto CAP, unsigned grid) {
        hipLaunchKernelGGL((bcsr4_refresh_kernel<CAP()>), dim3(grid), dim3(256), 0, s, nslices, A->nbrows, d_csr_ptrow, d_src, d_csr_out, A->d_ptrow, A->d_coef, sptr, sv);
    });
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

// new block values from a device array in the caller's layout: the handle's row-major blocks and the sliced values in one pass
static int bcsr4_refresh_from_blocks(mi_bcsr4_s* A, const double* d_src, bool colmajor, hipStream_t s)
{
    if (!A || A->nbrows == 0 || A->nblocks == 0) return MI_OK;
    const int nslices = (A->nbrows + kSellRows - 1) / kSellRows;
    const int* sptr = A->sell.val ? A->sell.sptr : nullptr;
    double* out = d_src == A->d_coef ? nullptr : A->d_coef;
    if (colmajor && !out) return fail(MI_ERR_ARG, "column-major blocks cannot be transposed in place");
    if (!out && !A->sell.val) return MI_OK;
    by_slice_cap(A, nslices, [&](auto CAP, unsigned grid) {
        pick([&](auto CM) {
            hipLaunchKernelGGL((bcsr4_blocks_refresh_kernel<CAP(), CM()>), dim3(grid), dim3(256), 0, s, nslices, A->nbrows, A->d_ptrow, d_src, out, sptr, A->sell.val);
        }, colmajor);
    });
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

int bcsr4_values_changed(mi_bcsr4_s* A, hipStream_t s)
{
    if (A && A->sell.val && A->nblocks > 0) return sell_fill(A, s);
    return MI_OK;
}

extern "C" int mi_bcsr4_sell_info(mi_bcsr4_t A, int* built, int* form_in_use, long long* steps, double* padding, double us[4])
{
    CHECK_ARG(A, "null handle");
    if (built) *built = A->sell.val != nullptr;
    if (form_in_use) *form_in_use = A->sell.val ? A->sell_form : -1;
    if (steps) *steps = A->sell_nsteps;
    if (padding) *padding = A->nblocks > 0 && A->sell.val ? (double)A->sell_nsteps * kSellRows / (double)A->nblocks - 1.0 : 0.0;
    if (us)
        for (int i = 0; i < 4; i++) us[i] = A->tune_us_sell[i];
    return MI_OK;
}

// The plan of the sliced copy without a device: build_sell_plan as build_bcsr4_sell calls it (which asks for 1024 waves, then for the
// ranges of 2048 through build_sell_wave_ranges — what build_sell_plan itself calls with nwaves_max), copied out.
extern "C" int mi_bcsr4_sell_plan_probe(int nbrows, const int* ptrow, const int* indcol, int nwaves_max, int* nslices, long long* nsteps,
                                        int* nwaves, int* sptr, int* wrng, unsigned* col)
{
    CHECK_ARG(nbrows >= 0 && ptrow && ptrow[0] == 0 && nwaves_max >= 1, "bad argument");
    for (int i = 0; i < nbrows; i++) CHECK_ARG(ptrow[i] <= ptrow[i + 1], "ptrow must be non-decreasing");
    const long long nb = ptrow[nbrows];
    CHECK_ARG(nb == 0 || indcol, "indcol is null");
    for (long long k = 0; k < nb; k++) CHECK_ARG(indcol[k] >= 0 && indcol[k] < (1 << 30), "block column outside [0, 2^30)");
    SellPlanHost P;
    build_sell_plan(nbrows, ptrow, indcol, nwaves_max, P);
    if (nslices) *nslices = P.nslices;
    if (nsteps) *nsteps = P.nsteps;
    if (nwaves) *nwaves = P.nwaves;
    if (sptr) std::copy(P.sptr.begin(), P.sptr.end(), sptr);
    if (wrng) std::copy(P.wrng.begin(), P.wrng.end(), wrng);
    if (col) std::copy(P.col.begin(), P.col.end(), col);
    return MI_OK;
}

// ---- PETSc BAIJ block layout (column-major 4x4 blocks: v[0], v[4], v[8], v[12] are row 0 — src/kernels/baij4_mad.c:73-76) ------
// The kernels read row-major blocks (mpk/SpMV.cpp:112).  A PETSc-side caller hands its Mat_SeqBAIJ arrays over as they are and
// says so; the blocks are transposed on the way to the device (setup-time / value-refresh traffic, never per product).
static void transpose_blocks_host(long long nb, const double* src, double* dst)
{
    for (long long k = 0; k < nb; k++)
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) dst[16 * k + 4 * r + c] = src[16 * k + 4 * c + r];
}

extern "C" int mi_bcsr4_create_layout(int nbrows, int nbcols, const int* ptrow, const int* indcol, const double* coef, int layout,
                                      mi_bcsr4_t* out)
{
    CHECK_ARG(layout == MI_BLOCK_ROWMAJOR || layout == MI_BLOCK_COLMAJOR, "unknown block layout");
    if (layout == MI_BLOCK_ROWMAJOR) return mi_bcsr4_create(nbrows, nbcols, ptrow, indcol, coef, out);
    CHECK_ARG(out, "out is null");
    *out = nullptr;
    CHECK_ARG(nbrows >= 0 && ptrow && ptrow[0] == 0 && ptrow[nbrows] >= 0, "bad argument");
    const long long nb = ptrow[nbrows];
    CHECK_ARG(nb == 0 || coef, "coef is null");
    std::vector<double> t((size_t)nb * 16);
    transpose_blocks_host(nb, coef, t.data());
    return mi_bcsr4_create(nbrows, nbcols, ptrow, indcol, t.data(), out);
}

extern "C" int mi_bcsr4_update_values_layout(mi_bcsr4_t A, const double* coef, int layout)
{
    CHECK_ARG(A, "null handle");
    CHECK_ARG(layout == MI_BLOCK_ROWMAJOR || layout == MI_BLOCK_COLMAJOR, "unknown block layout");
    if (layout == MI_BLOCK_ROWMAJOR || A->nblocks == 0) return mi_bcsr4_update_values(A, coef);
    CHECK_ARG(coef, "null coef");
    std::vector<double> t((size_t)A->nblocks * 16);
    transpose_blocks_host(A->nblocks, coef, t.data());
    return mi_bcsr4_update_values(A, t.data());
}

extern "C" int mi_bcsr4_update_values_layout_dev(mi_bcsr4_t A, const double* d_coef, int layout, mi_stream_t s)
{
    CHECK_ARG(A, "null handle");
    CHECK_ARG(layout == MI_BLOCK_ROWMAJOR || layout == MI_BLOCK_COLMAJOR, "unknown block layout");
    if (layout == MI_BLOCK_ROWMAJOR || A->nblocks == 0) return mi_bcsr4_update_values_dev(A, d_coef, s);
    CHECK_ARG(d_coef && d_coef != A->d_coef, "null coef, or the handle's own array");
    return bcsr4_refresh_from_blocks(A, d_coef, true, (hipStream_t)s); // transposed on the way, blocks and sliced values in one pass
}

extern "C" int mi_bcsr4_tile_info(mi_bcsr4_t A, int* built, int* in_use, double* us_plain, double* us_tile)
{
    CHECK_ARG(A, "null handle");
    if (built) *built = A->tl.ptr != nullptr;
    if (in_use) *in_use = A->use_tile && A->tl.ptr;
    if (us_plain) *us_plain = A->tune_us_plain;
    if (us_tile) *us_tile = A->tune_us_tile;
    return MI_OK;
}

// new block values (16 per block, row-major) for an unchanged block pattern
extern "C" int mi_bcsr4_update_values(mi_bcsr4_t A, const double* coef)
{
    CHECK_ARG(A, "null handle");
    if (A->nblocks == 0) return MI_OK;
    CHECK_ARG(coef, "null coef");
    HIP_TRY(hipMemcpy(A->d_coef, coef, sizeof(double) * 16 * (size_t)A->nblocks, hipMemcpyHostToDevice));
    int rc = bcsr4_values_changed(A, nullptr);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return MI_OK;
}

extern "C" int mi_bcsr4_update_values_dev(mi_bcsr4_t A, const double* d_coef, mi_stream_t s)
{
    CHECK_ARG(A, "null handle");
    if (A->nblocks == 0) return MI_OK;
    CHECK_ARG(d_coef, "null coef");
    return bcsr4_refresh_from_blocks(A, d_coef, false, (hipStream_t)s);
}

extern "C" int mi_bcsr4_destroy(mi_bcsr4_t A)
{
    if (!A) return MI_OK;
    delete A;
    return MI_OK;
}

int launch_bcsr4(mi_bcsr4_t A, const double* d_x, double* d_y, mi_stream_t s, bool use_map)
{
    CHECK_ARG(A, "null handle");
    if (A->nbrows == 0) return MI_OK;
    CHECK_ARG(d_x && d_y, "null vector");
    CHECK_ARG((((uintptr_t)d_x) & 15) == 0, "x must be 16-byte aligned");
    Bcsr4View V{A->nbrows, A->nbcols, A->d_ptrow, A->d_indcol, A->d_coef, use_map ? A->d_browmap : nullptr};
    const long long threads = 4LL * A->nbrows;
    const int nwg = (int)((threads + kWG - 1) / kWG);
    static const int chunk = getenv("MI355_BCSR_XCD_CHUNK") ? atoi(getenv("MI355_BCSR_XCD_CHUNK")) : 0;
    const int grid = nwg;
    // the sliced form (a relabelled matrix's blocked copy stores through its block-row map)
    if (A->sell_form >= 0 && A->sell.val) {
        // forms (mi_bcsr4_sell_info): 0 / 1 / 3 one wave per SIMD — one workgroup of four waves per CU, 8 (12) steps of prefetch,
        // non-temporal / temporal / non-temporal; 2 one workgroup of eight waves per CU, 4 steps, non-temporal.  All park y in LDS.
        const bool two = A->sell_form == 2;
        SellView S{A->sell.val, A->sell.col, A->sell.sptr, two ? A->sell.wrng2 : A->sell.wrng, A->sell_nslices, A->nbrows, V.browmap};
        const int swg = two ? A->sell_nwaves2 / 8 : A->sell_nwaves / 4;
        pick_int<0, 1, 2, 3>(A->sell_form, [&](auto F) {
            constexpr int DEPTH = F() == 2 ? 4 : (F() == 3 ? 12 : 8), WAVES = F() == 2 ? 8 : 4;
            hipLaunchKernelGGL((spmv_bcsr4_sell<DEPTH, F() != 1, 0, 2, WAVES>), dim3((unsigned)swg), dim3(64 * WAVES), 0, (hipStream_t)s, S, d_x, d_y, swg);
        });
        HIP_TRY(hipGetLastError());
        return MI_OK;
    }
    if (A->use_tile && A->tl.ptr) {
        Bcsr4Tile Tl{A->tl.ptr, A->tl.nodes, A->tl.slots};
        hipLaunchKernelGGL(spmv_bcsr4_tile<kBcsrDepth>, dim3((unsigned)grid), dim3(kWG), 0, (hipStream_t)s, V, Tl, d_x, d_y, nwg);
        HIP_TRY(hipGetLastError());
        return MI_OK;
    }
    hipLaunchKernelGGL(spmv_bcsr4<kBcsrDepth>, dim3((unsigned)grid), dim3(kWG), 0, (hipStream_t)s, V, d_x, d_y, chunk, nwg);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

void bcsr4_drop_sliced(mi_bcsr4_s* A)
{
    if (!A || !A->sell.val) return;
    (void)hipDeviceSynchronize();
    A->sell = {};
    A->sell_form = -1;
}

extern "C" int mi_bcsr4_spmv_dev(mi_bcsr4_t A, const double* d_x, double* d_y, mi_stream_t s)
{
    return launch_bcsr4(A, d_x, d_y, s, true);
}

extern "C" int mi_bcsr4_spmv(mi_bcsr4_t A, const double* x, double* y)
{
    CHECK_ARG(A, "null handle");
    if (A->nbrows == 0) return MI_OK;
    CHECK_ARG(x && y, "null vector");
    if (!A->d_x) HIP_TRY(A->d_x.alloc(4 * (size_t)(A->nbcols > 0 ? A->nbcols : 1)));
    if (!A->d_y) HIP_TRY(A->d_y.alloc(4 * (size_t)A->nbrows));
    HIP_TRY(hipMemcpy(A->d_x, x, sizeof(double) * 4 * (size_t)A->nbcols, hipMemcpyHostToDevice));
    int rc = mi_bcsr4_spmv_dev(A, A->d_x, A->d_y, nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(y, A->d_y, sizeof(double) * 4 * (size_t)A->nbrows, hipMemcpyDeviceToHost));
    return MI_OK;
}

extern "C" int mi_bcsr4_spmk_dev(mi_bcsr4_t A, int k, const double* d_x, double* const* d_y_out, mi_stream_t s)
{
    CHECK_ARG(A, "null handle");
    if (k < 1 || k > MI_MAX_POWERS) return fail(MI_ERR_UNSUPPORTED, "k must be in 1..MI_MAX_POWERS");
    CHECK_ARG(A->nbrows == A->nbcols, "matrix powers need a square matrix");
    CHECK_ARG(d_y_out, "null output array");
    const double* src = d_x;
    for (int p = 0; p < k; p++) {
        CHECK_ARG(A->nbrows == 0 || d_y_out[p], "null output vector");
        int rc = mi_bcsr4_spmv_dev(A, src, d_y_out[p], s);
        if (rc) return rc;
        src = d_y_out[p];
    }
    return MI_OK;
}

extern "C" int mi_bcsr4_spmk(mi_bcsr4_t A, int k, const double* x, double* const* y_out)
{
    CHECK_ARG(A, "null handle");
    if (k < 1 || k > MI_MAX_POWERS) return fail(MI_ERR_UNSUPPORTED, "k must be in 1..MI_MAX_POWERS");
    CHECK_ARG(A->nbrows == A->nbcols, "matrix powers need a square matrix");
    if (A->nbrows == 0) return MI_OK;
    CHECK_ARG(x && y_out, "null vector");
    const size_t n = 4 * (size_t)A->nbrows;
    if (!A->d_x) HIP_TRY(A->d_x.alloc(n));
    if (int rc = A->d_pow.grow(k, n)) return rc;
    HIP_TRY(hipMemcpy(A->d_x, x, sizeof(double) * n, hipMemcpyHostToDevice));
    int rc = mi_bcsr4_spmk_dev(A, k, A->d_x, A->d_pow.ptr.data(), nullptr);
    if (rc) return rc;
    for (int p = 0; p < k; p++) {
        CHECK_ARG(y_out[p], "null output vector");
        HIP_TRY(hipMemcpy(y_out[p], A->d_pow.ptr[p], sizeof(double) * n, hipMemcpyDeviceToHost));
    }
    return MI_OK;
}

// ---------------------------------------------------------------- multi-vector products, Krylov basis
template <int S>
static void launch_spmm_s(const Bcsr4View& V, int arith, const double* X, long long ldx, double* Y, long long ldy, hipStream_t s)
{
    const long long threads = 4LL * V.nbrows;
    const int nwg = (int)((threads + kWG - 1) / kWG);
    // measured on the FE matrix (bench.py --workload fe_spmm4 / fe_spmm8, MI355_SPMM_XCD=0|1): 8 columns 284 us in XCD order
    // against 343 in dispatch order (x traffic is 8x a single product's and every L2 fetched all of it); 4 columns 179
    // against 173 (not bound by x traffic yet) — so XCD order from five columns on.  MI355_SPMM_XCD=0|1 forces.
    static const int xcd_env = getenv("MI355_SPMM_XCD") ? atoi(getenv("MI355_SPMM_XCD")) : -1;
    const bool xcd = xcd_env >= 0 ? xcd_env != 0 : S > 4;
    const dim3 grid((unsigned)(xcd ? kNXCD * ((nwg + kNXCD - 1) / kNXCD) : nwg)), block(kWG);
    constexpr bool PF = S <= 4; // beyond four columns the prefetch stage costs more occupancy than it hides latency
    static const bool quad = !env_is("MI355_SPMM_QUAD", "0");
    if (S % 4 == 0 && quad) { // the quad of a block row shares its x blocks through DPP (spmv_kernels.hpp: spmm_bcsr4_quad)
        constexpr int SQ = S % 4 == 0 ? S : 4;
        static const int depth_env = getenv("MI355_SPMM_DEPTH") ? atoi(getenv("MI355_SPMM_DEPTH")) : 0;
        // measured on the FE matrix (bench.py fe_spmm4 / fe_spmm8, MI355_SPMM_DEPTH): 4 columns 254 / 168 / 168 / 173 us at depth 1 / 2 / 3 / 4
        // (registers cost occupancy: 7 / 5 / 4 / 3 waves per SIMD), 8 columns 223 / 232 / 237 us at depth 1 / 2 / 3
        const int depth = depth_env >= 1 && depth_env <= 4 ? depth_env : (S == 4 ? 2 : 1);
        pick_int<1, 2, 3, 4>(depth, [&](auto PD) {
            pick([&](auto BA, auto XCD) { hipLaunchKernelGGL((spmm_bcsr4_quad<SQ, BA() ? 1 : 0, XCD(), PD()>), grid, block, 0, s, V, X, ldx, Y, ldy, nwg); },
                 arith == MI_ARITH_BLOCKACC, xcd);
        });
        return;
    }
    pick([&](auto BA, auto XCD) { hipLaunchKernelGGL((spmm_bcsr4<S, BA() ? 1 : 0, PF, XCD()>), grid, block, 0, s, V, X, ldx, Y, ldy, nwg); },
         arith == MI_ARITH_BLOCKACC, xcd);
}

// ---- the tile form (spmm_tile.hpp) ------------------------------------------------------------------------------------------

// The plan itself — clusters, halving, lists, slots, rows, the 16-bit refusal — is spmm_tile_plan.hpp's build_spmm_tile_plan_host
// (host only; mi_bcsr4_spmm_plan_probe below copies the same arrays out).  Here: the upload, unchanged.
// MI355_SPMM_TILE_SORT=0: a tile's rows in growth order (A/B); read once per process.
static bool spmm_tile_sort_rows()
{
    static const bool sort_rows = !env_is("MI355_SPMM_TILE_SORT", "0");
    return sort_rows;
}

static int build_spmm_tile_plan(mi_bcsr4_t A, int per, int ucap, const std::vector<int>& ptrow, const std::vector<int>& indcol, SpmmTilePlan& out)
{
    SpmmTilePlanHost H;
    if (build_spmm_tile_plan_host(A->nbrows, ptrow.data(), indcol.data(), per, ucap, spmm_tile_sort_rows(), H) != 1) return -1;
    SpmmTilePlan T;
    if (T.d_ptr.alloc(H.wg_ptr.size()) != hipSuccess || T.d_nodes.alloc(H.nodes.size()) != hipSuccess || T.d_slots.alloc(H.slots.size()) != hipSuccess ||
        T.d_rows.alloc(H.rows.size()) != hipSuccess || T.d_ptr.fill(H.wg_ptr) != hipSuccess || T.d_nodes.fill(H.nodes) != hipSuccess ||
        T.d_slots.fill(H.slots) != hipSuccess || T.d_rows.fill(H.rows) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    T.rows = per;
    T.umax = H.umax;
    T.ntiles = H.ntiles;
    T.mean_list = H.mean_list;
    out = std::move(T);
    return 1;
}

// The plan without a device: the arrays build_spmm_tile_plan uploads for this pattern, `per` and `ucap`, copied out.
extern "C" int mi_bcsr4_spmm_plan_probe(int nbrows, const int* ptrow, const int* indcol, int per, int ucap, int* refused, int* ntiles, int* umax,
                                        double* mean_list, int* wg_ptr, long long wg_ptr_cap, unsigned* nodes, long long nodes_cap,
                                        unsigned short* slots, long long slots_cap, int* rows, long long rows_cap)
{
    CHECK_ARG(nbrows >= 0 && ptrow && ptrow[0] == 0, "bad argument");
    CHECK_ARG(per == 128 || per == 64, "per must be 128 or 64");
    CHECK_ARG(ucap >= 1, "ucap must be positive");
    for (int i = 0; i < nbrows; i++) CHECK_ARG(ptrow[i] <= ptrow[i + 1], "ptrow must be non-decreasing");
    const long long nb = ptrow[nbrows];
    CHECK_ARG(nb == 0 || indcol, "indcol is null");
    for (long long k = 0; k < nb; k++) CHECK_ARG(indcol[k] >= 0, "negative block column");
    SpmmTilePlanHost H;
    const int rc = build_spmm_tile_plan_host(nbrows, ptrow, indcol, per, ucap, spmm_tile_sort_rows(), H);
    if (refused) *refused = rc != 1;
    if (ntiles) *ntiles = H.ntiles;
    if (umax) *umax = H.umax;
    if (mean_list) *mean_list = H.mean_list;
    if (rc != 1) return MI_OK;
    CHECK_ARG(!wg_ptr || wg_ptr_cap >= (long long)H.wg_ptr.size(), "wg_ptr buffer too small");
    CHECK_ARG(!nodes || nodes_cap >= (long long)H.nodes.size(), "nodes buffer too small");
    CHECK_ARG(!slots || slots_cap >= (long long)H.slots.size(), "slots buffer too small");
    CHECK_ARG(!rows || rows_cap >= (long long)H.rows.size(), "rows buffer too small");
    if (wg_ptr) std::copy(H.wg_ptr.begin(), H.wg_ptr.end(), wg_ptr);
    if (nodes) std::copy(H.nodes.begin(), H.nodes.end(), nodes);
    if (slots) std::copy(H.slots.begin(), H.slots.end(), slots);
    if (rows) std::copy(H.rows.begin(), H.rows.end(), rows);
    return MI_OK;
}

static int build_spmm_tile(mi_bcsr4_t A)
{
    if (A->st_state) return A->st_state;
    A->st_state = -1;
    if (env_is("MI355_SPMM_TILE", "0") || A->nblocks < 4096) return -1;
    std::vector<int> ptrow((size_t)A->nbrows + 1), indcol((size_t)A->nblocks);
    if (hipMemcpy(ptrow.data(), A->d_ptrow, sizeof(int) * ptrow.size(), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(indcol.data(), A->d_indcol, sizeof(int) * indcol.size(), hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    // list caps: what lets two workgroups share a CU at four columns (128-row tiles: 368 x 144 B = 53 KB) and at eight (64-row tiles,
    // two quads per block row: 256 x 272 B = 70 KB); MI355_SPMM_TILE_UCAP=<128-row cap>,<64-row cap> for A/B
    int cap128 = 368, cap64 = 256;
    if (const char* ce = getenv("MI355_SPMM_TILE_UCAP")) (void)sscanf(ce, "%d,%d", &cap128, &cap64);
    A->st_state = build_spmm_tile_plan(A, 128, cap128, ptrow, indcol, A->st);
    (void)build_spmm_tile_plan(A, 64, cap64, ptrow, indcol, A->st64);
    return A->st_state;
}

static const SpmmTilePlan* spmm_plan_of(const mi_bcsr4_s* A, int s)
{
    if (s < 1 || s > 4) return nullptr;
    const SpmmTilePlan* Pl = A->st.d_ptr ? &A->st : nullptr;
    if (!Pl || spmm_tile_lds(Pl, s) > kLdsBytesPerCU) return nullptr;
    return Pl;
}

enum { kSpmmGather = 0, kSpmmTile = 1, kSpmmOct = 2, kSpmmOctNt = 3, kSpmmSell = 4, kSpmmForms = 5 };

static int sell_fill(mi_bcsr4_t A, hipStream_t s);

static bool spmm_form_possible(const mi_bcsr4_s* A, int s, int form, bool mapped = false)
{
    if (form == kSpmmGather) return true;
    // the sliced stream (spmm_bcsr4_sell): four or eight columns, unmapped products of a handle that holds the sliced copy
    if (form == kSpmmSell) return (s == 4 || s == 8) && A->sell.val; // (mapped products store through the block-row map)
    if (form == kSpmmTile) return spmm_plan_of(A, s) != nullptr;
    return s % 2 == 0 && A->st64.d_ptr && spmm_tile_lds(&A->st64, s) <= kLdsBytesPerCU;
}

static void launch_spmm_gather(const Bcsr4View& V, int m, int arith, const double* Xj, long long ldx, double* Yj, long long ldy, hipStream_t st)
{
    pick_int<1, 2, 3, 4, 5, 6, 7, 8>(m, [&](auto S) { launch_spmm_s<S()>(V, arith, Xj, ldx, Yj, ldy, st); });
}

static int launch_spmm(mi_bcsr4_t A, int s, int arith, const double* X, long long ldx, double* Y, long long ldy, hipStream_t st,
                       bool use_map)
{
    Bcsr4View V{A->nbrows, A->nbcols, A->d_ptrow, A->d_indcol, A->d_coef, use_map ? A->d_browmap : nullptr};
    for (int j0 = 0; j0 < s; j0 += 8) { // more than eight columns: batches of eight (the matrix is read once per batch)
        const int m = std::min(8, s - j0);
        const double* Xj = X + (size_t)j0 * ldx;
        double* Yj = Y + (size_t)j0 * ldy;
        // four forms, same bits: gather kernels; LDS tile with four lanes per block row (up to four columns); LDS tile with eight
        // lanes per block row (even column counts), coefficients loaded temporally or non-temporally.  The first product of a handle
        // at a column count times the possible ones and keeps the fastest (MI355_SPMM_TILE=0..3 forces a form)
        const bool mapped = V.browmap != nullptr;
        auto run = [&](int form) -> hipError_t {
            if (form == kSpmmSell) {
                SellView Sv{A->sell.val, A->sell.col, A->sell.sptr, A->sell.wrng, A->sell_nslices, A->nbrows, V.browmap};
                const int swg = A->sell_nwaves / 4;
                pick_int<4, 8>(m, [&](auto M) {
                    pick([&](auto CHAIN) { hipLaunchKernelGGL((spmm_bcsr4_sell<M(), CHAIN() ? 0 : 1, 6, true>), dim3((unsigned)swg), dim3(256), 0, st, Sv, Xj, ldx, Yj, ldy, swg); },
                         arith == MI_ARITH_CHAIN);
                });
                return hipGetLastError();
            }
            if (form == kSpmmTile) return spmm_tile_launch(A, spmm_plan_of(A, m), V, m, arith, Xj, ldx, Yj, ldy, st);
            if (form == kSpmmOct || form == kSpmmOctNt) return spmm_otile_launch(A, &A->st64, V, m, arith, form == kSpmmOctNt, Xj, ldx, Yj, ldy, st);
            launch_spmm_gather(V, m, arith, Xj, ldx, Yj, ldy, st);
            return hipGetLastError();
        };
        int form = kSpmmGather;
        const bool capturing = stream_is_capturing(st); // no first-use measurement (it synchronises) and no plan upload under capture
        if (capturing && A->spmm_choice[m] > 0 && (A->st_state == 1 || A->spmm_choice[m] - 1 == kSpmmSell) &&
            !(A->spmm_choice[m] - 1 == kSpmmSell && mapped))
            form = A->spmm_choice[m] - 1;
        const bool tiles = !capturing && build_spmm_tile(A) == 1;
        if (!capturing && (tiles || spmm_form_possible(A, m, kSpmmSell, mapped))) {
            const char* e = getenv("MI355_SPMM_TILE");
            const int forced = e ? atoi(e) : -1;
            auto possible = [&](int f) { return (f == kSpmmGather || f == kSpmmSell || tiles) && spmm_form_possible(A, m, f, mapped); };
            if (forced >= 0 && forced < kSpmmForms) form = possible(forced) ? forced : kSpmmGather;
            else {
                if (A->spmm_choice[m] == 0) {
                    int best = kSpmmGather;
                    LaunchTimer tm(st);
                    if (tm.init() == MI_OK) {
                        double us[kSpmmForms] = {0, 0, 0, 0, 0};
                        bool ok = true;
                        for (int round = 0; round < 2 && ok; round++)
                            for (int f = 0; f < kSpmmForms && ok; f++) {
                                if (!possible(f)) continue;
                                double t = 0.0;
                                ok = tm.time(2, 5, [&] { return run(f) == hipSuccess ? MI_OK : MI_ERR_HIP; }, &t) == MI_OK;
                                if (ok) us[f] = min_measured(us[f], t);
                            }
                        for (int f = 0; f < kSpmmForms; f++) {
                            A->spmm_us[m][f] = us[f];
                            if (ok && us[f] > 0 && us[f] < us[best]) best = f;
                        }
                        if (!ok) { (void)hipGetLastError(); best = kSpmmGather; }
                    }
                    A->spmm_choice[m] = 1 + best;
                }
                form = A->spmm_choice[m] - 1;
                if (!possible(form)) form = kSpmmGather; // (e.g. the measured choice was the sliced form and this product is a mapped one)
            }
        }
        hipError_t er = run(form);
        if (er != hipSuccess) return fail(MI_ERR_HIP, std::string("multi-vector product: ") + hipGetErrorString(er));
    }
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

extern "C" int mi_bcsr4_spmm_info(mi_bcsr4_t A, int s, int* tile_built, int* form_in_use, int* longest_list, double us[5])
{
    CHECK_ARG(A && s >= 1 && s <= 8, "bad argument");
    if (tile_built) *tile_built = A->st_state == 1;
    if (form_in_use) {
        const char* e = getenv("MI355_SPMM_TILE");
        const int forced = e ? atoi(e) : -1;
        int form = kSpmmGather;
        if (A->st_state == 1 || spmm_form_possible(A, s, kSpmmSell)) {
            auto possible = [&](int f) { return (f == kSpmmGather || f == kSpmmSell || A->st_state == 1) && spmm_form_possible(A, s, f); };
            if (forced >= 0 && forced < kSpmmForms) form = possible(forced) ? forced : kSpmmGather;
            else if (A->spmm_choice[s] > 0) form = A->spmm_choice[s] - 1;
        }
        *form_in_use = form;
    }
    if (longest_list) {
        const SpmmTilePlan* Pl = spmm_plan_of(A, s) ? spmm_plan_of(A, s) : (A->st64.d_ptr ? &A->st64 : nullptr);
        *longest_list = Pl ? Pl->umax : 0;
    }
    if (us)
        for (int f = 0; f < kSpmmForms; f++) us[f] = A->spmm_us[s][f];
    return MI_OK;
}


extern "C" int mi_bcsr4_spmm_dev(mi_bcsr4_t A, int s, const double* d_X, long long ldx, double* d_Y, long long ldy, int arith,
                                 mi_stream_t st)
{
    CHECK_ARG(A, "null handle");
    CHECK_ARG(s >= 0, "negative column count");
    CHECK_ARG(arith == MI_ARITH_CHAIN || arith == MI_ARITH_BLOCKACC, "unknown arithmetic id");
    if (s == 0 || A->nbrows == 0) return MI_OK;
    CHECK_ARG(d_X && d_Y, "null matrix");
    CHECK_ARG(ldx >= 4LL * A->nbcols && ldy >= 4LL * A->nbrows, "leading dimension shorter than a column");
    CHECK_ARG((((uintptr_t)d_X) & 15) == 0 && (ldx & 1) == 0, "X columns must be 16-byte aligned (even ldx)");
    return launch_spmm(A, s, arith, d_X, ldx, d_Y, ldy, (hipStream_t)st, true);
}

extern "C" int mi_bcsr4_spmm(mi_bcsr4_t A, int s, const double* X, long long ldx, double* Y, long long ldy, int arith)
{
    CHECK_ARG(A, "null handle");
    CHECK_ARG(s >= 0, "negative column count");
    if (s == 0 || A->nbrows == 0) return MI_OK;
    CHECK_ARG(X && Y, "null matrix");
    CHECK_ARG(ldx >= 4LL * A->nbcols && ldy >= 4LL * A->nbrows, "leading dimension shorter than a column");
    int rc = need_device();
    if (rc) return rc;
    Scratch S;
    double *dX = nullptr, *dY = nullptr;
    const size_t nx = 4 * (size_t)A->nbcols, ny = 4 * (size_t)A->nbrows;
    if ((rc = S.up(nullptr, nx * s, &dX)) || (rc = S.up(nullptr, ny * s, &dY))) return rc;
    for (int j = 0; j < s; j++) HIP_TRY(hipMemcpy(dX + nx * j, X + (size_t)ldx * j, sizeof(double) * nx, hipMemcpyHostToDevice));
    if ((rc = mi_bcsr4_spmm_dev(A, s, dX, (long long)nx, dY, (long long)ny, arith, nullptr))) return rc;
    for (int j = 0; j < s; j++) HIP_TRY(hipMemcpy(Y + (size_t)ldy * j, dY + ny * j, sizeof(double) * ny, hipMemcpyDeviceToHost));
    return MI_OK;
}

// CSR handle: through the blocked copy when the matrix has one (matrix read once for all columns; a BCSR chain visits
// the CSR row's terms in CSR order, so every column carries the bits of SpMV_CSR_FMA), else column by column.
extern "C" int mi_spmm_dev(mi_csr_t A, int s, const double* d_X, long long ldx, double* d_Y, long long ldy, mi_stream_t st_)
{
    CHECK_ARG(A, "null handle");
    CHECK_ARG(s >= 0, "negative column count");
    CHECK_ARG(!A->mapped, "multi-vector products need an unmapped matrix");
    if (s == 0 || A->n == 0) return MI_OK;
    CHECK_ARG(d_X && d_Y, "null matrix");
    CHECK_ARG(ldx >= A->ncols && ldy >= A->n, "leading dimension shorter than a column");
    hipStream_t st = (hipStream_t)st_;
    const bool aligned = (((uintptr_t)d_X) & 15) == 0 && (ldx & 1) == 0;
    if (A->inner && A->inner->blocked && aligned) { // reordered: gather the s columns into the new numbering first
        const size_t n = (size_t)A->n;
        double* Xp = nullptr; // the gathered columns as one dense block, stream-ordered allocation
        HIP_TRY(hipMallocAsync((void**)&Xp, sizeof(double) * n * s, st));
        int rc = MI_OK;
        for (int j = 0; j < s && !rc; j++) rc = gather_perm(A, d_X + (size_t)j * ldx, Xp + n * j, st);
        if (!rc) rc = launch_spmm(A->inner->blocked, s, MI_ARITH_CHAIN, Xp, (long long)n, d_Y, ldy, st, true);
        (void)hipFreeAsync(Xp, st);
        return rc;
    }
    if (!A->inner && A->blocked && aligned) return launch_spmm(A->blocked, s, MI_ARITH_CHAIN, d_X, ldx, d_Y, ldy, st, true);
    for (int j = 0; j < s; j++) {
        int rc = launch_spmv(A, d_X + (size_t)j * ldx, d_Y + (size_t)j * ldy, st);
        if (rc) return rc;
    }
    return MI_OK;
}

// V[:, 0] = v0, V[:, k+1] = A V[:, k] for k < s: BuildKrylovBasis_AVX2, src/kernels/spmm_avx2.c:112-168 (a dense n x (s+1)
// column-major V, each new column one product) — that is orth == 0, the monomial basis, bit-equal to the matrix-powers
// chain.  orth != 0 builds the ORTHONORMAL (Arnoldi) basis an s-step GMRES needs out of the reference's own pieces:
// V[:, 0] = v0 / ||v0||; each product is passed through orthonormalize_against_basis (mpk/2SpMV.cpp:13-28) against the
// columns before it and then divided by its norm2 (mpk/utils.cpp:131-136) — the normalisation that helper computes and
// drops (:23-26), without which its projections y -= (y.v) v are only meaningful for unit v.  Coefficients (the Hessenberg
// column of step k) go to d_coef[k * (s + 2) + j]: j <= k the dots in the order taken, j = k + 1 the norm;
// d_coef[s * (s + 2)] = ||v0||.  d_coef: s * (s + 2) + 1 doubles.
extern "C" int mi_krylov_basis_dev(mi_csr_t A, int s, const double* d_v0, double* d_V, long long ldv, int orth, double* d_coef,
                                   mi_stream_t st_)
{
    CHECK_ARG(A, "null handle");
    CHECK_ARG(s >= 0 && s <= 64, "s must be in 0..64");
    CHECK_ARG(A->n == A->ncols && !A->mapped, "a Krylov basis needs a square, unmapped matrix");
    if (A->n == 0) return MI_OK;
    CHECK_ARG(d_v0 && d_V && ldv >= A->n, "bad argument");
    CHECK_ARG(!orth || d_coef, "null coefficient array");
    hipStream_t st = (hipStream_t)st_;
    const int n = A->n;
    const int grid = launch_grid(n, 256, 2048);
    int rc;
    if (d_V != d_v0) HIP_TRY(hipMemcpyAsync(d_V, d_v0, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
    if (orth) {
        double* nrm0 = d_coef + (size_t)s * (s + 2);
        if ((rc = mi_norm2_dev(n, d_V, nrm0, st))) return rc;
        hipLaunchKernelGGL(div_by_scalar_kernel, dim3(grid), dim3(256), 0, st, n, nrm0, d_V);
    }
    std::vector<const double*> cols;
    for (int k = 0; k < s; k++) {
        double* next = d_V + (size_t)(k + 1) * ldv;
        if ((rc = launch_spmv(A, d_V + (size_t)k * ldv, next, st))) return rc;
        if (orth) {
            double* h = d_coef + (size_t)k * (s + 2);
            cols.push_back(d_V + (size_t)k * ldv);
            if ((rc = mi_orthonormalize_against_basis_dev(n, (int)cols.size(), cols.data(), next, h, st))) return rc;
            if ((rc = mi_norm2_dev(n, next, h + k + 1, st))) return rc;
            hipLaunchKernelGGL(div_by_scalar_kernel, dim3(grid), dim3(256), 0, st, n, h + k + 1, next);
        }
    }
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

// mi_krylov_basis_dev's orthonormal basis with classical Gram-Schmidt (mi_cgs_dev: VecMDot + VecMAXPY, src/solve_newton.c:1265)
// in place of the sequential sweep: step k is one product, `passes` x (all k + 1 dots against the same vector, one update), the
// norm out of the last update, one division — 3 * passes + 2 launches whatever k.  passes = 2 (CGS2) keeps V orthonormal to a
// few ulps where the sweep and a single pass lose it.  The same V and d_coef layout as mi_krylov_basis_dev;
// entry [k * (s + 2) + j] is the sum of the two passes' dots.
extern "C" int mi_krylov_basis_cgs_dev(mi_csr_t A, int s, const double* d_v0, double* d_V, long long ldv, int passes, double* d_coef,
                                       mi_stream_t st_)
{
    CHECK_ARG(A, "null handle");
    CHECK_ARG(s >= 0 && s <= 64, "s must be in 0..64");
    CHECK_ARG(passes == 1 || passes == 2, "passes must be 1 or 2");
    CHECK_ARG(A->n == A->ncols && !A->mapped, "a Krylov basis needs a square, unmapped matrix");
    if (A->n == 0) return MI_OK;
    CHECK_ARG(d_v0 && d_V && d_coef && ldv >= A->n, "bad argument");
    hipStream_t st = (hipStream_t)st_;
    const int n = A->n;
    const int grid = launch_grid(n, 256, 2048);
    int rc;
    if (d_V != d_v0) HIP_TRY(hipMemcpyAsync(d_V, d_v0, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
    double* nrm0 = d_coef + (size_t)s * (s + 2);
    if ((rc = mi_norm2_dev(n, d_V, nrm0, st))) return rc;
    hipLaunchKernelGGL(div_by_scalar_kernel, dim3(grid), dim3(256), 0, st, n, nrm0, d_V);
    std::vector<const double*> cols;
    for (int k = 0; k < s; k++) {
        double* next = d_V + (size_t)(k + 1) * ldv;
        double* h = d_coef + (size_t)k * (s + 2);
        if ((rc = launch_spmv(A, d_V + (size_t)k * ldv, next, st))) return rc;
        cols.push_back(d_V + (size_t)k * ldv);
        if ((rc = mi_cgs_dev(n, (int)cols.size(), cols.data(), next, passes, h, h + k + 1, st))) return rc;
        hipLaunchKernelGGL(div_by_scalar_kernel, dim3(grid), dim3(256), 0, st, n, h + k + 1, next);
    }
    HIP_TRY(hipGetLastError());
    return MI_OK;
}
