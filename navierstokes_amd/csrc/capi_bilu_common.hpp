// capi_bilu_common.hpp — what a block ILU handle (capi_ilu.hip, mi_bilu4_*) and a block DILU handle (capi_dilu.hip, mi_dilu4_*) have in
// common, each rule ONCE; those two files include it and nothing else does.  Both preconditioners are triangular sweeps over the
// level schedule of bilu4_plan.hpp on a pattern that bilu4_order.hpp may have renumbered, so they share: the argument rules of a
// create, the host part of the handle (ordering, pattern, schedule), the level-major device copy of the two triangles and how
// values move into it, the guard of a device entry point, the steps of a refactor, and the bracket that takes a call on an
// ordered handle through the handle's own vectors.  What a family computes, its kernels and its launchers stay in its own file.
#pragma once
#include "capi_internal.hpp"
#include "bilu4_plan.hpp"
#include "bilu4_order.hpp"
#include "bilu4_order_kernels.hpp"

#include <thread>

// ---------------------------------------------------------------- ownership
// Every device array of the two files is a DevArray (dev_array.hpp, the type all handles of the library own their device memory
// with): member destructors are the only release path.  Both floor every allocation at ONE entry (an empty level or list still gets
// an address the kernels may be handed), which the shared type leaves to the caller: hence the 1s.

// the level-major copy of one sweep's off-diagonal blocks (bilu4_solve.hpp)
struct Bilu4DevSweep {
    DevArray<int> perm, ptr, col;
    DevArray<double> val, dinv; // dinv: the ILU's backward sweep only (allocated by capi_ilu.hip)
    DevArray<int> lev_ptr;
    std::vector<long long> src; // per device block: its place in the host copy of the values (they move through it, both ways)
    size_t blocks() const { return src.size(); }
};

// the host part of a handle and the device tables every sweep reads; mi_bilu4_s and mi_dilu4_s derive from it
struct Bilu4Handle {
    int device = -1;               // -1: host-only handle (mi_*_create_host)
    Bilu4Order ord;                // the ordering behind the handle (natural: empty tables)
    std::vector<int> a_ptr, a_col; // the pattern the schedule is made on: the caller's, or on an ordered handle that of the
                                   // permuted matrix, whose blocks ord.src maps back to the caller's
    Bilu4Schedule sched;
    double factor_seconds = 0.0;   // host time of the last numeric factorisation
    Bilu4DevSweep lev[2];          // forward, backward
    DevArray<int> d_perm;          // ordered: [nb] the caller's block row -> the handle's
    const Bilu4Pattern& pat() const { return sched.pat; }
};

static int bilu_threads()
{
    const char* e = getenv("MI355_BILU_THREADS");
    if (e && atoi(e) > 0) return atoi(e);
    const unsigned hw = std::thread::hardware_concurrency();
    return (int)std::max(1u, std::min(hw, 16u));
}

// ---------------------------------------------------------------- arguments
static const char* bilu_bad_layout(int layout) { return layout == MI_BLOCK_ROWMAJOR || layout == MI_BLOCK_COLMAJOR ? nullptr : "unknown block layout"; }

static const char* bilu_bad_ordering(int ordering)
{
    return ordering == MI_BILU_ORDER_NATURAL || ordering == MI_BILU_ORDER_COLOUR ? nullptr : "unknown ordering (0: natural, 1: multicolour)";
}

// a square block pattern and a fill; prefix: the family's, in front of what bilu4_check_pattern refuses ("mi_bilu4: ", "mi_dilu4: ")
static int bilu_check_args(const char* prefix, int nbrows, const int* ptrow, const int* indcol, int fill)
{
    CHECK_ARG(nbrows >= 0, "negative nbrows");
    CHECK_ARG(fill >= 0, "fill must be >= 0");
    if (nbrows == 0) return MI_OK;
    CHECK_ARG(ptrow, "null ptrow");
    CHECK_ARG(ptrow[nbrows] <= 0 || indcol, "null indcol");
    const std::string why = bilu4_check_pattern(nbrows, ptrow, indcol);
    if (!why.empty()) return fail(MI_ERR_ARG, prefix + why);
    return MI_OK;
}

// what a create is given, in the order it is checked — before anything is allocated; *out is null from the first check on
template <class H>
static int bilu_check_create(const char* prefix, int nbrows, const int* ptrow, const int* indcol, const double* coef, int layout, int fill, int ordering, H** out)
{
    CHECK_ARG(out, "null output handle");
    *out = nullptr;
    CHECK_ARG(!bilu_bad_layout(layout), bilu_bad_layout(layout));
    CHECK_ARG(!bilu_bad_ordering(ordering), bilu_bad_ordering(ordering));
    if (const int rc = bilu_check_args(prefix, nbrows, ptrow, indcol, fill)) return rc;
    CHECK_ARG(nbrows == 0 || coef, "null coef");
    return MI_OK;
}

// What the device entry points begin with: MI_ERR_ARG without a handle or with a bad argument (bad_arg: what is wrong with the
// arguments that are checked even on an empty matrix; bad_data: with those that are not), MI_OK at once on an empty matrix,
// host_only's status on a host-only handle.  kBiluGo: none of these, go on.
constexpr int kBiluGo = -1;

// what a host-only handle gets: a status, and the text behind the entry point's name
struct BiluHostOnly {
    int status;
    const char* tail;
};

static int bilu_guard(const Bilu4Handle* H, const char* name, const BiluHostOnly& host_only, const char* bad_arg = nullptr, const char* bad_data = nullptr)
{
    CHECK_ARG(H, "null handle");
    CHECK_ARG(!bad_arg, bad_arg);
    if (H->pat().nb == 0) return MI_OK;
    CHECK_ARG(!bad_data, bad_data);
    if (H->device < 0) return fail(host_only.status, std::string(name) + host_only.tail);
    return kBiluGo;
}

// ---------------------------------------------------------------- the host part of a handle
// the ordering of a pattern that bilu_check_args has accepted, checked (bilu4_order_check) before anything relies on it
static int bilu_order(int nbrows, const int* ptrow, const int* indcol, int ordering, const char* who, Bilu4Order* O)
{
    *O = Bilu4Order{};
    if (ordering == MI_BILU_ORDER_NATURAL) return MI_OK;
    bilu4_colour(nbrows, ptrow, indcol, O);
    const std::string bad = bilu4_order_check(nbrows, ptrow, indcol, *O);
    if (!bad.empty()) return fail(MI_ERR_STATE, std::string(who) + ": " + bad);
    return MI_OK;
}

// ordering, pattern and schedule of a new handle from arguments that bilu_check_create has accepted; who: the entry point, for the
// message of an ordering that fails its check
static int bilu_plan_host(Bilu4Handle* H, int nbrows, const int* ptrow, const int* indcol, int fill, int ordering, const char* who)
{
    if (nbrows == 0) {
        H->ord.ordering = ordering; // (an empty matrix: no tables, but the handle says what it was asked for)
        H->a_ptr.assign(1, 0);
    } else if (ordering != MI_BILU_ORDER_NATURAL) {
        if (const int rc = bilu_order(nbrows, ptrow, indcol, ordering, who, &H->ord)) return rc;
        bilu4_permute_pattern(nbrows, ptrow, indcol, &H->ord, &H->a_ptr, &H->a_col);
    } else {
        H->a_ptr.assign(ptrow, ptrow + nbrows + 1);
        H->a_col.assign(indcol, indcol + ptrow[nbrows]);
    }
    bilu4_schedule(nbrows, H->a_ptr.data(), H->a_col.data(), fill, &H->sched);
    return MI_OK;
}

// ---------------------------------------------------------------- the level-major device copy
// the level-major copy of both sweeps: their pattern, and room for their off-diagonal values
static int bilu_upload_pattern(Bilu4Handle* H)
{
    const Bilu4Pattern& P = H->pat();
    for (int b = 0; b < 2; b++) {
        const Bilu4Sweep& S = H->sched.sweep[b];
        Bilu4DevSweep& D = H->lev[b];
        std::vector<int> ptr(P.nb + 1, 0), col;
        D.src.clear();
        for (int q = 0; q < P.nb; q++) {
            const auto [k0, k1] = P.offdiag(S.perm[q], b == 1);
            for (int k = k0; k < k1; k++) {
                col.push_back(P.col[k]);
                D.src.push_back(k);
            }
            ptr[q + 1] = (int)col.size();
        }
        int rc;
        if ((rc = dev_upload(D.perm, S.perm, 1)) || (rc = dev_upload(D.ptr, ptr, 1)) || (rc = dev_upload(D.col, col, 1)) ||
            (rc = dev_alloc(D.val, 16 * std::max<size_t>(col.size(), 1))) || (rc = dev_upload(D.lev_ptr, S.lev_ptr, 1)))
            return rc;
    }
    return MI_OK;
}

// n blocks between a device array and a host array of blocks, block k of the device array at host_block(k) of the host array, to
// the device or back; v: scratch that one call after another may share
template <class Map>
static int bilu_move_blocks(double* dev, size_t n, double* host, Map&& host_block, bool to_device, std::vector<double>& v)
{
    if (!n) return MI_OK;
    v.resize(16 * n);
    if (!to_device) HIP_TRY(hipMemcpy(v.data(), dev, sizeof(double) * v.size(), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < n; k++) {
        double *h = &host[16 * (size_t)host_block(k)], *d = &v[16 * k];
        memcpy(to_device ? d : h, to_device ? h : d, sizeof(double) * 16);
    }
    if (to_device) HIP_TRY(hipMemcpy(dev, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice));
    return MI_OK;
}

// the off-diagonal values between the host array (the pattern's block order) and the two level-major device arrays, through src
static int bilu_move_offdiag(const Bilu4Handle* H, double* host, bool to_device)
{
    std::vector<double> v;
    for (const Bilu4DevSweep& D : H->lev)
        if (const int rc = bilu_move_blocks(D.val, D.blocks(), host, [&](size_t k) { return D.src[k]; }, to_device, v)) return rc;
    return MI_OK;
}

// ---------------------------------------------------------------- refactor
// mi_*_refactor: the argument rules, the family's host numerics (factor), and on a device handle its upload — work already enqueued
// reads the old values: wait for it, then replace (a Newton step refactors between solves)
template <class Factor, class Upload>
static int bilu_refactor(const Bilu4Handle* H, const double* coef, int layout, Factor&& factor, Upload&& upload)
{
    CHECK_ARG(H, "null handle");
    CHECK_ARG(!bilu_bad_layout(layout), bilu_bad_layout(layout));
    if (H->pat().nb == 0) return MI_OK;
    CHECK_ARG(coef, "null coef");
    if (const int rc = factor()) return rc;
    if (H->device < 0) return MI_OK;
    HIP_TRY(hipDeviceSynchronize());
    return upload();
}

// ---------------------------------------------------------------- ordered handles
// THE ONE PLACE an ordering meets the caller's vectors: whatever a family applies runs as inner(in, out) on vectors in the handle's
// numbering.  Natural order: the caller's own.  Ordered: the handle's vectors own_in and own_out (which may be one), with a gather
// in front and a scatter behind, on the same stream — two launches, nothing allocated or synchronised.  d_out may be d_in: the
// gather has read all of it before the scatter writes.
constexpr int kBiluOrderLaunches = 2;

// the kernels' AL: x may be read and written as 16-byte pairs
template <class Fn>
static auto bilu_by_alignment(const double* d_x, Fn&& fn)
{
    return pick(fn, (((uintptr_t)d_x) & 15) == 0);
}

template <bool IN>
static void bilu_order_move(const Bilu4Handle* H, const double* from, double* to, const double* user, hipStream_t s)
{
    const int nb = H->pat().nb;
    bilu_by_alignment(user, [&](auto al) {
        constexpr bool AL = decltype(al)::value;
        const int grid = launch_grid((long long)nb * kBiluOrderLanes<AL>, kWG, INT_MAX, 1);
        hipLaunchKernelGGL((bilu4_order_move<IN, AL>), dim3(grid), dim3(kWG), 0, s, H->d_perm, nb, from, to);
        return 0;
    });
}

template <class Fn>
static int bilu_in_order(const Bilu4Handle* H, const double* d_in, double* d_out, double* own_in, double* own_out, hipStream_t s, Fn&& inner)
{
    if (!H->ord.on()) return inner(d_in, d_out);
    bilu_order_move<true>(H, d_in, own_in, d_in, s);
    if (const int rc = inner((const double*)own_in, own_out)) return rc;
    bilu_order_move<false>(H, own_out, d_out, d_out, s);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}
