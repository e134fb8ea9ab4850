// capi_csr.hip: CSR handles — create (plans, autotuner, relabelling), update, info, products — part of libmi355spmv.so (see capi_internal.hpp for the layout of the library).
// Built for gfx950 only; no CPU fallback anywhere: every compute entry point needs a HIP device.
#include "capi_internal.hpp"
#include "reorder.hpp"
#include "mring_plan.hpp"
#include "tile_plan.hpp"
#include "rowblock_census.hpp"

// ---------------------------------------------------------------- CSR create
int get_table(mi_csr_t A, int nnzb, BlockTable** out)
{
    auto it = A->tables.find(nnzb);
    if (it == A->tables.end()) {
        std::vector<int> rows, ptrs;
        // the row-alignment rule of partition.hpp (row_block_align); MI355_STREAM_ROW_ALIGN=1|64 forces (A/B)
        int row_align = row_block_align(A->nnz);
        if (const char* e = getenv("MI355_STREAM_ROW_ALIGN")) row_align = std::max(1, atoi(e));
        build_row_blocks(A->n, A->h_ptrow.data(), nnzb, 4 * kWG, rows, ptrs, row_align, kRowBlockKeepEighths);
        BlockTable T;
        T.nnzb = nnzb;
        T.nblk = (int)rows.size() - 1;
        T.row_align = row_align;
        std::vector<int2> h(rows.size());
        for (size_t i = 0; i < rows.size(); i++) h[i] = make_int2(rows[i], ptrs[i]);
        HIP_TRY(T.d_blk.upload(h));
        it = A->tables.emplace(nnzb, std::move(T)).first; // (only a table that was filled: a failed upload leaves none behind)
    }
    *out = &it->second;
    return MI_OK;
}

// the matrix stream (bytes_per_nnz per nonzero) and two vectors no longer fit the 256 MB Infinity Cache with room to spare: stream past it
static inline bool beyond_infinity_cache(double bytes_per_nnz, long long nnz, int n) { return bytes_per_nnz * (double)nnz + 16.0 * (double)n > 0.75 * 256e6; }

constexpr double kSsMaxPadding = 0.12; // padded places per nonzero from which the sliced copy is not worth its bytes
// MI355_SSTREAM_MAX_PADDING=<places per nonzero> (tests: the reference-made goldens — a few hundred ragged rows — through the sliced kernels)
static double ss_max_padding()
{
    if (const char* e = getenv("MI355_SSTREAM_MAX_PADDING")) return std::max(0.0, atof(e));
    return kSsMaxPadding;
}

// The sliced copy of the sliced-stream kernel (spmv_sstream.hpp): plan + slot stream on the host, values filled on the device from the
// handle's CSR values (already uploaded).  MI_OK with A->ss left empty when the matrix is not eligible.
// A handle whose rows go to y[r + odd offset] (the interior rows of a rank) is planned one row down: its row pairs then start on
// even rows of y and leave as 16-byte stores like any other's.  ghost_lo < ghost_hi: a combined piece of the fused multi-GPU step.
static int build_sstream(mi_csr_t A, const int* ptrow, const int* indcol, int ghost_lo = 0, int ghost_hi = 0)
{
    if (A->ss.dev.val) return MI_OK;
    SsPlanHost P;
    SsMwPlanHost M;
    const int shift = (A->y_offset & 1) && !A->d_rowmap ? 1 : 0;
    build_sstream_plan(A->n, A->ncols, ptrow, indcol, ss_max_padding(), P, true, shift, ghost_lo, ghost_hi);
    SstreamCopy T;
    hipError_t e;
    if (!P.eligible) {
        // rows that name several column neighbourhoods (3-D mesh operators in natural order): the cut-ring form (spmv_sstream_mw.hpp).
        // Not for a combined piece with ghost columns (the fused step has no such form).  MI355_SSTREAM_MW=0: never.
        if (ghost_lo < ghost_hi || env_is("MI355_SSTREAM_MW", "0")) return MI_OK;
        build_sstream_mw_plan(A->n, A->ncols, ptrow, indcol, ss_max_padding(), M, shift);
        if (!M.eligible) return MI_OK;
        e = ss_mw_upload(M, T.dev);
        T.mw = e == hipSuccess;
    } else e = ss_upload(P, T.dev, ghost_lo < ghost_hi);
    const SsPlanHost& Q = P.eligible ? P : M; // (the tables both forms share: rounds, steps, slices)
    if (e != hipSuccess) {
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return MI_OK; } // no room for a second copy of the matrix: the other kernels serve it
        return fail(MI_ERR_HIP, std::string("sliced copy: ") + hipGetErrorString(e));
    }
    T.nwg = Q.nwg;
    T.rounds = Q.rounds;
    T.shift = Q.shift;
    T.steps = Q.steps;
    T.padding = (double)Q.pad_places / (double)A->nnz;
    T.max_slice_nnz = Q.max_slice_nnz;
    if (ghost_lo < ghost_hi) {
        T.h_wg_halo = P.wg_halo;
        T.h_wg = P.wg;
        T.fusable = P.fusable;
    }
    // the sliced values are filled HERE and refilled where the CSR values change (mi_csr_update_values*), on that call's stream — never
    // lazily in front of a product: a product captured into a HIP graph holds only the product's node and must find the values in place
    sstream_fill_values(T.rounds, A->n, T.shift, A->d_ptrow, A->d_coef, nullptr, T.dev.slice_step, T.dev.slice_len, T.dev.val, T.max_slice_nnz, nullptr, T.mw ? 1 : 0);
    if ((e = hipGetLastError()) != hipSuccess) {
        T = {};
        return fail(MI_ERR_HIP, std::string("sliced copy fill: ") + hipGetErrorString(e));
    }
    T.nt = beyond_infinity_cache(10.0, A->nnz, A->n);
    T.deep = T.nt;
    if (const char* fe = getenv("MI355_SSTREAM_FORM")) { // tests: one variant (0 D=8 nt, 1 D=8 temporal, 2 D=12 nt, 3 D=12 temporal)
        const int f = atoi(fe);
        T.nt = (f & 1) == 0;
        T.deep = f >= 2;
    }
    A->ss.copy() = std::move(T);
    return MI_OK;
}

// y = A x through the sliced-stream kernel (the caller has checked sstream_y_ok); rowmap: nullptr or the handle's row map
int launch_sstream(mi_csr_t A, const double* d_x, double* d_y, const int* rowmap, hipStream_t s, const RingComm* comm)
{
    SstreamTable& T = A->ss;
    SsView S{T.dev.val, T.dev.slot, T.dev.wg, T.dev.win, T.nwg, A->n + T.shift, A->ncols, rowmap, T.shift};
    double* yy = rowmap ? d_y : d_y - T.shift;
    if (T.mw) {
        if (comm) return fail(MI_ERR_STATE, "the cut-ring sliced stream has no fused multi-GPU form");
        SsMwView V{S, T.dev.winK};
        pick([&](auto DEEP, auto NT) { hipLaunchKernelGGL((spmv_sstream_mw<DEEP() ? 12 : 8, NT()>), dim3((unsigned)T.nwg), dim3(256), 0, s, V, d_x, yy); }, T.deep, T.nt);
        HIP_TRY(hipGetLastError());
        return MI_OK;
    }
    pick([&](auto DEEP, auto NT) {
        constexpr int DEPTH = DEEP() ? 12 : 8;
        if (comm) hipLaunchKernelGGL((spmv_sstream_fused<DEPTH, NT()>), dim3((unsigned)(T.nwg + comm->push_wgs)), dim3(256), 0, s, S, d_x, yy, *comm);
        else hipLaunchKernelGGL((spmv_sstream<DEPTH, NT()>), dim3((unsigned)T.nwg), dim3(256), 0, s, S, d_x, yy);
    }, T.deep, T.nt);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

// Plan of the multi-window ring kernel (host arrays of the caller, or nullptr: the handle's device copy is read back)
// Block shape of the ring / multi-window ring plans by matrix size (row_align argument of the planners; 0 = their default of 64).
// Whole waves of rows per block pay below ~20 M nonzeros (2-5 % on every box tried).  Beyond, their rate turned out to depend on
// WHERE THE CALLER'S x AND y lie in device memory — 133 / 144 / 153 us for three x / y pairs on one and the same C4 handle, and
// 149-154 us for sixteen pairs in another process — while blocks cut at the nonzero count alone run 138-146 us whatever the
// vectors (tools/state_probe.py, state_probe2.py; profiles/r03_state_probe.txt): their 1088-byte steps through y, x and the
// row pointers keep the 512 workgroups' streams out of phase with each other, the whole-wave plan's 1 KiB steps do not.  The
// create-time comparison of the two (rounds 2-3) timed them on the library's own scratch vectors and so could not tell what the
// caller would see; large matrices now take the unaligned blocks outright.
// Staging layout of the ring kernels' row chains (SKEW template argument): one pad slot per 32 staged nonzeros, or none.  A row
// chain reads its terms as 16-byte {coef, x} pairs (ring_stage_cx), lane l starting 16 * (length of the rows in front) bytes into the
// staging area: rows whose length is a multiple of 16 put every lane of a wave on the same four banks (16-way conflicts: uniform
// rows of 16 run 134-139 us plain and 92-102 us padded, rows of 32 132-136 against 107.5, rows of 8 89 against 79-85), and the pad
// slot breaks that up — at the price of index arithmetic per term, which is why every other shape is faster WITHOUT it: S15 140.5
// against 147.5 us, SVAR (lengths 8..22 mixed) 147 against 159-163, rows of 24 96.7 against 103.5, the FE shape (rows of 56) 162.6
// against 201.  (Measured with the merged staging of round 3's second session, tools/skew_ab.py; the two-array staging of
// rounds 1-2 wanted the pad for every multiple of 8.)  Mixed lengths do not line up whatever their share, so the rule asks for a
// MAJORITY of such rows.
static bool ring_wants_skew(int n, const int* ptrow)
{
    long long bad = 0;
    for (int i = 0; i < n; i++) {
        const int len = ptrow[i + 1] - ptrow[i];
        bad += len > 0 && (len % 16 == 0 || len == 8);
    }
    return 2 * bad > n;
}

constexpr long long kLargeNnz = 20000000;
// doubles in a vector handed out by mi_vec_alloc_placed (64 of slack: the kernels' clamped loads stay inside)
static size_t placed_vector_len(int n, int ncols) { return (size_t)std::max(n, ncols) + 64; }
static int large_row_align(long long nnz) { return nnz >= kLargeNnz ? 1 : 0; }

static int build_mring(mi_csr_t A, const int* indcol, int row_align = 0)
{
    if (A->mring.d_plan || A->n == 0 || A->nnz == 0) return MI_OK;
    std::vector<int> back;
    if (!indcol) {
        if (!A->d_indcol) return fail(MI_ERR_STATE, "mring plan: the handle no longer holds its column indices");
        back.resize((size_t)A->nnz);
        HIP_TRY(hipMemcpy(back.data(), A->d_indcol, sizeof(int) * (size_t)A->nnz, hipMemcpyDeviceToHost));
        indcol = back.data();
    }
    MringPlanHost P;
    build_mring_plan(A->n, A->h_ptrow.data(), indcol, P, row_align);
    MringTable M;
    HIP_TRY(M.d_plan.alloc(P.plan.size()));
    HIP_TRY(M.d_first.upload(P.first));
    HIP_TRY(M.d_ok.alloc(P.run_ok.size()));
    HIP_TRY(M.d_rng.alloc(P.run_rng.size()));
    HIP_TRY(M.d_slots.alloc(P.slots.size()));
    HIP_TRY(M.d_plan.fill(P.plan));
    HIP_TRY(M.d_ok.fill(P.run_ok));
    HIP_TRY(M.d_rng.fill(P.run_rng));
    HIP_TRY(M.d_slots.fill(P.slots));
    M.nblk = P.nblk;
    M.wgs = P.wgs;
    M.nruns = P.nruns;
    M.bpw = P.bpw;
    M.bad_runs = P.bad_runs;
    M.restarts = P.restarts;
    M.ok_fraction = 1.0 - (double)P.bad_nnz / (double)A->nnz;
    M.depth = mring_default_depth(P);
    M.skew = ring_wants_skew(A->n, A->h_ptrow.data());
    M.nt = beyond_infinity_cache(10.0, A->nnz, A->n);
    A->mring = std::move(M);
    return MI_OK;
}

// Plan of the tile kernel for this handle's pattern (host arrays of the caller, or nullptr: the handle's own device
// copy is read back — explicit MI_KERNEL_TILE requests on a handle created without it).
static int build_tile(mi_csr_t A, const int* indcol)
{
    if (A->tile.d_desc || A->n == 0 || A->nnz == 0) return MI_OK;
    std::vector<int> back;
    if (!indcol) {
        if (!A->d_indcol) return fail(MI_ERR_STATE, "tile plan: the handle no longer holds its column indices");
        back.resize((size_t)A->nnz);
        HIP_TRY(hipMemcpy(back.data(), A->d_indcol, sizeof(int) * (size_t)A->nnz, hipMemcpyDeviceToHost));
        indcol = back.data();
    }
    TilePlanHost P;
    build_tile_plan(A->n, A->h_ptrow.data(), indcol, P, kTileNnzb, 0, row_block_align(A->nnz));
    TileTable T;
    HIP_TRY(T.d_desc.alloc(P.desc.size()));
    HIP_TRY(T.d_ulist.alloc(P.ulist.size()));
    HIP_TRY(T.d_slots.alloc(P.slots.size()));
    HIP_TRY(T.d_desc.fill(P.desc));
    HIP_TRY(T.d_ulist.fill(P.ulist));
    HIP_TRY(T.d_slots.fill(P.slots));
    T.nblk = P.nblk;
    T.unique_per_nnz = (double)(P.ulist.size() - kTileThreads) / (double)A->nnz;
    T.skew = tile_wants_skew(A->n, A->h_ptrow.data());
    T.nt = beyond_infinity_cache(10.0, A->nnz, A->n);
    A->tile = std::move(T);
    return MI_OK;
}

// device copy of a ring plan (plan records, run tables, 16-bit column stream) and what the launch needs to know about it, into R — a fresh
// table of the caller's, moved to its place once this returns MI_OK
static int fill_ring_table(RingTable& R, const RingPlanHost& best, int n, const int* ptrow, const int* indcol, long long nnz, bool ghosts,
                           const int* row_min = nullptr, const int* row_max = nullptr, bool square = false)
{
    R.cfg = best.cfg;
    // Blocks of prefetch: with long runs (C4: 72 blocks per workgroup) four blocks in flight instead of two hide more of
    // the HBM latency — same handle, same box, back to back 172.8 / 168.8 / 167.5 us at depth 2 / 3 / 4, cold caches
    // 198.2 / 194.2 / 191.9 us; with short runs (1 M rows: 14 blocks) the longer pipeline fill costs more than it hides:
    // 34.7 / 35.1 / 37.3 us (tools/depth_ab.py, profiles/r02_ring_depth_ab.txt).  Configuration 4 only.
    R.cfg.depth = ring_default_depth(best);
    if (const char* e = getenv("MI355_RING_DEPTH")) {
        const int d = atoi(e);
        if (best.cfg.id == 4 && d >= 2 && d <= 4) R.cfg.depth = d;
    }
    R.nblk = best.nblk;
    R.wgs = best.wgs;
    R.bpw = best.bpw;
    R.bad_runs = best.bad_runs;
    R.ok_fraction = nnz ? 1.0 - (double)best.bad_nnz / (double)nnz : 0.0;
    R.lean = best.lean && best.cfg.id == 4 && !env_is("MI355_RING_LEAN", "0");
    if (best.nblk <= 0) return MI_OK;
    HIP_TRY(R.d_plan.upload(best.plan));
    HIP_TRY(R.d_ok.upload(best.run_ok));
    R.all_in_loop = true;
    for (int g = 0; g < best.wgs; g++) R.all_in_loop = R.all_in_loop && best.run_ok[g] == 1;
    R.h_dep_ptr.clear();
    R.h_dep_run.clear();
    if (square && row_min && R.all_in_loop && R.lean && best.cfg.id == 4 && !ghosts) build_run_deps(best, n, R.h_dep_ptr, R.h_dep_run);
    for (int g = 0; g < best.wgs; g++)
        R.uniform = R.uniform && best.run_rng[2 * g] == std::min(best.nblk, g * best.bpw) &&
                    best.run_rng[2 * g + 1] == std::min(best.nblk, (g + 1) * best.bpw);
    HIP_TRY(R.d_rng.upload(best.run_rng));
    if (ghosts) {
        R.h_run_halo = best.run_halo;
        HIP_TRY(R.d_run_halo.upload(best.run_halo));
    }
    {
        std::vector<unsigned short> slots;
        build_ring_slots(best, indcol, slots);
        HIP_TRY(R.d_slots.upload(slots));
    }
    R.skew = ring_wants_skew(n, ptrow);
    if (const char* e2 = getenv("MI355_RING_SKEW")) R.skew = atoi(e2) != 0;
    return MI_OK;
}

// mean launch time of A's current choice on the pair x / y, on the null stream
static int time_on(LaunchTimer& tm, mi_csr_t A, const double* x, double* y, int warm, int timed, double* us)
{
    return tm.time(warm, timed, [&] { return launch_spmv(A, x, y, nullptr); }, us);
}

// Placement draws (round 3, profiles/NOTES.md §4.12; FROZEN in round 4: no further work goes into it).  WHERE the value array lies in device
// memory moves a warm launch of the streaming kernels by up to 15 % on some boxes (tools/placement_lottery.py: 137-139 us against 158-166
// for handles of one and the same matrix and plan in one process; the coefficient array decides, the 16-bit column stream adds a few us,
// row pointers and plan records nothing; no allocation flag or address property found that predicts it).  So for matrices beyond the
// caches the chosen kernel is timed on a few fresh copies of those two arrays and the fastest copy is the one kept; every candidate
// stays allocated until the draws are over (a freed block would just be handed out again).
// Default since round 4: at most 4 draws of the value array (2 of the column stream), and none after the first when the first copy
// times within 2 % of the original (a box where placements are alike: nothing to find).  MI355_PLACEMENT_DRAWS=N (0..16) sets the
// number and disables the early stop — the 12-draw / 7 GB form of round 3 is MI355_PLACEMENT_DRAWS=12; =0 turns the draws off.
// given: the x / y pair to time on (null: a fresh pair is allocated); it moves into A->kept_x/y when keep_pair and draws were made.
static int placement_draws(mi_csr_t A, ScratchPair* given, bool keep_pair)
{
    const long long nnz = A->nnz;
    const char* pe = getenv("MI355_PLACEMENT_DRAWS");
    int draws = pe ? std::max(0, std::min(16, atoi(pe))) : 4;
    const bool early_stop = pe == nullptr;
    if (!pe) {
        size_t mem_free = 0, mem_total = 0;
        if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess && nnz > 0)
            draws = (int)std::min<size_t>((size_t)draws, mem_free / 8 / (sizeof(double) * (size_t)nnz));
        else (void)hipGetLastError();
    }
    // (a blocked copy served by its SLICED form streams sell.val, never d_coef: drawing d_coef there timed noise and could swap the array on it — ADVICE r4)
    const bool blocked_choice = A->auto_kernel == MI_KERNEL_BCSR4 && A->blocked && A->blocked->d_coef && !(A->blocked->sell_form >= 0 && A->blocked->sell.val);
    const bool streams_coef = A->auto_kernel == MI_KERNEL_RING || A->auto_kernel == MI_KERNEL_MRING || A->auto_kernel == MI_KERNEL_STREAM || A->auto_kernel == MI_KERNEL_TILE || blocked_choice;
    if (!(draws > 0 && streams_coef && nnz >= kLargeNnz)) return MI_OK;
    LaunchTimer tm;
    ScratchPair own;
    ScratchPair& pair = given ? *given : own;
    if (!given) {
        const size_t len = std::max(placed_vector_len(A->n, A->ncols), (size_t)(A->n_out > 0 ? A->n_out : 1));
        if (int rc = own.alloc(len, len)) return rc;
    }
    double *const tx = pair.x, *const ty = pair.y;
    if (int rc = tm.init()) return rc;
    auto time_now = [&](double* us) { return time_on(tm, A, tx, ty, 3, 8, us); };
    // pad_bytes: the zeroed tail the array was ALLOCATED with behind its payload — the ring family's unclamped loads read up to
    // kRingPadNnz values past the last nonzero, the blocked kernel one block past the last block; a copy must carry it too
    // (round 3's draws copied the payload into an exactly-sized buffer: every product on a redrawn array then read past its end)
    // (entries, not bytes: slot is the owning member itself, and the copy that loses a draw stays with `losers` until the draws are over)
    auto redraw = [&](auto& slot, size_t len, size_t pad, int ndraws) {
        using Arr = std::remove_reference_t<decltype(slot)>;
        double best = 0.0;
        if (!slot || len == 0 || time_now(&best) != MI_OK) return;
        const double first = best;
        A->place_us.push_back(best);
        std::vector<Arr> losers;
        for (int d = 0; d < ndraws; d++) {
            Arr fresh;
            if (fresh.alloc(len + pad) != hipSuccess) { (void)hipGetLastError(); break; } // no room for a copy: keep what there is
            if ((pad && hipMemset(fresh + len, 0, sizeof(*fresh.get()) * pad) != hipSuccess) ||
                hipMemcpy(fresh, slot, sizeof(*fresh.get()) * len, hipMemcpyDeviceToDevice) != hipSuccess) { (void)hipGetLastError(); break; }
            std::swap(slot, fresh); // fresh = the previous holder from here
            double t = 0.0;
            const int rct = time_now(&t);
            A->place_us.push_back(rct == MI_OK ? t : -1.0);
            if (rct == MI_OK && t < 0.96 * best) best = t; // the copy is clearly faster (two timings of ONE placement differ by 2-3 %): it holds the data from now on
            else std::swap(slot, fresh);
            losers.push_back(std::move(fresh));
            if (early_stop && d == 0 && rct == MI_OK && std::fabs(t - first) <= 0.02 * first) break; // placements are alike on this box
        }
        for (Arr& l : losers) l = {};
    };
    // (a matrix that runs the blocked kernel streams the BLOCKED copy's values: 16 doubles per block, zero fill included)
    if (blocked_choice) redraw(A->blocked->d_coef, 16 * (size_t)A->blocked->nblocks, 16, draws); // capi_bcsr.hip: 16 * (nb + 1)
    else redraw(A->d_coef, (size_t)nnz, (size_t)kRingPadNnz, draws);
    A->place_draws_coef = (int)A->place_us.size();
    // (the slot streams are allocated at exactly nblk * nnzb entries: no tail to carry)
    if (A->auto_kernel == MI_KERNEL_RING) redraw(A->ring.d_slots, (size_t)A->ring.nblk * A->ring.cfg.nnzb, 0, (draws + 1) / 2);
    else if (A->auto_kernel == MI_KERNEL_MRING) redraw(A->mring.d_slots, (size_t)A->mring.nblk * kMringNnzb, 0, (draws + 1) / 2);
    // The draws chose copies that are fast WITH THIS x / y pair; a caller that asks the library for its vectors gets the pair
    // itself as the first candidate (user-facing square handles only: a partition's pieces and mapped views are not handed vectors)
    if (keep_pair && !A->kept_x) A->kept_x = std::move(pair.x), A->kept_y = std::move(pair.y);
    return MI_OK;
}

// ---- csr_create_impl, one stage at a time
// nonzeros from which a matrix is measured at create (and its optional plans built by default); below, a product costs a few us and
// the stream kernel serves it
constexpr long long kMeasureNnz = 200000;

// what csr_create_impl was given, once checked, with the column range of every row (the ring planner's input)
struct CsrInput {
    int n, ncols;
    const int* ptrow;
    const int* indcol;
    const double* coef;
    const int* rowmap;
    int ghost_lo, ghost_hi; // ghost_lo < ghost_hi: a partition's combined piece (columns outside the range are ghosts)
    long long nnz = 0;
    bool offset_only = false; // the row map is "row r -> y[r + rowmap[0]]"
    std::vector<int> row_min, row_max;
    bool ghosts() const { return ghost_lo < ghost_hi; }
};

static int check_input(CsrInput& in)
{
    const int n = in.n;
    const int* ptrow = in.ptrow;
    CHECK_ARG(n >= 0 && in.ncols >= 0, "negative dimension");
    CHECK_ARG(ptrow, "ptrow is null");
    CHECK_ARG(ptrow[0] == 0, "ptrow[0] must be 0");
    for (int i = 0; i < n; i++) CHECK_ARG(ptrow[i] <= ptrow[i + 1], "ptrow must be non-decreasing");
    in.nnz = ptrow[n];
    CHECK_ARG(in.nnz == 0 || (in.indcol && in.coef), "indcol/coef is null");
    // 32-bit element offsets inside the kernels, padding included (ring_plan.hpp)
    CHECK_ARG(in.nnz <= 0x7fffffffLL - 2 * kRingPadNnz && n <= 0x7fffffff - 2 * kRingPadRows, "matrix too large for 32-bit offsets: partition it (mi_part_*)");
    in.row_min.resize((size_t)n);
    in.row_max.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        int lo = 0x7fffffff, hi = -1;
        for (int k = ptrow[i]; k < ptrow[i + 1]; k++) {
            const int c = in.indcol[k];
            CHECK_ARG(c >= 0 && c < in.ncols, "column index outside [0, ncols)");
            lo = c < lo ? c : lo;
            hi = c > hi ? c : hi;
        }
        in.row_min[i] = lo;
        in.row_max[i] = hi;
    }
    in.offset_only = in.rowmap != nullptr && n > 0; // e.g. the interior rows of a banded partition: one contiguous range
    for (int i = 1; in.offset_only && i < n; i++) in.offset_only = in.rowmap[i] == in.rowmap[0] + i;
    return MI_OK;
}

// the CSR arrays and the row map on the device, each with a zeroed tail: the kernels' unclamped / vector loads may touch it (ring_plan.hpp)
static int upload(mi_csr_t A, const CsrInput& in)
{
    const int n = in.n;
    const long long nnz = in.nnz;
    const size_t pad = 8, padv = kRingPadNnz, padr = kRingPadRows;
    HIP_TRY(hipGetDevice(&A->device));
    HIP_TRY(A->d_ptrow.alloc((size_t)n + 1 + padr));
    HIP_TRY(A->d_indcol.alloc((size_t)nnz + pad));
    HIP_TRY(A->d_coef.alloc((size_t)nnz + padv));
    HIP_TRY(hipMemset(A->d_ptrow + n + 1, 0, sizeof(int) * padr));
    HIP_TRY(hipMemset(A->d_indcol + nnz, 0, sizeof(int) * pad));
    HIP_TRY(hipMemset(A->d_coef + nnz, 0, sizeof(double) * padv));
    HIP_TRY(A->d_ptrow.fill(in.ptrow, (size_t)n + 1));
    HIP_TRY(A->d_indcol.fill(in.indcol, (size_t)nnz));
    HIP_TRY(A->d_coef.fill(in.coef, (size_t)nnz));
    A->mapped = in.rowmap != nullptr;
    if (in.offset_only) A->y_offset = in.rowmap[0];
    if (in.rowmap && n > 0 && !in.offset_only) {
        HIP_TRY(A->d_rowmap.alloc((size_t)n + padr));
        HIP_TRY(hipMemset(A->d_rowmap + n, 0, sizeof(int) * padr));
        HIP_TRY(A->d_rowmap.fill(in.rowmap, (size_t)n));
    }
    return MI_OK;
}

// window plan of the ring kernel: first configuration (in preference order) that
// serves at least 90 % of the nonzeros; MI355_RING_CONFIG=1..4 forces one
static int plan_ring(mi_csr_t A, const CsrInput& in)
{
    const int n = in.n;
    const long long nnz = in.nnz;
    if (n == 0 || nnz == 0) return MI_OK;
    int forced = 0;
    if (const char* e = getenv("MI355_RING_CONFIG")) forced = atoi(e);
    RingPlanHost best;
    bool have = false;
    for (int t = 0; t < kNumRingConfigs && !have; t++) {
        const int id = forced >= 1 && forced <= kNumRingConfigs ? forced : kRingConfigOrder[t];
        RingPlanHost P;
        build_ring_plan(kRingConfigs[id - 1], n, in.ptrow, in.row_min.data(), in.row_max.data(), P, in.ghost_lo, in.ghost_hi, large_row_align(nnz));
        const double okf = 1.0 - (double)P.bad_nnz / (double)nnz;
        if (forced || okf >= 0.90) {
            best = std::move(P);
            have = true;
        } else if (t == 0) {
            best = std::move(P); // remember the preferred one for explicit MI_KERNEL_RING requests
        }
        if (forced) break;
    }
    RingTable R;
    if (int rc = fill_ring_table(R, best, n, in.ptrow, in.indcol, nnz, in.ghosts(), in.row_min.data(), in.row_max.data(), n == in.ncols)) return rc;
    A->ring = std::move(R);
    A->auto_kernel = (have && A->ring.ok_fraction >= 0.90) ? MI_KERNEL_RING : MI_KERNEL_STREAM;
    return MI_OK;
}

// The optional plans share one rule: MI355_<switch>=0 never builds one; =1 or MI355_SPMV_KERNEL=<name> asks for it (built whatever the
// size, and kept); otherwise it is built when `by_size` holds
static bool plan_wanted(const char* sw, const char* name, bool by_size, bool* asked)
{
    *asked = env_is(sw, "1") || env_is("MI355_SPMV_KERNEL", name);
    return !env_is(sw, "0") && (*asked || by_size);
}

static int plan_optional(mi_csr_t A, const CsrInput& in)
{
    if (in.n == 0 || in.nnz == 0) return MI_OK;
    const bool measured = in.nnz >= kMeasureNnz;
    bool asked;
    int rc;
    // wide-band matrices (the ring does not serve them): the tile kernel's plan, kept if neighbouring rows share
    // enough columns for it to pay (tile_plan.hpp)
    if (plan_wanted("MI355_TILE", "tile", measured && A->auto_kernel != MI_KERNEL_RING, &asked)) {
        if ((rc = build_tile(A, in.indcol))) return rc;
        if (!asked && A->tile.unique_per_nnz > 0.6) A->tile = {}; // little sharing: nothing to gain over the stream kernel
    }
    // ... and the multi-window ring's (3-D mesh operators: a few narrow column clusters far apart), kept if it serves >= 90 %
    if (plan_wanted("MI355_MRING", "mring", measured && A->auto_kernel != MI_KERNEL_RING, &asked)) {
        if ((rc = build_mring(A, in.indcol, large_row_align(in.nnz)))) return rc;
        if (!asked && A->mring.ok_fraction < 0.90) A->mring = {};
    }
    // ... and the sliced copy of the sliced-stream kernel (spmv_sstream.hpp): matrices whose rounds of 512 rows fit the LDS window and
    // whose slices pad little.  (Row-mapped handles — partition pieces, the relabelled twin — included since the store goes through the
    // map; since round 5 also the fused multi-GPU step's combined piece: spmv_sstream_fused reads its ghost columns from the receive window)
    if (plan_wanted("MI355_SSTREAM", "sstream", measured, &asked)) {
        if ((rc = build_sstream(A, in.ptrow, in.indcol, in.ghost_lo, in.ghost_hi))) return rc;
        A->ss.asked = asked;
    }
    return MI_OK;
}

// FE matrices: a blocked copy for the BCSR 4x4 kernel (same bits, 8.25 instead of 12 B per nonzero)
// (a row map that moves whole nodes — rowmap[4b + q] = rowmap[4b] + q, 4-aligned — becomes a block-row map)
static int attach_blocked(mi_csr_t A, const CsrInput& in)
{
    const int n = in.n;
    const int* rowmap = in.rowmap;
    bool node_map = rowmap != nullptr && !in.offset_only && n % 4 == 0;
    for (int b = 0; node_map && b < n / 4; b++)
        node_map = rowmap[4 * b] % 4 == 0 && rowmap[4 * b + 1] == rowmap[4 * b] + 1 && rowmap[4 * b + 2] == rowmap[4 * b] + 2 &&
                   rowmap[4 * b + 3] == rowmap[4 * b] + 3;
    if (!(!rowmap || in.offset_only || node_map) || n < 4 || in.nnz < 16 || in.ncols % 4 != 0 || env_is("MI355_AUTO_BCSR", "0")) return MI_OK;
    std::vector<int> bptr, bcol;
    std::vector<double> bval;
    if (!csr_to_bcsr4_exact(n, in.ptrow, in.indcol, in.coef, bptr, bcol, bval)) return MI_OK;
    mi_bcsr4_t B = nullptr;
    if (int rc = mi_bcsr4_create(n / 4, in.ncols / 4, bptr.data(), bcol.data(), bval.data(), &B)) return rc;
    A->blocked.reset(B);
    if (node_map) {
        std::vector<int> bmap((size_t)n / 4);
        for (int b = 0; b < n / 4; b++) bmap[b] = rowmap[4 * b] / 4;
        HIP_TRY(B->d_browmap.upload(bmap));
    }
    return MI_OK;
}

// what holds when nothing is measured: value loads non-temporal once the matrix stream (10 B per nonzero in the ring kernel, 12 in the
// stream kernel) no longer fits the Infinity Cache (MI355_<kernel>_NT=0|1 forces), and the blocked copy where there is one
static void load_defaults(mi_csr_t A, const CsrInput& in)
{
    A->ring.nt = A->ring.d_slots && beyond_infinity_cache(10.0, in.nnz, in.n);
    if (const char* e = getenv("MI355_RING_NT")) A->ring.nt = A->ring.d_slots && atoi(e) != 0;
    A->stream_nt = beyond_infinity_cache(12.0, in.nnz, in.n);
    if (const char* e = getenv("MI355_STREAM_NT")) A->stream_nt = atoi(e) != 0;
    if (const char* e = getenv("MI355_TILE_NT")) A->tile.nt = atoi(e) != 0;
    if (const char* e = getenv("MI355_MRING_NT")) A->mring.nt = atoi(e) != 0;
    if (A->blocked) A->auto_kernel = MI_KERNEL_BCSR4; // unless measured otherwise
    A->n_out = in.n;
    if (in.rowmap)
        for (int i = 0; i < in.n; i++) A->n_out = in.rowmap[i] + 1 > A->n_out ? in.rowmap[i] + 1 : A->n_out;
}

// MI355_SPMV_KERNEL=<name>: that kernel, unmeasured, if the handle holds what it needs; true if it applied
static bool apply_forced_kernel(mi_csr_t A)
{
    const char* e = getenv("MI355_SPMV_KERNEL");
    if (!e) return false;
    if (!strcmp(e, "stream")) A->auto_kernel = MI_KERNEL_STREAM;
    else if (!strcmp(e, "ring") && A->ring.d_plan) A->auto_kernel = MI_KERNEL_RING;
    else if (!strcmp(e, "rowpar")) A->auto_kernel = MI_KERNEL_ROWPAR;
    else if (!strcmp(e, "bcsr4") && A->blocked) A->auto_kernel = MI_KERNEL_BCSR4;
    else if (!strcmp(e, "tile") && A->tile.d_desc) A->auto_kernel = MI_KERNEL_TILE;
    else if (!strcmp(e, "mring") && A->mring.d_plan) A->auto_kernel = MI_KERNEL_MRING;
    else if (!strcmp(e, "sstream") && A->ss.dev.val) A->auto_kernel = MI_KERNEL_SSTREAM;
    else return false;
    return true;
}

// the load form (non-temporal or not) a CSR kernel's launches use
static bool& nt_flag(mi_csr_t A, int k)
{
    switch (k) {
    case MI_KERNEL_RING: return A->ring.nt;
    case MI_KERNEL_TILE: return A->tile.nt;
    case MI_KERNEL_MRING: return A->mring.nt;
    default: return A->stream_nt;
    }
}

// measured microseconds of kernel k in the form it holds (0: not measured).  A blocked matrix enters the race with the blocked copy as
// its default (load_defaults), which stands on the stream kernel's time until the blocked copy itself has been timed.
static double tuned_us(mi_csr_t A, int k)
{
    if (k == MI_KERNEL_BCSR4 && A->tune_us[k][0] > 0) return A->tune_us[k][0];
    if (k != MI_KERNEL_RING && k != MI_KERNEL_TILE && k != MI_KERNEL_MRING) k = MI_KERNEL_STREAM;
    return A->tune_us[k][nt_flag(A, k)];
}

// The race on this very matrix, on the scratch pair (x = 0: timing does not depend on the values).  Timed in this order: the CSR kernels
// of kTuneKernels, each with temporal and then non-temporal matrix loads, in two interleaved rounds of which the faster counts (one round
// is not enough to tell two candidates 5 % apart: clock ramps, what the previous candidate left in the caches); then the blocked copy,
// one round; then the four forms of the sliced stream, two rounds.  A kernel takes over from the one in use only if strictly faster.
// A candidate whose measurement fails counts as not measured (0 us): it never wins.
static const struct {
    int kernel;
    const char* nt_env; // forces the load form: only that one is timed
} kTuneKernels[4] = {{MI_KERNEL_RING, "MI355_RING_NT"}, {MI_KERNEL_STREAM, "MI355_STREAM_NT"}, {MI_KERNEL_TILE, "MI355_TILE_NT"}, {MI_KERNEL_MRING, "MI355_MRING_NT"}};

static void tune(mi_csr_t A, LaunchTimer& tm, const ScratchPair& sp)
{
    // warm launches first: a temporal candidate is judged with the Infinity Cache holding
    // what it can of the matrix, as it would between the iterations of a solver
    const int timed = A->nnz < 40000000 ? 12 : 6;
    auto measure = [&](int warm, int count, double& slot, bool& failed) {
        double t = 0.0;
        if (time_on(tm, A, sp.x, sp.y, warm, count, &t) == MI_OK) slot = min_measured(slot, t);
        else failed = true;
    };
    const bool ring_ok = A->auto_kernel == MI_KERNEL_RING;
    auto in_race = [&](int k) {
        return k == MI_KERNEL_RING ? ring_ok : k == MI_KERNEL_TILE ? A->tile.d_desc != nullptr : k == MI_KERNEL_MRING ? A->mring.d_plan != nullptr : true;
    };
    bool nt0[4], failed[4][2] = {};
    for (int i = 0; i < 4; i++) nt0[i] = nt_flag(A, kTuneKernels[i].kernel);
    const double* ring_us = A->tune_us[MI_KERNEL_RING];
    for (int round = 0; round < 2; round++)
        for (int i = 0; i < 4; i++)
            for (int nt = 0; nt < 2; nt++) {
                const int k = kTuneKernels[i].kernel;
                double& us = A->tune_us[k][nt];
                if (!in_race(k) || failed[i][nt] || (getenv(kTuneKernels[i].nt_env) && nt != nt0[i])) continue;
                if (k == MI_KERNEL_RING && nt && !A->ring.d_slots) continue;
                if (k == MI_KERNEL_STREAM && round == 1 && ring_ok &&
                    us > 1.25 * std::min(ring_us[0] > 0 ? ring_us[0] : ring_us[1], ring_us[1] > 0 ? ring_us[1] : ring_us[0]))
                    continue; // stream is out of the race already
                nt_flag(A, k) = nt;
                A->kernel = k;
                measure(3, timed, us, failed[i][nt]);
            }
    for (int i = 0; i < 4; i++) {
        const int k = kTuneKernels[i].kernel;
        for (int nt = 0; nt < 2; nt++)
            if (failed[i][nt]) A->tune_us[k][nt] = 0.0;
        nt_flag(A, k) = in_race(k) ? better(A->tune_us[k][1], A->tune_us[k][0]) : nt0[i];
    }
    for (int i = 0; i < 4; i++)
        if (better(tuned_us(A, kTuneKernels[i].kernel), tuned_us(A, A->auto_kernel))) A->auto_kernel = kTuneKernels[i].kernel;
    if (A->blocked) { // the blocked copy against the best CSR kernel
        const double holder = tuned_us(A, A->auto_kernel);
        bool bfailed = false;
        A->kernel = MI_KERNEL_BCSR4;
        measure(3, 6, A->tune_us[MI_KERNEL_BCSR4][0], bfailed);
        if (better(A->tune_us[MI_KERNEL_BCSR4][0], holder)) A->auto_kernel = MI_KERNEL_BCSR4;
    }
    if (A->ss.dev.val && !getenv("MI355_SSTREAM_FORM")) { // the sliced stream against whatever won so far: 8 / 12 steps of prefetch x non-temporal / temporal value loads
        const double holder = tuned_us(A, A->auto_kernel);
        double* us = A->ss.tune_us;
        bool sfailed[4] = {};
        A->kernel = MI_KERNEL_SSTREAM;
        for (int round = 0; round < 2; round++)
            for (int f = 0; f < 4; f++) {
                if (sfailed[f]) continue;
                A->ss.nt = (f & 1) == 0;
                A->ss.deep = f >= 2;
                measure(3, timed, us[f], sfailed[f]);
            }
        int bf = -1;
        for (int f = 0; f < 4; f++) {
            if (sfailed[f]) us[f] = 0.0;
            if (us[f] > 0 && (bf < 0 || us[f] < us[bf])) bf = f;
        }
        if (bf >= 0) {
            A->ss.nt = (bf & 1) == 0;
            A->ss.deep = bf >= 2;
            if (better(us[bf], holder)) A->auto_kernel = MI_KERNEL_SSTREAM;
        }
        // A sliced copy that lost the measurement is released (+10 B per nonzero and its padding): mi_csr_set_kernel(MI_KERNEL_SSTREAM)
        // rebuilds it on demand.  Kept: one the environment asked for, and a combined piece's (the fused multi-GPU step takes the
        // sliced stream wherever EVERY rank can: its choice is collective, not this rank's measurement).
        if (A->auto_kernel != MI_KERNEL_SSTREAM && !A->ss.asked && !(A->ghost_lo < A->ghost_hi)) A->ss.copy() = {}; // (what it measured stays readable: mi_csr_sstream_info)
    }
    A->kernel = MI_KERNEL_AUTO;
}

// Large ring-served matrices take UNALIGNED blocks (large_row_align()).  MI355_RING_SHAPE_COMPARE=1 also builds the plan of
// whole-wave blocks and times both on the create-time scratch vectors (mi_csr_ring_shape_info; the shape in use stays unless
// the other is 2 % faster) — a comparison that says little about the caller's vectors, which is why it is no longer the rule.
// (a rank's combined piece of the fused multi-GPU step included: timed here without the exchange, as a plain product)
static void compare_ring_shapes(mi_csr_t A, const CsrInput& in, LaunchTimer& tm, const ScratchPair& sp)
{
    const long long nnz = in.nnz;
    if (!env_is("MI355_RING_SHAPE_COMPARE", "1") || getenv("MI355_RING_ROW_ALIGN") || nnz < kLargeNnz) return;
    auto time_now = [&](double* us) { return time_on(tm, A, sp.x, sp.y, 3, 8, us); };
    double us64 = 0.0, us1 = 0.0;
    if (A->auto_kernel == MI_KERNEL_RING && A->ring.cfg.id == 4) {
        RingPlanHost alt;
        build_ring_plan(kRingConfigs[3], in.n, in.ptrow, in.row_min.data(), in.row_max.data(), alt, in.ghost_lo, in.ghost_hi, 64);
        RingTable aligned;
        if (1.0 - (double)alt.bad_nnz / (double)nnz >= 0.90 &&
            fill_ring_table(aligned, alt, in.n, in.ptrow, in.indcol, nnz, in.ghosts(), in.row_min.data(), in.row_max.data(), in.n == in.ncols) == MI_OK) {
            aligned.nt = A->ring.nt;
            A->kernel = MI_KERNEL_RING;
            int rct = time_now(&us1);
            RingTable unaligned = std::move(A->ring);
            A->ring = std::move(aligned);
            if (rct == MI_OK) rct = time_now(&us64);
            A->kernel = MI_KERNEL_AUTO;
            A->tune_us_ring_aligned = us64;
            A->tune_us_ring_unaligned = us1;
            if (rct != MI_OK || !(us64 < 0.98 * us1)) A->ring = std::move(unaligned); // keep the default unless the other is clearly faster
            else unaligned = {};
        }
    } else if (A->auto_kernel == MI_KERNEL_MRING) { // the same for the multi-window ring
        MringTable unaligned = std::move(A->mring);
        if (build_mring(A, in.indcol, 64) == MI_OK && A->mring.d_plan && A->mring.ok_fraction >= 0.90) {
            A->mring.nt = unaligned.nt;
            A->kernel = MI_KERNEL_MRING;
            int rct = time_now(&us64);
            MringTable aligned = std::move(A->mring);
            A->mring = std::move(unaligned);
            if (rct == MI_OK) rct = time_now(&us1);
            A->kernel = MI_KERNEL_AUTO;
            A->tune_us_ring_aligned = us64;
            A->tune_us_ring_unaligned = us1;
            if (rct == MI_OK && us64 < 0.98 * us1) A->mring = std::move(aligned); // the whole-wave plan is clearly faster here
            else aligned = {};
        } else {
            A->mring = std::move(unaligned); // (releases a whole-wave plan that serves too little)
        }
    }
}

// the measurements of create: the race, the optional shape comparison, and (unless the caller defers them) the placement draws, all on
// one scratch pair — where a vector lies in device memory moves a launch by a few per cent
static int measure_at_create(mi_csr_t A, const CsrInput& in, bool defer_placement)
{
    // (sized like the vectors mi_vec_alloc_placed hands out: for a large square matrix this very pair becomes its first candidate)
    const size_t scratch_len = placed_vector_len(in.n, in.ncols);
    LaunchTimer tm;
    ScratchPair sp;
    int rc = sp.alloc(std::max(scratch_len, (size_t)(in.ncols > 0 ? in.ncols : 1)), std::max(scratch_len, (size_t)(A->n_out > 0 ? A->n_out : 1)));
    if (rc || (rc = tm.init())) return rc;
    tune(A, tm, sp);
    compare_ring_shapes(A, in, tm, sp);
    // placement draws (placement_draws() above): deferred when the caller (mi_csr_create) may still replace this handle's arrays by a
    // relabelled twin.  The handle keeps the pair when the draws were made (mi_vec_alloc_placed's first candidate).
    if (!defer_placement) (void)placement_draws(A, &sp, !in.rowmap && in.n == in.ncols && in.n == A->n_out && !in.ghosts());
    return MI_OK;
}

int csr_create_impl(int n, int ncols, const int* ptrow, const int* indcol, const double* coef,
                    const int* rowmap, mi_csr_t* out, int ghost_lo, int ghost_hi, bool defer_placement)
{
    CHECK_ARG(out, "out is null");
    *out = nullptr;
    CsrInput in{n, ncols, ptrow, indcol, coef, rowmap, ghost_lo, ghost_hi};
    int rc = check_input(in);
    if (rc || (rc = need_device())) return rc;
    // destroyed on every early return below, released to the caller on success
    std::unique_ptr<mi_csr_s> owner(new (std::nothrow) mi_csr_s());
    mi_csr_t A = owner.get();
    if (!A) return fail(MI_ERR_ALLOC, "host allocation failed");
    A->n = n;
    A->ncols = ncols;
    A->nnz = in.nnz;
    A->ghost_lo = ghost_lo;
    A->ghost_hi = ghost_hi;
    A->h_ptrow.assign(ptrow, ptrow + n + 1);
    if ((rc = upload(A, in)) || (rc = plan_ring(A, in)) || (rc = plan_optional(A, in)) || (rc = attach_blocked(A, in))) return rc;
    load_defaults(A, in);
    const bool forced_kernel = apply_forced_kernel(A);
    // Too small to be measured (< 200 000 nonzeros: a partition's boundary rows, a test matrix): the stream kernel — a launch of as
    // many workgroups as there are row blocks — not the ring kernel's persistent grid with its plan loads and window fill: a rank's
    // 2 000 boundary rows cost 11-17 us through the ring and 4.8 through the stream kernel (profiles/r05_sp2_trace_tail.txt).
    if (!forced_kernel && in.nnz < kMeasureNnz && A->auto_kernel == MI_KERNEL_RING && !in.ghosts()) A->auto_kernel = MI_KERNEL_STREAM;
    if (!forced_kernel && !env_is("MI355_SPMV_AUTOTUNE", "0") && in.nnz >= kMeasureNnz && (rc = measure_at_create(A, in, defer_placement))) return rc;
    // the handle is complete on return: the fills, zeroed paddings and uploads queued on the null stream above are done, so the first
    // product may come on any stream (a non-blocking one is not ordered behind the null stream)
    HIP_TRY(hipStreamSynchronize(nullptr));
    *out = owner.release();
    return MI_OK;
}

// mean launch time of A's current choice over `timed` launches after `warm` (x = 0: timing does not depend on values)
static int time_handle(mi_csr_t A, int warm, int timed, double* us)
{
    LaunchTimer tm;
    ScratchPair sp;
    int rc = sp.alloc((size_t)(A->ncols > 0 ? A->ncols : 1), (size_t)(A->n_out > 0 ? A->n_out : 1));
    if (rc || (rc = tm.init())) return rc;
    return time_on(tm, A, sp.x, sp.y, warm, timed, us);
}

// Locality reordering at create time (reorder.hpp).  Tried when the matrix is square, not row-mapped, large enough
// to matter, NOT already served by the ring kernel, and its nonzeros lie far from the diagonal for its size (an
// unstructured node numbering); kept when the reordered twin — x gather included — measures faster.
// MI355_REORDER=0 never, =1 always try and keep (tests), unset: as described.
static int maybe_reorder(mi_csr_t A, const int* ptrow, const int* indcol, const double* coef)
{
    const bool force = env_is("MI355_REORDER", "1");
    if (env_is("MI355_REORDER", "0")) return MI_OK;
    const int n = A->n;
    if (A->mapped || n != A->ncols || n < 8 || A->nnz == 0) return MI_OK;
    if (!force && (n < 100000 || resolve_kernel(A) == MI_KERNEL_RING || resolve_kernel(A) == MI_KERNEL_SSTREAM)) return MI_OK; // (a band served by its window: nothing to relabel)
    const int block = csr_has_block4_pattern(n, ptrow, indcol) ? 4 : 1;
    const double nn = (double)n / block;
    const double spread = mean_column_distance(n, ptrow, indcol, block);
    A->spread_before = spread;
    // a mesh of nn nodes in d >= 2 dimensions cannot be numbered with a mean distance much below nn^(1 - 1/d);
    // far above the 3-D figure means the numbering, not the mesh, spreads the columns
    if (!force && spread < 2.0 * std::pow(nn, 2.0 / 3.0)) return MI_OK;
    Reorder R;
    rcm_reorder(n, ptrow, indcol, block, R);
    A->reorder_block = block;
    A->spread_after = R.spread_after;
    if (!force && R.spread_after > 0.5 * spread) return MI_OK; // nothing gained
    std::vector<int> p2, c2, src_start;
    std::vector<double> v2;
    permute_csr(n, ptrow, indcol, coef, R, p2, c2, v2, src_start);
    mi_csr_t inner = nullptr;
    int rc = csr_create_impl(n, n, p2.data(), c2.data(), v2.data(), R.iperm.data(), &inner);
    if (rc) return rc;
    A->inner.reset(inner); // from here on launch_spmv(A) goes through the twin, which goes with A
    HIP_TRY(A->d_iperm.alloc((size_t)n));
    HIP_TRY(A->d_src_start.alloc((size_t)n));
    HIP_TRY(A->d_xp.alloc((size_t)n));
    HIP_TRY(A->d_iperm.fill(R.iperm));
    HIP_TRY(A->d_src_start.fill(src_start));
    bool keep = true;
    if (!force && !env_is("MI355_SPMV_AUTOTUNE", "0")) { // measure: natural choice against the twin (gather included)
        const int timed = A->nnz < 40000000 ? 12 : 6;
        (void)A->inner.own.release(); // (the natural handle, for a moment)
        rc = time_handle(A, 3, timed, &A->us_natural);
        A->inner.reset(inner);
        if (rc) return rc;
        if ((rc = time_handle(A, 3, timed, &A->us_reordered))) return rc;
        keep = A->us_reordered < 0.97 * A->us_natural;
    }
    if (!keep) {
        A->inner.reset(), A->d_iperm = {}, A->d_src_start = {}, A->d_xp = {};
        return MI_OK;
    }
    A->h_iperm = R.iperm; // host copy for mi_csr_perm (callers that keep their vectors in the library's numbering)
    A->xp_claimed = false; // (the measurement above ran on the default stream: the gather buffer goes to the caller's first stream)
    // the natural-order arrays and everything planned on them go: the twin serves the handle
    A->d_ptrow = {}, A->d_indcol = {}, A->d_coef = {};
    A->drop_tables();
    A->ring = {}, A->tile = {}, A->mring = {}, A->ss = {}, A->blocked.reset();
    return MI_OK;
}

extern "C" int mi_csr_create(int n, int ncols, const int* ptrow, const int* indcol, const double* coef, mi_csr_t* out)
{
    // (placement draws deferred: a handle that maybe_reorder replaces by its relabelled twin would draw for arrays it is about to release)
    int rc = csr_create_impl(n, ncols, ptrow, indcol, coef, nullptr, out, 0, 0, true);
    if (rc) return rc;
    if ((rc = maybe_reorder(*out, ptrow, indcol, coef)) || (!(*out)->inner && (rc = placement_draws(*out, nullptr, n == ncols))) ||
        (hipStreamSynchronize(nullptr) != hipSuccess && (rc = fail(MI_ERR_HIP, "mi_csr_create: synchronize")))) {
        mi_csr_destroy(*out);
        *out = nullptr;
    }
    return rc;
}

// host-only: the relabelling maybe_reorder would compute (reverse Cuthill-McKee on the node graph), for CPU tests
extern "C" int mi_reorder_probe(int n, const int* ptrow, const int* indcol, int* block, int* perm, double* spread_before,
                                double* spread_after)
{
    CHECK_ARG(n >= 0 && ptrow && (ptrow[n] == 0 || indcol), "bad argument");
    for (int i = 0; i < n; i++) {
        CHECK_ARG(ptrow[i] <= ptrow[i + 1], "ptrow must be non-decreasing");
        for (int k = ptrow[i]; k < ptrow[i + 1]; k++) CHECK_ARG(indcol[k] >= 0 && indcol[k] < n, "column index outside [0, n)");
    }
    const int b = csr_has_block4_pattern(n, ptrow, indcol) ? 4 : 1;
    Reorder R;
    rcm_reorder(n, ptrow, indcol, b, R);
    if (block) *block = b;
    if (perm)
        for (int i = 0; i < n; i++) perm[i] = R.perm[i];
    if (spread_before) *spread_before = R.spread_before;
    if (spread_after) *spread_after = R.spread_after;
    return MI_OK;
}

extern "C" int mi_csr_reorder_info(mi_csr_t A, int* reordered, int* block, double* spread_before, double* spread_after,
                                   double* us_natural, double* us_reordered)
{
    CHECK_ARG(A, "null handle");
    if (reordered) *reordered = A->inner ? 1 : 0;
    if (block) *block = A->reorder_block;
    if (spread_before) *spread_before = A->spread_before;
    if (spread_after) *spread_after = A->spread_after;
    if (us_natural) *us_natural = A->us_natural;
    if (us_reordered) *us_reordered = A->us_reordered;
    return MI_OK;
}

// ---- the library's own numbering, for callers that own the loop (a Krylov solve: many products per matrix) ----------------
extern "C" int mi_csr_perm(mi_csr_t A, int* reordered, int* perm)
{
    CHECK_ARG(A, "null handle");
    if (reordered) *reordered = A->inner ? 1 : 0;
    if (perm) {
        if (A->inner) {
            CHECK_ARG((int)A->h_iperm.size() == A->n, "permutation not kept on this handle");
            for (int r = 0; r < A->n; r++) perm[A->h_iperm[r]] = r; // perm[old] = new
        } else {
            for (int i = 0; i < A->n; i++) perm[i] = i;
        }
    }
    return MI_OK;
}

extern "C" int mi_vec_to_internal_dev(mi_csr_t A, const double* d_x, double* d_x_int, mi_stream_t s)
{
    CHECK_ARG(A, "null handle");
    if (A->n == 0) return MI_OK;
    CHECK_ARG(d_x && d_x_int && d_x != d_x_int, "null vector, or in place");
    if (A->inner) return gather_perm(A, d_x, d_x_int, (hipStream_t)s);
    HIP_TRY(hipMemcpyAsync(d_x_int, d_x, sizeof(double) * (size_t)A->n, hipMemcpyDeviceToDevice, (hipStream_t)s));
    return MI_OK;
}

extern "C" int mi_vec_from_internal_dev(mi_csr_t A, const double* d_x_int, double* d_x, mi_stream_t s)
{
    CHECK_ARG(A, "null handle");
    if (A->n == 0) return MI_OK;
    CHECK_ARG(d_x && d_x_int && d_x != d_x_int, "null vector, or in place");
    if (A->inner) return scatter_perm(A, d_x_int, d_x, (hipStream_t)s);
    HIP_TRY(hipMemcpyAsync(d_x, d_x_int, sizeof(double) * (size_t)A->n, hipMemcpyDeviceToDevice, (hipStream_t)s));
    return MI_OK;
}

extern "C" int mi_spmv_internal_dev(mi_csr_t A, const double* d_x_int, double* d_y_int, mi_stream_t s)
{
    CHECK_ARG(A, "null handle");
    CHECK_ARG(A->n == A->ncols && !A->mapped, "the internal numbering is defined for square, unmapped matrices");
    CHECK_ARG(A->n == 0 || (d_x_int && d_y_int), "null vector");
    // a relabelled handle: the twin alone, reading and writing its own numbering — no gather, no row map, no per-handle
    // scratch (so products on several streams may overlap); any other handle: its numbering IS the caller's
    if (A->inner) return launch_spmv(A->inner, d_x_int, d_y_int, (hipStream_t)s, false);
    return launch_spmv(A, d_x_int, d_y_int, (hipStream_t)s);
}

extern "C" int mi_spmk_internal_dev(mi_csr_t A, int k, const double* d_x_int, double* const* d_y_int_out, mi_stream_t s)
{
    CHECK_ARG(A, "null handle");
    if (k < 1 || k > MI_MAX_POWERS) return fail(MI_ERR_UNSUPPORTED, "k must be in 1..MI_MAX_POWERS");
    CHECK_ARG(d_y_int_out, "null output array");
    CHECK_ARG(A->n == A->ncols && !A->mapped, "the internal numbering is defined for square, unmapped matrices");
    if (A->n == 0) return MI_OK;
    CHECK_ARG(d_x_int, "null vector");
    for (int p = 0; p < k; p++) CHECK_ARG(d_y_int_out[p], "null output vector");
    return spmk_unmapped(A->inner ? A->inner : A, k, d_x_int, d_y_int_out, (hipStream_t)s);
}

extern "C" int mi_csr_create_mapped(int n, int ncols, const int* ptrow, const int* indcol, const double* coef,
                                    const int* rowmap, mi_csr_t* out)
{
    return csr_create_impl(n, ncols, ptrow, indcol, coef, rowmap, out);
}

extern "C" int mi_csr_destroy(mi_csr_t A)
{
    if (!A) return MI_OK;
    delete A;
    return MI_OK;
}

// every value refresh comes by here, on the stream the new CSR values were written on: the copies derived from them follow AT ONCE on
// that stream (the sliced values of spmv_sstream unless the caller filled them in the same pass as the CSR values; the blocked copy and
// its sliced values), so that stream order — and a HIP graph captured earlier — see them like the CSR values themselves
static int refresh_blocked_values(mi_csr_t A, hipStream_t s, bool sliced_done = false)
{
    if (A->ss.dev.val && !sliced_done) {
        SstreamTable& T = A->ss;
        sstream_fill_values(T.rounds, A->n, T.shift, A->d_ptrow, A->d_coef, nullptr, T.dev.slice_step, T.dev.slice_len, T.dev.val, T.max_slice_nnz, s, T.mw ? 1 : 0);
        HIP_TRY(hipGetLastError());
    }
    if (!A->blocked || A->blocked->nbrows == 0) return MI_OK;
    return bcsr4_refresh_from_csr(A->blocked, A->d_ptrow, A->d_coef, nullptr, s); // blocks and sliced values from the CSR values, one pass
}

// New coefficients for an unchanged sparsity pattern (what a Newton loop does to its Jacobian every
// iteration, src/solve_newton.c:1245-1247): only the value array is replaced.  Row-block tables, the
// ring plan, the 16-bit column stream and the kernel choice depend on the pattern alone and are kept;
// the blocked copy's values are regenerated on the device.
// values of a reordered twin from the caller's (original order) values: new row r' copies its segment
__global__ __launch_bounds__(256) void permute_values_kernel(int n, const int* __restrict__ new_ptrow, const int* __restrict__ src_start,
                                                             const double* __restrict__ src, double* __restrict__ dst)
{
    // (round 5) 64 new rows per workgroup and turn: their destination is ONE contiguous segment, written coalesced; every element finds
    // its row by bisection over the 65 row pointers in LDS and reads from that row's (contiguous) source segment.  The first form — a
    // thread per row walking it — took 2.0-2.8 ms per value update of the relabelled mesh / FE matrices.
    __shared__ int s_p[65], s_a[64];
    const int tid = threadIdx.x;
    for (int r0 = blockIdx.x * 64; r0 < n; r0 += gridDim.x * 64) {
        const int nr = min(64, n - r0);
        if (tid <= nr) s_p[tid] = new_ptrow[r0 + tid];
        if (tid < nr) s_a[tid] = src_start[r0 + tid];
        __syncthreads();
        const int b0 = s_p[0], seg = s_p[nr] - b0;
        for (int k = tid; k < seg; k += 256) {
            const int p = b0 + k;
            int lo = 0, hi = nr; // s_p[lo] <= p < s_p[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_p[mid] <= p) lo = mid;
                else hi = mid;
            }
            dst[p] = src[s_a[lo] + (p - s_p[lo])];
        }
        __syncthreads();
    }
}

extern "C" int mi_csr_update_values_dev(mi_csr_t A, const double* d_coef, mi_stream_t s_)
{
    CHECK_ARG(A, "null handle");
    if (A->nnz == 0) return MI_OK;
    CHECK_ARG(d_coef, "null coef");
    hipStream_t s = (hipStream_t)s_;
    if (A->inner) {
        mi_csr_t I = A->inner;
        hipLaunchKernelGGL(permute_values_kernel, dim3(launch_grid(A->n, 64, 4096, 1)), dim3(256), 0, s, A->n, I->d_ptrow, A->d_src_start, d_coef, I->d_coef);
        HIP_TRY(hipGetLastError());
        return refresh_blocked_values(I, s);
    }
    if (A->ss.dev.val && d_coef != A->d_coef) { // ONE pass over the caller's values: the CSR values and the sliced values leave together
        SstreamTable& T = A->ss;
        sstream_fill_values(T.rounds, A->n, T.shift, A->d_ptrow, d_coef, A->d_coef, T.dev.slice_step, T.dev.slice_len, T.dev.val, T.max_slice_nnz, s, T.mw ? 1 : 0);
        HIP_TRY(hipGetLastError());
        return refresh_blocked_values(A, s, true);
    }
    if (A->blocked && A->blocked->nbrows > 0 && d_coef != A->d_coef) // the same pass for a blocked copy: CSR values, blocks and sliced values leave together
        return bcsr4_refresh_from_csr(A->blocked, A->d_ptrow, d_coef, A->d_coef, s);
    if (d_coef != A->d_coef) HIP_TRY(hipMemcpyAsync(A->d_coef, d_coef, sizeof(double) * (size_t)A->nnz, hipMemcpyDeviceToDevice, s));
    return refresh_blocked_values(A, s);
}

extern "C" int mi_csr_update_values(mi_csr_t A, const double* coef)
{
    CHECK_ARG(A, "null handle");
    if (A->nnz == 0) return MI_OK;
    CHECK_ARG(coef, "null coef");
    if (A->inner) {
        if (!A->d_vtmp) HIP_TRY(A->d_vtmp.alloc((size_t)A->nnz));
        HIP_TRY(hipMemcpy(A->d_vtmp, coef, sizeof(double) * (size_t)A->nnz, hipMemcpyHostToDevice));
        int rc = mi_csr_update_values_dev(A, A->d_vtmp, nullptr);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        return MI_OK;
    }
    HIP_TRY(hipMemcpy(A->d_coef, coef, sizeof(double) * (size_t)A->nnz, hipMemcpyHostToDevice));
    int rc = refresh_blocked_values(A, nullptr);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return MI_OK;
}

extern "C" int mi_csr_dims(mi_csr_t A, int* n, int* ncols, long long* nnz)
{
    CHECK_ARG(A, "null handle");
    if (n) *n = A->n;
    if (ncols) *ncols = A->ncols;
    if (nnz) *nnz = A->nnz;
    return MI_OK;
}

int resolve_kernel(const mi_csr_s* A)
{
    int k = A->kernel != MI_KERNEL_AUTO ? A->kernel : A->auto_kernel;
    if (k == MI_KERNEL_RING && !A->ring.d_plan) k = MI_KERNEL_STREAM; // empty matrix: nothing to plan
    if (k == MI_KERNEL_BCSR4 && !A->blocked) k = MI_KERNEL_STREAM;
    if (k == MI_KERNEL_TILE && !A->tile.d_desc) k = MI_KERNEL_STREAM;
    if (k == MI_KERNEL_MRING && !A->mring.d_plan) k = MI_KERNEL_STREAM;
    if (k == MI_KERNEL_SSTREAM && !A->ss.dev.val) k = A->ring.d_plan && A->ring.ok_fraction >= 0.90 ? MI_KERNEL_RING : MI_KERNEL_STREAM;
    return k;
}

extern "C" int mi_csr_tune_info(mi_csr_t A, double* us_ring, double* us_stream)
{
    CHECK_ARG(A, "null handle");
    if (A->inner) A = A->inner;
    if (us_ring) *us_ring = A->tune_us[MI_KERNEL_RING][A->ring.nt];
    if (us_stream) *us_stream = A->tune_us[MI_KERNEL_STREAM][A->stream_nt];
    return MI_OK;
}

extern "C" int mi_csr_tune_detail(mi_csr_t A, double us[5], int* ring_nt, int* stream_nt)
{
    CHECK_ARG(A, "null handle");
    if (A->inner) A = A->inner;
    if (us) {
        us[0] = A->tune_us[MI_KERNEL_RING][0];
        us[1] = A->tune_us[MI_KERNEL_RING][1];
        us[2] = A->tune_us[MI_KERNEL_STREAM][0];
        us[3] = A->tune_us[MI_KERNEL_STREAM][1];
        us[4] = A->tune_us[MI_KERNEL_BCSR4][0];
    }
    if (ring_nt) *ring_nt = A->ring.nt ? 1 : 0;
    if (stream_nt) *stream_nt = A->stream_nt ? 1 : 0;
    return MI_OK;
}

// smallest / largest column of every row (row_min > row_max for an empty row): the ring planner's input, for the host-only probes
static void row_ranges(int n, const int* ptrow, const int* indcol, std::vector<int>& row_min, std::vector<int>& row_max)
{
    row_min.assign((size_t)n, 0x7fffffff);
    row_max.assign((size_t)n, -1);
    for (int i = 0; i < n; i++)
        for (int k = ptrow[i]; k < ptrow[i + 1]; k++) {
            row_min[i] = std::min(row_min[i], indcol[k]);
            row_max[i] = std::max(row_max[i], indcol[k]);
        }
}

// host-only: build the ring plan and the 16-bit column stream for one configuration exactly as
// mi_csr_create would, and check their invariants (every block of a served run keeps its columns
// inside one window of at most RING entries, distinct columns of a block get distinct slots, slots
// are < RING, rows/nonzeros are covered once and in order).  For CPU-side tests of the planner.
extern "C" int mi_ring_plan_probe(int n, const int* ptrow, const int* indcol, int config_id, int* nblk, int* runs,
                                  int* runs_not_ringable, double* nnz_fraction_ringable, int* max_slot)
{
    CHECK_ARG(n >= 0 && ptrow && config_id >= 1 && config_id <= kNumRingConfigs, "bad argument");
    const long long nnz = ptrow[n];
    CHECK_ARG(nnz == 0 || indcol, "indcol is null");
    std::vector<int> row_min, row_max;
    row_ranges(n, ptrow, indcol, row_min, row_max);
    RingPlanHost P;
    build_ring_plan(kRingConfigs[config_id - 1], n, ptrow, row_min.data(), row_max.data(), P);
    std::vector<unsigned short> slots;
    if (P.nblk > 0) build_ring_slots(P, indcol, slots);
    const RingConfig& c = P.cfg;
    const int T = c.threads, per = c.nnzb / T;
    int next_row = 0, mslot = -1;
    long long next_nz = 0;
    // replay of the window as the kernel keeps it: content[s] = the column whose x value slot s holds
    std::vector<int> content((size_t)c.ring, -1);
    int cur_run = -1;
    // the runs: every block in exactly one, none longer than the kernel's LDS plan, dealt out by weight (ring_plan.hpp)
    std::vector<int> run_of((size_t)P.nblk, -1);
    long long wmax = 0, wsum = 0;
    for (int g = 0; g < P.wgs; g++) {
        const int b0 = P.run_rng[2 * g], b1 = P.run_rng[2 * g + 1];
        if (b0 < 0 || b1 < b0 || b1 > P.nblk || b1 - b0 > kRingMaxB) return fail(MI_ERR_STATE, "run range out of bounds or longer than the kernel's plan");
        long long w = 0;
        for (int b = b0; b < b1; b++) {
            if (run_of[b] >= 0) return fail(MI_ERR_STATE, "a block belongs to two runs");
            run_of[b] = g;
            w += !P.run_ok[g] || P.plan[(size_t)8 * b + 7] == 2 ? kRingPlainWeight : 1;
        }
        wmax = std::max(wmax, w);
        wsum += w;
    }
    for (int b = 0; b < P.nblk; b++)
        if (run_of[b] < 0) return fail(MI_ERR_STATE, "a block belongs to no run");
    if (P.wgs > 0 && wmax > 2 * (wsum / P.wgs) + 4 * kRingPlainWeight) return fail(MI_ERR_STATE, "one run carries more than twice the mean weight");
    for (int b = 0; b < P.nblk; b++) {
        const int* Q = &P.plan[(size_t)8 * b];
        if (Q[0] != next_row || Q[1] != next_nz) return fail(MI_ERR_STATE, "plan does not cover rows / nonzeros in order");
        const int brows = Q[7] == 2 ? Q[4] : Q[2]; // a PLAIN block keeps its row count out of the loop's sight
        next_row += brows;
        next_nz += Q[3];
        if (Q[3] != ptrow[Q[0] + brows] - ptrow[Q[0]]) return fail(MI_ERR_STATE, "block nonzero count disagrees with ptrow");
        const int run = run_of[b];
        if (P.lean && P.run_ok[run] && brows > T) return fail(MI_ERR_STATE, "a LEAN plan holds a block of more than T rows");
        if (!P.run_ok[run] || Q[3] == 0) {
            if (Q[7] == 2 || (Q[7] && Q[3] == 0)) return fail(MI_ERR_STATE, "flags of a block outside the ring loop");
            continue;
        }
        if (Q[7] == 2) { // computed behind the loop: the loop must see an empty block
            if (Q[2] != 0 || Q[5] != 0) return fail(MI_ERR_STATE, "a PLAIN block is visible to the ring loop");
            if (P.run_ok[run] != 3) return fail(MI_ERR_STATE, "a run with a PLAIN block does not tell the kernel to look behind its loop");
            continue;
        }
        if (Q[7] != 1 || Q[3] > c.nnzb || Q[2] > 2 * T) return fail(MI_ERR_STATE, "a served run holds a block the kernel cannot take");
        int cmin = 0x7fffffff, cmax = -1;
        for (long long k = Q[1]; k < (long long)Q[1] + Q[3]; k++) {
            cmin = std::min(cmin, indcol[k]);
            cmax = std::max(cmax, indcol[k]);
        }
        if (cmax - cmin + 1 > c.ring) return fail(MI_ERR_STATE, "block window wider than the ring");
        if (cmin - Q[6] < 0 || cmax - Q[6] >= 2 * c.ring) return fail(MI_ERR_STATE, "ring base out of range for the block's columns");
        if (Q[4] + Q[5] < cmax + 1) return fail(MI_ERR_STATE, "window does not reach the block's last column");
        if (P.lean && Q[5] > T && b != P.run_rng[2 * run]) return fail(MI_ERR_STATE, "a LEAN plan brings more than T new columns into a block inside a run");
        if (run != cur_run) { // a new workgroup: nothing in its ring yet
            std::fill(content.begin(), content.end(), -1);
            cur_run = run;
        }
        for (int col = Q[4]; col < Q[4] + Q[5]; col++) { // the columns this block brings in
            int sl = col - Q[6];
            if (sl >= c.ring) sl -= c.ring;
            if (sl < 0 || sl >= c.ring) return fail(MI_ERR_STATE, "a new column falls outside the ring");
            content[sl] = col;
        }
        for (int k = 0; k < Q[3]; k++)
            if (content[(indcol[Q[1] + k] - Q[6]) >= c.ring ? indcol[Q[1] + k] - Q[6] - c.ring : indcol[Q[1] + k] - Q[6]] != indcol[Q[1] + k])
                return fail(MI_ERR_STATE, "a nonzero's column is not in the window when its block runs");
        for (int k = 0; k < Q[3]; k++) { // slot of nonzero k as the kernel's thread (k % T), element k / T reads it
            const int slot = slots[(size_t)b * c.nnzb + (size_t)ring_slot_pos(T, per, k)];
            int want = indcol[Q[1] + k] - Q[6];
            if (want >= c.ring) want -= c.ring;
            if (slot != want || slot < 0 || slot >= c.ring) return fail(MI_ERR_STATE, "16-bit slot disagrees with the column");
            mslot = std::max(mslot, slot);
        }
    }
    if (next_row != n || next_nz != nnz) return fail(MI_ERR_STATE, "plan does not cover the matrix");
    if (nblk) *nblk = P.nblk;
    if (runs) *runs = P.wgs;
    if (runs_not_ringable) *runs_not_ringable = P.bad_runs;
    if (nnz_fraction_ringable) *nnz_fraction_ringable = nnz ? 1.0 - (double)P.bad_nnz / (double)nnz : 0.0;
    if (max_slot) *max_slot = mslot;
    return MI_OK;
}

// host-only: ring configuration 4's plan of a square pattern and the run dependencies of the one-launch powers step, built by the two
// calls mi_csr_create makes (build_ring_plan, build_run_deps) — the one source of what mi_spmk_plan_probe checks and
// mi_spmk_plan_dump copies out.  in_loop: every row is computed inside the LEAN ring loop; without that no lists are built.
struct SpmkPlanHost {
    RingPlanHost P;
    bool in_loop = false;
    std::vector<int> dep_ptr, dep_run;
};
static int build_spmk_plan_host(int n, const int* ptrow, const int* indcol, SpmkPlanHost& S)
{
    std::vector<int> row_min((size_t)n), row_max((size_t)n);
    for (int i = 0; i < n; i++) {
        int lo = 0x7fffffff, hi = -1;
        for (int k = ptrow[i]; k < ptrow[i + 1]; k++) {
            CHECK_ARG(indcol[k] >= 0 && indcol[k] < n, "column index outside [0, n)");
            lo = std::min(lo, indcol[k]);
            hi = std::max(hi, indcol[k]);
        }
        row_min[i] = lo;
        row_max[i] = hi;
    }
    build_ring_plan(kRingConfigs[3], n, ptrow, row_min.data(), row_max.data(), S.P);
    S.in_loop = S.P.lean && S.P.nblk > 0;
    for (int g = 0; g < S.P.wgs; g++) S.in_loop = S.in_loop && S.P.run_ok[g] == 1;
    S.dep_ptr.clear();
    S.dep_run.clear();
    if (S.in_loop) build_run_deps(S.P, n, S.dep_ptr, S.dep_run);
    return MI_OK;
}

// host-only: the run dependencies of the one-launch powers step exactly as mi_csr_create derives them (ring configuration 4),
// checked against the matrix: every column a run's rows NAME, and every column its lanes LOAD when the plan is replayed (window
// fills, the T lanes behind a block's new columns, the empty blocks behind the run), lies in the rows of a run on its list.
extern "C" int mi_spmk_plan_probe(int n, const int* ptrow, const int* indcol, int* eligible, int* runs, int* max_deps)
{
    CHECK_ARG(n >= 0 && ptrow && ptrow[0] == 0 && eligible, "bad argument");
    CHECK_ARG(ptrow[n] == 0 || indcol, "indcol is null");
    *eligible = 0;
    if (runs) *runs = 0;
    if (max_deps) *max_deps = 0;
    if (n == 0 || ptrow[n] == 0) return MI_OK;
    SpmkPlanHost S;
    if (int rc = build_spmk_plan_host(n, ptrow, indcol, S)) return rc;
    if (!S.in_loop) return MI_OK; // such a handle runs k launches
    const RingPlanHost& P = S.P;
    const std::vector<int>&dp = S.dep_ptr, &dr = S.dep_run;
    const int W = P.wgs, T = P.cfg.threads;
    std::vector<int> owner((size_t)n, -1);
    for (int g = 0; g < W; g++)
        for (int b = P.run_rng[2 * g]; b < P.run_rng[2 * g + 1]; b++)
            for (int r = P.plan[(size_t)8 * b]; r < P.plan[(size_t)8 * b] + P.plan[(size_t)8 * b + 2]; r++) owner[r] = g;
    for (int i = 0; i < n; i++)
        if (owner[i] < 0) return fail(MI_ERR_STATE, "a row belongs to no run");
    int md = 0;
    std::vector<char> on_list((size_t)W);
    for (int g = 0; g < W; g++) {
        md = std::max(md, dp[g + 1] - dp[g]);
        std::fill(on_list.begin(), on_list.end(), 0);
        for (int j = dp[g]; j < dp[g + 1]; j++) on_list[dr[j]] = 1;
        const int b0 = P.run_rng[2 * g], b1 = P.run_rng[2 * g + 1];
        if (b0 >= b1) continue;
        for (int b = b0; b < b1; b++) {
            const int* Q = &P.plan[(size_t)8 * b];
            for (int k = Q[1]; k < Q[1] + Q[3]; k++)
                if (!on_list[owner[indcol[k]]]) return fail(MI_ERR_STATE, "a run names a column of a run that is not on its list");
            const int load_hi = std::min(n - 1, Q[4] + std::max(Q[5], T) - 1);
            for (int col = Q[4]; col <= load_hi; col++)
                if (!on_list[owner[col]]) return fail(MI_ERR_STATE, "a run loads a column of a run that is not on its list");
        }
    }
    *eligible = md <= 64 ? 1 : 0;
    if (runs) *runs = W;
    if (max_deps) *max_deps = md;
    return MI_OK;
}

// host-only: the plan and the lists mi_spmk_plan_probe checks, copied out (sizes from a first call without arrays)
extern "C" int mi_spmk_plan_dump(int n, const int* ptrow, const int* indcol, int info[8], int* plan, int* run_rng, int* dep_ptr, int* dep_run,
                                 int cap_blocks, int cap_runs, int cap_deps)
{
    CHECK_ARG(n >= 0 && ptrow && ptrow[0] == 0 && info, "bad argument");
    CHECK_ARG(ptrow[n] == 0 || indcol, "indcol is null");
    for (int j = 0; j < 8; j++) info[j] = 0;
    if (n == 0 || ptrow[n] == 0) return MI_OK;
    SpmkPlanHost S;
    if (int rc = build_spmk_plan_host(n, ptrow, indcol, S)) return rc;
    const RingPlanHost& P = S.P;
    bool uniform = true; // the comparison fill_ring_table makes: the kernel derives the runs from bpw, else reads run_rng
    for (int g = 0; g < P.wgs; g++)
        uniform = uniform && P.run_rng[2 * g] == std::min(P.nblk, g * P.bpw) && P.run_rng[2 * g + 1] == std::min(P.nblk, (g + 1) * P.bpw);
    info[0] = P.cfg.threads;
    info[1] = P.nblk;
    info[2] = P.wgs;
    info[3] = P.bpw;
    info[4] = uniform ? 1 : 0;
    info[5] = S.in_loop ? 1 : 0;
    info[6] = (int)S.dep_run.size();
    info[7] = P.lean ? 1 : 0;
    if (plan) {
        CHECK_ARG(cap_blocks >= P.nblk, "plan: room for 8 ints per block needed");
        std::copy(P.plan.begin(), P.plan.end(), plan);
    }
    if (run_rng) {
        CHECK_ARG(cap_runs >= P.wgs, "run_rng: room for 2 ints per run needed");
        std::copy(P.run_rng.begin(), P.run_rng.end(), run_rng);
    }
    if (dep_ptr) {
        CHECK_ARG(cap_runs >= P.wgs, "dep_ptr: room for runs + 1 ints needed");
        for (int g = 0; g <= P.wgs; g++) dep_ptr[g] = S.in_loop ? S.dep_ptr[g] : 0;
    }
    if (dep_run) {
        CHECK_ARG(cap_deps >= (int)S.dep_run.size(), "dep_run: too small");
        std::copy(S.dep_run.begin(), S.dep_run.end(), dep_run);
    }
    return MI_OK;
}

extern "C" int mi_csr_sstream_info(mi_csr_t A, int* built, int* rounds, long long* steps, double* padding, double us[4], int* form)
{
    CHECK_ARG(A, "null handle");
    if (A->inner) A = A->inner;
    if (built) *built = A->ss.dev.val != nullptr;
    if (rounds) *rounds = A->ss.rounds;
    if (steps) *steps = A->ss.steps;
    if (padding) *padding = A->ss.padding;
    if (us)
        for (int f = 0; f < 4; f++) us[f] = A->ss.tune_us[f];
    if (form) *form = A->ss.dev.val ? (A->ss.deep ? 2 : 0) + (A->ss.nt ? 0 : 1) : -1;
    return MI_OK;
}

extern "C" int mi_sstream_plan_probe(int n, int ncols, const int* ptrow, const int* indcol, int* eligible, int* rounds, long long* steps, double* padding)
{
    return mi_sstream_plan_probe_ex(n, ncols, ptrow, indcol, 0, 0, 0, eligible, rounds, steps, padding, nullptr, nullptr);
}

extern "C" int mi_sstream_plan_probe_ex(int n, int ncols, const int* ptrow, const int* indcol, int shift, int ghost_lo, int ghost_hi, int* eligible, int* rounds,
                                        long long* steps, double* padding, int* ghost_workgroups, int* rounds_min_max)
{
    CHECK_ARG(n >= 0 && ncols >= 0 && ptrow && ptrow[0] == 0 && eligible, "bad argument");
    CHECK_ARG(shift == 0 || shift == 1, "shift must be 0 or 1");
    CHECK_ARG(ghost_lo >= 0 && ghost_hi <= ncols, "ghost range outside the columns");
    CHECK_ARG(ptrow[n] == 0 || indcol, "indcol is null");
    for (int i = 0; i < n; i++) CHECK_ARG(ptrow[i] <= ptrow[i + 1], "ptrow must be non-decreasing");
    for (int k = 0; k < ptrow[n]; k++) CHECK_ARG(indcol[k] >= 0 && indcol[k] < ncols, "column index outside [0, ncols)");
    SsPlanHost P;
    build_sstream_plan(n, ncols, ptrow, indcol, ss_max_padding(), P, true, shift, ghost_lo, ghost_hi);
    *eligible = P.eligible ? 1 : 0;
    if (rounds) *rounds = P.rounds;
    if (steps) *steps = P.steps;
    if (padding) *padding = ptrow[n] > 0 ? (double)P.pad_places / (double)ptrow[n] : 0.0;
    if (ghost_workgroups) *ghost_workgroups = 0;
    if (rounds_min_max) rounds_min_max[0] = rounds_min_max[1] = 0;
    if (!P.eligible) {
        g_err = std::string("not eligible: ") + P.why;
        return MI_OK;
    }
    if (const char* bad = check_sstream_plan(P, n, ptrow, indcol, ghost_lo, ghost_hi)) return fail(MI_ERR_STATE, std::string("sliced-stream plan: ") + bad);
    int gw = 0, rmin = 0x7fffffff, rmax = 0, rmax_ghost = 0, pmin = 0x7fffffff, pmax = 0;
    for (int g = 0; g < P.nwg; g++) {
        const int c = P.rptr[g + 1] - P.rptr[g];
        gw += P.wg_halo[g];
        rmin = std::min(rmin, c);
        rmax = std::max(rmax, c);
        if (P.wg_halo[g]) rmax_ghost = std::max(rmax_ghost, c);
        else { pmin = std::min(pmin, c); pmax = std::max(pmax, c); }
    }
    // the dealing's promises: the shares of the workgroups that read no ghost differ by at most one round, a ghost-reading workgroup
    // never carries the longest share when there is more than one round per workgroup to deal, and (checked in the replay above) takes
    // all its columns in with its first fill
    if (pmax > 0 && pmax - pmin > 1) return fail(MI_ERR_STATE, "sliced-stream plan: the workgroups' shares differ by more than a round");
    if (gw && gw < P.nwg && rmax > 1 && rmax_ghost >= rmax && P.rounds >= 2 * P.nwg) return fail(MI_ERR_STATE, "sliced-stream plan: a ghost-reading workgroup carries the longest share");
    if (ghost_lo < ghost_hi && !P.fusable) g_err = "eligible, but a ghost-reading workgroup's columns do not fit its first fill: the fused step keeps the ring kernel";
    if (ghost_workgroups) *ghost_workgroups = gw;
    if (rounds_min_max) { rounds_min_max[0] = rmin; rounds_min_max[1] = rmax; }
    return MI_OK;
}

// the cut-ring form's plan (spmv_sstream_mw.hpp) built as mi_csr_create would and replayed against the matrix (host only: no device needed)
extern "C" int mi_sstream_mw_plan_probe(int n, int ncols, const int* ptrow, const int* indcol, int shift, int* eligible, int* rounds, long long* steps, double* padding)
{
    CHECK_ARG(n >= 0 && ncols >= 0 && ptrow && ptrow[0] == 0 && eligible, "bad argument");
    CHECK_ARG(shift == 0 || shift == 1, "shift must be 0 or 1");
    CHECK_ARG(ptrow[n] == 0 || indcol, "indcol is null");
    for (int i = 0; i < n; i++) CHECK_ARG(ptrow[i] <= ptrow[i + 1], "ptrow must be non-decreasing");
    for (int k = 0; k < ptrow[n]; k++) CHECK_ARG(indcol[k] >= 0 && indcol[k] < ncols, "column index outside [0, ncols)");
    SsMwPlanHost P;
    build_sstream_mw_plan(n, ncols, ptrow, indcol, ss_max_padding(), P, shift);
    *eligible = P.eligible ? 1 : 0;
    if (rounds) *rounds = P.rounds;
    if (steps) *steps = P.steps;
    if (padding) *padding = ptrow[n] > 0 ? (double)P.pad_places / (double)ptrow[n] : 0.0;
    if (!P.eligible) {
        g_err = std::string("not eligible: ") + P.why;
        return MI_OK;
    }
    if (const char* bad = check_sstream_mw_plan(P, n, ptrow, indcol)) return fail(MI_ERR_STATE, std::string("cut-ring sliced-stream plan: ") + bad);
    return MI_OK;
}

extern "C" int mi_csr_block4_structure(int n, const int* ptrow, const int* indcol, int* is_blocked, long long* nblocks)
{
    CHECK_ARG(n >= 0 && ptrow && is_blocked, "bad argument");
    CHECK_ARG(ptrow[n] == 0 || indcol, "indcol is null");
    // values are irrelevant to the structure test: hand the converter a dummy array of the right length
    std::vector<double> dummy((size_t)ptrow[n], 0.0);
    std::vector<int> bptr, bcol;
    std::vector<double> bval;
    const bool ok = csr_to_bcsr4_exact(n, ptrow, indcol, dummy.data(), bptr, bcol, bval);
    *is_blocked = ok ? 1 : 0;
    if (nblocks) *nblocks = ok ? (long long)bcol.size() : 0;
    return MI_OK;
}

extern "C" int mi_csr_set_nontemporal(mi_csr_t A, int ring_nt, int stream_nt)
{
    CHECK_ARG(A, "null handle");
    if (A->inner) A = A->inner;
    if (ring_nt >= 0) A->ring.nt = ring_nt != 0 && A->ring.d_slots;
    if (stream_nt >= 0) A->stream_nt = stream_nt != 0;
    return MI_OK;
}

extern "C" int mi_csr_ring_info(mi_csr_t A, int* config_id, int* runs, int* runs_not_ringable, double* nnz_fraction_ringable)
{
    CHECK_ARG(A, "null handle");
    if (A->inner) A = A->inner;
    if (config_id) *config_id = A->ring.cfg.id;
    if (runs) *runs = A->ring.wgs;
    if (runs_not_ringable) *runs_not_ringable = A->ring.bad_runs;
    if (nnz_fraction_ringable) *nnz_fraction_ringable = A->ring.ok_fraction;
    return MI_OK;
}

extern "C" int mi_csr_tile_info(mi_csr_t A, int* built, int* nblk, double* unique_per_nnz, double us[2], int* nt)
{
    CHECK_ARG(A, "null handle");
    if (A->inner) A = A->inner;
    if (built) *built = A->tile.d_desc != nullptr;
    if (nblk) *nblk = A->tile.nblk;
    if (unique_per_nnz) *unique_per_nnz = A->tile.unique_per_nnz;
    if (us) {
        us[0] = A->tune_us[MI_KERNEL_TILE][0];
        us[1] = A->tune_us[MI_KERNEL_TILE][1];
    }
    if (nt) *nt = A->tile.nt;
    return MI_OK;
}

extern "C" int mi_csr_placement_info(mi_csr_t A, int* n_values, int* n_total, double* us, int cap)
{
    CHECK_ARG(A && cap >= 0 && (cap == 0 || us), "bad argument");
    if (A->inner) A = A->inner;
    if (n_values) *n_values = A->place_draws_coef;
    if (n_total) *n_total = (int)A->place_us.size();
    for (int i = 0; i < cap && i < (int)A->place_us.size(); i++) us[i] = A->place_us[i];
    return MI_OK;
}

// Placement draws for the caller's vectors (include/mi355_spmv.h; profiles/NOTES.md §4.12)
extern "C" int mi_vec_alloc_placed(mi_csr_t A, int nvec, int draws, double** d_vecs, double* us, int cap, int* n_us)
{
    CHECK_ARG(A && nvec >= 1 && d_vecs && cap >= 0 && (cap == 0 || us), "bad argument");
    int rc = need_device();
    if (rc) return rc;
    if (n_us) *n_us = 0;
    const size_t bytes = sizeof(double) * placed_vector_len(A->n, A->ncols);
    const int npairs = (nvec + 1) / 2;
    if (draws > 64) draws = 64;
    const bool timed = draws > npairs && A->nnz >= kLargeNnz && A->n == A->ncols;
    const int cand = timed ? draws : npairs;
    std::vector<double*> xs((size_t)cand, nullptr), ys((size_t)cand, nullptr);
    auto release = [&]() {
        for (double* q : xs) if (q) (void)hipFree(q);
        for (double* q : ys) if (q) (void)hipFree(q);
    };
    for (int c = 0; c < cand; c++) { // pairs one after the other: the levels come in windows of consecutive allocations
        hipError_t e = hipSuccess;
        if (c == 0 && A->kept_x && A->kept_y) { // the pair the create-time placement draws were timed on (ownership leaves the handle)
            xs[0] = A->kept_x.own.release();
            ys[0] = A->kept_y.own.release();
        } else {
            e = hipMalloc(&xs[c], bytes);
            if (e == hipSuccess) e = hipMalloc(&ys[c], bytes);
        }
        // (the kept pair too: its y holds what the draws' products left there)
        if (e == hipSuccess) e = hipMemset(xs[c], 0, bytes);
        if (e == hipSuccess) e = hipMemset(ys[c], 0, bytes);
        if (e != hipSuccess) {
            release();
            return fail(e == hipErrorOutOfMemory ? MI_ERR_ALLOC : MI_ERR_HIP, std::string("mi_vec_alloc_placed: ") + hipGetErrorString(e));
        }
    }
    std::vector<int> order((size_t)cand);
    for (int c = 0; c < cand; c++) order[c] = c;
    if (timed) {
        std::vector<double> t((size_t)cand, 0.0);
        int rct;
        {
            LaunchTimer tm;
            rct = tm.init();
            for (int c = 0; c < cand && !rct; c++) rct = tm.time(4, 10, [&] { return mi_spmv_dev(A, xs[c], ys[c], nullptr); }, &t[c]);
        }
        if (rct) {
            release();
            return fail(MI_ERR_HIP, "mi_vec_alloc_placed: timing a candidate pair failed");
        }
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return t[a] < t[b]; });
        for (int c = 0; c < cand && c < cap; c++) us[c] = t[c];
        if (n_us) *n_us = std::min(cand, cap);
        // y = A * 0 left zeros in the y candidates (or NaN-free garbage if A holds infinities): hand out zero-filled vectors
        for (int c = 0; c < cand; c++) (void)hipMemset(ys[c], 0, bytes);
        (void)hipDeviceSynchronize();
    }
    for (int v = 0; v < nvec; v++) { // vector 2k and 2k + 1 = the x and the y of the k-th fastest pair
        double*& slot = (v & 1) ? ys[order[v >> 1]] : xs[order[v >> 1]];
        d_vecs[v] = slot;
        slot = nullptr;
    }
    release(); // everything not handed out
    return MI_OK;
}

extern "C" int mi_vec_free_placed(double* d_vec)
{
    if (d_vec) HIP_TRY(hipFree(d_vec));
    return MI_OK;
}

extern "C" int mi_csr_mring_info(mi_csr_t A, int* built, int* runs, int* runs_not_served, double* nnz_fraction_served, double us[2], int* nt)
{
    CHECK_ARG(A, "null handle");
    if (A->inner) A = A->inner;
    if (built) *built = A->mring.d_plan != nullptr;
    if (runs) *runs = A->mring.nruns;
    if (runs_not_served) *runs_not_served = A->mring.bad_runs;
    if (nnz_fraction_served) *nnz_fraction_served = A->mring.ok_fraction;
    if (us) {
        us[0] = A->tune_us[MI_KERNEL_MRING][0];
        us[1] = A->tune_us[MI_KERNEL_MRING][1];
    }
    if (nt) *nt = A->mring.nt;
    return MI_OK;
}

extern "C" int mi_mring_plan_probe(int n, const int* ptrow, const int* indcol, int* nblk, int* runs, int* runs_not_served,
                                   double* nnz_fraction_served, long long* window_restarts)
{
    CHECK_ARG(n >= 0 && ptrow && ptrow[0] == 0, "bad matrix");
    CHECK_ARG(ptrow[n] == 0 || indcol, "indcol is null");
    MringPlanHost P;
    build_mring_plan(n, ptrow, indcol, P);
    if (const char* bad = check_mring_plan(P, n, ptrow, indcol)) return fail(MI_ERR_STATE, std::string("mring plan: ") + bad);
    if (nblk) *nblk = P.nblk;
    if (runs) *runs = P.nruns;
    if (runs_not_served) *runs_not_served = P.bad_runs;
    if (nnz_fraction_served) *nnz_fraction_served = ptrow[n] ? 1.0 - (double)P.bad_nnz / (double)ptrow[n] : 0.0;
    if (window_restarts) *window_restarts = P.restarts;
    return MI_OK;
}

extern "C" int mi_mring_plan_deal_probe(int n, const int* ptrow, const int* indcol, int* table_len, int* run_blocks, int cap)
{
    CHECK_ARG(n >= 0 && ptrow && ptrow[0] == 0 && table_len && cap >= 0 && (cap == 0 || run_blocks), "bad argument");
    CHECK_ARG(ptrow[n] == 0 || indcol, "indcol is null");
    MringPlanHost P;
    build_mring_plan(n, ptrow, indcol, P);
    *table_len = P.wgs;
    for (int g = 0; g < P.wgs && g < cap; g++) run_blocks[g] = P.run_rng[2 * g + 1] - P.run_rng[2 * g];
    return MI_OK;
}

extern "C" int mi_tile_plan_probe(int n, const int* ptrow, const int* indcol, int threads, int* nblk, long long* distinct_total,
                                  int* max_distinct, long long* nnz_listed)
{
    CHECK_ARG(n >= 0 && ptrow && ptrow[0] == 0, "bad matrix");
    CHECK_ARG(ptrow[n] == 0 || indcol, "indcol is null");
    TilePlanHost P;
    build_tile_plan(n, ptrow, indcol, P, kTileNnzb, threads);
    if (const char* bad = check_tile_plan(P, n, ptrow, indcol)) return fail(MI_ERR_STATE, std::string("tile plan: ") + bad);
    if (nblk) *nblk = P.nblk;
    if (distinct_total) *distinct_total = P.nblk > 0 ? (long long)P.ulist.size() - kTileThreads : 0;
    if (max_distinct) *max_distinct = P.max_unique;
    if (nnz_listed) *nnz_listed = P.listed;
    return MI_OK;
}

extern "C" int mi_ring_plan_lean(int n, const int* ptrow, const int* indcol, int config_id, int* lean)
{
    CHECK_ARG(n >= 0 && ptrow && lean && config_id >= 1 && config_id <= kNumRingConfigs, "bad argument");
    std::vector<int> row_min, row_max;
    row_ranges(n, ptrow, indcol, row_min, row_max);
    RingPlanHost P;
    build_ring_plan(kRingConfigs[config_id - 1], n, ptrow, row_min.data(), row_max.data(), P);
    *lean = P.lean && P.cfg.id == 4 && P.bad_runs == 0;
    return MI_OK;
}

// host-only: the census of the plan mi_csr_create builds for this matrix and configuration (ring_plan.hpp: ring_plan_census) — the
// same planner call, the same row alignment rule (large_row_align)
static_assert(kRingCensusLen == MI_RING_CENSUS_LEN && kMringCensusLen == MI_MRING_CENSUS_LEN, "include/mi355_spmv.h lists the counters");
extern "C" int mi_ring_plan_census(int n, const int* ptrow, const int* indcol, int config_id, long long* counters, int cap)
{
    CHECK_ARG(n >= 0 && ptrow && ptrow[0] == 0 && config_id >= 1 && config_id <= kNumRingConfigs && counters, "bad argument");
    CHECK_ARG(cap >= kRingCensusLen, "counters holds fewer than MI_RING_CENSUS_LEN entries");
    const long long nnz = ptrow[n];
    CHECK_ARG(nnz == 0 || indcol, "indcol is null");
    std::vector<int> row_min, row_max;
    row_ranges(n, ptrow, indcol, row_min, row_max);
    RingPlanHost P;
    build_ring_plan(kRingConfigs[config_id - 1], n, ptrow, row_min.data(), row_max.data(), P, 0, 0, large_row_align(nnz));
    ring_plan_census(P, indcol, counters);
    return MI_OK;
}

// ... and of the multi-window plan (mring_plan.hpp: mring_plan_census)
extern "C" int mi_mring_plan_census(int n, const int* ptrow, const int* indcol, long long* counters, int cap)
{
    CHECK_ARG(n >= 0 && ptrow && ptrow[0] == 0 && counters, "bad argument");
    CHECK_ARG(cap >= kMringCensusLen, "counters holds fewer than MI_MRING_CENSUS_LEN entries");
    CHECK_ARG(ptrow[n] == 0 || indcol, "indcol is null");
    MringPlanHost P;
    build_mring_plan(n, ptrow, indcol, P, large_row_align(ptrow[n]));
    mring_plan_census(P, n, indcol, counters);
    return MI_OK;
}

// ... and of the row blocks of the stream kernel (get_table's call) or the tile kernel (build_tile's call): rowblock_census.hpp
static_assert(kRowblockCensusLen == MI_ROWBLOCK_CENSUS_LEN, "include/mi355_spmv.h lists the counters");
extern "C" int mi_rowblock_census(int n, const int* ptrow, const int* indcol, int which, long long* counters, int cap)
{
    CHECK_ARG(n >= 0 && ptrow && ptrow[0] == 0 && counters && (which == MI_KERNEL_STREAM || which == MI_KERNEL_TILE), "bad argument");
    CHECK_ARG(cap >= kRowblockCensusLen, "counters holds fewer than MI_ROWBLOCK_CENSUS_LEN entries");
    for (int i = 0; i < n; i++) CHECK_ARG(ptrow[i] <= ptrow[i + 1], "ptrow must be non-decreasing");
    const long long nnz = ptrow[n];
    CHECK_ARG(nnz == 0 || indcol, "indcol is null");
    const bool tile = which == MI_KERNEL_TILE;
    const int nnzb = tile ? kTileNnzb : 1024, threads = tile ? kTileThreads : kWG, row_align = row_block_align(nnz);
    std::vector<int> rows, ptrs, ucount;
    std::vector<char> why;
    build_row_blocks(n, ptrow, nnzb, 4 * threads, rows, ptrs, row_align, kRowBlockKeepEighths, &why);
    const int nblk = (int)rows.size() - 1;
    if (tile) {
        TilePlanHost P;
        build_tile_plan(n, ptrow, indcol, P, kTileNnzb, 0, row_align);
        if (const char* bad = check_tile_plan(P, n, ptrow, indcol)) return fail(MI_ERR_STATE, std::string("tile plan: ") + bad);
        if (P.nblk != nblk) return fail(MI_ERR_STATE, "tile plan: its blocks are not those of build_row_blocks");
        ucount.resize((size_t)nblk);
        for (int b = 0; b < nblk; b++) {
            if (P.desc[(size_t)4 * b] != rows[b] || P.desc[(size_t)4 * b + 1] != ptrs[b]) return fail(MI_ERR_STATE, "tile plan: its blocks are not those of build_row_blocks");
            ucount[b] = P.desc[(size_t)4 * (b + 1) + 2] - P.desc[(size_t)4 * b + 2];
        }
    }
    rowblock_census(n, ptrow, nnzb, threads, row_align, rows, ptrs, why, tile ? ucount.data() : nullptr, tile && tile_wants_skew(n, ptrow), counters);
    if ((long long)cap >= (long long)kRowblockCensusLen + nblk + 1) // room for the row starts: blocks + 1 entries behind the counters
        for (int b = 0; b <= nblk; b++) counters[kRowblockCensusLen + b] = rows[b];
    return MI_OK;
}

extern "C" int mi_csr_stream_info(mi_csr_t A, int* nblk, int* row_align)
{
    CHECK_ARG(A, "null handle");
    if (A->inner) A = A->inner;
    BlockTable* T = nullptr;
    int rc = need_device();
    if (rc || (rc = get_table(A, 1024, &T))) return rc;
    if (nblk) *nblk = T->nblk;
    if (row_align) *row_align = T->row_align;
    return MI_OK;
}

extern "C" int mi_csr_ring_shape_info(mi_csr_t A, int* blocks, int* lean, int* depth, double* us_aligned, double* us_unaligned)
{
    CHECK_ARG(A, "null handle");
    if (A->inner) A = A->inner;
    if (blocks) *blocks = A->ring.nblk;
    if (lean) *lean = A->ring.lean;
    if (depth) *depth = A->ring.cfg.depth;
    if (us_aligned) *us_aligned = A->tune_us_ring_aligned;
    if (us_unaligned) *us_unaligned = A->tune_us_ring_unaligned;
    return MI_OK;
}

extern "C" int mi_csr_set_kernel(mi_csr_t A, int kernel_id)
{
    CHECK_ARG(A, "null handle");
    if (A->inner) A = A->inner;
    CHECK_ARG(kernel_id >= MI_KERNEL_AUTO && kernel_id <= MI_KERNEL_SSTREAM, "unknown kernel id");
    if (kernel_id == MI_KERNEL_SSTREAM && !A->ss.dev.val && A->nnz > 0 && A->d_indcol && !env_is("MI355_SSTREAM", "0")) {
        // not built at create (a small matrix) or released after losing the create-time measurement: built on request
        int rc = need_device();
        if (rc) return rc;
        std::vector<int> back((size_t)A->nnz);
        HIP_TRY(hipMemcpy(back.data(), A->d_indcol, sizeof(int) * (size_t)A->nnz, hipMemcpyDeviceToHost));
        if ((rc = build_sstream(A, A->h_ptrow.data(), back.data(), A->ghost_lo, A->ghost_hi))) return rc;
        A->ss.asked = true;
    }
    if (kernel_id == MI_KERNEL_SSTREAM && !A->ss.dev.val)
        return fail(MI_ERR_UNSUPPORTED, "MI_KERNEL_SSTREAM: the handle holds no sliced copy (the matrix pads too much or its rows do "
                                        "not fit the sliding LDS window: mi_sstream_plan_probe says which)");
    if (kernel_id == MI_KERNEL_BCSR4 && !A->blocked)
        return fail(MI_ERR_UNSUPPORTED, "MI_KERNEL_BCSR4: this matrix has no exact 4x4 block structure (or is row-mapped)");
    if (kernel_id == MI_KERNEL_TILE) { // the plan is built on first request if mi_csr_create did not keep one
        int rc = need_device();
        if (rc) return rc;
        if ((rc = build_tile(A, nullptr))) return rc;
    }
    if (kernel_id == MI_KERNEL_MRING) {
        int rc = need_device();
        if (rc) return rc;
        if ((rc = build_mring(A, nullptr, large_row_align(A->nnz)))) return rc;
    }
    A->kernel = kernel_id;
    HIP_TRY(hipStreamSynchronize(nullptr)); // (whatever a plan built on request queued on the null stream: usable from any stream on return)
    return MI_OK;
}

extern "C" int mi_csr_get_kernel(mi_csr_t A, int* kernel_id)
{
    CHECK_ARG(A && kernel_id, "null argument");
    if (A->inner) A = A->inner;
    *kernel_id = resolve_kernel(A);
    return MI_OK;
}

extern "C" const char* mi_csr_kernel_name(mi_csr_t A)
{
    if (!A) return "";
    if (A->inner) A = A->inner;
    switch (resolve_kernel(A)) {
    case MI_KERNEL_STREAM: return A->stream_nt ? "spmv_csr_stream<1024, true>" : "spmv_csr_stream<1024, false>";
    case MI_KERNEL_RING: { // the name rocprofv3 prints for the instantiation launch_ring picks
        static thread_local char nm[128];
        const RingConfig& c = A->ring.cfg;
        snprintf(nm, sizeof nm, "spmv_csr_ring<%d, %d, %d, %d, %d, %s, %s, %s, false, %s, false>", c.threads, c.nnzb, c.ring, c.depth, kRingMaxB,
                 A->d_rowmap ? "true" : "false", A->ring.nt ? "true" : "false", A->ring.skew ? "true" : "false",
                 A->ring.lean && c.threads == 256 && c.depth != 3 ? "true" : "false");
        return nm;
    }
    case MI_KERNEL_ROWPAR: return "spmv_csr_rowpar";
    case MI_KERNEL_BCSR4: {
        const mi_bcsr4_s* B = A->blocked;
        static const char* const sell_names[4] = {"spmv_bcsr4_sell<8, true, 0, 2, 4>", "spmv_bcsr4_sell<8, false, 0, 2, 4>", "spmv_bcsr4_sell<4, true, 0, 2, 8>", "spmv_bcsr4_sell<12, true, 0, 2, 4>"};
        if (B && B->sell_form >= 0 && B->sell.val) return sell_names[B->sell_form & 3];
        return B && B->use_tile && B->tl.ptr ? "spmv_bcsr4_tile<2>" : "spmv_bcsr4<2>";
    }
    case MI_KERNEL_MRING: {
        static thread_local char nm[96];
        snprintf(nm, sizeof nm, "spmv_csr_mring<%d, %d, %d, %d, %s, %s, %s>", kMringThreads, kMringNnzb, A->mring.depth, kMringMaxB,
                 A->d_rowmap ? "true" : "false", A->mring.nt ? "true" : "false", A->mring.skew ? "true" : "false");
        return nm;
    }
    case MI_KERNEL_SSTREAM: {
        static thread_local char nm[64];
        if (A->ss.mw) snprintf(nm, sizeof nm, "spmv_sstream_mw<%d, %s>", A->ss.deep ? 12 : 8, A->ss.nt ? "true" : "false");
        else snprintf(nm, sizeof nm, "spmv_sstream<%d, %s, 0>", A->ss.deep ? 12 : 8, A->ss.nt ? "true" : "false");
        return nm;
    }
    case MI_KERNEL_TILE: {
        static thread_local char nm[64];
        snprintf(nm, sizeof nm, "spmv_csr_tile<%d, %s, %s>", kTileNnzb, A->tile.nt ? "true" : "false", A->tile.skew ? "true" : "false");
        return nm;
    }
    default: return "";
    }
}
extern "C" int mi_spmv_dev(mi_csr_t A, const double* d_x, double* d_y, mi_stream_t s)
{
    CHECK_ARG(A, "null handle");
    CHECK_ARG(A->n == 0 || (d_x && d_y), "null vector");
    return launch_spmv(A, d_x, d_y, (hipStream_t)s);
}

extern "C" int mi_spmv(mi_csr_t A, const double* x, double* y)
{
    CHECK_ARG(A, "null handle");
    CHECK_ARG(A->n == 0 || (x && y), "null vector");
    if (A->mapped) return fail(MI_ERR_UNSUPPORTED, "mapped matrices are device-only (use mi_spmv_dev)");
    if (A->n == 0) return MI_OK;
    if (!A->d_x) HIP_TRY(A->d_x.alloc((size_t)(A->ncols > 0 ? A->ncols : 1)));
    if (!A->d_y) HIP_TRY(A->d_y.alloc((size_t)A->n));
    HIP_TRY(hipMemcpy(A->d_x, x, sizeof(double) * (size_t)A->ncols, hipMemcpyHostToDevice));
    int rc = launch_spmv(A, A->d_x, A->d_y, nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(y, A->d_y, sizeof(double) * (size_t)A->n, hipMemcpyDeviceToHost));
    return MI_OK;
}

// ---------------------------------------------------------------- matrix powers
extern "C" int mi_spmk_dev(mi_csr_t A, int k, const double* d_x, double* const* d_y_out, mi_stream_t s)
{
    CHECK_ARG(A, "null handle");
    if (k < 1 || k > MI_MAX_POWERS) return fail(MI_ERR_UNSUPPORTED, "k must be in 1..MI_MAX_POWERS");
    CHECK_ARG(A->n == A->ncols, "matrix powers need a square matrix");
    CHECK_ARG(!A->mapped, "matrix powers need an unmapped matrix");
    CHECK_ARG(d_y_out, "null output array");
    if (A->n == 0) return MI_OK;
    for (int p = 0; p < k; p++) CHECK_ARG(d_y_out[p], "null output vector");
    if (A->inner) {
        // the whole chain in the new numbering (each power feeds the next without leaving it), then every power scattered to
        // the caller's numbering
        int rc = A->d_pp.grow(k, (size_t)A->n);
        if (rc) return rc;
        double* xp = nullptr;
        if ((rc = reorder_scratch(A, (hipStream_t)s, &xp))) return rc;
        if ((rc = gather_perm(A, d_x, xp, (hipStream_t)s))) return rc;
        if ((rc = spmk_unmapped(A->inner, k, xp, A->d_pp.ptr.data(), (hipStream_t)s))) return rc;
        for (int p = 0; p < k; p++)
            if ((rc = scatter_perm(A, A->d_pp.ptr[p], d_y_out[p], (hipStream_t)s))) return rc;
        return MI_OK;
    }
    return spmk_unmapped(A, k, d_x, d_y_out, (hipStream_t)s);
}

extern "C" int mi_spmk(mi_csr_t A, int k, const double* x, double* const* y_out)
{
    CHECK_ARG(A, "null handle");
    if (k < 1 || k > MI_MAX_POWERS) return fail(MI_ERR_UNSUPPORTED, "k must be in 1..MI_MAX_POWERS");
    CHECK_ARG(A->n == A->ncols, "matrix powers need a square matrix");
    CHECK_ARG(A->n == 0 || (x && y_out), "null vector");
    if (A->n == 0) return MI_OK;
    if (!A->d_x) HIP_TRY(A->d_x.alloc((size_t)A->ncols));
    if (int rc = A->d_pow.grow(k, (size_t)A->n)) return rc;
    HIP_TRY(hipMemcpy(A->d_x, x, sizeof(double) * (size_t)A->ncols, hipMemcpyHostToDevice));
    int rc = mi_spmk_dev(A, k, A->d_x, A->d_pow.ptr.data(), nullptr);
    if (rc) return rc;
    for (int p = 0; p < k; p++) {
        CHECK_ARG(y_out[p], "null output vector");
        HIP_TRY(hipMemcpy(y_out[p], A->d_pow.ptr[p], sizeof(double) * (size_t)A->n, hipMemcpyDeviceToHost));
    }
    return MI_OK;
}
