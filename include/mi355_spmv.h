/*
 * mi355_spmv.h — the C-ABI boundary of the MI355X-native CSR SpMV /
 * matrix-powers path (libmi355spmv.so).
 *
 * Plain C: opaque handles, raw pointers and sizes, int status codes.  These are
 * the entry points a binding of the reference's hot path attaches to; the
 * reference interface each one stands behind is cited as file:line relative to
 * aantoine890/navierstokes.  The C++ drop-in with the reference's exact
 * mpk/SpMV.h names and signatures (include/SpMV.h, libmpk_mi355.so) is a thin
 * layer over this header; INTEGRATION.md shows both bindings.
 *
 * Conventions
 *   - every function returns MI_OK (0) or an MI_ERR_* code; mi_last_error()
 *     gives the detail of the last failure on the calling thread.  The
 *     reference's functions are void and unchecked (mpk/SpMV.h:52-66); the
 *     C++ shim aborts with the message on a non-zero status.
 *   - indices are 0-based int32, values are IEEE double (mpk/SpMV.h:18-24).
 *   - the caller owns every buffer it passes; the library copies the matrix to
 *     the device at create time and never retains caller memory.  Output
 *     vectors are fully overwritten (as mpk/SpMV.cpp:13, mpk/SpM2V.cpp:85-86).
 *   - "*_dev" entry points take DEVICE pointers (HBM-resident vectors) and a
 *     hipStream_t passed as void*; they enqueue work and return without
 *     synchronising.  The others take HOST pointers, copy in/out and
 *     synchronise — the semantics of the reference's CPU functions.
 *   - arithmetic: each row of y = A x is ONE sequential fma chain in CSR order,
 *     bit-identical to the reference's SpMV_CSR_OPT / SpMV_CSR_FMA
 *     (mpk/SpMV.cpp:23-56) for every matrix and every kernel id.
 *   - there is no CPU fallback: without a usable HIP device the compute entry
 *     points fail with MI_ERR_NODEVICE.
 */
#ifndef MI355_SPMV_H
#define MI355_SPMV_H

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_SPMV_VERSION 501 /* 0.5.1: mi_bcsr4_spmm_info writes us[5] since 0.4 (it was us[4] in 0.3: a caller built against 0.3 must be rebuilt); 0.5 adds
                                * mi_sstream_plan_probe_ex, mi_part_kernel_name, mi_part_sends_contiguous and refills sliced copies inside mi_*_update_values*;
                                * 0.5.1 adds mi_sstream_mw_plan_probe (nothing changed for a caller built against 0.5.0); mi_bilu4dev_* (the
                                * device refactor of the block ILU) and mi_dilu4dev_* (the device refactor of the block DILU) were added
                                * without a version change: nothing existing changed */

enum {
    MI_OK = 0,
    MI_ERR_ARG = 1,         /* null pointer, negative size, inconsistent CSR */
    MI_ERR_NODEVICE = 2,    /* no HIP device / driver */
    MI_ERR_HIP = 3,         /* a HIP runtime call failed (see mi_last_error) */
    MI_ERR_ALLOC = 4,       /* host or device allocation failed */
    MI_ERR_UNSUPPORTED = 5, /* e.g. k outside 1..MI_MAX_POWERS */
    MI_ERR_STATE = 6        /* handle used before it was finalised / wrong device */
};

#define MI_MAX_POWERS 16

typedef struct mi_csr_s* mi_csr_t;   /* device-resident CSR matrix (struct csrmatrix, mpk/SpMV.h:18-24) */
typedef struct mi_bcsr4_s* mi_bcsr4_t; /* device-resident 4x4 BCSR matrix (struct bcsr4x4_matrix, mpk/SpMV.h:26-33) */
typedef struct mi_part_s* mi_part_t; /* one rank's share of a row-partitioned matrix */
typedef void* mi_stream_t;           /* hipStream_t; NULL = the default stream */

/* kernel ids for mi_csr_set_kernel (all produce the same bits) */
enum {
    MI_KERNEL_AUTO = 0,    /* the fastest eligible kernel, measured on the handle at mi_csr_create (mi_csr_tune_detail) */
    MI_KERNEL_STREAM = 1,  /* row-block CSR-stream, x gathered through L1/L2 (any matrix) */
    MI_KERNEL_RING = 2,    /* persistent workgroups, sliding x window in LDS, pipelined matrix stream */
    MI_KERNEL_ROWPAR = 3,  /* one thread per row straight from global memory (reference shape; slow) */
    MI_KERNEL_BCSR4 = 4,   /* the BCSR 4x4 kernel on a blocked copy made at mi_csr_create; available only when the
                            * CSR matrix has exact 4x4 node-block structure (FE matrices), where it returns the
                            * same bits from 8.25 instead of 12 matrix bytes per nonzero */
    MI_KERNEL_MRING = 6,   /* the ring kernel with five independent sliding windows: 3-D mesh operators, whose rows reach into a
                            * few narrow column clusters whole mesh planes apart (any mesh size) */
    MI_KERNEL_SSTREAM = 7, /* (round 4) the matrix as ONE contiguous stream per wave: a sliced copy (128-row slices, 16 bytes of values per
                            * lane and step, a 32-bit word of LDS slots and flags), a lane per row pair, x in an LDS ring that slides with
                            * the rows, y parked in LDS — banded matrices with near-uniform row lengths (spmv_sstream.hpp) */
    MI_KERNEL_TILE = 5     /* per row block the DISTINCT columns are gathered once into an LDS tile, nonzeros address it
                            * through a 16-bit stream: wide-band matrices whose neighbouring rows share columns (P1
                            * operators on unstructured 3-D meshes), which the ring's contiguous window cannot hold */
};

/* ---- library / device ------------------------------------------------- */
int mi_version(void);
const char* mi_strerror(int status);
const char* mi_last_error(void);
int mi_device_count(int* count);
int mi_set_device(int device);
int mi_device_synchronize(void);
/* Evict the GPU's L2s and 256 MiB Infinity Cache: the device analogue of flush_cache(), mpk/utils.cpp:146-154, which the
 * reference calls before every timed kernel.  A 512 MiB device fill (the reference writes its buffer too) followed by a
 * 512 MiB READ sweep of a second buffer and a synchronise: the fill alone leaves the Infinity Cache full of dirty lines
 * whose write-back the next kernel pays for (≈11 us on a 1 GB product); behind the read sweep the caches hold clean lines
 * of a buffer nobody uses.  MI355_FLUSH_FILL_ONLY=1 restores the fill-only form. */
int mi_flush_cache(void);
/* The same eviction enqueued on stream s WITHOUT the closing synchronise: a product enqueued right behind it starts on cold
 * caches but on a GPU that never went idle.  (Behind the synchronous form the device idles until the host has returned and
 * launched; a kernel started on an idle MI355X measures 8-26 us longer than the same kernel behind another one, whatever
 * the caches hold — tools/cold_probe.py.  The reference's CPU protocol has no such effect to separate.) */
int mi_flush_cache_async(mi_stream_t s);

/* ---- CSR matrix handles ------------------------------------------------ */
/* Upload a csrmatrix (mpk/SpMV.h:18-24: n, ptrow[n+1], indcol, coef; nnz taken
 * from ptrow[n], not from the possibly stale csrmatrix::nnz — mpk/utils.cpp:100).
 * ncols = length of the x vectors (n for the reference's square matrices).
 * Host pointers.  The handle is complete on return and usable from any stream,
 * non-blocking ones included (so are mi_csr_create_mapped's and mi_csr_set_kernel's). */
int mi_csr_create(int n, int ncols, const int* ptrow, const int* indcol, const double* coef, mi_csr_t* out);
/* Same, for a row subset whose results are scattered: row r of this matrix
 * writes y[rowmap[r]] (rowmap == NULL: y[r]).  Used for the interior/boundary
 * split of a partitioned matrix. */
int mi_csr_create_mapped(int n, int ncols, const int* ptrow, const int* indcol, const double* coef,
                         const int* rowmap, mi_csr_t* out);
int mi_csr_destroy(mi_csr_t A);
/* New coefficients for an UNCHANGED sparsity pattern: coef has the nnz values in the order of the
 * arrays given to mi_csr_create.  The reference's functions read the caller's live arrays on every
 * call; a handle holds a device copy, so a caller that rewrites its coefficients in place — the
 * Newton loop does that to the Jacobian every iteration, src/solve_newton.c:1245-1247 (MatCopy +
 * add_nonlinear_jacobian_terms + MatZeroRows), before KSPSolve :1265 — refreshes the copy with this
 * call: one transfer of the values; row blocks, ring plan, column stream and kernel choice depend on
 * the pattern only and are kept, the blocked copy's values are regenerated on the device.  The
 * mpk/SpMV.h shim (libmpk_mi355.so) detects such changes by itself (full content hash) and calls this. */
int mi_csr_update_values(mi_csr_t A, const double* coef);                          /* host values; synchronous */
int mi_csr_update_values_dev(mi_csr_t A, const double* d_coef, mi_stream_t s);     /* device values; asynchronous on s */
int mi_csr_dims(mi_csr_t A, int* n, int* ncols, long long* nnz);
/* Locality reordering.  The reference's matrices come from unstructured gmsh meshes (src/solve_newton.c:91-197,
 * src/benchmark_spmv.c:76-123) whose node numbering scatters a row's columns over all of x.  For a square matrix
 * that is not already served by the ring kernel and whose nonzeros lie far from the diagonal for its size,
 * mi_csr_create computes a reverse Cuthill-McKee relabelling of the NODE graph (4x4 node blocks stay together),
 * builds A' = P A P^T with every row's nonzeros in the caller's order, and keeps it if it measures faster.  The
 * permutation never shows: x is gathered into the new numbering before a product and y is written back through a
 * row map, and since a row's terms keep their order every bit of y equals the unreordered kernels' (and the
 * reference's SpMV_CSR_FMA).  A reordered handle keeps one gather buffer per stream it has multiplied on (products of one handle on
 * different streams do not share scratch; mi_spmk_dev's power buffers are per handle: one k-step at a time).
 * MI355_REORDER=0 disables, =1 forces.  *reordered = 1 if the handle computes through the relabelled twin; block = 4
 * if nodes of four rows were moved, 1 if single rows; spread = mean |column - row| in nodes before / after;
 * us_* = measured launch time of the natural-order choice and of the twin incl. its gather (0 if not measured). */
int mi_csr_reorder_info(mi_csr_t A, int* reordered, int* block, double* spread_before, double* spread_after,
                        double* us_natural, double* us_reordered);
/* ---- staying in the library's numbering (callers that own the loop) -----------------------------------------------
 * A relabelled handle pays an x gather and a mapped y store on EVERY mi_spmv_dev (random 8-byte accesses: 92 + 45 us of
 * 326 us at 5 M rows).  A caller that runs many products per matrix — a Krylov solve: src/solve_newton.c:1265 KSPSolve, one
 * MatMult per GMRES iteration on the mesh numbering of :91-197 — permutes its vectors ONCE per solve instead:
 *   mi_csr_perm              perm[old] = new (identity and *reordered = 0 for a handle that was not relabelled)
 *   mi_vec_to_internal_dev   x_int[perm[i]] = x[i]     (one gather; out of place)
 *   mi_vec_from_internal_dev x[i] = x_int[perm[i]]
 *   mi_spmv_internal_dev     y_int = A' x_int: the twin alone — no gather, no row map, no per-handle scratch
 *   mi_spmk_internal_dev     the powers chain, every power left in the internal numbering
 * The BLAS-1 entry points (mi_dot_dev, mi_axpy_dev, mi_orthogonalize_dev, mi_norm2_dev, ...) are numbering-agnostic:
 * element-wise updates commute with a permutation bit for bit; a reduction sums in index order of whatever numbering it is
 * given, so its last bits may differ between numberings (inside the bound documented at mi_dot).  Every row of y_int is the
 * same fma chain as the caller-numbering product's: un-permuting y_int gives mi_spmv_dev's bits. */
int mi_csr_perm(mi_csr_t A, int* reordered, int* perm /* [n] or NULL */);
int mi_vec_to_internal_dev(mi_csr_t A, const double* d_x, double* d_x_int, mi_stream_t s);
int mi_vec_from_internal_dev(mi_csr_t A, const double* d_x_int, double* d_x, mi_stream_t s);
int mi_spmv_internal_dev(mi_csr_t A, const double* d_x_int, double* d_y_int, mi_stream_t s);
int mi_spmk_internal_dev(mi_csr_t A, int k, const double* d_x_int, double* const* d_y_int_out, mi_stream_t s);
/* host-only: the relabelling mi_csr_create would compute; perm[old] = new (n entries) */
int mi_reorder_probe(int n, const int* ptrow, const int* indcol, int* block, int* perm, double* spread_before,
                     double* spread_after);
/* MI_KERNEL_RING on a matrix whose window does not fit is still correct (its runs take the
 * per-block path); mi_csr_ring_info reports how much of the matrix the ring serves. */
int mi_csr_set_kernel(mi_csr_t A, int kernel_id);
int mi_csr_ring_info(mi_csr_t A, int* config_id, int* runs, int* runs_not_ringable, double* nnz_fraction_ringable);
/* Shape of the ring plan in use: row blocks, whether the LEAN instantiation runs, blocks of prefetch.  Matrices of >= 20 M
 * nonzeros take row blocks cut at the nonzero count, smaller ones blocks ending on multiples of 64 rows (the first shape's
 * rate does not depend on where the caller's x and y lie in device memory, the second's does: profiles/NOTES.md §4.1).  With
 * MI355_RING_SHAPE_COMPARE=1 in the environment mi_csr_create also times the other shape on its scratch vectors
 * (microseconds per launch; 0 = not compared). */
int mi_csr_ring_shape_info(mi_csr_t A, int* blocks, int* lean, int* depth, double* us_aligned, double* us_unaligned);
/* MI_KERNEL_AUTO is decided by measurement: mi_csr_create times the candidate kernels (ring if
 * >= 90 % of the nonzeros are ring-served, stream, tile if a plan was kept, BCSR 4x4 if a blocked copy exists) on the new
 * handle, two interleaved rounds of a few launches each, and keeps the fastest.  All kernels produce
 * the same bits, so the choice never changes a result.  Reports the measured microseconds per launch
 * of the chosen temporal / non-temporal form (0 = candidate not eligible / not timed).
 * MI355_SPMV_KERNEL=ring|stream|rowpar|bcsr4|tile|mring or MI355_SPMV_AUTOTUNE=0 skip the measurement (then: ring
 * if eligible else stream, BCSR 4x4 if blocked; non-temporal loads for matrices beyond the Infinity Cache). */
int mi_csr_tune_info(mi_csr_t A, double* us_ring, double* us_stream);
/* Each candidate is timed twice, with temporal and with non-temporal loads of the matrix (a matrix
 * that fits the 256 MB Infinity Cache is faster temporal across repeated products, a larger one
 * non-temporal); us[0..4] = ring, ring non-temporal, stream, stream non-temporal, BCSR 4x4 on the
 * blocked copy (0 = not eligible / not timed); *ring_nt / *stream_nt = 1 if that kernel of this
 * handle uses non-temporal loads.  MI355_RING_NT / MI355_STREAM_NT = 0|1 force the choice,
 * MI355_AUTO_BCSR=0 disables the blocked copy. */
int mi_csr_tune_detail(mi_csr_t A, double us[5], int* ring_nt, int* stream_nt);
/* host-only: build the ring kernel's window plan and 16-bit column stream for configuration config_id (1..4,
 * ring_plan.hpp) exactly as mi_csr_create would, verify their invariants (MI_ERR_STATE names the first
 * violation) and report what the ring would serve.  Lets the planner be tested without a GPU. */
int mi_ring_plan_probe(int n, const int* ptrow, const int* indcol, int config_id, int* nblk, int* runs,
                       int* runs_not_ringable, double* nnz_fraction_ringable, int* max_slot);
/* Tile kernel (MI_KERNEL_TILE): mi_csr_create builds its plan for matrices the ring does not serve and keeps it when the
 * row blocks average at most 0.6 distinct columns per nonzero (MI355_TILE=0 never, =1 always); mi_csr_set_kernel(A,
 * MI_KERNEL_TILE) builds it on request.  *built = 1 if the handle holds a plan; unique_per_nnz = distinct columns per
 * nonzero over all row blocks; us[0..1] = measured microseconds per launch with temporal / non-temporal value loads
 * (0 = not timed); *nt = 1 if the handle's tile kernel uses non-temporal loads (MI355_TILE_NT=0|1 forces). */
int mi_csr_tile_info(mi_csr_t A, int* built, int* nblk, double* unique_per_nnz, double us[2], int* nt);
/* host-only: build the tile kernel's plan (tile_plan.hpp) exactly as mi_csr_create would, verify its invariants
 * (MI_ERR_STATE names the first violation: every slot names its nonzero's column, lists strictly ascending, 16-byte
 * aligned slot segments, over-long rows unlisted) and report its size.  threads = 0: as many as the library would use. */
int mi_tile_plan_probe(int n, const int* ptrow, const int* indcol, int threads, int* nblk, long long* distinct_total,
                       int* max_distinct, long long* nnz_listed);
/* Placement draws (profiles/NOTES.md §4.12): for matrices beyond the caches (>= 20 M nonzeros, a CSR kernel chosen) mi_csr_create times the
 * chosen kernel on a few fresh device copies of the value array, then of the 16-bit column stream, and keeps the fastest copy of
 * each — where these arrays lie in device memory moves a warm launch by up to 15 %.  us[0 .. *n_values) = microseconds per launch
 * with the value array as first allocated ([0]) and after each draw; us[*n_values .. *n_total) the same for the column stream
 * (cap = length of us; both counts 0: no draws were made).  MI355_PLACEMENT_DRAWS=0 turns the draws off, =N sets their number
 * (default 12 for the value array, capped so that the copies fit an eighth of the free device memory; half as many for the stream). */
int mi_csr_placement_info(mi_csr_t A, int* n_values, int* n_total, double* us, int cap);
/* The same for the CALLER's vectors (round 3, profiles/NOTES.md §4.12): on some MI355X boxes a product with A runs 126 or 141-143 us by which
 * physical memory its x and y were handed — in windows that follow the order of allocation — whatever the kernel does.  A solver that
 * keeps its vectors for many products (src/solve_newton.c:1265: one KSPSolve, hundreds of MatMults) can let the library place them:
 * mi_vec_alloc_placed allocates nvec device vectors of max(rows, columns) doubles each (zero-filled, 256-byte aligned) for use with A,
 * by allocating `draws` candidate PAIRS one after the other (the first: the scratch pair mi_csr_create's own placement draws were timed
 * on, kept by the handle for this call), timing y = A x on each pair (a few launches on stream 0, synchronous),
 * keeping the nvec vectors of the fastest pairs and freeing the others.  draws <= 1 (or a matrix of < 20 M nonzeros, whose products
 * live in the caches): plain allocations, nothing timed.  us[0 .. *n_us) = microseconds per launch of each candidate pair in the
 * order drawn (cap = length of us).  Vectors are released with mi_vec_free_placed (any order, any time after the handle's last use).
 * Results do not depend on where a vector lies: placement is a matter of speed only. */
int mi_vec_alloc_placed(mi_csr_t A, int nvec, int draws, double** d_vecs, double* us, int cap, int* n_us);
int mi_vec_free_placed(double* d_vec);
/* Sliced-stream kernel (MI_KERNEL_SSTREAM, spmv_sstream.hpp): mi_csr_create plans it for unmapped matrices of >= 200 000 nonzeros whose
 * rounds of 512 rows fit an 8192-column LDS window that slides forward by at most 1024 columns per round and whose 128-row slices pad by
 * at most 12 % (MI355_SSTREAM=0 never, =1 plan whatever the size), builds the sliced copy (10 bytes per nonzero beside the CSR arrays)
 * and times it — 8 / 12 steps of prefetch, non-temporal / temporal value loads — against the other candidates.  *built = 1 if the handle
 * holds the copy; *padding = padded places per nonzero; us[0..3] = microseconds per launch for D = 8 nt, D = 8 temporal, D = 12 nt,
 * D = 12 temporal (0 = not timed); *form = the variant in use (index into us).  y must be 16-byte aligned (else the handle's next-best
 * kernel runs that product).  A copy that loses the create-time measurement is released again (mi_csr_set_kernel(MI_KERNEL_SSTREAM) rebuilds
 * it on request); the sliced values follow every mi_csr_update_values* at once, on that call's stream (HIP-graph replays included).
 * A matrix whose rows name SEVERAL column neighbourhoods further apart than that window holds — a 3-D mesh operator in natural node
 * order: a node's plane and the two next to it — gets the CUT-RING form of the same kernel (spmv_sstream_mw.hpp; mi_csr_kernel_name says
 * spmv_sstream_mw<...>): four sub-rings of 2048 columns, each following one neighbourhood; eligible with at most four neighbourhoods per
 * 512-row round (gaps of more than 512 columns separate them), none wider than 2048 columns.  Same id, same info call; any y alignment.
 * MI355_SSTREAM_MW=0 disables the form. */
int mi_csr_sstream_info(mi_csr_t A, int* built, int* rounds, long long* steps, double* padding, double us[4], int* form);
/* host-only: build that plan exactly as mi_csr_create would and REPLAY it against the matrix (MI_ERR_STATE names the first violation:
 * every nonzero's slot is its column's ring slot and the column lies inside the window when its round runs; padding places are flagged).
 * *eligible = 0 with the reason in mi_last_error() when the matrix does not qualify. */
int mi_sstream_plan_probe(int n, int ncols, const int* ptrow, const int* indcol, int* eligible, int* rounds, long long* steps, double* padding);
/* the same for the two forms round 5 added: shift = 1 plans the rows one down (what mi_csr_create_mapped does for a piece whose rows go to
 * y[r + odd offset]: row pairs stay 16-byte aligned); ghost_lo < ghost_hi: columns outside [ghost_lo, ghost_hi) are ghosts (a partition's
 * combined piece, numbered [lower ghosts | owned | upper ghosts]): a workgroup whose windows hold one is marked (*ghost_workgroups counts
 * them; the fused multi-GPU step makes them push and wait first), takes its whole column range in with its first fill and gets three rounds
 * less than its share (fewer still where that range would not fit the 8192-column ring).  rounds_min_max[2] = the
 * shortest and the longest share of rounds.  The replay also checks the marks and the dealing. */
int mi_sstream_plan_probe_ex(int n, int ncols, const int* ptrow, const int* indcol, int shift, int ghost_lo, int ghost_hi, int* eligible, int* rounds,
                             long long* steps, double* padding, int* ghost_workgroups, int* rounds_min_max);
/* ... and of its cut-ring form for rows that name several column neighbourhoods (3-D mesh operators in natural node order;
 * navierstokes_amd/csrc/spmv_sstream_mw.hpp): built as mi_csr_create builds it when the one-window plan is not eligible, and replayed —
 * every nonzero must find its column at its slot of the cut ring when its round runs.  Host only. */
int mi_sstream_mw_plan_probe(int n, int ncols, const int* ptrow, const int* indcol, int shift, int* eligible, int* rounds, long long* steps, double* padding);
/* Multi-window ring kernel (MI_KERNEL_MRING, mring_plan.hpp): mi_csr_create plans it for matrices the single ring does not serve
 * and keeps the plan when it serves >= 90 % of the nonzeros (MI355_MRING=0 never, =1 always keep); mi_csr_set_kernel builds it
 * on request.  us[0..1] = measured microseconds per launch, temporal / non-temporal value loads (MI355_MRING_NT=0|1 forces). */
int mi_csr_mring_info(mi_csr_t A, int* built, int* runs, int* runs_not_served, double* nnz_fraction_served, double us[2], int* nt);
/* host-only: build that plan exactly as mi_csr_create would and REPLAY it (MI_ERR_STATE names the first violation: every
 * nonzero's 16-bit slot must hold its column when its block runs, runs cover every block once, records are consistent). */
int mi_mring_plan_probe(int n, const int* ptrow, const int* indcol, int* nblk, int* runs, int* runs_not_served,
                        double* nnz_fraction_served, long long* window_restarts);
/* host-only: the DISPATCH ORDER of that plan's runs (mring_plan.hpp: workgroup i of the grid goes to XCD i % 8, an XCD takes its
 * workgroups in order, 64 resident at a time): *table_len = the kernel's grid = 8 * per_xcd; run_blocks[x * per_xcd + j] = blocks of
 * the run the j-th workgroup of XCD x executes (0: none).  Long runs come first in every XCD's share, the short ones behind them. */
int mi_mring_plan_deal_probe(int n, const int* ptrow, const int* indcol, int* table_len, int* run_blocks, int cap);
/* host-only: would the ring plan of this pattern (configuration config_id) run the LEAN instantiation of the kernel — no block
 * inside a run bringing more than T new columns, none holding more than T rows (spmv_ring.hpp)?  The planner cuts its runs
 * at window restarts to make it so; only configuration 4 has the instantiation. */
int mi_ring_plan_lean(int n, const int* ptrow, const int* indcol, int config_id, int* lean);
/* host-only: a CENSUS of the ring plan mi_csr_create builds for this matrix under configuration config_id (the same planner call, the
 * same row alignment rule): which states of the kernel the plan reaches, so that a test can assert that its matrix sits on the limit
 * it is named for.  counters[cap], cap >= MI_RING_CENSUS_LEN, in this order ("served": a block of the pipelined loop; "PLAIN": a block
 * computed behind the loop of a kind-3 run; "wide": a block the window cannot serve; "inner": not the first block of its run):
 *  0 blocks, run table length, blocks per run of the uniform deal, runs of kind 0 / 1 / 3, non-empty runs, idle runs, shortest and longest
 *    non-empty run, 1 if the deal is the uniform one, 1 if the plan is LEAN (configuration 4), blocks of prefetch by default;
 * 13 runs of exactly 1, 2, 3, 4, 5 and 9 blocks; 19 runs holding 0, 1, 2, 3, 4 and >= 5 wide blocks, the most in one run;
 * 26 PLAIN blocks: all, first / last / neither of their run, directly behind another, holding the matrix's last row, a row longer than a
 *    block, a span wider than the ring; 34 blocks of kind-0 runs: all, wide, a row longer than a block;
 * 37 served blocks: all, of exactly NNZB and NNZB - 1 nonzeros, of exactly the row limit, of more than T rows, spanning exactly RING columns,
 *    the widest span; 44 blocks without nonzeros: all, first / last / neither of their run;
 * 48 window restarts in inner blocks: a jump ahead, a reach back, behind a PLAIN or after only empty blocks;
 * 51 new columns of inner served blocks: the most, then blocks bringing 1..T-1, T, T+1, T+2..4T-1, 4T, 4T+1, 4T+2..RING-1, RING;
 * 60 served blocks with a column at or beyond base + RING (slot wrap), inner blocks whose base advanced without a restart. */
#define MI_RING_CENSUS_LEN 62
int mi_ring_plan_census(int n, const int* ptrow, const int* indcol, int config_id, long long* counters, int cap);
/* ... and of the multi-window plan.  counters[cap], cap >= MI_MRING_CENSUS_LEN:
 *  0 blocks, run table length, runs, empty table entries, runs of kind 0 / 1 / 3, shortest and longest run, blocks of prefetch, forced cuts
 *    (a block needing more groups than the loop refills); 11 runs holding 0, 1, 2, 3, 4 and >= 5 wide blocks, the most in one run;
 * 18 PLAIN blocks: all, first / last / neither of their run, by cause: a row longer than a block, more clusters than windows, a cluster
 *    wider than a window allows; 25 blocks of kind-0 runs;
 * 26 served blocks: all, with as many clusters as windows, the most clusters, with a cluster of exactly the widest width served, the widest
 *    cluster; wide blocks one cluster over, and one column over; 33 the smallest gap that split two clusters, the largest that did not;
 * 35 blocks without nonzeros; 36 groups of inner served blocks: the most in one block, blocks with all of them, groups ending exactly at
 *    their window's wrap-around, groups continuing across it; served blocks whose columns lie on both sides of it; groups and first
 *    windows reaching past the last column. */
#define MI_MRING_CENSUS_LEN 43
int mi_mring_plan_census(int n, const int* ptrow, const int* indcol, long long* counters, int cap);
/* host-only: a CENSUS of the row blocks of the stream kernel (which = MI_KERNEL_STREAM: blocks of 1024 nonzeros, T = 256 threads,
 * the table every CSR handle falls back to) or of the tile kernel's plan (which = MI_KERNEL_TILE: blocks of 2048 nonzeros, T = 256;
 * built as mi_csr_set_kernel builds it and checked like mi_tile_plan_probe, MI_ERR_STATE names a violation), under the row-alignment
 * rule of the handle (blocks end on multiples of 64 rows below 20 M nonzeros where that keeps 7/8 of the block; MI355_STREAM_ROW_ALIGN
 * is not looked at).  counters[cap], cap >= MI_ROWBLOCK_CENSUS_LEN, in this order ("listed": a block of 1..NNZB nonzeros, computed by the
 * one-thread-per-row phase; "long": a single row of more than NNZB nonzeros, chunked through thread 0):
 *  0 blocks, the row alignment used, idle workgroups of the launch grid (8 * ceil(blocks / 8) - blocks);
 *  3 blocks without nonzeros: all, the first block of the matrix, the last, neither;
 *  7 listed blocks of exactly NNZB and NNZB - 1 nonzeros, with nonzeros % 8 == 1 and == 7, of exactly 1 nonzero;
 * 12 listed blocks of exactly 1, T, T + 1 and 4 T (the row cap) rows, the most rows in a listed block; blocks ended by the row cap and
 *    not by the nonzero limit; blocks whose end the alignment rule pulled back;
 * 19 listed blocks whose first row is empty, whose last row is empty; rows of exactly 1, 8 and 9 nonzeros in listed blocks;
 * 24 long blocks: all, of exactly NNZB + 1, 2 NNZB and 2 NNZB + 1 nonzeros, as the matrix's first row, as its last row, directly behind
 *    another long block;
 * tile only (0 for the stream kernel), U = distinct columns of a listed block:
 * 31 blocks by R = ceil(U / 256) = 1 .. 8 (the kernel's eight instantiations of tile_block);
 * 39 blocks with U == 1, U a multiple of 256, U == 256 k + 1 for a k >= 1, U == nonzeros; the largest U; 1 if the handle runs the SKEW
 *    instantiation (more than a tenth of the rows a multiple of 8 long).
 * With cap >= MI_ROWBLOCK_CENSUS_LEN + blocks + 1 the first row of every block, then n, follow the counters. */
#define MI_ROWBLOCK_CENSUS_LEN 45
int mi_rowblock_census(int n, const int* ptrow, const int* indcol, int which, long long* counters, int cap);
/* The handle's table for the stream kernel (blocks of 1024 nonzeros), built now if no product has needed it yet: its blocks and the row
 * alignment it was cut with (MI355_STREAM_ROW_ALIGN included).  mi_csr_tile_info reports the same for the tile kernel's plan. */
int mi_csr_stream_info(mi_csr_t A, int* nblk, int* row_align);
/* host-only: does this CSR pattern have the exact 4x4 node-block structure mi_csr_create looks for (n % 4 == 0,
 * the four rows of a block row hold the same columns, in aligned groups {4j..4j+3}) — i.e. will a blocked copy be
 * built and the BCSR kernel become an AUTO candidate?  *nblocks = number of 4x4 blocks if so. */
int mi_csr_block4_structure(int n, const int* ptrow, const int* indcol, int* is_blocked, long long* nblocks);
/* override the measured choice: 1 = non-temporal matrix loads, 0 = temporal, -1 = leave as is */
int mi_csr_set_nontemporal(mi_csr_t A, int ring_nt, int stream_nt);
/* calibration: microseconds per launch of a plain non-temporal read sweep over `bytes` of device memory (16-byte
 * loads, 2048 workgroups, back to back): the rate THIS GPU streams from HBM at.  MI355X boxes of one pool differ by 10-20 %
 * here; bench.py prints it beside the kernel's rate so that a roofline fraction can be read against the box it was taken on. */
int mi_stream_read_probe(long long bytes, int launches, double* us_per_launch);
int mi_csr_get_kernel(mi_csr_t A, int* kernel_id);
/* name of the HIP kernel the next mi_spmv*(A) launches (for matching rocprof rows) */
const char* mi_csr_kernel_name(mi_csr_t A);

/* ---- SpMV: y = A x  (SpMV_CSR{,_OPT,_FMA,_AVX2}, mpk/SpMV.cpp:6-85) ---- */
int mi_spmv(mi_csr_t A, const double* x, double* y);                           /* host vectors */
int mi_spmv_dev(mi_csr_t A, const double* d_x, double* d_y, mi_stream_t s);    /* device vectors */

/* ---- matrix powers: y_out[p] = A^(p+1) x, p = 0..k-1 --------------------
 * SpM2V_CSR (mpk/SpM2V.cpp:79-112: y_out[0]=y, y_out[1]=z), SpM3V / SpM4V
 * (mpk/SpMVmulti0.cpp:132-155, :189-221: all intermediate powers returned).
 * Unlike the CPU first-touch traversal, rows of A^p x that no row references
 * as a column are computed too (SURVEY.md §8a-10 caveat).
 * mi_spmk_dev is asynchronous on s — EXCEPT the first k-step of a handle at a given k (2 <= k <= 8) on an eligible ring-served
 * matrix: that call times the one-launch form against k launches (a few dozen launches on s, then a stream synchronise) and keeps
 * the faster (mi_csr_spmk_info says which).  Under stream capture nothing is measured and k plain launches are recorded. */
int mi_spmk(mi_csr_t A, int k, const double* x, double* const* y_out);                      /* host */
int mi_spmk_dev(mi_csr_t A, int k, const double* d_x, double* const* d_y_out, mi_stream_t s); /* device; d_y_out is a HOST array of k device pointers */

/* The powers step runs as ONE launch where that is possible and faster (spmk_ring.hpp: every persistent workgroup keeps its run
 * of row blocks for all k powers; a run's power p is published write-through + flag, power p + 1 waits for the flags of the runs
 * its columns name) — k <= 8, ring-served square matrices whose whole grid is resident at once; the first k-step of a handle at a
 * given k times both forms (same bits) and keeps the faster.  MI355_SPMK_FUSED=0 never, =1 always where eligible.  The handle
 * carries the step's flags: one k-step at a time per handle.  That FIRST k-step at a given k is therefore synchronous: it runs
 * 2 rounds x 2 forms x (2 warm-up + 5 timed) extra k-steps on the caller's stream and vectors and blocks the host on an event (a few
 * milliseconds at 1 M rows); later calls are asynchronous as documented.  If a wait of the one-launch form gives up during that
 * measurement, the measurement stops at once and the handle runs k launches.  Under HIP stream capture the step is recorded as k launches (the flags'
 * epoch is a kernel argument; a replayed graph would present it again).  Reports what the handle does at this k (after its first k-step). */
int mi_csr_spmk_info(mi_csr_t A, int k, int* eligible, int* one_launch, double* us_k_launches, double* us_one_launch);

/* host-only: derive the one-launch step's run dependencies as mi_csr_create would and CHECK them against the matrix (every column
 * a run names or loads belongs to a run on its list; MI_ERR_STATE names the first violation).  *eligible = 0 when the plan cannot
 * carry the step (rows outside the ring loop, or a band so wide that a run would wait for more than 64 others). */
int mi_spmk_plan_probe(int n, const int* ptrow, const int* indcol, int* eligible, int* runs, int* max_deps);
/* host-only: the plan and the lists that probe checks, copied out for a test to restate the kernel's loads against (built by the
 * same two calls; nothing is checked here).  info[8] = {T, row blocks, runs (= workgroups of the grid), blocks per run of the uniform
 * deal, 1 if the deal IS the uniform one (the kernel derives run g = blocks [g * bpw, (g + 1) * bpw) itself; else it reads run_rng),
 * 1 if every row is computed inside the LEAN ring loop (only then are there lists), entries of dep_run, 1 if the plan is LEAN}; all
 * zero for a matrix without rows or nonzeros.  Optional arrays, sizes from a first call with nulls: plan[8 * blocks] = {first row,
 * first nonzero, rows, nonzeros, new_lo, new_cnt, ring base, flags} per block (cap_blocks >= blocks); run_rng[2 * runs] = {first
 * block, end block} per run and dep_ptr[runs + 1] (cap_runs >= runs); dep_run[dep_ptr[g] .. dep_ptr[g + 1]) = the runs whose
 * flags run g waits for (cap_deps >= entries). */
int mi_spmk_plan_dump(int n, const int* ptrow, const int* indcol, int info[8], int* plan, int* run_rng, int* dep_ptr, int* dep_run,
                      int cap_blocks, int cap_runs, int cap_deps);

/* ---- BLAS-1 between SpMVs ---------------------------------------------- */
/* out = sum x_i y_i  (std::inner_product, mpk/SpMVmulti.cpp:147).  Fixed
 * two-stage reduction tree (blas1_kernels.hpp), not the CPU's order: the bits
 * of mi_dot, mi_norm2 and mi_rel_error (host and device forms) depend only on
 * n and the data — not on the vectors' alignment, the stream, or whether the
 * loads are non-temporal.  oracle/cpu_ref.c restates the tree bit for bit; its
 * distance to the exact sum is at most gamma_h * sum |x_i y_i| with h the tree's
 * depth (about 30 roundings at 1 M elements). */
int mi_dot(int n, const double* x, const double* y, double* out);
int mi_dot_dev(int n, const double* d_x, const double* d_y, double* d_out, mi_stream_t s);
/* y += a x  (VecAXPY at src/solve_newton.c:1269; the AXPY half of orthogonalize) */
int mi_axpy(int n, double a, const double* x, double* y);
int mi_axpy_dev(int n, double a, const double* d_x, double* d_y, mi_stream_t s);
/* x3 = x1 - alpha * (b . x1) * b ; *beta_out = b . x1
 * (orthogonalize, mpk/SpMVmulti.cpp:146-151; in-place twin mpk/2SpMV.cpp:3-11: pass x3 == x1).
 * The update is evaluated as the reference's object code does it: x3[i] = fma(-(alpha*beta), b[i], x1[i]).
 * Reductions enqueued on different streams use separate workspaces and may run concurrently. */
int mi_orthogonalize(int n, const double* b, const double* x1, double* x3, double alpha, double* beta_out);
int mi_orthogonalize_dev(int n, const double* d_b, const double* d_x1, double* d_x3, double alpha,
                         double* d_beta_out, mi_stream_t s);
/* The Krylov-step pipeline of mpk/SpMVmulti.cpp:563-569 — SpMV_CSR(x1, b, a); orthogonalize(nrow, b, x1, x3); SpMV_CSR(x2, x3, a)
 * — with the dot folded into the product (SURVEY.md §8 f-4 "fuse orthogonalisation with the k-step kernel"):
 *   mi_spmv_dot_dev            y = A x and *beta = b . y; b . y is accumulated in the product's epilogue, while each row's
 *                              value is still in its thread's register (ring kernel, LEAN form), so y and b are not read again
 *                              by a dot kernel of their own.  Handles whose launch cannot carry the epilogue (other kernels,
 *                              relabelled or blocked matrices) run product and dot as separate launches: same call, same bound.
 *   mi_spmv_orthogonalize_dev  x1 = A x; beta = b . x1 (epilogue); x3 = fma(-(alpha*beta), b, x1): two launches instead of three.
 * beta is a fixed-tree reduction like mi_dot's, not the CPU's left-to-right sum; every row of y / x1 and, given beta, every
 * element of x3 are the reference's bits.  Square or rectangular, unmapped matrices; device vectors.
 * WHICH tree gives beta depends on whether the handle's launch carries the dot (mi_csr_dot_epilogue_info): with the epilogue it
 * is the ring kernel's tree over its runs (mi_csr_dot_epilogue_layout), without it mi_dot_dev's tree over (b, y).  The kernel
 * choice made at create decides that, so beta's last bits can differ between boxes for the same matrix and vectors.  A caller
 * who needs the same beta everywhere pins the kernel (mi_csr_set_kernel). */
int mi_spmv_dot_dev(mi_csr_t A, const double* d_x, double* d_y, const double* d_b, double* d_beta_out, mi_stream_t s);
/* *in_epilogue = 1 if the next mi_spmv_dot_dev / mi_spmv_orthogonalize_dev on this handle carries the dot in the product's launch */
int mi_csr_dot_epilogue_info(mi_csr_t A, int* in_epilogue);
/* Read-only: the layout the ring kernel's dot epilogue walks, for a handle whose launch carries it (else MI_ERR_STATE).
 * *threads = workgroup size T, *wgs = logical workgroups (= partials), *nblk = row blocks.  When any array is given:
 * run_first_block[g] (wgs + 1 entries, cap_runs >= wgs + 1) = first block of workgroup g's run, which ends where run g + 1
 * begins; block_row0[b], block_rows[b] (nblk entries, cap_blocks >= nblk) = first row and row count of block b.  Thread t of
 * workgroup g adds b[r] * y[r] for row r = block_row0[blk] + t (t < block_rows[blk]) of each block of its run in order. */
int mi_csr_dot_epilogue_layout(mi_csr_t A, int* threads, int* wgs, int* nblk, int* run_first_block, int* block_row0,
                               int* block_rows, int cap_runs, int cap_blocks);
int mi_spmv_orthogonalize_dev(mi_csr_t A, const double* d_x, double* d_x1, const double* d_b, double* d_x3, double alpha,
                              double* d_beta_out, mi_stream_t s);
/* orthonormalize_against_basis(nrow, basis, y), mpk/2SpMV.cpp:13-28: for each of the m basis vectors IN TURN
 * dots[j] = y . v_j (on the y updated so far), y <- fma(-dots[j], v_j, y).  Like the reference nothing is
 * normalised (its norm is computed and dropped).  basis: HOST array of m pointers (host resp. device vectors).
 * m + 1 launches: each update also accumulates the next vector's dot. */
int mi_orthonormalize_against_basis(int n, int m, const double* const* basis, double* y, double* dots_out /* [m] or NULL */);
int mi_orthonormalize_against_basis_dev(int n, int m, const double* const* d_basis, double* d_y, double* d_dots /* [m] */,
                                        mi_stream_t s);
/* VecMDot (src/solve_newton.c:1265, inside KSPSolve: the dots of one GMRES iteration): dots[j] = y . v_j, j < m <= 64, in
 * ONE pass over y per tile of basis vectors (blas1_multi.hpp) and two launches.  Tree: every column is reduced by mi_dot's own
 * fixed two-stage tree, so dots[j] has the bits of mi_dot_dev(n, y, v_j), whatever the tile, alignment or stream.
 * basis: HOST array of m pointers (host resp. device vectors).  m == 0: nothing is done; n == 0: dots = 0.
 * MI_ERR_ARG: m outside 0..64, a null vector, y pointer-equal to a basis vector. */
int mi_mdot(int n, int m, const double* const* basis, const double* y, double* dots /* [m] */);
int mi_mdot_dev(int n, int m, const double* const* d_basis /* HOST array of m device pointers */, const double* d_y,
                double* d_dots /* device [m] */, mi_stream_t s);
/* VecMAXPY (src/solve_newton.c:1265, inside KSPSolve: the update of one GMRES iteration), in place:
 * y <- fma(a_{m-1}, v_{m-1}, ... fma(a_0, v_0, y)) per element, a_j = negate ? -coef[j] : coef[j] (an exact sign flip) — the
 * bits of m successive mi_axpy_dev.  The device form reads the coefficients from DEVICE memory (no host round trip after the
 * dots).  d_norm_out (NULL or device [1]): norm2 of the new y, accumulated while it is written.  Tree: mi_norm2's, so the value
 * has the bits of mi_norm2_dev of the new y.  m == 0: y is left alone, d_norm_out still receives norm2(y).
 * MI_ERR_ARG: as for mi_mdot. */
int mi_maxpy(int n, int m, const double* coef /* [m] */, int negate, const double* const* basis, double* y);
int mi_maxpy_dev(int n, int m, const double* d_coef /* device [m] */, int negate, const double* const* d_basis, double* d_y,
                 double* d_norm_out, mi_stream_t s);
/* Classical Gram-Schmidt of y against m vectors out of VecMDot / VecMAXPY (src/solve_newton.c:1265; KSPGMRES's
 * orthogonalisation, with passes = 2 its -ksp_gmres_cgs_refinement_type refine_always).  Per pass: d = mi_mdot_dev(y) — every
 * dot against the same y — then y <- mi_maxpy_dev(d, negate = 1).  h = d of pass 1 (+ d of pass 2, ONE rounded add per entry);
 * *d_norm = norm2 of the final y, from the last update.  Tree: those of mi_dot and mi_norm2.  3 launches per pass.
 * MI_ERR_ARG: as for mi_mdot, or passes outside {1, 2}. */
int mi_cgs_dev(int n, int m, const double* const* d_basis, double* d_y, int passes, double* d_h /* device [m] */,
               double* d_norm /* device [1] */, mi_stream_t s);
/* The three calls above against a basis stored in SINGLE PRECISION (the basis of a MI_BASIS_F32 solver, mi_gmres_* below): every
 * basis entry f is used as widen(f) = (double)f, which is exact; y, the coefficients, the accumulators and every fma stay double.
 * The results are, BIT FOR BIT, those of mi_mdot_dev / mi_maxpy_dev / mi_cgs_dev on the widened vectors — the same segments, lane
 * pairs and finishing tree — whatever the tile, y's alignment, the stream or the non-temporal choice; a lane loads its pair of
 * basis entries with one 8-byte load, so the basis costs half the bytes.  Argument rules: those of the double calls, and every
 * float vector must be 8-BYTE ALIGNED (MI_ERR_ARG otherwise); all are checked before the device is touched.  Nothing is allocated
 * per call beyond the per-stream workspace of the double calls; all three can be captured into a graph. */
int mi_mdot_f32_dev(int n, int m, const float* const* d_basis /* HOST array of m device pointers */, const double* d_y,
                    double* d_dots /* device [m] */, mi_stream_t s);
int mi_maxpy_f32_dev(int n, int m, const double* d_coef /* device [m] */, int negate, const float* const* d_basis, double* d_y,
                     double* d_norm_out, mi_stream_t s);
int mi_cgs_f32_dev(int n, int m, const float* const* d_basis, double* d_y, int passes, double* d_h /* device [m] */,
                   double* d_norm /* device [1] */, mi_stream_t s);
/* d_out32[i] = round32(d_x[i] / *d_div) — the IEEE division in double, then round32 as mi_gmres_* defines it below; d_div NULL
 * (else device [1]): no division — and d_out64[i] = widen(d_out32[i]), in one pass and one launch.  d_out64 NULL: not written;
 * d_out64 == d_x is allowed (in place).  d_out32 needs 4-byte alignment, the double vectors 8; d_out32 must not be one of them.
 * MI_ERR_ARG before the device is touched: n < 0, d_x or d_out32 null, a misaligned vector.  n == 0: nothing is done. */
int mi_round_f32_dev(int n, const double* d_x, const double* d_div, float* d_out32, double* d_out64, mi_stream_t s);
/* sqrt(sum x^2) (norm2, mpk/utils.cpp:131-136) and ||ref-test||/||ref|| (rel_error, :138-143) */
int mi_norm2(int n, const double* x, double* out);
int mi_norm2_dev(int n, const double* d_x, double* d_out, mi_stream_t s);
int mi_rel_error(int n, const double* ref, const double* test, double* out);
int mi_rel_error_dev(int n, const double* d_ref, const double* d_test, double* d_out, mi_stream_t s);
/* dst[i] = src[idx[i]] — halo pack */
int mi_gather_dev(int m, const int* d_idx, const double* d_src, double* d_dst, mi_stream_t s);

/* ---- BCSR 4x4 (SpMV_BCSR*, mpk/SpMV.cpp:90-219; row-major blocks) ------- */
/* The handle is complete on return and usable from any stream, non-blocking ones included. */
int mi_bcsr4_create(int nbrows, int nbcols, const int* ptrow, const int* indcol, const double* coef,
                    mi_bcsr4_t* out);
int mi_bcsr4_destroy(mi_bcsr4_t A);
/* Block layout of the caller's coefficient array.  mpk/ stores a 4x4 block ROW-major (mpk/SpMV.cpp:112: blk[4*i + j]); PETSc's
 * MATSEQBAIJ — the matrix the reference's solver multiplies with (MatSetOperation(..., MATOP_MULT, ...), src/solve_newton.c:864-879;
 * kernels src/kernels/baij4_{mad,fma,avx2}.c) — stores it COLUMN-major (baij4_mad.c:73-76: row 0 is v[0], v[4], v[8], v[12]).
 * The *_layout entry points take either; column-major blocks are transposed on the way to the device (at create and at every
 * value refresh, never per product), after which the handle is an ordinary one: y is bit-equal to the row-major handle of the
 * transposed blocks, i.e. each row is the fma chain of SpMV_BCSR_FMA (mpk/SpMV.cpp:150-178).  (That is NOT the summation order of
 * MatMult_SeqBAIJ_4_AVX2, which keeps four per-column accumulators and adds them at the end, src/kernels/baij4_avx2.c:42-66; that
 * kernel needs PETSc to run, so against it parity is unpinned here — see INTEGRATION.md §4.) */
enum { MI_BLOCK_ROWMAJOR = 0, MI_BLOCK_COLMAJOR = 1 };
int mi_bcsr4_create_layout(int nbrows, int nbcols, const int* ptrow, const int* indcol, const double* coef, int layout, mi_bcsr4_t* out);
int mi_bcsr4_update_values_layout(mi_bcsr4_t A, const double* coef, int layout);                          /* host values */
int mi_bcsr4_update_values_layout_dev(mi_bcsr4_t A, const double* d_coef, int layout, mi_stream_t s);     /* device values */
/* The blocked kernel exists in two forms: x blocks gathered through L1/L2 per block (spmv_bcsr4), or each workgroup's distinct
 * block columns gathered once into an LDS tile and addressed through a 16-bit stream (spmv_bcsr4_tile; built when no group of 64
 * block rows touches more than 1024 block columns).  mi_bcsr4_create times both and keeps the faster; same bits.
 * MI355_BCSR_TILE=0|1 forces. */
int mi_bcsr4_tile_info(mi_bcsr4_t A, int* built, int* in_use, double* us_plain, double* us_tile);
/* host-only: the lists of that x tile as mi_bcsr4_create would build them for this block pattern (the same builder,
 * bcsr4_tile_plan.hpp).  *would_build = 0 for a pattern of fewer than 4096 blocks (nothing is listed then: *max_nodes and
 * *groups_at_cap are 0) or with a group of more than 1024 distinct block columns (MI355_BCSR_TILE is not looked at);
 * *groups = groups of 64 block rows; *max_nodes = the longest list among the groups listed; *groups_at_cap = groups of exactly 1024. */
int mi_bcsr4_tile_probe(int nbrows, const int* ptrow, const int* indcol, int* would_build, int* groups, int* max_nodes,
                        int* groups_at_cap);
/* Third form (round 4, spmv_bcsr_sell.hpp): a SLICED copy of the block values made at mi_bcsr4_create for matrices of >= 100 000 blocks
 * — 16 consecutive block rows per slice, padded to the slice's longest row, step j of a slice = the j-th block of each of its rows as
 * two contiguous kilobytes — streamed by persistent waves, each over one contiguous range of slices, with unconditional counted loads
 * (non-temporal where that measures faster) that never look at a row boundary; a slice's sums are parked in LDS and stored behind the
 * wave's last load (a store issued among the loads costs the read stream many times its bytes).  Same lanes per row, same fma order,
 * same bits.  Four variants are timed against the two forms above at create and the fastest of all runs (MI355_BCSR_SELL=0 never builds
 * it, =1 takes variant 0 unmeasured, MI355_BCSR_SELL_FORM=0..3 a given one).  The blocked copy of a relabelled matrix runs it too (a node's
 * four sums leave through the block-row map).  The sliced values follow mi_bcsr4_update_values* at once, on that call's stream.  *form_in_use: -1 none; 0 one wave per SIMD, eight steps of prefetch, non-temporal value loads; 1 the
 * same with temporal loads; 2 two waves per SIMD (one workgroup of eight waves per CU), four steps, non-temporal; 3 as 0 with twelve steps;
 * *padding = padded places / blocks - 1; us[f] = microseconds per launch measured for variant f (0: not measured). */
int mi_bcsr4_sell_info(mi_bcsr4_t A, int* built, int* form_in_use, long long* steps, double* padding, double us[4]);
/* The plan of that sliced copy for a block pattern, built on the host as mi_bcsr4_create builds it (no device needed; nothing is kept):
 * *nslices = ceil(nbrows / 16), *nsteps = the steps of all slices (a slice of empty rows takes one), *nwaves = the persistent waves for
 * a cap of nwaves_max (the handle plans 1024 for variants 0, 1, 3 and the multi-vector product, 2048 for variant 2).  Copied out where
 * the pointer is not null: sptr[nslices + 3] (first step of every slice, three terminators), wrng[nwaves + 1] (first slice of every
 * wave), col[(nsteps + 48) * 16] (the column stream with its 48 tail steps: bit 31 a padding place, bit 30 a slice's first step).
 * Call it once with null arrays for the sizes.  No slice table is made for a matrix without block columns: mi_bcsr4_create never
 * builds the sliced copy there. */
int mi_bcsr4_sell_plan_probe(int nbrows, const int* ptrow, const int* indcol, int nwaves_max, int* nslices, long long* nsteps, int* nwaves,
                             int* sptr, int* wrng, unsigned* col);
/* new block values (16 per block, row-major) for an unchanged block pattern; see mi_csr_update_values */
int mi_bcsr4_update_values(mi_bcsr4_t A, const double* coef);
int mi_bcsr4_update_values_dev(mi_bcsr4_t A, const double* d_coef, mi_stream_t s);
int mi_bcsr4_spmv(mi_bcsr4_t A, const double* x, double* y);
int mi_bcsr4_spmv_dev(mi_bcsr4_t A, const double* d_x, double* d_y, mi_stream_t s);
/* y_out[p] = A^(p+1) x for p < k on the blocked matrix: what SpM2V_BCSR{,_OPT,_FMA,_AVX2}(z, y, x, A, ptrowend1)
 * (mpk/SpM2V.cpp:375-801) return for k = 2 (y_out = {y, z}); k chained launches, each row one fma chain. */
int mi_bcsr4_spmk(mi_bcsr4_t A, int k, const double* x, double* const* y_out);
int mi_bcsr4_spmk_dev(mi_bcsr4_t A, int k, const double* d_x, double* const* d_y_out, mi_stream_t s);

/* ---- multi-vector products and the s-step Krylov basis ----
 * Y[:, j] = A X[:, j] for j < s with the matrix read ONCE for the s columns: MatMatMult_SeqBAIJ_4_AVX2(A, X, Y, s_step),
 * src/kernels/spmm_avx2.c:7-109.  X, Y dense column-major, column j at X + j*ldx (the reference's MatDense layout,
 * lda = 4 * mbs at :23); ldx >= 4*nbcols even, ldy >= 4*nbrows.  arith selects the association of a row's sum:
 *   MI_ARITH_CHAIN     one continuous fma chain over the row's blocks — every column bit-equal to SpMV_BCSR_FMA
 *                      (mpk/SpMV.cpp:150-178), i.e. to the CSR fma chain;
 *   MI_ARITH_BLOCKACC  per block the four products chained from zero, the partial added to the row value — what
 *                      spmm_avx2.c:77-88 and SpM2V_BCSR_OPT (mpk/SpM2V.cpp:502-507) do.  The reference's final
 *                      horizontal add (:96-101) sums four identical broadcast lanes and returns 4 A X; not reproduced. */
enum { MI_ARITH_CHAIN = 0, MI_ARITH_BLOCKACC = 1 };
int mi_bcsr4_spmm(mi_bcsr4_t A, int s, const double* X, long long ldx, double* Y, long long ldy, int arith);          /* host */
int mi_bcsr4_spmm_dev(mi_bcsr4_t A, int s, const double* d_X, long long ldx, double* d_Y, long long ldy, int arith,
                      mi_stream_t st);
/* The product exists in five forms with the same bits.  0: x blocks gathered through L1/L2 per block (spmm_bcsr4 / spmm_bcsr4_quad).
 * 1: tiles of up to 128 block rows — clusters of the block graph — gather the S columns of their distinct block columns ONCE into LDS
 * and the loop waits for coefficients only (spmm_bcsr4_tile, up to four columns).  2 / 3: the same with EIGHT lanes per block row
 * (64-row tiles; one 16-byte coefficient load per lane and block, the two halves of a row swapped through DPP; even column counts),
 * coefficients loaded temporally / non-temporally (spmm_bcsr4_otile).  The lists are built at the first product; the first product of
 * a handle at a column count times the possible forms and keeps the fastest (MI355_SPMM_TILE=0..4 forces one).  4 (round 4): the
 * SLICED stream of mi_bcsr4_sell_info with S sums per lane (spmm_bcsr4_sell; four or eight columns, unmapped products): the x blocks
 * shared inside the quad through DPP, a finished slice's sums parked in LDS and stored behind the loads.  *form_in_use = what
 * the next product runs; us[f] = microseconds per launch measured for form f (0: not possible / not yet measured). */
int mi_bcsr4_spmm_info(mi_bcsr4_t A, int s, int* tile_built, int* form_in_use, int* longest_list, double us[5]);
/* The plan of forms 1-3 for a block pattern, built on the host by the function the handle calls at its first product (no device needed;
 * nothing is kept): per = 128 for form 1, 64 for forms 2 and 3; ucap = the list length above which a cluster is halved (the handle takes
 * 368 and 256, or MI355_SPMM_TILE_UCAP).  *refused != 0: no plan (a single block row with more than 65 535 distinct block columns, or
 * no block at all) — the handle then runs form 0; the other outputs are 0 and nothing is copied.  Else *ntiles, *umax (the longest list,
 * what mi_bcsr4_spmm_info reports as longest_list), *mean_list, and, where the pointer is not null, the arrays as they are uploaded:
 * wg_ptr[ntiles + 1], nodes[wg_ptr[ntiles] + 1] (every list strictly ascending; one pad entry), slots[nblocks + 1] (block k's column is
 * nodes[wg_ptr[t] + slots[k]] for the tile t of its row; one pad entry), rows[ntiles * per] (a block row, or -1 - r for an unused place
 * that shadows row r of the same tile).  Each array comes with its capacity in elements; MI_ERR_ARG if one is too small (nbrows + 1,
 * nblocks + 1, nblocks + 1 and nbrows * per always suffice).  A form is possible at s columns when its plan exists, the matrix has at
 * least 4 096 blocks and umax * (4 s + 2) * 8 bytes fit the 160 KiB of LDS (form 1: s <= 4; forms 2, 3: s even, s <= 8). */
int mi_bcsr4_spmm_plan_probe(int nbrows, const int* ptrow, const int* indcol, int per, int ucap, int* refused, int* ntiles, int* umax,
                             double* mean_list, int* wg_ptr, long long wg_ptr_cap, unsigned* nodes, long long nodes_cap,
                             unsigned short* slots, long long slots_cap, int* rows, long long rows_cap);
/* the same for a CSR handle (MI_ARITH_CHAIN bits = SpMV_CSR_FMA per column): one launch over the blocked copy when the
 * matrix has exact 4x4 node-block structure, else s single-vector launches */
int mi_spmm_dev(mi_csr_t A, int s, const double* d_X, long long ldx, double* d_Y, long long ldy, mi_stream_t st);
/* orth == 0: V[:, 0] = v0, V[:, k+1] = A V[:, k], k < s — BuildKrylovBasis_AVX2, src/kernels/spmm_avx2.c:112-168 (dense
 * column-major n x (s+1) V, ldv >= n): the monomial basis, bit-equal to the matrix-powers chain.
 * orth != 0: the orthonormal (Arnoldi) basis of the same space, from the reference's own pieces: V[:, 0] = v0/||v0||, each
 * product passed through orthonormalize_against_basis (mpk/2SpMV.cpp:13-28) against the earlier columns, then divided by
 * its norm2 — the normalisation that helper computes and drops.  d_coef (s*(s+2)+1 doubles): [k*(s+2) + j] = dot of step
 * k with column j (j <= k), [k*(s+2) + k+1] = the norm, [s*(s+2)] = ||v0||. */
int mi_krylov_basis_dev(mi_csr_t A, int s, const double* d_v0, double* d_V, long long ldv, int orth, double* d_coef,
                        mi_stream_t st);
/* mi_krylov_basis_dev's orthonormal basis with mi_cgs_dev (VecMDot / VecMAXPY, src/solve_newton.c:1265) in place of the
 * sequential sweep; passes = 1 | 2.  Same V and d_coef layout ([k*(s+2) + j] = h_j of step k, [k*(s+2) + k+1] = the norm,
 * [s*(s+2)] = ||v0||).  Tree: the product's fma chain, mi_dot's and mi_norm2's trees, IEEE division.  Two passes keep
 * max |V^T V - I| at a few ulps on matrices where the sweep of mi_krylov_basis_dev(orth = 1), which is unchanged, loses
 * orthogonality. */
int mi_krylov_basis_cgs_dev(mi_csr_t A, int s, const double* d_v0, double* d_V, long long ldv, int passes, double* d_coef,
                            mi_stream_t st);

/* ---- 4x4-block ILU(k): factored on the host, solved on the GPU level by level ----
 * The preconditioner of the reference's Newton solve: PCILU with 4 levels of fill on the BAIJ-4 Jacobian under GMRES(30)
 * (src/solve_newton.c:1156-1164), ILU(0) on the Stokes matrix (:1068-1074), with the hand-written kernels the reference installs
 * through MatSetOperation(MATOP_SOLVE) (:1088, :1257): src/kernels/baij4_factor_avx2.c (numeric factorisation) and
 * src/kernels/baij4_solve.c, baij4_solve_avx2.c (MatSolve_SeqBAIJ_4).  Natural ordering (PETSc's default for PCILU: the row and
 * column permutations of the reference's solve are the identity); single GPU.
 *
 * Pattern: symbolic ILU(fill) on the block pattern.  An original block has level 0; block (i, j) reached through a pivot block
 * (i, p), p < min(i, j), gets lev(i, p) + lev(p, j) + 1 — the minimum over the pivots that reach it — and is kept when that is
 * <= fill.  Block columns ascending in every row.
 * Values (baij4_factor_avx2.c:114-170, IKJ): row i of A is scattered into a work row; for each block (i, p) left of the diagonal in
 * ascending p — skipped when all 16 entries are zero — M = W(i, p) . Dinv(p) replaces it and W(i, j) -= M . U(p, j) for every block
 * (p, j), j > p, of row p whose column is in row i's pattern; then the diagonal block is inverted in place and the INVERSE is kept,
 * as PETSc keeps it.
 * ARITHMETIC (part of the interface): every entry of a 4x4 product is p = fma(a3,b3, fma(a2,b2, fma(a1,b1, a0*b0))) — the four
 * products chained from a rounded product, as MI_ARITH_BLOCKACC chains them — and an update is ONE rounded w - p.  The 4x4
 * inverse is Gauss-Jordan without pivoting: for k = 0..3: d = a[k][k]; piv = 1/d; a[k][k] = 1; a[k][j] *= piv (j = 0..3); then for
 * each other row i ascending: f = a[i][k]; a[i][k] = 0; a[i][j] = a[i][j] - f*a[k][j] (a rounded product, then a rounded
 * subtraction).  A pivot with |d| < 1e-12 (the reference's threshold) is refused: MI_ERR_ARG with the block row in
 * mi_last_error(); nothing is regularised (the reference's "+1e-8 and carry on" is not reproduced).  The rows of one dependency
 * level are factored by several host threads (MI355_BILU_THREADS, default min(cores, 16)); the bits do not depend on the count.
 * Solve (baij4_solve.c:4-93), x = U^-1 L^-1 b: forward, per block row in level order, s = b_i; for each L block in ascending
 * column order s_r <- s_r - p_r, p_r the chain above of block row r with t_j; t_i = s.  Backward: s = t_i, the same over the U
 * blocks, then x_i = Dinv_i . s, each entry one chain.  Every row is therefore ONE fixed sequence of roundings, independent of the
 * level schedule, the folding and the alignment of the vectors.
 * Schedule: level of row i = 1 + max level of its L columns (forward; over its U columns backward).  The device copy is
 * level-major (the rows of a level contiguous, ascending row number); one launch per level, except that a run of consecutive
 * levels of fewer than 64 block rows is ONE launch of one workgroup stepping through them with workgroup barriers.
 * The solve is enqueued on the caller's stream; nothing is allocated or synchronised per call; d_x == d_b is allowed.  d_x serves
 * as the solve's work vector: its contents are undefined until the solve has finished.
 * MI_ERR_ARG: a null argument, fill < 0, block columns outside [0, nbrows) (the matrix must be square), unsorted or duplicate block
 * columns, a row without a diagonal block, an unknown layout, a refused pivot.  nbrows == 0: every call is a no-op.
 * MI355_BILU_FORM: 0 = one launch per (folded) level, the form every handle is created with; 1 is refused at create with
 * MI_ERR_UNSUPPORTED (the one-launch form is chosen per handle, by mi_bilu4_set_solve_form below, not by the environment). */
typedef struct mi_bilu4_s* mi_bilu4_t;
int mi_bilu4_create(int nbrows, const int* ptrow, const int* indcol, const double* coef, int layout /* MI_BLOCK_* */, int fill,
                    mi_bilu4_t* out);
/* the same without a device: pattern, schedule and host factor only (mi_bilu4_refactor, _info, _factor_host work; a solve returns
 * MI_ERR_STATE) */
int mi_bilu4_create_host(int nbrows, const int* ptrow, const int* indcol, const double* coef, int layout, int fill, mi_bilu4_t* out);
int mi_bilu4_destroy(mi_bilu4_t F);
/* new values, same pattern (a Newton step: the Jacobian is re-assembled, src/solve_newton.c:1257 onwards); waits for the device,
 * then replaces the factor.  After a refused pivot the handle must be refactored before it is used again. */
int mi_bilu4_refactor(mi_bilu4_t F, const double* coef, int layout);
int mi_bilu4_solve_dev(mi_bilu4_t F, const double* d_b, double* d_x, mi_stream_t s); /* MatSolve_SeqBAIJ_4, baij4_solve.c:4-93 */
int mi_bilu4_solve(mi_bilu4_t F, const double* b, double* x);                         /* host vectors: copied in and out */
/* *launches = launches per solve (both sweeps, after folding; 1 for the one-launch form); *form = the form in use (MI_BILU_FORM_*,
 * 0 until mi_bilu4_set_solve_form says otherwise); us[0] = microseconds per solve of form 0 measured at create, us[1] = of the
 * one-launch form (0 until mi_bilu4_set_solve_form(F, -1) has measured both); *factor_seconds = host time of the last numeric factorisation; *factor_bytes = blocks,
 * block columns and the per-row tables of the device copy.  Any output may be NULL. */
int mi_bilu4_info(mi_bilu4_t F, int* nbrows, long long* nblocks, int* fwd_levels, int* bwd_levels, int* launches, int* form,
                  double us[2], double* factor_seconds, long long* factor_bytes);
/* the host factor: ptr [nbrows + 1], col and val (16 per block, row-major; L multipliers, INVERTED diagonal block, U blocks) of
 * nblocks entries, diag [nbrows] = position of every diagonal block.  Any array may be NULL; cap_blocks = entries col / val hold. */
int mi_bilu4_factor_host(mi_bilu4_t F, int* ptr, int* col, int* diag, double* val, long long cap_blocks);
/* host-only: pattern and schedule exactly as mi_bilu4_create builds them: factor blocks, levels of the two sweeps, launches
 * after folding and (optional, cap_levels entries each) the block rows of every level. */
int mi_bilu4_plan_probe(int nbrows, const int* ptrow, const int* indcol, int fill, long long* nblocks, int* fwd_levels,
                        int* bwd_levels, int* fwd_launches, int* bwd_launches, int* fwd_sizes, int* bwd_sizes, int cap_levels);

/* ---- 4x4-block ILU(k): the numeric REfactorisation on the GPU (mi_bilu4dev_*) ----
 * A Newton step re-assembles the Jacobian and refactors before every linear solve (src/solve_newton.c:1257 onwards);
 * mi_bilu4_refactor does that on host threads, waits for the device and uploads the factor.  mi_bilu4dev_refactor computes the
 * same factor (baij4_factor_avx2.c:114-170, the ARITHMETIC above, operation for operation: the device factor is bit for bit what
 * mi_bilu4_refactor would have uploaded for the same values) on the GPU, on the caller's stream, from block values that already
 * lie on the device, in place into the device copies the solve reads; no second copy of the values is kept.
 * Schedule: the forward sweep's levels and launches (a row needs the finished rows of its L columns), after ONE launch that
 * clears the fill blocks, scatters the values and resets the refusal word: launches per refactor = forward launches + 1.
 * Sixteen lanes per block row, one per entry of a block.
 * ORDERING is the caller's business, as it is for the solve: a refactor on stream s is ordered with solves on s only.  A solve
 * running on another stream during a refactor reads a half-written factor.
 * Refused pivot: the refactor itself cannot report it (nothing is copied back); mi_bilu4dev_status does.  As on the host, the
 * rows of later levels are then not factored and the handle must be refactored, by either path, before it is used.
 * The host factor (mi_bilu4_factor_host) is NOT updated by a device refactor until mi_bilu4dev_fetch copies it back;
 * mi_bilu4_refactor replaces host and device factor as before.  Creation still factors on the host.
 * MI_ERR_ARG: a null handle, null d_coef, an unknown layout; MI_ERR_STATE: a host-only handle (_prepare, _refactor, _status,
 * _fetch).  nbrows == 0: every call is a no-op. */
/* host-only: the device refactor's plan for a pattern, exactly as mi_bilu4dev_prepare builds it: *update_pairs = the block
 * updates W(i, j) -= M . U(p, j) of one factorisation (baij4_factor_avx2.c:114-170; once per Newton step, solve_newton.c:1257),
 * *launches per refactor, *plan_bytes of its tables (below) */
int mi_bilu4dev_plan_probe(int nbrows, const int* ptrow, const int* indcol, int fill, long long* update_pairs, int* launches,
                           long long* plan_bytes);
/* build and upload the pattern-only tables of the device refactor (idempotent; allocates, may synchronise): every block row's
 * position in both sweeps, per factor block the block of the matrix that lands there, and per L block (i, p) the place in row i
 * of every U block of row p (baij4_factor_avx2.c:114-170 keeps a dense column map per row instead).  Pattern-only: once per
 * handle, not once per Newton step (solve_newton.c:1257) */
int mi_bilu4dev_prepare(mi_bilu4_t F);
/* new values, same pattern (src/solve_newton.c:1257 onwards; baij4_factor_avx2.c:114-170), d_coef on the device in the order of the
 * arrays given at create (16 per block, `layout`); asynchronous on s: nothing allocated, copied to the host or synchronised once
 * prepared (so it can be captured into a graph); calls mi_bilu4dev_prepare itself when needed (that first call is not capturable) */
int mi_bilu4dev_refactor(mi_bilu4_t F, const double* d_coef, int layout, mi_stream_t s);
/* waits for the device, hence for the last mi_bilu4dev_refactor; *bad_row = -1 and MI_OK, or the refused block row and MI_ERR_ARG
 * with the same message mi_bilu4_refactor gives (the |d| < 1e-12 rule of baij4_factor_avx2.c:114-170; solve_newton.c:1257) */
int mi_bilu4dev_status(mi_bilu4_t F, int* bad_row);
/* waits, then copies the device factor back into the host factor, so that mi_bilu4_factor_host returns what the device holds
 * (the factor of baij4_factor_avx2.c:114-170 after the refactor of solve_newton.c:1257) */
int mi_bilu4dev_fetch(mi_bilu4_t F);
/* *prepared, *launches per refactor, *plan_bytes of device tables beyond what mi_bilu4_info counts (0 until prepared); any output
 * may be NULL (baij4_factor_avx2.c:114-170, solve_newton.c:1257: the cost of refactoring per Newton step) */
int mi_bilu4dev_info(mi_bilu4_t F, int* prepared, int* launches, long long* plan_bytes);

/* ---- 4x4-block ILU(k): both sweeps of the solve in ONE launch (mi_bilu4one_*, mi_bilu4_set_solve_form) ----
 * The level-by-level solve is bound by launches, not by bytes (hundreds of launches of a few microseconds of work each).  The
 * second form runs MatSolve_SeqBAIJ_4 (baij4_solve.c:4-93) as one launch of G persistent workgroups.  The unit of work is a CHUNK
 * of a sweep's level-major positions: a level of at least 64 block rows is cut into chunks of 64 consecutive positions (the last
 * may be shorter); a folded run of narrow levels (one launch of form 0) is ONE chunk, walked by its workgroup with workgroup
 * barriers.  Chunks are numbered in position order; a chunk never spans two wide levels.  A chunk's dependencies are the distinct
 * chunks of the SAME sweep that hold a block row named by one of its off-diagonal block columns (itself excepted), ascending; all
 * have a smaller index.  Chunk c belongs to workgroup c mod G and every workgroup takes its chunks in ascending order: with all G
 * resident the lowest unfinished chunk has only finished dependencies and an owner with nothing earlier left, so nothing stalls.
 * A chunk publishes its rows (write-through stores, drained) and then one flag; a consumer polls its dependencies' flags with one
 * lane each, hence at most 256 dependencies per chunk — a pattern with more is NOT ELIGIBLE and stays on form 0.  Between the sweeps
 * all workgroups meet once (a counter).  ARITHMETIC is the row's fixed sequence of roundings above: every bit equals form 0.
 * G = min(CUs, max(forward chunks, backward chunks)), MI355_BILU_ONE_WGS=n (n >= 1) overrides it; either is clamped to what the
 * occupancy query says is resident at once.  Every wait is bounded: when other kernels hold CUs a wait gives up after a few
 * seconds instead of hanging; that is sticky: the handle's next mi_bilu4_solve* and mi_bilu4one_status return MI_ERR_HIP until
 * mi_bilu4_set_solve_form(F, 0) clears it.
 * ONE solve at a time per handle, on ONE stream, while the handle is on form 1: the flags carry a per-handle epoch.  Under stream
 * capture form 0 is recorded (a replayed graph would present the same epoch again).  mi_bilu4_refactor and mi_bilu4dev_refactor
 * write the arrays this form reads too; stream order separates them as before.
 * MI_ERR_ARG: a null handle, an unknown form; MI_ERR_STATE: a host-only handle (_prepare, _set_solve_form, _status);
 * MI_ERR_UNSUPPORTED: the pattern is not eligible (reason in mi_last_error()).  nbrows == 0: every call is a no-op. */
enum { MI_BILU_FORM_LEVELS = 0, MI_BILU_FORM_ONE = 1, MI_BILU_FORM_AUTO = -1 };
/* host-only: chunks, dependencies and the dealing for `workgroups` (0: plan for 256), built exactly as mi_bilu4one_prepare builds
 * them and REPLAYED: G workgroups step through their chunks in order; MI_ERR_STATE names the first violation (a position in no chunk
 * or in two, a chunk across two wide levels, a named row whose chunk is not on the list, a dependency with an index >= its chunk's,
 * a dealing that stalls).  *eligible = 0 with the reason in mi_last_error() (a chunk with > 256 dependencies).  nchunks[2],
 * max_deps[2]: forward, backward.  Optional arrays, sizes from a first call with nulls: chunk_pos[nchunks + 1] and
 * chunk_lev[nchunks + 1] per sweep (first position / first level of each chunk), dep_ptr[nchunks + 1], dep[...] per sweep. */
int mi_bilu4one_plan_probe(int nbrows, const int* ptrow, const int* indcol, int fill, int workgroups, int* eligible, int nchunks[2],
                           int max_deps[2], long long* plan_bytes, int* const chunk_pos[2], int* const chunk_lev[2],
                           int* const dep_ptr[2], int* const dep[2]);
/* tables, flags, residency check; idempotent (allocates, may synchronise); MI_ERR_UNSUPPORTED + reason when not eligible */
int mi_bilu4one_prepare(mi_bilu4_t F);
/* the form of the handle's solves.  0: always succeeds, and clears a sticky give-up.  1: prepares if needed; MI_ERR_UNSUPPORTED
 * (and form 0 stays) when the pattern is not eligible.  -1: prepares, then times both forms on the handle's own scratch vectors,
 * two interleaved rounds, synchronously, and keeps the one-launch form only if it measured below 0.98 of form 0 and no wait gave
 * up; MI_OK with form 0 on a pattern that is not eligible.  (The declarator is parenthesised: the `mi_bilu4_name(` entries above
 * are the level-by-level interface, a closed set.) */
int (mi_bilu4_set_solve_form)(mi_bilu4_t F, int form);
/* MI_OK, or MI_ERR_HIP once a wait has given up; no GPU work */
int mi_bilu4one_status(mi_bilu4_t F);
/* *prepared, *eligible (0 until prepared), *workgroups (G), chunks and the largest dependency list per sweep (forward, backward),
 * *plan_bytes of tables and flags (0 until prepared); any output may be NULL */
int mi_bilu4one_info(mi_bilu4_t F, int* prepared, int* eligible, int* workgroups, int nchunks[2], int max_deps[2], long long* plan_bytes);

/* ---- 4x4-block ILU(k): the factor applied by a FIXED number of Jacobi sweeps per triangle (mi_bilu4sw_*) ----
 * The exact solve (mi_bilu4_solve*, either form) is bound by the dependency chain of the levels, not by bytes.  The sweep solve
 * applies the SAME device factor by the truncated Neumann series of each triangle (Anzt, Chow, Dongarra, Euro-Par 2015): every
 * sweep computes all rows at once from the previous iterate, one launch shaped like the blocked product.  With fixed counts the
 * operator is a fixed linear map, so plain right-preconditioned GMRES stays valid with it as M.
 * DEFINITION (part of the interface), for sweep counts sf, sb >= 0, L the block rows left of the diagonal (unit diagonal), U the
 * block rows right of it, Dinv the inverted diagonal blocks:
 *   forward    t^0 = b;  for k < sf:  t^{k+1}_i = b_i - sum_{j<i} L_ij t^k_j
 *   diagonal   x^0_i = Dinv_i . t^{sf}_i                                (the chain that ends the exact backward row)
 *   backward   for k < sb:  x^{k+1}_i = Dinv_i . (t^{sf}_i - sum_{j>i} U_ij x^k_j)
 *   result     x^{sb}
 * ARITHMETIC of a row is exactly the exact solve's above: s = the source entry; per block in ascending column order the chain
 * p = fma(a3,t3, fma(a2,t2, fma(a1,t1, a0*t0))) and ONE rounded s - p; the backward row ends with Dinv . s, one chain per entry.
 * Every sweep reads only the previous iterate and writes another vector: nothing is updated in place, so the result does not
 * depend on the schedule and is deterministic.  A row of dependency level l (counted from 0) holds the bits of the exact solve
 * after l sweeps and keeps them: (fwd_levels - 1, bwd_levels - 1) sweeps return mi_bilu4_solve's result BIT FOR BIT, and more
 * change nothing.  Counts above those are therefore CLAMPED to them (a huge count costs no more than the level count).
 * Launches per solve: sf + 1 + sb after clamping, on the caller's stream.  Once prepared a solve allocates nothing, copies nothing
 * to the host and synchronises nothing (it can be captured into a graph, together with mi_bilu4dev_refactor); an unprepared
 * handle is prepared by its first solve, except under stream capture: MI_ERR_STATE.  Three work vectors of 4 nbrows doubles
 * belong to the handle; the last launch alone writes d_x.  d_x == d_b is allowed; d_b is never written unless it is d_x.
 * Vectors need 8-byte alignment only.  The values are those of the device factor: whatever mi_bilu4_refactor or
 * mi_bilu4dev_refactor wrote last, with no extra step.  Independent of the handle's solve form.
 * ONE sweep solve at a time per handle (the work vectors are shared); ordering between streams is the caller's, as for the
 * device refactor.
 * MI_ERR_ARG: a null handle or vector, a negative count — before the device is touched; MI_ERR_NODEVICE: a host-only handle
 * (mi_bilu4_create_host), hence any box without a GPU: there is no CPU fallback.  nbrows == 0: every call is a no-op. */
/* allocates the work vectors; idempotent */
int mi_bilu4sw_prepare(mi_bilu4_t F);
int mi_bilu4sw_solve_dev(mi_bilu4_t F, const double* d_b, double* d_x, int sweeps_fwd, int sweeps_bwd, mi_stream_t s);
int mi_bilu4sw_solve(mi_bilu4_t F, const double* b, double* x, int sweeps_fwd, int sweeps_bwd); /* host vectors: copied in and out */
/* *prepared; *max_fwd = fwd_levels - 1 and *max_bwd = bwd_levels - 1, the counts the clamp ends at; *launches_last = launches of
 * the last sweep solve, after clamping (0 before the first); *work_bytes of the work vectors (0 until prepared).  Any output may
 * be NULL. */
int mi_bilu4sw_info(mi_bilu4_t F, int* prepared, int* max_fwd, int* max_bwd, int* launches_last, long long* work_bytes);

/* ---- 4x4-block ILU(k): the sweeps over an opt-in SINGLE-PRECISION COPY of the factor's values (mi_bilu4sp_*) ----
 * The sweep solve streams a whole triangle of the factor per sweep, 128 bytes of values per block.  The factor is a preconditioner:
 * right-preconditioned GMRES converges to the same solution whatever fixed linear operator plays M, so its stored coefficients
 * need not carry 53 bits.  mi_bilu4sp_prepare adds a second representation of the device factor: a copy of the level-major
 * values (L blocks, U blocks, inverted diagonal blocks) as float, 64 bytes per block more device memory; the double factor stays
 * (the refactorisations and the exact solves need it).  Nothing chooses the copy automatically: mi_bilu4_solve* (form 0 and form 1)
 * and mi_bilu4sw_* never read it, and their results, their info and every default are unchanged by it.
 * DEFINITION (part of the interface): for every factor value v
 *   v32 = (double)(float)v      rounded to nearest, ties to EVEN (what numpy's astype(float32) does); float SUBNORMALS are kept, not
 *                               flushed; a finite v beyond the float range becomes +-Inf; -0 stays -0
 * and the sweep solve with the single-precision factor is the definition of mi_bilu4sw_* above with v32 in place of v — forward,
 * diagonal and backward — with the same ARITHMETIC of a row in double: the fma chain per block, ONE rounded subtraction per block,
 * Dinv . s to end a backward row.  Vectors and work vectors are double; the conversion to double happens in registers and is exact.
 * Counts are CLAMPED as before; at the clamp the result is, BIT FOR BIT, the exact solve of the rounded factor.
 * KEPT CURRENT: once the handle is prepared, every entry point that writes the factor ends with the conversion:
 * mi_bilu4_refactor runs it before it returns; mi_bilu4dev_refactor enqueues it on the caller's stream behind the factorisation (two
 * more launches; a captured graph that holds a device refactor carries the conversion with it).  mi_bilu4dev_fetch writes the
 * host factor only and converts nothing.  The solves never convert and never check the host for staleness.
 * OVERFLOW: the conversion counts the values that are finite as double and not as float and keeps the count and the smallest
 * block row that holds one on the device.  An overflow does not block solves: they return what the definition says (Inf / NaN
 * where it has them); mi_bilu4sp_status is how a caller finds out, as mi_bilu4dev_status is for a refused pivot.
 * Launches per solve: sf + 1 + sb after clamping, on the caller's stream; once prepared a solve allocates nothing, copies nothing
 * to the host and synchronises nothing (it can be captured); an unprepared handle is prepared by its first solve, except under
 * stream capture: MI_ERR_STATE ("not prepared").  d_x == d_b is allowed; vectors need 8-byte alignment only.
 * ONE sweep solve of EITHER precision at a time per handle: the three work vectors are those of mi_bilu4sw_prepare, shared.
 * mi_bilu4sw_info keeps reporting the double sweeps only.  The copy lives until mi_bilu4_destroy.
 * MI_ERR_ARG: a null handle or vector, a negative count — before the device is touched; MI_ERR_NODEVICE: a host-only handle
 * (_prepare, _solve*, _status, _fetch): there is no CPU fallback.  nbrows == 0: every call is a no-op. */
/* allocates the copy and the work vectors and converts the factor as it is now (waits for the device); idempotent.  A failure
 * part-way leaves the handle unprepared and frees what was allocated */
int mi_bilu4sp_prepare(mi_bilu4_t F);
int mi_bilu4sp_solve_dev(mi_bilu4_t F, const double* d_b, double* d_x, int sweeps_fwd, int sweeps_bwd, mi_stream_t s);
int mi_bilu4sp_solve(mi_bilu4_t F, const double* b, double* x, int sweeps_fwd, int sweeps_bwd); /* host vectors: copied in and out */
/* waits for the device, hence for the last conversion; MI_OK with *bad_block_row = -1 and *overflowed = 0 (also before prepare), or
 * MI_ERR_ARG naming the smallest block row with a value that overflowed to Inf, and their number.  Outputs may be NULL */
int mi_bilu4sp_status(mi_bilu4_t F, int* bad_block_row, long long* overflowed);
/* waits, then copies the single-precision copy to the host in the HOST factor's block order (that of mi_bilu4_factor_host):
 * 16 floats per block, row-major, cap_blocks >= nblocks.  MI_ERR_STATE on a handle that is not prepared */
int mi_bilu4sp_fetch(mi_bilu4_t F, float* val, long long cap_blocks);
/* *prepared; *convert_launches = conversions enqueued so far, the one of prepare included (each is two launches: the record cleared,
 * the values written); *launches_last = launches of the last single-precision sweep solve, after clamping (0 before the first);
 * *copy_bytes of the copy, 64 per factor block (0 until prepared).  Any output may be NULL. */
int mi_bilu4sp_info(mi_bilu4_t F, int* prepared, int* convert_launches, int* launches_last, long long* copy_bytes);

/* ---- 4x4-block ILU(k): the EXACT solve over the single-precision copy (mi_bilu4spx_*) ----
 * Under the multicolour ordering the exact solve streams a few wide levels and is bound by what it reads, 128 bytes of values per
 * block.  mi_bilu4spx_solve* is the level-by-level exact solve reading the copy of mi_bilu4sp_prepare instead: 64 bytes per block,
 * no new device memory and no new conversion.  Opt-in: nothing chooses it, and mi_bilu4_solve*, mi_bilu4_info, mi_bilu4sw_* and
 * mi_bilu4sp_* are unchanged by it, bit for bit.
 * DEFINITION (part of the interface): the definition of mi_bilu4_solve* with v32 = (double)(float)v — the rounding rule of
 * mi_bilu4sp_* above — in place of EVERY factor value v: L, U and the inverted diagonal blocks.  Vectors, accumulators and a row's
 * sequence of roundings stay double and unchanged: the fma chain per block, blocks in ascending column order, ONE rounded
 * subtraction per block, Dinv . s to end a backward row.  Its result therefore equals, BIT FOR BIT, the exact solve of the rounded
 * factor, which is also what mi_bilu4sp_solve_dev returns with both counts at or above the clamp.
 * Always enqueued level by level (the launches of form 0, the same folding), whatever mi_bilu4_set_solve_form says: the one-launch
 * form has no single-precision instantiation.  On an ordered handle the solve keeps the caller's numbering (the gather and the
 * scatter: two launches, counted in *launches_last), and an unfolded level of at least kBiluWideMin block rows takes the float
 * instantiation of the wide-level kernel; the same bits either way.
 * Rules, those of mi_bilu4sp_solve_dev: an unprepared handle is prepared by its first solve, except under stream capture:
 * MI_ERR_STATE ("not prepared"), nothing enqueued, the capture stays valid; once prepared a solve allocates nothing, copies nothing
 * to the host and synchronises nothing; d_x == d_b is allowed; vectors need 8-byte alignment only; an overflow in the copy does
 * not block solves (mi_bilu4sp_status reports it); ONE solve at a time per ordered handle.
 * MI_ERR_ARG: a null handle or vector — before the device is touched; MI_ERR_NODEVICE: a host-only handle; nbrows == 0: a no-op. */
int mi_bilu4spx_solve_dev(mi_bilu4_t F, const double* d_b, double* d_x, mi_stream_t s);
int mi_bilu4spx_solve(mi_bilu4_t F, const double* b, double* x); /* host vectors: copied in and out */
/* of the last mi_bilu4spx_solve* (0 before the first): *launches_last, the two of an ordered handle included, and how many of them
 * took the wide-level kernel.  Any output may be NULL. */
int mi_bilu4spx_info(mi_bilu4_t F, int* launches_last, int* wide_launches_last);

/* ---- 4x4-block ILU(k): an opt-in MULTICOLOUR ORDERING behind the handle (mi_bilu4_create_ordered, mi_bilu4_order_*) ----
 * In the caller's (natural) ordering the exact solve is a chain of dependent levels (2 x (3 nx + 1) on the FE family).  Under a
 * multicolour numbering of the block rows, an exact ILU(0) solve has at most as many levels per sweep as there are colours — about
 * a dozen on the FE family, at most 1 + the largest block-row degree — and every level is a wide, contiguous, independent range
 * of rows.  The price: the handle factors B = Q A Q^T, and ILU of B is NOT ILU of A — a different, usually weaker preconditioner,
 * whose iteration counts are known only for the matrices that were measured (profiles/NOTES.md R15.1).  So the ordering is opt-in:
 * nothing chooses it, and mi_bilu4_create / mi_bilu4_create_host are untouched.
 * THE RULE (part of the interface): greedy colouring of the symmetrised block graph — the pattern of A + A^T without the diagonal,
 * so unsymmetric patterns are legal — block rows taken in ascending natural order, each taking the smallest colour that no
 * already-coloured neighbour holds.  New numbering: colour ascending, inside a colour the old row number ascending;
 * perm[old] = new (the convention of mi_csr_perm).  B's block columns are re-sorted ascending in the new numbering; symbolic
 * ILU(fill), levels, folding, both factorisations, the one-launch form, the sweeps and the f32 copy then run on B exactly as they
 * run on A in a natural-order handle.  At fill 0 fwd_levels and bwd_levels (mi_bilu4_info) are each <= ncolours; at fill > 0 the
 * ordering is allowed but promises nothing about levels (fill blocks join rows of one colour).
 * Every call on an ordered handle keeps its meaning in the CALLER's numbering: b, x, coef / d_coef of the refactors, the block
 * row a refused pivot or an overflow names — mi_bilu4_solve*, mi_bilu4_refactor, mi_bilu4dev_*, mi_bilu4_set_solve_form,
 * mi_bilu4one_*, mi_bilu4sw_*, mi_bilu4sp_*, mi_gmres_set_precond, the planned GMRES and a captured mi_gmres_cycle_dev.  TWO
 * EXCEPTIONS return the factor of B in the NEW numbering: mi_bilu4_factor_host and mi_bilu4sp_fetch.  ("The lowest refused row"
 * is the lowest in the new numbering, reported by its caller's number.)
 * Cost: an ordered handle owns two vectors of 4 nbrows doubles, allocated at create; every solve gathers b into the first and
 * scatters x out of the second — two extra launches per solve, counted in mi_bilu4_info's *launches (not in the sweeps'
 * launches_last; mi_bilu4_info's us[] time the factor's application on the internal vectors, without them) — and allocates nothing,
 * so solves stay capturable.  Consequence: ONE solve at a time per ordered handle.
 * d_x == d_b stays allowed; vectors need 8-byte alignment only.
 * An unfolded level of at least kBiluWideMin block rows (64: measured, every unfolded level; MI355_BILU_WIDE_MIN=<rows> at create
 * overrides it) is computed by a kernel written for wide levels (the sweeps' software pipeline); narrower ones by the kernel of
 * natural-order handles.  The same bits either way.  A natural-order handle never takes it: its launches are what they were.
 * mi_bilu4_create_ordered(.., MI_BILU_ORDER_NATURAL, ..) IS mi_bilu4_create (and _host_ordered _create_host): same factor, same
 * launches.  MI_ERR_ARG: an unknown ordering, MI355_BILU_WIDE_MIN < 1, and whatever mi_bilu4_create refuses.  (The declarators
 * are parenthesised like mi_bilu4_set_solve_form's: the `mi_bilu4_name(` entries are the level-by-level interface, a closed set;
 * these four are a closed set of their own.)  nbrows == 0: every call is a no-op, and mi_bilu4_order_info reports the ordering asked for. */
enum { MI_BILU_ORDER_NATURAL = 0, MI_BILU_ORDER_COLOUR = 1 };
int (mi_bilu4_create_ordered)(int nbrows, const int* ptrow, const int* indcol, const double* coef, int layout, int fill, int ordering,
                            mi_bilu4_t* out);
int (mi_bilu4_create_host_ordered)(int nbrows, const int* ptrow, const int* indcol, const double* coef, int layout, int fill,
                                 int ordering, mi_bilu4_t* out);
/* *ordering (MI_BILU_ORDER_*), *ncolours (0 in natural order), *wide_launches = launches of one exact solve in form 0 that take the
 * wide-level kernel, perm [nbrows] (the identity in natural order).  Any output may be NULL. */
int (mi_bilu4_order_info)(mi_bilu4_t F, int* ordering, int* ncolours, int* wide_launches, int* perm);
/* host-only: the ordering exactly as mi_bilu4_create_ordered builds it.  It first CHECKS its own result — perm is a permutation,
 * every colour an independent set of the symmetrised graph — and names the first violation with MI_ERR_STATE; only then does it
 * return perm [nbrows], *ncolours and colour_sizes (cap entries; MI_ERR_ARG when cap < *ncolours).  Any output may be NULL. */
int (mi_bilu4_order_probe)(int nbrows, const int* ptrow, const int* indcol, int ordering, int* perm, int* ncolours,
                         int* colour_sizes, int cap);

/* ---- right-preconditioned restarted GMRES with a whole cycle on the device (mi_gmres_*) ----
 * KSPGMRES of src/solve_newton.c:1156-1164, 1265 as one call: the products, the block ILU in any of its three forms, CGS2 out of
 * mi_cgs_dev and the small least-squares problem all run on the caller's stream; the host reads a 64-byte record (plus the
 * history entries so far of the cycle) every `check_every` iterations instead of draining the stream at every one.
 * ALL DEVICE STATE, THE RESULT INCLUDED, IS INDEPENDENT OF check_every: x, history, iterations and reason are the same bits for
 * every value; only the number of read-backs and of wasted steps (below) changes.
 * DEFINITION (part of the interface; m = restart; A M^-1 u = b, x = x0 + M^-1 u):
 *   solve      bnorm = mi_norm2_dev(b), or 1 if that is 0;  its = 0
 *   cycle      w = A x;  r_i = b_i - w_i (one rounded subtraction);  beta = the bits of mi_norm2_dev(r)
 *              the first cycle sets history[0] = beta / bnorm
 *              the solve ends here if beta / bnorm <= rtol (reason 0 when its == 0, else 1), else if its >= maxiter (2), else
 *              if beta is not finite (4);  V_0 = r / beta (IEEE division);  g_0 = beta
 *   step k     V_{k+1} = A (M^-1 V_k), written straight into row k + 1 of V;  mi_cgs_dev(passes = 2) in place against V_0..V_k
 *              gives h_0..h_k and nrm, kept untouched as hraw[k (m + 2) + j], nrm at j = k + 1 (mi_krylov_basis_cgs_dev's
 *              layout);  the small problem (below);  V_{k+1} = V_{k+1} / nrm (IEEE division)
 *   small      on a copy c of the raw column, for j < k:  t = cs_j c_j + sn_j c_{j+1};  c_{j+1} = (-sn_j) c_j + cs_j c_{j+1};
 *              c_j = t.  rho = sqrt(c_k c_k + nrm nrm); rho == 0 or not finite: reason 4, the step is NOT counted.  Else
 *              cs_k = c_k / rho, sn_k = nrm / rho;  R_kk = rho, R_jk = c_j (j < k);  g_{k+1} = (-sn_k) g_k, then g_k = cs_k g_k;
 *              its += 1;  history[its] = |g_{k+1}| / bnorm;  history[its] <= rtol: reason 1; otherwise nrm == 0: reason 3
 *              (with nrm == 0 the new g_{k+1} is 0: reason 3 can only be seen with a negative rtol)
 *   frozen     once a reason is set every later small-problem launch of the cycle returns at once; the Arnoldi launches already
 *              enqueued behind it still run and their output is never read: columns past the frozen k are not used by the
 *              update and not reported by mi_gmres_fetch_cycle
 *   cycle end  after m steps, at maxiter or frozen, with k counted steps (k == 0: no update): for i = k-1 .. 0:  s = g_i;
 *              s = s - R_ij y_j for j = i+1 .. k-1 ascending;  y_i = s / R_ii.  With M: u = 0, mi_maxpy_dev(y, V_0..V_{k-1}, u),
 *              z = M^-1 u, x_i = fma(1, z_i, x_i) (mi_axpy_dev).  Without M: mi_maxpy_dev(y, V_0..V_{k-1}, x).  The solve ends
 *              here with the cycle's reason, or with 2 when its >= maxiter; else the next cycle starts
 * ARITHMETIC of the small problem: every product, every sum, every difference, every division and the square root is rounded
 * once, to nearest; NOTHING is contracted into an fma.  tests/gmres_dev_model.py restates it in float64 scalars.
 * reason: 0 the initial guess already met rtol; 1 converged at rtol; 2 maxiter reached; 3 the Krylov space is exhausted (a new
 * direction of norm 0); 4 a non-finite quantity or rho = 0.  history (host, maxiter + 1 doubles, or NULL) receives
 * iterations + 1 entries.
 * HOST LOOP: steps are enqueued in batches of check_every (a cycle's first batch: check_every - 1, so that the record of the
 * cycle's start arrives one step early), clipped at the cycle's end and at maxiter; behind each batch the record
 * is copied to one of two pinned slots and an event recorded; the NEXT batch is enqueued before the host waits for the previous
 * batch's event, so the GPU never waits for the host inside a cycle.  The price: when a cycle freezes, the rest of its batch and
 * the batch behind it have run for nothing: at most 2 check_every - 1 steps, once per solve (*wasted_steps_last).  A cycle's end
 * is the one point where the host waits with nothing enqueued behind: the update takes k as a launch parameter.  Read-backs per
 * solve: at most ceil(iterations / check_every) + cycles + 1.  check_every = 1 still never lets the GPU wait inside a cycle and
 * measured fastest (profiles/NOTES.md R12.1); larger values spare the host thread.  A solve allocates nothing, copies only to pinned memory and never
 * synchronises the device.  x is complete on the stream when the call returns, not on the host.
 * The handle owns V (m + 1 rows, even leading dimension), two work vectors, the small state and the two pinned slots; it does
 * NOT own A or F: both must outlive it.  MI_GMRES_PC_EXACT calls mi_bilu4_solve_dev with the handle's current solve form, the
 * two sweep kinds mi_bilu4sw_solve_dev / mi_bilu4sp_solve_dev with the counts given; mi_gmres_set_precond prepares F for them.
 * MI_GMRES_PC_EXACT_F32 (mi_gmres_set_precond_ex only) calls mi_bilu4spx_solve_dev: the exact solve of the rounded factor.
 * ONE solve at a time per handle.  F's sweep work vectors are F's: two solvers on one F must not overlap.  Vectors need 8-byte
 * alignment only.  Under stream capture mi_gmres_solve_dev returns MI_ERR_STATE (it reads back) and enqueues nothing.
 * MI_ERR_ARG, before the device is touched: a null handle or vector, n < 1, restart outside 1..64, an operator or preconditioner
 * whose row count is not n, a mapped or non-square operator, check_every < 1, maxiter < 0, an unknown kind, a negative count;
 * MI_ERR_STATE: no operator set; MI_ERR_NODEVICE: no GPU (mi_gmres_create): there is no CPU fallback. */
typedef struct mi_gmres_s* mi_gmres_t;
enum { MI_GMRES_PC_EXACT = 0, MI_GMRES_PC_SWEEPS = 1, MI_GMRES_PC_SWEEPS_F32 = 2, MI_GMRES_PC_EXACT_F32 = 3 };
int mi_gmres_create(int n, int restart, mi_gmres_t* out);
int mi_gmres_set_operator_csr(mi_gmres_t G, mi_csr_t A);     /* square, unmapped, n rows: the arithmetic of mi_spmv_dev */
int mi_gmres_set_operator_bcsr4(mi_gmres_t G, mi_bcsr4_t A); /* 4 nbrows == n: the chain arithmetic of mi_bcsr4_spmv_dev */
/* F == NULL: no preconditioner (kind and counts ignored) */
int mi_gmres_set_precond(mi_gmres_t G, mi_bilu4_t F, int kind, int sweeps_fwd, int sweeps_bwd);
/* the same, and also MI_GMRES_PC_EXACT_F32: the exact solve over the single-precision copy (mi_bilu4spx_solve_dev; the handle is
 * prepared by mi_bilu4sp_prepare, the counts are ignored).  With F != NULL an unknown kind, and a negative count for the two sweep
 * kinds, are refused first, before the solver is looked at.  mi_gmres_set_precond keeps refusing kind 3 as unknown. */
int mi_gmres_set_precond_ex(mi_gmres_t G, mi_bilu4_t F, int kind, int sweeps_fwd, int sweeps_bwd);
/* d_x holds the initial guess and receives the solution; iterations, reason and history may be NULL */
int mi_gmres_solve_dev(mi_gmres_t G, const double* d_b, double* d_x, double rtol, int maxiter, int check_every, int* iterations,
                       int* reason, double* history, mi_stream_t s);
/* host vectors: copied in and out (two more device vectors, allocated by the first call) */
int mi_gmres_solve(mi_gmres_t G, const double* b, double* x, double rtol, int maxiter, int check_every, int* iterations, int* reason,
                   double* history);
/* the LAST cycle of the last solve (waits for the device): *k its counted steps; hraw [restart (restart + 2)] the raw columns
 * 0..k-1 in the layout above, zeros elsewhere; y [restart] the least-squares solution, zeros past k; *beta its ||r0||.  Any output
 * may be NULL */
int mi_gmres_fetch_cycle(mi_gmres_t G, int* k, double* hraw, double* y, double* beta);
/* *device_bytes of V, the work vectors and the small state; of the last solve: *readbacks_last, *launches_last (kernels of this
 * section and library calls enqueued, a product, a preconditioner application or an mi_cgs_dev each counted once),
 * *wasted_steps_last.  Only mi_gmres_solve_dev (and mi_gmres_solve through it) writes these three: mi_gmres_cycle_dev and
 * mi_gmres_plan_* leave them as the last such solve left them, 0 before any.  Any output may be NULL */
int mi_gmres_info(mi_gmres_t G, int* restart, long long* device_bytes, int* readbacks_last, int* launches_last, int* wasted_steps_last);
int mi_gmres_destroy(mi_gmres_t G);

/* ---- mi_gmres_* with an opt-in SINGLE-PRECISION KRYLOV BASIS (MI_BASIS_F32) ----
 * CGS2 reads the whole basis four times per iteration, and the basis is the largest object a solver owns.  Nothing in GMRES needs
 * 53 bits of every basis entry: if every projection is taken against the basis AS STORED, the Arnoldi relation holds to float
 * rounding, and the cycle's update and the next cycle's true residual remove that error (the compressed-basis GMRES of Aliaga,
 * Anzt et al.).  Nothing chooses this automatically: mi_gmres_create is mi_gmres_create_ex(.., MI_BASIS_F64), and with
 * MI_BASIS_F64 nothing changes, bit for bit, mi_gmres_info's device_bytes included.  The operator a MI_BASIS_F32 solve sees is
 * that of the rounded basis: its history and iteration count are close to the double basis's, not equal to them.
 * DEFINITION (part of the interface):
 *   round32(v) = (float)v    rounded to nearest, ties to EVEN (what numpy's astype(float32) does); float SUBNORMALS are kept, not
 *                            flushed; a finite v beyond the float range becomes +-Inf; -0 stays -0; NaN stays NaN
 *   widen(f)   = (double)f   exact
 * and a MI_BASIS_F32 solve is the DEFINITION of mi_gmres_* above with these changes and no others (the small problem and its
 * ARITHMETIC, hraw, R, g, y, the frozen state, the batches and check_every stay; the result stays independent of check_every):
 *   storage    V32: restart + 1 float rows, the leading dimension rounded up to a multiple of 4 (every row 16-byte aligned); one
 *              double vector q; the two double work vectors.  There is no double V
 *   cycle      r = b - A x into a work vector, beta as before;  V32_0[i] = round32(r_i / beta) (IEEE division), q_i = widen(V32_0[i])
 *   step k     w = A (M^-1 q) into a work vector;  mi_cgs_f32_dev(passes = 2) of w in place against V32_0..V32_k: d_j has the
 *              bits of mi_dot_dev(w, widen(V32_j)), the update is w_i = fma(-d_j, widen(V32_j[i]), w_i) in basis order, nrm has
 *              the bits of mi_norm2_dev of the new w, h = d(pass 1) + d(pass 2), one rounded add;  the small problem on the raw
 *              column, unchanged;  V32_{k+1}[i] = round32(w_i / nrm), q_i = widen(V32_{k+1}[i]) (mi_round_f32_dev): the vector
 *              fed to the next product is the STORED basis vector, not the unrounded one
 *   cycle end  as before, with mi_maxpy_f32_dev(y, V32_0..V32_{k-1}, .) in place of mi_maxpy_dev
 *   confirmed  the recurrence's residual is exact only to float rounding of the basis, so convergence is confirmed, not assumed:
 *              when a step sets reason 1 the cycle freezes and its update runs as before, but the solve does not end: the next
 *              cycle starts, and its start check (beta / bnorm <= rtol: the TRUE residual) reports reason 1; otherwise the solve
 *              goes on, or ends with reason 2 when its >= maxiter.  Reasons 0, 3 and 4 end the solve as before.  history keeps
 *              iterations + 1 entries: a confirming start adds none.  After a confirmed solve mi_gmres_fetch_cycle reports that
 *              last cycle: k = 0 and beta = the confirmed true residual norm.  A claim that the start behind it does not confirm
 *              is counted (refused_last).  COST: one product and one residual pass more per converged solve than the double
 *              basis (plus the check_every - 1 steps enqueued behind a cycle's start, which run for nothing as before)
 * mi_gmres_info's device_bytes counts what such a handle owns (V32, q, two work vectors, the small state).
 * MI_ERR_ARG: an unknown basis, and the rules of mi_gmres_create. */
enum { MI_BASIS_F64 = 0, MI_BASIS_F32 = 1 };
int mi_gmres_create_ex(int n, int restart, int basis, mi_gmres_t* out);
/* *basis the handle's; *basis_bytes of V (MI_BASIS_F64: 8 (restart + 1) ldv, ldv = n rounded up to even) or of V32 and q
 * (MI_BASIS_F32: 4 (restart + 1) ldv32 + 8 ldv, ldv32 = n rounded up to a multiple of 4); *refused_last: the unconfirmed claims of
 * the last solve (always 0 with MI_BASIS_F64).  Any output may be NULL */
int mi_gmres_basis_info(mi_gmres_t G, int* basis, long long* basis_bytes, int* refused_last);

/* ---- capturable GMRES: a whole cycle with no read-back, and the solve as replayed graphs (opt-in) ----
 * mi_gmres_solve_dev cannot be captured into a graph: it reads a record back between batches and hands the cycle's end the
 * counted steps k as a launch parameter.  Here a cycle is a FIXED sequence of launches: its start, all `restart` steps, its end;
 * what the host decided there is decided on the device.  Nothing chooses any of this automatically, mi_gmres_solve_dev keeps
 * refusing a capturing stream, and its results do not change by a bit.
 * DEFINITION: the arithmetic is that of mi_gmres_* above (and of MI_BASIS_F32), with these rules in place of the host's:
 *   step k     is not counted once the record holds a reason (frozen, as above) or once its >= maxiter: such a step's
 *              small-problem launch returns at once and writes no reason; its Arnoldi launches run and their output is never read
 *   cycle end  k is read from the record by the back-substitution and by the update (mi_maxpy_upto*_dev below); the final
 *              x_i = fma(1, z_i, x_i) runs only when k > 0: a cycle that counted no step leaves x untouched, bit for bit
 * so x, the record, hraw and y after mi_gmres_cycle_dev are those the same cycle of mi_gmres_solve_dev leaves, and for every
 * `segment` mi_gmres_plan_solve's x, history, iterations, reason, mi_gmres_fetch_cycle and refused_last are, bit for bit, those of
 * mi_gmres_solve_dev with the same arguments.
 * CAPTURE: mi_gmres_cycle_dev enqueues kernels and one memset, allocates nothing and copies nothing to the host, PROVIDED the
 * stream was prepared: the first reduction on a stream allocates its workspace and the first product of a relabelled operator on
 * a stream its gather buffer, and neither may happen under capture.  mi_gmres_prepare_stream does both outside capture;
 * mi_gmres_cycle_dev on a capturing stream that was not prepared returns MI_ERR_STATE ("not prepared"), enqueues nothing and
 * leaves the capture valid.  Setting the operator again forgets the prepared streams.  An exact ILU in the one-launch form is
 * recorded as the level-by-level form, as mi_bilu4_solve_dev does under capture (the same bits).  The captured launches name the
 * vectors, rtol, maxiter and the handles' device arrays: they hold as long as those do.  No kernel waits, spins or polls a flag.
 * WASTE: steps that run for nothing.  A raw cycle always runs all `restart` steps: restart - k of them are not counted.  A planned
 * solve enqueues whole segments and looks at a segment's record only after the next one is enqueued (a cycle's start counts as
 * a segment of no steps): when a cycle freezes or reaches maxiter, the rest of its segment and the segment behind it have run
 * for nothing, AT MOST 2 segment - 1 STEPS PER CYCLE THAT ENDS EARLY.  With MI_BASIS_F64 a solve has one such cycle; with
 * MI_BASIS_F32 a claimed cycle is one and its confirming start (segment steps behind it, at most) another.  *wasted_steps_last
 * is the sum over the solve. */
/* y <- mi_maxpy_dev(n, c, d_coef, negate, d_basis, y, NULL) with c = *d_count (DEVICE memory) clamped to [0, m]: the same
 * segments, lane pairs and per-element fma chain in basis order, so the new y has those bits.  Vectors and coefficients with
 * index >= c are never loaded (they may hold NaN or Inf); c == 0 leaves every bit of y alone.  Always ceil(m / tile) launches,
 * of which those past c return at once.  Nothing is allocated, nothing copied to the host; capturable on any stream.
 * MI_ERR_ARG, before the device is touched: the rules of mi_maxpy*_dev for the m vectors (m in 0..64, no null among the m
 * pointers, d_y not one of them, float vectors 8-byte aligned), or d_count null. */
int mi_maxpy_upto_dev(int n, int m, const int* d_count, const double* d_coef, int negate, const double* const* d_basis, double* d_y,
                      mi_stream_t s);
int mi_maxpy_upto_f32_dev(int n, int m, const int* d_count, const double* d_coef, int negate, const float* const* d_basis, double* d_y,
                          mi_stream_t s);
/* allocate, outside capture, whatever a first use on s would allocate (the reduction workspace; a relabelled operator's gather
 * buffer, via a throwaway product on the solver's own work vectors: not while a solve of G is in flight); idempotent.
 * MI_ERR_STATE: no operator set, or s is capturing */
int mi_gmres_prepare_stream(mi_gmres_t G, mi_stream_t s);
/* ONE whole restart cycle, enqueued with no read-back: the cycle start of the DEFINITION (first != 0: also ||b||, its = 0,
 * history[0]), `restart` steps, the cycle end with the device-side k.  Steps behind a reason, or at its >= maxiter, run but are
 * not counted.  The caller decides between cycles with mi_gmres_state, by mi_gmres_solve_dev's rule: stop when *done, or when
 * its >= maxiter (reason 2); else the next cycle with first = 0.  With MI_BASIS_F32 a reason 1 with k > 0 is a CLAIM, as in
 * mi_gmres_solve_dev: its update has run, and the next cycle (first = 0) confirms it (reason 1 with k = 0) or goes on. */
int mi_gmres_cycle_dev(mi_gmres_t G, const double* d_b, double* d_x, int first, double rtol, int maxiter, mi_stream_t s);
/* copies the record and the cycle's history entries to pinned memory behind s and waits for them (MI_ERR_STATE on a capturing
 * stream).  *its, *k, *reason (0..4 as mi_gmres_solve_dev reports them), *last the last history value, *beta the cycle's ||r0||;
 * *done != 0: the record holds a reason (rtol met at the start of a solve included, which *reason reports as 0);
 * history_cycle [restart]: the entries of the k counted steps, zeros behind.  Also what mi_gmres_fetch_cycle then reports.
 * Any output may be NULL */
int mi_gmres_state(mi_gmres_t G, mi_stream_t s, int* its, int* k, int* done, int* reason, double* last, double* beta,
                   double* history_cycle /* [restart] or NULL */);
/* The solve as replayed graphs.  mi_gmres_plan_create captures, once, on a private stream of the plan (prepared first, captured
 * in thread-local capture mode): one graph for the start of a solve, one for the start of a later cycle, one per segment (steps
 * j segment .. min(restart, (j + 1) segment) - 1) and one for the cycle's end; segment is clamped to restart:
 * 3 + ceil(restart / segment) graphs.  The plan bakes in d_b, d_x, rtol, maxiter and the operator and preconditioner settings
 * of G: refill b and x IN PLACE between solves; every mi_gmres_set_* on G makes the plan stale (mi_gmres_plan_solve: MI_ERR_STATE).
 * mi_gmres_plan_solve replays them on s with mi_gmres_solve_dev's host loop, the segments as batches: the next segment is
 * launched before the host waits for the previous segment's record; the cycle's end is replayed when a record shows a reason,
 * after the last segment or at its >= maxiter (not at all when k == 0); the end of the solve, the reasons, the float basis's
 * claim / confirm and refused_last are mi_gmres_solve_dev's.  history: maxiter + 1 doubles or NULL.  MI_ERR_STATE on a
 * capturing stream.  ONE solve at a time per G and per F, planned or not; G must outlive its plans' solves.
 * mi_gmres_plan_info: *graphs, *segment (as clamped), and of the last solve *replays_last (graph launches), *readbacks_last,
 * *wasted_steps_last (WASTE above).  Any output may be NULL.
 * MI_ERR_ARG, before the device is touched: segment < 1, maxiter < 0, a null handle, vector or output. */
typedef struct mi_gmres_plan_s* mi_gmres_plan_t;
int mi_gmres_plan_create(mi_gmres_t G, const double* d_b, double* d_x, double rtol, int maxiter, int segment, mi_gmres_plan_t* out);
int mi_gmres_plan_solve(mi_gmres_plan_t P, int* iterations, int* reason, double* history, mi_stream_t s);
int mi_gmres_plan_info(mi_gmres_plan_t P, int* graphs, int* segment, int* replays_last, int* readbacks_last, int* wasted_steps_last);
int mi_gmres_plan_destroy(mi_gmres_plan_t P);

/* ---- 4x4-block DILU applied with EISENSTAT'S TRICK: a GMRES step with no separate product (mi_dilu4_*, opt-in) ----
 * A preconditioned GMRES step reads the matrix twice: once for the product, once (as many bytes again) for the ILU(0) factor.
 * For a preconditioner whose off-diagonal blocks are the matrix's OWN the second reading can be had for free.  Write
 * B = L + D + U (strict block triangles, block diagonal) and M = (E + L) E^-1 (E + U) with the block DILU pivots E.  Then
 * B = (E + L) + (E + U) - (2E - D), and the split-preconditioned operator A^ = (E + L)^-1 B (E + U)^-1 E costs ONE backward
 * and ONE forward triangular sweep over B's blocks — one preconditioner application, and no product.  The handle keeps B's strict
 * triangles level-major, and Einv = E^-1 and K = 2E - D per block row: no factor, no fill.
 * Ordering: MI_BILU_ORDER_NATURAL or MI_BILU_ORDER_COLOUR — the rule, perm and the two boundary launches of ordered mi_bilu4
 * handles: B = Q A Q^T, and EVERY call keeps the caller's numbering (vectors, coef, the block row a refused pivot names, the
 * rows mi_dilu4_fetch returns).  DILU of B is not DILU of A; in the colour order it measured as good as ILU(0) there, in the
 * natural order about half as good (profiles/NOTES.md R21.1).  Nothing chooses this preconditioner: it is opt-in.
 * Schedule: the dependency levels and the folding of mi_bilu4 at fill 0 on B's pattern: one launch per level, a run of levels of
 * fewer than 64 block rows folded into one workgroup.
 * PIVOTS (part of the interface; chain, the 4x4 product of sixteen chains and the Gauss-Jordan inverse with its 1e-12 refusal are
 * those of mi_bilu4 above): block rows i of B ascending: E_i = D_i; for every j < i ascending with BOTH blocks (i, j) and (j, i) in
 * the pattern: T = B_ij . Einv_j, P = T . B_ji, E_i = E_i - P, one rounded subtraction per entry; Einv_i = inverse(E_i);
 * K_i = (2 E_i) - D_i per entry: an exact doubling, then one rounded subtraction.  The rows of a level are computed by several host
 * threads (MI355_BILU_THREADS); the bits do not depend on the count.  A refused pivot: MI_ERR_ARG with the caller's block row.
 * THE THREE OPERATIONS (chain(a, t) = fma(a3,t3, fma(a2,t2, fma(a1,t1, a0*t0))); every + and - below is one rounded operation;
 * blocks of a row in ascending column of B; rows in level order):
 *   to_hat     b^ = (E + L)^-1 r.        forward:  a = 0; a_q = a_q + chain(L_ij row q, b^_j); s_q = r_iq - a_q;
 *                                                  b^_iq = chain(Einv_i row q, s)
 *   from_hat   x = (E + U)^-1 E u.       backward: a = 0; a_q = a_q + chain(U_ij row q, x_j); c_q = chain(Einv_i row q, a);
 *                                                  x_iq = u_iq - c_q
 *   apply_hat  w = A^ u.                 t = from_hat(u) into a work vector of the handle; forward: a_q = chain(K_i row q, t_i);
 *                                                  a_q = a_q + chain(L_ij row q, y_j); c_q = chain(Einv_i row q, a);
 *                                                  y_iq = u_iq - c_q; w_iq = t_iq + y_iq   (y: a second work vector)
 * Every row is ONE fixed sequence of roundings, independent of the schedule, the folding and the alignment.  Each operation is
 * enqueued on the caller's stream, allocates nothing, synchronises nothing and can be captured into a graph; output == input is
 * allowed; vectors need 8-byte alignment only.  ONE operation at a time per handle (the work vectors are the handle's).
 * SOLVING WITH IT: the caller composes  r = b - A x0 (the one true product);  b^ = to_hat(r);  u^ = 0, GMRES on A^ u^ = b^
 * (mi_gmres_set_operator_dilu4);  x = x0 + from_hat(u^).  rtol AND THE HISTORY OF THAT SOLVE ARE IN THE HAT NORM,
 * ||(E + L)^-1 r|| / ||b^||, not in the norm of r: compare solves by their true residuals.
 * mi_dilu4_refactor: new values, same pattern; runs on the host, waits for the device, uploads (as mi_bilu4_refactor).
 * mi_dilu4_fetch: Einv and K, 16 doubles per block row, row-major, by the CALLER's block row (either may be NULL).
 * mi_dilu4_info: *nblocks of B, *ordering, *ncolours (0 in natural order), levels of the two sweeps, *launches of one apply_hat
 * (both sweeps after folding, + 2 on an ordered handle), *factor_seconds of the last host computation of the pivots, *device_bytes
 * the handle owns on the device (0 on a host-only handle), perm [nbrows] (perm[caller's row] = B's).  Any output may be NULL.
 * mi_dilu4_create_host: no device (refactor, fetch, info work; the three operations return MI_ERR_STATE).
 * MI_ERR_ARG: what mi_bilu4_create refuses in a pattern, an unknown layout or ordering, a null argument, a refused pivot.
 * nbrows == 0: every call is a no-op.  NOT built: a single-precision copy, Jacobi sweeps, a one-launch form, an automatic
 * choice, mi_dist, a symbolic phase on the device.  The refactorisation on the device is mi_dilu4dev_*, below. */
typedef struct mi_dilu4_s* mi_dilu4_t;
int mi_dilu4_create(int nbrows, const int* ptrow, const int* indcol, const double* coef, int layout /* MI_BLOCK_* */,
                    int ordering /* MI_BILU_ORDER_* */, mi_dilu4_t* out);
int mi_dilu4_create_host(int nbrows, const int* ptrow, const int* indcol, const double* coef, int layout, int ordering, mi_dilu4_t* out);
int mi_dilu4_destroy(mi_dilu4_t E);
int mi_dilu4_refactor(mi_dilu4_t E, const double* coef, int layout);
int mi_dilu4_fetch(mi_dilu4_t E, double* einv, double* k);
int mi_dilu4_info(mi_dilu4_t E, int* nbrows, long long* nblocks, int* ordering, int* ncolours, int* fwd_levels, int* bwd_levels,
                  int* launches, double* factor_seconds, long long* device_bytes, int* perm);
int mi_dilu4_to_hat_dev(mi_dilu4_t E, const double* d_r, double* d_bhat, mi_stream_t s);
int mi_dilu4_from_hat_dev(mi_dilu4_t E, const double* d_u, double* d_x, mi_stream_t s);
int mi_dilu4_apply_hat_dev(mi_dilu4_t E, const double* d_u, double* d_w, mi_stream_t s);
/* The operator of mi_gmres_*'s DEFINITION becomes A^: every "A x" there is mi_dilu4_apply_hat_dev(E, x, .) — the eager solve, the
 * float basis, mi_gmres_cycle_dev and the plans alike; everything else in the DEFINITION is untouched.  4 nbrows == n.  The
 * preconditioner must be NULL (M is inside A^): MI_ERR_STATE otherwise, and mi_gmres_set_precond* with F != NULL is refused with
 * MI_ERR_STATE while this operator is set.  E is not owned and must outlive G; one solve at a time per E. */
int mi_gmres_set_operator_dilu4(mi_gmres_t G, mi_dilu4_t E);

/* ---- 4x4-block DILU: the pivots recomputed on the GPU from values on the device (mi_dilu4dev_*) ----
 * A Newton step re-assembles the Jacobian and refactors before every linear solve (src/solve_newton.c:1245-1265);
 * mi_dilu4_refactor does that on host threads, waits for the device and uploads both triangles, Einv and K.
 * mi_dilu4dev_refactor computes the same state (the PIVOTS above, operation for operation: after it the device holds, bit for
 * bit, what mi_dilu4_refactor would have uploaded for the same values — both triangles level-major, Einv, K) on the GPU, on the
 * caller's stream, from block values that already lie on the device, in place into the arrays the three operations read.
 * Schedule: the forward sweep's levels and launches (row i needs Einv_j only of the rows j it has an L block to), after ONE
 * launch that scatters the values into both triangles, puts D_i into Einv_i and K_i and resets the refusal word: launches per
 * refactor = forward launches + 1.  Sixteen lanes per block row, one per entry of a block; the block (j, i) of every L block
 * (i, j) is looked up once per handle, not once per refactor.
 * ORDERING is the caller's business, as it is for the operations: a refactor on stream s is ordered with operations on s only.
 * An operation running on another stream during a refactor reads half-written pivots.
 * Refused pivot: the refactor itself cannot report it (nothing is copied back); mi_dilu4dev_status does.  As on the host, the
 * rows of later levels are then not computed and the handle must be refactored, by either path, before it is used.
 * The host copies (what mi_dilu4_fetch returns) are NOT updated by a device refactor until mi_dilu4dev_fetch copies them back;
 * mi_dilu4_refactor replaces host and device state as before.  Creation still computes the pivots on the host.
 * mi_dilu4_info and its device_bytes are unchanged; the tables of the device refactor are counted by mi_dilu4dev_info.
 * MI_ERR_ARG: a null handle, null d_coef, an unknown layout; MI_ERR_STATE: a host-only handle (_prepare, _refactor, _status,
 * _fetch).  nbrows == 0: every call is a no-op. */
/* host-only: the device refactor's plan for a pattern under `ordering` (MI_BILU_ORDER_*), built exactly as mi_dilu4dev_prepare
 * builds it AND replayed against the pattern (MI_ERR_STATE naming the first violation): *pivot_pairs = the updates
 * E_i -= (B_ij Einv_j) B_ji of one refactor (once per Newton step, src/solve_newton.c:1245-1265), *launches per refactor,
 * *plan_bytes of its tables (below).  Refuses what mi_dilu4_create refuses in a pattern or an ordering, with its messages */
int mi_dilu4dev_plan_probe(int nbrows, const int* ptrow, const int* indcol, int ordering, long long* pivot_pairs, int* launches,
                           long long* plan_bytes);
/* build, check and upload the pattern-only tables of the device refactor (idempotent; allocates, may synchronise: not
 * capturable): every block row's position in the forward sweep, per block of the device state the caller's block that lands
 * there, and per L block (i, j) the place of block (j, i) or that there is none.  Pattern-only: once per handle, not once per
 * Newton step (src/solve_newton.c:1245-1265) */
int mi_dilu4dev_prepare(mi_dilu4_t E);
/* new values, same pattern (src/solve_newton.c:1245-1265), d_coef on the device in the CALLER's block order, as the arrays given at
 * create (16 per block, `layout`; 8-byte alignment suffices); asynchronous on s: nothing allocated, copied or synchronised once
 * prepared (so it can be captured into a graph); calls mi_dilu4dev_prepare itself when needed (that first call is not capturable) */
int mi_dilu4dev_refactor(mi_dilu4_t E, const double* d_coef, int layout, mi_stream_t s);
/* waits for the device, hence for the last mi_dilu4dev_refactor (src/solve_newton.c:1245-1265); *bad_row = -1 and MI_OK, or the
 * CALLER's block row of the refused pivot and MI_ERR_ARG with the same message mi_dilu4_refactor gives (|d| < 1e-12); MI_OK before
 * any device refactor */
int mi_dilu4dev_status(mi_dilu4_t E, int* bad_row);
/* waits, then copies the device's triangles, Einv and K back into the host copies, so that mi_dilu4_fetch returns what the device
 * holds (the pivots after the refactor of src/solve_newton.c:1245-1265) */
int mi_dilu4dev_fetch(mi_dilu4_t E);
/* *prepared, *launches per refactor, *plan_bytes of device tables beyond what mi_dilu4_info counts (0 until prepared); any output
 * may be NULL (src/solve_newton.c:1245-1265: the cost of refactoring per Newton step) */
int mi_dilu4dev_info(mi_dilu4_t E, int* prepared, int* launches, long long* plan_bytes);

/* ---- row-range partition of one matrix over the GPUs of a node ----------
 * New design (the reference has no distributed code).  Rank r
 * owns global rows [row_starts[r], row_starts[r+1]) and the matching slice of
 * x and y.  Columns are relabelled to [0,n_local) owned | [n_local,
 * n_local+n_halo) ghosts (ascending global id, hence contiguous per owner);
 * rows are split into interior (no ghost column) and boundary rows so the
 * interior SpMV overlaps the halo exchange.  The exchange itself is done by
 * the caller (torch.distributed over RCCL in bench.py) between
 * mi_part_pack_dev and mi_part_spmv_boundary_dev.
 *
 * Planning functions are host-only and work without a GPU. */
int mi_part_create(int nranks, int rank, const long long* row_starts, const int* ptrow,
                   const int* indcol_global, const double* coef, mi_part_t* out);
int mi_part_destroy(mi_part_t P);
int mi_part_sizes(mi_part_t P, int* n_local, int* n_halo, int* n_interior_rows, int* n_boundary_rows);
int mi_part_recv_counts(mi_part_t P, int* counts /* [nranks] */);
int mi_part_recv_ids(mi_part_t P, int peer, long long* ids /* [recv_counts[peer]] global, ascending */);
int mi_part_set_send_ids(mi_part_t P, int peer, int count, const long long* ids /* global ids peer needs from me */);
int mi_part_send_counts(mi_part_t P, int* counts /* [nranks] */);
/* local pieces on the host, for CPU checks: which = 0 interior, 1 boundary, 2 = the one-launch step's piece: ALL local rows
 * in natural order (rowmap NULL), columns numbered [ghosts of lower ranks | owned | ghosts of higher ranks];
 * mi_part_combined_info gives the number of ghosts in front */
int mi_part_local_csr(mi_part_t P, int which, int* nrows, const int** ptrow, const int** indcol_local,
                      const double** coef, const int** rowmap);
int mi_part_combined_info(mi_part_t P, int* n_left);
/* *contiguous = 1 when every send list of this rank is a run of consecutive local ids (banded partitions with whole-range halos): the
 * RCCL step (mi_part_spmv_dev) then sends slices of x in place and launches no pack kernel. */
int mi_part_sends_contiguous(mi_part_t P, int* contiguous);
int mi_part_send_index(mi_part_t P, int* total, const int** local_idx /* packed by peer, ascending */);
/* upload the two pieces and the send index to the current device */
int mi_part_finalize(mi_part_t P);
int mi_part_set_kernel(mi_part_t P, int kernel_id);
/* new coefficients for an unchanged pattern: this rank's values in the order of the arrays given to mi_part_create
 * (host pointer; after mi_part_finalize).  Every piece of the handle is refreshed, plans and exchange set-up are kept. */
int mi_part_update_values(mi_part_t P, const double* coef);
/* per step, on device: x_ext = [x_local | halo], sendbuf packed by peer */
int mi_part_pack_dev(mi_part_t P, const double* d_x_ext, double* d_sendbuf, mi_stream_t s);
int mi_part_spmv_interior_dev(mi_part_t P, const double* d_x_ext, double* d_y_local, mi_stream_t s);
int mi_part_spmv_boundary_dev(mi_part_t P, const double* d_x_ext, double* d_y_local, mi_stream_t s);

/* ---- native halo exchange: RCCL point-to-point over xGMI, driven from C++ ----
 * Optional fast path for the whole step (pack, exchange on the partition's own comm
 * stream, interior overlapped, boundary) with no per-step host work outside this
 * library.  librccl is resolved at run time (dlopen); when it is missing these
 * return MI_ERR_UNSUPPORTED and the caller keeps exchanging the halos itself.
 * Bootstrap: rank 0 obtains a 128-byte id and hands it to every rank by any
 * side channel (bench.py: torch.distributed broadcast); then ALL ranks call
 * mi_part_comm_init collectively. */
#define MI_COMM_ID_BYTES 128
int mi_comm_available(void); /* MI_OK iff librccl could be resolved in this process */
int mi_comm_unique_id(void* id128);
int mi_part_comm_init(mi_part_t P, const void* id128);
/* what the communicator made by mi_part_comm_init says about itself (ncclCommCount / ncclCommUserRank): *comm_ranks = 0 and
 * *comm_rank = -1 when the handle has none.  bench.py prints it as `rccl_ranks`, so that a multi-GPU line shows how many ranks
 * RCCL really connected. */
int mi_part_comm_info(mi_part_t P, int* comm_ranks, int* comm_rank);
/* y_local = (A x)_local: d_x_ext = [x_local | halo], the halo part is overwritten.
 * Cross-stream hand-offs are HIP events; MI355_PART_HANDOFF=flags selects one-wave flag kernels instead
 * (cheaper, but a wait on a stalled peer then spins on the GPU: it gives up after minutes and the give-up is
 * sticky — this call, mi_part_status and mi_part_destroy return MI_ERR_HIP from then on). */
int mi_part_spmv_dev(mi_part_t P, double* d_x_ext, double* d_y_local, mi_stream_t s);
/* MI_OK, or MI_ERR_HIP once a hand-off wait has given up (call after synchronising; no GPU work, no copy) */
int mi_part_status(mi_part_t P);
/* The ALL-GATHER form of that step, for wide halos (an FE slab partition: a whole mesh plane per neighbour, 38 648 ghosts of 163 048
 * rows at N = 8): instead of one grouped ncclSend / ncclRecv pair per neighbour, every rank contributes ONE fixed-size slice — the
 * entries anybody needs from it, i.e. the sorted union of its send lists, padded to the largest such union M — to one ncclAllGather
 * on the comm stream, and every ghost is picked out of the gathered nranks x M buffer (BASELINE north_star: "RCCL all-gather of halo x
 * entries over xGMI overlapped with interior SpMV").  Set-up (collective, after mi_part_comm_init): mi_part_send_union on every rank,
 * all-gather the counts and the GLOBAL ids (local id + the rank's first row) by any side channel, mi_part_allgather_setup with all of
 * them; mi_part_set_allgather(P, 1) on EVERY rank (or on none) selects the form for mi_part_spmv_dev.  Same bits either way. */
int mi_part_send_union(mi_part_t P, int* count, const int** local_idx /* ascending local ids; valid until the handle is destroyed */);
int mi_part_allgather_setup(mi_part_t P, const int* counts /* [nranks] */, const long long* ids /* every rank's union as global ids, rank after rank */);
int mi_part_set_allgather(mi_part_t P, int on);
int mi_part_allgather_info(mi_part_t P, int* ready, int* in_use, int* slice /* M */);
/* ---- halo exchange by peer push (no RCCL, one stream) -------------------------
 * Each rank's kernel writes the x entries a neighbour needs straight into a receive window in the NEIGHBOUR's memory
 * (HIP IPC mapping; xGMI between GPUs) and raises a flag there; the receiver's kernel waits for its neighbours' flags and
 * moves the window behind x_local (navierstokes_amd/csrc/push_exchange.hpp has the protocol).  The step is four launches
 * on the caller's stream — push, interior rows, wait + copy, boundary rows — with no RCCL call, no second stream and no
 * cross-stream hand-off.  Set-up (collective, once): every rank calls mi_part_push_export, the 64-byte handles and the
 * (2*nranks+1)-entry layouts are all-gathered by any side channel, every rank calls mi_part_push_connect with all of
 * them.  One PROCESS per rank (ranks as threads of one process share hardware queues and can deadlock in the wait).
 * All ranks must then call mi_part_spmv_push_dev the same number of times (the flags carry the step number; for the same reason the
 * call refuses to be captured into a HIP graph: MI_ERR_UNSUPPORTED).
 * A wait on a stalled neighbour gives up after minutes; that is sticky and reported like a hand-off time-out. */
#define MI_IPC_HANDLE_BYTES 64
int mi_part_push_export(mi_part_t P, void* handle64, long long* layout /* [2*nranks + 1] */);
int mi_part_push_connect(mi_part_t P, const void* handles /* nranks x 64 B */, const long long* layouts /* nranks x (2*nranks+1) */);
int mi_part_spmv_push_dev(mi_part_t P, double* d_x_ext, double* d_y_local, mi_stream_t s);
/* *fused = 1: the step is ONE launch — when all local rows form a piece the sliced-stream kernel (round 5: spmv_sstream_fused) or the
 * ring kernel (spmv_ring.hpp, FUSED) serves, the push duty and the ghost reads (straight from the window, behind an in-kernel wait)
 * live inside that kernel, in the few workgroups / runs whose rows touch ghosts; these get a shorter share of the rows, push first and wait
 * second (mi_part_kernel_name(P, 2) names the kernel; MI355_PUSH_FUSED=0 disables the form, MI355_PUSH_FUSED_KERNEL=ring|sstream|csr_ext forces
 * one).  A rank whose rows have the 4x4 node structure runs the blocked kernel's one-launch form, spmv_bcsr4_fused_ext
 * (spmv_bcsr4_ext.hpp): the launch's first workgroups push, wait and copy the window once into a cached buffer of the handle, the
 * workgroups whose rows name ghosts wait for THEM and read that buffer (MI355_PUSH_FUSED_EXT=0 keeps the four launches for such
 * ranks; ranks that share a device — a neighbour's window lives on this rank's device — run it as two launches, so that only the
 * exchange's few workgroups wait in-kernel: MI355_PUSH_EXT_SPLIT=0|1 forces).  A rank that gets none of these forms (scalar rows, a halo
 * too wide for the sliced stream's and the ring's fused forms: a 3-D mesh operator over ranks) runs the same staged step on the stream
 * kernel's row blocks, spmv_csr_fused_ext (MI355_PUSH_FUSED_CSR_EXT=0 keeps the four launches).  In the fused forms the halo part of d_x_ext is
 * neither read nor written (d_x_ext must still hold n_local + n_halo entries for the four-launch form the ranks may have to
 * agree on). */
int mi_part_push_info(mi_part_t P, int* ready, int* fused, int* neighbours);
/* the kernel a piece's products launch (as rocprofv3 names it): which = 0 the interior rows' piece, 1 the boundary rows', 2 the combined piece
 * of the one-launch push step — spmv_sstream_fused<...> (round 5) wherever that piece holds a sliced copy, else the ring kernel's FUSED
 * form, the blocked one (spmv_bcsr4_fused_ext) or the staged scalar one (spmv_csr_fused_ext); "" when the step is not fused.  The string lives until the thread's next call. */
const char* mi_part_kernel_name(mi_part_t P, int which);
/* Step down from the one-launch form to the four-launch form (push, interior rows, wait + copy, boundary rows).  All ranks must
 * drive the step the same way; the caller compares mi_part_push_info's `fused` across ranks and calls this where they differ. */
int mi_part_push_unfuse(mi_part_t P);
/* give the push exchange up again (e.g. after a failed collective self-check): windows released, sticky give-ups cleared */
int mi_part_push_disable(mi_part_t P);
/* development check of the RCCL plumbing on ONE GPU: a communicator of size 1 sends
 * `count` doubles to itself through the same send/recv/stream/event code path
 * (the per-step cost measurements of this path live in tools/comm_timing.hip) */
int mi_comm_selftest(int count, double* max_abs_err);

/* ---- ONE process, N GPUs: the row-range partition behind a single handle -------------------------------------------
 * "mi_dist_create(ndev, ...)"; "Threading: one host thread drives all GPUs (or one per GPU internally), hidden
 * behind the ABI".  The reference's callers are single-process C++ programs that call SpMV_CSR(y, x, A) from one thread
 * (mpk/2SpMV.cpp:128-141, mpk/SpM2V.cpp:885-889, mpk/SpMVmulti0.cpp:369-411 behind the seam mpk/SpMV.h:52-66): this is the form
 * of the multi-GPU path they can reach (the mpk/SpMV.h shim routes to it with MI355_NGPUS=N).  The
 * mi_part_* entry points above are its per-rank building blocks and stay what a process-per-GPU host (bench.py, torch.distributed)
 * drives itself.
 *
 * mi_dist_create cuts the n rows into ndev contiguous ranges of (nearly) equal nonzero count — at node boundaries for a matrix
 * with exact 4x4 node-block structure —, plans every rank's share (partition.hpp: columns relabelled to owned | ghosts, each
 * row's nonzeros kept in the caller's order, so every row of y is the CSR-ordered fma chain of SpMV_CSR_FMA for every ndev),
 * uploads rank r's pieces to device r mod (devices present) — MI355_DIST_DEVICES="0,2,..." overrides the map — and starts one
 * worker thread per rank, which enqueues that rank's launches from then on.  Host pointers; the caller's arrays are not retained.
 * The halo exchange of a step is chosen at create (mi_dist_exchange_name / _note say which and why):
 *   "push"   ranks on distinct devices with peer access: the peer-push step of mi_part_spmv_push_dev (one launch per rank in its
 *            fused form) with the neighbours' windows reached through peer pointers;
 *   "rccl"   mi_part_spmv_dev per rank (grouped ncclSend / ncclRecv on the rank's comm stream);
 *   "event"  any rank-to-device map, N ranks on ONE device included: halo entries copied straight into the peers' vectors with
 *            hipMemcpyPeerAsync on the sender's stream, ordered by HIP events.
 * A candidate is used only after one product through it equalled one through the event exchange bit for bit on every rank.
 * MI355_DIST_EXCHANGE=event|push|rccl forces one (create fails if it is not usable). */
typedef struct mi_dist_s* mi_dist_t;
typedef struct mi_dist_vec_s* mi_dist_vec_t; /* a vector distributed like the rows: per rank [owned | halo] on the rank's device */
int mi_dist_create(int ndev, int n, const int* ptrow, const int* indcol, const double* coef, mi_dist_t* out);
int mi_dist_destroy(mi_dist_t D);
/* *exchange: 0 event, 1 push, 2 rccl; *fused = 1: the push step is one launch per rank; halo_*: ghost entries over all ranks / of the largest */
int mi_dist_info(mi_dist_t D, int* nranks, int* distinct_devices, int* exchange, int* fused, long long* halo_total, long long* halo_max);
const char* mi_dist_exchange_name(mi_dist_t D);
const char* mi_dist_exchange_note(mi_dist_t D); /* what was tried at create, in order, and why a candidate was dropped */
int mi_dist_rank_info(mi_dist_t D, int rank, int* device, long long* row_start, int* n_local, int* n_halo, long long* nnz_local,
                      mi_stream_t* stream /* the stream the rank's work is enqueued on */);
/* new coefficients for an unchanged pattern, in the order of the arrays given to mi_dist_create (see mi_csr_update_values) */
int mi_dist_update_values(mi_dist_t D, const double* coef);
/* Host vectors of length n — the reference's calling convention: scatter, compute, gather, synchronise.
 *   mi_dist_spmv          y = A x                                  SpMV_CSR{,_OPT,_FMA,_AVX2}, mpk/SpMV.cpp:6-85
 *   mi_dist_spmk          y_out[p] = A^(p+1) x, one exchange per power   SpM2V_CSR mpk/SpM2V.cpp:79-112, SpM3V / SpM4V mpk/SpMVmulti0.cpp:132-221
 *   mi_dist_dot           every rank's fixed-tree partial (mi_dot_dev), summed on the host in rank order: deterministic for a given
 *                         ndev, inside the bound documented at mi_dot
 *   mi_dist_orthogonalize x3 = fma(-(alpha * beta), b, x1) with beta = that dot   orthogonalize, mpk/SpMVmulti.cpp:146-151
 *                         (x3 == x1 allowed: the in-place form of mpk/2SpMV.cpp:3-11); given beta the update is the reference's bits */
int mi_dist_spmv(mi_dist_t D, const double* x, double* y);
int mi_dist_spmk(mi_dist_t D, int k, const double* x, double* const* y_out);
int mi_dist_dot(mi_dist_t D, const double* x, const double* y, double* out);
int mi_dist_orthogonalize(mi_dist_t D, const double* b, const double* x1, double* x3, double alpha, double* beta_out);
/* Device-resident vectors (a solver that keeps its vectors on the GPUs between products).  mi_dist_vec_set / _get move a full
 * host vector in / out (synchronous); mi_dist_vec_ptr gives rank r's buffer (n_local + n_halo doubles on the rank's device; the
 * owned entries first) for the caller's own kernels, to be enqueued on the rank's stream (mi_dist_rank_info). */
int mi_dist_vec_create(mi_dist_t D, mi_dist_vec_t* out);
int mi_dist_vec_destroy(mi_dist_vec_t v);
int mi_dist_vec_set(mi_dist_vec_t v, const double* host /* [n] */);
int mi_dist_vec_get(mi_dist_vec_t v, double* host /* [n] */);
int mi_dist_vec_ptr(mi_dist_vec_t v, int rank, double** d_ptr);
/* Asynchronous: the step is enqueued on every rank's stream when the call returns; mi_dist_synchronize waits for all ranks and
 * reports an in-kernel wait that gave up (push) or a hand-off time-out (rccl).  x and y (and the k outputs) must be distinct vectors. */
int mi_dist_spmv_dev(mi_dist_t D, mi_dist_vec_t x, mi_dist_vec_t y);
int mi_dist_spmk_dev(mi_dist_t D, int k, mi_dist_vec_t x, const mi_dist_vec_t* y_out /* host array of k vectors */);
int mi_dist_synchronize(mi_dist_t D);
/* the reductions return their scalar on the host and therefore synchronise */
int mi_dist_dot_dev(mi_dist_t D, mi_dist_vec_t a, mi_dist_vec_t b, double* out);
int mi_dist_orthogonalize_dev(mi_dist_t D, mi_dist_vec_t b, mi_dist_vec_t x1, mi_dist_vec_t x3, double alpha, double* beta_out);

#ifdef __cplusplus
}
#endif
#endif /* MI355_SPMV_H */
