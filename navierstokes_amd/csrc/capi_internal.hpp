// capi_internal.hpp — state shared by the translation units that implement include/mi355_spmv.h:
// error helpers, the handle structs, and the few functions one unit needs from another.  The library is
// built from capi_lib.hip (library / device / cache flush), capi_csr.hip (CSR handles: create, plans,
// autotuner, products), launch_csr.hip (the CSR kernels' instantiations and launch_spmv), capi_blas1.hip,
// capi_bcsr.hip (BCSR 4x4, multi-vector products, Krylov basis), capi_ilu.hip (block ILU preconditioner), capi_dilu.hip (block DILU with Eisenstat's trick), capi_gmres.hip (restarted GMRES) and capi_part.hip
// (partition, RCCL and peer-push exchange); devtools.hip (mi355_devtools.h) is linked into libmi355spmv_dev.so only.
#pragma once
#include "mi355_spmv.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <chrono>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "dev_array.hpp"
#include "dispatch.hpp"
#include "partition.hpp"
#include "push_exchange.hpp"
#include "ring_plan.hpp"
#include "spmv_kernels.hpp"
#include "spmv_ring.hpp"
#include "spmv_sstream_mw.hpp"

using namespace mi355;

// ---------------------------------------------------------------- errors
extern thread_local std::string g_err; // capi_lib.hip

static inline int fail(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}

// `what`: the call that failed, as the error text names it
static inline int hip_fail(hipError_t e, const char* what)
{
    const int code = (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver) ? MI_ERR_NODEVICE
                                                                                                               : (e == hipErrorOutOfMemory ? MI_ERR_ALLOC : MI_ERR_HIP);
    return fail(code, std::string(what) + ": " + hipGetErrorString(e));
}

// HIP_TRY_AS: an operation of an owning type (dev_array.hpp), reported under the name of the HIP call it makes
#define HIP_TRY_AS(what, expr)                            \
    do {                                                  \
        hipError_t e_ = (expr);                           \
        if (e_ != hipSuccess) return hip_fail(e_, what);  \
    } while (0)
#define HIP_TRY(expr) HIP_TRY_AS(#expr, expr)

#define CHECK_ARG(cond, msg)                        \
    do {                                            \
        if (!(cond)) return fail(MI_ERR_ARG, msg);  \
    } while (0)


// the MI_* forms of the owning types' operations (dev_array.hpp), for `(rc = ...) ||` chains; at_least: a floor, in entries, where the site wants one
template <class T> static inline int dev_alloc(DevArray<T>& a, size_t n, size_t at_least = 0) { HIP_TRY_AS("hipMalloc", a.alloc(std::max(n, at_least))); return MI_OK; }
template <class T> static inline int dev_zeros(DevArray<T>& a, size_t n, size_t at_least = 0) { HIP_TRY_AS("hipMalloc + hipMemset", a.zeros(std::max(n, at_least))); return MI_OK; }
template <class T> static inline int dev_upload(DevArray<T>& a, const std::vector<T>& h, size_t at_least = 0) { HIP_TRY_AS("hipMalloc + hipMemcpy", a.upload(h, at_least)); return MI_OK; }
static inline int dev_alloc(MappedWord& w) { HIP_TRY_AS("hipHostMalloc (mapped)", w.alloc()); return MI_OK; }
static inline int dev_create(OwnedStream& s, unsigned flags = hipStreamDefault) { HIP_TRY_AS("hipStreamCreate", s.create(flags)); return MI_OK; }
static inline int dev_create(OwnedEvent& e, unsigned flags = hipEventDefault) { HIP_TRY_AS("hipEventCreate", e.create(flags)); return MI_OK; }

int need_device(); // capi_lib.hip

// the environment switch `name` is set to exactly `value`
static inline bool env_is(const char* name, const char* value)
{
    const char* e = getenv(name);
    return e && !strcmp(e, value);
}

// ---------------------------------------------------------------- measurement
// Mean time of one launch of `launch` (a callable returning MI_OK or an error code) on stream s: `warm` launches, then `timed`
// launches between two events.  Stops at the first launch that fails and returns its status; an event call that fails returns
// MI_ERR_HIP.  What a failed measurement means is the caller's business.
struct LaunchTimer {
    hipStream_t s;
    OwnedEvent e1, e0; // (destroyed e0 first)
    explicit LaunchTimer(hipStream_t st = nullptr) : s(st) {}
    int init()
    {
        int rc;
        (rc = dev_create(e0)) || (rc = dev_create(e1));
        return rc;
    }
    template <class F>
    int time(int warm, int timed, F&& launch, double* us)
    {
        int rc;
        for (int w = 0; w < warm; w++)
            if ((rc = launch())) return rc;
        HIP_TRY(hipEventRecord(e0, s));
        for (int w = 0; w < timed; w++)
            if ((rc = launch())) return rc;
        HIP_TRY(hipEventRecord(e1, s));
        HIP_TRY(hipEventSynchronize(e1));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        *us = ms * 1e3 / timed;
        return MI_OK;
    }
};

// the x / y pair a measurement launches on (x zeroed: timing does not depend on the values); freed on scope exit, x first, unless moved out.
// Declare it AFTER the LaunchTimer that times on it: the pair is then freed before the events go, the order the library has always
// released them in — where later allocations land moves launch times by several per cent (profiles/NOTES.md §4.12)
struct ScratchPair {
    DevArray<double> x, y;
    ~ScratchPair() { x = {}, y = {}; }
    int alloc(size_t nx, size_t ny)
    {
        HIP_TRY(x.alloc(nx));
        HIP_TRY(y.alloc(ny));
        HIP_TRY(hipMemset(x, 0, sizeof(double) * nx));
        return MI_OK;
    }
};

// the lower of two measurements; 0 = not measured
static inline double min_measured(double a, double b) { return a > 0 ? std::min(a, b) : b; }
// a measured and faster than b (strictly)
static inline bool better(double a, double b) { return a > 0 && (b <= 0 || a < b); }

// true while stream s is being captured into a HIP graph.  Entry points whose kernels take a per-call counter as an ARGUMENT (the
// one-launch powers step's epoch, the push step's step number) or that measure on first use must not do either under capture:
// a replayed graph would present the same counter again and every in-kernel wait would pass at once.
static inline bool stream_is_capturing(hipStream_t s)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return st != hipStreamCaptureStatusNone;
}

// ---------------------------------------------------------------- handles
// Every device array below is owned by the member that names it (dev_array.hpp); a table's arrays are declared in the order they are freed in.
struct BlockTable {
    int nnzb = 0;
    int nblk = 0;
    int row_align = 1;     // what the table was cut with (mi_csr_stream_info)
    DevArray<int2> d_blk;  // [nblk+1]
};

struct RingTable {
    RingConfig cfg{};
    int nblk = 0, wgs = 0, bpw = 0, bad_runs = 0;
    double ok_fraction = 0.0; // share of the nonzeros in ring-served runs
    DevArray<int> d_plan; // 8 ints per block, read as two int4
    DevArray<int> d_ok;
    DevArray<int> d_rng;      // {first block, end block} per run
    DevArray<int> d_run_halo; // per run: touches a ghost column (fused multi-GPU step)
    std::vector<int> h_run_halo;
    bool uniform = true;       // runs are consecutive ranges of bpw blocks (the kernel then computes them)
    bool lean = false;         // the plan allows the LEAN instantiation (spmv_ring.hpp)
    bool all_in_loop = false;  // every run is ring-served and holds no PLAIN block: every row is computed inside the counted loop
    std::vector<int> h_dep_ptr, h_dep_run; // one-launch powers step: per run the runs its columns name (ring_plan.hpp: build_run_deps); empty if not built
    DevArray<unsigned short> d_slots; // 16-bit column stream (ring slots), nnzb per block
    bool nt = false;                  // non-temporal loads of the values (chosen by measurement)
    bool skew = false;                // padded staging layout (many rows with a length that is a multiple of 8)
};

// plan of the multi-window ring kernel (mring_plan.hpp); valid iff d_plan != nullptr
struct MringTable {
    int nblk = 0, wgs = 0, nruns = 0, bpw = 0, bad_runs = 0, depth = 2;
    double ok_fraction = 0.0;
    long long restarts = 0;
    DevArray<int> d_plan;              // kMringRec ints per block, read as int4
    DevArray<int> d_first;             // kMringFirst ints per run: the first block's windows
    DevArray<int> d_ok;
    DevArray<int> d_rng;
    DevArray<unsigned short> d_slots;
    bool nt = false, skew = false;
};

// plan of the tile kernel (tile_plan.hpp); valid iff d_desc != nullptr
struct TileTable {
    int nblk = 0;
    DevArray<int> d_desc;              // 4 ints per block, read as int4
    DevArray<unsigned> d_ulist;        // distinct columns per block
    DevArray<unsigned short> d_slots;  // 16-bit column stream: position in the block's list
    double unique_per_nnz = 0.0;       // distinct columns per nonzero, averaged over the matrix
    bool nt = false;                   // non-temporal loads of the values
    bool skew = false;                 // padded staging layout (see RingTable::skew)
};

// the sliced copy of the sliced-stream kernel (spmv_sstream.hpp); valid iff dev.val != nullptr
struct SstreamCopy {
    bool mw = false; // the cut-ring form (spmv_sstream_mw.hpp): several column neighbourhoods per row (3-D mesh operators)
    SsDevice dev;                 // values, slot stream, workgroup records, windows, slice tables (value refills), ghost marks
    int nwg = 0, rounds = 0;
    int shift = 0;                // the rows are planned one down (an odd y offset: row pairs stay 16-byte aligned)
    long long steps = 0;
    double padding = 0.0;         // padded places per nonzero
    int max_slice_nnz = 0;        // longest CSR segment of a slice (picks the refill kernel's LDS buffer)
    bool nt = true;               // non-temporal value loads (measured at create)
    bool deep = true;             // twelve steps of prefetch instead of eight (measured at create)
    bool fusable = false;         // a combined piece's plan that spmv_sstream_fused can run (every ghost-reading workgroup's columns fit its first fill)
    bool asked = false;           // built because the environment or the caller asked for it: never released for losing a measurement
    std::vector<int> h_wg_halo;   // a combined piece of the fused multi-GPU step: per workgroup, it reads ghost columns (empty otherwise)
    std::vector<SsWg> h_wg;       // ... and its workgroup records (capi_part.hip writes the push links into them at connect time)
};
// ... and what its four forms measured at create, which outlives a copy released for losing (copy() = {} leaves it; mi_csr_sstream_info)
struct SstreamTable : SstreamCopy {
    double tune_us[4] = {0, 0, 0, 0}; // D = 8 nt, D = 8 temporal, D = 12 nt, D = 12 temporal
    SstreamCopy& copy() { return *this; }
};

// a handle that goes with another (the blocked copy, the relabelled twin): deleted with its owner, read like the plain pointer it replaces
template <class H, class Destroy = std::default_delete<H>>
struct OwnedHandle {
    std::unique_ptr<H, Destroy> own;
    operator H*() const { return own.get(); }
    H* operator->() const { return own.get(); }
    void reset(H* p = nullptr) { own.reset(p); }
};

// vectors a handle allocates one by one as higher powers are asked for (the host-pointer and the relabelled k-step); freed first to last
struct DevPowers {
    std::vector<DevArray<double>> own;
    std::vector<double*> ptr; // the same, as the kernels' argument
    int grow(int k, size_t n) // at least k vectors of n doubles
    {
        while ((int)own.size() < k) {
            DevArray<double> a;
            HIP_TRY(a.alloc(n));
            ptr.push_back(a);
            own.push_back(std::move(a));
        }
        return MI_OK;
    }
    void release()
    {
        for (auto& a : own) a = {};
        own.clear(), ptr.clear();
    }
};

// the one-launch matrix-powers step's tables (launch_spmk.hip): run flags, dependency lists, give-ups (host-visible, sticky)
struct SpmkTables {
    DevArray<unsigned> flags;
    DevArray<int> dep_ptr, dep_run;
    MappedWord giveups;
};

struct SpmmTilePlan {
    int rows = 0, umax = 0, ntiles = 0; // block rows per tile (at most); longest list; tiles
    double mean_list = 0.0;
    DevArray<int> d_ptr;
    DevArray<unsigned> d_nodes;
    DevArray<unsigned short> d_slots;
    DevArray<int> d_rows;               // [ntiles * rows]: block row per lane group, -1 - r for unused places
};

// x tile per workgroup (spmv_bcsr4_tile): lists of distinct block columns and 16-bit positions; built iff ptr != nullptr
struct Bcsr4TileLists {
    DevArray<int> ptr;
    DevArray<unsigned> nodes;
    DevArray<unsigned short> slots;
};

// the sliced copy (spmv_bcsr_sell.hpp): 16 block rows per slice, one contiguous stream per persistent wave; built iff val != nullptr
struct Bcsr4Sliced {
    DevArray<double> val;
    DevArray<unsigned> col;
    DevArray<int> sptr;
    DevArray<int> wrng;  // slice ranges of the waves: [sell_nwaves + 1] for ONE wave per SIMD (1024 waves) ...
    DevArray<int> wrng2; // ... and [sell_nwaves2 + 1] for two (2048)
};

struct mi_bcsr4_s {
    int device = 0;
    int nbrows = 0, nbcols = 0;
    long long nblocks = 0;
    DevArray<int> d_ptrow, d_indcol;
    DevArray<double> d_coef;
    DevArray<int> d_browmap;  // block-row map of a reordered matrix's blocked copy, else null
    Bcsr4TileLists tl;
    bool use_tile = false;    // the measured choice between the two kernels (MI355_BCSR_TILE=0|1 forces)
    double tune_us_plain = 0.0, tune_us_tile = 0.0;
    Bcsr4Sliced sell;
    int sell_nslices = 0, sell_nwaves = 0, sell_nwaves2 = 0;
    long long sell_nsteps = 0;
    int max_slice_vals = 0;   // values of the longest slice of 16 block rows (the refresh kernel's LDS buffer)
    int sell_form = -1;       // -1: not in use; else the variant the create-time measurement kept (kSellForms, capi_bcsr.hip)
    double tune_us_sell[4] = {0, 0, 0, 0};
    // x tiles of the multi-vector product (spmm_tile.hpp): lists per group of 128 block rows (st) and of 64 (st64: the eight-column
    // form with two quads per block row), built at the first product
    SpmmTilePlan st, st64;
    int st_state = 0;         // 0 not tried, 1 built, -1 not possible
    int spmm_choice[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; // per column count <= 8: 0 not measured, else 1 + the form that measured fastest
    double spmm_us[9][5] = {};                         // [s][form] microseconds per launch: 0 gather kernels, 1 tile (four lanes per block row),
                                                       // 2 / 3 tile with eight lanes per block row, temporal / non-temporal coefficient loads,
                                                       // 4 the sliced stream (spmm_bcsr4_sell)
    DevArray<double> d_x, d_y;
    DevPowers d_pow;
    // the order the handle has always been freed in
    ~mi_bcsr4_s() { d_ptrow = {}, d_indcol = {}, d_coef = {}, d_browmap = {}, tl = {}, sell = {}, st = {}, st64 = {}, d_x = {}, d_y = {}, d_pow.release(); }
};


struct mi_csr_s {
    int device = 0;
    int n = 0, ncols = 0;
    long long nnz = 0;
    DevArray<int> d_ptrow, d_indcol;
    DevArray<double> d_coef;
    DevArray<int> d_rowmap;
    bool mapped = false;  // created with a rowmap (device-only entry points, no powers)
    int y_offset = 0;     // a rowmap that is just "row r -> y[r + offset]" is applied as a pointer offset, not as a gather
    int ghost_lo = 0, ghost_hi = 0; // ghost_lo < ghost_hi: a partition's combined piece, columns outside [ghost_lo, ghost_hi) are ghosts
    std::vector<int> h_ptrow; // kept to (re)build row-block tables
    std::map<int, BlockTable> tables;
    RingTable ring;           // valid iff ring.d_plan != nullptr
    TileTable tile;           // valid iff tile.d_desc != nullptr
    SstreamTable ss;          // valid iff ss.dev.val != nullptr
    MringTable mring;         // valid iff mring.d_plan != nullptr
    int kernel = MI_KERNEL_AUTO;
    int auto_kernel = MI_KERNEL_STREAM;
    std::vector<double> place_us; // placement draws at create (capi_csr.hip): microseconds per launch, value array first ([0] = as first allocated) ...
    int place_draws_coef = 0;     // ... place_us[0 .. place_draws_coef) belong to the value array, the rest to the 16-bit column stream
    DevArray<double> kept_x, kept_y; // the scratch pair the placement draws were timed on, kept for mi_vec_alloc_placed (its first candidate)
    double tune_us[MI_KERNEL_SSTREAM + 1][2] = {}; // create-time measurement per kernel id, [temporal, non-temporal] loads (the blocked copy: [BCSR4][0]); 0 = not measured
    double tune_us_ring_aligned = 0.0, tune_us_ring_unaligned = 0.0; // large matrices: the two block shapes (0 = not compared)
    bool stream_nt = false; // non-temporal matrix loads in the stream kernel
    OwnedHandle<mi_bcsr4_s> blocked; // BCSR 4x4 copy (exact 4x4 node-block structure only), else null
    int n_out = 0; // length of the y a launch may write (n, or max rowmap + 1)
    // Locality reordering (reorder.hpp): when `inner` is set, this handle is a front for A' = P A P^T, a row-mapped
    // handle in the new numbering; products gather x into d_xp (new numbering) and inner writes y through its row
    // map straight into the caller's numbering.  The natural-order device arrays are released then.
    OwnedHandle<mi_csr_s> inner;
    DevArray<int> d_iperm;      // [n] caller's index of new row / column
    std::vector<int> h_iperm;   // the same on the host (mi_csr_perm)
    DevArray<int> d_src_start;  // [n] offset of new row r' in the caller's coef (values refresh)
    DevArray<double> d_xp;      // x in the new numbering: the buffer of the FIRST stream that multiplies with this handle ...
    hipStream_t xp_stream = nullptr;
    bool xp_claimed = false;
    std::map<hipStream_t, DevArray<double>> xp_more; // ... products enqueued on other streams get a gather buffer of their own (reorder_scratch)
    DevPowers d_pp;             // powers in the new numbering (mi_spmk_dev: one k-step at a time per handle)
    DevArray<double> d_vtmp;    // staging for mi_csr_update_values (host values)
    double spread_before = 0.0, spread_after = 0.0, us_natural = 0.0, us_reordered = 0.0;
    int reorder_block = 0;      // 0: no reordering attempted
    // scratch for the host-pointer entry points
    DevArray<double> d_x, d_y;
    DevPowers d_pow;
    // the one-launch matrix-powers step (spmk_ring.hpp, launch_spmk.hip): run flags, dependency lists, the launch counter the
    // flags count from, give-ups (host-visible, sticky), and per k the measured choice between one launch and k launches
    SpmkTables kstep;
    unsigned kstep_epoch = 0;
    int kstep_setup = 0;                 // 0 not tried, 1 ready, -1 not eligible
    int kstep_choice[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; // per k <= 8: 0 not measured, 1 one launch, -1 k launches
    double kstep_us[9][2] = {};          // measured microseconds per step: [k][0] k launches, [k][1] one launch
    void drop_tables() // the row-block tables, lowest nnzb first
    {
        for (auto& kv : tables) kv.second = {};
        tables.clear();
    }
    // the order the handle has always been freed in, written here and nowhere else
    ~mi_csr_s()
    {
        d_ptrow = {}, d_indcol = {}, d_coef = {}, d_rowmap = {}, d_x = {}, d_y = {}, kept_x = {}, kept_y = {}, d_pow.release();
        drop_tables();
        ring = {}, tile = {}, mring = {}, ss = {}, blocked.reset(), inner.reset(), d_iperm = {}, d_src_start = {}, d_xp = {};
        for (auto& kv : xp_more) kv.second = {};
        d_vtmp = {}, d_pp.release(), kstep = {};
    }
};

// ---- what a partition owns besides its pieces: four tables, each declared in the order it is freed in, each dropped by assigning a fresh one.
// The three deleters below are capi_part.hip's: they need RCCL's function table and the window registry.
struct RcclCommDestroy { void operator()(void* comm) const; };                  // ncclCommDestroy
struct IpcMappingClose { void operator()(void* base) const; };                  // hipIpcCloseMemHandle
struct WinRegistryErase { void operator()(std::string* key) const; };           // erases the key (under g_mu), deletes the string
using RcclComm = std::unique_ptr<void, RcclCommDestroy>;
using IpcMappings = std::vector<std::unique_ptr<void, IpcMappingClose>>;
using WinRegistryEntry = std::unique_ptr<std::string, WinRegistryErase>;        // the IPC handle bytes under which my window is registered

// native exchange (mi_part_comm_init)
struct PartRccl {
    RcclComm comm; // ncclComm_t
    OwnedStream comm_stream;
    OwnedEvent ev_pack, ev_comm;
    DevArray<double> d_sendbuf;
    unsigned step_no = 0;
    // Hand-offs between the two streams: HIP events by default.  Flag kernels (handoff_kernels.hpp) are ~8 us per
    // step cheaper in the one-GPU harness but have not run against real multi-GPU RCCL yet: opt in with
    // MI355_PART_HANDOFF=flags.
    bool flag_handoff = false;
};

// the all-gather form of the RCCL exchange (wide halos): every rank contributes the M-entry slice of ITS entries that anybody
// needs (the sorted union of its send lists, padded to the largest), one ncclAllGather, each ghost picked out of the N x M result.
// Set up iff d_ag_idx != nullptr.
struct PartAllGather {
    DevArray<int> d_ag_idx;      // [M] my union, padded with entry 0
    DevArray<int> d_ag_src;      // [n_halo] where ghost h lies in the gathered buffer
    DevArray<double> d_ag_send;  // [M]
    DevArray<double> d_ag_recv;  // [nranks * M]
    int ag_slice = 0;            // M
    bool ready() const { return d_ag_idx != nullptr; }
};

// peer-push exchange (push_exchange.hpp): my receive window, the peers' windows I write to
struct PushWindow {
    IpcMappings ipc_opened; // the peers' windows, mapped
    WinRegistryEntry win_entry;
    DevArray<char> win;            // [flags: nranks x 64 B][pad][data: 2 x n_halo doubles], uncached
    unsigned* win_flags = nullptr; // views of win
    double* win_data = nullptr;
    bool peer_on_my_device = false; // a neighbour's window lives on this rank's device: ranks share a card
};
struct PushTables { // what connecting builds
    DevArray<PushLink> d_links;
    DevArray<int2> d_push_work;    // stand-alone push kernel: {link, chunk} per workgroup
    DevArray<int> d_link_chunks;   // chunks per link
    DevArray<unsigned> d_tickets;  // per link: chunks out so far
    DevArray<int> d_nb;            // ranks whose flags I wait for
    int n_links = 0, n_push_work = 0, n_nb = 0;
};
struct PartPush : PushWindow, PushTables {
    unsigned push_step = 0;
    bool push_ready = false;
    PushTables& tables() { return *this; }
};

// the one-launch form of the push step: all local rows in one piece.  Three forms: the ring kernel's or the sliced stream's FUSED
// form (spmv_ring.hpp, spmv_sstream.hpp), and the staged step (spmv_bcsr4_ext.hpp: piece_all numbered [owned | halo], exchange
// workgroups in front of the grid, ghosts staged) on blocked (FE) or on scalar rows
struct PartOneLaunch {
    DevArray<int> d_run_link;        // per run of piece_all: first push link it serves, or -1
    DevArray<double> d_stage;        // [n_halo] cached copy of the window's current parity
    DevArray<unsigned> d_ready;      // exchange workgroups done (up by ext_wgs per step)
    DevArray<int2> d_ext_units;      // blocked rows, per workgroup behind the exchange: {first block row, mode}
    DevArray<unsigned> d_ext_order;  // scalar rows, per workgroup behind the exchange: its row block of piece_all's 1024-nonzero table, bit 31: it waits
    OwnedHandle<mi_csr_s> piece_all;
    const int* d_run_halo = nullptr; // per run (ring) / workgroup (sliced stream) of piece_all: it reads ghosts (owned by piece_all)
    int npush_runs = 0;
    bool fused = false;
    bool ghost_readers = true; // some run / workgroup of the fused launch waits for the neighbours (false: the pushers wait)
    bool fused_ext = false;    // the staged step ...
    bool ext_csr = false;      // ... on SCALAR rows (spmv_csr_fused_ext): d_ext_order instead of d_ext_units
    int ext_wgs = 0;
    int n_ext_units = 0;       // plain units first, then the waiting ones
    int n_ext_plain = 0;
    bool ext_split = false;    // two launches (exchange + plain units, then the waiting units): no workgroup but the exchange's waits in-kernel
    int ext_debug = 0;         // devtools only (mi_debug_part_ext_mode): parts of the exchange left out, for timing
};

struct mi_part_s {
    PartPlan plan;
    OwnedHandle<mi_csr_s> piece[2];
    DevArray<int> d_send_idx;
    bool finalized = false;
    int kernel = MI_KERNEL_AUTO;
    PartRccl rccl;
    std::vector<int> ag_union;   // local ids, ascending (mi_part_send_union)
    PartAllGather ag;
    bool ag_use = false;
    DevArray<unsigned> d_flags; // the RCCL step's hand-off flags: [0] "x ready" (set on the caller's stream), [1] "halo rows done" (set on the comm stream)
    MappedWord timeouts; // hand-off and push waits that gave up (read by the host at every entry point); allocated by whichever exchange comes up first
    PartPush push;
    PartOneLaunch one;
    // the order the handle has always been freed in
    ~mi_part_s() { piece[0].reset(), piece[1].reset(), d_send_idx = {}, rccl = {}, ag = {}, d_flags = {}, timeouts = {}, push = {}, one = {}; }
};

static inline size_t win_data_offset(int nranks) { return ((size_t)nranks * kWinFlagStride * sizeof(unsigned) + 255) / 256 * 256; }

// g_mu guards every process-wide table of the library (reduction workspaces, flush buffers, window registry)
extern std::mutex g_mu; // capi_lib.hip
int get_ws(hipStream_t s, double** out); // capi_blas1.hip: reduction workspace of (device, stream)

// host-pointer helper: upload vectors, run on the device copies, download
struct Scratch {
    std::vector<DevArray<double>> bufs;
    ~Scratch()
    {
        for (auto& a : bufs) a = {}; // first to last
    }
    int up(const double* h, size_t n, double** d)
    {
        *d = nullptr;
        DevArray<double> a;
        int rc = dev_alloc(a, n, 1);
        if (rc) return rc;
        *d = a;
        bufs.push_back(std::move(a));
        if (h && n) HIP_TRY(hipMemcpy(*d, h, sizeof(double) * n, hipMemcpyHostToDevice));
        return MI_OK;
    }
};

// capi_csr.hip
int csr_create_impl(int n, int ncols, const int* ptrow, const int* indcol, const double* coef, const int* rowmap, mi_csr_t* out,
                    int ghost_lo = 0, int ghost_hi = 0, bool defer_placement = false);
int resolve_kernel(const mi_csr_s* A);
int get_table(mi_csr_t A, int nnzb, BlockTable** out);
// launch_csr.hip
int launch_spmv(mi_csr_t A, const double* d_x, double* d_y, hipStream_t s, bool use_map = true, const RingComm* comm = nullptr,
                const RingDot* dot = nullptr);
bool ring_dot_eligible(const mi_csr_s* A); // the next launch_spmv(A) can carry a dot epilogue (one partial per ring workgroup)
// launch_csr.hip: the x gather buffer of a relabelled handle for products enqueued on stream s (one per stream, so that products of
// one handle on different streams do not share scratch; allocated on first use — not under stream capture)
int reorder_scratch(mi_csr_t A, hipStream_t s, double** buf);
// launch_ring.hip
void launch_ring_cfg(const mi_csr_s* A, const CsrView& V, const double* d_x, double* d_y, hipStream_t s, const RingComm* comm, const RingDot* dot);
// launch_spmk.hip: the k powers on an unmapped view of H (its row map, if any, is not applied): one launch where that is
// eligible and measured faster, else k chained launches
int spmk_unmapped(mi_csr_t H, int k, const double* d_x, double* const* d_y, hipStream_t s);
// capi_blas1.hip
int gather_perm(mi_csr_t A, const double* d_x, double* d_xp, hipStream_t s);
int ortho_update_from_parts(int n, int nparts, const double* parts, double alpha, const double* d_b, const double* d_x1, double* d_x3, double* d_beta_out,
                            hipStream_t s);
int scatter_perm(mi_csr_t A, const double* d_src, double* d_dst, hipStream_t s);
int residual_norm_dev(int n, const double* d_b, const double* d_w, double* d_r, double* d_out, hipStream_t s); // r = b - w, *d_out = ||r||_2
// launch_spmm_tile.hip: the multi-vector product's tile form (spmm_tile.hpp), up to four columns
constexpr size_t kLdsBytesPerCU = 160 * 1024;
static inline size_t spmm_tile_lds(const SpmmTilePlan* T, int s) { return T ? (size_t)T->umax * (4 * s + 2) * sizeof(double) : (size_t)-1; }
hipError_t spmm_tile_launch(const mi_bcsr4_s* A, const SpmmTilePlan* Pl, const Bcsr4View& V, int s, int arith, const double* X, long long ldx,
                            double* Y, long long ldy, hipStream_t st);
hipError_t spmm_otile_launch(const mi_bcsr4_s* A, const SpmmTilePlan* Pl, const Bcsr4View& V, int s, int arith, bool nt, const double* X, long long ldx,
                             double* Y, long long ldy, hipStream_t st);
// capi_part.hip: pieces of the peer-push set-up that capi_dist.hip (ranks of one process on different devices) uses directly
int part_push_window(mi_part_s* P);
void part_push_layout(const mi_part_s* P, long long* layout /* [2*nranks + 1] */);
int part_push_connect_bases(mi_part_s* P, void* const* bases /* [nranks] */, const long long* layouts,
                            IpcMappings opened = {}, bool peer_on_my_device = false);
// the staged one-launch step of a blocked rank (spmv_bcsr4_ext.hpp); trace: devtools only (3 stamps per workgroup of the grid)
int part_ext_launch(mi_part_s* P, const double* d_x_ext, double* d_y_local, unsigned step, unsigned spin_max, hipStream_t s, unsigned long long* trace, int* grid_out);
// capi_csr.hip: the sliced-stream kernel of a handle (spmv_sstream.hpp); d_y: where the handle's row 0 goes (unmapped) or the mapped vector's base;
// comm: the fused multi-GPU step (the handle is a partition's combined piece with ghost marks)
int launch_sstream(mi_csr_t A, const double* d_x, double* d_y, const int* rowmap, hipStream_t s, const RingComm* comm = nullptr);
// the sliced-stream kernel can write this y (row pairs as 16 bytes; a mapped handle stores row by row)
static inline bool sstream_y_ok(const mi_csr_s* A, const double* yy, const int* map) { return map || A->ss.mw || (((uintptr_t)(yy - A->ss.shift)) & 15) == 0; } // (the cut-ring form stores row by row)
// capi_bcsr.hip
// the blocked copy's values were rewritten on stream s (by whoever holds d_coef): the sliced copy follows at once, on the same stream
int bcsr4_values_changed(mi_bcsr4_s* A, hipStream_t s);
// give the sliced copy up (a handle whose products never run the sliced kernels: the partition's combined piece of a blocked one-launch step)
void bcsr4_drop_sliced(mi_bcsr4_s* A);
// a CSR handle's blocked copy (blocks + sliced values) from its CSR values d_src, which also go to d_csr_out when that is given: one pass
int bcsr4_refresh_from_csr(mi_bcsr4_s* A, const int* d_csr_ptrow, const double* d_src, double* d_csr_out, hipStream_t s);
int launch_bcsr4(mi_bcsr4_t A, const double* d_x, double* d_y, mi_stream_t s, bool use_map);
// capi_ilu.hip: HOW a block ILU factor is applied — exactly, or by sf forward and sb backward Jacobi sweeps; over the factor's doubles
// or its single-precision copy.  The four solve families mi_bilu4{,sw,sp,spx}_solve* and GMRES's preconditioner are each one value.
struct Bilu4Apply {
    bool sweeps, f32;
    int sf, sb; // sweeps only
};
int bilu4_apply_prepare(mi_bilu4_t F, const Bilu4Apply& how); // the family's public prepare (nothing for exact f64)
int bilu4_apply_dev(mi_bilu4_t F, const Bilu4Apply& how, const double* d_b, double* d_x, hipStream_t s); // the family's *_solve_dev
