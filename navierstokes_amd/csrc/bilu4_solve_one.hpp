// bilu4_solve_one.hpp — the ONE-LAUNCH form of the block ILU solve (MatSolve_SeqBAIJ_4, src/kernels/baij4_solve.c:4-93): persistent
// workgroups run the forward and then the backward sweep; the unit of work is a CHUNK (bilu4_plan.hpp: 64 positions of a wide level,
// or a whole folded run of narrow levels) and one flag per chunk takes the place of a kernel boundary.  Chunk c belongs to workgroup
// c mod G; a workgroup takes its chunks in ascending order.
//
// Arithmetic: bilu4_row_value (bilu4_solve.hpp), untouched — every row is the same sequence of roundings as in the level-by-level
// form, bit for bit.
//
// Hand-off (the "write-through payload, drained, then flag" form spmk_ring.hpp uses, with ONE difference, below):
//   * the rows of a chunk store their result into x write-through (agent-scope relaxed atomic stores), every storing wave drains
//     its stores (`s_waitcnt vmcnt(0)`), the workgroup meets at a barrier and one lane stores the solve's epoch into the chunk's flag
//     (one 64-byte line per flag);
//   * a consumer polls the flags of its dependencies with one lane per dependency (agent-scope loads, s_sleep back-off, bounded),
//     then wave 0 executes an agent-scope ACQUIRE and waits for it, and the workgroup meets at a barrier before the first load of x.
// The acquire is what spmk_ring.hpp does without, and it cannot be dropped here: x is in block-row order, 32 bytes per block row,
// so a 128-byte line holds rows of different levels.  A workgroup that has read a published row has that line in its CU's L1 (and
// its XCD's L2); a neighbour in the line that is published later would be served stale from there.  spmk_ring never touches a line
// before its publication; this kernel does, all the time.  The loads of x behind the acquire stay bilu4_load4's plain 16-byte loads.
// Inside a folded chunk the levels are ordered as in bilu4_folded: __threadfence_block() plus a workgroup barrier (same CU).
//
// Between the sweeps x carries t, and the backward sweep overwrites t_i with x_i.  On a pattern that is not symmetric a forward row
// k > i may still have to read t_i (L(k, i) without U(i, k)), so every workgroup adds one to a counter after its last forward chunk
// and waits until the counter has reached G x epoch before its first backward chunk: one grid-wide meeting per solve, which also
// covers "a backward row reads its own t".
//
// Residency: every wait needs all G workgroups resident at once (a waiting workgroup keeps its CU slot); the host launches at most
// (occupancy query x CUs) workgroups.  Every wait is bounded; a wait that gives up counts in a host-mapped word, the workgroup
// leaves the kernel, and the other waiters see the word at their next check and leave too.  The host then fails the handle's next
// call (capi_ilu.hip).
//
// Epoch: the flags are never cleared; a solve publishes its own epoch, a kernel ARGUMENT that the host advances with every solve.
// Hence ONE solve at a time per handle, on ONE stream, and never under stream capture (a replayed graph would present the same
// epoch again: the host records the level-by-level form instead).
#pragma once
#include "bilu4_solve.hpp"

namespace mi355 {

constexpr int kBiluOneFlagStride = 16; // unsigneds: one 64-byte line per chunk

struct Bilu4OneTab {
    const int* chunk_pos; // [nchunks + 1]
    const int* chunk_lev; // [nchunks + 1]
    const int* dep_ptr;   // [nchunks + 1]
    const int* dep;
    unsigned* flags;      // [nchunks * kBiluOneFlagStride]
    int nchunks;
};

struct Bilu4OneArgs {
    Bilu4OneTab fwd, bwd;
    unsigned epoch;     // of this solve, >= 1 (flags and counter start at zero)
    unsigned* counter;  // workgroups that have finished their forward chunks, over all solves: G per epoch
    unsigned* giveups;  // host-mapped, sticky
    unsigned spin_max;
};

// Wait until *p has reached `want` (counters that wrap: compared by difference).  false: gave up — this wait ran out of polls (and
// counted itself in *giveups), or it saw at one of its checks that another wait had.
__device__ __forceinline__ bool bilu4one_wait(const unsigned* p, unsigned want, unsigned* giveups, unsigned spin_max)
{
    unsigned spins = 0;
    while ((int)(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - want) < 0) {
        if (spins < 256) __builtin_amdgcn_s_sleep(1);
        else __builtin_amdgcn_s_sleep(64);
        ++spins;
        if ((spins & 4095u) == 0 && __hip_atomic_load(giveups, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0) return false;
        if (spins > spin_max) {
            __hip_atomic_fetch_add(giveups, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            return false;
        }
    }
    return true;
}

// Behind the polls of a wait: wave 0 (whose lanes have polled, or which has passed the barrier behind the other waves' polls)
// invalidates this CU's L1 and waits for that; the workgroup's barrier then holds every wave's loads of x behind it.
// true: some wait of the workgroup gave up (uniform).
__device__ __forceinline__ bool bilu4one_acquire(bool ok)
{
    if (threadIdx.x < 64) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    return __syncthreads_or(!ok) != 0;
}

__device__ __forceinline__ void bilu4one_store(double* p, double v)
{
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one sweep's chunks of this workgroup; false (uniform): a wait gave up
template <bool BWD, bool AL>
__device__ __forceinline__ bool bilu4one_sweep(const Bilu4SweepView& V, const Bilu4OneTab& T, const Bilu4OneArgs& A, const double* src, double* x)
{
    const int tid = threadIdx.x, slot = tid >> 2, q = tid & 3;
    for (int c = blockIdx.x; c < T.nchunks; c += gridDim.x) {
        const int d0 = T.dep_ptr[c], nd = T.dep_ptr[c + 1] - d0; // <= kWG (the plan refuses more)
        if (nd > 0) {
            bool ok = true;
            if (tid < nd) ok = bilu4one_wait(T.flags + (size_t)T.dep[d0 + tid] * kBiluOneFlagStride, A.epoch, A.giveups, A.spin_max);
            if (nd > 64 && __syncthreads_or(!ok)) return false; // wave 0 must not invalidate before the other waves' flags have matched
            if (bilu4one_acquire(ok)) return false;
        }
        const int p0 = T.chunk_pos[c], p1 = T.chunk_pos[c + 1];
        const int l0 = T.chunk_lev[c], ln = T.chunk_lev[c + 1];
        const int l1 = ln == l0 ? l0 + 1 : ln; // a chunk of a wide level that the next chunk continues
        for (int l = l0; l < l1; l++) {
            const int pos = max(V.lev_ptr[l], p0) + slot;
            if (pos < min(V.lev_ptr[l + 1], p1)) {
                const int row = V.perm[pos];
                bilu4one_store(x + 4 * (size_t)row + q, bilu4_row_value<BWD, AL>(V, pos, row, q, src, x));
            }
            if (l + 1 < l1) { // the next level of a folded chunk reads these rows: same CU, as bilu4_folded
                __threadfence_block();
                __syncthreads();
            }
        }
        // publish: every storing wave's stores have left, then the flag
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) __hip_atomic_store(T.flags + (size_t)c * kBiluOneFlagStride, A.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return true;
}

template <bool AL>
__global__ __launch_bounds__(kWG) void bilu4_solve_one(Bilu4SweepView VF, Bilu4SweepView VB, Bilu4OneArgs A, const double* b, double* x)
{
    if (!bilu4one_sweep<false, AL>(VF, A.fwd, A, b, x)) return;
    // the meeting between the sweeps: this workgroup's forward stores were drained before its last flag store (tid 0 stored it)
    bool ok = true;
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(A.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = bilu4one_wait(A.counter, A.epoch * gridDim.x, A.giveups, A.spin_max);
    }
    if (bilu4one_acquire(ok)) return;
    (void)bilu4one_sweep<true, AL>(VB, A.bwd, A, x, x);
}

} // namespace mi355
