// launch_ring_impl.hpp — how one ring configuration <T, NNZB, RING, D> fans out into the kernel's instantiations (row map,
// non-temporal values, skewed staging, fused multi-GPU step, LEAN, dot epilogue).  Included by launch_ring_*.hip, one configuration
// group each: the 96 instantiations are most of the library's device-code compile time and build in parallel this way.
#pragma once
#include "capi_internal.hpp"

template <int T, int NNZB, int RING, int D>
static void launch_ring(const mi_csr_s* A, const CsrView& V, const double* d_x, double* d_y, hipStream_t s, const RingComm* comm, const RingDot* dot)
{
    static_assert(NNZB <= kRingPadNnz && 2 * T + 1 <= kRingPadRows, "device arrays are padded for the kernel's unclamped loads");
    const RingTable& R = A->ring;
    const int4* plan = reinterpret_cast<const int4*>(R.d_plan.get());
    const int2* rng = reinterpret_cast<const int2*>(R.d_rng.get());
    const int bpw = R.uniform ? R.bpw : 0;
    pick([&](auto MAPPED, auto NT, auto SKEW, auto LN) {
        // the LEAN instantiation exists for the configuration that runs in practice (4: 256 threads) at depths 2 and 4
        constexpr bool LEAN = LN() && T == 256 && D != 3;
        if constexpr (LEAN && !MAPPED()) {
            if (dot && !comm) { // the dot epilogue (spmv_ring.hpp: RingDot); the caller checked ring_dot_eligible()
                hipLaunchKernelGGL((spmv_csr_ring<T, NNZB, RING, D, kRingMaxB, false, NT(), SKEW(), false, true, true>), dim3(R.wgs), dim3(T), 0, s, V, plan, R.d_ok,
                                   R.d_slots, d_x, d_y, rng, bpw, RingComm{}, *dot);
                return;
            }
        }
        if (!MAPPED() && comm) // the fused multi-GPU step: push workgroups in front of the grid (spmv_ring.hpp)
            hipLaunchKernelGGL((spmv_csr_ring<T, NNZB, RING, D, kRingMaxB, MAPPED(), NT(), SKEW(), true, LEAN>), dim3(R.wgs + comm->push_wgs), dim3(T), 0, s, V, plan,
                               R.d_ok, R.d_slots, d_x, d_y, rng, bpw, *comm);
        else
            hipLaunchKernelGGL((spmv_csr_ring<T, NNZB, RING, D, kRingMaxB, MAPPED(), NT(), SKEW(), false, LEAN>), dim3(R.wgs), dim3(T), 0, s, V, plan, R.d_ok, R.d_slots,
                               d_x, d_y, rng, bpw, RingComm{});
    }, V.rowmap != nullptr, R.nt, R.skew, R.lean);
}
