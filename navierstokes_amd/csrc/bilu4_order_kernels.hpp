// bilu4_order_kernels.hpp — the two launches at the boundary of a solve on an ORDERED block ILU handle (bilu4_order.hpp): the
// caller's right-hand side gathered into the factor's numbering on the way in, the solution scattered back on the way out.
//   in:   b_int[4 perm[i] + q] = b[4 i + q]
//   out:  x[4 i + q] = x_int[4 perm[i] + q]
// perm[i] = the factor's number of the caller's block row i.  The internal vectors are the handle's own (16-byte aligned); the
// caller's need 8-byte alignment only, hence the two forms: AL moves a block as two 16-byte halves, one lane each; the scalar
// form one entry per lane.  Plain copies: no arithmetic, nothing to round.
#pragma once
#include "spmv_kernels.hpp"

namespace mi355 {

// lanes per block row of the two forms
template <bool AL>
constexpr int kBiluOrderLanes = AL ? 2 : 4;

// IN: from = b, to = b_int; else from = x_int, to = x.  The two never overlap (one is the handle's own vector).
template <bool IN, bool AL>
__global__ __launch_bounds__(kWG) void bilu4_order_move(const int* __restrict__ perm, int nb, const double* __restrict__ from, double* __restrict__ to)
{
    constexpr int L = kBiluOrderLanes<AL>;
    const long long g = (long long)blockIdx.x * kWG + threadIdx.x;
    const long long i = g / L;
    if (i >= nb) return;
    const int part = (int)(g % L);
    const size_t u = 4 * (size_t)i, n = 4 * (size_t)perm[i];
    const size_t r = IN ? u : n, w = IN ? n : u;
    if (AL) reinterpret_cast<double2*>(to + w)[part] = reinterpret_cast<const double2*>(from + r)[part];
    else to[w + part] = from[r + part];
}

} // namespace mi355
