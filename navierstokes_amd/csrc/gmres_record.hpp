// gmres_record.hpp — the 64-byte record of a GMRES solve that the device writes (gmres_kernels.hpp) and the host reads back
// (gmres_drive.hpp, capi_gmres.hip).  Plain C++: no HIP include.
#pragma once

namespace mi355 {

// the first 64 bytes of a solve's small state in device memory (gmres_kernels.hpp, GmresSmall), written by gmres_cycle_begin and
// gmres_hess_step; the history entries of the cycle's counted steps lie right behind it, and a read-back copies both
struct GmresRecord {
    int its;      // iterations counted so far in this solve
    int k;        // counted steps of the current cycle
    int reason;   // 0 while running; 1, 2, 3, 4 as mi_gmres_solve_dev reports them; kGmresMetAtStart: rtol met at a cycle's start
    int pad;
    double last;  // the last history value written
    double beta;  // ||r0|| of the current cycle
    double rel0;  // beta / bnorm
    double bnorm; // ||b||, or 1 where that is 0
    double spare[2];
};
static_assert(sizeof(GmresRecord) == 64, "the record is 64 bytes");
constexpr int kGmresMetAtStart = 5;
constexpr int kGmresRecDoubles = 8;

// the record as the ABI reports it: *reason in 0..4; returns whether the record holds a reason (done)
inline bool gmres_decode(const GmresRecord& rec, int* reason)
{
    *reason = rec.reason == kGmresMetAtStart ? 0 : rec.reason;
    return rec.reason != 0;
}

} // namespace mi355
