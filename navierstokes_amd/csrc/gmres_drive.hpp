// gmres_drive.hpp — THE host loop of mi_gmres_solve_dev and mi_gmres_plan_solve (capi_gmres.hip; include/mi355_spmv.h, HOST LOOP
// and WASTE).  Host only, no HIP include: tools/gmres_drive_check.cpp runs it against a scripted device under the
// host sanitizers.
#pragma once
#include "gmres_record.hpp"
#include <algorithm>

namespace mi355 {

// The two batch rules: the steps [k_enq, returned) are what the next batch enqueues.  room: min(m - k_enq, maxiter - its - k_enq),
// not below 0.
// mi_gmres_solve_dev: check_every steps clipped to the room; a cycle's first batch is one step short: a solve that ends at the
// cycle's start, which only this batch's record tells, has then wasted 2 check_every - 1 steps at most, like one that freezes
// inside a batch.
inline int gmres_eager_batch(int k_enq, int room, bool first_batch, int check_every)
{
    return k_enq + std::min(first_batch ? check_every - 1 : check_every, room);
}
// mi_gmres_plan_solve: a cycle's first batch has no step (the record of its start); then one whole segment graph, which maxiter does
// not clip (the device stops counting there).  *graph: which segment, -1 for none.  Called with room > 0, so k_enq is a segment's start.
inline int gmres_plan_batch(int k_enq, int m, bool first_batch, int segment, int* graph)
{
    *graph = first_batch ? -1 : k_enq / segment;
    return first_batch ? k_enq : std::min(m, (*graph + 1) * segment);
}

// what a solve leaves behind on the host
struct GmresOutcome {
    int its = 0, reason = 0;
    int refused = 0;                // MI_BASIS_F32: claims of the recurrence that the next cycle's true residual did not confirm
    int readbacks = 0, wasted = 0;  // slots waited for; steps enqueued behind the last counted one, summed over the cycles
    int last_k = 0;                 // the last cycle: its counted steps and its ||r0||
    double last_beta = 0.0;
};

// The solve.  Steps are enqueued in batches; behind each batch the record and the cycle's history entries go to one of two slots,
// and the host looks at a batch's slot only after the NEXT batch is enqueued, so the device never waits for the host inside a cycle;
// a cycle's end is the one point where the host waits with nothing enqueued behind.  B supplies what differs between the solves
// (every member returns 0 or an error, which ends the solve at once):
//   start(first)                      the start of a cycle (first: of the solve)
//   batch(k_enq, room, first_batch)   enqueue the next batch behind the k_enq steps of the cycle so far; k_enq becomes the new count
//   readback(entries, &slot)          the record and `entries` history values into the next slot, behind what is enqueued
//   wait(slot, &rec, &entries)        wait for that slot; its record, and where its history values lie until the next readback
//   end(k)                            the end of a cycle with k > 0 counted steps: y, then x += M^-1 (V y)
// history: maxiter + 1 doubles or null.  f32: the float basis, whose recurrence is exact only to float rounding of the basis, so a
// step's reason 1 (k > 0) is a CLAIM: the cycle's end has run, and the next cycle's start — the true residual — confirms it
// (reason 1 with k = 0) or not.
template <class Backend>
int gmres_drive(Backend& B, int m, int maxiter, bool f32, double* history, GmresOutcome& out)
{
    out.its = out.reason = out.refused = out.readbacks = out.wasted = out.last_k = 0;
    bool claimed = false; // the last cycle froze with a claim and this cycle's start has to confirm it
    for (bool first = true;; first = false) {
        int rc;
        if ((rc = B.start(first))) return rc;
        GmresRecord rec{};
        const double* entries = nullptr;
        int k_enq = 0, pending = -1;
        for (;;) {
            int cur = -1;
            const int room = std::max(0, std::min(m - k_enq, maxiter - out.its - k_enq));
            // (room == 0 with nothing pending: the cycle starts at maxiter, the record alone)
            if ((room > 0 || pending < 0) && ((rc = B.batch(k_enq, room, pending < 0)) || (rc = B.readback(k_enq, &cur)))) return rc;
            if (pending >= 0) {
                if ((rc = B.wait(pending, &rec, &entries))) return rc;
                out.readbacks++;
                if (rec.reason != 0 || cur < 0) break; // frozen (what is enqueued behind it is wasted), or the cycle's last batch
            }
            pending = cur;
        }
        if (history) { // (the last slot read holds the entries of all rec.k counted steps)
            if (first) history[0] = rec.rel0;
            for (int j = 0; j < rec.k; j++) history[out.its + 1 + j] = entries[j];
        }
        out.wasted += k_enq - rec.k;
        out.its = rec.its;
        out.last_k = rec.k, out.last_beta = rec.beta;
        if (rec.k > 0 && (rc = B.end(rec.k))) return rc; // (with k == 0 the end would change nothing)
        const bool done = gmres_decode(rec, &out.reason);
        if (claimed && !(rec.reason == 1 && rec.k == 0)) out.refused++;
        claimed = f32 && rec.reason == 1 && rec.k > 0;
        if (claimed) continue;
        if (done) break;
        if (out.its >= maxiter) {
            out.reason = 2;
            break;
        }
    }
    return 0;
}

} // namespace mi355
