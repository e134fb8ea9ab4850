#!/usr/bin/env python3
"""Restarted GMRES(30) to rtol = 1e-8 on the FE matrix: mpk.GMRES (the Python loop: one read-back of the Hessenberg column per
iteration) against mpk.gmres_solver (mi_gmres_*: a whole cycle enqueued on the device) at check_every = 1, 5 and restart, with
the SAME matrix and factor handles, in one process.  Prints one JSON line per preconditioner and appends it to
profiles/gmres_bench.jsonl.

    python3 tools/bench_gmres.py [--cells 68] [--fill 0] [--sweeps 3] [--precision f64|f32|both] [--basis f64|f32|both] [--runs 5] [--no-append]
                                 [--graph SEG[,SEG...]] [--order natural,colour] [--exact-precision f64|f32|both]

--exact-precision (default f64): which values the exact-solve rows stream — the double factor ("exact"), its single-precision
copy ("exact_f32": mpk.bilu4.exact("f32"), MI_GMRES_PC_EXACT_F32), or both on the SAME factor handle in the same process; the
records carry "exact_precision".

--order natural,colour (default natural): the ordering of the block rows behind the factor handle (mpk.bilu4(order=)); one factor
handle per ordering on the same matrix handle in one process, the records of each carry "order".

--basis f64 (the default) is the comparison above.  --basis f32 or both compares the solver handles instead: one gmres_solver per
basis asked for (basis="f64": the yardstick, the code path of the default; basis="f32": the single-precision Krylov basis), both at
check_every = 1 on the same matrix and factor handles, alternating inside every run; the records also carry basis_bytes and the
refused claims of the last solve (refused_last).

--graph 1,5,30 adds the PLANNED solve (gmres_solver.plan: graphs captured once and replayed, SEG steps per graph) as further solvers
gmres_plan_segSEG on every solver handle of the run, inside the same alternating runs; their records carry the graphs of the plan
and replays_last, readbacks_last and wasted_steps_last of the last solve.  The plans are captured before the warm-up.

Preconditioners per process: the sweeps (--sweeps per triangle) in each precision asked for, and the exact solve.  For each one a
record (tool = "bench_gmres") with, per solver: iterations, wall seconds (median of --runs runs; the solvers ALTERNATE inside every
run, after one warm-up each), the spread of the runs (max - min), microseconds per iteration, the true residual
||b - A x|| / ||b||, and for gmres_solver readbacks_last and wasted_steps_last.  The yardstick is mpk.GMRES in the same process."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RESTART, RTOL = 30, 1e-8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=68)
    ap.add_argument("--fill", type=int, default=0)
    ap.add_argument("--sweeps", type=int, default=3)
    ap.add_argument("--precision", choices=("f64", "f32", "both"), default="f64")
    ap.add_argument("--basis", choices=("f64", "f32", "both"), default="f64")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--maxiter", type=int, default=300)
    ap.add_argument("--no-append", action="store_true")
    ap.add_argument("--graph", default="", help="segments of the planned solve, e.g. 1,5,30")
    ap.add_argument("--exact-precision", choices=("f64", "f32", "both"), default="f64", help="the values the exact-solve rows stream")
    ap.add_argument("--order", default="natural", help="comma-separated orderings of the block rows: natural, colour")
    a = ap.parse_args()
    import torch
    from navierstokes_amd import mpk, synth

    bp, bc, bv = synth.csr_to_bcsr4(*synth.fe_matrix(a.cells))
    nb = len(bp) - 1
    n = 4 * nb
    A = mpk.bcsr4x4_matrix(nb, bp, bc, bv)
    orders = [o for o in a.order.split(",") if o]
    assert orders and all(o in mpk.BILU_ORDERS for o in orders), "--order: natural, colour"
    factors = {o: mpk.bilu4(A, fill=a.fill, order=o) for o in orders}
    b = synth.x_sin(0, n) + 1.0
    db = torch.from_numpy(b).cuda()
    dx, dy = torch.zeros_like(db), torch.zeros_like(db)
    bnorm = float(np.linalg.norm(b))
    preconds = []
    for o, F in factors.items():
        preconds += [(o, f"sweeps{a.sweeps}_{p}", F.sweeps(a.sweeps, precision=p)) for p in (("f64", "f32") if a.precision == "both" else (a.precision,))]
        preconds += [(o, "exact" if p == "f64" else "exact_f32", F.exact(p)) for p in (("f64", "f32") if a.exact_precision == "both" else (a.exact_precision,))]
    for order, label, M in preconds:
        if a.basis == "f64":
            S = mpk.gmres_solver(A, M, RESTART)
            handles = [S]
            solvers = [("mpk.GMRES", None)] + [(f"gmres_solver_ce{ce}", (S, ce)) for ce in (1, 5, RESTART)]
        else:
            handles = [mpk.gmres_solver(A, M, RESTART, basis=k) for k in (("f64", "f32") if a.basis == "both" else (a.basis,))]
            solvers = [(f"gmres_solver_{h.basis}_ce1", (h, 1)) for h in handles]
        plans = []
        for seg in (int(t) for t in a.graph.split(",") if t):
            for h in handles:
                plans.append(h.plan(db, dx, rtol=RTOL, maxiter=a.maxiter, segment=seg))
                solvers.append((f"gmres_plan_seg{seg}" + ("" if a.basis == "f64" else f"_{h.basis}"), (h, plans[-1])))

        def run(ce):
            dx.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if ce is None:
                its, hist = mpk.GMRES(A, db, dx, M=M, restart=RESTART, rtol=RTOL, maxiter=a.maxiter)
            elif isinstance(ce[1], mpk.gmres_plan):
                its, hist, _ = ce[1].solve()
            else:
                its, hist, _ = ce[0].solve(db, dx, rtol=RTOL, maxiter=a.maxiter, check_every=ce[1])
            torch.cuda.synchronize()
            sec = time.perf_counter() - t0
            mpk.SpMV_BCSR(dy, dx, A)
            true = float(np.linalg.norm(b - dy.cpu().numpy()) / bnorm)
            return its, sec, true, float(hist[-1])

        for _, ce in solvers:  # one warm-up each
            run(ce)
        secs = {name: [] for name, _ in solvers}
        last = {}
        for _ in range(a.runs):  # the solvers alternate inside every run
            for name, ce in solvers:
                its, sec, true, rec = run(ce)
                secs[name].append(sec)
                last[name] = dict(iterations=its, true_residual=true, recurrence_residual=rec)
                if ce is not None and isinstance(ce[1], mpk.gmres_plan):
                    last[name].update(ce[1].info())
                    if a.basis != "f64":
                        last[name].update(ce[0].basis_info())
                elif ce is not None:
                    info = ce[0].info()
                    last[name].update(readbacks_last=info["readbacks_last"], wasted_steps_last=info["wasted_steps_last"], launches_last=info["launches_last"])
                    if a.basis != "f64":
                        last[name].update(ce[0].basis_info(), device_bytes=info["device_bytes"])
        out = dict(tool="bench_gmres", cells=a.cells, rows=n, fill=a.fill, order=order, precond=label, exact_precision=a.exact_precision, restart=RESTART, rtol=RTOL, runs=a.runs,
                   default_check_every=mpk.GMRES_CHECK_EVERY, solvers={})
        for name, _ in solvers:
            med = statistics.median(secs[name])
            out["solvers"][name] = dict(last[name], seconds=round(med, 6), spread_seconds=round(max(secs[name]) - min(secs[name]), 6),
                                        us_per_iteration=round(med * 1e6 / max(last[name]["iterations"], 1), 2),
                                        spread_us_per_iteration=round((max(secs[name]) - min(secs[name])) * 1e6 / max(last[name]["iterations"], 1), 2))
        line = json.dumps(out)
        print(line, flush=True)
        if not a.no_append:
            with open(os.path.join(ROOT, "profiles", "gmres_bench.jsonl"), "a") as f:
                f.write(line + "\n")
        for h in plans + handles:
            h.close()
    for F in factors.values():
        F.close()
    A.close()


if __name__ == "__main__":
    main()
