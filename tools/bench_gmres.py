#!/usr/bin/env python3
"""Restarted GMRES(30) to rtol = 1e-8 on the FE matrix: mpk.GMRES (the Python loop: one read-back of the Hessenberg column per
iteration) against mpk.gmres_solver (mi_gmres_*: a whole cycle enqueued on the device) at check_every = 1, 5 and restart, with
the SAME matrix and factor handles, in one process.  Prints one JSON line per preconditioner and appends it to
profiles/gmres_bench.jsonl.

    python3 tools/bench_gmres.py [--cells 68] [--fill 0] [--sweeps 3] [--precision f64|f32|both] [--basis f64|f32|both] [--runs 5] [--no-append]
                                 [--graph SEG[,SEG...]] [--order natural,colour] [--exact-precision f64|f32|both]
    python3 tools/bench_gmres.py --precond dilu [--cells 68] [--order colour,natural] [--sweeps 3] [--runs 5] [--no-append] [--refactor]

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

--precond dilu: instead of the comparison above, the block DILU preconditioner applied with Eisenstat's trick (mpk.dilu4, mi_dilu4_*)
against block ILU(0) on the SAME matrix handle in one process.  One record (tool = "bench_gmres_dilu") with
  apply      microseconds per dilu4.apply_hat (200 applications between two events after 20 warm-ups, per ordering in --order) against
             the product plus the exact ILU(0) solve in colour order measured the same way, the bytes each streams (the byte model:
             blocks of 128 + 4 bytes, Einv twice and K once per block row, the vectors) and the handles' device bytes;
  solves     GMRES(30) to rtol 1e-8: DILU per ordering (mpk.dilu4.gmres's composition on ONE solver handle), exact ILU(0) in colour
             and natural order, and --sweeps Jacobi sweeps per triangle on the natural-order factor: iterations, seconds (median of
             --runs, the solvers alternating inside every run), microseconds per iteration and the TRUE residual ||b - A x|| / ||b||.
             THE TWO TOLERANCES ARE IN DIFFERENT NORMS: DILU's rtol is on ||(E + L)^-1 r|| / ||b^||, ILU's on the residual of the
             right-preconditioned system, which is the true one; compare the solves by true_residual.

--precond dilu --refactor adds to that record, per ordering and on the handles it already builds,
  refactor   mi_dilu4dev_refactor (mpk.dilu4.refactor_dev: events around 20 refactors after 3 warm-ups, values on the device) against
             mi_dilu4_refactor, the host path (median wall seconds of 3, values on the host: pivots on host threads, a wait, the upload),
             in the same process: device_us, host_seconds, their ratio, the launches per refactor, plan_bytes, pivot_pairs, and the
             byte model — scatter: every block read and written once, its gather index, D_i written twice; pivots: per L block itself,
             Einv_j, its mate and two indices, per block row Einv and K read and written — with its time at this box's
             mi_stream_read_probe rate and the fraction of that rate the device refactor reaches.

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


def dilu_mode(a):
    """--precond dilu (module docstring)."""
    import torch
    from navierstokes_amd import mpk, synth

    bp, bc, bv = synth.csr_to_bcsr4(*synth.fe_matrix(a.cells))
    nb = len(bp) - 1
    n = 4 * nb
    nblk = len(bc)
    A = mpk.bcsr4x4_matrix(nb, bp, bc, bv)
    orders = [o for o in a.order.split(",") if o]
    assert orders and all(o in mpk.BILU_ORDERS for o in orders), "--order: natural, colour"
    b = synth.x_sin(0, n) + 1.0
    db = torch.from_numpy(b).cuda()
    dx, dy, dz = torch.zeros_like(db), torch.zeros_like(db), torch.zeros_like(db)
    bnorm = float(np.linalg.norm(b))
    t0 = time.perf_counter()
    dilus = {o: mpk.dilu4(A, order=o) for o in orders}
    dilu_create = {o: dilus[o].info()["factor_seconds"] for o in orders}
    ilus = {o: mpk.bilu4(A, fill=0, order=o) for o in ("colour", "natural")}
    print(f"handles: {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)

    def timed(fn, warm=20, reps=200):
        for _ in range(warm):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return round(e0.elapsed_time(e1) * 1e3 / reps, 2)

    vec = 8 * n
    blk = 16 * 8 + 4
    apply = dict(product_us=timed(lambda: mpk.SpMV_BCSR(dy, db, A)), ilu0_colour_solve_us=timed(lambda: ilus["colour"].solve(dy, db)),
                 ilu0_natural_solve_us=timed(lambda: ilus["natural"].solve(dy, db)),
                 product_plus_ilu0_colour_us=timed(lambda: (ilus["colour"].solve(dz, db), mpk.SpMV_BCSR(dy, dz, A))),
                 # the product reads every block and x, writes y; the solve reads every factor block (fill 0: as many), b, and x twice
                 product_plus_ilu0_model_bytes=2 * nblk * blk + 7 * vec, ilu0_factor_bytes=ilus["colour"].info()["factor_bytes"])
    for o, E in dilus.items():
        info = E.info()
        apply[f"dilu_{o}"] = dict(apply_hat_us=timed(lambda: E.apply_hat(dy, db)), to_hat_us=timed(lambda: E.to_hat(dy, db)),
                                  from_hat_us=timed(lambda: E.from_hat(dy, db)), launches=info["launches"], levels=[info["fwd_levels"], info["bwd_levels"]],
                                  ncolours=info["ncolours"], device_bytes=info["device_bytes"], pivots_host_seconds=round(dilu_create[o], 3),
                                  # both sweeps: every off-diagonal block once, Einv twice and K once per block row, u twice, t three times, y and w
                                  model_bytes=(nblk - nb) * blk + 3 * nb * 128 + 8 * vec)
    refactor = {}
    if a.refactor:
        dcoef = torch.from_numpy(np.ascontiguousarray(bv, dtype=np.float64)).cuda()
        hbm = (1 << 30) / mpk.stream_read_us(1 << 30)  # bytes per microsecond of a plain read sweep
        rows = np.repeat(np.arange(nb), np.diff(bp))
        for o, E in dilus.items():
            perm = E.info()["perm"].astype(np.int64)
            n_l = int((perm[np.asarray(bc)] < perm[rows]).sum())
            E.prepare_dev()
            dev_us = timed(lambda: E.refactor_dev(dcoef), warm=3, reps=20)
            E.factor_status()
            host = []
            for _ in range(3):
                t0 = time.perf_counter()
                E.refactor(bv)
                host.append(time.perf_counter() - t0)
            E.refactor_dev(dcoef).factor_status()  # the solves below run on what the device refactor left
            probe = mpk.dilu4dev_plan_probe(nb, bp, bc, o)
            scatter = nblk * (2 * 128 + 4) + nb * 128
            pivots = n_l * (3 * 128 + 8) + nb * (4 * 128 + 8)
            model_us = (scatter + pivots) / hbm
            refactor[o] = dict(device_us=dev_us, host_seconds=round(statistics.median(host), 4), host_over_device=round(statistics.median(host) * 1e6 / dev_us, 1),
                               launches=E.info_dev()["launches"], plan_bytes=E.info_dev()["plan_bytes"], pivot_pairs=probe["pivot_pairs"],
                               model_bytes=dict(scatter=scatter, pivots=pivots), read_probe_bytes_per_us=round(hbm, 1), model_us=round(model_us, 2),
                               fraction_of_model=round(model_us / dev_us, 3))
        del dcoef
    solvers = {}
    for o, E in dilus.items():
        S = mpk.gmres_solver(E, None, RESTART)
        r, u = torch.zeros_like(db), torch.zeros_like(db)

        def run_dilu(E=E, S=S, r=r, u=u):  # mpk.dilu4.gmres, on one solver handle
            mpk.SpMV_BCSR(dy, dx, A)
            r.copy_(db)
            mpk.axpy(-1.0, dy, r)
            E.to_hat(r, r)
            u.zero_()
            its, hist, _ = S.solve(r, u, rtol=RTOL, maxiter=a.maxiter, check_every=1)
            E.from_hat(u, u)
            mpk.axpy(1.0, u, dx)
            return its, hist
        solvers[f"dilu_{o}"] = (run_dilu, S)
    for label, M in [("ilu0_colour_exact", ilus["colour"]), ("ilu0_natural_exact", ilus["natural"]), (f"ilu0_natural_sweeps{a.sweeps}", ilus["natural"].sweeps(a.sweeps))]:
        S = mpk.gmres_solver(A, M, RESTART)
        solvers[label] = ((lambda S=S: S.solve(db, dx, rtol=RTOL, maxiter=a.maxiter, check_every=1)[:2]), S)

    def run(fn):
        dx.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        its, hist = fn()
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        mpk.SpMV_BCSR(dy, dx, A)
        return its, sec, float(np.linalg.norm(b - dy.cpu().numpy()) / bnorm), float(hist[-1])

    for fn, _ in solvers.values():
        run(fn)
    secs, last = {k: [] for k in solvers}, {}
    for _ in range(a.runs):
        for k, (fn, _) in solvers.items():
            its, sec, true, rec = run(fn)
            secs[k].append(sec)
            last[k] = dict(iterations=its, true_residual=true, recurrence_residual=rec, norm="hat" if k.startswith("dilu") else "true")
    out = dict(tool="bench_gmres_dilu", cells=a.cells, rows=n, blocks=nblk, restart=RESTART, rtol=RTOL, runs=a.runs, apply=apply, solvers={})
    if a.refactor:
        out["refactor"] = refactor
    for k in solvers:
        med = statistics.median(secs[k])
        out["solvers"][k] = dict(last[k], seconds=round(med, 6), spread_seconds=round(max(secs[k]) - min(secs[k]), 6),
                                 us_per_iteration=round(med * 1e6 / max(last[k]["iterations"], 1), 2))
    line = json.dumps(out)
    print(line, flush=True)
    if not a.no_append:
        with open(os.path.join(ROOT, "profiles", "gmres_bench.jsonl"), "a") as f:
            f.write(line + "\n")
    for _, S in solvers.values():
        S.close()
    for h in list(dilus.values()) + list(ilus.values()) + [A]:
        h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precond", choices=("ilu", "dilu"), default="ilu", help="dilu: block DILU with Eisenstat's trick against ILU(0) (module docstring)")
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
    ap.add_argument("--refactor", action="store_true", help="with --precond dilu: the device refactor against the host path (module docstring)")
    ap.add_argument("--order", default="natural", help="comma-separated orderings of the block rows: natural, colour")
    a = ap.parse_args()
    if a.precond == "dilu":
        return dilu_mode(a)
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
