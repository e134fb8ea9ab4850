#!/usr/bin/env python3
"""The block ILU preconditioner on the FE matrix at the bench's size (fill = 0): host factor seconds, microseconds per solve of
every built form (device events around back-to-back solves, after warm-ups), launches per solve, the factor's bytes, the blocked
product's microseconds on a handle of the same matrix in the same process, and GMRES(30) iterations and seconds to rtol = 1e-8
with and without M.  Prints one JSON line and appends it to profiles/ilu_bench.jsonl.

    python3 tools/bench_ilu.py [--cells 68] [--fill 0] [--solves 200] [--maxiter 300] [--no-append]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_us(fn, warm, reps):
    import torch
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=68)
    ap.add_argument("--fill", type=int, default=0)
    ap.add_argument("--solves", type=int, default=200)
    ap.add_argument("--maxiter", type=int, default=300)
    ap.add_argument("--no-append", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    from navierstokes_amd import mpk, synth
    assert torch.cuda.is_available(), "bench_ilu.py needs a GPU"
    bp, bc, bv = synth.csr_to_bcsr4(*synth.fe_matrix(a.cells))
    nb = len(bp) - 1
    n = 4 * nb
    A = mpk.bcsr4x4_matrix(nb, bp, bc, bv)
    t0 = time.perf_counter()
    F = mpk.bilu4(A, fill=a.fill)
    create_s = time.perf_counter() - t0
    info = F.info()
    b = synth.x_sin(0, n) + 1.0
    db = torch.from_numpy(b).cuda()
    dx, dy = torch.zeros_like(db), torch.zeros_like(db)
    solve_us = timed_us(lambda: F.solve(dx, db), 20, max(a.solves, 200))
    spmv_us = timed_us(lambda: mpk.SpMV_BCSR(dy, db, A), 20, max(a.solves, 200))
    out = dict(tool="bench_ilu", cells=a.cells, rows=n, block_rows=nb, blocks=int(len(bc)), fill=a.fill, factor_blocks=info["nblocks"],
               factor_bytes=info["factor_bytes"], host_factor_seconds=round(info["factor_seconds"], 4), create_seconds=round(create_s, 3),
               fwd_levels=info["fwd_levels"], bwd_levels=info["bwd_levels"], launches_per_solve=info["launches"], form_in_use=info["form"],
               solve_us={"per_level_launches": round(solve_us, 2), "one_launch": None},
               us_per_launch=round(solve_us / max(info["launches"], 1), 3), bcsr4_spmv_us=round(spmv_us, 2),
               solve_over_spmv=round(solve_us / spmv_us, 2), gmres={})
    for label, M in (("ilu", F), ("none", None)):
        dx.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        its, hist = mpk.GMRES(A, db, dx, M=M, restart=30, rtol=1e-8, maxiter=a.maxiter)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        mpk.SpMV_BCSR(dy, dx, A)
        true = float(np.linalg.norm(b - dy.cpu().numpy()) / np.linalg.norm(b))
        out["gmres"][label] = dict(iterations=its, seconds=round(sec, 4), recurrence_residual=float(hist[-1]), true_residual=true,
                                   converged=bool(hist[-1] <= 1e-8))
    line = json.dumps(out)
    print(line)
    if not a.no_append:
        with open(os.path.join(ROOT, "profiles", "ilu_bench.jsonl"), "a") as f:
            f.write(line + "\n")
    F.close()
    A.close()


if __name__ == "__main__":
    main()
