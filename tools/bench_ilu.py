#!/usr/bin/env python3
"""The block ILU preconditioner on the FE matrix at the bench's size (fill = 0): host factor seconds, microseconds per solve of
every built form (device events around back-to-back solves, after warm-ups), launches per solve, the factor's bytes, the blocked
product's microseconds on a handle of the same matrix in the same process, and GMRES(30) iterations and seconds to rtol = 1e-8
with and without M.  Prints one JSON line and appends it to profiles/ilu_bench.jsonl.

    python3 tools/bench_ilu.py [--cells 68] [--fill 0] [--solves 200] [--maxiter 300] [--form both|0|1] [--no-append]

--form: which forms of the solve to measure, on the SAME handle in one process (mi_bilu4_set_solve_form): 0 one launch per level,
1 both sweeps in one launch, both (default; form 0 only, with the reason recorded, where the pattern is not eligible for form 1).
The record then also carries the one-launch plan (workgroups, chunks per sweep, the largest dependency list) and GMRES(30) with
each form as M.

--sweeps 1,2,3,4,6,8 adds the sweep solve (mi_bilu4sw_*, mpk.bilu4.sweeps) on the SAME handle in the same process: for each count s
(per triangle) microseconds per application (back-to-back solves between device events, as for the forms), its launches, the bytes
of the byte model s L + D + s (U + D) and the rate they amount to, and GMRES(30) iterations, seconds and true residual with
M = F.sweeps(s), beside the exact solve's.  The record names the depth of the kernel's software pipeline the library was built
with (pipeline_depth: kBiluSweepDepth of bilu4_sweep.hpp).

    python3 tools/bench_ilu.py --sweeps 1,2,3,4,6,8 [--cells 68] [--fill 0] [--precision f64|f32|both]

--precision (with --sweeps; default f64): which values the sweeps stream — the double factor, its single-precision copy
(mi_bilu4sp_*, mpk.bilu4.sweeps(.., precision="f32")), or both on the SAME handle in the same process.  With f32 the record carries
per count the same figures for the copy under "f32" (byte model: 68 bytes per block and 64 per inverted diagonal block), the ratio
f32 / f64 measured and modelled, the cost of one more sweep pair in each precision (from consecutive counts), the copy's bytes, the
depth of the f32 pipeline, and the microseconds of ONE conversion: mi_bilu4dev_refactor timed on this handle before the copy
exists and again with the conversion attached (median of single refactors between device events), and their difference.

--order natural,colour (default natural): which orderings of the block rows to measure, each on a handle of its own built on the
SAME matrix in one process (mpk.bilu4(order=)); one JSON line per ordering, combinable with --form, --sweeps and --precision.  A
colour-order record also carries the colours, the launches that take the wide-level kernel, and boundary_us: the cost of the two
launches at the solve's boundary, measured as the diagonal-only sweep solve (0 sweeps: one launch) on the ordered handle minus the
same on the natural-order handle (with both orderings asked for).  --wide-min 64,1024,...: for the colour order, form 0 timed on
further handles created with MI355_BILU_WIDE_MIN set to each value (0: the wide kernel never) — wide_min_curve.

    python3 tools/bench_ilu.py --order natural,colour [--wide-min 0,64,1024,4096,16384] [--sweeps 3,4] [--cells 68] [--fill 0]

--exact-precision f64|f32|both (default f64): which values the EXACT solve streams — the double factor (the forms above), its
single-precision copy (mi_bilu4spx_*, mpk.bilu4.exact("f32"): always level by level), or both on the SAME handle in the same
process.  With f32 the record carries under "exact_f32" the microseconds per solve, its launches and those that were wide, the
ratio to the double level-by-level solve measured on this handle just before and the ratio of the byte model (68 against 132
bytes per block, 64 against 128 per inverted diagonal block, the vectors the same), and GMRES(30) with M = F.exact("f32").  Every
record names what was asked for in "exact_precision".

    python3 tools/bench_ilu.py --order natural,colour --exact-precision both [--cells 68] [--fill 0]

--refactor measures the two refactorisations instead, in one process, and appends one record (tool = "bench_ilu_refactor"): the
wall time of the host path mi_bilu4_refactor (factor on host threads, wait for the device, upload; median of --host-reps calls),
the time of mi_bilu4dev_refactor between device events (median of --reps single refactors after warm-ups), launches per refactor,
the bytes of the device plan, and whether the fetched device factor equals the host factor bit for bit; then the device refactor
again with the single-precision copy prepared (the conversion attached: two more launches), and whether the fetched copy is the
rounded host factor bit for bit.

    python3 tools/bench_ilu.py --refactor [--cells 68] [--fill 0] [--reps 30] [--host-reps 3] [--no-append]
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


def dev_refactor_us(F, dcoef, reps):
    """Single device refactors between device events, after warm-ups: the list of their microseconds."""
    import torch
    for _ in range(3):
        F.refactor_dev(dcoef)
    F.factor_status()
    us = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):
        e0.record()
        F.refactor_dev(dcoef)
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return us


def refactor_record(a):
    import numpy as np
    import torch
    from navierstokes_amd import mpk, synth
    bp, bc, bv = synth.csr_to_bcsr4(*synth.fe_matrix(a.cells))
    nb = len(bp) - 1
    F = mpk.bilu4(nb, bp, bc, bv, fill=a.fill)
    info = F.info()
    new = np.asarray(bv) * 1.25  # other values, the same pivots up to scale
    host_s = []
    for _ in range(a.host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        F.refactor(new)
        host_s.append(time.perf_counter() - t0)
    host_factor = F.factor_host()[3].copy()
    host_only_s = F.info()["factor_seconds"]
    t0 = time.perf_counter()
    F.prepare_dev()
    prepare_s = time.perf_counter() - t0
    dcoef = torch.from_numpy(np.ascontiguousarray(new)).cuda()
    dev_us = dev_refactor_us(F, dcoef, a.reps)
    F.factor_status().fetch_factor()
    same = bool(np.array_equal(F.factor_host()[3].view(np.uint64), host_factor.view(np.uint64)))
    dinfo = F.info_dev()
    probe = mpk.bilu4dev_plan_probe(nb, bp, bc, a.fill)
    dev_med = float(np.median(dev_us))
    F.prepare_sweeps(precision="f32")
    sp_us = dev_refactor_us(F, dcoef, a.reps)
    F.factor_status().sweep_status_f32()
    with np.errstate(all="ignore"):
        sp_same = bool(np.array_equal(F.fetch_f32().view(np.uint32), host_factor.astype(np.float32).view(np.uint32)))
    sp_med = float(np.median(sp_us))
    out = dict(tool="bench_ilu_refactor", cells=a.cells, block_rows=nb, blocks=int(len(bc)), fill=a.fill, factor_blocks=info["nblocks"],
               fwd_levels=info["fwd_levels"], host_refactor_seconds=round(float(np.median(host_s)), 4), host_refactor_calls=a.host_reps,
               host_factor_only_seconds=round(host_only_s, 4), dev_refactor_us=round(dev_med, 1), dev_refactor_us_min=round(min(dev_us), 1),
               dev_refactor_us_max=round(max(dev_us), 1), dev_refactor_reps=a.reps, launches_per_refactor=dinfo["launches"],
               us_per_launch=round(dev_med / dinfo["launches"], 2), plan_bytes=dinfo["plan_bytes"], update_pairs=probe["update_pairs"],
               prepare_seconds=round(prepare_s, 3), host_over_dev=round(float(np.median(host_s)) * 1e6 / dev_med, 1), device_factor_equals_host_bits=same,
               dev_refactor_with_f32_copy_us=round(sp_med, 1), convert_us=round(sp_med - dev_med, 1), f32_copy_bytes=F.sweep_info_f32()["copy_bytes"],
               f32_copy_equals_rounded_host_bits=sp_same)
    F.close()
    return out


def sweeps_record(a, F, A, b, db, dx, dy, coef):
    """The sweep solve on the handle the forms were measured on (in whatever form it was left: the sweeps do not depend on it)."""
    import re
    import numpy as np
    import torch
    from navierstokes_amd import mpk
    F.prepare_sweeps()
    depth = int(re.search(r"kBiluSweepDepth = (\d+);", open(os.path.join(ROOT, "navierstokes_amd", "csrc", "bilu4_sweep.hpp")).read()).group(1))
    ptr, col, diag, _ = F.factor_host()
    nb = len(ptr) - 1
    n_l = int(np.sum(diag - ptr[:-1]))
    n_u = int(np.sum(ptr[1:] - diag - 1))
    # values and block columns of a triangle, the inverted diagonal blocks; per launch the source read and the result written
    # (the gathered iterate is left to the caches, as in the blocked product's byte model)
    l_bytes, u_bytes, d_bytes, vec = n_l * 132, n_u * 132, nb * 128, 2 * 32 * nb
    reps = max(a.solves, 200)
    rec = dict(pipeline_depth=depth, max=[F.sweep_info()["max_fwd"], F.sweep_info()["max_bwd"]], work_bytes=F.sweep_info()["work_bytes"], l_bytes=l_bytes, u_bytes=u_bytes,
               dinv_bytes=d_bytes, counts={})
    precisions = ["f64", "f32"] if a.precision == "both" else [a.precision]
    # per precision: bytes of a block with its column, of an inverted diagonal block
    per_block = {"f64": (132, 128), "f32": (68, 64)}
    if "f32" in precisions:
        src = open(os.path.join(ROOT, "navierstokes_amd", "csrc", "bilu4_sweep.hpp")).read()
        depth32 = int(os.environ.get("MI355_BILU_SWEEP_DEPTH_F32") or re.search(r"#define MI355_BILU_SWEEP_DEPTH_F32 (\d+)", src).group(1))
        dcoef = torch.from_numpy(np.ascontiguousarray(coef)).cuda()  # the values the handle holds: the factor does not change
        F.prepare_dev()
        without = float(np.median(dev_refactor_us(F, dcoef, 30)))
        F.prepare_sweeps(precision="f32")
        attached = float(np.median(dev_refactor_us(F, dcoef, 30)))
        F.factor_status().sweep_status_f32()
        rec.update(pipeline_depth_f32=depth32, f32_copy_bytes=F.sweep_info_f32()["copy_bytes"], dev_refactor_us=round(without, 1),
                   dev_refactor_with_f32_copy_us=round(attached, 1), convert_us=round(attached - without, 1))
    for s in [int(c) for c in a.sweeps.split(",") if c]:
        sf, sb = min(s, rec["max"][0]), min(s, rec["max"][1])
        entry = {}
        for prec in precisions:
            V = F.sweeps(s, precision=prec)
            us = timed_us(lambda: V.solve(dx, db), 20, reps)
            launches = (F.sweep_info_f32() if prec == "f32" else F.sweep_info())["launches_last"]
            blk, dia = per_block[prec]
            model = sf * n_l * blk + nb * dia + sb * (n_u * blk + nb * dia) + launches * vec
            dx.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            its, hist = mpk.GMRES(A, db, dx, M=V, restart=30, rtol=1e-8, maxiter=a.maxiter)
            torch.cuda.synchronize()
            sec = time.perf_counter() - t0
            mpk.SpMV_BCSR(dy, dx, A)
            true = float(np.linalg.norm(b - dy.cpu().numpy()) / np.linalg.norm(b))
            entry[prec] = dict(us=round(us, 2), launches=launches, us_per_launch=round(us / launches, 2), model_bytes=model,
                               model_gb_per_s=round(model / us * 1e-3, 1),
                               gmres=dict(iterations=its, seconds=round(sec, 4), recurrence_residual=float(hist[-1]), true_residual=true,
                                          converged=bool(hist[-1] <= 1e-8)))
        # (the double sweeps keep the record's earlier shape: their figures lie directly under the count)
        out = dict(entry["f64"]) if "f64" in entry else {}
        if "f32" in entry:
            out["f32"] = entry["f32"]
        if len(entry) == 2:
            out["f32_over_f64"] = round(entry["f32"]["us"] / entry["f64"]["us"], 3)
            out["f32_over_f64_model"] = round(entry["f32"]["model_bytes"] / entry["f64"]["model_bytes"], 3)
        rec["counts"][str(s)] = out
    # one more forward + backward sweep pair, from consecutive counts below the clamp
    done = sorted(int(c) for c in rec["counts"])
    pairs = {}
    for lo, hi in zip(done, done[1:]):
        if hi > min(rec["max"]):
            continue
        for prec in precisions:
            at = (lambda c: rec["counts"][str(c)]["f32"] if prec == "f32" else rec["counts"][str(c)])
            pairs.setdefault(prec, {})[f"{lo}->{hi}"] = round((at(hi)["us"] - at(lo)["us"]) / (hi - lo), 2)
    rec["us_per_sweep_pair"] = pairs
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refactor", action="store_true")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--cells", type=int, default=68)
    ap.add_argument("--fill", type=int, default=0)
    ap.add_argument("--solves", type=int, default=200)
    ap.add_argument("--maxiter", type=int, default=300)
    ap.add_argument("--form", choices=("both", "0", "1"), default="both")
    ap.add_argument("--sweeps", default="", help="comma-separated sweep counts per triangle")
    ap.add_argument("--precision", choices=("f64", "f32", "both"), default="f64", help="with --sweeps: the values the sweeps stream")
    ap.add_argument("--exact-precision", choices=("f64", "f32", "both"), default="f64", help="the values the exact solve streams")
    ap.add_argument("--order", default="natural", help="comma-separated orderings of the block rows: natural, colour")
    ap.add_argument("--wide-min", default="", help="with the colour order: comma-separated MI355_BILU_WIDE_MIN values to time form 0 at (0: never wide)")
    ap.add_argument("--no-append", action="store_true")
    a = ap.parse_args()
    import torch
    from navierstokes_amd import mpk, synth
    assert torch.cuda.is_available(), "bench_ilu.py needs a GPU"

    def emit(rec):
        line = json.dumps(rec)
        print(line)
        if not a.no_append:
            with open(os.path.join(ROOT, "profiles", "ilu_bench.jsonl"), "a") as f:
                f.write(line + "\n")

    if a.refactor:
        emit(refactor_record(a))
        return
    orders = [o for o in a.order.split(",") if o]
    assert orders and all(o in mpk.BILU_ORDERS for o in orders), "--order: natural, colour"
    bp, bc, bv = synth.csr_to_bcsr4(*synth.fe_matrix(a.cells))
    nb = len(bp) - 1
    A = mpk.bcsr4x4_matrix(nb, bp, bc, bv)
    diag_only_us = {}
    for order in orders:
        emit(order_record(a, A, bv, order, diag_only_us if orders != ["natural"] else None))
    A.close()


def wide_min_handle(A, fill, wide_min):
    """A colour-order handle created with MI355_BILU_WIDE_MIN=wide_min (0: a threshold no level reaches)."""
    from navierstokes_amd import mpk
    old = os.environ.get("MI355_BILU_WIDE_MIN")
    os.environ["MI355_BILU_WIDE_MIN"] = str(wide_min if wide_min > 0 else 2 ** 31 - 1)
    try:
        return mpk.bilu4(A, fill=fill, order="colour")
    finally:
        if old is None:
            del os.environ["MI355_BILU_WIDE_MIN"]
        else:
            os.environ["MI355_BILU_WIDE_MIN"] = old


def order_record(a, A, bv, order, diag_only_us):
    """Everything the tool measures, on a handle of `order` built on A.  diag_only_us: the orderings' diagonal-only times so far, or None."""
    import numpy as np
    import torch
    from navierstokes_amd import mpk, synth
    nb, bc = A.nrows, A.indcol
    n = 4 * nb
    t0 = time.perf_counter()
    F = mpk.bilu4(A, fill=a.fill, order=order)
    create_s = time.perf_counter() - t0
    info = F.info()
    b = synth.x_sin(0, n) + 1.0
    db = torch.from_numpy(b).cuda()
    dx, dy = torch.zeros_like(db), torch.zeros_like(db)
    forms = [0, 1] if a.form == "both" else [int(a.form)]
    one, why_not = None, None
    if 1 in forms:
        try:
            F.prepare_one()
            one = F.info_one()
        except mpk.MiError as e:
            if e.status != 5 or a.form == "1":
                raise
            forms, why_not = [0], str(e)
    names = {0: "per_level_launches", 1: "one_launch"}
    us = {0: None, 1: None}
    for form in forms:
        assert F.set_form(form) == form
        us[form] = timed_us(lambda: F.solve(dx, db), 20, max(a.solves, 200))
        F.one_status()
    solve_us = us[forms[0]]
    spmv_us = timed_us(lambda: mpk.SpMV_BCSR(dy, db, A), 20, max(a.solves, 200))
    out = dict(tool="bench_ilu", order=order, cells=a.cells, rows=n, block_rows=nb, blocks=int(len(bc)), fill=a.fill, factor_blocks=info["nblocks"],
               factor_bytes=info["factor_bytes"], host_factor_seconds=round(info["factor_seconds"], 4), create_seconds=round(create_s, 3),
               fwd_levels=info["fwd_levels"], bwd_levels=info["bwd_levels"], launches_per_solve=info["launches"], form_in_use=info["form"],
               solve_us={names[f]: (None if us[f] is None else round(us[f], 2)) for f in (0, 1)},
               us_per_launch=round(solve_us / max(info["launches"], 1), 3) if forms[0] == 0 else None, bcsr4_spmv_us=round(spmv_us, 2),
               solve_over_spmv=round(solve_us / spmv_us, 2), forms=forms, one_launch_plan=one, one_launch_not_eligible=why_not,
               one_over_levels=round(us[1] / us[0], 3) if len(forms) == 2 else None, exact_precision=a.exact_precision, gmres={})
    Mx = None
    if a.exact_precision != "f64":
        # the comparison base: the double level-by-level solve on this handle, timed again right beside the f32 one
        assert F.set_form(0) == 0
        Mx = F.exact("f32")
        Mx.solve(dx, db)  # (prepares the copy)
        F.sweep_status_f32()
        base_us = timed_us(lambda: F.solve(dx, db), 20, max(a.solves, 200))
        x32_us = timed_us(lambda: Mx.solve(dx, db), 20, max(a.solves, 200))
        xinfo = F.exact_info_f32()
        offdiag = info["nblocks"] - nb
        model = {prec: offdiag * blk + nb * dia + 2 * 2 * 32 * nb for prec, (blk, dia) in (("f64", (132, 128)), ("f32", (68, 64)))}
        out["exact_f32"] = dict(us=round(x32_us, 2), f64_levels_us=round(base_us, 2), launches=xinfo["launches_last"], wide_launches=xinfo["wide_launches_last"],
                                f32_over_f64=round(x32_us / base_us, 3), model_bytes=model, f32_over_f64_model=round(model["f32"] / model["f64"], 3),
                                model_gb_per_s={"f64": round(model["f64"] / base_us * 1e-3, 1), "f32": round(model["f32"] / x32_us * 1e-3, 1)},
                                f32_copy_bytes=F.sweep_info_f32()["copy_bytes"])
        if a.exact_precision == "f32":
            forms = []
    for label, M, form in [("ilu" if f == 0 else "ilu_one_launch", F, f) for f in forms] + ([("ilu_exact_f32", Mx, 0)] if Mx else []) + [("none", None, None)]:
        if form is not None:
            assert F.set_form(form) == form
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
    if a.sweeps:
        out["sweeps"] = sweeps_record(a, F, A, b, db, dx, dy, bv)
    # the diagonal-only sweep solve: ONE launch in natural order, the same plus the two boundary launches on an ordered handle
    # (timed only when an ordering other than natural is among those asked for: diag_only_us is None otherwise)
    if diag_only_us is not None:
        diag_only_us[order] = timed_us(lambda: F.sweeps(0).solve(dx, db), 20, max(a.solves, 200))
    if order != "natural":
        oinfo = F.order_info()
        sizes = mpk.bilu4_order_probe(nb, A.ptrow, A.indcol, order)["colour_sizes"]
        out.update(ncolours=oinfo["ncolours"], colour_sizes=[int(c) for c in sizes], wide_launches=oinfo["wide_launches"], diag_only_us=round(diag_only_us[order], 2),
                   boundary_us=round(diag_only_us[order] - diag_only_us["natural"], 2) if "natural" in diag_only_us else None)
        curve = {}
        for wm in [int(c) for c in a.wide_min.split(",") if c]:
            W = wide_min_handle(A, a.fill, wm)
            curve[str(wm)] = dict(us=round(timed_us(lambda: W.solve(dx, db), 20, max(a.solves, 200)), 2), wide_launches=W.order_info()["wide_launches"])
            W.close()
        if curve:
            out["wide_min_curve"] = curve
    F.close()
    return out


if __name__ == "__main__":
    main()
