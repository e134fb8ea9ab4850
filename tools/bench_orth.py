"""Orthogonalising one vector against m basis vectors, three ways, on device vectors:
  mgs_norm  mi_orthonormalize_against_basis_dev + mi_norm2_dev (the sequential sweep, m + 3 launches)
  cgs1      mi_cgs_dev, one pass  (3 launches per tile-chunked pass: blas1_multi.hpp)
  cgs2      mi_cgs_dev, two passes
for n in {1 M, 5 M} and m in {1, 2, 4, 8, 16, 30}: us per call (HIP events around a window of back-to-back calls on one stream,
after warm-up; the three paths alternate inside every repeat, the median over the repeats is reported with its min and max) and
bytes per second against the byte models
  mgs_norm  (32 m + 16) n          cgs, per pass  8 (2 m + 3 ceil(m / TILE)) n
One JSON line per case, and a last line that states the two requirements at n = 5 M (one pass faster than the sweep for every
m >= 2; two passes at m = 30 within 1.18 x (the byte model) plus the spread observed between repeats).

--basis f32 | both adds the same two passes against the basis STORED IN FLOAT (mi_cgs_f32_dev; paths cgs1_f32, cgs2_f32), byte model
per pass (4 . 2 m + 8 . 3 ceil(m / TILE)) n; --tiles then names the tile of the float basis too (MI355_MDOT_TILE_F32: 8 or 16).

Every (tile, n) is measured by a fresh child process under its own `timeout`; the first child that fails ends the run.
  python tools/bench_orth.py [--tiles 8 | 4,8,16] [--basis f64|f32|both] [--sizes 5000000] [--out profiles/orth_bench.jsonl]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (1_000_000, 5_000_000)
COUNTS = (1, 2, 4, 8, 16, 30)
PATHS = ("mgs_norm", "cgs1", "cgs2")
PATHS_F32 = ("cgs1_f32", "cgs2_f32")


def model_bytes(path, n, m, tile):
    if path == "mgs_norm":
        return (32 * m + 16) * n
    chunks = -(-m // tile)
    if path in PATHS_F32:
        return (1 if path == "cgs1_f32" else 2) * (4 * 2 * m + 8 * 3 * chunks) * n
    return (1 if path == "cgs1" else 2) * 8 * (2 * m + 3 * chunks) * n


def child(n, tile, iters, repeats, basis_kind="f64"):
    import torch
    from navierstokes_amd import mpk
    L = mpk.lib()
    g = torch.Generator(device="cuda").manual_seed(n)
    mmax = max(COUNTS)
    # small basis entries: the updates stay tiny, so y neither grows nor vanishes over thousands of calls
    basis = (torch.rand((mmax, n), dtype=torch.float64, device="cuda", generator=g) - 0.5) * (1e-3 / n ** 0.5)
    y = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
    h = torch.zeros(mmax, dtype=torch.float64, device="cuda")
    nrm = torch.zeros(1, dtype=torch.float64, device="cuda")
    vp = ctypes.c_void_p
    ptrs = (vp * mmax)(*[basis[j].data_ptr() for j in range(mmax)])
    paths = (PATHS if basis_kind != "f32" else ()) + (PATHS_F32 if basis_kind != "f64" else ())
    if basis_kind != "f64":
        basis32 = basis.float()  # (n is even: every row is 8-byte aligned)
        ptrs32 = (vp * mmax)(*[basis32[j].data_ptr() for j in range(mmax)])
    py, ph, pn = vp(y.data_ptr()), vp(h.data_ptr()), vp(nrm.data_ptr())
    st = vp(torch.cuda.current_stream().cuda_stream)
    stream_gbs = 200e6 / mpk.stream_read_us(200_000_000) / 1e3  # this box's plain read sweep (bench.py: roofline.this_box_stream_read)

    def run(path, m):
        if path == "mgs_norm":
            mpk.check(L.mi_orthonormalize_against_basis_dev(n, m, ptrs, py, ph, st))
            mpk.check(L.mi_norm2_dev(n, py, pn, st))
        elif path in PATHS_F32:
            mpk.check(L.mi_cgs_f32_dev(n, m, ptrs32, py, 1 if path == "cgs1_f32" else 2, ph, pn, st))
        else:
            mpk.check(L.mi_cgs_dev(n, m, ptrs, py, 1 if path == "cgs1" else 2, ph, pn, st))

    for m in COUNTS:
        for path in paths:
            for _ in range(5):
                run(path, m)
        torch.cuda.synchronize()
        us = {p: [] for p in paths}
        for _ in range(repeats):
            for path in paths:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    run(path, m)
                e1.record()
                e1.synchronize()
                us[path].append(e0.elapsed_time(e1) / iters * 1e3)
        assert bool(torch.isfinite(y).all()) and float(nrm.cpu()) > 0
        med = {p: statistics.median(us[p]) for p in paths}
        out = dict(tool="bench_orth", n=n, m=m, tile=tile, basis=basis_kind, iters=iters, repeats=repeats, stream_read_gbs=round(stream_gbs, 1))
        for p in paths:
            b = model_bytes(p, n, m, tile)
            out[p] = dict(us=round(med[p], 2), us_min=round(min(us[p]), 2), us_max=round(max(us[p]), 2),
                          spread=round((max(us[p]) - min(us[p])) / med[p], 4), bytes=b, gbs=round(b / med[p] / 1e3, 1))
        if "mgs_norm" in med:
            out["cgs1_over_mgs_norm"] = round(med["cgs1"] / med["mgs_norm"], 4)
            out["cgs2_over_mgs_norm"] = round(med["cgs2"] / med["mgs_norm"], 4)
        if basis_kind == "both":
            out["cgs2_f32_over_cgs2"] = round(med["cgs2_f32"] / med["cgs2"], 4)
        print(json.dumps(out), flush=True)


def verdict(lines, tile):
    """The two requirements at n = 5 M for one tile, from the measured medians and the spread between repeats."""
    big = [d for d in lines if d["n"] == 5_000_000 and d["tile"] == tile and "cgs1_over_mgs_norm" in d]
    if not big:
        return None
    one_pass = {d["m"]: d["cgs1_over_mgs_norm"] for d in big if d["m"] >= 2}
    d30 = next(d for d in big if d["m"] == 30)
    spread = max(d30["cgs2"]["spread"], d30["mgs_norm"]["spread"])
    return dict(tool="bench_orth", verdict=True, tile=tile, n=5_000_000, one_pass_over_sweep=one_pass,
                one_pass_faster_for_every_m_from_2=all(r < 1.0 for r in one_pass.values()),
                two_passes_over_sweep_m30=d30["cgs2_over_mgs_norm"], byte_model_ratio=1.18, observed_spread=spread,
                bound=round(1.18 + spread, 4), two_passes_within_bound=d30["cgs2_over_mgs_norm"] <= 1.18 + spread,
                two_passes_within_1p3=d30["cgs2_over_mgs_norm"] <= 1.3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", default="", help="comma-separated MI355_MDOT_TILE values to force (default: the library's own)")
    ap.add_argument("--out", default="")
    ap.add_argument("--basis", choices=("f64", "f32", "both"), default="f64")
    ap.add_argument("--sizes", default="", help="comma-separated n (default: 1 M and 5 M)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--tile", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.tile, a.iters, a.repeats, a.basis)
    tiles = [int(t) for t in a.tiles.split(",") if t] or [0]
    lines = []
    for tile in tiles:
        env = dict(os.environ)
        for var in ("MI355_MDOT_TILE",) + (("MI355_MDOT_TILE_F32",) if a.basis != "f64" else ()):
            if tile:
                env[var] = str(tile)
            else:
                env.pop(var, None)
        shown = tile or 8  # the library's default (MI355_MDOT_TILE_DEFAULT in capi_blas1.hip)
        for n in [int(v) for v in a.sizes.split(",") if v] or SIZES:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", str(n), "--tile", str(shown),
                   "--iters", str(a.iters), "--repeats", str(a.repeats), "--basis", a.basis]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            if r.returncode != 0:  # nothing more is started on the GPU after a failure
                sys.stderr.write(r.stderr[-4000:])
                sys.exit(f"bench_orth: child tile={shown} n={n} ended with status {r.returncode}")
            lines += [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
        v = verdict(lines, shown)
        if v:
            print(json.dumps(v), flush=True)
            lines.append(v)
    if a.out:
        with open(a.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
