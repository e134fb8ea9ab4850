"""The sliced-stream kernels (spmv_sstream.hpp, spmv_sstream_mw.hpp) at every limit of their plans.

CPU part (unmarked): for every case of tests/sstream_cases.py (the limit table and ~200 seeded cases), with shift 0 and 1,
mi_sstream_plan_probe_ex must agree EXACTLY with the plain restatement restate_plan — eligibility, rounds, steps, padding, the
refusal reason — and its replay must pass; mi_sstream_mw_plan_probe must give each cut-ring case its pinned outcome.  The table's
tags are checked against the restatement (a case tagged as sitting on a limit does), every limit has cases on both sides, and every
refusal reason of both planners is reached except those listed in sstream_cases.NOT_REACHED.

GPU part (gpu): every eligible case forced onto the sliced stream (MI355_SSTREAM=1, MI355_SPMV_KERNEL=sstream) in each of its four
forms (MI355_SSTREAM_FORM 0-3): the kernel and plan the probe predicts, y = A x bit for bit against the oracle's fma chain (y pre-filled
with NaN and a NaN guard behind it; x infinite at every column no nonzero names, so a padding place that were multiplied would show),
value refreshes from the host and from a device array on another stream (bitwise, and the handle's CSR copy too: read through the
stream kernel), the k = 3 powers, and row-mapped handles (a contiguous map with an odd offset: planned one row down; a scattered map).
Refused cases: mi_csr_set_kernel(sstream) fails, and a handle created without forcing gives the oracle's bits through another kernel.
Thinned: cases of 1 M rows or more (share_19 .. share_23) run forms 0 and 3 only, with one device refresh in form 0 and no powers or
row maps; row-mapped handles run in form 0 only; seeded cases run two forms each (all four over the set)."""
import ctypes

import numpy as np
import pytest

import sstream_cases as SC
from conftest import assert_bit_equal
from navierstokes_amd import mpk
from oracle import oracle as O

SEEDED = SC.seeded_cases()
BIG_ROWS = 1_000_000


def _padding_env(monkeypatch, case):
    monkeypatch.setenv("MI355_SSTREAM_MAX_PADDING", repr(case.padding_budget))


def probe_plain(n, ncols, p, c, shift):
    L = mpk.lib()
    e, r, st, pad = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong(), ctypes.c_double()
    rc = L.mi_sstream_plan_probe_ex(n, ncols, p.ctypes.data, c.ctypes.data, shift, 0, 0, ctypes.byref(e), ctypes.byref(r), ctypes.byref(st),
                                    ctypes.byref(pad), None, None)
    return dict(rc=rc, eligible=bool(e.value), rounds=r.value, steps=st.value, padding=pad.value, err=L.mi_last_error().decode())


def probe_mw(n, ncols, p, c, shift):
    L = mpk.lib()
    e, r, st, pad = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong(), ctypes.c_double()
    rc = L.mi_sstream_mw_plan_probe(n, ncols, p.ctypes.data, c.ctypes.data, shift, ctypes.byref(e), ctypes.byref(r), ctypes.byref(st), ctypes.byref(pad))
    return dict(rc=rc, eligible=bool(e.value), rounds=r.value, steps=st.value, padding=pad.value, err=L.mi_last_error().decode())


def refusal(err):
    assert err.startswith("not eligible: "), err
    return err[len("not eligible: "):]


def check_against_restatement(case, shift):
    """probe vs restate_plan at one shift; returns (restatement, plain probe, cut-ring probe or None)."""
    n, ncols, p, c = case.data
    R = SC.restate_plan(n, ncols, p, c, shift, case.padding_budget)
    P = probe_plain(n, ncols, p, c, shift)
    what = f"{case.name} shift {shift}"
    assert P["rc"] == 0, f"{what}: the probe's replay failed: {P['err']}"
    assert P["eligible"] == R["eligible"], (what, P, R["why"])
    assert (P["rounds"], P["steps"]) == (R["rounds"], R["steps"]), (what, P, R["rounds"], R["steps"])
    assert np.float64(P["padding"]).view(np.uint64) == np.float64(R["padding"]).view(np.uint64), (what, P["padding"], R["padding"])
    if not R["eligible"]:
        assert refusal(P["err"]) == R["why"], (what, P["err"], R["why"])
    M = None
    if not R["eligible"]:
        M = probe_mw(n, ncols, p, c, shift)
        assert M["rc"] == 0, f"{what}: the cut-ring probe's replay failed: {M['err']}"
        if not M["eligible"]:
            M["why"] = refusal(M["err"])
    return R, P, M


# ---- what each limit tag claims, measured on the restatement (shift 0) ---------------------------------------------------------
def _side(ok):
    return "in" if ok else "out"


TAG_SIDE = {
    "n_vs_slice": lambda c, R: _side(c.data[0] <= SC.SLICE),
    "n_vs_round": lambda c, R: _side(c.data[0] <= SC.ROUND),
    "n_vs_8_rounds": lambda c, R: _side(c.data[0] <= 8 * SC.ROUND),
    "rounds_vs_8": lambda c, R: _side(R["rounds"] < 8),
    "rounds_vs_256": lambda c, R: _side(R["rounds"] <= 256),
    "round_span": lambda c, R: _side(R["why"] != SC.R_REACH),
    "new_columns": lambda c, R: _side(R["why"] != SC.R_NEW and R["newcols"].max() <= SC.NEWMAX),
    "first_window_6144": lambda c, R: _side(R["w0"].max() <= SC.FILL * 256),
    "first_window_8192": lambda c, R: _side(R["why"] != SC.R_REACH and R["w0"].max() <= SC.RING),
    "padding": lambda c, R: _side(R["why"] != SC.R_PAD),
    "slice_2048": lambda c, R: _side(R["max_slice_nnz"] <= 2048),
    "slice_8192": lambda c, R: _side(R["max_slice_nnz"] <= 8192),
    "fill_grid": lambda c, R: _side(4 * R["rounds"] <= SC.fill_instantiation(R["max_slice_nnz"])[1]),
    "park": lambda c, R: _side(R["share"].max() - SC.TAIL <= SC.PARK),
}


@pytest.mark.parametrize("case", SC.TABLE, ids=lambda c: c.name)
def test_table_case_plans(case, monkeypatch):
    """The limit table: both planners, both shifts, against the restatement and the pinned outcomes."""
    _padding_env(monkeypatch, case)
    for shift in (0, 1):
        R, P, M = check_against_restatement(case, shift)
        if shift:
            continue
        outcome = "plain" if R["eligible"] else ("cut-ring" if M["eligible"] else "refused")
        assert outcome == case.expect, (case.name, outcome, R["why"], M and M.get("why"))
        if not R["eligible"]:
            assert R["why"] == case.why, (case.name, R["why"], case.why)
            assert ("cut-ring" if M["eligible"] else M["why"]) == case.mw, (case.name, M, case.mw)
        for t in case.tags:
            if ":" in t:
                lim, side = t.split(":")
                if lim in TAG_SIDE:
                    assert TAG_SIDE[lim](case, R) == side, f"{case.name}: tagged {t}, but the plan says {TAG_SIDE[lim](case, R)}"
        if "empty_workgroup" in case.tags:
            assert (R["w0"] == 0).any(), "no workgroup with an empty first window"
        if "reach_back" in case.tags:  # a round after a workgroup's first names a column more than half the ring below the window's end
            later = np.ones(R["rounds"], bool)
            later[R["rptr"][:-1]] = False
            assert R["eligible"] and (later & (R["cmin"] < R["whi"] - SC.RING // 2)).any(), case.name


@pytest.mark.parametrize("chunk", range(4))
def test_seeded_case_plans(chunk, monkeypatch):
    """~200 seeded cases near the limits: the probe agrees with the restatement at both shifts; every plan either form builds replays."""
    for case in SEEDED[chunk::4]:
        _padding_env(monkeypatch, case)
        for shift in (0, 1):
            check_against_restatement(case, shift)


def _reached():
    plain, mw = {}, {}
    for case in SC.TABLE:
        if case.expect != "plain" and case.why:
            plain.setdefault(case.why, []).append(case.name)
        if case.mw and case.mw != "cut-ring":
            mw.setdefault(case.mw, []).append(case.name)
    return plain, mw


def test_every_limit_both_sides_and_every_reason_reached(capsys):
    """Coverage: both sides of every limit tag, every feature, every refusal reason (minus NOT_REACHED, which must stay unreached)."""
    sides = {lim: {"in": [], "out": []} for lim in SC.LIMITS}
    for case in SC.TABLE:
        for t in case.tags:
            if ":" in t:
                lim, side = t.split(":")
                sides[lim][side].append(case.name)
    plain, mw = _reached()
    with capsys.disabled():
        print("\nsliced-stream limits: cases inside / outside")
        for lim in SC.LIMITS:
            print(f"  {lim:22s} {len(sides[lim]['in']):3d} / {len(sides[lim]['out']):3d}   e.g. {sides[lim]['in'][:1]} / {sides[lim]['out'][:1]}")
        print("refusal reasons reached (plain | cut-ring):")
        for why in dict.fromkeys(SC.PLAIN_REASONS + SC.MW_REASONS):
            print(f"  {len(plain.get(why, [])):3d} | {len(mw.get(why, [])):3d}  {why}" + (f"   (not reached: {SC.NOT_REACHED[why]})" if why in SC.NOT_REACHED else ""))
    for lim, s in sides.items():
        assert s["in"] and s["out"], f"limit {lim}: cases only on one side {s}"
    for feat in ("rectangular", "ncols_1", "ncols_odd", "unsorted", "repeated", "empty_rows", "empty_slice", "empty_round", "empty_workgroup",
                 "reach_back", "mw_mesh", "mw_late_narrow", "mw_late_wide", "mw_one_neighbourhood"):
        assert feat in SC.FEATURES, f"no case carries {feat}"
    for why in SC.PLAIN_REASONS:
        assert (why in plain) != (why in SC.NOT_REACHED), f"plain reason {why!r}: reached {plain.get(why)}, listed as not reached: {why in SC.NOT_REACHED}"
    for why in SC.MW_REASONS:
        assert (why in mw) != (why in SC.NOT_REACHED), f"cut-ring reason {why!r}: reached {mw.get(why)}, listed as not reached: {why in SC.NOT_REACHED}"


def _eligible_plain(case):
    n, ncols, p, c = case.data
    R = SC.restate_plan(n, ncols, p, c, 0, case.padding_budget)
    return R if R["eligible"] else None


def test_cases_cover_every_fill_instantiation_past_its_grid():
    """sstream_fill_kernel<2048 | 8192 | 0>: each served by some eligible case, and each with more slices than its grid (the grid-stride
    loop), counted from the row pointers here (not from the plan)."""
    seen = set()
    for case in SC.TABLE:
        if case.expect != "plain":
            continue
        n, _, p, _ = case.data
        ms = SC.max_slice_nnz(n, p)
        cap, grid = SC.fill_instantiation(ms)
        seen.add((cap, 4 * ((n + SC.ROUND - 1) // SC.ROUND) > grid))
    for cap in (2048, 8192, 0):
        assert (cap, True) in seen and (cap, False) in seen, (cap, sorted(seen))


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(m):
    import torch
    return torch.full((m,), float("nan"), dtype=torch.float64, device="cuda")


def _predict(case, shift):
    """('plain' | 'cut-ring' | None, the probe) for the handle that plans at `shift`."""
    n, ncols, p, c = case.data
    P = probe_plain(n, ncols, p, c, shift)
    if P["eligible"]:
        return "plain", P
    M = probe_mw(n, ncols, p, c, shift)
    return ("cut-ring" if M["eligible"] else None), M


def _name_ok(name, form):
    return name.startswith("spmv_sstream<") if form == "plain" else name.startswith("spmv_sstream_mw<")


GUARD = 7


def _gpu_case(case, monkeypatch, forms):
    import torch
    n, ncols, p, c = case.data
    v = SC.values(n + ncols, len(c))
    rng = np.random.default_rng(n * 7 + ncols)
    x = rng.uniform(-1, 1, ncols)
    named = np.zeros(ncols, bool)
    named[c] = True
    x_inf = np.where(named, x, np.inf)
    big = n >= BIG_ROWS
    _padding_env(monkeypatch, case)
    form0, pr0 = _predict(case, 0)
    if form0 is None:  # refused: loud when forced, right bits through another kernel otherwise
        with monkeypatch.context() as m:  # (the forcing variables come back for the next case of a loop)
            m.delenv("MI355_SPMV_KERNEL", raising=False)
            with pytest.raises(mpk.MiError):
                mpk.csrmatrix(n, p, c, v, ncols=ncols).set_kernel("sstream").handle
            m.delenv("MI355_SSTREAM", raising=False)
            A = mpk.csrmatrix(n, p, c, v, ncols=ncols)
            y = _nan(n + GUARD)
            mpk.SpMV_CSR(y[:n], _dev(x), A)
            got = y.cpu().numpy()
            assert not A.kernel_name().startswith("spmv_sstream"), A.kernel_name()
            assert_bit_equal(got[:n], O.spmv(p, c, v, x), f"{case.name} refused, {A.kernel_name()}")
            assert np.isnan(got[n:]).all()
            A.close()
        return
    y_ref = O.spmv(p, c, v, x)
    y_inf = O.spmv(p, c, v, x_inf)
    for f in forms:
        monkeypatch.setenv("MI355_SSTREAM_FORM", str(f))
        A = mpk.csrmatrix(n, p, c, v, ncols=ncols)
        name = A.kernel_name()
        info = A.sstream_info()
        what = f"{case.name} form {f} {name}"
        assert _name_ok(name, form0), what
        assert info["built"] and info["form"] == f, (what, info)
        assert (info["rounds"], info["steps"]) == (pr0["rounds"], pr0["steps"]) and info["padding"] == pr0["padding"], (what, info, pr0)
        y = _nan(n + GUARD)
        mpk.SpMV_CSR(y[:n], _dev(x_inf), A)
        got = y.cpu().numpy()
        assert_bit_equal(got[:n], y_inf, f"{what}: y = A x")
        assert np.isnan(got[n:]).all(), f"{what}: written behind y"
        if big and f != forms[0]:
            continue
        v3 = SC.values(n + ncols + 3, len(c))
        if not big:
            v2 = SC.values(n + ncols + 2, len(c))
            A.update_values(v2)
            y = _nan(n + GUARD)
            mpk.SpMV_CSR(y[:n], _dev(x), A)
            assert_bit_equal(y[:n].cpu().numpy(), O.spmv(p, c, v2, x), f"{what}: after a host refresh")
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            d3 = _dev(v3)
            A.update_values(d3)
        s2.wait_stream(s1)
        with torch.cuda.stream(s2):
            y = _nan(n + GUARD)
            mpk.SpMV_CSR(y[:n], _dev(x), A)
        s2.synchronize()
        y3 = O.spmv(p, c, v3, x)
        assert_bit_equal(y[:n].cpu().numpy(), y3, f"{what}: after a device refresh on another stream")
        assert np.isnan(y[n:].cpu().numpy()).all()
        del d3
        if big:
            continue
        if ncols == n:
            outs = [_nan(n) for _ in range(3)]
            mpk.SpMkV(outs, _dev(x), A)
            Y = O.spmk_chain(3, p, c, v3, x)
            for q in range(3):
                assert_bit_equal(outs[q].cpu().numpy(), Y[q], f"{what}: power {q + 1}")
        # the handle's CSR copy followed the refresh too (the fill writes it on; the stream kernel reads it)
        A.set_kernel("stream")
        y = _nan(n)
        mpk.SpMV_CSR(y, _dev(x), A)
        assert_bit_equal(y.cpu().numpy(), y3, f"{what}: the CSR values after the device refresh")
        A.close()
        if f != forms[0]:
            continue
        # row-mapped handles: a contiguous map with an odd offset (planned one row down) and a scattered one
        for tag, shift, rowmap in (("offset 5", 1, np.arange(n, dtype=np.int32) + 5),
                                   ("scattered", 0, rng.permutation(n + GUARD + 5)[:n].astype(np.int32))):
            fm, prm = _predict(case, shift)
            B = mpk.csrmatrix(n, p, c, v, ncols=ncols, rowmap=rowmap)
            bn = B.kernel_name()
            assert (fm is None and not bn.startswith("spmv_sstream")) or (fm is not None and _name_ok(bn, fm)), (what, tag, fm, bn)
            if fm is not None:
                bi = B.sstream_info()
                assert (bi["rounds"], bi["steps"]) == (prm["rounds"], prm["steps"]), (what, tag, bi, prm)
            y = _nan(n + GUARD + 5)
            mpk.SpMV_CSR(y, _dev(x_inf if fm else x), B)
            got = y.cpu().numpy()
            assert_bit_equal(got[rowmap], y_inf if fm else y_ref, f"{what}: row map {tag} ({bn})")
            rest = np.ones(len(got), bool)
            rest[rowmap] = False
            assert np.isnan(got[rest]).all(), f"{what}: row map {tag}: a row outside the map was written"
            B.close()


@pytest.fixture
def forced(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    mpk.lib()
    monkeypatch.setenv("MI355_SSTREAM", "1")
    monkeypatch.setenv("MI355_SPMV_KERNEL", "sstream")
    return monkeypatch


@pytest.mark.gpu
@pytest.mark.parametrize("case", SC.TABLE, ids=lambda c: c.name)
def test_gpu_table_case(case, forced):
    forms = (0, 3) if case.data[0] >= BIG_ROWS else (0, 1, 2, 3)
    _gpu_case(case, forced, forms)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(8))
def test_gpu_seeded_cases(chunk, forced):
    for q, case in enumerate(SEEDED):
        if q % 8 == chunk:
            _gpu_case(case, forced, (q % 4, (q + 2) % 4))
