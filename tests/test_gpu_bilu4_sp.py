"""The sweeps over the single-precision copy of the block ILU factor (mi_bilu4sp_*, mpk.bilu4.sweeps(.., precision="f32")) on the
GPU, bit for bit (uint32 / uint64 views) against tests/bilu4_sp_model.py:

  conversion  fetch_f32() is round_factor(model factor) on sp_edges (ties, subnormals, -0: tests/bilu4_sp_cases.py), fe:6 at fill 0
              and 1, arrow, limits:0, random:0..9 — after prepare, after refactor(host values) and after refactor_dev on another
              stream; sweep_status_f32() passes on all of them and names block row 0 and two values on sp_overflow, whose copy and
              solves are still the model's, Inf included
  solve       the cases, counts and vector variations of tests/test_gpu_bilu4_sweeps.py (and sp_edges) against solve_sweeps_sp
  both        f64, f32, f64 back to back on one handle; sweep_info() and the exact solve untouched by a prepared copy
  capture     a graph of refactor_dev + an f32 sweep solve, replayed twice with other values and another b; refused when unprepared
  specials    one NaN and one Inf in b reach exactly the model's rows
  gmres       mpk.GMRES with M = F.sweeps(4, precision="f32") against gmres_model.gmres with the dense operator of the ROUNDED factor
"""
import numpy as np
import pytest

import bilu4_cases as C
import bilu4_model as M
import bilu4_sp_cases as SC
import bilu4_sp_model as SP
import bilu4_sweeps_model as S
import gmres_model as G
import test_gpu_bilu4_sweeps as T
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

COUNTS = T.COUNTS
SOLVE_CASES = T.CASES + [("sp_edges", 0)]
CONVERT_CASES = [("sp_edges", 0), ("fe:6", 0), ("fe:6", 1), ("arrow", 0), ("limits:0", 0)] + [(f"random:{s}", s % 3) for s in range(10)]
_same, _dev, _poisoned = T._same, T._dev, T._poisoned


def _factor(name, fill, variant=0):
    fac = SC.model_factor(name, fill, variant)
    assert not isinstance(fac, M.ZeroPivot), f"{name} fill {fill} variant {variant} does not factor: not a case here"
    return fac


def _copy_is(F, fac, what):
    got, want = F.fetch_f32(), SP.round_factor(fac[3])
    assert got.dtype == np.float32 and got.shape == want.shape, (got.shape, want.shape)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad[0]) == 0, f"{what}: {len(bad[0])} of {want.size} values differ, first at block {bad[0][0]}: {got[bad][0]!r} against {want[bad][0]!r}"


@pytest.mark.parametrize("name,fill", CONVERT_CASES, ids=[C.case_id(c) for c in CONVERT_CASES])
def test_the_copy_is_the_rounded_factor_after_every_write(name, fill):
    import torch
    from navierstokes_amd import mpk
    nb, bp, bc, bv = SC.matrix(name)
    fac, fac_new = _factor(name, fill), _factor(name, fill, 1)
    F = mpk.bilu4(nb, bp, bc, bv, fill=fill)
    try:
        assert F.sweep_info_f32() == dict(prepared=False, convert_launches=0, launches_last=0, copy_bytes=0)
        F.sweep_status_f32()  # (no copy yet: nothing to report)
        F.prepare_sweeps(precision="f32")
        assert F.sweep_info_f32() == dict(prepared=True, convert_launches=1, launches_last=0, copy_bytes=64 * len(fac[1]))
        assert F.prepare_sweeps(precision="f32").sweep_info_f32()["convert_launches"] == 1, "prepare is idempotent"
        _copy_is(F, fac, f"{name} fill {fill} after prepare")
        F.sweep_status_f32()
        F.refactor(SC.new_values(name, 1))
        _copy_is(F, fac_new, f"{name} fill {fill} after refactor(host values)")
        F.sweep_status_f32()
        dcoef = _dev(bv)
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            F.refactor_dev(dcoef)
        st.synchronize()
        F.factor_status()
        _copy_is(F, fac, f"{name} fill {fill} after refactor_dev on another stream")
        F.sweep_status_f32()
        assert F.sweep_info_f32()["convert_launches"] == 3
    finally:
        F.close()


def test_an_overflow_is_reported_and_the_copy_and_solves_are_still_the_models():
    from navierstokes_amd import mpk
    name = "sp_overflow"
    nb, bp, bc, bv = SC.matrix(name)
    fac = _factor(name, 0)
    n = 4 * nb
    F = mpk.bilu4(nb, bp, bc, bv, fill=0).prepare_sweeps(precision="f32")
    try:
        with pytest.raises(mpk.MiError) as e:
            F.sweep_status_f32()
        assert e.value.status == 1 and "block row 0" in str(e.value), str(e.value)
        assert (e.value.bad_block_row, e.value.overflowed) == (0, 2) == SP.overflowed(fac[3], fac[0])[::-1]
        _copy_is(F, fac, name)
        assert np.isinf(F.fetch_f32()).sum() == 2
        b = np.random.default_rng(3).standard_normal(n)
        for c in ((2, 2), (10 ** 6, 10 ** 6)):
            dx = _poisoned(n)
            F.sweeps(*c, precision="f32").solve(dx, _dev(b))
            got = dx.cpu().numpy()
            _same(got, SP.solve_sweeps_sp(nb, *fac, b, *c), f"{name} sweeps {c}")
            assert not np.isfinite(got[:4]).all() and np.isfinite(got[4:]).all()
        # the double sweeps and the exact solve never read the copy
        dx = _poisoned(n)
        F.sweeps(2, 2).solve(dx, _dev(b))
        _same(dx.cpu().numpy(), S.solve_sweeps(nb, *fac, b, 2, 2), f"{name}: double sweeps")
        # halved by a refactor, one of the two is back inside the range of float
        F.refactor(SC.new_values(name, 1))
        with pytest.raises(mpk.MiError) as e:
            F.sweep_status_f32()
        assert (e.value.bad_block_row, e.value.overflowed) == (0, 1)
        _copy_is(F, _factor(name, 0, 1), f"{name} halved")
    finally:
        F.close()


@pytest.mark.parametrize("name,fill", SOLVE_CASES, ids=[C.case_id(c) for c in SOLVE_CASES])
def test_f32_sweeps_are_the_model_bit_for_bit(name, fill):
    import torch
    from navierstokes_amd import mpk
    nb, bp, bc, bv = SC.matrix(name)
    fac = _factor(name, fill)
    n = 4 * nb
    rng = np.random.default_rng(nb + 7 * fill)
    b, b2 = rng.standard_normal(n), rng.standard_normal(n)
    want = {c: SP.solve_sweeps_sp(nb, *fac, b, *c) for c in COUNTS}
    F = mpk.bilu4(nb, bp, bc, bv, fill=fill)
    mf, mb = S.max_sweeps(nb, *fac[:3])
    db = _dev(b)
    sp = lambda sf, sb: F.sweeps(sf, sb, precision="f32")
    try:
        for c in COUNTS:
            dx = _poisoned(n)
            sp(*c).solve(dx, db)  # (the first one prepares)
            _same(dx.cpu().numpy(), want[c], f"{name} fill {fill} f32 sweeps {c}")
            info = F.sweep_info_f32()
            assert info["prepared"] and info["convert_launches"] == 1 and info["copy_bytes"] == 64 * len(fac[1])
            assert info["launches_last"] == min(c[0], mf) + 1 + min(c[1], mb), (c, info)
            assert F.sweep_info()["launches_last"] == 0, "mi_bilu4sw_info reports the double sweeps only"
            assert_bit_equal(db.cpu().numpy(), b, "b was written")
            inplace = db.clone()
            sp(*c).solve(inplace, inplace)
            _same(inplace.cpu().numpy(), want[c], f"{name} fill {fill} f32 sweeps {c}, x == b")
        # offset by one double, on another stream, different counts back to back: each consumes the one before
        st = torch.cuda.Stream()
        buf_b, buf_x = torch.zeros(n + 1, dtype=torch.float64, device="cuda"), _poisoned(n + 1)
        buf_b[1:].copy_(db)
        d2 = _dev(b2)
        x1, x2, x3 = _poisoned(n), _poisoned(n), _poisoned(n)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            sp(3, 2).solve(buf_x[1:], buf_b[1:])
            sp(2, 5).solve(x1, d2)
            sp(0, 0).solve(x2, x1)
            sp(1, 3).solve(x3, x2)
            sp(2, 5).solve(buf_b[1:], buf_b[1:])
        st.synchronize()
        _same(buf_x[1:].cpu().numpy(), want[(3, 2)], f"{name} fill {fill} offset by 8 bytes, other stream")
        _same(buf_b[1:].cpu().numpy(), want[(2, 5)], f"{name} fill {fill} offset by 8 bytes, in place")
        w1 = SP.solve_sweeps_sp(nb, *fac, b2, 2, 5)
        w2 = SP.solve_sweeps_sp(nb, *fac, w1, 0, 0)
        _same(x1.cpu().numpy(), w1, f"{name} fill {fill} back to back, first")
        _same(x2.cpu().numpy(), w2, f"{name} fill {fill} back to back, second")
        _same(x3.cpu().numpy(), SP.solve_sweeps_sp(nb, *fac, w2, 1, 3), f"{name} fill {fill} back to back, third")
        # host vectors
        hx = np.full(n, np.nan)
        sp(3, 2).solve(hx, b)
        _same(hx, want[(3, 2)], f"{name} fill {fill} host vectors")
        F.sweep_status_f32()
    finally:
        F.close()


BOTH_CASES = [("fe:6", 0), ("limits:0", 0), ("sp_edges", 0)]


@pytest.mark.parametrize("name,fill", BOTH_CASES, ids=[C.case_id(c) for c in BOTH_CASES])
def test_both_precisions_share_one_handle(name, fill):
    from navierstokes_amd import mpk
    nb, bp, bc, bv = SC.matrix(name)
    fac = _factor(name, fill)
    ptr, col, diag, val = fac
    n = 4 * nb
    b = np.random.default_rng(41).standard_normal(n)
    mf, mb = S.max_sweeps(nb, ptr, col, diag)
    F = mpk.bilu4(nb, bp, bc, bv, fill=fill).prepare_sweeps(precision="f32")
    try:
        assert F.sweep_info() == dict(prepared=True, max_fwd=mf, max_bwd=mb, launches_last=0, work_bytes=3 * 8 * n)
        db = _dev(b)
        for prec, c in (("f64", (3, 2)), ("f32", (2, 4)), ("f64", (1, 3))):
            dx = _poisoned(n)
            F.sweeps(*c, precision=prec).solve(dx, db)
            model = SP.solve_sweeps_sp if prec == "f32" else S.solve_sweeps
            _same(dx.cpu().numpy(), model(nb, *fac, b, *c), f"{name}: {prec} sweeps {c}")
        assert F.sweep_info() == dict(prepared=True, max_fwd=mf, max_bwd=mb, launches_last=min(1, mf) + 1 + min(3, mb), work_bytes=3 * 8 * n)
        assert F.sweep_info_f32()["launches_last"] == min(2, mf) + 1 + min(4, mb)
        # the two differ (the copy is read by the f32 sweeps and by nothing else)
        assert not np.array_equal(SP.solve_sweeps_sp(nb, *fac, b, 2, 4), S.solve_sweeps(nb, *fac, b, 2, 4))
        dx = _poisoned(n)
        F.solve(dx, db)
        sched = (M.schedule(nb, ptr, col, diag, False), M.schedule(nb, ptr, col, diag, True))
        _same(dx.cpu().numpy(), M.solve(nb, ptr, col, diag, val, b, sched), f"{name}: the exact solve beside a prepared copy")
    finally:
        F.close()


def test_a_captured_refactor_carries_the_conversion():
    import torch
    from navierstokes_amd import mpk
    name = "limits:0"
    nb, bp, bc, bv = SC.matrix(name)
    n = 4 * nb
    rng = np.random.default_rng(11)
    F = mpk.bilu4(nb, bp, bc, bv, fill=0).prepare_dev().prepare_sweeps(precision="f32")
    dcoef, db, dx = _dev(bv), _dev(rng.standard_normal(n)), _poisoned(n)
    F.refactor_dev(dcoef)  # (warm: everything the capture needs exists)
    torch.cuda.synchronize()
    before = F.sweep_info_f32()["convert_launches"]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        F.refactor_dev(dcoef)
        F.sweeps(3, 2, precision="f32").solve(dx, db)
    assert F.sweep_info_f32()["convert_launches"] == before + 1
    try:
        for k, variant in enumerate((1, 0)):
            b = rng.standard_normal(n)
            db.copy_(_dev(b))
            dcoef.copy_(_dev(SC.new_values(name, variant) if variant else bv))
            dx.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            fac = _factor(name, 0, variant)
            _same(dx.cpu().numpy(), SP.solve_sweeps_sp(nb, *fac, b, 3, 2), f"replay {k}")
            _copy_is(F, fac, f"the copy after replay {k}")
            F.factor_status().sweep_status_f32()
    finally:
        F.close()


def test_capture_on_a_handle_not_prepared_for_f32_is_refused():
    import torch
    from navierstokes_amd import mpk
    name = "random:12"
    nb, bp, bc, bv = SC.matrix(name)
    fac = _factor(name, 0)
    n = 4 * nb
    b = np.random.default_rng(12).standard_normal(n)
    F = mpk.bilu4(nb, bp, bc, bv, fill=0).prepare_sweeps()  # for the double sweeps only
    db, dx = _dev(b), _poisoned(n)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dx.fill_(1.0)  # (so that the graph is not empty)
        with pytest.raises(mpk.MiError) as e:
            F.sweeps(1, precision="f32").solve(dx, db)
    assert e.value.status == 6 and "not prepared" in str(e.value)
    assert F.sweep_info_f32()["prepared"] is False
    F.sweeps(1, precision="f32").solve(dx, db)  # outside the capture the same call prepares and solves
    _same(dx.cpu().numpy(), SP.solve_sweeps_sp(nb, *fac, b, 1, 1), "after the refused capture")
    assert F.sweep_info_f32()["prepared"] is True
    F.close()


@pytest.mark.parametrize("name", ["fe:6", "arrow"])
def test_nan_and_inf_reach_the_rows_the_model_says(name):
    from navierstokes_amd import mpk
    nb, bp, bc, bv = SC.matrix(name)
    fac = _factor(name, 0)
    n = 4 * nb
    F = mpk.bilu4(nb, bp, bc, bv, fill=0)
    for at_nan, at_inf in ((n // 2, n // 3), (0, n - 1), (n - 1, 1)):
        b = np.random.default_rng(at_nan).standard_normal(n)
        b[at_nan], b[at_inf] = np.nan, np.inf
        dx = _poisoned(n)
        F.sweeps(2, 2, precision="f32").solve(dx, _dev(b))
        got = dx.cpu().numpy()
        _same(got, SP.solve_sweeps_sp(nb, *fac, b, 2, 2), f"{name}: NaN at {at_nan}, Inf at {at_inf}")
        assert not np.isfinite(got).all(), "the special values vanished"
        if name == "fe:6":
            assert np.isfinite(got).any(), "two sweeps per triangle cannot have carried them everywhere on this mesh"
    F.close()


RTOL = 1e-8
FLOOR = 1e-10
# The reference's own spread on these two cases with the ROUNDED operator, derived as tests/test_gpu_bilu4_sweeps.py derives its
# HISTORY_BOUND (not copied from it): the history of gmres_model.gmres in float64 against its history with wide=True (Arnoldi
# vectors, products and dots in numpy.longdouble), Minv = dense_operator(rounded factor, 4, 4), restart 30, entries above FLOOR:
# largest relative difference 1.068e-14 on fe:6 (18 iterations) and 6.70e-15 on fe:10 (24).  Ten times the larger:
HISTORY_BOUND = 1.068e-13


@pytest.mark.parametrize("name", ["fe:6", "fe:10"])
def test_gmres_with_four_f32_sweeps_follows_the_dense_reference_of_the_rounded_factor(name):
    import torch
    from navierstokes_amd import mpk
    A, _, b = G.problem(name, None)
    nb, bp, bc, bv = C.matrix(name)
    Msw = S.dense_operator(nb, SP.rounded(C.model_factor(name, 0)), 4, 4)
    rits, rhist, _ = G.gmres(A, b, np.zeros_like(b), Msw, restart=30, rtol=RTOL, maxiter=300)
    Ad = mpk.bcsr4x4_matrix(nb, bp, bc, bv)
    F = mpk.bilu4(nb, bp, bc, bv, fill=0)
    dx = torch.zeros(4 * nb, dtype=torch.float64, device="cuda")
    its, hist = mpk.GMRES(Ad, _dev(b), dx, M=F.sweeps(4, precision="f32"), restart=30, rtol=RTOL, maxiter=300)
    x = dx.cpu().numpy()
    assert F.sweep_info_f32()["launches_last"] == 9 and F.sweep_info()["launches_last"] == 0
    F.close()
    Ad.close()
    # the method of tests/test_gpu_gmres.py::_compare
    assert len(hist) == its + 1
    worst = max(abs(hist[k] - rhist[k]) / rhist[k] for k in range(min(len(hist), len(rhist))) if rhist[k] > FLOOR)
    true = G.true_residual(A, x, b)
    print(f"{name} with 4 f32 sweeps: {its} iterations (reference {rits}), largest relative difference of the history {worst:.3e}, last {hist[-1]:.3e}, true {true:.3e}")
    assert worst <= HISTORY_BOUND, worst
    near = RTOL / 2 <= rhist[-1] <= 2 * RTOL
    assert its == rits or (near and abs(its - rits) == 1), (its, rits, rhist[-1])
    assert hist[-1] <= RTOL and true <= 10 * RTOL, (hist[-1], true)
