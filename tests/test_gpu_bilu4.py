"""mi_bilu4_solve_dev on the GPU against the model's solve (tests/bilu4_model.py), bit for bit (uint64 views): every case of
tests/bilu4_cases.py that factors, for b = ones, x_sin, seeded random and a b of IEEE edge values; in place and out of place, on a
non-default stream, on vectors offset by 8 bytes, two solves back to back, after a refactor; NaN and Inf in b; one larger case."""
import os
import time

import numpy as np
import pytest

import bilu4_cases as C
import bilu4_model as M
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu
FORMS = ("0", None)  # MI355_BILU_FORM: form 0 forced, and the default (the one-launch form is chosen per handle, with mi_bilu4_set_solve_form: asking for it through the environment is refused)


def _rhs(nb):
    from navierstokes_amd import synth
    n = 4 * nb
    rng = np.random.default_rng(nb)
    edge = rng.standard_normal(n)
    specials = [0.0, -0.0, 5e-324, -5e-324, 1e-310, 2.2250738585072014e-308, 1e300, -1e300, 1e-300, -1e-300]
    edge[rng.permutation(n)[: min(n, len(specials))]] = specials[: min(n, len(specials))]
    return {"ones": np.ones(n), "x_sin": synth.x_sin(0, n), "random": rng.standard_normal(n), "edge": edge}


def _model_solve(fac, nb, b):
    ptr, col, diag, val = fac
    sched = (M.schedule(nb, ptr, col, diag, False), M.schedule(nb, ptr, col, diag, True))
    return M.solve(nb, ptr, col, diag, val, b, sched)


def _with_form(form, fn):
    old = os.environ.pop("MI355_BILU_FORM", None)
    if form is not None:
        os.environ["MI355_BILU_FORM"] = form
    try:
        return fn()
    finally:
        os.environ.pop("MI355_BILU_FORM", None)
        if old is not None:
            os.environ["MI355_BILU_FORM"] = old


def _same(got, want, what):
    """Bit-equal where the model is not NaN; NaN exactly where the model is NaN."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN reaches other rows than in the model"
    assert_bit_equal(np.where(nan, 0.0, got), np.where(nan, 0.0, want), what)


@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_solve_bits_equal_the_model(case):
    import torch
    from navierstokes_amd import mpk
    name, fill = case
    nb, bp, bc, bv = C.matrix(name)
    fac = C.model_factor(name, fill)
    if isinstance(fac, M.ZeroPivot):
        with pytest.raises(mpk.MiError):
            mpk.bilu4(nb, bp, bc, bv, fill=fill)
        return
    n = 4 * nb
    rhs = _rhs(nb)
    want = {k: _model_solve(fac, nb, b) for k, b in rhs.items()}
    # the model agrees with itself row by row (no schedule) on the smaller cases: the schedule does not touch the bits
    if len(fac[1]) < 3000:
        assert_bit_equal(M.solve(nb, *fac, rhs["edge"]), want["edge"], "model: natural order vs level order")
    for form in FORMS:
        F = _with_form(form, lambda: mpk.bilu4(nb, bp, bc, bv, fill=fill))
        assert F.info()["form"] == 0
        for k, b in rhs.items():
            db = torch.from_numpy(b).cuda()
            dx = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
            mpk.MatSolve_SeqBAIJ_4(F, db, dx)
            _same(dx.cpu().numpy(), want[k], f"{name} form {form} b={k} out of place")
            assert_bit_equal(db.cpu().numpy(), b, "b was written")
            F.solve(db, db)
            _same(db.cpu().numpy(), want[k], f"{name} form {form} b={k} in place")
        # the host-vector form
        xh = np.full(n, np.nan)
        F.solve(xh, rhs["random"])
        _same(xh, want["random"], f"{name} host vectors")
        # a non-default stream; vectors offset by 8 bytes; two solves back to back without a synchronise between them
        st = torch.cuda.Stream()
        buf_b = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
        buf_x = torch.full((n + 1,), float("nan"), dtype=torch.float64, device="cuda")
        buf_b[1:].copy_(torch.from_numpy(rhs["x_sin"]))
        d1 = torch.from_numpy(rhs["random"]).cuda()
        x1 = torch.empty_like(d1)
        x2 = torch.empty_like(d1)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            F.solve(buf_x[1:], buf_b[1:])
            F.solve(x1, d1)
            F.solve(x2, x1)   # consumes the solve before it: stream order is all that separates them
            F.solve(buf_b[1:], buf_b[1:])
        st.synchronize()
        _same(buf_x[1:].cpu().numpy(), want["x_sin"], f"{name} offset by 8 bytes, other stream")
        _same(buf_b[1:].cpu().numpy(), want["x_sin"], f"{name} offset by 8 bytes, in place")
        _same(x1.cpu().numpy(), want["random"], f"{name} back to back, first")
        _same(x2.cpu().numpy(), _model_solve(fac, nb, want["random"]), f"{name} back to back, second")
        if form is None:
            fac2 = C.model_factor(name, fill, 1)
            if not isinstance(fac2, M.ZeroPivot):
                F.refactor(C.new_values(name, 1))
                dx = torch.empty(n, dtype=torch.float64, device="cuda")
                F.solve(dx, torch.from_numpy(rhs["x_sin"]).cuda())
                _same(dx.cpu().numpy(), _model_solve(fac2, nb, rhs["x_sin"]), f"{name} after refactor")
        F.close()


@pytest.mark.parametrize("name,fill", [("fe:6", 0), ("fe_perm:6", 1), ("arrow", 0), ("chain", 0), ("random:7", 1)])
def test_nan_and_inf_reach_the_rows_the_model_says(name, fill):
    import torch
    from navierstokes_amd import mpk
    nb, bp, bc, bv = C.matrix(name)
    fac = C.model_factor(name, fill)
    n = 4 * nb
    F = mpk.bilu4(nb, bp, bc, bv, fill=fill)
    for at, bad in ((n // 2, np.nan), (n // 3, np.inf), (n - 1, -np.inf), (0, np.nan)):
        b = np.random.default_rng(at).standard_normal(n)
        b[at] = bad
        want = _model_solve(fac, nb, b)
        dx = torch.empty(n, dtype=torch.float64, device="cuda")
        F.solve(dx, torch.from_numpy(b).cuda())
        got = dx.cpu().numpy()
        _same(got, want, f"{name} {bad} at {at}")
        assert not np.isfinite(got).all(), "the special value vanished"
    F.close()


def test_asking_for_the_form_that_is_not_built_is_refused():
    from navierstokes_amd import mpk
    nb, bp, bc, bv = C.matrix("chain")
    with pytest.raises(mpk.MiError) as e:
        _with_form("1", lambda: mpk.bilu4(nb, bp, bc, bv))
    assert e.value.status == 5 and "not built" in str(e.value)
    with pytest.raises(mpk.MiError):
        _with_form("2", lambda: mpk.bilu4(nb, bp, bc, bv))


def test_larger_case_fe24():
    """fe_matrix(24): 15 625 block rows (62 500 rows), 73 levels.  The factor VALUES are read back from the handle
    (mi_bilu4_factor_host; tests/test_bilu4_factor.py pins them to the model on the smaller cases — the model's own factorisation
    of this size takes minutes); pattern, schedule and solve are the model's, numpy per level.  Model run time: printed."""
    import torch
    from navierstokes_amd import mpk, synth
    bp, bc, bv = synth.csr_to_bcsr4(*synth.fe_matrix(24))
    nb = len(bp) - 1
    F = mpk.bilu4(nb, bp, bc, bv, fill=0)
    info = F.info()
    assert nb == 15625 and info["fwd_levels"] == 73 and info["bwd_levels"] == 73
    ptr, col, diag, val = F.factor_host()
    t0 = time.time()
    mp, mc, md = M.symbolic(nb, bp, bc, 0)
    assert np.array_equal(ptr, mp) and np.array_equal(col, mc) and np.array_equal(diag, md)
    b = synth.x_sin(0, 4 * nb) + 1.0
    want = _model_solve((mp, mc, md, val), nb, b)
    print(f"model (symbolic + schedule + solve) of fe_matrix(24): {time.time() - t0:.1f} s; launches per solve {info['launches']}, "
          f"{info['us_per_level_launches']:.1f} us per solve at create")
    dx = torch.empty(4 * nb, dtype=torch.float64, device="cuda")
    F.solve(dx, torch.from_numpy(b).cuda())
    assert_bit_equal(dx.cpu().numpy(), want, "fe_matrix(24)")
    F.close()
