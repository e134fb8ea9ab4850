"""The sweep solve of the block ILU (mi_bilu4sw_*, mpk.bilu4.sweeps) on the GPU, bit for bit (uint64 views) against the model
of tests/bilu4_sweeps_model.py, on the shapes where this kernel can go wrong:

  edges      wide:63/64/65 (rows without off-diagonal blocks at the edge of a workgroup); limits:0 (782 rows, 13 workgroups, mixed
             row lengths); arrow (one row of 79 blocks: every clamp of the pipeline); chain, diag
  meshes     fe:6, fe_perm:6 at fill 0 and 1, fe:10 at fill 0;  random:0..29 (1 to 39 block rows, rows of a single block)
  counts     (0,0), (1,1), (3,2), (2,5) and the clamped (10^6, 10^6), which must also equal mi_bilu4_solve_dev on the same handle
             and report launches_last = max_fwd + 1 + max_bwd
  vectors    x == b; b and x offset by one double; a non-default stream; solves with different counts back to back (stale work vectors)
  capture    after prepare, replayed twice with a changed b; refused on an unprepared handle
  refactor   after mi_bilu4dev_refactor with other values the sweeps are the model's on that factor
  specials   one NaN and one Inf in b reach exactly the rows the model says
  gmres      mpk.GMRES with M = F.sweeps(4) against tests/gmres_model.py with the dense sweep operator
"""
import numpy as np
import pytest

import bilu4_cases as C
import bilu4_model as M
import bilu4_sweeps_model as S
import gmres_model as G
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

COUNTS = [(0, 0), (1, 1), (3, 2), (2, 5), (10 ** 6, 10 ** 6)]
CASES = ([("wide:63", 0), ("wide:64", 0), ("wide:65", 0), ("limits:0", 0), ("arrow", 0), ("chain", 0), ("diag", 0), ("fe:6", 0), ("fe:6", 1),
          ("fe_perm:6", 0), ("fe_perm:6", 1), ("fe:10", 0)] + [(f"random:{s}", s % 3) for s in range(30)])


def _same(got, want, what):
    """Bit-equal where the model is not NaN; NaN exactly where the model is NaN."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN reaches other rows than in the model"
    assert_bit_equal(np.where(nan, 0.0, got), np.where(nan, 0.0, want), what)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _poisoned(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("name,fill", CASES, ids=[C.case_id(c) for c in CASES])
def test_sweeps_are_the_model_bit_for_bit(name, fill):
    import torch
    from navierstokes_amd import mpk
    nb, bp, bc, bv = C.matrix(name)
    fac = C.model_factor(name, fill)
    if isinstance(fac, M.ZeroPivot):
        pytest.fail(f"{name} fill {fill} does not factor: not a case for the solve")
    n = 4 * nb
    rng = np.random.default_rng(nb + 7 * fill)
    b, b2 = rng.standard_normal(n), rng.standard_normal(n)
    want = {c: S.solve_sweeps(nb, *fac, b, *c) for c in COUNTS}
    F = mpk.bilu4(nb, bp, bc, bv, fill=fill)
    mf, mb = S.max_sweeps(nb, *fac[:3])
    assert F.sweep_info() == dict(prepared=False, max_fwd=mf, max_bwd=mb, launches_last=0, work_bytes=0)
    db = _dev(b)
    try:
        for c in COUNTS:
            dx = _poisoned(n)
            F.sweeps(*c).solve(dx, db)  # (the first one prepares)
            _same(dx.cpu().numpy(), want[c], f"{name} fill {fill} sweeps {c}")
            info = F.sweep_info()
            assert info["prepared"] and info["work_bytes"] == 3 * 8 * n
            assert info["launches_last"] == min(c[0], mf) + 1 + min(c[1], mb), (c, info)
            assert_bit_equal(db.cpu().numpy(), b, "b was written")
            inplace = db.clone()
            F.sweeps(*c).solve(inplace, inplace)
            _same(inplace.cpu().numpy(), want[c], f"{name} fill {fill} sweeps {c}, x == b")
        # the clamped count is the exact solve, by the handle's own level-by-level form too
        dx = _poisoned(n)
        F.solve(dx, db)
        _same(dx.cpu().numpy(), want[COUNTS[-1]], f"{name} fill {fill}: mi_bilu4_solve_dev against the clamped sweeps")
        assert F.sweep_info()["launches_last"] == mf + 1 + mb
        # offset by one double, on another stream, different counts back to back: each consumes the one before
        st = torch.cuda.Stream()
        buf_b, buf_x = torch.zeros(n + 1, dtype=torch.float64, device="cuda"), _poisoned(n + 1)
        buf_b[1:].copy_(db)
        d2 = _dev(b2)
        x1, x2, x3 = _poisoned(n), _poisoned(n), _poisoned(n)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            F.sweeps(3, 2).solve(buf_x[1:], buf_b[1:])
            F.sweeps(2, 5).solve(x1, d2)
            F.sweeps(0, 0).solve(x2, x1)
            F.sweeps(1, 3).solve(x3, x2)
            F.sweeps(2, 5).solve(buf_b[1:], buf_b[1:])
        st.synchronize()
        _same(buf_x[1:].cpu().numpy(), want[(3, 2)], f"{name} fill {fill} offset by 8 bytes, other stream")
        _same(buf_b[1:].cpu().numpy(), want[(2, 5)], f"{name} fill {fill} offset by 8 bytes, in place")
        w1 = S.solve_sweeps(nb, *fac, b2, 2, 5)
        w2 = S.solve_sweeps(nb, *fac, w1, 0, 0)
        _same(x1.cpu().numpy(), w1, f"{name} fill {fill} back to back, first")
        _same(x2.cpu().numpy(), w2, f"{name} fill {fill} back to back, second")
        _same(x3.cpu().numpy(), S.solve_sweeps(nb, *fac, w2, 1, 3), f"{name} fill {fill} back to back, third")
        # host vectors
        hx = np.full(n, np.nan)
        F.sweeps(3, 2).solve(hx, b)
        _same(hx, want[(3, 2)], f"{name} fill {fill} host vectors")
    finally:
        F.close()


def test_the_sweep_solve_does_not_depend_on_the_solve_form():
    from navierstokes_amd import mpk
    name = "fe:6"
    nb, bp, bc, bv = C.matrix(name)
    fac = C.model_factor(name, 0)
    b = np.random.default_rng(5).standard_normal(4 * nb)
    want = S.solve_sweeps(nb, *fac, b, 3, 2)
    F = mpk.bilu4(nb, bp, bc, bv, fill=0)
    assert F.set_form(1) == 1
    dx = _poisoned(4 * nb)
    F.sweeps(3, 2).solve(dx, _dev(b))
    _same(dx.cpu().numpy(), want, "sweeps on a handle in form 1")
    assert F.info()["form"] == 1
    F.one_status()
    F.close()


def test_capture_after_prepare_and_replay():
    import torch
    from navierstokes_amd import mpk
    name = "limits:0"
    nb, bp, bc, bv = C.matrix(name)
    fac = C.model_factor(name, 0)
    n = 4 * nb
    rng = np.random.default_rng(11)
    F = mpk.bilu4(nb, bp, bc, bv, fill=0).prepare_sweeps()
    assert F.sweep_info()["prepared"] and F.prepare_sweeps().sweep_info()["prepared"]
    db, dx = _dev(rng.standard_normal(n)), _poisoned(n)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        F.sweeps(3, 2).solve(dx, db)
    for k in range(2):
        b = rng.standard_normal(n)
        db.copy_(_dev(b))
        dx.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        _same(dx.cpu().numpy(), S.solve_sweeps(nb, *fac, b, 3, 2), f"replay {k}")
    F.close()


def test_capture_on_an_unprepared_handle_is_refused():
    import torch
    from navierstokes_amd import mpk
    name = "random:12"
    nb, bp, bc, bv = C.matrix(name)
    fac = C.model_factor(name, 0)
    n = 4 * nb
    b = np.random.default_rng(12).standard_normal(n)
    F = mpk.bilu4(nb, bp, bc, bv, fill=0)
    db, dx = _dev(b), _poisoned(n)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dx.fill_(1.0)  # (so that the graph is not empty)
        with pytest.raises(mpk.MiError) as e:
            F.sweeps(1).solve(dx, db)
    assert e.value.status == 6 and "not prepared" in str(e.value)
    assert F.sweep_info()["prepared"] is False
    F.sweeps(1).solve(dx, db)  # outside the capture the same call prepares and solves
    _same(dx.cpu().numpy(), S.solve_sweeps(nb, *fac, b, 1, 1), "after the refused capture")
    F.close()


REFACTOR_CASES = [("fe:6", 0), ("arrow", 0), ("random:7", 1)]


@pytest.mark.parametrize("name,fill", REFACTOR_CASES, ids=[C.case_id(c) for c in REFACTOR_CASES])
def test_sweeps_read_the_values_a_device_refactor_wrote(name, fill):
    import torch
    from navierstokes_amd import mpk
    nb, bp, bc, bv = C.matrix(name)
    fac_new = C.model_factor(name, fill, 1)
    assert not isinstance(fac_new, M.ZeroPivot)
    n = 4 * nb
    b = np.random.default_rng(21).standard_normal(n)
    F = mpk.bilu4(nb, bp, bc, bv, fill=fill)
    db, dx = _dev(b), _poisoned(n)
    F.sweeps(2, 2).solve(dx, db)
    _same(dx.cpu().numpy(), S.solve_sweeps(nb, *C.model_factor(name, fill), b, 2, 2), f"{name} before the refactor")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        F.refactor_dev(_dev(C.new_values(name, 1)))
        F.sweeps(2, 2).solve(dx, db)
    st.synchronize()
    F.factor_status()
    _same(dx.cpu().numpy(), S.solve_sweeps(nb, *fac_new, b, 2, 2), f"{name} after refactor_dev")
    F.refactor(np.asarray(bv))
    F.sweeps(1, 3).solve(dx, db)
    _same(dx.cpu().numpy(), S.solve_sweeps(nb, *C.model_factor(name, fill), b, 1, 3), f"{name} after the host refactor back")
    F.close()


@pytest.mark.parametrize("name", ["fe:6", "arrow"])
def test_nan_and_inf_reach_the_rows_the_model_says(name):
    from navierstokes_amd import mpk
    nb, bp, bc, bv = C.matrix(name)
    fac = C.model_factor(name, 0)
    n = 4 * nb
    F = mpk.bilu4(nb, bp, bc, bv, fill=0)
    for at_nan, at_inf in ((n // 2, n // 3), (0, n - 1), (n - 1, 1)):
        b = np.random.default_rng(at_nan).standard_normal(n)
        b[at_nan], b[at_inf] = np.nan, np.inf
        dx = _poisoned(n)
        F.sweeps(2, 2).solve(dx, _dev(b))
        got = dx.cpu().numpy()
        want = S.solve_sweeps(nb, *fac, b, 2, 2)
        _same(got, want, f"{name}: NaN at {at_nan}, Inf at {at_inf}")
        assert not np.isfinite(got).all(), "the special values vanished"
        if name == "fe:6":
            assert np.isfinite(got).any(), "two sweeps per triangle cannot have carried them everywhere on this mesh"
    F.close()


RTOL = 1e-8
FLOOR = 1e-10
# The reference's own spread on these cases, as tests/test_gpu_gmres.py derives its HISTORY_BOUND: the history of gmres_model.gmres
# in float64 against its history with the Arnoldi vectors, products and dots in numpy.longdouble, Minv = dense_operator(.., 4, 4),
# restart 30, entries above FLOOR: largest relative difference 4.03e-15 on fe:6 (18 iterations) and 6.88e-15 on fe:10 (24) — four
# orders below that file's figure: these runs are one short cycle of a well-conditioned preconditioned operator.  Ten times the larger:
HISTORY_BOUND = 6.9e-14


@pytest.mark.parametrize("name", ["fe:6", "fe:10"])
def test_gmres_with_four_sweeps_follows_the_dense_reference(name):
    import torch
    from navierstokes_amd import mpk
    A, _, b = G.problem(name, None)
    nb, bp, bc, bv = C.matrix(name)
    Msw = S.dense_operator(nb, C.model_factor(name, 0), 4, 4)
    rits, rhist, _ = G.gmres(A, b, np.zeros_like(b), Msw, restart=30, rtol=RTOL, maxiter=300)
    Ad = mpk.bcsr4x4_matrix(nb, bp, bc, bv)
    F = mpk.bilu4(nb, bp, bc, bv, fill=0)
    dx = torch.zeros(4 * nb, dtype=torch.float64, device="cuda")
    its, hist = mpk.GMRES(Ad, _dev(b), dx, M=F.sweeps(4), restart=30, rtol=RTOL, maxiter=300)
    x = dx.cpu().numpy()
    assert F.sweep_info()["launches_last"] == 9
    F.close()
    Ad.close()
    # the method of tests/test_gpu_gmres.py::_compare
    assert len(hist) == its + 1
    worst = max(abs(hist[k] - rhist[k]) / rhist[k] for k in range(min(len(hist), len(rhist))) if rhist[k] > FLOOR)
    true = G.true_residual(A, x, b)
    print(f"{name} with 4 sweeps: {its} iterations (reference {rits}), largest relative difference of the history {worst:.3e}, last {hist[-1]:.3e}, true {true:.3e}")
    assert worst <= HISTORY_BOUND, worst
    near = RTOL / 2 <= rhist[-1] <= 2 * RTOL
    assert its == rits or (near and abs(its - rits) == 1), (its, rits, rhist[-1])
    assert hist[-1] <= RTOL and true <= 10 * RTOL, (hist[-1], true)
