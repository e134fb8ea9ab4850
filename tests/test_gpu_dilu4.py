"""mi_dilu4_* (mpk.dilu4) on the GPU: the three sweeps of the block DILU preconditioner applied with Eisenstat's trick, BIT for bit
against tests/dilu4_model.py, and GMRES on the split-preconditioned operator against the loops composed from public pieces.

  sweeps     to_hat, from_hat and apply_hat on fe:6 in colour order (backward every level is narrower than 64 rows: one folded
             launch; forward levels of 64, 67, 49, 64, 42, .. rows: mixed), fe:10 in colour order (levels of 78 to 254 rows: every
             launch the pipelined level kernel), fe:6 in natural order (each sweep ONE folded launch of 19 levels), fe:10 in natural
             order (folded and unfolded launches mixed), limits:0 (levels of exactly 63, 64 and 65 rows), diag (no L and no U block
             anywhere), arrow and the
             unsymmetric pattern; each with outputs pre-filled with NaN, in place, and on a non-default stream with vectors offset
             by one double (8-byte aligned only)
  graph      the three operations captured into one graph and replayed on other inputs
  refactor   after refactor with other values
  nonfinite  one Inf and one NaN in the input land on the entries the model says
  gmres      the solver with a dilu4 operator against tests/test_gpu_gmres_dev.py::composed with apply_hat as the product: eager for
             check_every 1 and 4, the float basis (tests/test_gpu_gmres_f32.py::composed_f32), one captured cycle, a plan; the
             argument rules of mi_gmres_set_operator_dilu4
  residual   dilu4.gmres (r = b - A x0, to_hat, the solve in the hat variables, from_hat) leaves a true relative residual against the
             dense matrix within ten times rtol, the margin of test_gpu_gmres_dev.py's dense-reference test"""
import functools

import numpy as np
import pytest

import bilu4_cases as C
import bilu4_order_cases as OC
import dilu4_model as DM
import gmres_model as G
import test_gpu_gmres_dev as T
import test_gpu_gmres_f32 as T32
import test_gpu_gmres_plan as TP
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

MI_ERR_ARG, MI_ERR_STATE = 1, 6
RTOL = 1e-8
OPS = ("to_hat", "from_hat", "apply_hat")
SWEEP_CASES = [("fe:6", "colour"), ("fe:10", "colour"), ("fe:6", "natural"), ("fe:10", "natural"), ("limits:0", "natural"),
               ("limits:0", "colour"), ("diag", "natural"), ("arrow", "colour"), ("arrow", "natural"), ("unsym", "colour")]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()  # (a copy: the shared expectations are read-only)


def _poisoned(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def _vector(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)


@functools.lru_cache(maxsize=None)
def model(name, order, variant=0):
    nb, bp, bc, _ = OC.matrix(name)
    return DM.Ordered(nb, bp, bc, OC.values(name, variant), order)


@functools.lru_cache(maxsize=None)
def expected(name, order, variant=0, seed=0):
    """(u, {op: the model's result}) — computed once, read-only."""
    m = model(name, order, variant)
    u = _vector(4 * m.nb, 100 + seed)
    out = {op: getattr(m, op)(u) for op in OPS}
    for v in (u, *out.values()):
        v.setflags(write=False)
    return u, out


def _handle(name, order, variant=0):
    from navierstokes_amd import mpk
    nb, bp, bc, _ = OC.matrix(name)
    return mpk.dilu4(nb, bp, bc, OC.values(name, variant), order=order)


# ---------------------------------------------------------------- the three sweeps

@pytest.mark.parametrize("name,order", SWEEP_CASES, ids=[f"{n}-{o}" for n, o in SWEEP_CASES])
def test_the_three_operations_are_the_models(name, order):
    import torch
    from navierstokes_amd import mpk
    u, want = expected(name, order)
    n = u.size
    E = _handle(name, order)
    try:
        info = E.info()
        plan = mpk.bilu4_plan_probe(n // 4, model(name, order).B.ptr, model(name, order).B.col, 0)
        sizes = list(plan["fwd_sizes"]) + list(plan["bwd_sizes"])
        assert info["launches"] == plan["fwd_launches"] + plan["bwd_launches"] + (2 if order == "colour" else 0), (info, plan)
        assert info["device_bytes"] > 0
        # what each case is here for
        if (name, order) == ("fe:6", "colour"):  # backward every level is narrow: one folded launch; forward 64, 67, 49, 64, 42, ..: mixed
            assert max(plan["bwd_sizes"]) < 64 and plan["bwd_launches"] == 1 and 1 < plan["fwd_launches"] < plan["fwd_levels"], plan
        if (name, order) == ("fe:10", "colour"):  # levels of 78 to 254 rows: every launch is an unfolded level
            assert min(sizes) >= 64 and plan["fwd_launches"] == plan["fwd_levels"] and plan["bwd_launches"] == plan["bwd_levels"], sizes
        if (name, order) == ("fe:6", "natural"):  # 19 levels of at most 37 rows: each sweep is ONE folded launch
            assert max(sizes) < 64 and plan["fwd_launches"] == plan["bwd_launches"] == 1, sizes
        if (name, order) == ("fe:10", "natural"):  # 31 levels of 1 to 91 rows: folded runs around unfolded levels
            assert min(sizes) < 64 <= max(sizes) and 1 < plan["fwd_launches"] < plan["fwd_levels"], sizes
        if (name, order) == ("limits:0", "natural"):
            C.assert_layered_levels(name, plan["fwd_sizes"], plan["bwd_sizes"])
            assert {63, 64, 65} <= set(sizes)
        du = _dev(u)
        for op in OPS:
            out = _poisoned(n)
            getattr(E, op)(out, du)
            assert_bit_equal(out.cpu().numpy(), want[op], f"{name} {order} {op}")
            assert_bit_equal(du.cpu().numpy(), u, f"{name} {order} {op}: the input was written")
            inplace = du.clone()
            getattr(E, op)(inplace, inplace)
            assert_bit_equal(inplace.cpu().numpy(), want[op], f"{name} {order} {op}: in place")
        # offset by one double (8-byte aligned only), on another stream, out of place and in place
        st = torch.cuda.Stream()
        buf_in, buf_out = torch.zeros(n + 1, dtype=torch.float64, device="cuda"), _poisoned(n + 1)
        torch.cuda.synchronize()
        for op in OPS:
            with torch.cuda.stream(st):
                buf_in[1:].copy_(du)
                getattr(E, op)(buf_out[1:], buf_in[1:])
                getattr(E, op)(buf_in[1:], buf_in[1:])
            st.synchronize()
            assert_bit_equal(buf_out[1:].cpu().numpy(), want[op], f"{name} {order} {op}: offset by 8 bytes, other stream")
            assert_bit_equal(buf_in[1:].cpu().numpy(), want[op], f"{name} {order} {op}: offset by 8 bytes, in place")
            assert float(buf_in[0].item()) == 0.0 and np.isnan(buf_out[0].item()), "written in front of the vector"
    finally:
        E.close()


@pytest.mark.parametrize("name,order", [("fe:6", "colour"), ("limits:0", "natural")])
def test_captured_and_replayed(name, order):
    import torch
    u0, want0 = expected(name, order)
    u1, want1 = expected(name, order, seed=1)
    n = u0.size
    E = _handle(name, order)
    du = _dev(u0)
    outs = {op: _poisoned(n) for op in OPS}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for op in OPS:
            getattr(E, op)(outs[op], du)
    for u, want in ((u1, want1), (u0, want0), (u1, want1)):
        du.copy_(_dev(u))
        for op in OPS:
            outs[op].fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for op in OPS:
            assert_bit_equal(outs[op].cpu().numpy(), want[op], f"{name} {order} {op}: replayed")
    E.close()


@pytest.mark.parametrize("name,order", [("fe:6", "colour"), ("arrow", "natural")])
def test_after_refactor(name, order):
    u, want0 = expected(name, order)
    _, want1 = expected(name, order, variant=1)
    assert not np.array_equal(want0["apply_hat"], want1["apply_hat"])
    E = _handle(name, order)
    du = _dev(u)
    for variant, want in ((1, want1), (0, want0)):
        E.refactor(OC.values(name, variant))
        wein, wk = model(name, order, variant).fetch()
        assert_bit_equal(E.fetch()[0], wein, "Einv after refactor")
        assert_bit_equal(E.fetch()[1], wk, "K after refactor")
        for op in OPS:
            out = _poisoned(u.size)
            getattr(E, op)(out, du)
            assert_bit_equal(out.cpu().numpy(), want[op], f"{name} {order} {op}: after refactor to variant {variant}")
    E.close()


@pytest.mark.parametrize("name,order", [("fe:6", "colour"), ("fe:6", "natural")])
def test_inf_and_nan_land_where_the_model_says(name, order):
    m = model(name, order)
    u = np.array(expected(name, order)[0])
    at = np.random.default_rng(9).permutation(u.size)[:2]
    u[at[0]], u[at[1]] = np.inf, np.nan
    E = _handle(name, order)
    du = _dev(u)
    partial = 0
    for op in OPS:
        want = getattr(m, op)(u)
        out = _poisoned(u.size)
        getattr(E, op)(out, du)
        got = out.cpu().numpy()
        nan = np.isnan(want)
        assert nan.any(), op
        partial += not nan.all()
        assert np.array_equal(np.isnan(got), nan), (op, np.nonzero(np.isnan(got) != nan)[0][:8])
        assert_bit_equal(got[~nan], want[~nan], f"{name} {order} {op}: the entries that are not NaN (Inf included)")
    assert partial >= 2  # a single sweep spreads it over a part of the vector only (both sweeps of apply_hat may reach every row)
    E.close()


# ---------------------------------------------------------------- GMRES on the split-preconditioned operator

@pytest.fixture
def apply_hat_is_the_product(monkeypatch):
    """The composed loops of the GMRES tests call mpk.SpMV_CSR(y, x, A) for an operator that is not a bcsr4x4_matrix: hand them
    the public apply_hat of a dilu4 there."""
    from navierstokes_amd import mpk
    plain = mpk.SpMV_CSR
    monkeypatch.setattr(mpk, "SpMV_CSR", lambda y, x, A: A.apply_hat(y, x) if isinstance(A, mpk.dilu4) else plain(y, x, A))


def _hat_system(name, order):
    """(E, b^, u0): the right-hand side of the hat system for b = _rhs, x0 = 0, from the public to_hat."""
    E = _handle(name, order)
    n = 4 * E.nbrows
    bhat = _dev(T._rhs(n))
    E.to_hat(bhat, bhat)
    return E, bhat, _dev(np.zeros(n))


@pytest.mark.parametrize("check_every", [1, 4])
@pytest.mark.parametrize("name,order", [("fe:3", "colour"), ("random:31", "natural")])
def test_gmres_is_the_composed_loop(name, order, check_every, apply_hat_is_the_product):
    E, bhat, u0 = _hat_system(name, order)
    want = T.composed(E, None, bhat, u0, 5, 1e-30, 12)
    got = T.solver_run(E, None, bhat, u0, 5, 1e-30, 12, check_every=check_every)
    assert want[0] == 12 and want[2] == 2 and want[4][0] == 2  # three cycles, the last of two steps
    T.assert_same_solve(got, want, f"{name} {order} check_every {check_every}")
    E.close()


def test_gmres_with_the_float_basis_is_the_composed_loop(apply_hat_is_the_product):
    E, bhat, u0 = _hat_system("fe:3", "colour")
    want = T32.composed_f32(E, None, bhat, u0, 5, 1e-30, 12)
    got = T32.solver_run(E, None, bhat, u0, 5, 1e-30, 12)
    assert want[0] == 12
    T32.assert_same_solve(got, want, "fe:3 colour, float basis")
    E.close()


def test_a_plan_is_the_composed_loop(apply_hat_is_the_product):
    E, bhat, u0 = _hat_system("fe:3", "colour")
    want = T.composed(E, None, bhat, u0, 5, 1e-30, 12)
    got = TP.planned_run(E, None, bhat, u0, 5, 1e-30, 12, 2)
    TP.assert_same(got, want + (0,), "fe:3 colour, planned in segments of 2")
    E.close()


def test_one_captured_cycle_is_the_composed_loop(apply_hat_is_the_product):
    import torch
    from navierstokes_amd import mpk
    restart = 5
    E, bhat, u0 = _hat_system("fe:3", "colour")
    want = T.composed(E, None, bhat, u0, restart, 1e-30, restart)  # maxiter = restart: exactly one cycle
    assert want[0] == restart and want[2] == 2
    S = mpk.gmres_solver(E, None, restart)
    u = u0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        S.prepare_stream()
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        S.cycle(bhat, u, True, 1e-30, restart)
    for _ in range(2):
        u.copy_(u0)
        g.replay()
        torch.cuda.synchronize()
        st = S.state()
        assert (st["its"], st["k"]) == (restart, restart), st
        assert_bit_equal(st["history"][:restart], want[1][1:], "the captured cycle's history")
        assert_bit_equal(u.cpu().numpy(), want[3], "the captured cycle's x")
    S.close()
    E.close()


def test_set_operator_rules():
    from navierstokes_amd import mpk
    L = mpk.lib()
    mat = C.matrix("fe:3")
    E = _handle("fe:3", "colour")
    F = mpk.bilu4(*mat, fill=0)
    A = mpk.bcsr4x4_matrix(*mat)
    with pytest.raises(ValueError):
        mpk.gmres_solver(E, F, 5)
    S = mpk.gmres_solver(A, F, 5)  # a preconditioner is set: the DILU operator is refused, and the solver keeps what it had
    assert L.mi_gmres_set_operator_dilu4(S.handle, E.handle) == MI_ERR_STATE and "preconditioner" in L.mi_last_error().decode()
    assert L.mi_gmres_set_precond(S.handle, None, 0, 0, 0) == 0 and L.mi_gmres_set_operator_dilu4(S.handle, E.handle) == 0
    assert L.mi_gmres_set_precond(S.handle, F.handle, 0, 0, 0) == MI_ERR_STATE and "DILU" in L.mi_last_error().decode()
    S.close()
    other = mpk.bcsr4x4_matrix(*C.matrix("chain"))
    S = mpk.gmres_solver(other, None, 5)
    assert L.mi_gmres_set_operator_dilu4(S.handle, E.handle) == MI_ERR_ARG and "row count" in L.mi_last_error().decode()
    S.close()
    for o in (other, F, A, E):
        o.close()


# ---------------------------------------------------------------- the composed solve

@pytest.mark.parametrize("name,order", [("fe:6", "colour"), ("fe:6", "natural"), ("random:31", "colour")])
def test_the_composed_solve_has_a_true_residual_within_the_dense_tests_margin(name, order):
    import torch
    from navierstokes_amd import mpk
    Ad, _, b = G.problem(name, None)
    mat = C.matrix(name)
    A = mpk.bcsr4x4_matrix(*mat)
    E = _handle(name, order)
    x = _dev(np.zeros_like(b))
    its, hist, reason = E.gmres(A, _dev(b), x, restart=30, rtol=RTOL, maxiter=300)
    torch.cuda.synchronize()
    true = G.true_residual(Ad, x.cpu().numpy(), b)
    print(f"dilu4.gmres {name} {order}: {its} iterations, hat history {hist[0]:.3e} -> {hist[-1]:.3e}, reason {reason}, true residual {true:.3e}")
    assert reason == 1 and hist[-1] <= RTOL and len(hist) == its + 1, (reason, hist[-1])
    assert true <= 10 * RTOL, true
    E.close()
    A.close()
