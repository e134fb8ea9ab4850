"""The ordered block ILU (mpk.bilu4(order="colour"), mi_bilu4_create_ordered) on the GPU: every way of applying the factor keeps its
meaning in the caller's numbering, bit for bit (uint64 views).

  exact      solve(b) is: permute b, tests/bilu4_model.py's solve of the explicitly permuted system, un-permute — on the patterns of
             tests/bilu4_order_cases.py at fill 0 and 1, both layouts; form 0 and form 1 with 1, 2 and the default number of
             workgroups; x == b; vectors offset by 8 bytes (this reaches the scalar form of the two boundary kernels; the level
             kernels of an ordered handle always run on its own aligned vectors); a non-default stream; host vectors
  refactor   mi_bilu4dev_refactor + mi_bilu4dev_fetch leave the host refactor's factor; the solve follows
  sweeps     sweeps(levels - 1) is the exact solve, sweeps(2) the model of tests/bilu4_sweeps_model.py on the permuted system; the same
             with precision="f32" against the rounded-factor model
  gmres      mpk.GMRES with M = the ordered handle against mpk.GMRES with a Python object that permutes, solves with a natural-order
             handle built from the explicitly permuted matrix, and un-permutes: x and history
  gmres_dev  GMRES_dev's solver with M = the ordered handle against the loop composed from public pieces (the one of
             tests/test_gpu_gmres_dev.py, restated here), eagerly and through plan(segment=5)
  graph      (device refactor, mi_gmres_cycle_dev) captured with an ordered handle replays to the eager bits
"""
import ctypes
import os

import numpy as np
import pytest

import bilu4_order_cases as OC
import bilu4_sp_model as SP
import bilu4_sweeps_model as S
import gmres_dev_model as D
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

CASES = [(name, fill) for name in OC.PATTERNS for fill in (0, 1)]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _poisoned(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def _colour_handle(name, fill, layout="row", wgs=None, form=0):
    """An ordered handle; form 1: on the one-launch form with `wgs` persistent workgroups (None: the library's choice)."""
    from navierstokes_amd import mpk
    nb, bp, bc, _ = OC.matrix(name)
    blocks = OC.values(name).reshape(-1, 4, 4)
    coef = (blocks.transpose(0, 2, 1) if layout == "col" else blocks).reshape(-1).copy()
    old = os.environ.pop("MI355_BILU_ONE_WGS", None)
    if wgs is not None:
        os.environ["MI355_BILU_ONE_WGS"] = wgs
    try:
        F = mpk.bilu4(nb, bp, bc, coef, fill=fill, layout=layout, order="colour")
        if form == 1:
            assert F.set_form(1) == 1
    finally:
        os.environ.pop("MI355_BILU_ONE_WGS", None)
        if old is not None:
            os.environ["MI355_BILU_ONE_WGS"] = old
    return F


@pytest.mark.parametrize("name,fill", CASES, ids=[f"{n}-fill{f}" for n, f in CASES])
def test_the_exact_solve_is_the_models_solve_of_the_permuted_system(name, fill):
    import torch
    nb = OC.matrix(name)[0]
    n = 4 * nb
    rng = np.random.default_rng(nb + 13 * fill)
    b = rng.standard_normal(n)
    want = OC.model_solve(name, fill, b)
    db = _dev(b)
    F = _colour_handle(name, fill)
    try:
        info, oinfo = F.info(), F.order_info()
        assert oinfo["order"] == "colour" and np.array_equal(oinfo["perm"], OC.ordered(name)[1])
        if fill == 0:
            assert info["fwd_levels"] <= oinfo["ncolours"] and info["bwd_levels"] <= oinfo["ncolours"]
        dx = _poisoned(n)
        F.solve(dx, db)
        assert_bit_equal(dx.cpu().numpy(), want, f"{name} fill {fill}: form 0")
        assert_bit_equal(db.cpu().numpy(), b, "b was written")
        inplace = db.clone()
        F.solve(inplace, inplace)
        assert_bit_equal(inplace.cpu().numpy(), want, f"{name} fill {fill}: x == b")
        # offset by one double (8-byte aligned only), on another stream, in place too
        st = torch.cuda.Stream()
        buf_b, buf_x = torch.zeros(n + 1, dtype=torch.float64, device="cuda"), _poisoned(n + 1)
        buf_b[1:].copy_(db)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            F.solve(buf_x[1:], buf_b[1:])
            F.solve(buf_b[1:], buf_b[1:])
        st.synchronize()
        assert_bit_equal(buf_x[1:].cpu().numpy(), want, f"{name} fill {fill}: offset by 8 bytes, other stream")
        assert_bit_equal(buf_b[1:].cpu().numpy(), want, f"{name} fill {fill}: offset by 8 bytes, in place")
        hx = np.full(n, np.nan)
        F.solve(hx, b)
        assert_bit_equal(hx, want, f"{name} fill {fill}: host vectors")
        # the same handle on the one-launch form, the library's number of workgroups
        assert F.set_form(1) == 1 and F.info()["launches"] == 1 + 2
        dx = _poisoned(n)
        F.solve(dx, db)
        assert_bit_equal(dx.cpu().numpy(), want, f"{name} fill {fill}: form 1")
        inplace = db.clone()
        F.solve(inplace, inplace)
        assert_bit_equal(inplace.cpu().numpy(), want, f"{name} fill {fill}: form 1, x == b")
        F.one_status()
    finally:
        F.close()
    for wgs in ("1", "2"):
        F = _colour_handle(name, fill, wgs=wgs, form=1)
        dx = _poisoned(n)
        F.solve(dx, db)
        got = dx.cpu().numpy()
        F.one_status()
        F.close()
        assert_bit_equal(got, want, f"{name} fill {fill}: form 1 with {wgs} workgroup(s)")
    F = _colour_handle(name, fill, layout="col")
    dx = _poisoned(n)
    F.solve(dx, db)
    got = dx.cpu().numpy()
    F.close()
    assert_bit_equal(got, want, f"{name} fill {fill}: column-major blocks")


REFACTOR_CASES = [("fe:4", 0), ("arrow", 1), ("unsym", 0), ("random:7", 1)]


@pytest.mark.parametrize("name,fill", REFACTOR_CASES, ids=[f"{n}-fill{f}" for n, f in REFACTOR_CASES])
def test_the_device_refactor_leaves_the_host_refactors_factor(name, fill):
    from navierstokes_amd import mpk
    nb, bp, bc, bv = OC.matrix(name)
    new = OC.values(name, 1)
    H = mpk.bilu4(nb, bp, bc, bv, fill=fill, host_only=True, order="colour").refactor(new)
    host = H.factor_host()
    H.close()
    F = _colour_handle(name, fill)
    F.refactor_dev(_dev(new)).factor_status().fetch_factor()
    got = F.factor_host()
    for a, w, m in zip(got, host, OC.model_factor(name, fill, 1)):
        assert_bit_equal(np.asarray(a, np.float64), np.asarray(w, np.float64), f"{name} fill {fill}: against the host refactor")
        assert_bit_equal(np.asarray(a, np.float64), np.asarray(m, np.float64), f"{name} fill {fill}: against the model")
    b = np.random.default_rng(3).standard_normal(4 * nb)
    dx = _poisoned(4 * nb)
    F.solve(dx, _dev(b))
    assert_bit_equal(dx.cpu().numpy(), OC.model_solve(name, fill, b, 1), f"{name} fill {fill}: the solve after refactor_dev")
    F.refactor(OC.values(name))
    F.solve(dx, _dev(b))
    assert_bit_equal(dx.cpu().numpy(), OC.model_solve(name, fill, b), f"{name} fill {fill}: the solve after the host refactor back")
    F.close()


SWEEP_CASES = [("fe:3", 0), ("fe:4", 1), ("chain", 0), ("arrow", 0), ("unsym", 0), ("random:3", 0), ("random:11", 1)]


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name,fill", SWEEP_CASES, ids=[f"{n}-fill{f}" for n, f in SWEEP_CASES])
def test_sweeps_on_an_ordered_handle(name, fill, precision):
    nb, perm = OC.ordered(name)[:2]
    fac = OC.model_factor(name, fill)
    model = SP.solve_sweeps_sp if precision == "f32" else S.solve_sweeps
    n = 4 * nb
    b = np.random.default_rng(nb + 5).standard_normal(n)
    db = _dev(b)
    F = _colour_handle(name, fill)
    mf, mb = S.max_sweeps(nb, *fac[:3])
    assert (mf, mb) == (F.info()["fwd_levels"] - 1, F.info()["bwd_levels"] - 1)
    try:
        dx = _poisoned(n)
        F.sweeps(mf, mb, precision=precision).solve(dx, db)
        full = dx.cpu().numpy()
        assert_bit_equal(full, OC.vec_out(model(nb, *fac, OC.vec_in(b, perm), mf, mb), perm), f"{name} fill {fill} {precision}: sweeps(levels - 1) against the model")
        if precision == "f64":
            exact = _poisoned(n)
            F.solve(exact, db)
            assert_bit_equal(full, exact.cpu().numpy(), f"{name} fill {fill}: sweeps(levels - 1) against the exact solve")
            assert_bit_equal(full, OC.model_solve(name, fill, b), f"{name} fill {fill}: sweeps(levels - 1) against the model's exact solve")
        dx = _poisoned(n)
        F.sweeps(2, precision=precision).solve(dx, db)
        want = OC.vec_out(model(nb, *fac, OC.vec_in(b, perm), 2, 2), perm)
        assert_bit_equal(dx.cpu().numpy(), want, f"{name} fill {fill} {precision}: sweeps(2)")
        inplace = db.clone()
        F.sweeps(2, precision=precision).solve(inplace, inplace)
        assert_bit_equal(inplace.cpu().numpy(), want, f"{name} fill {fill} {precision}: sweeps(2), x == b")
    finally:
        F.close()


# ---------------------------------------------------------------- GMRES

class PermutedNatural:
    """What an ordered handle is, spelled out: permute, solve with a NATURAL-order handle of the explicitly permuted matrix, un-permute."""

    def __init__(self, name, fill=0):
        import torch
        from navierstokes_amd import mpk
        nb, perm, _, bptr, bcol, _ = OC.ordered(name)
        self.F = mpk.bilu4(nb, bptr, bcol, OC.permuted_values(name).reshape(-1), fill=fill)
        self.perm = torch.from_numpy(np.asarray(perm, np.int64)).cuda()
        self.iperm = torch.argsort(self.perm)

    def solve(self, x, b):
        t = b.view(-1, 4)[self.iperm].contiguous().view(-1)  # t[perm[i]] = b[i]
        self.F.solve(t, t)
        x.copy_(t.view(-1, 4)[self.perm].reshape(-1))        # x[i] = t[perm[i]]
        return x

    def close(self):
        self.F.close()


def _rhs(n):
    return np.sin(0.37 * np.arange(n)) + 1.0 + 0.25 * np.cos(0.011 * np.arange(n) ** 2)


def test_gmres_with_an_ordered_handle_is_gmres_with_the_permutation_spelled_out():
    import torch
    from navierstokes_amd import mpk
    nb, bp, bc, bv = OC.matrix("fe:6")
    A = mpk.bcsr4x4_matrix(nb, bp, bc, bv)
    Fc = mpk.bilu4(nb, bp, bc, bv, fill=0, order="colour")
    ref = PermutedNatural("fe:6")
    assert np.array_equal(Fc.order_info()["perm"], OC.ordered("fe:6")[1]) and Fc.order_info()["ncolours"] >= 2
    b = _dev(_rhs(4 * nb))
    x, xr = torch.zeros_like(b), torch.zeros_like(b)
    its, hist = mpk.GMRES(A, b, x, M=Fc, restart=30, rtol=1e-8, maxiter=300)
    rits, rhist = mpk.GMRES(A, b, xr, M=ref, restart=30, rtol=1e-8, maxiter=300)
    print(f"fe:6, ILU(0) in colour order ({Fc.order_info()['ncolours']} colours): {its} iterations to {hist[-1]:.3e}")
    assert its == rits and its >= 2 and hist[-1] <= 1e-8
    assert_bit_equal(hist, rhist, "history")
    assert_bit_equal(x.cpu().numpy(), xr.cpu().numpy(), "x")
    ref.close()
    Fc.close()
    A.close()


def composed(A, Mpc, b, x0, restart, rtol, maxiter):
    """Restarted GMRES as include/mi355_spmv.h defines it, from the library's public pieces: the loop of tests/test_gpu_gmres_dev.py.
    Returns (iterations, history, reason, x, (k, hraw, y, beta))."""
    import torch
    from navierstokes_amd import mpk
    mult = mpk.SpMV_BCSR
    n = int(b.numel())
    x = x0.clone()
    V = torch.empty((restart + 1, n), dtype=torch.float64, device=b.device)
    w, z = torch.empty_like(b), torch.empty_like(b)
    bnorm = D.bnorm_of(float(mpk.norm2(b).item()))
    its, hist = 0, []
    while True:
        mult(w, x, A)
        r = V[0]
        r.copy_(b)
        mpk.axpy(-1.0, w, r)
        beta = float(mpk.norm2(r).item())
        rel, reason = D.cycle_start(beta, bnorm, its, rtol, maxiter)
        if not hist:
            hist.append(rel)
        if reason is not None:
            return its, hist, reason, x.cpu().numpy(), (0, np.zeros((restart, restart + 2)), np.zeros(0), beta)
        with np.errstate(all="ignore"):
            r.copy_(_dev(r.cpu().numpy() / beta))
        cyc = D.Cycle(restart, beta, bnorm, rtol)
        hraw = np.zeros((restart, restart + 2))
        while cyc.k < restart and its < maxiter and not cyc.reason:
            k = cyc.k
            Mpc.solve(z, V[k])
            mult(V[k + 1], z, A)
            h, nrm = mpk.cgs([V[j] for j in range(k + 1)], V[k + 1], passes=2)
            col = torch.cat([h, nrm]).cpu().numpy()
            entry = cyc.step(col)
            if entry is None:
                break
            hraw[k, : k + 2] = col
            its += 1
            hist.append(entry)
            with np.errstate(all="ignore"):
                V[k + 1].copy_(_dev(V[k + 1].cpu().numpy() / col[-1]))
        k = cyc.k
        y = np.array(cyc.solve())
        if k:
            w.zero_()
            mpk.maxpy(y, [V[j] for j in range(k)], w)
            Mpc.solve(z, w)
            mpk.axpy(1.0, z, x)
        last = (k, hraw, y, beta)
        if cyc.reason:
            return its, hist, cyc.reason, x.cpu().numpy(), last
        if its >= maxiter:
            return its, hist, 2, x.cpu().numpy(), last


def _assert_same_solve(got, want, what):
    assert (got[0], got[2]) == (want[0], want[2]), (what, got[0], got[2], want[0], want[2])
    assert len(got[1]) == got[0] + 1
    assert_bit_equal(got[1], want[1], f"{what}: history")
    assert_bit_equal(got[3], want[3], f"{what}: x")
    (k, hraw, y, beta), (wk, whraw, wy, wbeta) = got[4], want[4]
    assert k == wk, (what, k, wk)
    assert_bit_equal(hraw, whraw, f"{what}: raw columns of the last cycle")
    assert_bit_equal(y, wy, f"{what}: y of the last cycle")
    assert_bit_equal([beta], [wbeta], f"{what}: beta of the last cycle")


@pytest.mark.parametrize("kind", ["exact", "sweeps", "sweeps_f32"])
@pytest.mark.parametrize("name", ["fe:3", "random:19"])
def test_gmres_dev_with_an_ordered_handle_is_the_composed_loop(name, kind):
    import torch
    from navierstokes_amd import mpk
    nb, bp, bc, bv = OC.matrix(name)
    A = mpk.bcsr4x4_matrix(nb, bp, bc, bv)
    F = _colour_handle(name, 0)
    Mpc = F if kind == "exact" else F.sweeps(2, 2, precision="f32" if kind == "sweeps_f32" else "f64")
    n = 4 * nb
    b, x0 = _dev(_rhs(n)), _dev(np.zeros(n))
    restart, rtol, maxiter = 5, 1e-30, 12
    want = composed(A, Mpc, b, x0, restart, rtol, maxiter)
    assert want[0] >= 2
    for how in ("eager", "planned"):
        Sv = mpk.gmres_solver(A, Mpc, restart)
        x = x0.clone()
        if how == "eager":
            its, hist, reason = Sv.solve(b, x, rtol=rtol, maxiter=maxiter, check_every=5)
            P = None
        else:
            P = Sv.plan(b, x, rtol=rtol, maxiter=maxiter, segment=5)
            its, hist, reason = P.solve()
        torch.cuda.synchronize()
        got = its, hist, reason, x.cpu().numpy(), Sv.fetch_cycle()
        if P is not None:
            P.close()
        Sv.close()
        _assert_same_solve(got, want, f"{name} {kind} {how}")
    F.close()
    A.close()


def test_device_refactor_and_cycle_as_one_graph_with_an_ordered_handle():
    import torch
    from navierstokes_amd import mpk
    L = mpk.lib()
    name, restart, maxiter, rtol = "fe:4", 5, 300, 1e-8
    nb, bp, bc, bv = OC.matrix(name)
    n = 4 * nb
    A = mpk.bcsr4x4_matrix(nb, bp, bc, bv)
    F = _colour_handle(name, 0).prepare_dev()
    Sv = mpk.gmres_solver(A, F, restart)
    values = [_dev(OC.values(name)), _dev(OC.values(name, 1))]
    coef = torch.empty_like(values[0])  # what the graph reads
    b, x0 = _dev(_rhs(n)), _dev(0.01 * np.cos(0.3 * np.arange(n)))
    x = x0.clone()
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def step():
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        mpk.check(L.mi_bcsr4_update_values_dev(A.handle, p(coef), s))
        mpk.check(L.mi_bilu4dev_refactor(F.handle, p(coef), 0, s))
        Sv.cycle(b, x, True, rtol, maxiter)

    def record():
        st = Sv.state()
        return (st["its"], st["k"], st["done"], st["reason"]), [st["last"], st["beta"]] + st["history"]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    eager = []
    with torch.cuda.stream(side):
        Sv.prepare_stream()
        for v in values:
            coef.copy_(v), x.copy_(x0)
            step()
            eager.append(record() + (x.cpu().numpy(),))
        F.factor_status()
    side.synchronize()
    assert eager[0][0][1] >= 1 and not np.array_equal(eager[0][2], eager[1][2])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step()
    for which in (1, 0, 1):
        coef.copy_(values[which]), x.copy_(x0)
        g.replay()
        ints, floats = record()
        torch.cuda.synchronize()
        assert ints == eager[which][0], (which, ints, eager[which][0])
        assert_bit_equal(floats, eager[which][1], f"values {which}: the record")
        assert_bit_equal(x.cpu().numpy(), eager[which][2], f"values {which}: x")
    F.factor_status()
    Sv.close()
    F.close()
    A.close()
