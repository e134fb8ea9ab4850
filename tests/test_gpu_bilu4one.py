"""The one-launch form of the block ILU solve (mi_bilu4_set_solve_form(F, 1)) on the GPU, bit for bit (uint64 views) against the
model's solve (tests/bilu4_model.py) and against form 0 of the same handle: every case of tests/bilu4_cases.py that factors and
the chunked patterns of tests/bilu4one_cases.py, with 1, 2, 3 and the default number of persistent workgroups; the four right-hand
sides, out of place and in place, vectors offset by 8 bytes, a non-default stream, three solves back to back, after both refactors;
NaN and Inf; fe_matrix(10) and fe_matrix(16), whose middle planes are wider than a chunk (50 solves into poisoned vectors: rows of
one 128-byte line of x lie in different levels there); switching forms; stream capture; the pattern that is not eligible.
No chunk of these patterns waits for more than 44 others.  The limits of the hand-off itself — 63, 64, 65, 128, 129, 255 and 256
dependencies (the polling lanes of one wave, of several, of the whole workgroup), a last-listed dependency that finishes last,
more chunks than the default grid has workgroups, two handles on form 1 on two streams, the cap of 256 from both sides — are in
tests/test_gpu_bilu4one_limits.py.
No test makes a wait give up (none shortens the spin bound): that path is read against launch_spmk.hip, not provoked."""
import os

import numpy as np
import pytest

import bilu4_cases as C
import bilu4_model as M
import bilu4one_cases as C1
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu
WGS = ("1", "2", "3", None)  # MI355_BILU_ONE_WGS
CASES = [(C, c) for c in C.ALL_CASES] + [(C1, c) for c in C1.SOLVE_CASES]


def _rhs(nb):
    """The four right-hand sides of tests/test_gpu_bilu4.py."""
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


def _same(got, want, what):
    """Bit-equal where the model is not NaN; NaN exactly where the model is NaN."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN reaches other rows than in the model"
    assert_bit_equal(np.where(nan, 0.0, got), np.where(nan, 0.0, want), what)


def _handle(wgs, nb, bp, bc, bv, fill):
    """A handle on form 1 with `wgs` persistent workgroups (None: the library's choice), and its form-0 solver for comparison."""
    from navierstokes_amd import mpk
    old = os.environ.pop("MI355_BILU_ONE_WGS", None)
    if wgs is not None:
        os.environ["MI355_BILU_ONE_WGS"] = wgs
    try:
        F = mpk.bilu4(nb, bp, bc, bv, fill=fill)
        assert F.info()["form"] == 0 and F.info_one()["prepared"] is False
        assert F.set_form(1) == 1
    finally:
        os.environ.pop("MI355_BILU_ONE_WGS", None)
        if old is not None:
            os.environ["MI355_BILU_ONE_WGS"] = old
    info, one = F.info(), F.info_one()
    assert info["form"] == 1 and info["launches"] == 1
    assert one["prepared"] and one["eligible"] and one["plan_bytes"] > 0 and max(one["max_deps"]) <= 256
    assert 1 <= one["workgroups"] <= (int(wgs) if wgs is not None else max(one["nchunks"]))
    return F


def _form0(F, b):
    """Form 0's result for b on the same handle (a device tensor); the handle is back on form 1 afterwards."""
    import torch
    assert F.set_form(0) == 0 and F.info()["launches"] > 1
    x = torch.full((b.numel(),), float("nan"), dtype=torch.float64, device="cuda")
    F.solve(x, b)
    torch.cuda.synchronize()
    assert F.set_form(1) == 1
    return x.cpu().numpy()


@pytest.mark.parametrize("mod,case", CASES, ids=[C.case_id(c) for _, c in CASES])
def test_one_launch_bits_equal_the_model_and_form_0(mod, case):
    import torch
    name, fill = case
    nb, bp, bc, bv = mod.matrix(name)
    fac = mod.model_factor(name, fill)
    if isinstance(fac, M.ZeroPivot):
        return  # no handle to solve with (tests/test_gpu_bilu4.py checks that creation refuses)
    n = 4 * nb
    rhs = _rhs(nb)
    want = {k: _model_solve(fac, nb, b) for k, b in rhs.items()}
    want2 = _model_solve(fac, nb, want["random"])
    want3 = _model_solve(fac, nb, want2)
    fac_new = mod.model_factor(name, fill, 1)
    want_new = None if isinstance(fac_new, M.ZeroPivot) else _model_solve(fac_new, nb, rhs["x_sin"])
    for wgs in WGS:
        F = _handle(wgs, nb, bp, bc, bv, fill)
        what = f"{name} fill {fill} workgroups {wgs}"
        for k, b in rhs.items():
            db = torch.from_numpy(b).cuda()
            x0 = _form0(F, db)
            dx = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
            F.solve(dx, db)
            got = dx.cpu().numpy()
            _same(got, want[k], f"{what} b={k} out of place")
            _same(got, x0, f"{what} b={k} against form 0")
            assert_bit_equal(db.cpu().numpy(), b, "b was written")
            F.solve(db, db)
            _same(db.cpu().numpy(), want[k], f"{what} b={k} in place")
        # a non-default stream; vectors offset by 8 bytes; three solves back to back, each consuming the one before: the epoch
        # advances, and flags of the earlier solve must not satisfy the later one
        st = torch.cuda.Stream()
        buf_b = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
        buf_x = torch.full((n + 1,), float("nan"), dtype=torch.float64, device="cuda")
        buf_b[1:].copy_(torch.from_numpy(rhs["x_sin"]))
        d1 = torch.from_numpy(rhs["random"]).cuda()
        x1, x2, x3 = (torch.full((n,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(3))
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            F.solve(buf_x[1:], buf_b[1:])
            F.solve(x1, d1)
            F.solve(x2, x1)
            F.solve(x3, x2)
            F.solve(buf_b[1:], buf_b[1:])
        st.synchronize()
        _same(buf_x[1:].cpu().numpy(), want["x_sin"], f"{what} offset by 8 bytes, other stream")
        _same(buf_b[1:].cpu().numpy(), want["x_sin"], f"{what} offset by 8 bytes, in place")
        _same(x1.cpu().numpy(), want["random"], f"{what} back to back, first")
        _same(x2.cpu().numpy(), want2, f"{what} back to back, second")
        _same(x3.cpu().numpy(), want3, f"{what} back to back, third")
        # after a host refactor, and after a device refactor back to the first values on the same stream as the solve
        if want_new is not None:
            F.refactor(mod.new_values(name, 1))
            dx = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
            F.solve(dx, torch.from_numpy(rhs["x_sin"]).cuda())
            _same(dx.cpu().numpy(), want_new, f"{what} after refactor")
        with torch.cuda.stream(st):
            F.refactor_dev(torch.from_numpy(np.asarray(bv, np.float64)).cuda())
            dx = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
            F.solve(dx, torch.from_numpy(rhs["edge"]).cuda())
        st.synchronize()
        F.factor_status()
        _same(dx.cpu().numpy(), want["edge"], f"{what} after refactor_dev")
        assert F.info()["form"] == 1
        F.one_status()
        F.close()


NAN_CASES = [(C, "fe:6", 0), (C, "fe_perm:6", 1), (C, "arrow", 0), (C, "chain", 0), (C, "random:7", 1), (C1, "wide3", 0), (C1, "fold_wide_fold", 0),
             (C1, "arrow200", 0)]


@pytest.mark.parametrize("mod,name,fill", NAN_CASES, ids=[C.case_id(c[1:]) for c in NAN_CASES])
def test_nan_and_inf_reach_the_rows_the_model_says(mod, name, fill):
    import torch
    nb, bp, bc, bv = mod.matrix(name)
    fac = mod.model_factor(name, fill)
    n = 4 * nb
    for wgs in ("2", None):
        F = _handle(wgs, nb, bp, bc, bv, fill)
        for at, bad in ((n // 2, np.nan), (n // 3, np.inf), (n - 1, -np.inf), (0, np.nan)):
            b = np.random.default_rng(at).standard_normal(n)
            b[at] = bad
            dx = torch.empty(n, dtype=torch.float64, device="cuda")
            F.solve(dx, torch.from_numpy(b).cuda())
            got = dx.cpu().numpy()
            _same(got, _model_solve(fac, nb, b), f"{name} {bad} at {at}, workgroups {wgs}")
            assert not np.isfinite(got).all(), "the special value vanished"
        F.close()


@pytest.mark.parametrize("nx,solves", [(10, 8), (16, 50)])
def test_planes_wider_than_a_chunk(nx, solves):
    """fe_matrix(10) and fe_matrix(16): 1 331 and 4 913 block rows.  The factor VALUES are read back from the handle
    (mi_bilu4_factor_host, pinned to the model by tests/test_bilu4_factor.py on the smaller cases); pattern, schedule and solve are
    the model's.  Then `solves` solves, each with another seeded b into a NaN-poisoned x, each compared with form 0's result for the
    same b: neighbouring rows of one 128-byte line of x lie in different levels, so a line served stale shows as a wrong row."""
    import torch
    from navierstokes_amd import mpk, synth
    bp, bc, bv = synth.csr_to_bcsr4(*synth.fe_matrix(nx))
    nb = len(bp) - 1
    assert nb == (nx + 1) ** 3
    for wgs in ("3", None):
        F = _handle(wgs, nb, bp, bc, bv, 0)
        one = F.info_one()
        probe = mpk.bilu4_plan_probe(nb, bp, bc, 0)  # (narrow levels fold, so chunks are compared with launches, not with levels)
        assert one["nchunks"][0] > probe["fwd_launches"] and one["nchunks"][1] > probe["bwd_launches"], "no level of this matrix is cut into chunks"
        ptr, col, diag, val = F.factor_host()
        mp, mc, md = M.symbolic(nb, bp, bc, 0)
        assert np.array_equal(ptr, mp) and np.array_equal(col, mc) and np.array_equal(diag, md)
        b = synth.x_sin(0, 4 * nb) + 1.0
        dx = torch.full((4 * nb,), float("nan"), dtype=torch.float64, device="cuda")
        F.solve(dx, torch.from_numpy(b).cuda())
        assert_bit_equal(dx.cpu().numpy(), _model_solve((mp, mc, md, val), nb, b), f"fe_matrix({nx}) workgroups {wgs}")
        rng = np.random.default_rng(nx)
        bs = [torch.from_numpy(rng.standard_normal(4 * nb)).cuda() for _ in range(solves)]
        assert F.set_form(0) == 0
        x0 = [torch.full((4 * nb,), float("nan"), dtype=torch.float64, device="cuda") for _ in bs]
        for x, v in zip(x0, bs):
            F.solve(x, v)
        torch.cuda.synchronize()
        assert F.set_form(1) == 1
        x1 = [torch.full((4 * nb,), float("nan"), dtype=torch.float64, device="cuda") for _ in bs]
        for x, v in zip(x1, bs):
            F.solve(x, v)
        torch.cuda.synchronize()
        for s, (a, c) in enumerate(zip(x1, x0)):
            assert_bit_equal(a.cpu().numpy(), c.cpu().numpy(), f"fe_matrix({nx}) workgroups {wgs} solve {s} against form 0")
        F.one_status()
        F.close()


def test_switching_forms_and_the_measured_choice():
    import torch
    nb, bp, bc, bv = C1.matrix("wide3")
    fac = C1.model_factor("wide3", 0)
    b = _rhs(nb)["random"]
    want = _model_solve(fac, nb, b)
    F = _handle(None, nb, bp, bc, bv, 0)
    db = torch.from_numpy(b).cuda()

    def check(what):
        dx = torch.full((4 * nb,), float("nan"), dtype=torch.float64, device="cuda")
        F.solve(dx, db)
        _same(dx.cpu().numpy(), want, what)

    check("form 1")
    assert F.set_form(0) == 0 and F.info()["form"] == 0 and F.info()["launches"] > 1
    check("back on form 0")
    chosen = F.set_form(-1)
    info = F.info()
    assert chosen in (0, 1) and info["form"] == chosen
    assert info["us_per_level_launches"] > 0 and info["us_one_launch"] > 0
    assert chosen == int(info["us_one_launch"] < 0.98 * info["us_per_level_launches"]), info
    print(f"wide3: {info['us_per_level_launches']:.1f} us per level-by-level solve, {info['us_one_launch']:.1f} us in one launch: form {chosen}")
    check("after the measured choice")
    assert F.set_form(1) == 1
    check("form 1 again")
    F.one_status()
    F.close()


def test_a_captured_solve_is_recorded_level_by_level():
    """Under stream capture form 0 is recorded (the one-launch form's epoch is a kernel argument): one stream, so one linear chain of
    kernel nodes.  Replayed twice with different right-hand sides."""
    import torch
    nb, bp, bc, bv = C1.matrix("fold_wide_fold")
    fac = C1.model_factor("fold_wide_fold", 0)
    rhs = _rhs(nb)
    F = _handle(None, nb, bp, bc, bv, 0)
    db = torch.from_numpy(rhs["ones"]).cuda()
    dx = torch.full((4 * nb,), float("nan"), dtype=torch.float64, device="cuda")
    F.solve(dx, db)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        F.solve(dx, db)
    assert F.info()["form"] == 1
    for k in ("random", "edge"):
        db.copy_(torch.from_numpy(rhs[k]))
        dx.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        _same(dx.cpu().numpy(), _model_solve(fac, nb, rhs[k]), f"replay with b={k}")
    F.solve(dx, db)  # and the handle still solves in one launch afterwards
    _same(dx.cpu().numpy(), _model_solve(fac, nb, rhs["edge"]), "after the replays")
    F.one_status()
    F.close()


def test_a_pattern_that_is_not_eligible_stays_on_form_0():
    import torch
    from navierstokes_amd import mpk
    nb, bp, bc, bv = C1.matrix("over_cap")
    F = mpk.bilu4(nb, bp, bc, bv, fill=0)
    with pytest.raises(mpk.MiError) as e:
        F.set_form(1)
    assert e.value.status == 5 and "256" in str(e.value)
    with pytest.raises(mpk.MiError) as e:
        F.prepare_one()
    assert e.value.status == 5
    assert F.info()["form"] == 0 and F.info_one()["eligible"] is False and F.info_one()["max_deps"] == (257, 0)
    assert F.set_form(-1) == 0 and F.info()["us_one_launch"] == 0.0
    # the trivial pattern by hand: t = b but for the last row, which subtracts its L blocks in ascending column order; x_i = Dinv_i t_i
    ptr, col, diag, val = F.factor_host()
    b = np.random.default_rng(9).standard_normal(4 * nb)
    t = b.reshape(nb, 4).copy()
    for k in range(ptr[nb - 1], diag[nb - 1]):
        t[nb - 1] = t[nb - 1] - M.matvec4(val[k], t[col[k]])
    want = M.matvec4(val[diag], t).reshape(-1)
    dx = torch.full((4 * nb,), float("nan"), dtype=torch.float64, device="cuda")
    F.solve(dx, torch.from_numpy(b).cuda())
    assert_bit_equal(dx.cpu().numpy(), want, "over_cap on form 0")
    F.close()
