"""The exact block ILU solve over the single-precision copy of the factor (mi_bilu4spx_*, mpk.bilu4.exact("f32"),
MI_GMRES_PC_EXACT_F32) on the GPU.  Every comparison is bit for bit.  The oracle has two statements, which
tests/test_bilu4spx_model.py shows to agree: (a) tests/bilu4_model.solve on the rounded factor, (b) the f32 sweeps at the clamp.

  model     natural-order handles, fill 0, 1 and 2, vectors 16-byte aligned and offset by one double, out of place and x is b,
            host vectors: (a), and mi_bilu4sp_solve_dev at (max_fwd, max_bwd) and far above
  ordered   order="colour": (a) on the explicitly permuted system, brought back; wide launches where a level has 64 rows
  wide      tests/bilu4_wide_cases.py with MI355_BILU_WIDE_MIN default, 128 and above every width: the same bits, and (a)
  current   after refactor(host values) and after refactor_dev the solve follows the new rounded factor; the double solve is its own
  form      on the one-launch form the f32 exact solve is still enqueued level by level; the double solve still runs form 1
  overflow  sp_overflow: Inf / NaN exactly in the model's rows, the solve is not blocked, sweep_status_f32() names block row 0
  capture   refactor_dev + the f32 exact solve as one graph, replayed with two sets of values; refused when unprepared
  gmres     M = F.exact("f32") against M = F.sweeps(max_fwd, max_bwd, precision="f32"): the same operator, hence the same solve —
            eager (check_every 1 and 3), planned (segment 1 and restart) and a captured cycle
"""
import functools
import os

import numpy as np
import pytest

import bilu4_cases as C
import bilu4_model as M
import bilu4_order_cases as OC
import bilu4_sp_cases as SC
import bilu4_sp_model as SP
import bilu4_wide_cases as W
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

# a layered pattern small enough for the model at fill 2.  Fill 0: the folded runs (2), (5, 1) and (3, 40, 1) between unfolded levels of 64
# and 65 block rows; fill 1 and 2 join the layers into one folded run of many levels of two or three rows
SMALL_LAYERS = ((2, 64, 5, 1, 65, 3, 40, 1), 0, 36)
MODEL_PATTERNS = ["fe:6", "chain", "arrow", "diag", "layers", "sp_edges", "random:3", "random:7", "random:12", "random:25"]
MODEL_CASES = [(name, fill) for name in MODEL_PATTERNS for fill in (0, 1, 2)] + [("limits:0", 0)]
ORDER_CASES = [(name, fill) for name in OC.PATTERNS for fill in (0, 1)]
NEVER = 2 ** 31 - 1  # MI355_BILU_WIDE_MIN above every width


def _same(got, want, what):
    """Bit-equal, NaN and Inf included (NaN wherever the model has NaN: their payloads are not part of the interface)."""
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


@functools.lru_cache(maxsize=None)
def _matrix(name):
    return C.layered(*SMALL_LAYERS) if name == "layers" else SC.matrix(name)


@functools.lru_cache(maxsize=None)
def _factor(name, fill, variant=0):
    if name == "layers":
        assert variant == 0
        nb, bp, bc, bv = _matrix(name)
        return M.factor(nb, bp, bc, bv, fill)
    fac = SC.model_factor(name, fill, variant)
    assert not isinstance(fac, M.ZeroPivot), f"{name} fill {fill} variant {variant} does not factor: not a case here"
    return fac


def _model_f32(nb, fac, b):
    """Statement (a): the exact solve with v32 in place of every factor value."""
    with np.errstate(all="ignore"):
        return M.solve(nb, *SP.rounded(fac), b)


def _level_launches(F):
    """Launches of a level-by-level solve of this handle (asked before the form is changed)."""
    info = F.info()
    assert info["form"] == 0
    return info["launches"]


@pytest.mark.parametrize("name,fill", MODEL_CASES, ids=[C.case_id(c) for c in MODEL_CASES])
def test_the_f32_exact_solve_is_the_model_and_the_f32_sweeps_at_the_clamp(name, fill):
    import torch
    from navierstokes_amd import mpk
    nb, bp, bc, bv = _matrix(name)
    fac = _factor(name, fill)
    n = 4 * nb
    b = np.random.default_rng(3 * nb + fill).standard_normal(n)
    want = _model_f32(nb, fac, b)
    if nb > 3:
        assert not np.array_equal(want, M.solve(nb, *fac, b)), "the rounded factor must be another operator, or the test shows nothing"
    F = mpk.bilu4(nb, bp, bc, bv, fill=fill)
    view = F.exact("f32")
    try:
        launches = _level_launches(F)
        assert F.exact_info_f32() == dict(launches_last=0, wide_launches_last=0)
        db = _dev(b)
        assert db.data_ptr() % 16 == 0
        dx = _poisoned(n)
        assert view.solve(dx, db) is dx  # (the first one prepares)
        _same(dx.cpu().numpy(), want, f"{name} fill {fill}: aligned")
        assert_bit_equal(db.cpu().numpy(), b, "b was written")
        assert F.exact_info_f32() == dict(launches_last=launches, wide_launches_last=0), "a natural-order handle never takes the wide kernel"
        info = F.sweep_info_f32()
        assert info["prepared"] and info["convert_launches"] == 1 and info["launches_last"] == 0, info
        inplace = db.clone()
        view.solve(inplace, inplace)
        _same(inplace.cpu().numpy(), want, f"{name} fill {fill}: aligned, x is b")
        # offset by one double: 8-byte aligned only
        buf_b, buf_x = torch.zeros(n + 1, dtype=torch.float64, device="cuda"), _poisoned(n + 1)
        ob, ox = buf_b[1:], buf_x[1:]
        assert ob.data_ptr() % 16 == 8 and ox.data_ptr() % 16 == 8
        ob.copy_(db)
        view.solve(ox, ob)
        _same(ox.cpu().numpy(), want, f"{name} fill {fill}: offset by 8 bytes")
        view.solve(ob, ob)
        _same(ob.cpu().numpy(), want, f"{name} fill {fill}: offset by 8 bytes, x is b")
        assert float(buf_b[0]) == 0.0 and np.isnan(float(buf_x[0])), "the entry in front of an offset vector was written"
        hx = np.full(n, np.nan)
        view.solve(hx, b)
        _same(hx, want, f"{name} fill {fill}: host vectors")
        # statement (b): the sweeps over the same copy, at the clamp and far above
        sw = F.sweep_info()
        for counts in ((sw["max_fwd"], sw["max_bwd"]), (10 ** 6, 10 ** 6)):
            dx = _poisoned(n)
            F.sweeps(*counts, precision="f32").solve(dx, db)
            _same(dx.cpu().numpy(), want, f"{name} fill {fill}: f32 sweeps {counts}")
        F.sweep_status_f32()
    finally:
        F.close()


@pytest.mark.parametrize("name,fill", ORDER_CASES, ids=[f"{n}-fill{f}" for n, f in ORDER_CASES])
def test_an_ordered_handle_solves_the_rounded_factor_of_the_permuted_system(name, fill):
    import torch
    from navierstokes_amd import mpk
    nb, bp, bc, _ = OC.matrix(name)
    n = 4 * nb
    b = np.random.default_rng(nb + 17 * fill).standard_normal(n)
    perm = OC.ordered(name)[1]
    fac = OC.model_factor(name, fill)
    want = OC.vec_out(_model_f32(nb, fac, OC.vec_in(b, perm)), perm)
    # what the launch rule makes of the permuted system's levels: 64 rows and more are never folded, and wide on an ordered handle
    wide = sum(int(np.sum(M.schedule(nb, *fac[:3], backward)["sizes"] >= M.ROWS_PER_WG)) for backward in (False, True))
    F = mpk.bilu4(nb, bp, bc, OC.values(name), fill=fill, order="colour")
    view = F.exact("f32")
    try:
        launches = _level_launches(F)
        oinfo = F.order_info()
        assert np.array_equal(oinfo["perm"], perm)
        db = _dev(b)
        dx = _poisoned(n)
        view.solve(dx, db)
        _same(dx.cpu().numpy(), want, f"{name} fill {fill}")
        assert_bit_equal(db.cpu().numpy(), b, "b was written")
        got = F.exact_info_f32()
        assert got == dict(launches_last=launches, wide_launches_last=oinfo["wide_launches"]), (got, launches, oinfo["wide_launches"])
        assert got["wide_launches_last"] == wide, (got, wide)
        if name in ("chain", "arrow") and fill == 0:
            assert got["wide_launches_last"] > 0, "a colour of 64 block rows or more is a wide level"
        inplace = db.clone()
        view.solve(inplace, inplace)
        _same(inplace.cpu().numpy(), want, f"{name} fill {fill}: x is b")
        st = torch.cuda.Stream()
        buf_b, buf_x = torch.zeros(n + 1, dtype=torch.float64, device="cuda"), _poisoned(n + 1)
        buf_b[1:].copy_(db)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            view.solve(buf_x[1:], buf_b[1:])
            view.solve(buf_b[1:], buf_b[1:])
        st.synchronize()
        _same(buf_x[1:].cpu().numpy(), want, f"{name} fill {fill}: offset by 8 bytes, other stream")
        _same(buf_b[1:].cpu().numpy(), want, f"{name} fill {fill}: offset by 8 bytes, x is b")
        sw = F.sweep_info()
        dx = _poisoned(n)
        F.sweeps(sw["max_fwd"], sw["max_bwd"], precision="f32").solve(dx, db)
        _same(dx.cpu().numpy(), want, f"{name} fill {fill}: f32 sweeps at the clamp")
        # the double solve of the same handle is untouched
        dx = _poisoned(n)
        F.solve(dx, db)
        assert_bit_equal(dx.cpu().numpy(), OC.model_solve(name, fill, b), f"{name} fill {fill}: the double solve beside it")
    finally:
        F.close()


def test_the_levels_of_the_ordered_cases_include_wide_ones():
    """(no GPU work) chain's two colours are 75 block rows each and arrow's first is 79: the cases the wide assertion above rests on"""
    for name in ("chain", "arrow"):
        nb, _, colour = OC.ordered(name)[:3]
        assert np.bincount(colour).max() >= 64, (name, np.bincount(colour))


def _wide_handle(wide_min):
    from navierstokes_amd import mpk
    old = os.environ.pop("MI355_BILU_WIDE_MIN", None)
    if wide_min is not None:
        os.environ["MI355_BILU_WIDE_MIN"] = str(wide_min)
    try:
        return mpk.bilu4(*W.matrix(), fill=0, order="colour")
    finally:
        os.environ.pop("MI355_BILU_WIDE_MIN", None)
        if old is not None:
            os.environ["MI355_BILU_WIDE_MIN"] = old


@pytest.mark.parametrize("offset", [0, 1], ids=["16-byte aligned", "offset by 8 bytes"])
def test_the_wide_kernel_at_its_limits_gives_the_bits_of_the_narrow_one(offset):
    import torch
    nb, bp, bc, bv = W.matrix()
    n = 4 * nb
    perm, _ = OC.colour_model(nb, bp, bc)
    assert np.array_equal(perm, np.arange(nb)), "the pattern is already in colour order"
    b = np.random.default_rng(62).standard_normal(n)
    want = _model_f32(nb, _wide_factor(), b)
    got = {}
    for wide_min in (None, 128, NEVER):
        F = _wide_handle(wide_min)
        try:
            launches = _level_launches(F)
            buf_b, buf_x = torch.zeros(n + 2, dtype=torch.float64, device="cuda"), _poisoned(n + 2)
            db, dx = buf_b[offset:offset + n], buf_x[offset:offset + n]
            assert db.data_ptr() % 16 == 8 * offset and dx.data_ptr() % 16 == 8 * offset
            db.copy_(_dev(b))
            F.exact("f32").solve(dx, db)
            info = F.exact_info_f32()
            threshold = W.WIDE_MIN if wide_min is None else wide_min
            assert info == dict(launches_last=launches, wide_launches_last=2 * sum(w >= threshold for w in W.WIDTHS)), (wide_min, info)
            got[wide_min] = dx.cpu().numpy()
            F.exact("f32").solve(db, db)
            assert_bit_equal(db.cpu().numpy(), got[wide_min], f"MI355_BILU_WIDE_MIN={wide_min}: x is b")
        finally:
            F.close()
    assert info["wide_launches_last"] == 0, "above every width nothing is wide"
    for wide_min in (None, 128, NEVER):
        assert_bit_equal(got[wide_min], want, f"MI355_BILU_WIDE_MIN={wide_min} against the model")


@functools.lru_cache(maxsize=None)
def _wide_factor():
    nb, bp, bc, bv = W.matrix()
    return M.factor(nb, bp, bc, bv, 0)


@pytest.mark.parametrize("order", ["natural", "colour"])
def test_the_solve_follows_the_copy_through_both_refactorisations(order):
    from navierstokes_amd import mpk
    name, fill = "fe:4", 0
    nb, bp, bc, _ = OC.matrix(name)
    n = 4 * nb
    b = np.random.default_rng(44).standard_normal(n)
    perm = OC.ordered(name)[1] if order == "colour" else np.arange(nb)
    values = [OC.values(name, v) for v in (0, 1)]

    def models(variant):
        if order == "colour":
            fac = OC.model_factor(name, fill, variant)
        else:
            fac = M.factor(nb, bp, bc, values[variant], fill)
        bi = OC.vec_in(b, perm)
        return OC.vec_out(_model_f32(nb, fac, bi), perm), OC.vec_out(M.solve(nb, *fac, bi), perm)

    want = [models(0), models(1)]
    assert not np.array_equal(want[0][0], want[1][0]) and not np.array_equal(want[0][0], want[0][1])
    F = mpk.bilu4(nb, bp, bc, values[0], fill=fill, order=order)
    db = _dev(b)

    def check(variant, what):
        dx = _poisoned(n)
        F.solve(dx, db)
        assert_bit_equal(dx.cpu().numpy(), want[variant][1], f"{what}: the double solve")
        dx = _poisoned(n)
        F.exact("f32").solve(dx, db)
        _same(dx.cpu().numpy(), want[variant][0], f"{what}: the f32 exact solve")

    try:
        check(0, "as created")
        F.refactor(values[1])
        check(1, "after refactor(host values)")
        F.refactor(values[0])
        check(0, "after refactor back")
        F.prepare_dev()
        F.refactor_dev(_dev(values[1]))
        F.factor_status()
        check(1, "after refactor_dev")
        assert F.sweep_info_f32()["convert_launches"] == 4
    finally:
        F.close()


def test_the_f32_exact_solve_is_level_by_level_whatever_the_form():
    from navierstokes_amd import mpk
    name, fill = "fe:6", 0
    nb, bp, bc, bv = _matrix(name)
    fac = _factor(name, fill)
    n = 4 * nb
    b = np.random.default_rng(9).standard_normal(n)
    want = _model_f32(nb, fac, b)
    F = mpk.bilu4(nb, bp, bc, bv, fill=fill)
    try:
        launches = _level_launches(F)
        assert launches > 1
        assert F.set_form(1) == 1 and F.info()["launches"] == 1
        db, dx = _dev(b), _poisoned(n)
        F.exact("f32").solve(dx, db)
        _same(dx.cpu().numpy(), want, "on a handle in form 1")
        assert F.exact_info_f32() == dict(launches_last=launches, wide_launches_last=0)
        assert F.info()["form"] == 1 and F.info()["launches"] == 1, "the double solve keeps its form"
        dx = _poisoned(n)
        F.solve(dx, db)
        F.one_status()
        assert_bit_equal(dx.cpu().numpy(), M.solve(nb, *fac, b), "the double solve in form 1")
    finally:
        F.close()


def test_an_overflow_does_not_block_the_solve():
    from navierstokes_amd import mpk
    name = "sp_overflow"
    nb, bp, bc, bv = SC.matrix(name)
    fac = _factor(name, 0)
    n = 4 * nb
    b = np.random.default_rng(3).standard_normal(n)
    want = _model_f32(nb, fac, b)
    assert not np.isfinite(want[:4]).all() and np.isfinite(want[4:]).all(), "block row 0 is the sink that holds the planted values"
    F = mpk.bilu4(nb, bp, bc, bv, fill=0)
    try:
        dx = _poisoned(n)
        F.exact("f32").solve(dx, _dev(b))
        got = dx.cpu().numpy()
        _same(got, want, name)
        assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(np.isfinite(got), np.isfinite(want))
        with pytest.raises(mpk.MiError) as e:
            F.sweep_status_f32()
        assert e.value.status == 1 and "block row 0" in str(e.value), str(e.value)
        assert (e.value.bad_block_row, e.value.overflowed) == (0, 2)
        dx = _poisoned(n)
        F.solve(dx, _dev(b))
        assert_bit_equal(dx.cpu().numpy(), M.solve(nb, *fac, b), "the double solve never reads the copy")
    finally:
        F.close()


def test_a_graph_of_refactor_and_f32_exact_solve_follows_its_values():
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
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        F.refactor_dev(dcoef)
        F.exact("f32").solve(dx, db)
    try:
        for k, variant in enumerate((1, 0)):
            b = rng.standard_normal(n)
            db.copy_(_dev(b))
            dcoef.copy_(_dev(SC.new_values(name, variant) if variant else bv))
            dx.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            _same(dx.cpu().numpy(), _model_f32(nb, _factor(name, 0, variant), b), f"replay {k}")
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
            F.exact("f32").solve(dx, db)
    assert e.value.status == 6 and "not prepared" in str(e.value)
    assert F.sweep_info_f32()["prepared"] is False and F.exact_info_f32()["launches_last"] == 0
    g.replay()  # the capture ended valid: its one node runs
    torch.cuda.synchronize()
    assert (dx.cpu().numpy() == 1.0).all()
    F.exact("f32").solve(dx, db)  # outside the capture the same call prepares and solves
    _same(dx.cpu().numpy(), _model_f32(nb, fac, b), "after the refused capture")
    assert F.sweep_info_f32()["prepared"] is True
    F.close()


GMRES_CASES = [(name, order, restart) for name in ("fe:6", "fe:10") for order in ("natural", "colour") for restart in (5, 30)]
RTOL, MAXITER = 1e-8, 60


def _solve(S, b, x0, **kw):
    import torch
    x = x0.clone()
    its, hist, reason = S.solve(b, x, rtol=RTOL, maxiter=MAXITER, **kw)
    torch.cuda.synchronize()
    return its, hist, reason, x.cpu().numpy()


def _assert_same_solve(got, want, what):
    assert (got[0], got[2]) == (want[0], want[2]), (what, got[0], got[2], want[0], want[2])
    assert len(got[1]) == got[0] + 1
    assert_bit_equal(got[1], want[1], f"{what}: history")
    assert_bit_equal(got[3], want[3], f"{what}: x")


@pytest.mark.parametrize("name,order,restart", GMRES_CASES, ids=[f"{n}-{o}-restart{r}" for n, o, r in GMRES_CASES])
def test_gmres_with_the_f32_exact_solve_is_gmres_with_the_f32_sweeps_at_the_clamp(name, order, restart):
    import torch
    from navierstokes_amd import mpk
    nb, bp, bc, bv = C.matrix(name)
    n = 4 * nb
    A = mpk.bcsr4x4_matrix(nb, bp, bc, bv)
    F = mpk.bilu4(nb, bp, bc, bv, fill=0, order=order)
    b, x0 = _dev(np.sin(0.37 * np.arange(n)) + 0.5), _dev(np.zeros(n))
    try:
        sw = F.sweep_info()
        Ssw = mpk.gmres_solver(A, F.sweeps(sw["max_fwd"], sw["max_bwd"], precision="f32"), restart)
        want = _solve(Ssw, b, x0, check_every=1)
        Ssw.close()
        assert want[0] >= 2 and want[2] in (1, 2), want[:3:2]
        S = mpk.gmres_solver(A, F.exact("f32"), restart)
        assert F.sweep_info_f32()["prepared"], "mi_gmres_set_precond_ex prepares the copy"
        for check_every in (1, 3):
            _assert_same_solve(_solve(S, b, x0, check_every=check_every), want, f"{name} {order} restart {restart}: check_every {check_every}")
        assert F.exact_info_f32()["launches_last"] == _level_launches(F)
        for segment in (1, restart):
            x = x0.clone()
            P = S.plan(b, x, rtol=RTOL, maxiter=MAXITER, segment=segment)
            its, hist, reason = P.solve()
            torch.cuda.synchronize()
            got = its, hist, reason, x.cpu().numpy()
            P.close()
            _assert_same_solve(got, want, f"{name} {order} restart {restart}: planned, segment {segment}")
        # one captured cycle against the eager solve that is allowed one cycle's steps
        x = x0.clone()
        its1, hist1, reason1 = S.solve(b, x, rtol=RTOL, maxiter=restart, check_every=1)
        torch.cuda.synchronize()
        first = x.cpu().numpy()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            S.prepare_stream()
        side.synchronize()
        x.copy_(x0)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            S.cycle(b, x, True, RTOL, restart)
        g.replay()
        st = S.state()  # (behind the replay, on the stream it was launched on)
        torch.cuda.synchronize()
        assert st["its"] == its1 == st["k"], (st, its1)
        assert_bit_equal(st["history"], hist1[1:], "a captured cycle: history")
        assert_bit_equal(x.cpu().numpy(), first, "a captured cycle: x")
        # the function it stands behind still does not know the kind
        L = mpk.lib()
        assert L.mi_gmres_set_precond(S.handle, F.handle, 3, 0, 0) == 1 and "kind" in L.mi_last_error().decode()
        S.close()
    finally:
        F.close()
        A.close()
