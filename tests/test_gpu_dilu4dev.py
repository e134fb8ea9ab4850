"""mi_dilu4dev_refactor — the block DILU's pivots recomputed on the GPU from values on the device — against the model
(tests/dilu4_model.py) and the host path, bit for bit (uint64 views).  The device state is read back with fetch_dev() / fetch(), and
the three operations show that the level-major triangles were rewritten, not only the pivots.

  bits           created with the first values, then refactor_dev(second values): fetch() and to_hat / from_hat / apply_hat equal the
                 model's with the second values; refactor_dev(first values) gives the first pivots again; info_dev() is the probe.
                 The cases: the sweep cases of tests/test_gpu_dilu4.py, every case of tests/dilu4_limit_cases.py and the three
                 dropped cases of tests/dilu4dev_cases.py (L blocks without a mate) in both orders.  Level widths are asserted
                 first where a case is named for them; test_the_cases_meet_the_limits says what they meet between them
  column-major   the values transposed per block, on a layout="col" handle, give the same bits
  unaligned      d_coef 8 bytes off a 16-byte boundary
  refused pivot  the row and the message of the host path, on a natural and on a colour handle (the caller's row); the first LEVEL
                 with a refusal decides, folded and with a launch of its own; the threshold; a repaired refactor
  NaN            a NaN in an L block reaches the entries of Einv and K it reaches on the host, and no others
  both paths     device, host and device refactors interleaved on one handle
  stream, graph  refactor_dev + apply_hat on a side stream, then captured as one graph and replayed with other values and inputs
  Newton step    update of A's values, refactor_dev, r = b - A x0, to_hat, one GMRES cycle on the DILU operator, from_hat and the
                 update of x captured as ONE graph; replayed with the second values it equals the eager sequence on fresh handles
  gmres          dilu4.gmres after refactor_dev equals the solve on a handle created with those values"""
import ctypes
import functools

import numpy as np
import pytest

import bilu4_cases as C
import bilu4_order_cases as OC
import bilu4_wide_cases as W
import dilu4_limit_cases as LC
import dilu4_model as DM
import dilu4dev_cases as DC
import test_gpu_dilu4 as T4
import test_gpu_dilu4_limits as TL
from conftest import assert_bit_equal
from test_gpu_bilu4 import _same

pytestmark = pytest.mark.gpu
MI_ERR_ARG = 1
OPS = ("to_hat", "from_hat", "apply_hat")
ORDERS = ("natural", "colour")


@functools.lru_cache(maxsize=None)
def _dropped_expected(name, order, variant=0):
    m = DC.model(name, order, variant)
    u = np.random.default_rng(300).uniform(-1.0, 1.0, 4 * m.nb)
    out = {op: getattr(m, op)(u) for op in OPS}
    for v in (u, *out.values()):
        v.setflags(write=False)
    return u, out


# kind -> (matrix, values(name, variant), model(name, order, variant), expected(name, order, variant) = (u, {op: result}));
# the expectations are those the tests of the sweeps compute, shared through their caches
KINDS = {
    "sweep": (OC.matrix, OC.values, T4.model, lambda n, o, v: T4.expected(n, o, v)),
    "limit": (LC.matrix, LC.values, LC.model, TL.expected),
    "dropped": (DC.dropped, DC.values, DC.model, _dropped_expected),
}
BIT_CASES = ([("sweep", n, o) for n, o in T4.SWEEP_CASES] + [("limit", n, o) for n in LC.NAMES for o in ORDERS] +
             [("dropped", n, o) for n in DC.NAMES for o in ORDERS])


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()  # (a copy: the shared values are read-only)


def _nan(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def _col(v):
    return np.ascontiguousarray(np.asarray(v).reshape(-1, 4, 4).transpose(0, 2, 1)).reshape(-1)


def _handle(kind, name, order, variant=0, **kw):
    from navierstokes_amd import mpk
    matrix, values = KINDS[kind][:2]
    nb, bp, bc, _ = matrix(name)
    return mpk.dilu4(nb, bp, bc, np.asarray(values(name, variant)), order=order, **kw)


def _assert_pivots(E, m, what):
    einv, k = E.fetch()
    weinv, wk = m.fetch()
    assert_bit_equal(einv, weinv, f"{what}: Einv")
    assert_bit_equal(k, wk, f"{what}: K")


def _assert_ops(E, u, want, what):
    du = _dev(u)
    for op in OPS:
        out = _nan(u.size)
        getattr(E, op)(out, du)
        assert_bit_equal(out.cpu().numpy(), want[op], f"{what}: {op}")


def _probe(B):
    from navierstokes_amd import mpk
    return mpk.bilu4_plan_probe(B.nb, B.ptr, B.col, 0)


def _assert_named_widths(kind, name, order, fwd):
    """The level widths a case is named for, of the forward sweep the refactor follows."""
    fwd = list(fwd)
    if order != "natural":
        return
    if name == "wide":
        assert fwd == list(W.WIDTHS)
    elif name == "limits:0" or name == "limits:3":
        assert fwd == list(C.LIMITS_WIDTHS)
    elif name == "limits:3~":
        assert fwd == list(C.LIMITS_WIDTHS)[::-1]
    elif name == "fold_deep":
        assert len(fwd) == C.FOLD_DEEP_LAYERS and max(fwd) < 64
    elif name == "alternating":
        assert fwd == list(C.ALTERNATING_WIDTHS)
    elif name.startswith("wide:"):
        assert fwd == [int(name.partition(":")[2])]
    elif name.startswith("tiny:"):
        assert fwd == [1] * int(name.partition(":")[2])


# ---------------------------------------------------------------- bits

def test_the_cases_meet_the_limits():
    """Between them the bit cases hold: folded runs of 1 and of 252 levels; unfolded levels of 64, 65, 128, 129 and 200 rows (the
    16-rows-per-workgroup launches exactly full and one group over) beside folded ones of 63; a change of kernel at every launch;
    rows of 0 to 13 and of 64 to 203 L blocks; and in the dropped cases every mate position (tests/dilu4dev_cases.py's census)."""
    from navierstokes_amd import mpk
    widths, folded_runs, l_counts = set(), set(), set()
    for kind, name, order in BIT_CASES:
        B = KINDS[kind][2](name, order).B
        pr = _probe(B)
        sizes = list(pr["fwd_sizes"])
        widths |= set(sizes)
        l_counts |= set((np.asarray(B.diag) - np.asarray(B.ptr[:-1])).tolist())
        run = 0
        for s in sizes + [64]:  # (a wide level ends a run)
            if s < 64:
                run += 1
            elif run:
                folded_runs.add(run)
                run = 0
    assert {1, 252} <= folded_runs, sorted(folded_runs)
    assert {63, 64, 65, 128, 129, 200} <= widths
    assert set(range(14)) | {64, 65, 67, 68, 200, 203} <= l_counts, sorted(l_counts)
    alt = mpk.dilu4dev_plan_probe(*LC.matrix("alternating")[:3], "natural")
    assert alt["launches"] == len(C.ALTERNATING_WIDTHS) + 1  # every level a launch of its own: folded, unfolded, folded, ..
    for name in DC.NAMES:
        DC.assert_census(name)


@pytest.mark.parametrize("kind,name,order", BIT_CASES, ids=[f"{k}-{n}-{o}" for k, n, o in BIT_CASES])
def test_device_pivots_and_triangles_equal_the_model(kind, name, order):
    from navierstokes_amd import mpk
    matrix, values, model, expected = KINDS[kind]
    nb, bp, bc, _ = matrix(name)
    m0, m1 = model(name, order, 0), model(name, order, 1)
    _assert_named_widths(kind, name, order, _probe(m0.B)["fwd_sizes"])
    u, want1 = expected(name, order, 1)
    E = _handle(kind, name, order)
    try:
        assert E.info_dev()["prepared"] is False
        assert E.refactor_dev(_dev(values(name, 1))).factor_status().fetch_dev() is E
        what = f"{name} {order}"
        _assert_pivots(E, m1, f"{what}: device refactor with the second values")
        _assert_ops(E, u, want1, f"{what}: after the device refactor")
        probe = mpk.dilu4dev_plan_probe(nb, bp, bc, order)
        assert E.info_dev() == dict(prepared=True, launches=probe["launches"], plan_bytes=probe["plan_bytes"])
        E.refactor_dev(_dev(values(name, 0))).factor_status().fetch_dev()
        _assert_pivots(E, m0, f"{what}: device refactor with the first values again")
        if nb:
            assert not np.array_equal(m0.fetch()[0], m1.fetch()[0])
    finally:
        E.close()


@pytest.mark.parametrize("kind,name,order", [("dropped", "limits:3~", "colour"), ("sweep", "fe:6", "natural")])
def test_column_major_values_give_the_same_bits(kind, name, order):
    _, values, model, expected = KINDS[kind]
    u, want1 = expected(name, order, 1)
    from navierstokes_amd import mpk
    nb, bp, bc, _ = KINDS[kind][0](name)
    E = mpk.dilu4(nb, bp, bc, _col(values(name, 0)), layout="col", order=order)
    E.refactor_dev(_dev(_col(values(name, 1)))).factor_status().fetch_dev()
    _assert_pivots(E, model(name, order, 1), f"{name} {order}: column-major on the device")
    _assert_ops(E, u, want1, f"{name} {order}: column-major on the device")
    E.close()


@pytest.mark.parametrize("kind,name,order", [("dropped", "wide", "natural"), ("limit", "limits:3", "colour")])
def test_values_eight_bytes_off_a_sixteen_byte_boundary(kind, name, order):
    import torch
    _, values, model, expected = KINDS[kind]
    vals = np.asarray(values(name, 1))
    E = _handle(kind, name, order)
    buf = torch.zeros(vals.size + 2, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[1:-1].copy_(_dev(vals))
    E.refactor_dev(buf[1:-1]).factor_status().fetch_dev()
    _assert_pivots(E, model(name, order, 1), f"{name} {order}: values offset by 8 bytes")
    u, want1 = expected(name, order, 1)
    _assert_ops(E, u, want1, f"{name} {order}: values offset by 8 bytes")
    assert_bit_equal(buf[1:-1].cpu().numpy(), vals, "the values were written")
    E.close()


# ---------------------------------------------------------------- refused pivots

def _refusal(E, values):
    from navierstokes_amd import mpk
    E.refactor_dev(_dev(values))
    with pytest.raises(mpk.MiError) as e:
        E.factor_status()
    assert e.value.status == MI_ERR_ARG and "zero pivot" in str(e.value)
    return str(e.value)


@pytest.mark.parametrize("order", ORDERS)
def test_a_refused_pivot_is_reported_with_the_caller_s_block_row(order):
    """Block row 37 of the chain is all zero: E_37 = 0 whatever the order (in colour order row 37 is not row 37 of B)."""
    from navierstokes_amd import mpk
    nb, bp, bc, bv = C.matrix("chain")
    v = np.array(bv).reshape(-1, 4, 4)
    v[bp[37]:bp[38]] = 0.0
    E = mpk.dilu4(nb, bp, bc, bv, order=order)
    H = mpk.dilu4(nb, bp, bc, bv, order=order, host_only=True)
    if order == "colour":
        assert E.info()["perm"][37] != 37
    with pytest.raises(mpk.MiError) as h:
        H.refactor(v.reshape(-1))
    msg = _refusal(E, v.reshape(-1))
    assert "block row 37" in msg and msg == str(h.value)
    bad = ctypes.c_int(-5)
    assert mpk.lib().mi_dilu4dev_status(E.handle, ctypes.byref(bad)) == MI_ERR_ARG and bad.value == 37
    # after a good refactor the pivots are the model's again
    E.refactor_dev(_dev(bv)).factor_status().fetch_dev()
    _assert_pivots(E, DM.Ordered(nb, bp, bc, bv, order), "after a repaired device refactor")
    assert mpk.lib().mi_dilu4dev_status(E.handle, ctypes.byref(bad)) == 0 and bad.value == -1
    E.close()
    H.close()


def test_status_before_any_device_refactor_is_ok():
    from navierstokes_amd import mpk
    E = _handle("sweep", "arrow", "colour")
    bad = ctypes.c_int(-5)
    assert mpk.lib().mi_dilu4dev_status(E.handle, ctypes.byref(bad)) == 0 and bad.value == -1
    assert E.prepare_dev().prepare_dev().info_dev()["prepared"] is True
    assert mpk.lib().mi_dilu4dev_status(E.handle, ctypes.byref(bad)) == 0 and bad.value == -1
    E.close()


def test_the_pivot_threshold_is_the_host_s():
    from navierstokes_amd import mpk
    E = mpk.dilu4(1, [0, 1], [0], np.eye(4).reshape(-1), order="natural")
    for d, ok in ((1.5e-12, True), (0.5e-12, False), (-0.5e-12, False)):
        blk = np.eye(4)
        blk[2, 2] = d
        if ok:
            H = mpk.dilu4(1, [0, 1], [0], blk.reshape(-1), order="natural", host_only=True)
            E.refactor_dev(_dev(blk.reshape(-1))).factor_status().fetch_dev()
            for got, want in zip(E.fetch(), H.fetch()):
                assert_bit_equal(got, want, f"pivot {d}")
            H.close()
        else:
            assert "block row 0" in _refusal(E, blk.reshape(-1))
    E.close()


@pytest.mark.parametrize("wide", [False, True], ids=["folded", "launches"])
def test_the_first_level_with_a_refusal_decides_the_row(wide):
    """Row 1 (level 1: it has an L block to row 0) and a higher-numbered row of level 0 both have a zero diagonal block.  The host
    stops after level 0 and reports that row, not the lower-numbered row 1.  folded: 4 block rows, one launch, the refusal ends the
    run at its barrier; launches: level 0 is 70 rows wide — a launch of its own — and the launch of level 1 must find it refused."""
    from navierstokes_amd import mpk
    nb, other = (71, 50) if wide else (4, 2)
    rows = [{i} for i in range(nb)]
    rows[1].add(0)
    nb, bp, bc, bv = C._from_rows(rows, 91)
    sizes = mpk.bilu4_plan_probe(nb, bp, bc, 0)["fwd_sizes"]
    assert list(sizes) == [nb - 1, 1] and mpk.dilu4dev_plan_probe(nb, bp, bc, "natural")["launches"] == (3 if wide else 2)
    v = np.array(bv).reshape(-1, 4, 4)
    v[bp[1]:bp[2]] = 0.0
    v[bp[other]] = 0.0
    H = mpk.dilu4(nb, bp, bc, bv, order="natural", host_only=True)
    with pytest.raises(mpk.MiError) as h:
        H.refactor(v.reshape(-1))
    assert f"block row {other}" in str(h.value)
    E = mpk.dilu4(nb, bp, bc, bv, order="natural")
    assert _refusal(E, v.reshape(-1)) == str(h.value)
    H.refactor(bv)
    E.refactor_dev(_dev(bv)).factor_status().fetch_dev()
    for got, want in zip(E.fetch(), H.fetch()):
        assert_bit_equal(got, want, "after a repaired device refactor")
    E.close()
    H.close()


def test_a_nan_in_an_l_block_reaches_what_it_reaches_on_the_host():
    from navierstokes_amd import mpk
    nb, bp, bc, bv = C.matrix("chain")
    v = np.array(bv).reshape(-1, 4, 4)
    v[bp[60], 1, 3] = np.nan  # block (60, 59)
    H = mpk.dilu4(nb, bp, bc, bv, order="natural", host_only=True)
    H.refactor(v.reshape(-1))
    E = mpk.dilu4(nb, bp, bc, bv, order="natural")
    E.refactor_dev(_dev(v.reshape(-1))).factor_status().fetch_dev()
    for got, want, part in zip(E.fetch(), H.fetch(), ("Einv", "K")):
        assert np.isnan(want).any() and not np.isnan(want).all()
        _same(got.reshape(-1), want.reshape(-1), f"chain with a NaN: {part}")  # NaN payloads are not compared
    E.close()
    H.close()


# ---------------------------------------------------------------- both paths, streams, graphs

def test_device_and_host_refactors_on_one_handle():
    kind, name, order = "dropped", "alternating", "colour"
    _, values, model, expected = KINDS[kind]
    u = expected(name, order, 0)[0]
    E = _handle(kind, name, order)
    for step, (variant, device) in enumerate(((1, True), (0, False), (1, False), (0, True), (1, True))):
        if device:
            E.refactor_dev(_dev(values(name, variant)))
        else:
            E.refactor(np.asarray(values(name, variant)))
        _assert_ops(E, u, expected(name, order, variant)[1], f"step {step}: values {variant} by the {'device' if device else 'host'}")
        if device:
            E.factor_status().fetch_dev()
        _assert_pivots(E, model(name, order, variant), f"step {step}: values {variant}")
    E.close()


@pytest.mark.parametrize("kind,name,order", [("dropped", "limits:3~", "colour"), ("sweep", "fe:6", "natural")])
def test_captured_refactor_and_apply_replay_with_new_values(kind, name, order):
    import torch
    _, values, model, _ = KINDS[kind]
    n = 4 * model(name, order).nb
    us = [np.random.default_rng(40 + k).uniform(-1.0, 1.0, n) for k in range(3)]
    E = _handle(kind, name, order)
    E.prepare_dev()
    dcoef, du, dw = _dev(values(name, 0)), _dev(us[0]), _nan(n)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        E.refactor_dev(dcoef)
        E.apply_hat(dw, du)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert_bit_equal(dw.cpu().numpy(), model(name, order, 0).apply_hat(us[0]), f"{name} {order} on a side stream, before capture")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        E.refactor_dev(dcoef)
        E.apply_hat(dw, du)
    for variant in (1, 2):
        vals = np.asarray(values(name, variant))
        dcoef.copy_(_dev(vals))
        du.copy_(_dev(us[variant]))
        dw.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        m = model(name, order, variant)
        assert_bit_equal(dw.cpu().numpy(), m.apply_hat(us[variant]), f"{name} {order}: replay with values {variant}")
        assert_bit_equal(dcoef.cpu().numpy(), vals, "the values were written")
        assert_bit_equal(du.cpu().numpy(), us[variant], "the input was written")
        E.factor_status().fetch_dev()
        _assert_pivots(E, m, f"{name} {order}: replay with values {variant}")
    del g
    E.close()


def _newton_step(mpk, A, E, S, dcoef, b, x, w, r, u, restart, refresh):
    """One Newton step's linear solve with a fixed number of cycles (one), on torch's current stream, nothing allocated."""
    if refresh:
        A.update_values(dcoef)
        E.refactor_dev(dcoef)
    mpk.SpMV_BCSR(w, x, A)
    r.copy_(b)
    mpk.axpy(-1.0, w, r)
    E.to_hat(r, r)
    u.zero_()
    S.cycle(r, u, True, 1e-30, restart)
    E.from_hat(u, u)
    mpk.axpy(1.0, u, x)


@pytest.mark.parametrize("kind,name,order", [("sweep", "fe:6", "colour"), ("dropped", "wide", "colour")])
def test_a_newton_step_is_one_graph(kind, name, order):
    import torch
    from navierstokes_amd import mpk
    matrix, values, _, _ = KINDS[kind]
    nb, bp, bc, _ = matrix(name)
    n, restart = 4 * nb, 5
    rng = np.random.default_rng(8)
    b0, x0 = rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)

    def fresh(variant):
        A = mpk.bcsr4x4_matrix(nb, bp, bc, np.array(values(name, variant)))
        E = mpk.dilu4(nb, bp, bc, np.asarray(values(name, variant)), order=order)
        return A, E, mpk.gmres_solver(E, None, restart)

    work = lambda: [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(3)]
    # eagerly, on handles created from the second values: no refresh
    A1, E1, S1 = fresh(1)
    x_want = _dev(x0)
    _newton_step(mpk, A1, E1, S1, None, _dev(b0), x_want, *work(), restart, False)
    torch.cuda.synchronize()
    st_want = S1.state()
    assert st_want["k"] == restart and st_want["its"] == restart
    # captured on handles created from the first values, replayed with the second
    A, E, S = fresh(0)
    E.prepare_dev()
    dcoef, b, x = _dev(values(name, 0)), _dev(b0), _dev(x0)
    w, r, u = work()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        S.prepare_stream()
        _newton_step(mpk, A, E, S, dcoef, b, x, w, r, u, restart, True)  # (warm: whatever a first use allocates)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        _newton_step(mpk, A, E, S, dcoef, b, x, w, r, u, restart, True)
    for _ in range(2):
        dcoef.copy_(_dev(values(name, 1)))
        x.copy_(_dev(x0))
        g.replay()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            st = S.state()
        assert (st["its"], st["k"], st["done"], st["reason"]) == (st_want["its"], st_want["k"], st_want["done"], st_want["reason"]), (st, st_want)
        assert_bit_equal(st["history"], st_want["history"], f"{name} {order}: the replayed cycle's history")
        assert_bit_equal([st["last"], st["beta"]], [st_want["last"], st_want["beta"]], f"{name} {order}: the replayed cycle's state")
        assert_bit_equal(x.cpu().numpy(), x_want.cpu().numpy(), f"{name} {order}: the replayed step's x")
        assert_bit_equal(b.cpu().numpy(), b0, "b was written")
        assert_bit_equal(dcoef.cpu().numpy(), np.asarray(values(name, 1)), "the values were written")
    del g
    for o in (S, S1, E, E1, A, A1):
        o.close()


@pytest.mark.parametrize("kind,name,order", [("sweep", "fe:6", "colour"), ("dropped", "limits:3~", "natural")])
def test_gmres_after_a_device_refactor_is_the_solve_of_a_fresh_handle(kind, name, order):
    import torch
    from navierstokes_amd import mpk
    matrix, values, _, _ = KINDS[kind]
    nb, bp, bc, _ = matrix(name)
    b = np.random.default_rng(12).uniform(-1.0, 1.0, 4 * nb)
    A = mpk.bcsr4x4_matrix(nb, bp, bc, np.array(values(name, 1)))
    runs = []
    for refactored in (True, False):
        E = _handle(kind, name, order, 0 if refactored else 1)
        if refactored:
            E.refactor_dev(_dev(values(name, 1)))
        x = _dev(np.zeros_like(b))
        its, hist, reason = E.gmres(A, _dev(b), x, restart=10, rtol=1e-10, maxiter=60)
        torch.cuda.synchronize()
        runs.append((its, reason, np.array(hist), x.cpu().numpy()))
        E.close()
    got, want = runs
    assert got[:2] == want[:2] and want[0] > 0, (got[:2], want[:2])
    assert_bit_equal(got[2], want[2], f"{name} {order}: the history")
    assert_bit_equal(got[3], want[3], f"{name} {order}: x")
    A.close()
