"""mi_bilu4dev_refactor — the numeric block ILU(k) factorisation on the GPU — against the model (tests/bilu4_model.py) and the
host factorisation, bit for bit (uint64 views).  The device factor is read back with fetch_factor() / factor_host().

  bits             every case of tests/bilu4_cases.py: new values factored on the device equal the model's factor, pattern
                   included; the solve follows; a second device refactor with the first values gives the first factor.  The
                   layered and wide cases prescribe the level widths (asserted first), so every limit of the schedule is met:
                   folded runs of 1, 2, 3 and 252 levels, levels of 63 / 64 / 65 / 128 / 129 / 200 rows (the 16-rows-per-workgroup
                   launches exactly full and one row over), a switch of kernel at every launch (alternating)
  column-major     the values transposed per block give the same bits
  fold_huge        48 006 block rows in ONE folded launch with 1 500 barriers, against a host-refactored handle
  zero-block skip  an explicit all-zero (or -0.0) L block in front of an Inf is skipped, as on the host: no NaN
  NaN              a NaN in the values reaches the entries it reaches on the host, and no others
  refused pivot    the row the host reports, also when a lower-numbered row of a LATER level would refuse as well
  stream, graph    refactor + solve captured as one chain and replayed with other values and right-hand sides
  both paths       device and host refactors interleaved on one handle"""
import ctypes

import numpy as np
import pytest

import bilu4_cases as C
import bilu4_model as M
from conftest import assert_bit_equal
from test_gpu_bilu4 import _model_solve, _rhs, _same

pytestmark = pytest.mark.gpu
MI_ERR_ARG = 1


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _nan(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def _col(v):
    return np.ascontiguousarray(np.asarray(v).reshape(-1, 4, 4).transpose(0, 2, 1)).reshape(-1)


def _device_factor(F, values):
    """(ptr, col, diag, val) the device holds after refactor_dev(values)."""
    F.refactor_dev(_dev(values)).factor_status().fetch_factor()
    return F.factor_host()


def _assert_factor(got, want, what):
    for g, w, part in zip(got[:3], want[:3], ("ptr", "col", "diag")):
        assert np.array_equal(np.asarray(g), np.asarray(w)), f"{what}: {part} differs"
    assert_bit_equal(np.asarray(got[3]).reshape(-1), np.asarray(want[3]).reshape(-1), what)


def _solve(F, nb, b):
    dx = _nan(4 * nb)
    F.solve(dx, _dev(b))
    return dx.cpu().numpy()


@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_device_factor_bits_equal_the_model(case):
    from navierstokes_amd import mpk
    name, fill = case
    nb, bp, bc, bv = C.matrix(name)
    fac0, fac1 = C.model_factor(name, fill), C.model_factor(name, fill, 1)
    assert not isinstance(fac0, M.ZeroPivot) and not isinstance(fac1, M.ZeroPivot), f"{name} must factor"
    if case in C.LAYERED_CASES + C.WIDE_CASES:
        pr = mpk.bilu4_plan_probe(nb, bp, bc, fill)
        C.assert_layered_levels(name, pr["fwd_sizes"], pr["bwd_sizes"])
    F = mpk.bilu4(nb, bp, bc, bv, fill=fill)
    assert F.info_dev()["prepared"] is False
    _assert_factor(_device_factor(F, C.new_values(name, 1)), fac1, f"{name} fill {fill}: device factor of the new values")
    info, probe = F.info_dev(), mpk.bilu4dev_plan_probe(nb, bp, bc, fill)
    assert info == dict(prepared=True, launches=probe["launches"], plan_bytes=probe["plan_bytes"])
    b = _rhs(nb)["edge"]
    _same(_solve(F, nb, b), _model_solve(fac1, nb, b), f"{name} fill {fill}: solve after the device refactor")
    _assert_factor(_device_factor(F, bv), fac0, f"{name} fill {fill}: device factor of the first values again")
    F.close()


@pytest.mark.parametrize("name", ["limits:3", "fe:6"])
def test_column_major_values_give_the_same_bits(name):
    """fill 1, a handle of layout "col": against a row-major host factorisation of the same values (tests/test_bilu4_factor.py
    pins that to the model) and, where the model's factor is at hand, against the model."""
    from navierstokes_amd import mpk
    nb, bp, bc, bv = C.matrix(name)
    new = C.new_values(name, 1)
    H = mpk.bilu4(nb, bp, bc, bv, fill=1, host_only=True)
    H.refactor(new)
    want = H.factor_host()
    F = mpk.bilu4(nb, bp, bc, _col(bv), fill=1, layout="col")
    _assert_factor(_device_factor(F, _col(new)), want, f"{name}: column-major on the device")
    if (name, 1) in C.ALL_CASES:
        _assert_factor(F.factor_host(), C.model_factor(name, 1, 1), f"{name}: column-major on the device against the model")
    F.close()
    H.close()


def test_fold_huge_one_folded_launch():
    from navierstokes_amd import mpk
    widths, extra, seed = C.FOLD_HUGE
    nb, bp, bc, bv = C.layered(widths, extra, seed)
    v = np.array(bv).reshape(-1, 4, 4)
    new = v * np.random.default_rng(78).uniform(0.5, 1.5, (len(bc), 1, 1))
    isdiag = np.asarray(bc) == np.repeat(np.arange(nb), np.diff(bp))
    new[isdiag] = v[isdiag] * 1.25
    new = new.reshape(-1)
    F = mpk.bilu4(nb, bp, bc, bv, fill=0)
    assert nb == 48006 and F.info()["fwd_levels"] == 1500 and F.info_dev()["launches"] == 2
    H = mpk.bilu4(nb, bp, bc, bv, fill=0, host_only=True)
    H.refactor(new)
    _assert_factor(_device_factor(F, new), H.factor_host(), "fold_huge")
    F.close()
    H.close()


@pytest.mark.parametrize("zero", [0.0, -0.0], ids=["zero", "minus_zero"])
def test_an_all_zero_l_block_is_skipped(zero):
    """Block (2, 0) is stored and all zero (one entry -0.0 in the second matrix); block (0, 2) holds an Inf.  Not skipped, the
    update of row 2 would be 0 . Inf = NaN."""
    from navierstokes_amd import mpk
    bp, bc = np.array([0, 2, 3, 5], np.int32), np.array([0, 2, 1, 0, 2], np.int32)
    rng = np.random.default_rng(5)
    v = rng.uniform(-1.0, 1.0, (5, 4, 4))
    for k in (0, 2, 4):
        v[k] += 8.0 * np.eye(4)
    good = v.copy()
    v[1, 1, 2] = np.inf
    v[3] = 0.0
    v[3, 2, 1] = zero
    H = mpk.bilu4(3, bp, bc, v.reshape(-1), host_only=True)
    want = H.factor_host()
    F = mpk.bilu4(3, bp, bc, good.reshape(-1))
    got = _device_factor(F, v.reshape(-1))
    assert not np.isnan(got[3][got[0][2]:got[0][3]]).any(), "NaN in block row 2: the zero block was not skipped"
    assert np.isinf(got[3]).any()
    _assert_factor(got, want, "the zero-block skip")
    F.close()
    H.close()


def test_a_nan_in_the_values_reaches_what_it_reaches_on_the_host():
    from navierstokes_amd import mpk
    nb, bp, bc, bv = C.matrix("chain")
    v = np.array(bv).reshape(-1, 4, 4)
    v[bp[60], 1, 3] = np.nan  # block (60, 59)
    H = mpk.bilu4(nb, bp, bc, bv, host_only=True)
    H.refactor(v.reshape(-1))
    want = H.factor_host()[3]
    F = mpk.bilu4(nb, bp, bc, bv)
    got = _device_factor(F, v.reshape(-1))[3]
    assert np.isnan(want).any() and not np.isnan(want).all()
    _same(got.reshape(-1), want.reshape(-1), "chain with a NaN")  # NaN payloads are not compared
    F.close()
    H.close()


def _refusal(F, values):
    from navierstokes_amd import mpk
    F.refactor_dev(_dev(values))
    with pytest.raises(mpk.MiError) as e:
        F.factor_status()
    assert e.value.status == MI_ERR_ARG and "zero pivot" in str(e.value)
    return str(e.value)


def test_a_refused_pivot_is_reported_with_its_block_row():
    from navierstokes_amd import mpk
    nb, bp, bc, bv = C.matrix("chain")
    v = np.array(bv).reshape(-1, 4, 4)
    k = bp[37] + list(bc[bp[37]:bp[38]]).index(37)
    v[k] = 0.0
    v[bp[37]] = 0.0
    F = mpk.bilu4(nb, bp, bc, bv, fill=0)
    H = mpk.bilu4(nb, bp, bc, bv, fill=0, host_only=True)
    with pytest.raises(mpk.MiError) as h:
        H.refactor(v.reshape(-1))
    msg = _refusal(F, v.reshape(-1))
    assert "block row 37" in msg and msg == str(h.value)
    bad = ctypes.c_int(-5)
    assert mpk.lib().mi_bilu4dev_status(F.handle, ctypes.byref(bad)) == MI_ERR_ARG and bad.value == 37
    # after a good refactor the factor is the model's again
    _assert_factor(_device_factor(F, bv), C.model_factor("chain", 0), "after a repaired device refactor")
    assert mpk.lib().mi_bilu4dev_status(F.handle, ctypes.byref(bad)) == 0 and bad.value == -1
    F.close()
    H.close()


def test_the_pivot_threshold_is_the_host_s():
    from navierstokes_amd import mpk
    F = mpk.bilu4(1, [0, 1], [0], np.eye(4).reshape(-1))
    for d, ok in ((1.5e-12, True), (0.5e-12, False), (-0.5e-12, False)):
        blk = np.eye(4)
        blk[2, 2] = d
        if ok:
            H = mpk.bilu4(1, [0, 1], [0], blk.reshape(-1), host_only=True)
            _assert_factor(_device_factor(F, blk.reshape(-1)), H.factor_host(), f"pivot {d}")
            H.close()
        else:
            assert "block row 0" in _refusal(F, blk.reshape(-1))
    F.close()


@pytest.mark.parametrize("wide", [False, True], ids=["folded", "launches"])
def test_the_first_level_with_a_refusal_decides_the_row(wide):
    """Row 1 (level 1: it depends on row 0) and a higher-numbered row of level 0 both have a zero diagonal block.  The host stops
    after level 0 and reports that row, not the lower-numbered row 1.  folded: 4 block rows, one launch, the refusal ends the run
    at its barrier; launches: level 0 is 70 rows wide — a launch of its own — and the launch of level 1 must find it refused."""
    from navierstokes_amd import mpk
    nb, other = (71, 50) if wide else (4, 2)
    rows = [{i} for i in range(nb)]
    rows[1].add(0)
    nb, bp, bc, bv = C._from_rows(rows, 91)
    sizes = mpk.bilu4_plan_probe(nb, bp, bc, 0)["fwd_sizes"]
    assert list(sizes) == [nb - 1, 1] and mpk.bilu4dev_plan_probe(nb, bp, bc, 0)["launches"] == (3 if wide else 2)
    v = np.array(bv).reshape(-1, 4, 4)
    v[bp[1]:bp[2]] = 0.0
    v[bp[other]] = 0.0
    H = mpk.bilu4(nb, bp, bc, bv, host_only=True)
    with pytest.raises(mpk.MiError) as h:
        H.refactor(v.reshape(-1))
    assert f"block row {other}" in str(h.value)
    F = mpk.bilu4(nb, bp, bc, bv)
    assert _refusal(F, v.reshape(-1)) == str(h.value)
    H.refactor(bv)
    _assert_factor(_device_factor(F, bv), H.factor_host(), "after a repaired device refactor")
    F.close()
    H.close()


@pytest.mark.parametrize("name", ["limits:3", "fold_deep"])
def test_captured_refactor_and_solve_replay_with_new_values(name):
    import torch
    from navierstokes_amd import mpk
    nb, bp, bc, bv = C.matrix(name)
    pr = mpk.bilu4_plan_probe(nb, bp, bc, 0)
    C.assert_layered_levels(name, pr["fwd_sizes"], pr["bwd_sizes"])
    n = 4 * nb
    rhs = _rhs(nb)
    F = mpk.bilu4(nb, bp, bc, bv, fill=0)
    F.prepare_dev()
    assert F.info_dev()["prepared"] is True
    dcoef, db, dx = _dev(bv).clone(), _dev(rhs["ones"]).clone(), _nan(n)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        F.refactor_dev(dcoef)
        F.solve(dx, db)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _same(dx.cpu().numpy(), _model_solve(C.model_factor(name, 0), nb, rhs["ones"]), f"{name} on a side stream, before capture")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        F.refactor_dev(dcoef)
        F.solve(dx, db)
    for variant, k in ((1, "random"), (2, "edge")):
        vals = C.new_values(name, variant)
        dcoef.copy_(_dev(vals))
        db.copy_(_dev(rhs[k]))
        dx.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        fac = C.model_factor(name, 0, variant)
        _same(dx.cpu().numpy(), _model_solve(fac, nb, rhs[k]), f"{name} replay with values {variant}, b={k}")
        assert_bit_equal(dcoef.cpu().numpy(), vals, "the values were written")
        assert_bit_equal(db.cpu().numpy(), rhs[k], "b was written")
        F.factor_status().fetch_factor()
        _assert_factor(F.factor_host(), fac, f"{name} replay with values {variant}: the factor")
    del g
    # values 8 bytes off a 16-byte boundary
    buf = torch.zeros(len(bv) + 1, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[1:].copy_(_dev(C.new_values(name, 1)))
    F.refactor_dev(buf[1:]).factor_status().fetch_factor()
    _assert_factor(F.factor_host(), C.model_factor(name, 0, 1), f"{name} values offset by 8 bytes")
    F.close()


def test_device_and_host_refactors_on_one_handle():
    from navierstokes_amd import mpk
    name = "limits:0"
    nb, bp, bc, bv = C.matrix(name)
    b = _rhs(nb)["random"]
    F = mpk.bilu4(nb, bp, bc, bv, fill=0)
    v1, v2 = C.new_values(name, 1), C.new_values(name, 2)
    want = {k: _model_solve(C.model_factor(name, 0, k), nb, b) for k in (0, 1, 2)}
    F.refactor_dev(_dev(v1))
    _same(_solve(F, nb, b), want[1], "device refactor")
    F.refactor(v2)
    _same(_solve(F, nb, b), want[2], "host refactor after a device refactor")
    _assert_factor(F.factor_host(), C.model_factor(name, 0, 2), "the host factor after the host refactor")
    F.refactor_dev(_dev(bv))
    _same(_solve(F, nb, b), want[0], "device refactor after a host refactor")
    F.factor_status().fetch_factor()
    _assert_factor(F.factor_host(), C.model_factor(name, 0), "the fetched factor")
    F.close()
