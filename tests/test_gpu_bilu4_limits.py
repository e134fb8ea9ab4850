"""mi_bilu4_solve_dev at every limit of its schedule, bit for bit against the model (tests/bilu4_model.py).  A workgroup of the
solve serves 64 block rows: a level of fewer is folded with its narrow neighbours into one launch of bilu4_folded (one workgroup,
a barrier between levels), a level of 64 or more is one launch of bilu4_level on ceil(rows / 64) workgroups.  The layered cases of
tests/bilu4_cases.py prescribe their level widths (asserted here, per case, before anything relies on them):

  limits:0 / limits:3   widths 1, 63, 64, 65, 1, 1, 128, 129, 2, 63, 64, 200, 1 (0 / 3 far links per row): the widest level that
                        folds and the narrowest that does not, side by side; workgroups exactly full and one row over, at one and
                        at two workgroups (64, 65, 128, 129); folded runs of 1, 2 and 3 levels between wide ones; a wide level
                        first in the backward sweep and last in the forward one; 10 launches per sweep; rows of 128 and 200
                        off-diagonal blocks in one sweep (the look-ahead of bilu4_row clamps at the row's last block); with far
                        links, rows that read what earlier launches and many barriers before wrote
  wide:63 / 64 / 65     one level: the largest folded one, the first workgroup of a launch that is exactly full, one row over
  fold_deep             252 layers of widths 1 + 5 i mod 63 (every slot count from 1 to 63, all four waves), 2 far links per row:
                        ONE launch per sweep, 252 barriers, rows reading what other waves wrote one and many levels earlier
  alternating           63, 64 repeated 24 times: 48 launches per sweep, every launch boundary a switch between the two kernels
  fold_huge             1500 layers of the fold_deep kind, 48 006 block rows, one launch per sweep (factor values read back from
                        the handle: the model's own factorisation of this size takes minutes)

tests/test_gpu_bilu4.py runs its whole battery on each of them through ALL_CASES (except fold_huge).  This file adds what that
battery does not do: the launch plan the handle reports, x filled with NaN before every solve (a row no lane served shows), a
solve captured into a graph and replayed with other right-hand sides and after a refactor (the solve allocates and synchronises
nothing; refactor writes into the same device buffers), b and x misaligned independently (AL is chosen from x alone), one handle on
two streams at once, column-major blocks on a device handle.  Wall time of the file on an MI355X: 28 s, most of it the model."""
import time

import numpy as np
import pytest

import bilu4_cases as C
import bilu4_model as M
from conftest import assert_bit_equal
from test_gpu_bilu4 import _model_solve, _rhs, _same

pytestmark = pytest.mark.gpu


def _handle(name):
    """(handle, nb, model factor, (forward, backward) model schedule), the prescribed level widths asserted on both sides."""
    from navierstokes_amd import mpk
    nb, bp, bc, bv = C.matrix(name)
    fac = C.model_factor(name, 0)
    assert not isinstance(fac, M.ZeroPivot), f"{name} must factor"
    ptr, col, diag, _ = fac
    sched = M.schedule(nb, ptr, col, diag, False), M.schedule(nb, ptr, col, diag, True)
    C.assert_layered_levels(name, sched[0]["sizes"], sched[1]["sizes"])
    pr = mpk.bilu4_plan_probe(nb, bp, bc, 0)
    C.assert_layered_levels(name, pr["fwd_sizes"], pr["bwd_sizes"])
    return mpk.bilu4(nb, bp, bc, bv, fill=0), nb, fac, sched


def _nan(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("case", C.LAYERED_CASES + C.WIDE_CASES, ids=C.case_id)
def test_launch_plan_and_solve(case):
    name, _ = case
    F, nb, fac, sched = _handle(name)
    info = F.info()
    assert info["launches"] == sched[0]["launches"] + sched[1]["launches"]
    assert (info["fwd_levels"], info["bwd_levels"]) == (sched[0]["nlev"], sched[1]["nlev"])
    rhs = _rhs(nb)
    for k in ("ones", "random", "edge"):
        want = M.solve(nb, *fac, rhs[k], sched)
        dx = _nan(4 * nb)
        F.solve(dx, _dev(rhs[k]))
        _same(dx.cpu().numpy(), want, f"{name} b={k}")
    F.close()


@pytest.mark.parametrize("name", ["limits:3", "fold_deep"])
def test_captured_solve_replays_with_new_b_and_after_refactor(name):
    """One solve captured on a side stream (a straight chain of launches), replayed with two other contents of b, then after
    refactor(): each replay gives the model's solve with the factor current at replay time."""
    import torch
    F, nb, fac, sched = _handle(name)
    n = 4 * nb
    rhs = _rhs(nb)
    db, dx = _dev(rhs["ones"]).clone(), _nan(n)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        F.solve(dx, db)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _same(dx.cpu().numpy(), M.solve(nb, *fac, rhs["ones"], sched), f"{name} before capture")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        F.solve(dx, db)
    for k in ("random", "edge"):
        db.copy_(_dev(rhs[k]))
        dx.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        _same(dx.cpu().numpy(), M.solve(nb, *fac, rhs[k], sched), f"{name} replay with b={k}")
        assert_bit_equal(db.cpu().numpy(), rhs[k], "b was written")
    fac2 = C.model_factor(name, 0, 1)
    assert not isinstance(fac2, M.ZeroPivot)
    F.refactor(C.new_values(name, 1))
    for k in ("edge", "x_sin"):  # the b of the last replay, untouched, and a new one
        db.copy_(_dev(rhs[k]))
        dx.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        _same(dx.cpu().numpy(), M.solve(nb, *fac2, rhs[k], sched), f"{name} replay after refactor, b={k}")
    del g
    F.close()


def test_b_and_x_misaligned_independently():
    """Vectors 8 bytes off a 16-byte boundary: b alone, x alone, both, and in place at an offset."""
    import torch
    name = "limits:3"
    F, nb, fac, sched = _handle(name)
    n = 4 * nb
    rhs = _rhs(nb)
    want = M.solve(nb, *fac, rhs["edge"], sched)
    for off_b, off_x in ((1, 0), (0, 1), (1, 1)):
        bb = torch.zeros(n + 2, dtype=torch.float64, device="cuda")
        xx = _nan(n + 2)
        assert bb.data_ptr() % 16 == 0 and xx.data_ptr() % 16 == 0
        b, x = bb[off_b:off_b + n], xx[off_x:off_x + n]
        b.copy_(_dev(rhs["edge"]))
        F.solve(x, b)
        _same(x.cpu().numpy(), want, f"{name} b off by {8 * off_b} bytes, x off by {8 * off_x}")
        assert_bit_equal(b.cpu().numpy(), rhs["edge"], "b was written")
        rest = torch.cat([xx[:off_x], xx[off_x + n:]]).cpu().numpy()
        assert np.isnan(rest).all(), "x was written outside its n entries"
    xx = _nan(n + 2)
    xx[1:n + 1].copy_(_dev(rhs["edge"]))
    F.solve(xx[1:n + 1], xx[1:n + 1])
    _same(xx[1:n + 1].cpu().numpy(), want, f"{name} in place at an offset of 8 bytes")
    assert np.isnan(xx[0].item()) and np.isnan(xx[n + 1].item())
    F.close()


@pytest.mark.parametrize("name", ["limits:3", "fold_deep"])
def test_one_handle_on_two_streams(name):
    """Two right-hand sides through one handle on two streams, enqueued with no synchronise between them: the handle holds no
    state a solve writes (x is the only working storage), so both results are the model's."""
    import torch
    F, nb, fac, sched = _handle(name)
    rhs = _rhs(nb)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    b1, b2 = _dev(rhs["random"]), _dev(rhs["edge"])
    x1, x2 = _nan(4 * nb), _nan(4 * nb)
    torch.cuda.synchronize()
    for _ in range(3):
        with torch.cuda.stream(s1):
            F.solve(x1, b1)
        with torch.cuda.stream(s2):
            F.solve(x2, b2)
    torch.cuda.synchronize()
    _same(x1.cpu().numpy(), M.solve(nb, *fac, rhs["random"], sched), f"{name} stream 1")
    _same(x2.cpu().numpy(), M.solve(nb, *fac, rhs["edge"], sched), f"{name} stream 2")
    F.close()


@pytest.mark.parametrize("name", ["limits:0", "fe_perm:6"])
def test_column_major_blocks_on_a_device_handle(name):
    """Column-major create and refactor on a handle with a device factor: the same solve bits as row-major (and the model)."""
    from navierstokes_amd import mpk
    nb, bp, bc, bv = C.matrix(name)
    col = lambda v: np.ascontiguousarray(np.asarray(v).reshape(-1, 4, 4).transpose(0, 2, 1)).reshape(-1)
    b = _rhs(nb)["edge"]
    Fr = mpk.bilu4(nb, bp, bc, bv, fill=0)
    Fc = mpk.bilu4(nb, bp, bc, col(bv), fill=0, layout="col")
    for variant in (0, 1):
        if variant:
            Fr.refactor(C.new_values(name, 1))
            Fc.refactor(col(C.new_values(name, 1)))
        want = _model_solve(C.model_factor(name, 0, variant), nb, b)
        xr, xc = _nan(4 * nb), _nan(4 * nb)
        Fr.solve(xr, _dev(b))
        Fc.solve(xc, _dev(b))
        _same(xr.cpu().numpy(), want, f"{name} row-major, values {variant}")
        _same(xc.cpu().numpy(), want, f"{name} column-major, values {variant}")
    Fr.close()
    Fc.close()


def test_fold_huge_one_launch_per_sweep():
    """1500 layers of widths 1 + 5 i mod 63 with one far link per row: 48 006 block rows, every level narrow, so each sweep is ONE
    launch of bilu4_folded with 1500 barriers.  The factor VALUES are read back from the handle (mi_bilu4_factor_host;
    tests/test_bilu4_factor.py pins them to the model on the smaller cases, fold_deep among them); pattern, schedule and solve are
    the model's.  Model run time: printed."""
    from navierstokes_amd import mpk
    widths, extra, seed = C.FOLD_HUGE
    nb, bp, bc, bv = C.layered(widths, extra, seed)
    F = mpk.bilu4(nb, bp, bc, bv, fill=0)
    info = F.info()
    assert nb == 48006 and info["launches"] == 2 and (info["fwd_levels"], info["bwd_levels"]) == (1500, 1500)
    ptr, col, diag, val = F.factor_host()
    t0 = time.time()
    mp, mc, md = M.symbolic(nb, bp, bc, 0)
    assert np.array_equal(ptr, mp) and np.array_equal(col, mc) and np.array_equal(diag, md)
    sched = M.schedule(nb, mp, mc, md, False), M.schedule(nb, mp, mc, md, True)
    assert list(sched[0]["sizes"]) == list(widths) and list(sched[1]["sizes"]) == list(widths)[::-1]
    assert sched[0]["launches"] == 1 and sched[1]["launches"] == 1
    b = _rhs(nb)["edge"]
    want = M.solve(nb, mp, mc, md, val, b, sched)
    print(f"model (symbolic + schedule + solve) of fold_huge: {time.time() - t0:.1f} s; {info['us_per_level_launches']:.1f} us per solve at create")
    dx = _nan(4 * nb)
    F.solve(dx, _dev(b))
    _same(dx.cpu().numpy(), want, "fold_huge")
    F.close()
