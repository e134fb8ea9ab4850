"""The two PETSc seams on the GPU (integration/petsc_matmult_mi355.c) against what the reference's own
compiled kernels returned — tests/golden/ref_baij.npz, recorded by tests/golden/make_golden.py from oracle/_ref/libref_baij_*.so
and held to the models on the CPU by tests/test_ref_baij.py.  Every call is one a PETSc caller is told to make, every matrix and
factor input is COLUMN-major, as Mat_SeqBAIJ::a is.  Only the recording and tests/ helpers are read.

  products   bcsr4x4_matrix(layout="col") then SpMV_BCSR with device and with host vectors, again after update_values from a host
             and from a device array, with nothing forced, with the sliced copy forced (MI355_BCSR_SELL=1) and with the tiled copy
             forced (MI355_BCSR_TILE=1), so that every copy a column-major refresh writes is read.  BIT-equal to what
             MatMult_SeqBAIJ_4_FMA returned; error against a longdouble product within 10 x that of MatMult_SeqBAIJ_4_AVX2's output.
  solves     bilu4(layout="col", fill): solve in form 0 and form 1, sweeps(10**6, 10**6) (clamped, so exact), after refactor_dev with
             column-major device values, and MatSolve_SeqBAIJ_4(F, b, x) in place.  max|x - x_ld| / max|x_ld| <= 10 max(e_scalar,
             e_avx2) with the yardstick and the reference's two errors from the recording, and BIT-equal to the model's solve (also
             recorded; tests/test_ref_baij.py holds the recording to the live model): reference -> model -> GPU in one file.
  multi      MatMatMult_SeqBAIJ_4(arith="blockacc") at s = 1, 3, 4, 5, 8: the reference's kernel returns 4 A X (its horizontal
             reduction adds four lanes that hold the same sum — tests/test_ref_baij.py) with MI_ARITH_BLOCKACC's association, and
             scaling by 4 is exact: 4 x the library's Y is BIT-equal to the recording.

Not covered here: order="colour" and exact("f32") are different operators from the reference's; tests/test_gpu_bilu4_order.py and
tests/test_gpu_bilu4spx.py hold them to their own models."""
import ctypes
import functools
import os

import numpy as np
import pytest

import bilu4_cases as C
import petsc_layout as P
import ref_baij_cases as R
from conftest import GOLDEN, assert_bit_equal
from navierstokes_amd import mpk

pytestmark = pytest.mark.gpu
MARGIN = 10.0
SOLVE_CASES = [c for c in R.SOLVE_CASES if c[0] not in R.GOLDEN_SKIP]
PRODUCT_MATRICES = [m for m in R.PRODUCT_MATRICES if m not in R.GOLDEN_SKIP]
QUIET = ("MI355_SPMV_AUTOTUNE", "MI355_PLACEMENT_DRAWS", "MI355_REORDER")  # "0": nothing measured, nothing relabelled
COPIES = {"default": {}, "sliced": dict(MI355_BCSR_SELL="1", MI355_BCSR_SELL_FORM="3", MI355_REORDER="0"),
          "tiled": dict(MI355_BCSR_TILE="1", MI355_BCSR_SELL="0", **{k: "0" for k in QUIET})}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    mpk.lib()
    yield


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLDEN, "ref_baij.npz"))


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()


def nan_dev(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


# ------------------------------------------------------------------ products

def _copies_in_use(B):
    sell, tb, tu = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    mpk.check(mpk.lib().mi_bcsr4_sell_info(B.handle, ctypes.byref(sell), None, None, None, None))
    mpk.check(mpk.lib().mi_bcsr4_tile_info(B.handle, ctypes.byref(tb), ctypes.byref(tu), None, None))
    return dict(sliced=sell.value, tiled=tu.value)


# the tiled copy exists from 4096 blocks up: one matrix of the recording is that large
PRODUCT_RUNS = [(m, c) for m in PRODUCT_MATRICES for c in ("default", "sliced")] + [(R.TILED, "tiled")]


@pytest.mark.parametrize("name,copy", PRODUCT_RUNS, ids=lambda v: v)
def test_column_major_product_is_the_references_fma_kernel(name, copy, monkeypatch):
    for k, v in COPIES[copy].items():
        monkeypatch.setenv(k, v)
    nb, bp, bc, bv = R.matrix(name)
    rec = R.load_product(golden(), name)
    x = R.product_x(name)
    y_ld = R.mult_ld(nb, bp, bc, bv, x)
    bound = MARGIN * R.err(rec["y_avx2"], y_ld)
    col = P.to_petsc_blocks(bv)
    other = P.to_petsc_blocks(np.asarray(bv) * np.cos(np.arange(len(bv))))  # what a Newton step overwrites
    dx = dev(x)

    def check(B, what):
        y = nan_dev(4 * nb)
        mpk.SpMV_BCSR(y, dx, B)
        yh = np.full(4 * nb, np.nan)
        mpk.SpMV_BCSR(yh, x, B)
        for got, vec in ((y.cpu().numpy(), "device"), (yh, "host")):
            assert_bit_equal(got, rec["y_fma"], f"{name} {copy} {what}, {vec} vectors vs MatMult_SeqBAIJ_4_FMA")
            assert R.err(got, y_ld) <= bound, (name, copy, what, vec, R.err(got, y_ld), bound)

    B = mpk.bcsr4x4_matrix(nb, bp, bc, col, nbcols=nb, layout="col")
    used = _copies_in_use(B)
    if copy == "sliced" and len(bc):
        assert used["sliced"] == 1, used
    if copy == "tiled":
        assert used["tiled"] == 1, used
    check(B, "as created")
    B.update_values(other)
    y = nan_dev(4 * nb)
    mpk.SpMV_BCSR(y, dx, B)
    assert len(bc) == 0 or not np.array_equal(y.cpu().numpy(), rec["y_fma"]), "the refresh changed nothing"
    B.update_values(col)
    check(B, "after a host refresh")
    B.update_values(other)
    B.update_values(dev(col))
    check(B, "after a device refresh")
    B.close()


@pytest.mark.parametrize("name", R.SPMM_GOLDEN)
def test_multi_vector_blockacc_is_a_quarter_of_the_references_spmm(name):
    nb, bp, bc, bv = R.matrix(name)
    rec = R.load_product(golden(), name)
    B = mpk.bcsr4x4_matrix(nb, bp, bc, P.to_petsc_blocks(bv), nbcols=nb, layout="col")
    for s in R.SPMM_WIDTHS:
        X = R.product_x(name, s)
        Y = nan_dev(s, 4 * nb)
        mpk.MatMatMult_SeqBAIJ_4(B, dev(X), Y, arith="blockacc")
        assert_bit_equal(4.0 * Y.cpu().numpy(), rec["spmm"][s], f"{name} s={s}, device vectors")
        Yh = np.full((s, 4 * nb), np.nan)
        mpk.MatMatMult_SeqBAIJ_4(B, X, Yh, arith="blockacc")
        assert_bit_equal(4.0 * Yh, rec["spmm"][s], f"{name} s={s}, host vectors")
    B.close()


# ------------------------------------------------------------------ solves

def _solves(F, b, eligible):
    """{path: x} by every path of the MATOP_SOLVE seam on the handle as it stands."""
    out = {}
    db = dev(b)
    F.set_form(0)
    x = nan_dev(len(b))
    F.solve(x, db)
    out["form 0"] = x.cpu().numpy()
    xh = np.full(len(b), np.nan)
    F.solve(xh, b)
    out["form 0, host vectors"] = xh
    if eligible:
        assert F.set_form(1) == 1
        x = nan_dev(len(b))
        F.solve(x, db)
        out["form 1"] = x.cpu().numpy()
        F.set_form(0)
    x = nan_dev(len(b))
    F.sweeps(10 ** 6, 10 ** 6).solve(x, db)
    out["sweeps clamped"] = x.cpu().numpy()
    x = db.clone()
    mpk.MatSolve_SeqBAIJ_4(F, x, x)
    out["MatSolve_SeqBAIJ_4 in place"] = x.cpu().numpy()
    return out


@pytest.mark.parametrize("case", SOLVE_CASES, ids=R.case_id)
def test_column_major_solve_against_the_references_solves(case):
    name, fill = case
    nb, bp, bc, bv = C.matrix(name)
    col = P.to_petsc_blocks(bv)
    F = mpk.bilu4(nb, bp, bc, col, fill=fill, layout="col")
    try:
        F.set_form(1)
        eligible = True
    except mpk.MiError:
        eligible = False
        assert F.info_one()["eligible"] is False and F.info()["form"] == 0
    assert eligible or not name.startswith("fe"), "the FE cases run the one-launch form"
    # the same handle after a Newton step's values and back, factored on the device from column-major device values
    G = mpk.bilu4(nb, bp, bc, P.to_petsc_blocks(C.new_values(name, 1)), fill=fill, layout="col")
    G.prepare_dev()
    G.refactor_dev(dev(col)).factor_status()
    for kind, b in R.rhs(nb).items():
        rec = R.load_solve(golden(), case, kind)
        bound = MARGIN * max(rec["e_scalar"], rec["e_avx2"])
        got = _solves(F, b, eligible)
        xg = nan_dev(len(b))
        G.solve(xg, dev(b))
        got["after refactor_dev"] = xg.cpu().numpy()
        for path, x in got.items():
            e = R.err(x, rec["x_ld"])
            print(f"petsc seam solve {R.case_id(case)} {kind} {path}: e_gpu={e:.3e} e_scalar={rec['e_scalar']:.3e} e_avx2={rec['e_avx2']:.3e}")
            assert e <= bound, (R.case_id(case), kind, path, e, bound)
            assert_bit_equal(x, rec["x_model"], f"{R.case_id(case)} {kind} {path} vs the model's solve")
    F.close()
    G.close()
