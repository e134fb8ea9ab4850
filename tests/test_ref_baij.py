"""The reference's PETSc-bound solver kernels themselves (src/kernels/*.c, compiled where they lie against oracle/petsc_stub into
oracle/_ref/libref_baij_*.so) against this project's models — on the CPU, no GPU involved.  Until this module the solve and the
BAIJ products were held only to models written from include/mi355_spmv.h; a reading error shared by model and code (a block
transposed at the PETSc seam, the order of the U blocks, the side Dinv multiplies on) would have passed.

  solve      MatSolve_SeqBAIJ_4 and MatSolve_SeqBAIJ_4_AVX2 over the model's factor in PETSc's factored layout
             (tests/petsc_layout.py), three right-hand sides per case.  Yardstick: the same substitution in np.longdouble over the
             same factor values.  e = max|x - x_ld| / max|x_ld| for both reference solves and for bilu4_model.solve; asserted
             e_model <= 10 max(e_scalar, e_avx2) — ten times the reference's own spread, the margin of test_gpu_gmres.py and
             test_bilu4_factor.py.  Nothing bitwise: the scalar solve's bits depend on how its compiler contracts a*b + c.
             The rows that are NaN / Inf for one Inf and one NaN in b are the same rows.
  products   MatMult_SeqBAIJ_4_FMA is one fma chain per row across all blocks (baij4_fma.c:48-79), the chain O.spmv_bcsr4
             restates: BIT-equal.  MatMult_SeqBAIJ_4_AVX2 keeps four per-column accumulators and adds (s0 + s1) + (s2 + s3)
             (baij4_avx2.c:39-65): ref_baij_cases.avx2_mult_model, BIT-equal.  MatMult_SeqBAIJ_4 (MAD), MatMult_SeqAIJ and
             MatMult_SeqAIJ_FMA: error against a longdouble product <= 10 x the FMA kernel's; MatMult_SeqAIJ_FMA walks the same
             chain as the BAIJ FMA kernel, so it is also bit-equal to it.  Every BAIJ product also through compressedrow.
  multi      MatMatMult_SeqBAIJ_4_AVX2 at s = 1, 3, 4, 5, 8.  TWO FINDINGS about that kernel.  (1) It indexes a block as
             Ablock[4 r + c] (spmm_avx2.c:83): it reads the bytes ROW-major, while MatMult_* read the same bytes column-major —
             on a PETSc matrix it multiplies by the matrix of transposed blocks.  It is fed the row-major bytes here, which make
             it compute with A.  (2) Its accumulators hold the same value in all four lanes (every operand is a broadcast) and
             the horizontal reduction at :95-100 adds the four lanes: it returns 4 A X.  The association inside a block and
             across blocks IS MI_ARITH_BLOCKACC's (O.spmv_bcsr4_blockacc: a chain per block from zero, block sums added in
             order), and scaling by 4 is exact, so: reference == 4 x blockacc, BIT-equal.  The library computes A X.

Every comparison is also fed one deliberately wrong input on the MODEL side (blocks not transposed, Dinv transposed, the U blocks
of a row reversed) and must reject it.  The measured errors are in profiles/NOTES.md; tests/golden/make_golden.py records the
reference's outputs for tests/test_gpu_petsc_seam.py through solve_record / product_record below."""
import functools

import numpy as np
import pytest

import bilu4_cases as C
import petsc_layout as P
import ref_baij_cases as R
from conftest import assert_bit_equal
from oracle import oracle as O
from test_gpu_bilu4 import _model_solve

pytestmark = pytest.mark.skipif(not O.have_ref_baij(), reason="oracle/_ref/libref_baij_*.so not built (needs the reference at build time)")

MARGIN = 10.0


@functools.lru_cache(maxsize=None)
def solve_record(name, fill):
    """{rhs kind: dict(b, x_ld, x_scalar, x_avx2, x_model, e_scalar, e_avx2, e_model)} — computed once, read-only."""
    nb = C.matrix(name)[0]
    fac = C.model_factor(name, fill)
    assert not isinstance(fac, Exception), fac
    bi, bj, bdiag, ba = P.to_petsc_factor(*fac)
    out = {}
    for kind, b in R.rhs(nb).items():
        d = dict(b=b, x_ld=R.solve_ld(nb, *fac, b), x_scalar=O.ref_baij_solve("scalar", bi, bj, bdiag, ba, b),
                 x_avx2=O.ref_baij_solve("avx2", bi, bj, bdiag, ba, b), x_model=_model_solve(fac, nb, b))
        for k in ("scalar", "avx2", "model"):
            d["e_" + k] = R.err(d["x_" + k], d["x_ld"])
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out[kind] = d
    return out


@functools.lru_cache(maxsize=None)
def product_record(name):
    """dict(x, y_fma, y_avx2, y_mad, spmm={s: (X, Y)}) of the reference's products on a matrix of ref_baij_cases.PRODUCT_MATRICES:
    column-major bytes for MatMult_*, row-major bytes for MatMatMult (module docstring)."""
    nb, bp, bc, bv = R.matrix(name)
    x = R.product_x(name)
    col = P.to_petsc_blocks(bv)
    d = dict(x=x, spmm={})
    for kind in ("fma", "avx2", "mad"):
        d["y_" + kind] = O.ref_baij_mult(kind, bp, bc, col, x)
    for s in R.SPMM_WIDTHS:
        X = R.product_x(name, s)
        d["spmm"][s] = (X, O.ref_baij_spmm(bp, bc, bv, X))
    return d


# ------------------------------------------------------------------ solve

@pytest.mark.parametrize("case", R.SOLVE_CASES, ids=R.case_id)
def test_solve_error_within_ten_times_the_references(case):
    rec = solve_record(*case)
    for kind, d in rec.items():
        bound = MARGIN * max(d["e_scalar"], d["e_avx2"])
        print(f"ref_baij solve {R.case_id(case)} {kind}: e_scalar={d['e_scalar']:.3e} e_avx2={d['e_avx2']:.3e} e_model={d['e_model']:.3e} "
              f"ratio={d['e_model'] / max(d['e_scalar'], d['e_avx2'], 1e-300):.2f}")
        assert np.isfinite(d["e_model"]) and d["e_model"] <= bound, (R.case_id(case), kind, d["e_model"], d["e_scalar"], d["e_avx2"])


@pytest.mark.parametrize("case", R.SOLVE_CASES, ids=R.case_id)
def test_solve_in_place_and_nonfinite_rows(case):
    """The reference solves with x == b give the bits of the out-of-place call (the glue hands them ONE vector); one Inf and one NaN
    in b make the same entries NaN and the same entries +Inf / -Inf in the model's solve as in both reference solves."""
    name, fill = case
    nb = C.matrix(name)[0]
    fac = C.model_factor(name, fill)
    arrays = P.to_petsc_factor(*fac)
    b = solve_record(name, fill)["random"]["b"]
    for kind in ("scalar", "avx2"):
        assert_bit_equal(O.ref_baij_solve(kind, *arrays, b, inplace=True), solve_record(name, fill)["random"]["x_" + kind], f"{kind} in place")
    rng = np.random.default_rng(5 + nb)
    bad = np.ones(4 * nb)
    at = rng.permutation(4 * nb)[:2]
    bad[at[0]] = np.inf
    bad[at[1]] = np.nan
    xm = _model_solve(fac, nb, bad)
    assert not np.isfinite(xm[at[0]]) or nb == 0
    for kind in ("scalar", "avx2"):
        xr = O.ref_baij_solve(kind, *arrays, bad)
        assert np.array_equal(np.isnan(xm), np.isnan(xr)), (kind, np.nonzero(np.isnan(xm) != np.isnan(xr))[0][:8])
        assert np.array_equal(np.isposinf(xm), np.isposinf(xr)) and np.array_equal(np.isneginf(xm), np.isneginf(xr)), kind


WRONG_SOLVE_CASES = [("fe:3", 4), ("fe_perm:6", 1), ("random:5", 2), ("random:8", 2)]  # each has rows with two U blocks or more


def _wrong_factors(ptr, col, diag, val):
    """The three reading errors at the PETSc seam, made on purpose on the model's side."""
    val = np.asarray(val).reshape(-1, 4, 4)
    every = val.transpose(0, 2, 1).copy()
    dinv = val.copy()
    dinv[diag] = val[diag].transpose(0, 2, 1)
    rev = val.copy()
    for i in range(len(ptr) - 1):
        rev[diag[i] + 1:ptr[i + 1]] = val[diag[i] + 1:ptr[i + 1]][::-1]
    return {"blocks not transposed": every, "Dinv transposed": dinv, "U blocks of a row reversed": rev}


@pytest.mark.parametrize("case", WRONG_SOLVE_CASES, ids=R.case_id)
def test_solve_comparison_rejects_a_wrong_model(case):
    name, fill = case
    nb = C.matrix(name)[0]
    ptr, col, diag, val = C.model_factor(name, fill)
    assert (np.asarray(ptr[1:]) - np.asarray(diag) > 2).any()
    d = solve_record(name, fill)["random"]
    bound = MARGIN * max(d["e_scalar"], d["e_avx2"])
    for what, wrong in _wrong_factors(ptr, col, diag, val).items():
        e = R.err(_model_solve((ptr, col, diag, wrong), nb, d["b"]), d["x_ld"])
        assert not e <= bound, (what, e, bound)


# ------------------------------------------------------------------ products

def _both_views(kind, bp, bc, col, x):
    """The reference product with the rows as they are, and through PETSc's compressed-row view: the same bits."""
    y = O.ref_baij_mult(kind, bp, bc, col, x)
    assert_bit_equal(O.ref_baij_mult(kind, bp, bc, col, x, compressed=True), y, f"{kind}: compressedrow")
    return y


@pytest.mark.parametrize("name", R.PRODUCT_MATRICES)
def test_products_bitwise(name):
    nb, bp, bc, bv = R.matrix(name)
    rec = product_record(name)
    x, col = rec["x"], P.to_petsc_blocks(bv)
    y_fma = _both_views("fma", bp, bc, col, x)
    assert_bit_equal(y_fma, rec["y_fma"], "record")
    assert_bit_equal(O.spmv_bcsr4(bp, bc, bv, x), y_fma, "MatMult_SeqBAIJ_4_FMA vs the oracle's block chain")
    y_avx2 = _both_views("avx2", bp, bc, col, x)
    assert_bit_equal(R.avx2_mult_model(nb, bp, bc, bv, x), y_avx2, "MatMult_SeqBAIJ_4_AVX2 vs its numpy model")
    ap, ac, av = R.to_csr(nb, bp, bc, bv)
    assert_bit_equal(O.ref_aij_mult("fma", ap, ac, av, x), y_fma, "MatMult_SeqAIJ_FMA walks the chain of MatMult_SeqBAIJ_4_FMA")
    if name == R.EMPTY_ROWS:
        assert (np.diff(bp)[[0, 1, 9, 10, 11, 20, 37, 38, 39]] == 0).all() and (y_fma.reshape(-1, 4)[[0, 20, 39]] == 0).all()
    # the comparisons can fail: the column-major bytes read as if they were row-major
    if not np.array_equal(col, np.asarray(bv).reshape(-1)):
        assert not np.array_equal(O.spmv_bcsr4(bp, bc, col, x), y_fma)
        assert not np.array_equal(R.avx2_mult_model(nb, bp, bc, col, x), y_avx2)


@pytest.mark.parametrize("name", R.PRODUCT_MATRICES)
def test_products_error_within_ten_times_the_fma_kernels(name):
    nb, bp, bc, bv = R.matrix(name)
    rec = product_record(name)
    x, col = rec["x"], P.to_petsc_blocks(bv)
    y_ld = R.mult_ld(nb, bp, bc, bv, x)
    e_fma = R.err(rec["y_fma"], y_ld)
    ap, ac, av = R.to_csr(nb, bp, bc, bv)
    print(f"ref_baij product {name} baij avx2: e={R.err(rec['y_avx2'], y_ld):.3e} e_fma={e_fma:.3e}")
    got = {"baij mad": _both_views("mad", bp, bc, col, x), "aij mad": O.ref_aij_mult("mad", ap, ac, av, x), "aij fma": O.ref_aij_mult("fma", ap, ac, av, x)}
    assert_bit_equal(got["baij mad"], rec["y_mad"], "record")
    for what, y in got.items():
        e = R.err(y, y_ld)
        print(f"ref_baij product {name} {what}: e={e:.3e} e_fma={e_fma:.3e}")
        assert e <= MARGIN * e_fma, (name, what, e, e_fma)
    assert not R.err(O.spmv_bcsr4(bp, bc, col, x), y_ld) <= MARGIN * e_fma or np.array_equal(col, np.asarray(bv).reshape(-1))


@pytest.mark.parametrize("name", R.PRODUCT_MATRICES)
def test_multi_vector_product_is_four_times_blockacc(name):
    """Module docstring, "multi": row-major bytes in, 4 A X out, the block sums associated as MI_ARITH_BLOCKACC does."""
    nb, bp, bc, bv = R.matrix(name)
    rec = product_record(name)
    for s in R.SPMM_WIDTHS:
        X, Y = rec["spmm"][s]
        want = np.array([O.spmv_bcsr4_blockacc(bp, bc, bv, X[q]) for q in range(s)])
        assert_bit_equal(Y, 4.0 * want, f"{name} s={s}")
        assert_bit_equal(O.ref_baij_spmm(bp, bc, bv, X, compressed=True), Y, f"{name} s={s}: compressedrow")
    col = P.to_petsc_blocks(bv)
    if not np.array_equal(col, np.asarray(bv).reshape(-1)):  # the PETSc bytes make it multiply by the transposed blocks
        X, Y = rec["spmm"][3]
        assert not np.array_equal(O.ref_baij_spmm(bp, bc, col, X), Y)
        assert not np.array_equal(4.0 * np.array([O.spmv_bcsr4_blockacc(bp, bc, col, X[q]) for q in range(3)]), Y)


# ------------------------------------------------------------------ the recording the GPU test reads

def test_recording_holds_the_live_model():
    """tests/golden/ref_baij.npz carries the model's solve next to the reference's (tests/test_gpu_petsc_seam.py compares the GPU with
    both without factoring in Python): it must be what bilu4_model computes now, and the reference's outputs what they are now."""
    import os

    from conftest import GOLDEN
    g = np.load(os.path.join(GOLDEN, "ref_baij.npz"))
    for case in R.SOLVE_CASES:
        if case[0] in R.GOLDEN_SKIP:
            continue
        for kind, d in solve_record(*case).items():
            got = R.load_solve(g, case, kind)
            for k in ("x_model", "x_scalar", "x_avx2"):
                assert_bit_equal(got[k], d[k], f"{R.case_id(case)} {kind} {k}")
            assert np.array_equal(got["x_ld"], d["x_ld"]), (case, kind)
            assert (got["e_scalar"], got["e_avx2"], got["e_model"]) == (d["e_scalar"], d["e_avx2"], d["e_model"])
