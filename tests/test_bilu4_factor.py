"""The host factorisation of mi_bilu4_* against the model (tests/bilu4_model.py), bit for bit: row-major and column-major input,
1 and 4 host threads, and after a refactor with new values.  Factorisation is host code: no GPU.  Plus a zero pivot, refused with
its block row named, and a check against mathematics on the matrices where nothing is dropped."""
import os

import numpy as np
import pytest

import bilu4_cases as C
import bilu4_model as M
from conftest import assert_bit_equal

MI_ERR_ARG = 1


def _with_threads(n, fn):
    old = os.environ.get("MI355_BILU_THREADS")
    os.environ["MI355_BILU_THREADS"] = str(n)
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["MI355_BILU_THREADS"]
        else:
            os.environ["MI355_BILU_THREADS"] = old


def _colmajor(bv):
    return np.ascontiguousarray(np.asarray(bv).reshape(-1, 4, 4).transpose(0, 2, 1)).reshape(-1)


def _expect(make, want, what):
    """make() builds (or refactors) a handle and returns it; want: the model's factor or its ZeroPivot."""
    from navierstokes_amd import mpk
    if isinstance(want, M.ZeroPivot):
        with pytest.raises(mpk.MiError) as e:
            make()
        assert e.value.status == MI_ERR_ARG and f"block row {want.row}" in str(e.value), (what, str(e.value))
        return
    F = make()
    ptr, col, diag, val = F.factor_host()
    assert np.array_equal(ptr, want[0]) and np.array_equal(col, want[1]) and np.array_equal(diag, want[2]), what
    assert_bit_equal(val, want[3], what)


@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_factor_bits_equal_the_model(case):
    from navierstokes_amd import mpk
    name, fill = case
    nb, bp, bc, bv = C.matrix(name)
    want = C.model_factor(name, fill)
    made = []

    def build(threads, layout):
        vals = bv if layout == "row" else _colmajor(bv)
        made.append(_with_threads(threads, lambda: mpk.bilu4(nb, bp, bc, vals, fill=fill, layout=layout, host_only=True)))
        return made[-1]

    for threads in (1, 4):
        for layout in ("row", "col"):
            _expect(lambda: build(threads, layout), want, f"{name} fill {fill}: {threads} threads, {layout}-major")
    # a Newton step: new values on the same pattern, through each of the handles that exist
    want2 = C.model_factor(name, fill, 1)
    v2 = C.new_values(name, 1)
    for k, F in enumerate(made):
        vals = v2 if F.layout == 0 else _colmajor(v2)
        _expect(lambda: _with_threads(1 + 3 * (k % 2), lambda: F.refactor(vals)), want2, f"{name} fill {fill}: refactor through handle {k}")
    for F in made:
        F.close()


def test_a_zero_pivot_is_refused_with_its_block_row():
    from navierstokes_amd import mpk
    nb, bp, bc, bv = C.matrix("chain")
    v = np.array(bv).reshape(-1, 4, 4)
    k = bp[37] + list(bc[bp[37]:bp[38]]).index(37)
    v[k] = 0.0            # with its neighbours' coupling blocks zeroed nothing is subtracted from it: the pivot stays an exact zero
    v[bp[37]] = 0.0
    with pytest.raises(mpk.MiError) as e:
        mpk.bilu4(nb, bp, bc, v.reshape(-1), fill=0, host_only=True)
    assert e.value.status == MI_ERR_ARG and "zero pivot" in str(e.value) and "block row 37" in str(e.value)
    with pytest.raises(M.ZeroPivot) as m:
        M.factor(nb, bp, bc, v.reshape(-1), 0)
    assert m.value.row == 37
    # a pivot just above the threshold passes, one just below does not (|d| < 1e-12)
    one = np.eye(4)
    for d, ok in ((1.5e-12, True), (0.5e-12, False), (-0.5e-12, False)):
        blk = one.copy()
        blk[2, 2] = d
        if ok:
            mpk.bilu4(1, [0, 1], [0], blk.reshape(-1), host_only=True).close()
        else:
            with pytest.raises(mpk.MiError) as e:
                mpk.bilu4(1, [0, 1], [0], blk.reshape(-1), host_only=True)
            assert "block row 0" in str(e.value)
    # a refused refactor leaves a handle that a good refactor repairs
    F = mpk.bilu4(nb, bp, bc, bv, fill=0, host_only=True)
    with pytest.raises(mpk.MiError):
        F.refactor(v.reshape(-1))
    F.refactor(bv)
    assert_bit_equal(F.factor_host()[3], C.model_factor("chain", 0)[3], "after a repaired refactor")
    F.close()


@pytest.mark.parametrize("name,fill", [("chain", 0), ("fe:3", 64)])
def test_nothing_dropped_means_lu_reproduces_a(name, fill):
    """Mathematics, not bits: where the pattern drops nothing (a block-tridiagonal chain at any fill; fe_matrix(3) at a fill no
    block can exceed) L U = A up to rounding.  Yardstick: max |L U - P A| / max |A| of a dense LU with partial pivoting of the same
    matrix, in numpy (numpy.linalg keeps its LU to itself, so the elimination is written out here); ten times it is allowed.
    Measured: chain ours 3.8e-16, dense 2.5e-16; fe:3 at fill 64 ours 4.8e-16, dense 1.3e-15."""
    from navierstokes_amd import mpk
    nb, bp, bc, bv = C.matrix(name)
    F = mpk.bilu4(nb, bp, bc, bv, fill=fill, host_only=True)
    ptr, col, diag, val = F.factor_host()
    F.close()
    A = M.dense(nb, bp, bc, np.asarray(bv).reshape(-1, 4, 4))
    ours = np.abs(M.lu_product(nb, ptr, col, diag, val) - A).max() / np.abs(A).max()
    # dense LU with partial pivoting
    n = A.shape[0]
    LU, piv = A.copy(), np.arange(n)
    for k in range(n - 1):
        r = k + int(np.argmax(np.abs(LU[k:, k])))
        if r != k:
            LU[[k, r]] = LU[[r, k]]
            piv[[k, r]] = piv[[r, k]]
        LU[k + 1:, k] /= LU[k, k]
        LU[k + 1:, k + 1:] -= np.outer(LU[k + 1:, k], LU[k, k + 1:])
    dense = np.abs((np.tril(LU, -1) + np.eye(n)) @ np.triu(LU) - A[piv]).max() / np.abs(A).max()
    print(f"{name} fill {fill}: |LU - A|/|A| ours {ours:.3e}, dense LU {dense:.3e}")
    assert ours <= 10 * dense, (ours, dense)
