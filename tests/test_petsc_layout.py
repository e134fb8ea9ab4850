"""tests/petsc_layout.py on the CPU, without the reference: the factor in PETSc's factored BAIJ layout is the model's factor — L . U
rebuilt out of the PETSc arrays equals bilu4_model.lu_product bit for bit — and the arrays obey the rules MatSolve_SeqBAIJ_4 reads
them by (src/kernels/baij4_solve.c:29-85)."""
import numpy as np
import pytest

import bilu4_cases as C
import bilu4_model as M
import petsc_layout as P

CASES = [("fe:3", 0), ("fe:3", 4), ("arrow", 0), ("arrow", 1), ("chain", 2), ("diag", 0), ("wide:65", 0)] + [(f"random:{s}", s % 3) for s in range(10)]


@pytest.mark.parametrize("case", CASES, ids=C.case_id)
def test_factored_layout_rebuilds_the_models_lu(case):
    name, fill = case
    nb = C.matrix(name)[0]
    ptr, col, diag, val = C.model_factor(name, fill)
    bi, bj, bdiag, ba = P.to_petsc_factor(ptr, col, diag, val)
    assert bi.dtype == bj.dtype == bdiag.dtype == np.int32 and ba.dtype == np.float64 and ba.shape == (16 * len(col),)
    assert bi[0] == 0 and bdiag[nb] == bi[nb] - 1 and bdiag[0] == len(col) - 1 and (np.diff(bdiag) < 0).all()
    for i in range(nb):
        lower, upper = bj[bi[i]:bi[i + 1]], bj[bdiag[i + 1] + 1:bdiag[i]]
        assert (np.diff(lower) > 0).all() and (lower < i).all() and (np.diff(upper) > 0).all() and (upper > i).all() and bj[bdiag[i]] == i
    got, want = P.lu_product(bi, bj, bdiag, ba), M.lu_product(nb, ptr, col, diag, val)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    # a block is column-major: entry (r, c) at 4 c + r
    k = int(diag[nb - 1])
    assert np.array_equal(ba.reshape(-1, 16)[bdiag[nb - 1]], np.asarray(val[k]).T.reshape(-1))


def test_product_blocks_are_transposed_in_place():
    bv = np.arange(48.0)
    col = P.to_petsc_blocks(bv)
    assert col.shape == (48,) and col[1] == 4.0 and col[4] == 1.0 and col[16 + 7] == 16 + 13.0
    assert np.array_equal(P.to_petsc_blocks(col), bv)
