"""The arrays a PETSc MATSEQBAIJ (block size 4) holds, made from this project's arrays in plain numpy — what a PETSc caller hands
the reference's MatMult_SeqBAIJ_4* and MatSolve_SeqBAIJ_4* (src/kernels/*.c), and so what tests/test_ref_baij.py hands them.

A factored matrix (the one MATOP_SOLVE receives, src/kernels/baij4_solve.c:29-85) keeps L and U apart:
  bi[i] .. bi[i+1]-1              the L blocks of block row i, columns ascending (the forward loop reads exactly these);
  bdiag[i]                        the INVERTED diagonal block of row i; bdiag descends: bdiag[0] is the last index of the arrays;
  bdiag[i+1]+1 .. bdiag[i]-1      the U blocks of row i, columns ascending (so the rows of U lie in reverse order behind L);
  bdiag[n] = bi[n] - 1            one before row n-1's U blocks.
Every 4x4 block is column-major: entry (r, c) at 4 c + r.
"""
import numpy as np


def to_petsc_blocks(bv):
    """Row-major 4x4 blocks (any shape holding 16 values per block) -> the column-major values of Mat_SeqBAIJ::a, flat."""
    return np.ascontiguousarray(np.asarray(bv, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)).reshape(-1)


def to_petsc_factor(ptr, col, diag, val):
    """(bi, bj, bdiag, ba) from (ptr, col, diag, val) of mpk.bilu4.factor_host() / bilu4_model.factor (row-major blocks: L
    multipliers, inverted diagonal blocks, U)."""
    ptr, col, diag = np.asarray(ptr, np.int64), np.asarray(col, np.int64), np.asarray(diag, np.int64)
    val = np.asarray(val, np.float64).reshape(-1, 4, 4)
    n = len(ptr) - 1
    nl = diag - ptr[:-1]
    nu = ptr[1:] - diag - 1
    bi = np.concatenate([[0], np.cumsum(nl)])
    bdiag = np.empty(n + 1, np.int64)
    bdiag[n] = bi[n] - 1
    for i in range(n - 1, -1, -1):
        bdiag[i] = bdiag[i + 1] + nu[i] + 1
    assert n == 0 or bdiag[0] == len(col) - 1
    bj = np.empty(len(col), np.int64)
    ba = np.empty((len(col), 4, 4))
    for i in range(n):
        for src, dst, cnt in ((ptr[i], bi[i], nl[i]), (diag[i] + 1, bdiag[i + 1] + 1, nu[i]), (diag[i], bdiag[i], 1)):
            bj[dst:dst + cnt] = col[src:src + cnt]
            ba[dst:dst + cnt] = val[src:src + cnt].transpose(0, 2, 1)
    return bi.astype(np.int32), bj.astype(np.int32), bdiag.astype(np.int32), ba.reshape(-1)


def lu_product(bi, bj, bdiag, ba):
    """L . U as a dense matrix, read back out of the PETSc arrays by the rules above (the counterpart of bilu4_model.lu_product)."""
    n = len(bi) - 1
    blk = np.asarray(ba, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)
    L, U = np.eye(4 * n), np.zeros((4 * n, 4 * n))
    for i in range(n):
        for k in range(bi[i], bi[i + 1]):
            L[4 * i:4 * i + 4, 4 * bj[k]:4 * bj[k] + 4] = blk[k]
        for k in range(bdiag[i + 1] + 1, bdiag[i]):
            U[4 * i:4 * i + 4, 4 * bj[k]:4 * bj[k] + 4] = blk[k]
        assert bj[bdiag[i]] == i
        U[4 * i:4 * i + 4, 4 * i:4 * i + 4] = np.linalg.inv(blk[bdiag[i]])
    return L @ U
