"""Model of the sweep solve (mi_bilu4sw_*), restated from the definition in include/mi355_spmv.h in plain numpy on top of
tests/bilu4_model.py: the factor of the block ILU applied by a fixed number of Jacobi sweeps per triangle.

    forward    t^0 = b;  k < sf:  t^{k+1}_i = b_i - sum_{j<i} L_ij t^k_j
    diagonal   x^0_i = Dinv_i . t^{sf}_i
    backward   k < sb:  x^{k+1}_i = Dinv_i . (t^{sf}_i - sum_{j>i} U_ij x^k_j)

A row's arithmetic is the exact solve's (bilu4_model.solve): blocks in ascending column order, per block matvec4's chain, then one
rounded subtraction; Dinv . s is one matvec4.  All rows of a sweep are computed at once from the previous iterate, step by step over
the rows' blocks, as bilu4_model.solve computes the rows of a level."""
import numpy as np

import bilu4_model as M


def max_sweeps(nb, ptr, col, diag):
    """(fwd_levels - 1, bwd_levels - 1): the counts at which the sweeps return the exact solve's bits, where the library clamps."""
    if nb == 0:
        return 0, 0
    return int(M.levels(nb, ptr, col, diag, False).max()), int(M.levels(nb, ptr, col, diag, True).max())


def _sweep(val, col, k0, k1, src, old):
    """src_i - sum over the blocks [k0_i, k1_i) of row i of val_k . old_{col k}, every row from `old`."""
    s = src.copy()
    a, e = np.asarray(k0, np.int64), np.asarray(k1, np.int64)
    with np.errstate(all="ignore"):
        for step in range(int((e - a).max()) if len(a) else 0):
            live = np.nonzero(a + step < e)[0]
            kk = a[live] + step
            s[live] = s[live] - M.matvec4(val[kk], old[col[kk]])
    return s


def solve_sweeps(nb, ptr, col, diag, val, b, sf, sb, clamp=True):
    """x^{sb} of the definition above.  clamp: counts above max_sweeps are cut to it, as the library does (the bits are the same:
    tests/test_bilu4_sweeps_model.py checks that with clamp=False)."""
    assert sf >= 0 and sb >= 0
    if clamp:
        mf, mb = max_sweeps(nb, ptr, col, diag)
        sf, sb = min(sf, mf), min(sb, mb)
    b = np.array(b, np.float64).reshape(nb, 4)
    val = np.asarray(val, np.float64).reshape(-1, 4, 4)
    t = b.copy()
    for _ in range(sf):
        t = _sweep(val, col, ptr[:-1], diag, b, t)
    with np.errstate(all="ignore"):
        x = M.matvec4(val[diag], t)
        for _ in range(sb):
            x = M.matvec4(val[diag], _sweep(val, col, diag + 1, ptr[1:], t, x))
    return x.reshape(-1)


def dense_operator(nb, fac, sf, sb):
    """The sweep solve as a dense matrix: (sum_{j<=sb} (-Dinv Us)^j . Dinv) . (sum_{j<=sf} (-Ls)^j), Ls / Us the strictly lower /
    upper block triangle of the factor, Dinv its (already inverted) diagonal blocks.  Counts are NOT clamped: beyond levels - 1
    the powers vanish (Ls and Dinv Us are nilpotent)."""
    ptr, col, diag, val = fac
    n = 4 * nb
    F = M.dense(nb, ptr, col, val)
    blk = np.arange(n) // 4
    Ls = np.where(blk[:, None] > blk[None, :], F, 0.0)
    Us = np.where(blk[:, None] < blk[None, :], F, 0.0)
    Dinv = np.where(blk[:, None] == blk[None, :], F, 0.0)
    fwd = np.eye(n)
    for _ in range(sf):  # Horner: I - Ls (I - Ls (...))
        fwd = np.eye(n) - Ls @ fwd
    G = Dinv @ Us
    bwd = np.eye(n)
    for _ in range(sb):
        bwd = np.eye(n) - G @ bwd
    return (bwd @ Dinv) @ fwd
