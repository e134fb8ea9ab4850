"""Model of the single-precision copy of the block ILU factor (mi_bilu4sp_*), restated from the definition in
include/mi355_spmv.h: every factor value v becomes v32 = (double)(float)v — numpy's astype(float32): round to nearest, ties to even,
subnormals kept, a finite value beyond the float range +-Inf — and the sweep solve is tests/bilu4_sweeps_model.py on those values,
in double."""
import numpy as np

import bilu4_sweeps_model as S


def round_factor(val):
    """The factor values as float32, same shape."""
    with np.errstate(all="ignore"):
        return np.asarray(val, np.float64).astype(np.float32)


def rounded(fac):
    """(ptr, col, diag, v32 as float64): the factor the single-precision sweeps apply."""
    ptr, col, diag, val = fac
    return ptr, col, diag, round_factor(val).astype(np.float64)


def solve_sweeps_sp(nb, ptr, col, diag, val, b, sf, sb, clamp=True):
    """bilu4_sweeps_model.solve_sweeps with v32 in place of v."""
    return S.solve_sweeps(nb, ptr, col, diag, round_factor(val).astype(np.float64), b, sf, sb, clamp)


def overflowed(val, ptr):
    """(count, first block row): the values that are finite as double and not as float, and the smallest block row that holds one
    (-1: none).  ptr: the factor's row pointers."""
    val = np.asarray(val, np.float64).reshape(-1, 4, 4)
    bad = np.isfinite(val) & ~np.isfinite(round_factor(val))
    if not bad.any():
        return 0, -1
    first = int(np.nonzero(bad.any(axis=(1, 2)))[0][0])
    return int(bad.sum()), int(np.searchsorted(np.asarray(ptr), first, side="right") - 1)
