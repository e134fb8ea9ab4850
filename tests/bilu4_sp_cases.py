"""Two hand-made cases for the single-precision copy of the block ILU factor (mi_bilu4sp_*), and the lookups of
tests/bilu4_cases.py extended by them.

Pattern (70 block rows: one workgroup of 64 block rows and a second, short one): block row 0 holds its diagonal block and three
blocks right of it; the rows 1..69 are a chain with a few longer links AMONG THEMSELVES — no row has a block in column 0.  The ILU
leaves block row 0 of the matrix as it is (U_0j = A_0j: there is nothing left of its diagonal to eliminate), A_00 is a diagonal of
powers of two, so Dinv_0 is exact, and since nothing below the diagonal touches column 0 no other row's factor ever reads row 0:
whatever is planted in A_0j is in the factor bit for bit and nowhere else.  In the solve row 0 is a sink: it reads x_j, and no row
reads x_0.

sp_edges     PLANTED in U_03 (and Dinv_00 = 2^-140): the values whose rounding to float the definition spells out
sp_overflow  the same with two finite doubles that are Inf as float, in block row 0
"""
import functools

import numpy as np

import bilu4_cases as C
import bilu4_model as M

NB = 70
FMAX = float(np.finfo(np.float32).max)            # (2 - 2^-23) 2^127
TIE_TO_INF = (2.0 - 2.0 ** -24) * 2.0 ** 127      # half-way between FMAX and 2^128: the tie goes to the even 2^128, which is Inf
# (value, what astype(float32) must make of it, as a double); all of them exact doubles
PLANTED = [
    (1.0 + 2.0 ** -24, 1.0),                                      # tie: to even
    (1.0 + 2.0 ** -24 + 2.0 ** -52, 1.0 + 2.0 ** -23),            # just above the tie
    (1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -22),                     # tie: to even, upwards
    (FMAX, FMAX),
    (float(np.nextafter(TIE_TO_INF, 0.0)), FMAX),                 # the largest double that still rounds to FMAX
    (2.0 ** -126, 2.0 ** -126),                                   # the smallest normal float
    (2.0 ** -127, 2.0 ** -127),                                   # subnormal, exact
    (2.0 ** -149, 2.0 ** -149),                                   # the smallest subnormal
    (2.0 ** -150, 0.0),                                           # tie between 0 and 2^-149: to even, +0
    (2.0 ** -150 * (1.0 + 2.0 ** -52), 2.0 ** -149),              # just above it
    (-(2.0 ** -151), -0.0),
    (-0.0, -0.0),
]
DINV00 = 2.0 ** -140                                              # a subnormal float, exact
OVERFLOW = [TIE_TO_INF, 1e300]
ROW0_COLS = (0, 3, 7, 69)
PLANT_COL = 3
NAMES = ("sp_edges", "sp_overflow")


def _pattern():
    rows = [set(ROW0_COLS)]
    for i in range(1, NB):
        r = {j for j in (i - 1, i, i + 1) if 1 <= j < NB}
        if i % 5 == 0 and i >= 10:
            r.add(i - 9)
        if i % 7 == 0 and i + 11 < NB:
            r.add(i + 11)
        rows.append(r)
    return rows


@functools.lru_cache(maxsize=None)
def _sp_matrix(name):
    nb, ptr, col, val = C._from_rows(_pattern(), 50)
    assert not any(0 in col[ptr[i]:ptr[i + 1]] for i in range(1, nb)), "a block below the diagonal touches column 0"
    val = val.reshape(-1, 4, 4).copy()
    val[0] = np.diag([1.0 / DINV00, 1.0, 2.0, 0.5])
    k = list(col[ptr[0]:ptr[1]]).index(PLANT_COL)
    flat = val[k].reshape(-1)
    if name == "sp_edges":
        flat[:len(PLANTED)] = [v for v, _ in PLANTED]
    else:
        flat[5], flat[10] = OVERFLOW
    return nb, ptr, col, val.reshape(-1)


def planted_block(name, fac):
    """The 16 values of the factor block that holds the planted values, flat."""
    ptr, col, diag, val = fac
    return np.asarray(val).reshape(-1, 4, 4)[int(ptr[0]) + list(col[ptr[0]:ptr[1]]).index(PLANT_COL)].reshape(-1)


def matrix(name):
    return _sp_matrix(name) if name in NAMES else C.matrix(name)


def new_values(name, variant):
    """As bilu4_cases.new_values; the two cases here are scaled by 1/2 off the diagonal blocks instead (exact: the planted values
    stay inside the range of double), which takes TIE_TO_INF back into the range of float and leaves 1e300 / 2 outside."""
    if name not in NAMES:
        return C.new_values(name, variant)
    nb, bp, bc, bv = matrix(name)
    v = np.array(bv, np.float64).reshape(-1, 4, 4) * 0.5
    for i in range(nb):
        k = bp[i] + list(bc[bp[i]:bp[i + 1]]).index(i)
        v[k] = np.asarray(bv).reshape(-1, 4, 4)[k] * 1.25
    return v.reshape(-1)


@functools.lru_cache(maxsize=None)
def model_factor(name, fill, variant=0):
    if name not in NAMES:
        return C.model_factor(name, fill, variant)
    nb, bp, bc, bv = matrix(name)
    return M.factor(nb, bp, bc, new_values(name, variant) if variant else bv, fill)
