"""Model of the 4x4-block ILU(k) preconditioner (mi_bilu4_*), restated from the description in include/mi355_spmv.h in plain
Python / numpy: symbolic ILU(k), the numeric factorisation, the level schedule with folding, and the solve.

The correctly rounded fma comes from the C library through ctypes (libm's fma), never from the library under test.  Calling it
once per multiply-add is too slow for the factorisations the tests ask for, so the bulk arithmetic runs through `fma_vec`: a numpy
emulation of the fma from error-free transformations and one rounding to odd (Boldo and Melquiond, "Emulation of FMA and
correctly rounded sums: proved algorithms using rounding to odd", IEEE TC 2008): a*b = uh + ul exactly (Dekker / Veltkamp),
c + uh = th + tl exactly (Knuth), v = tl + ul rounded to odd, result = th + v rounded to nearest.  The emulation is exact only
while nothing overflows or underflows inside it, so `fma_vec` sends every element whose operands or results leave a safe range
(or are not finite) to libm's fma one by one; tests/test_bilu4_plan.py checks the emulation against libm on random, cancelling
and edge operands.
"""
import ctypes
import ctypes.util

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3
fma = _libm.fma

ROWS_PER_WG = 64   # block rows one workgroup of the solve serves: a level with fewer is narrow
PIVOT_MIN = 1e-12
_LO, _HI = 2.0 ** -400, 2.0 ** 400


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a
    h = c - (c - a)
    return h, a - h


def fma_vec(a, b, c):
    """Correctly rounded a*b + c, elementwise, as float64 arrays of one shape."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    a, b, c = a.copy(), b.copy(), c.copy()
    with np.errstate(all="ignore"):
        uh = a * b
        ah, al = _split(a)
        bh, bl = _split(b)
        ul = (((ah * bh - uh) + ah * bl) + al * bh) + al * bl
        th, tl = _two_sum(c, uh)
        v, e = _two_sum(tl, ul)
        even = (v.view(np.int64) & 1) == 0
        nudge = (e != 0) & even
        v = np.where(nudge, np.nextafter(v, np.where(e > 0, np.inf, -np.inf)), v)
        out = th + v

        def unsafe(t):
            m = np.abs(t)
            return ~np.isfinite(t) | ((m != 0) & ((m < _LO) | (m > _HI)))
        bad = unsafe(a) | unsafe(b) | unsafe(c) | unsafe(out) | (out == 0)
        # an exact zero on one side needs no emulation: the other side is the result (safe operands: a nonzero product is normal);
        # zero on both sides goes to libm for the sign rules
        zp, zc = (a == 0) | (b == 0), c == 0
        out = np.where(zp & ~zc, c, np.where(zc & ~zp, uh, out))
        bad |= zp & zc
    if bad.any():
        idx = np.nonzero(bad.reshape(-1))[0]
        fa, fb, fc, fo = a.reshape(-1), b.reshape(-1), c.reshape(-1), out.reshape(-1)
        for t in idx:
            fo[t] = fma(fa[t], fb[t], fc[t])
        out = fo.reshape(a.shape)
    return out


def matmul4(A, B):
    """C = A . B for stacks of 4x4 blocks (..., 4, 4): every entry fma(a3,b3, fma(a2,b2, fma(a1,b1, a0*b0)))."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    with np.errstate(all="ignore"):
        p = A[..., :, 0:1] * B[..., 0:1, :]
    for k in (1, 2, 3):
        p = fma_vec(A[..., :, k:k + 1], B[..., k:k + 1, :], p)
    return p


def matvec4(A, t):
    """p = A . t for stacks of blocks (..., 4, 4) and vectors (..., 4), the same chain per entry."""
    A, t = np.asarray(A, np.float64), np.asarray(t, np.float64)
    with np.errstate(all="ignore"):
        p = A[..., :, 0] * t[..., 0:1]
    for k in (1, 2, 3):
        p = fma_vec(A[..., :, k], t[..., k:k + 1], p)
    return p


def invert4(a):
    """In-place Gauss-Jordan without pivoting on a (4, 4) array, plain rounded products and subtractions; False: refused pivot."""
    for k in range(4):
        d = float(a[k, k])
        if abs(d) < PIVOT_MIN:
            return False
        with np.errstate(all="ignore"):
            piv = np.float64(1.0) / np.float64(d)
            a[k, k] = 1.0
            a[k, :] = a[k, :] * piv
            for i in range(4):
                if i == k:
                    continue
                f = a[i, k]
                a[i, k] = 0.0
                a[i, :] = a[i, :] - f * a[k, :]
    return True


# ------------------------------------------------------------------ pattern

def check_pattern(nb, ptrow, indcol):
    """None, or why mi_bilu4_* must refuse the pattern."""
    if nb and ptrow[0] != 0:
        return "ptrow[0]"
    for i in range(nb):
        cols = list(indcol[ptrow[i]:ptrow[i + 1]])
        if any(c < 0 or c >= nb for c in cols):
            return "out of range"
        if any(cols[k] == cols[k - 1] for k in range(1, len(cols))) and sorted(cols) == cols:
            return "duplicate"
        if any(cols[k] <= cols[k - 1] for k in range(1, len(cols))):
            return "unsorted"
        if i not in cols:
            return "missing diagonal"
    return None


def symbolic(nb, ptrow, indcol, fill):
    """(ptr, col, diag) of the ILU(fill) pattern: lev(i, j) = min over pivots p of lev(i, p) + lev(p, j) + 1, kept when <= fill."""
    ptr, col, lev, diag = [0], [], [], []
    for i in range(nb):
        row = {int(c): 0 for c in indcol[ptrow[i]:ptrow[i + 1]]}
        if fill > 0:
            done = set()
            while True:
                cand = [c for c in row if c < i and c not in done]
                if not cand:
                    break
                p = min(cand)
                done.add(p)
                for k in range(diag[p] + 1, ptr[p + 1]):
                    nl = row[p] + lev[k] + 1
                    j = col[k]
                    if j in row:
                        row[j] = min(row[j], nl)
                    elif nl <= fill:
                        row[j] = nl
        for c in sorted(row):
            if c == i:
                diag.append(len(col))
            col.append(c)
            lev.append(row[c])
        ptr.append(len(col))
    return np.array(ptr, np.int32), np.array(col, np.int32), np.array(diag, np.int32)


def levels(nb, ptr, col, diag, backward):
    lev = np.zeros(nb, np.int64)
    order = range(nb - 1, -1, -1) if backward else range(nb)
    for i in order:
        deps = col[diag[i] + 1:ptr[i + 1]] if backward else col[ptr[i]:diag[i]]
        lev[i] = 1 + max(lev[j] for j in deps) if len(deps) else 0
    return lev


def schedule(nb, ptr, col, diag, backward):
    """dict(perm, lev_ptr, sizes, launches, launch_ptr): level-major order (ascending row inside a level); a run of consecutive
    narrow levels is one launch."""
    lev = levels(nb, ptr, col, diag, backward)
    nlev = int(lev.max()) + 1 if nb else 0
    perm = np.lexsort((np.arange(nb), lev)).astype(np.int32) if nb else np.zeros(0, np.int32)
    sizes = np.bincount(lev, minlength=nlev).astype(np.int32) if nb else np.zeros(0, np.int32)
    lev_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    launch_ptr, l = [0], 0
    while l < nlev:
        e = l + 1
        if sizes[l] < ROWS_PER_WG:
            while e < nlev and sizes[e] < ROWS_PER_WG:
                e += 1
        launch_ptr.append(e)
        l = e
    return dict(perm=perm, lev_ptr=lev_ptr, sizes=sizes, launches=len(launch_ptr) - 1, launch_ptr=launch_ptr, nlev=nlev)


# ------------------------------------------------------------------ numeric

class ZeroPivot(Exception):
    def __init__(self, row):
        super().__init__(f"zero pivot in block row {row}")
        self.row = row


def factor(nb, ptrow, indcol, coef, fill, layout="row"):
    """(ptr, col, diag, val): val (nblocks, 4, 4) row-major — L multipliers, INVERTED diagonal blocks, U blocks.  Rows in
    natural order (any order that respects the dependencies gives the same bits)."""
    ptr, col, diag = symbolic(nb, ptrow, indcol, fill)
    blocks = np.asarray(coef, np.float64).reshape(-1, 4, 4)
    if layout == "col":
        blocks = blocks.transpose(0, 2, 1)
    val = np.zeros((len(col), 4, 4))
    for i in range(nb):
        k0, k1 = int(ptr[i]), int(ptr[i + 1])
        pos = {int(col[k]): k - k0 for k in range(k0, k1)}
        w = np.zeros((k1 - k0, 4, 4))
        for k in range(ptrow[i], ptrow[i + 1]):
            w[pos[int(indcol[k])]] = blocks[k]
        for k in range(k0, int(diag[i])):
            wk = w[k - k0]
            if not wk.any():  # all 16 entries zero (either sign)
                continue
            p = int(col[k])
            m = matmul4(wk, val[diag[p]])
            w[k - k0] = m
            ks = [kk for kk in range(int(diag[p]) + 1, int(ptr[p + 1])) if int(col[kk]) in pos]
            if ks:
                at = [pos[int(col[kk])] for kk in ks]
                with np.errstate(all="ignore"):
                    w[at] = w[at] - matmul4(m[None], val[ks])
        val[k0:k1] = w
        if not invert4(val[diag[i]]):
            raise ZeroPivot(i)
    return ptr, col, diag, val


def solve(nb, ptr, col, diag, val, b, sched=None):
    """x = U^-1 L^-1 b.  sched = (forward schedule, backward schedule): the rows of a level at once (numpy); None: row by row in
    natural order.  The same bits either way — which is the point."""
    t = np.array(b, np.float64).reshape(nb, 4).copy()
    with np.errstate(all="ignore"):
        if sched is None:
            for i in range(nb):
                s = t[i].copy()
                for k in range(ptr[i], diag[i]):
                    s = s - matvec4(val[k], t[col[k]])
                t[i] = s
            for i in range(nb - 1, -1, -1):
                s = t[i].copy()
                for k in range(diag[i] + 1, ptr[i + 1]):
                    s = s - matvec4(val[k], t[col[k]])
                t[i] = matvec4(val[diag[i]], s)
            return t.reshape(-1)
        for backward, S in ((False, sched[0]), (True, sched[1])):
            k0 = (diag + 1) if backward else ptr[:-1]
            k1 = ptr[1:] if backward else diag
            for l in range(S["nlev"]):
                rows = S["perm"][S["lev_ptr"][l]:S["lev_ptr"][l + 1]]
                s = t[rows].copy()
                a, e = k0[rows].astype(np.int64), k1[rows].astype(np.int64)
                for step in range(int((e - a).max()) if len(rows) else 0):
                    live = np.nonzero(a + step < e)[0]
                    kk = a[live] + step
                    s[live] = s[live] - matvec4(val[kk], t[col[kk]])
                t[rows] = matvec4(val[diag[rows]], s) if backward else s
    return t.reshape(-1)


def dense(nb, ptr, col, val):
    A = np.zeros((4 * nb, 4 * nb))
    for i in range(nb):
        for k in range(ptr[i], ptr[i + 1]):
            A[4 * i:4 * i + 4, 4 * col[k]:4 * col[k] + 4] = np.asarray(val[k]).reshape(4, 4)
    return A


def lu_product(nb, ptr, col, diag, val):
    """L . U as a dense matrix (unit block lower triangle of multipliers; U with the diagonal blocks inverted back)."""
    L, U = np.eye(4 * nb), np.zeros((4 * nb, 4 * nb))
    for i in range(nb):
        for k in range(ptr[i], ptr[i + 1]):
            j = col[k]
            if j < i:
                L[4 * i:4 * i + 4, 4 * j:4 * j + 4] = val[k]
            elif j == i:
                U[4 * i:4 * i + 4, 4 * j:4 * j + 4] = np.linalg.inv(val[k])
            else:
                U[4 * i:4 * i + 4, 4 * j:4 * j + 4] = val[k]
    return L @ U
