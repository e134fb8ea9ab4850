"""Model of the block DILU preconditioner applied with Eisenstat's trick (mi_dilu4_*), restated from the description in
include/mi355_spmv.h in plain Python / numpy floats, in the style of tests/bilu4_model.py, whose chain (matvec4, matmul4: libm's fma
or its proved emulation) and Gauss-Jordan inverse (invert4) it reuses.  Nothing here comes from the library under test.

B = L + D + U is the matrix IN THE HANDLE'S NUMBERING (the caller's, or Q A Q^T under the multicolour rule of
tests/bilu4_order_cases.py); M = (E + L) E^-1 (E + U).

  pivots     block rows ascending: E_i = D_i; for j < i ascending with (i, j) AND (j, i) in the pattern: T = B_ij . Einv_j,
             P = T . B_ji, E_i = E_i - P; Einv_i = invert4(E_i); K_i = (2 E_i) - D_i
  to_hat     b^ = (E + L)^-1 r:    a = 0; a += chain(L_ij, b^_j) ascending j; s = r_i - a; b^_i = chain(Einv_i, s)
  from_hat   x = (E + U)^-1 E u:   a = 0; a += chain(U_ij, x_j) ascending j; c = chain(Einv_i, a); x_i = u_i - c
  apply_hat  w = A^ u:             t = from_hat(u); a = chain(K_i, t_i); a += chain(L_ij, y_j); c = chain(Einv_i, a);
                                   y_i = u_i - c; w_i = t_i + y_i

The rows of a dependency level are computed at once (numpy), level by level: any order that respects the dependencies gives the
same bits, which is the point.  The levels are those of bilu4_model.schedule on B's pattern."""
import numpy as np

import bilu4_model as M
import bilu4_order_cases as OC


def diag_positions(nb, ptr, col):
    return np.array([ptr[i] + list(col[ptr[i]:ptr[i + 1]]).index(i) for i in range(nb)], np.int64)


def schedules(nb, ptr, col):
    diag = diag_positions(nb, ptr, col)
    return diag, M.schedule(nb, ptr, col, diag, False), M.schedule(nb, ptr, col, diag, True)


def pivots(nb, ptr, col, val):
    """(E, Einv, K), each (nb, 4, 4); raises bilu4_model.ZeroPivot(lowest refused row of B)."""
    val = np.asarray(val, np.float64).reshape(-1, 4, 4)
    diag, F, _ = schedules(nb, ptr, col)
    where = {(i, int(col[k])): k for i in range(nb) for k in range(ptr[i], ptr[i + 1])}
    E = val[diag].copy() if nb else np.zeros((0, 4, 4))
    Einv, K = np.zeros_like(E), np.zeros_like(E)
    for l in range(F["nlev"]):
        rows = F["perm"][F["lev_ptr"][l]:F["lev_ptr"][l + 1]]
        a, e = np.asarray(ptr)[rows].astype(np.int64), diag[rows]
        for step in range(int((e - a).max()) if len(rows) else 0):
            live = np.nonzero(a + step < e)[0]
            kk = a[live] + step
            mirror = np.array([where.get((int(col[k]), int(rows[r])), -1) for r, k in zip(live, kk)], np.int64)
            has = mirror >= 0  # no block (j, i): the term is skipped
            if not has.any():
                continue
            live, kk, mirror = live[has], kk[has], mirror[has]
            T = M.matmul4(val[kk], Einv[col[kk]])
            with np.errstate(all="ignore"):
                E[rows[live]] = E[rows[live]] - M.matmul4(T, val[mirror])
        with np.errstate(all="ignore"):
            K[rows] = (2.0 * E[rows]) - val[diag[rows]]
        bad = []
        for i in rows:
            inv = E[i].copy()
            if not M.invert4(inv):
                bad.append(int(i))
            Einv[i] = inv
        if bad:
            raise M.ZeroPivot(min(bad))
    return E, Einv, K


def _sweep(nb, ptr, col, val, S, k0, k1, start, finish):
    """One triangular sweep by levels: a = start(rows) (n, 4); a += chain(block, g_col) over the blocks [k0, k1) of each row in
    ascending column; g[rows] = finish(rows, a).  Returns g (nb, 4)."""
    g = np.zeros((nb, 4))
    for l in range(S["nlev"]):
        rows = S["perm"][S["lev_ptr"][l]:S["lev_ptr"][l + 1]]
        a = start(rows)
        lo, hi = k0[rows].astype(np.int64), k1[rows].astype(np.int64)
        for step in range(int((hi - lo).max()) if len(rows) else 0):
            live = np.nonzero(lo + step < hi)[0]
            kk = lo[live] + step
            with np.errstate(all="ignore"):
                a[live] = a[live] + M.matvec4(val[kk], g[col[kk]])
        g[rows] = finish(rows, a, g)
    return g


class Dilu:
    """The model of one handle: B's pattern and values in the handle's numbering, the pivots, the three operations on vectors in
    THAT numbering.  einv / kmat may be replaced (the deliberately wrong inputs of tests/test_dilu4.py)."""

    def __init__(self, nb, ptr, col, val):
        self.nb, self.ptr, self.col = nb, np.asarray(ptr), np.asarray(col)
        self.val = np.asarray(val, np.float64).reshape(-1, 4, 4)
        self.diag, self.F, self.Bw = schedules(nb, self.ptr, self.col)
        self.E, self.einv, self.kmat = pivots(nb, self.ptr, self.col, self.val)

    def to_hat(self, r):
        r = np.asarray(r, np.float64).reshape(self.nb, 4)

        def finish(rows, a, g):
            with np.errstate(all="ignore"):
                return M.matvec4(self.einv[rows], r[rows] - a)
        return _sweep(self.nb, self.ptr, self.col, self.val, self.F, self.ptr[:-1], self.diag, lambda rows: np.zeros((len(rows), 4)), finish).reshape(-1)

    def from_hat(self, u):
        u = np.asarray(u, np.float64).reshape(self.nb, 4)

        def finish(rows, a, g):
            with np.errstate(all="ignore"):
                return u[rows] - M.matvec4(self.einv[rows], a)
        return _sweep(self.nb, self.ptr, self.col, self.val, self.Bw, self.diag + 1, self.ptr[1:], lambda rows: np.zeros((len(rows), 4)), finish).reshape(-1)

    def apply_hat(self, u):
        u = np.asarray(u, np.float64).reshape(self.nb, 4)
        t = self.from_hat(u).reshape(self.nb, 4)
        w = np.zeros((self.nb, 4))

        def finish(rows, a, g):
            with np.errstate(all="ignore"):
                y = u[rows] - M.matvec4(self.einv[rows], a)
                w[rows] = t[rows] + y
            return y
        _sweep(self.nb, self.ptr, self.col, self.val, self.F, self.ptr[:-1], self.diag, lambda rows: M.matvec4(self.kmat[rows], t[rows]), finish)
        return w.reshape(-1)


class Ordered:
    """The model of a handle as the CALLER sees it: order "natural" or "colour" (the rule of tests/bilu4_order_cases.py), block
    layout "row" or "col" of the caller's values; vectors, fetch() and a refused pivot's row in the caller's numbering."""

    def __init__(self, nb, ptr, col, coef, order="colour", layout="row"):
        blocks = np.asarray(coef, np.float64).reshape(-1, 4, 4)
        if layout == "col":
            blocks = blocks.transpose(0, 2, 1)
        self.nb = nb
        if order == "colour":
            self.perm, _ = OC.colour_model(nb, ptr, col)
            bptr, bcol, bval, _ = OC.permute(nb, ptr, col, blocks, self.perm)
        else:
            self.perm = np.arange(nb, dtype=np.int32)
            bptr, bcol, bval = np.asarray(ptr), np.asarray(col), blocks
        try:
            self.B = Dilu(nb, bptr, bcol, bval)
        except M.ZeroPivot as z:
            raise M.ZeroPivot(int(np.nonzero(self.perm == z.row)[0][0])) from None

    def fetch(self):
        return self.B.einv[self.perm], self.B.kmat[self.perm]

    def _through(self, op, v):
        return OC.vec_out(op(OC.vec_in(v, self.perm)), self.perm)

    def to_hat(self, r):
        return self._through(self.B.to_hat, r)

    def from_hat(self, u):
        return self._through(self.B.from_hat, u)

    def apply_hat(self, u):
        return self._through(self.B.apply_hat, u)


# ------------------------------------------------------------------ the algebra, densely, in longdouble

def dense_parts(D):
    """(B, E, L, U) of a Dilu as dense longdouble matrices: E the block diagonal of the pivots, L and U B's strict block triangles."""
    n = 4 * D.nb
    B, E, L, U = (np.zeros((n, n), np.longdouble) for _ in range(4))
    for i in range(D.nb):
        E[4 * i:4 * i + 4, 4 * i:4 * i + 4] = D.E[i]
        for k in range(D.ptr[i], D.ptr[i + 1]):
            j = int(D.col[k])
            B[4 * i:4 * i + 4, 4 * j:4 * j + 4] = D.val[k]
            if j != i:
                (L if j < i else U)[4 * i:4 * i + 4, 4 * j:4 * j + 4] = D.val[k]
    return B, E, L, U


def solve_ld(A, b):
    """A x = b by Gaussian elimination with partial pivoting, every operation in longdouble."""
    A = np.array(A, np.longdouble)
    x = np.array(b, np.longdouble)
    n = len(x)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            x[[k, p]] = x[[p, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= f[:, None] * A[k, k:][None, :]
        x[k + 1:] -= f * x[k]
    for k in range(n - 1, -1, -1):
        x[k] = (x[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def dense_apply_hat(D, u):
    """(E + L)^-1 B (E + U)^-1 E u in longdouble."""
    B, E, L, U = dense_parts(D)
    return solve_ld(E + L, B @ solve_ld(E + U, E @ np.asarray(u, np.longdouble)))


def dense_minv(D, r):
    """M^-1 r = (E + U)^-1 E (E + L)^-1 r in longdouble."""
    _, E, L, U = dense_parts(D)
    return solve_ld(E + U, E @ solve_ld(E + L, np.asarray(r, np.longdouble)))
