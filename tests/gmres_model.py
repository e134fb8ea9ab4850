"""Reference for mpk.GMRES: restarted, right-preconditioned GMRES on dense numpy arrays, written to share as little as possible
with the code it checks.  Arnoldi with classical Gram-Schmidt applied twice; the small least-squares problem
min || beta e1 - Hbar y || is solved afresh at every iteration with numpy.linalg.lstsq (no Givens rotations, no recurrence for the
residual: the residual norm is evaluated from y, in numpy.longdouble); the preconditioner is a dense inverse handed in by the
caller (inv(lu_product(...)) of the model's factor, tests/bilu4_model.py).

What it keeps in common with mpk.GMRES is the definition only: history[0] is the true relative residual of the initial guess,
then one entry per iteration, the least-squares residual over ||b||; a cycle ends at `restart` iterations, at rtol, at maxiter or
at a breakdown (the new direction has norm zero); the loop ends at rtol, at maxiter or on a non-finite residual.

wide=True keeps the Arnoldi vectors, the products and the dots in numpy.longdouble (the Hessenberg matrix is rounded to float64
for lstsq): the difference between the two histories is the reference's own spread, from which tests/test_gpu_gmres.py takes its
bound."""
import numpy as np


def true_residual(A, x, b):
    """||b - A x|| / ||b|| in numpy.longdouble."""
    L = np.longdouble
    r = np.asarray(b, L) - np.asarray(A, L) @ np.asarray(x, L)
    return float(np.sqrt(r @ r) / np.sqrt(np.asarray(b, L) @ np.asarray(b, L)))


def gmres(A, b, x0, Minv=None, restart=30, rtol=1e-8, maxiter=300, wide=False):
    """(iterations, history, iterates): iterates[c] is x after restart cycle c (float64)."""
    T = np.longdouble if wide else np.float64
    A = np.asarray(A, T)
    b = np.asarray(b, T)
    Minv = None if Minv is None else np.asarray(Minv, T)
    x = np.array(x0, T)
    norm = lambda v: float(np.sqrt(v @ v))
    bnorm = norm(b) or 1.0
    its, hist, iterates = 0, [], []
    while True:
        r = b - A @ x
        beta = norm(r)
        if not hist:
            hist.append(beta / bnorm)
        if beta / bnorm <= rtol or its >= maxiter or not np.isfinite(beta):
            return its, hist, iterates
        V = [r / T(beta)]
        H = np.zeros((restart + 1, restart))
        k, y = 0, None
        while k < restart and its < maxiter:
            w = A @ (V[k] if Minv is None else Minv @ V[k])
            h = np.zeros(k + 1, T)
            for _ in range(2):
                d = np.array([v @ w for v in V], T)
                for dj, v in zip(d, V):
                    w = w - dj * v
                h = h + d
            nrm = norm(w)
            H[: k + 1, k] = h.astype(np.float64)
            H[k + 1, k] = nrm
            k += 1
            its += 1
            g = np.zeros(k + 1)
            g[0] = beta
            y = np.linalg.lstsq(H[: k + 1, :k], g, rcond=None)[0]
            res = g.astype(np.longdouble) - H[: k + 1, :k].astype(np.longdouble) @ y.astype(np.longdouble)
            hist.append(float(np.sqrt(res @ res)) / bnorm)
            if hist[-1] <= rtol or nrm == 0.0:
                break
            V.append(w / T(nrm))
        u = sum(T(yj) * v for yj, v in zip(y, V))
        x = x + (u if Minv is None else Minv @ u)
        iterates.append(np.asarray(x, np.float64).copy())
        if hist[-1] <= rtol or its >= maxiter:
            return its, hist, iterates


def problem(name, fill):
    """(A dense, Minv dense or None, b) for a matrix of tests/bilu4_cases.py; fill None: no preconditioner.  Minv is the inverse
    of the product of the MODEL's factors."""
    import bilu4_cases as C
    import bilu4_model as M
    nb, bp, bc, bv = C.matrix(name)
    A = M.dense(nb, bp, bc, np.asarray(bv).reshape(-1, 4, 4))
    Minv = None
    if fill is not None:
        fac = M.factor(nb, bp, bc, bv, fill) if fill > 2 else C.model_factor(name, fill)
        Minv = np.linalg.inv(M.lu_product(nb, *fac))
    n = 4 * nb
    b = np.sin(0.37 * np.arange(n)) + 1.0 + 0.25 * np.cos(0.011 * np.arange(n) ** 2)
    return A, Minv, b


HISTORY_CASES = [(name, fill) for name in ("fe:3", "fe:6", "chain", "random:12", "random:31", "random:62") for fill in (None, 0)] + [("fe:6", 1)]
RESTARTS = (30, 5)
