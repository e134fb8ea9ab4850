"""mi_gmres_* with MI_BASIS_F32 (include/mi355_spmv.h) as a dense numpy model: round32 / widen of the interface's DEFINITION, and
restarted, right-preconditioned GMRES with the Krylov basis STORED in float32 — every projection against the stored basis, the
vector fed to the next product the stored one, the small problem that of tests/gmres_dev_model.py unchanged, and a converged
recurrence only a CLAIM that the next cycle's true residual confirms or refuses.

The model follows the definition's steps, not the device's summation trees: its dots are numpy's, so it shares the device's
iteration counts and refusals only where those do not hang on the last bits.  tests/test_gpu_gmres_f32.py holds the device to
its bits with a loop composed from the library's own pieces instead."""
import numpy as np

import gmres_dev_model as D


def round32(v):
    """(float)v of the interface: to nearest, ties to even, subnormals kept, beyond the float range +-Inf, -0 and NaN kept.  Returns
    float32 (a scalar for a scalar)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(v, dtype=np.float64).astype(np.float32)[()]


def widen(f):
    """(double)f: exact."""
    return np.asarray(f, dtype=np.float32).astype(np.float64)[()]


def gmres(A, b, x0, Minv=None, restart=30, rtol=1e-8, maxiter=300):
    """dict(its, hist, reason, x, refused, claims, last=(k, beta)): reason as mi_gmres_solve_dev reports it; refused the claims of the
    recurrence that the next cycle's start did not confirm; claims every (iterations, true relative residual behind the claim's update)."""
    A, b = np.asarray(A, np.float64), np.asarray(b, np.float64)
    x = np.array(x0, np.float64)
    n = len(b)
    norm = lambda v: float(np.sqrt(v @ v))
    bnorm = D.bnorm_of(norm(b))
    its, hist, refused, claimed, claims = 0, [], 0, False, []
    while True:
        r = b - A @ x
        beta = norm(r)
        rel, reason = D.cycle_start(beta, bnorm, its, rtol, maxiter)
        if not hist:
            hist.append(rel)
        if claimed:
            claims.append((its, rel))
            if reason != 1:
                refused += 1
            claimed = False
        if reason is not None:
            return dict(its=its, hist=hist, reason=reason, x=x, refused=refused, claims=claims, last=(0, beta))
        V32 = np.zeros((restart + 1, n), np.float32)
        with np.errstate(all="ignore"):
            V32[0] = round32(r / beta)
        q = widen(V32[0])
        cyc = D.Cycle(restart, beta, bnorm, rtol)
        while cyc.k < restart and its < maxiter and not cyc.reason:
            k = cyc.k
            w = A @ (q if Minv is None else Minv @ q)
            B = widen(V32[: k + 1])
            h = np.zeros(k + 1)
            for _ in range(2):
                d = B @ w  # every dot against the same w
                for dj, v in zip(d, B):
                    w = w - dj * v
                h = h + d
            nrm = norm(w)
            entry = cyc.step(list(h) + [nrm])
            if entry is None:
                break
            its += 1
            hist.append(entry)
            with np.errstate(all="ignore"):
                V32[k + 1] = round32(w / nrm)
            q = widen(V32[k + 1])
        k = cyc.k
        if k:
            u = np.array(cyc.solve()) @ widen(V32[:k])
            x = x + (u if Minv is None else Minv @ u)
        if cyc.reason == 1:
            claimed = True  # the update has run; the next start confirms or refuses
            continue
        if cyc.reason:
            return dict(its=its, hist=hist, reason=cyc.reason, x=x, refused=refused, claims=claims, last=(k, beta))
        if its >= maxiter:
            return dict(its=its, hist=hist, reason=2, x=x, refused=refused, claims=claims, last=(k, beta))


# the edges of round32: ties both ways, the float subnormals and the smallest normal, what rounds to 0, -0, the largest float, the
# tie above it and a value far beyond (Inf), NaN — each with both signs (tests/test_gmres_f32_model.py says what each becomes)
EDGE_VALUES = [s * v for v in (1.0 + 2.0 ** -24, 1.0 + 3.0 * 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -52, 2.0 ** -126 - 2.0 ** -149, 2.0 ** -126,
                               2.0 ** -149, 2.0 ** -150, 3.0 * 2.0 ** -151, 2.0 ** -151, 0.0, 0.1, 1.0 / 3.0, 3.4028234663852886e38,
                               2.0 ** 128 - 2.0 ** 103, 1e39, 1e300, 5e-324) for s in (1.0, -1.0)] + [float("nan")]

# the refusal case of tests/test_gmres_f32_model.py and tests/test_gpu_gmres_f32.py: (matrix of tests/bilu4_cases.py, fill, restart,
# rtol) — 124 rows, well conditioned, converging inside its first cycle: the claim comes with a true residual above rtol
REFUSAL_CASE = ("random:72", None, 30, 1e-8)
