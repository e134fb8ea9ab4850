"""The small problem of mi_gmres_* (include/mi355_spmv.h; gmres_kernels.hpp: gmres_cycle_begin, gmres_hess_step, gmres_backsolve)
restated in Python float64 scalars: the Givens rotations, the residual recurrence g, the history, the stopping rule with its
frozen state, and the back-substitution, from RAW Gram-Schmidt columns.  Every product, sum, difference, division and the square
root is one correctly rounded IEEE operation (Python's float arithmetic and math.sqrt never contract into an fma), which is the
interface's ARITHMETIC: the device must produce these bits.

A column is fed as (h_0..h_k, nrm): the dots of mi_cgs_dev(passes=2) and the norm, untouched."""
import math


def bnorm_of(norm_b):
    """||b|| as the norm kernel wrote it, or 1 where that is 0 (NaN stays NaN)."""
    return 1.0 if norm_b == 0.0 else norm_b


def cycle_start(beta, bnorm, its, rtol, maxiter):
    """(beta / bnorm, reason or None): the three ends of a solve at a cycle's start, in order."""
    rel = beta / bnorm
    if rel <= rtol:
        return rel, (0 if its == 0 else 1)
    if its >= maxiter:
        return rel, 2
    if not math.isfinite(beta):
        return rel, 4
    return rel, None


class Cycle:
    """One restart cycle's small state.  step(column) returns the history entry, or None for a step that is not counted (reason 4,
    or a frozen cycle)."""

    def __init__(self, restart, beta, bnorm, rtol):
        self.m, self.bnorm, self.rtol = restart, bnorm, rtol
        self.cs, self.sn = [0.0] * restart, [0.0] * restart
        self.g = [0.0] * (restart + 1)
        self.g[0] = beta
        self.R = [[0.0] * restart for _ in range(restart)]  # R[j][k]
        self.k = 0
        self.reason = 0

    def step(self, column):
        if self.reason:
            return None  # frozen
        k = self.k
        c = [float(v) for v in column]
        assert len(c) == k + 2
        cs, sn, g = self.cs, self.sn, self.g
        for j in range(k):
            t = cs[j] * c[j] + sn[j] * c[j + 1]
            c[j + 1] = (-sn[j]) * c[j] + cs[j] * c[j + 1]
            c[j] = t
        nrm = c[k + 1]
        rho = math.sqrt(c[k] * c[k] + nrm * nrm)
        if rho == 0.0 or not math.isfinite(rho):
            self.reason = 4
            return None
        cs[k], sn[k] = c[k] / rho, nrm / rho
        for j in range(k):
            self.R[j][k] = c[j]
        self.R[k][k] = rho
        g[k + 1] = (-sn[k]) * g[k]
        g[k] = cs[k] * g[k]
        self.k = k + 1
        h = abs(g[k + 1]) / self.bnorm
        if h <= self.rtol:
            self.reason = 1
        elif nrm == 0.0:
            self.reason = 3
        return h

    def solve(self):
        """y of the k counted steps: for i = k-1 .. 0, s = g_i, s -= R_ij y_j for j ascending, y_i = s / R_ii."""
        k = self.k
        y = [0.0] * k
        for i in range(k - 1, -1, -1):
            s = self.g[i]
            for j in range(i + 1, k):
                s = s - self.R[i][j] * y[j]
            y[i] = s / self.R[i][i]
        return y
