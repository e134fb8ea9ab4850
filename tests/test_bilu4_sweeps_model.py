"""The model of the sweep solve (tests/bilu4_sweeps_model.py) against what it must reduce to, without a GPU:

  bits       at (fwd_levels - 1, bwd_levels - 1) sweeps it equals bilu4_model.solve BIT for bit, and ten times as many sweeps
             (not clamped) change nothing: a row of level l is final after l sweeps
  short      one sweep short, forward or backward, the result differs (on the cases where the last level's contribution is
             above rounding: not on `chain`)
  operator   it agrees with dense_operator @ b to a few ulps of the operator's norm (32 eps of the absolute-value operator on |b|)
  gmres      as a preconditioner, s = 4 sweeps per triangle cost at most 1.5 times the exact solve's iterations on fe:6 and fe:10
"""
import numpy as np
import pytest

import bilu4_cases as C
import bilu4_model as M
import bilu4_sweeps_model as S
import gmres_model as G
from conftest import assert_bit_equal

BIT_CASES = [("chain", 0), ("arrow", 0), ("arrow", 1), ("fe:3", 0), ("fe:3", 2), ("fe:6", 0), ("random:7", 1), ("random:12", 0), ("random:31", 1),
             ("limits:0", 0)]
SHORT_CASES = [("arrow", 0), ("fe:3", 0), ("random:12", 0), ("limits:0", 0)]


def _b(nb, seed=0):
    return np.random.default_rng(100 + seed + nb).standard_normal(4 * nb)


def _exact(nb, fac, b):
    ptr, col, diag, val = fac
    sched = (M.schedule(nb, ptr, col, diag, False), M.schedule(nb, ptr, col, diag, True))
    return M.solve(nb, ptr, col, diag, val, b, sched)


@pytest.mark.parametrize("name,fill", BIT_CASES, ids=[C.case_id(c) for c in BIT_CASES])
def test_levels_minus_one_sweeps_are_the_exact_solve(name, fill):
    nb = C.matrix(name)[0]
    fac = C.model_factor(name, fill)
    mf, mb = S.max_sweeps(nb, *fac[:3])
    ptr, col, diag, _ = fac
    assert mf == M.schedule(nb, ptr, col, diag, False)["nlev"] - 1 and mb == M.schedule(nb, ptr, col, diag, True)["nlev"] - 1
    b = _b(nb)
    want = _exact(nb, fac, b)
    assert_bit_equal(S.solve_sweeps(nb, *fac, b, mf, mb, clamp=False), want, f"{name} fill {fill} at ({mf}, {mb})")
    assert_bit_equal(S.solve_sweeps(nb, *fac, b, 10 * mf, 10 * mb, clamp=False), want, f"{name} fill {fill} at ten times ({mf}, {mb})")
    assert_bit_equal(S.solve_sweeps(nb, *fac, b, 10 ** 6, 10 ** 6), want, f"{name} fill {fill} clamped")


@pytest.mark.parametrize("name,fill", SHORT_CASES, ids=[C.case_id(c) for c in SHORT_CASES])
def test_one_sweep_short_differs(name, fill):
    nb = C.matrix(name)[0]
    fac = C.model_factor(name, fill)
    mf, mb = S.max_sweeps(nb, *fac[:3])
    assert mf >= 1 and mb >= 1
    b = _b(nb)
    want = _exact(nb, fac, b)
    assert not np.array_equal(S.solve_sweeps(nb, *fac, b, mf - 1, mb), want), "the last forward sweep changed nothing"
    assert not np.array_equal(S.solve_sweeps(nb, *fac, b, mf, mb - 1), want), "the last backward sweep changed nothing"


def test_zero_sweeps_is_the_diagonal_and_an_empty_matrix_is_empty():
    name = "random:12"
    nb = C.matrix(name)[0]
    ptr, col, diag, val = C.model_factor(name, 0)
    b = _b(nb)
    assert_bit_equal(S.solve_sweeps(nb, ptr, col, diag, val, b, 0, 0), M.matvec4(val[diag], b.reshape(nb, 4)).reshape(-1), "x = Dinv b")
    e = np.zeros(0, np.int32)
    assert S.solve_sweeps(0, np.zeros(1, np.int32), e, e, np.zeros((0, 4, 4)), np.zeros(0), 3, 3).shape == (0,)
    assert S.max_sweeps(0, np.zeros(1, np.int32), e, e) == (0, 0)


OPERATOR_CASES = [("fe:3", 0, 2, 3), ("fe:3", 2, 4, 4), ("arrow", 0, 1, 1), ("random:31", 1, 3, 0), ("random:12", 0, 0, 2), ("chain", 0, 6, 5), ("fe:6", 0, 4, 4)]


@pytest.mark.parametrize("name,fill,sf,sb", OPERATOR_CASES, ids=[f"{c[0]}-fill{c[1]}-{c[2]}-{c[3]}" for c in OPERATOR_CASES])
def test_the_model_is_the_dense_operator(name, fill, sf, sb):
    """A few ulps of the operator's norm, componentwise: |model - dense_operator @ b|_i <= 32 eps (Abar |b|)_i, eps = 2^-53, Abar the
    operator built from the absolute values of the factor, (sum (|Dinv| |Us|)^j |Dinv|) (sum |Ls|^j) — the scale every rounding of
    either side is relative to.  32 = 2^5 is "a few" taken generously; it does not grow with n, the row length or the sweep counts.
    (The a-priori worst case, for comparison only, to first order in eps:
      the model:  a row of m blocks is 5 m roundings (four per chain, one subtraction), the Dinv chain 4 more; the error of one sweep
                  is at most (5 m + 4) eps times the absolute row sum, and it passes through the later sweeps, each bounded by
                  Abar's factors: (sf + sb + 1) (5 m_max + 4) eps (Abar |b|)_i over the sf + 1 + sb launches;
      the dense side:  sf + sb Horner products, two more to join the three factors and the product with b, each a dot product of
                  at most n terms: (sf + sb + 3) n eps (Abar |b|)_i, the worst case of recursive summation.
    That is 742 to 15 758 eps on these cases and is NOT what is asserted.)  The measured figure is printed as a multiple of
    eps (Abar |b|)_i; on these cases it is 0.1 to 9.9."""
    nb = C.matrix(name)[0]
    fac = C.model_factor(name, fill)
    ptr, col, diag, val = fac
    n = 4 * nb
    b = _b(nb, 1)
    got = S.solve_sweeps(nb, *fac, b, sf, sb, clamp=False)
    want = S.dense_operator(nb, fac, sf, sb) @ b
    # Abar from dense_operator itself: with -|L|, +|U| and -|Dinv| every power (-Ls)^j and (-Dinv Us)^j is entrywise >= 0, and the
    # trailing Dinv only flips the sign of the whole
    rows = np.repeat(np.arange(nb), np.diff(ptr))
    sign = np.where(col > rows, 1.0, -1.0)[:, None, None]
    scale = np.abs(S.dense_operator(nb, (ptr, col, diag, sign * np.abs(val)), sf, sb)) @ np.abs(b)
    m_max = int(np.max(np.diff(ptr))) - 1
    eps = 2.0 ** -53
    worst_case = (sf + sb + 1) * (5 * m_max + 4) + (sf + sb + 3) * n
    worst = float(np.max(np.abs(got - want) / (eps * scale)))
    print(f"{name} fill {fill} ({sf}, {sb}): largest difference {worst:.2f} eps (Abar |b|)_i (asserted: 32; a-priori worst case {worst_case})")
    assert (np.abs(got - want) <= 32 * eps * scale).all(), worst


@pytest.mark.parametrize("name,exact_its,sweep_its", [("fe:6", 16, 18), ("fe:10", 20, 24)])
def test_four_sweeps_cost_at_most_half_as_many_iterations_again(name, exact_its, sweep_its):
    """GMRES(30) to 1e-8 with the right-hand side of gmres_model.problem: the exact preconditioner against 4 sweeps per triangle.
    Measured: fe:6 16 and 18 iterations, fe:10 20 and 24."""
    A, Minv, b = G.problem(name, 0)
    nb = C.matrix(name)[0]
    Msw = S.dense_operator(nb, C.model_factor(name, 0), 4, 4)
    exact = G.gmres(A, b, np.zeros_like(b), Minv, restart=30, rtol=1e-8, maxiter=300)
    sweeps = G.gmres(A, b, np.zeros_like(b), Msw, restart=30, rtol=1e-8, maxiter=300)
    print(f"{name}: exact solve {exact[0]} iterations, 4 sweeps {sweeps[0]}")
    assert exact[1][-1] <= 1e-8 and sweeps[1][-1] <= 1e-8
    assert sweeps[0] <= 1.5 * exact[0], (sweeps[0], exact[0])
    assert abs(exact[0] - exact_its) <= 1 and abs(sweeps[0] - sweep_its) <= 1, "the counts the issue was argued from no longer hold"
