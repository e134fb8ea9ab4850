"""The model of the single-precision copy of the block ILU factor (tests/bilu4_sp_model.py) and its two hand-made cases
(tests/bilu4_sp_cases.py), without a GPU:

  planted    the values planted in block row 0 of sp_edges / sp_overflow are in the model's factor bit for bit, Dinv_0 is exact,
             and no other row's factor depends on them
  rounding   round_factor makes of each what the definition says: ties to even, subnormals kept, -0, Inf beyond the range
  overflow   overflowed gives (0, -1) for sp_edges and (2, 0) for sp_overflow
  clamp      the clamped solve_sweeps_sp is bilu4_model.solve on the rounded factor, bit for bit
  gmres      with the dense operator of the ROUNDED factor gmres_model.gmres takes the iterations it takes with the double factor
"""
import numpy as np
import pytest

import bilu4_cases as C
import bilu4_model as M
import bilu4_sp_cases as SC
import bilu4_sp_model as SP
import bilu4_sweeps_model as S
import gmres_model as G
from conftest import assert_bit_equal


def test_the_planted_values_are_in_the_factor_bit_for_bit():
    nb = SC.NB
    fac = SC.model_factor("sp_edges", 0)
    ptr, col, diag, val = fac
    assert nb == 70 and len(ptr) == nb + 1 and int(diag[0]) == 0
    blk = SC.planted_block("sp_edges", fac)
    assert_bit_equal(blk[:len(SC.PLANTED)], np.array([v for v, _ in SC.PLANTED]), "planted values")
    assert_bit_equal(val[0], np.diag([SC.DINV00, 1.0, 0.5, 2.0]), "Dinv_0")
    over = SC.model_factor("sp_overflow", 0)
    assert_bit_equal(SC.planted_block("sp_overflow", over)[[5, 10]], np.array(SC.OVERFLOW), "planted overflows")
    # nothing leaks: beyond block row 0 the two factors are the same, and they are those of the pattern without the planted values
    assert_bit_equal(val[ptr[1]:], over[3][ptr[1]:], "rows 1.. of the two cases")
    _, bp, bc, bv = SC.matrix("sp_edges")
    plain = np.array(bv).reshape(-1, 4, 4)
    plain[bp[0] + 1:bp[1]] = 0.25
    assert_bit_equal(M.factor(nb, bp, bc, plain.reshape(-1), 0)[3][ptr[1]:], val[ptr[1]:], "rows 1.. without the planted values")
    for fill in (0, 1):  # (fill adds nothing to row 0 and nothing in column 0)
        p1, c1, d1, v1 = SC.model_factor("sp_edges", fill)
        assert list(c1[p1[0]:p1[1]]) == list(SC.ROW0_COLS) and not any(0 in c1[p1[i]:p1[i + 1]] for i in range(1, nb))


def test_round_factor_is_the_definition():
    vals = np.array([v for v, _ in SC.PLANTED] + [SC.DINV00] + SC.OVERFLOW + [-1e300, np.inf, -np.inf])
    want = np.array([w for _, w in SC.PLANTED] + [SC.DINV00, np.inf, np.inf, -np.inf, np.inf, -np.inf])
    got = SP.round_factor(vals)
    assert got.dtype == np.float32
    assert_bit_equal(got.astype(np.float64), want, "round_factor of the planted values")
    assert np.isnan(SP.round_factor(np.array([np.nan]))[0])
    # the subnormals are floats, not doubles that happen to be small: their float bits
    assert list(SP.round_factor(np.array([2.0 ** -127, 2.0 ** -149, SC.DINV00, -(2.0 ** -151)])).view(np.uint32)) == [1 << 22, 1, 1 << 9, 1 << 31]
    fac = SC.model_factor("sp_edges", 0)
    r = SP.round_factor(fac[3])
    assert r.shape == np.asarray(fac[3]).shape
    assert_bit_equal(SC.planted_block("sp_edges", SP.rounded(fac))[:len(SC.PLANTED)], np.array([w for _, w in SC.PLANTED]), "the rounded factor")


def test_overflowed_counts_and_names_the_first_block_row():
    e, o = SC.model_factor("sp_edges", 0), SC.model_factor("sp_overflow", 0)
    assert SP.overflowed(e[3], e[0]) == (0, -1)
    assert SP.overflowed(o[3], o[0]) == (2, 0)
    assert SP.overflowed(*[SC.model_factor("sp_overflow", 0, 1)[k] for k in (3, 0)]) == (1, 0), "halved: only 1e300 / 2 is left outside"
    ptr, _, diag, val = C.model_factor("arrow", 0)
    v = np.array(val)
    v[diag[5]][1, 2] = -1e39
    v[ptr[9]][0, 0] = 1e39
    v[ptr[9]][3, 3] = np.inf  # not finite as double: not counted
    assert SP.overflowed(v, ptr) == (2, 5)
    assert SP.overflowed(val, ptr) == (0, -1)


CLAMP_CASES = [("fe:6", 0), ("arrow", 0)] + [(f"random:{s}", s % 3) for s in range(10)] + [("sp_edges", 0), ("sp_overflow", 0)]


@pytest.mark.parametrize("name,fill", CLAMP_CASES, ids=[C.case_id(c) for c in CLAMP_CASES])
def test_the_clamped_sweeps_are_the_exact_solve_of_the_rounded_factor(name, fill):
    nb = SC.matrix(name)[0]
    fac = SC.model_factor(name, fill)
    ptr, col, diag, val = SP.rounded(fac)
    sched = (M.schedule(nb, ptr, col, diag, False), M.schedule(nb, ptr, col, diag, True))
    b = np.random.default_rng(300 + nb).standard_normal(4 * nb)
    want = M.solve(nb, ptr, col, diag, val, b, sched)
    got = SP.solve_sweeps_sp(nb, *fac, b, 10 ** 6, 10 ** 6)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and nan.any() == (name == "sp_overflow")
    assert_bit_equal(np.where(nan, 0.0, got), np.where(nan, 0.0, want), f"{name} fill {fill} clamped, rounded factor")
    if name != "sp_overflow":
        assert not np.array_equal(got, S.solve_sweeps(nb, *fac, b, 10 ** 6, 10 ** 6)), "rounding the factor changed nothing"
    else:
        assert np.isfinite(got[4:]).all(), "row 0 is a sink: its Inf reaches no other row"


@pytest.mark.parametrize("name,counts", [("fe:6", (26, 21, 18)), ("fe:10", (33, 28, 24))])
def test_gmres_takes_the_same_iterations_with_the_rounded_factor(name, counts):
    A, _, b = G.problem(name, None)
    nb = C.matrix(name)[0]
    fac = C.model_factor(name, 0)
    for s, its in zip((2, 3, 4), counts):
        r32 = G.gmres(A, b, np.zeros_like(b), S.dense_operator(nb, SP.rounded(fac), s, s), restart=30, rtol=1e-8, maxiter=300)
        r64 = G.gmres(A, b, np.zeros_like(b), S.dense_operator(nb, fac, s, s), restart=30, rtol=1e-8, maxiter=300)
        worst = max(abs(x - y) / y for x, y in zip(r32[1], r64[1]))
        print(f"{name}, {s} sweeps: {r32[0]} iterations with the rounded factor, {r64[0]} with the double one; histories differ by {worst:.2e} relative")
        assert r32[0] == its and r64[0] == its, (s, r32[0], r64[0], its)
        assert r32[1][-1] <= 1e-8
