"""The float-basis GMRES of include/mi355_spmv.h (MI_BASIS_F32) as tests/gmres_f32_model.py models it, no GPU: round32 against the
bytes struct.pack('f', ..) writes at the edge values of the DEFINITION, and the model's convergence — on the history cases of
tests/gmres_model.py it ends with reason 1, every reason 1 stands on a recomputed true residual <= rtol, and on the refusal case
(which tests/test_gpu_gmres_f32.py runs on the device) the recurrence's first claim is refused."""
import math
import struct

import numpy as np
import pytest

import gmres_f32_model as F
import gmres_model as G

RTOL = 1e-8


def _bits32(f):
    return struct.unpack("<I", struct.pack("<f", f))[0]


EDGES = [
    (1.0 + 2.0 ** -24, 1.0),                       # a tie: to even, down
    (1.0 + 3.0 * 2.0 ** -24, 1.0 + 2.0 ** -22),    # a tie: to even, up
    (1.0 + 2.0 ** -24 + 2.0 ** -52, 1.0 + 2.0 ** -23),  # just above a tie
    (2.0 ** -126 - 2.0 ** -149, 2.0 ** -126 - 2.0 ** -149),  # the largest float subnormal: kept
    (2.0 ** -126, 2.0 ** -126),                    # the smallest normal float
    (2.0 ** -149, 2.0 ** -149),                    # the smallest subnormal
    (2.0 ** -150, 0.0),                            # a tie between 0 and the smallest subnormal: to even, 0
    (3.0 * 2.0 ** -151, 2.0 ** -149),              # above that tie
    (-0.0, -0.0),
    (0.1, struct.unpack("<f", struct.pack("<f", 0.1))[0]),
    (-1.0 / 3.0, struct.unpack("<f", struct.pack("<f", -1.0 / 3.0))[0]),
    (3.4028234663852886e38, 3.4028234663852886e38),  # the largest float
    (2.0 ** 128 - 2.0 ** 103, math.inf),           # the tie above the largest float: to even, Inf
]


@pytest.mark.parametrize("v,want", EDGES)
def test_round32_at_the_edges_of_the_definition(v, want):
    for s in (1.0, -1.0):
        got = F.round32(s * v)
        assert got.dtype == np.float32
        if math.isfinite(want):  # struct.pack rounds a double to float itself (it raises beyond the range)
            assert _bits32(float(got)) == _bits32(s * want), (v, got)
            assert struct.pack("<f", float(got)) == struct.pack("<f", s * v), (v, got)
        else:
            assert float(got) == s * want, (v, got)
        assert F.widen(got) == float(got) and F.widen(got).dtype == np.float64


def test_round32_beyond_the_range_and_nan():
    assert F.round32(1e39) == math.inf and F.round32(-1e39) == -math.inf
    assert math.isnan(float(F.round32(math.nan)))
    assert math.copysign(1.0, float(F.round32(-0.0))) == -1.0 and math.copysign(1.0, float(F.round32(-2.0 ** -151))) == -1.0
    v = np.array([1.0 + 2.0 ** -24, 1e39, -0.0, 2.0 ** -150, math.nan])
    got = F.round32(v)
    assert got.dtype == np.float32 and got.shape == v.shape
    assert got[0] == 1.0 and got[1] == math.inf and got[3] == 0.0 and math.isnan(got[4])


@pytest.mark.parametrize("restart", G.RESTARTS)
@pytest.mark.parametrize("case", G.HISTORY_CASES, ids=lambda c: f"{c[0]}-{'none' if c[1] is None else 'ilu%d' % c[1]}")
def test_model_converges_and_every_reason_one_is_a_true_residual(case, restart):
    """Restart 30: every case ends with reason 1.  Restart 5: wherever the double reference converges within 300 iterations (all
    but fe:3 and fe:6 without a preconditioner, where it does not either)."""
    name, fill = case
    A, Minv, b = G.problem(name, fill)
    ref = G.gmres(A, b, np.zeros_like(b), Minv, restart=restart, rtol=RTOL, maxiter=300)
    r = F.gmres(A, b, np.zeros_like(b), Minv, restart=restart, rtol=RTOL, maxiter=300)
    true = G.true_residual(A, r["x"], b)
    print(f"{name} fill {fill} restart {restart}: {r['its']} iterations (double reference {ref[0]}), reason {r['reason']}, refused {r['refused']}, true {true:.3e}")
    assert len(r["hist"]) == r["its"] + 1
    if restart == 30 or ref[1][-1] <= RTOL:
        assert r["reason"] == 1, r["reason"]
    else:
        assert (r["its"], r["reason"]) == (300, 2)
    if r["reason"] == 1:
        assert true <= RTOL, true  # (longdouble, against beta / bnorm in float64: the difference is of the order of 1e-16)
        assert r["last"][0] == 0 and r["claims"][-1][1] <= RTOL and r["refused"] == len(r["claims"]) - 1
    # the float basis costs a few iterations at most (1 to 11 in the emulation the design rests on)
    assert ref[0] <= r["its"] <= ref[0] + 11 or r["reason"] == 2, (r["its"], ref[0])


def test_refusal_case_is_refused_by_the_model():
    name, fill, restart, rtol = F.REFUSAL_CASE
    A, Minv, b = G.problem(name, fill)
    assert len(b) == 124 and np.linalg.cond(A) < 10.0  # well conditioned
    r = F.gmres(A, b, np.zeros_like(b), Minv, restart=restart, rtol=rtol, maxiter=300)
    print(f"refusal case: {r['its']} iterations, claims {r['claims']}, refused {r['refused']}")
    assert r["reason"] == 1 and r["refused"] >= 1
    its0, true0 = r["claims"][0]
    assert its0 < restart and true0 > 2 * rtol  # inside the first cycle, and not a near miss: the device sees it too
    assert r["hist"][its0] <= rtol < true0
    assert G.true_residual(A, r["x"], b) <= rtol


def test_model_exits():
    A, Minv, b = G.problem("random:31", None)
    n = len(b)
    r = F.gmres(A, np.zeros(n), np.zeros(n))
    assert (r["its"], r["hist"], r["reason"], r["refused"]) == (0, [0.0], 0, 0)
    r = F.gmres(A, b, np.linalg.solve(A, b))
    assert (r["its"], r["reason"]) == (0, 0) and len(r["hist"]) == 1
    for maxiter in (0, 1, 5, 6):
        r = F.gmres(A, b, np.zeros(n), restart=5, rtol=1e-30, maxiter=maxiter)
        assert (r["its"], r["reason"], r["refused"]) == (maxiter, 2, 0) and len(r["hist"]) == maxiter + 1
    bad = b.copy()
    bad[3] = np.nan
    r = F.gmres(A, bad, np.zeros(n))
    assert (r["its"], r["reason"]) == (0, 4) and np.isnan(r["hist"][0])
    # a claim at maxiter that the start does not confirm ends with reason 2 and is counted
    name, fill, restart, rtol = F.REFUSAL_CASE
    A, Minv, b = G.problem(name, fill)
    n = len(b)
    full = F.gmres(A, b, np.zeros(n), restart=restart, rtol=rtol, maxiter=300)
    r = F.gmres(A, b, np.zeros(n), restart=restart, rtol=rtol, maxiter=full["claims"][0][0])
    assert (r["its"], r["reason"], r["refused"]) == (full["claims"][0][0], 2, 1) and r["last"][0] == 0
