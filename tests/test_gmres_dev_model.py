"""The specification of mi_gmres_*'s small problem (tests/gmres_dev_model.py: Givens rotations, the recurrence for the residual,
back-substitution, all from raw Gram-Schmidt columns, one rounded operation at a time) against the dense reference of
tests/gmres_model.py, which solves the least-squares problem afresh with numpy.linalg.lstsq at every iteration and shares none of
that.  On the CPU, before any kernel: the raw columns are those of the reference's own Arnoldi (its float64 operations, repeated
here), on G.HISTORY_CASES x G.RESTARTS.

  history   every entry within the bound tests/test_gpu_gmres.py derives from the reference's own spread (1.6e-8 relative, above
            the floor 1e-10), the same count, len(history) == iterations + 1
  y         at the end of every cycle y solves min || beta e1 - Hbar y || to 1e-12: Givens QR is backward stable, y is the exact
            solution for Hbar + E with ||E|| <= c eps ||Hbar|| (c of the order k^1.5), hence the normal-equations residual
            || Hbar^T (beta e1 - Hbar y) || <= ||E|| (||r|| + ||Hbar|| ||y||); asserted with c eps = 1e-12, in numpy.longdouble
  exits     rho = 0 and a NaN column give reason 4 and are not counted; a frozen cycle ignores later columns; nrm = 0 gives reason
            3 only when rtol is negative (g_{k+1} = 0 then, so any rtol >= 0 reports 1)"""
import numpy as np
import pytest

import gmres_dev_model as D
import gmres_model as G

RTOL = 1e-8
FLOOR = 1e-10
HISTORY_BOUND = 1.6e-8  # tests/test_gpu_gmres.py
LSQ_BOUND = 1e-12


def run(A, b, Minv, restart, rtol=RTOL, maxiter=300, check_y=True):
    """(iterations, history, reason, x) of the model driven by the reference's Arnoldi."""
    norm = lambda v: float(np.sqrt(v @ v))
    x = np.zeros_like(b)
    bnorm = D.bnorm_of(norm(b))
    its, hist = 0, []
    while True:
        r = b - A @ x
        beta = norm(r)
        rel, reason = D.cycle_start(beta, bnorm, its, rtol, maxiter)
        if not hist:
            hist.append(rel)
        if reason is not None:
            return its, hist, reason, x
        V = [r / beta]
        cyc = D.Cycle(restart, beta, bnorm, rtol)
        Hbar = np.zeros((restart + 1, restart))
        while cyc.k < restart and its < maxiter and not cyc.reason:
            k = cyc.k
            w = A @ (V[k] if Minv is None else Minv @ V[k])
            h = np.zeros(k + 1)
            for _ in range(2):
                d = np.array([v @ w for v in V])
                for dj, v in zip(d, V):
                    w = w - dj * v
                h = h + d
            nrm = norm(w)
            Hbar[: k + 1, k], Hbar[k + 1, k] = h, nrm
            entry = cyc.step(list(h) + [nrm])
            if entry is None:
                break
            its += 1
            hist.append(entry)
            if nrm != 0.0:
                V.append(w / nrm)
        k = cyc.k
        if k:
            y = np.array(cyc.solve())
            if check_y:
                L = np.longdouble
                Hk = Hbar[: k + 1, :k].astype(L)
                e1 = np.zeros(k + 1, L)
                e1[0] = beta
                res = e1 - Hk @ y.astype(L)
                nH = float(np.linalg.norm(Hbar[: k + 1, :k], 2))
                grad = float(np.sqrt((Hk.T @ res) @ (Hk.T @ res)))
                assert grad <= LSQ_BOUND * nH * (float(np.sqrt(res @ res)) + nH * norm(y)), (k, grad)
                # and the recurrence's last entry is that residual
                assert abs(float(np.sqrt(res @ res)) / bnorm - hist[-1]) <= HISTORY_BOUND * max(hist[-1], FLOOR)
            u = sum(yj * v for yj, v in zip(y, V))
            x = x + (u if Minv is None else Minv @ u)
        if cyc.reason:
            return its, hist, cyc.reason, x
        if its >= maxiter:
            return its, hist, 2, x


@pytest.mark.parametrize("restart", G.RESTARTS)
@pytest.mark.parametrize("case", G.HISTORY_CASES, ids=lambda c: f"{c[0]}-{'none' if c[1] is None else 'ilu%d' % c[1]}")
def test_history_agrees_with_the_lstsq_reference(case, restart):
    A, Minv, b = G.problem(*case)
    rits, rhist, _ = G.gmres(A, b, np.zeros_like(b), Minv, restart=restart, rtol=RTOL, maxiter=300)
    its, hist, reason, x = run(A, b, Minv, restart)
    assert len(hist) == its + 1
    worst = max((abs(h - r) / r for h, r in zip(hist, rhist) if r > FLOOR), default=0.0)
    print(f"{case} restart {restart}: {its} iterations (reference {rits}), history within {worst:.3e}, reason {reason}")
    assert worst <= HISTORY_BOUND, worst
    near = RTOL / 2 <= rhist[-1] <= 2 * RTOL
    assert its == rits or (near and abs(its - rits) == 1), (its, rits)
    if hist[-1] <= RTOL:
        assert reason == 1 and G.true_residual(A, x, b) <= 10 * RTOL
    else:  # (fe:3 without M at restart 5 stagnates: the reference runs into maxiter as well)
        assert (its, reason) == (300, 2)


def test_maxiter_clips_a_cycle():
    A, Minv, b = G.problem("fe:3", 0)
    for maxiter in (1, 5, 6, 12):
        its, hist, reason, x = run(A, b, Minv, 5, rtol=1e-30, maxiter=maxiter)
        ref = G.gmres(A, b, np.zeros_like(b), Minv, restart=5, rtol=1e-30, maxiter=maxiter)
        assert (its, reason, len(hist)) == (maxiter, 2, maxiter + 1) and ref[0] == maxiter
        assert np.abs(x - ref[2][-1]).max() <= 1e-9 * np.abs(x).max()
    assert run(A, b, Minv, 5, maxiter=0)[:3] == (0, [1.0], 2)


def test_cycle_start_exits():
    assert D.cycle_start(0.0, 1.0, 0, RTOL, 300) == (0.0, 0)
    assert D.cycle_start(1e-9, 1.0, 7, RTOL, 300) == (1e-9, 1)
    assert D.cycle_start(0.5, 1.0, 300, RTOL, 300) == (0.5, 2)
    rel, reason = D.cycle_start(float("nan"), 1.0, 0, RTOL, 300)
    assert np.isnan(rel) and reason == 4
    assert D.cycle_start(float("inf"), 1.0, 0, RTOL, 300)[1] == 4
    assert D.bnorm_of(0.0) == 1.0 and D.bnorm_of(2.5) == 2.5 and np.isnan(D.bnorm_of(float("nan")))


def test_uncounted_steps_and_the_frozen_state():
    c = D.Cycle(4, 2.0, 1.0, RTOL)
    assert c.step([0.0, 0.0]) is None and (c.reason, c.k) == (4, 0)  # rho = 0
    assert c.step([1.0, 1.0]) is None and c.k == 0  # frozen
    c = D.Cycle(4, 2.0, 1.0, RTOL)
    assert c.step([3.0, 4.0]) == pytest.approx(2.0 * 0.8) and c.k == 1
    assert c.step([1.0, float("nan"), 1.0]) is None and (c.reason, c.k) == (4, 1)
    assert c.solve() == [2.0 * 0.6 / 5.0]
    # nrm = 0: the new g is 0 and the entry 0, so rtol >= 0 reports 1 and only a negative rtol reports 3
    for rtol, reason in ((0.0, 1), (RTOL, 1), (-1.0, 3)):
        c = D.Cycle(4, 2.0, 1.0, rtol)
        assert c.step([3.0, 0.0]) == 0.0 and c.reason == reason
        assert c.step([1.0, 1.0, 1.0]) is None
        assert c.solve() == [2.0 / 3.0]
