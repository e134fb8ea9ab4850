"""What mi_gmres_info counts (include/mi355_spmv.h): launches_last of the eager solve, exactly, and that nothing but mi_gmres_solve_dev
writes launches_last, readbacks_last and wasted_steps_last.

  launches   6 for the first start and 5 for a later one; 4 per ENQUEUED step (counted or wasted), 5 with a preconditioner; 2 per
             end with k > 0, 5 with a preconditioner.  rtol 1e-30, maxiter 12, restart 5: three starts, three ends, no freeze, for
             check_every in {1, 2, 5, 9}; on chain with ILU(0), which is exact there, the double basis ends early instead (tests/
             test_gpu_gmres_dev.py) and the starts and ends are counted from its iterations and its last cycle.  maxiter 0: the
             start alone.  A solve that converges at a step: as many starts as ends
  untouched  prepare_stream(), two cycle() calls, plan() and plan.solve() leave the three counts of the last eager solve alone, and
             they are 0 on a solver that has only run cycle()"""
import numpy as np
import pytest

import bilu4_cases as C
from test_gpu_gmres_dev import RTOL, _dev, _precond, _rhs

pytestmark = pytest.mark.gpu

RESTART = 5
COUNTS = ("launches_last", "readbacks_last", "wasted_steps_last")


def _system(name, kind):
    from navierstokes_amd import mpk
    mat = C.matrix(name)
    M, F = _precond(kind, mat)
    return mpk.bcsr4x4_matrix(*mat), M, F, 4 * mat[0]


def _launches(p, starts, steps, ends):
    return 6 + 5 * (starts - 1) + (4 + p) * steps + ends * (5 if p else 2)


@pytest.mark.parametrize("basis", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["none", "ilu0"])
@pytest.mark.parametrize("name", ["chain", "random:31"])
def test_launches_of_the_eager_solve_are_exact(name, kind, basis):
    import torch
    from navierstokes_amd import mpk
    A, M, F, n = _system(name, kind)
    p = 0 if M is None else 1
    b, x0 = _dev(_rhs(n)), _dev(np.zeros(n))
    S = mpk.gmres_solver(A, M, RESTART, basis=basis)
    for check_every in (1, 2, 5, 9):
        its, _, reason = S.solve(b, x0.clone(), rtol=1e-30, maxiter=12, check_every=check_every)
        torch.cuda.synchronize()
        info, last_k = S.info(), S.fetch_cycle()[0]
        print(f"{name} {kind} {basis} check_every {check_every}: {its} iterations, reason {reason}, last k {last_k}, {info}")
        if (name, kind, basis) != ("chain", "ilu0", "f64"):
            assert (its, reason, S.basis_info()["refused_last"]) == (12, 2, 0)
            assert info["launches_last"] == 6 + 5 * 2 + (4 + p) * (12 + info["wasted_steps_last"]) + 3 * (5 if p else 2), info
        else:  # an exact preconditioner and a double basis: over after a few iterations, every cycle but the last one full
            assert 0 < its < 12 and reason != 2
            ends = -(-its // RESTART)
            starts = ends + (1 if last_k == 0 else 0)
            assert info["launches_last"] == _launches(p, starts, its + info["wasted_steps_last"], ends), (info, its, last_k)
    its, _, reason = S.solve(b, x0.clone(), rtol=1e-30, maxiter=0)
    info = S.info()
    assert (its, reason) == (0, 2) and info["launches_last"] == 6 and info["wasted_steps_last"] == 0, info
    if basis == "f64":  # converging at a step: the last cycle has an end, so as many starts as ends
        its, _, reason = S.solve(b, x0.clone(), rtol=RTOL, maxiter=300, check_every=2)
        torch.cuda.synchronize()
        info, last_k = S.info(), S.fetch_cycle()[0]
        assert its > 0 and reason == 1 and last_k > 0, (its, reason, last_k)
        cycles = -(-its // RESTART)
        assert info["launches_last"] == _launches(p, cycles, its + info["wasted_steps_last"], cycles), (info, its)
    for obj in (S, F, A):
        if obj is not None:
            obj.close()


@pytest.mark.parametrize("basis", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["none", "ilu0"])
@pytest.mark.parametrize("name", ["chain", "random:31"])
def test_raw_cycles_and_plans_leave_the_counts_of_the_last_eager_solve(name, kind, basis):
    import torch
    from navierstokes_amd import mpk
    A, M, F, n = _system(name, kind)
    b, x = _dev(_rhs(n)), _dev(np.zeros(n))
    S = mpk.gmres_solver(A, M, RESTART, basis=basis)
    S.solve(b, x, rtol=1e-30, maxiter=12, check_every=2)
    want = {c: S.info()[c] for c in COUNTS}
    assert want["launches_last"] > 0 and want["readbacks_last"] > 0
    S.prepare_stream()
    S.cycle(b, x, True, RTOL, 300)
    S.cycle(b, x, False, RTOL, 300)
    P = S.plan(b, x, rtol=RTOL, maxiter=300, segment=2)
    P.solve()
    torch.cuda.synchronize()
    assert {c: S.info()[c] for c in COUNTS} == want
    fresh = mpk.gmres_solver(A, M, RESTART, basis=basis)
    fresh.cycle(b, x, True, RTOL, 300)
    torch.cuda.synchronize()
    assert {c: fresh.info()[c] for c in COUNTS} == dict.fromkeys(COUNTS, 0)
    for obj in (P, fresh, S, F, A):
        if obj is not None:
            obj.close()
