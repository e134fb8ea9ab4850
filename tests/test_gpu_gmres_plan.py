"""The capturable GMRES on the GPU (mi_gmres_plan_*, mi_gmres_cycle_dev, mi_gmres_state, mi_gmres_prepare_stream; mpk.gmres_plan,
gmres_solver.plan / cycle / state / prepare_stream).  Every comparison is bitwise, against the eager solve (mi_gmres_solve_dev,
tests/test_gpu_gmres_dev.py's solver_run), which that file pins to a loop composed from the library's public pieces.

  planned     history, count, reason, x and fetch_cycle of the planned solve equal the eager solve's for segment in {1, 2, 3, 5, 9},
              on fe:3, chain and random:31 with every preconditioner, restart 5, maxiter 12; the same with the float basis on fe:3
              and random:31, refused_last included; and solves that converge (a freeze inside a segment; with the float basis a
              claim and its confirming start); an exact ILU on its one-launch form, which the graphs hold level by level
  small       restart 1; restart 64 on random:62 with segment 7 and 64; one block (n = 4) with restart 30; b = 0; x0 the solution,
              with entries of -0.0; NaN in b; maxiter in {0, 1, 5, 6} at restart 5
  reuse       one plan solved twice with b and x refilled in place; a non-default stream; a capturing stream is refused and stays
              usable; MI_ERR_STATE after mi_gmres_set_precond; the number of graphs; wasted steps within 2 segment - 1
  raw cycle   cycle(first=1) and cycle(first=0) in two torch graphs after prepare_stream(), replayed with state() between them, reach
              the eager solve's x, count and reason; an unprepared capture is refused (status 6) and the graph's other node replays
  Newton      mi_bcsr4_update_values_dev + mi_bilu4dev_refactor + cycle(first=1) on fe:6 at fill 0 as ONE graph, replayed with a
              second set of values: x and the record equal the same three calls made eagerly"""
import ctypes
import math

import numpy as np
import pytest

import bilu4_cases as C
import gmres_model as G
from conftest import assert_bit_equal
from test_gpu_gmres_dev import PRECONDS, _dev, _precond, _rhs, solver_run

pytestmark = pytest.mark.gpu

RTOL = 1e-8
SEGMENTS = (1, 2, 3, 5, 9)


def eager_run(A, M, b, x0, restart, rtol, maxiter, basis="f64"):
    """(iterations, history, reason, x, fetch_cycle(), refused_last) of a fresh gmres_solver's eager solve."""
    import torch
    from navierstokes_amd import mpk
    if basis == "f64":
        return solver_run(A, M, b, x0, restart, rtol, maxiter, check_every=1)[:5] + (0,)
    S = mpk.gmres_solver(A, M, restart, basis=basis)
    x = x0.clone()
    its, hist, reason = S.solve(b, x, rtol=rtol, maxiter=maxiter, check_every=1)
    torch.cuda.synchronize()
    out = its, hist, reason, x.cpu().numpy(), S.fetch_cycle(), S.basis_info()["refused_last"]
    S.close()
    return out


def planned_run(A, M, b, x0, restart, rtol, maxiter, segment, basis="f64"):
    """The same of a fresh solver's planned solve, and the plan's info()."""
    import torch
    from navierstokes_amd import mpk
    S = mpk.gmres_solver(A, M, restart, basis=basis)
    x = x0.clone()
    P = S.plan(b, x, rtol=rtol, maxiter=maxiter, segment=segment)
    its, hist, reason = P.solve()
    torch.cuda.synchronize()
    info = P.info()
    out = its, hist, reason, x.cpu().numpy(), S.fetch_cycle(), S.basis_info()["refused_last"], info
    assert info["graphs"] == 3 + math.ceil(restart / min(segment, restart)) and info["segment"] == min(segment, restart), info
    P.close()
    S.close()
    return out


def assert_same(got, want, what):
    assert (got[0], got[2], got[5]) == (want[0], want[2], want[5]), (what, got[0], got[2], got[5], want[0], want[2], want[5])
    assert len(got[1]) == got[0] + 1
    assert_bit_equal(got[1], want[1], f"{what}: history")
    assert_bit_equal(got[3], want[3], f"{what}: x")
    (k, hraw, y, beta), (wk, whraw, wy, wbeta) = got[4], want[4]
    assert k == wk, (what, k, wk)
    assert_bit_equal(hraw, whraw, f"{what}: raw columns of the last cycle")
    assert_bit_equal(y, wy, f"{what}: y of the last cycle")
    assert_bit_equal([beta], [wbeta], f"{what}: beta of the last cycle")


def _within_waste_bound(info, basis, refused=0):
    """include/mi355_spmv.h, WASTE: 2 segment - 1 per cycle that ends early.  The double basis has one such cycle per solve; the
    float basis two per claim (the claimed cycle and its confirming start), claims = refused + 1 at most, and the solve's last."""
    early = 1 if basis == "f64" else 2 * (refused + 1) + 1
    assert 0 <= info["wasted_steps_last"] <= early * (2 * info["segment"] - 1), (info, early)


def _system(name, kind):
    from navierstokes_amd import mpk
    mat = C.matrix(name)
    A = mpk.bcsr4x4_matrix(*mat)
    M, F = _precond(kind, mat)
    n = 4 * mat[0]
    return A, M, F, n


def _close(*objs):
    for o in objs:
        if o is not None:
            o.close()


# ---------------------------------------------------------------- the planned solve against the eager one

@pytest.mark.parametrize("kind", PRECONDS)
@pytest.mark.parametrize("name", ["fe:3", "chain", "random:31"])
def test_planned_solve_equals_the_eager_solve(name, kind):
    A, M, F, n = _system(name, kind)
    b, x0 = _dev(_rhs(n)), _dev(np.zeros(n))
    want = eager_run(A, M, b, x0, 5, 1e-30, 12)
    for segment in SEGMENTS:
        got = planned_run(A, M, b, x0, 5, 1e-30, 12, segment)
        assert_same(got, want, f"{name} {kind} segment {segment}")
        _within_waste_bound(got[6], "f64")
        if want[0] == 12:  # three cycles, the last of two steps: clipped by maxiter inside a segment, nothing frozen
            assert got[6]["wasted_steps_last"] == (min(segment, 5) - 2 if segment >= 2 else 0), got[6]
    _close(F, A)


@pytest.mark.parametrize("kind", PRECONDS)
@pytest.mark.parametrize("name", ["fe:3", "random:31"])
def test_planned_solve_equals_the_eager_solve_with_the_float_basis(name, kind):
    A, M, F, n = _system(name, kind)
    b, x0 = _dev(_rhs(n)), _dev(np.zeros(n))
    want = eager_run(A, M, b, x0, 5, 1e-30, 12, basis="f32")
    for segment in SEGMENTS:
        got = planned_run(A, M, b, x0, 5, 1e-30, 12, segment, basis="f32")
        assert_same(got, want, f"float basis, {name} {kind} segment {segment}")
    _close(F, A)


@pytest.mark.parametrize("basis", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["none", "ilu0"])
def test_a_solve_that_converges_inside_a_segment(kind, basis):
    """rtol 1e-8 on random:31, restart 5: the cycle freezes at a step (with the float basis: a claim, then the confirming start)."""
    A, M, F, n = _system("random:31", kind)
    b, x0 = _dev(_rhs(n)), _dev(np.zeros(n))
    want = eager_run(A, M, b, x0, 5, RTOL, 300, basis=basis)
    assert want[2] == 1 and want[0] >= 1, want[:3]
    for segment in (1, 2, 5):
        got = planned_run(A, M, b, x0, 5, RTOL, 300, segment, basis=basis)
        assert_same(got, want, f"converging, {kind} {basis} segment {segment}")
        _within_waste_bound(got[6], basis, got[5])
        print(f"{kind} {basis} segment {segment}: {got[0]} iterations, {got[6]}")
    _close(F, A)


def test_an_exact_ilu_in_the_one_launch_form_is_recorded_level_by_level():
    """The eager solve applies the factor in form 1 (one launch); the plan's graphs hold form 0, as mi_bilu4_solve_dev records it
    under capture: the same bits, and the handle stays on form 1."""
    A, M, F, n = _system("fe:3", "ilu0")
    assert F.set_form(1) == 1
    b, x0 = _dev(_rhs(n)), _dev(np.zeros(n))
    want = eager_run(A, M, b, x0, 5, 1e-30, 12)
    got = planned_run(A, M, b, x0, 5, 1e-30, 12, 2)
    assert_same(got, want, "form 1 eager, form 0 in the graphs")
    assert F.info()["form"] == 1
    _close(F, A)


# ---------------------------------------------------------------- small cases

@pytest.mark.parametrize("name,restart,maxiter,segments", [("chain", 1, 7, (1, 3)), ("random:62", 64, 64, (7, 64))])
def test_restart_one_and_restart_sixty_four(name, restart, maxiter, segments):
    A, M, F, n = _system(name, "none")
    assert n >= restart + 1
    b, x0 = _dev(_rhs(n)), _dev(np.zeros(n))
    want = eager_run(A, None, b, x0, restart, 1e-300, maxiter)
    assert want[0] == maxiter and want[4][0] == min(restart, maxiter), want[:3]
    for segment in segments:
        assert_same(planned_run(A, None, b, x0, restart, 1e-300, maxiter, segment), want, f"{name} restart {restart} segment {segment}")
    A.close()


def test_one_block_with_restart_thirty():
    from navierstokes_amd import mpk
    one = C._from_rows([{0}], 91)
    A = mpk.bcsr4x4_matrix(*one)
    b, x0 = _dev(np.array([1.0, -2.0, 0.5, 3.0])), _dev(np.zeros(4))
    want = eager_run(A, None, b, x0, 30, 1e-13, 300)
    assert want[0] <= 4 and want[2] in (1, 3), want[:3]
    for segment in (1, 4, 30):
        got = planned_run(A, None, b, x0, 30, 1e-13, 300, segment)
        assert_same(got, want, f"one block, segment {segment}")
        _within_waste_bound(got[6], "f64")
    A.close()


@pytest.mark.parametrize("kind", ["none", "ilu0"])
def test_solves_that_end_at_their_start(kind):
    name = "random:31"
    A, M, F, n = _system(name, kind)
    Ad, _, b = G.problem(name, None)
    zero = np.zeros(n)
    xs = np.where(np.arange(n) % 3 == 0, 0.0, np.cos(0.7 * np.arange(n)))  # a solution with entries of zero ...
    bs = Ad @ xs
    xs0 = np.where(np.arange(n) % 6 == 0, -0.0, xs)  # ... half of them given as -0.0
    assert np.signbit(xs0).sum() > np.signbit(xs).sum()
    bad = b.copy()
    bad[n // 2] = np.nan
    start = np.arange(n) * 0.5
    cases = {"b = 0": (zero, zero, RTOL, 300, (0, 0)), "x0 the solution": (bs, xs0, RTOL, 300, (0, 0)),
             "NaN in b": (bad, start, RTOL, 300, (0, 4)), "maxiter 0": (b, start, RTOL, 0, (0, 2))}
    for what, (bb, xx, rtol, maxiter, expect) in cases.items():
        want = eager_run(A, M, _dev(bb), _dev(xx), 5, rtol, maxiter)
        assert (want[0], want[2]) == expect, (what, want[:3])
        for segment in (1, 5):
            got = planned_run(A, M, _dev(bb), _dev(xx), 5, rtol, maxiter, segment)
            assert_same(got, want, f"{what}, {kind} segment {segment}")
            assert_bit_equal(got[3], xx, f"{what}: x untouched")
            assert got[6]["wasted_steps_last"] == (0 if maxiter == 0 else segment), (what, got[6])  # the segment behind the start
    _close(F, A)


@pytest.mark.parametrize("kind", ["none", "ilu0"])
@pytest.mark.parametrize("maxiter", [0, 1, 5, 6])
def test_maxiter_at_and_around_a_restart(maxiter, kind):
    A, M, F, n = _system("fe:3", kind)
    b, x0 = _dev(_rhs(n)), _dev(0.01 * np.cos(0.3 * np.arange(n)))
    want = eager_run(A, M, b, x0, 5, 1e-30, maxiter)
    assert (want[0], want[2]) == (maxiter, 2)
    for segment in (1, 2, 5):
        got = planned_run(A, M, b, x0, 5, 1e-30, maxiter, segment)
        assert_same(got, want, f"maxiter {maxiter} {kind} segment {segment}")
        _within_waste_bound(got[6], "f64")
    _close(F, A)


# ---------------------------------------------------------------- reuse, streams, refusals

def test_reuse_streams_capture_and_a_stale_plan():
    import torch
    from navierstokes_amd import mpk
    name, restart, segment = "random:31", 5, 2
    A, M, F, n = _system(name, "ilu0")
    b1, b2, x0 = _dev(_rhs(n)), _dev(np.cos(0.21 * np.arange(n)) - 0.5), _dev(np.zeros(n))
    fresh1 = eager_run(A, M, b1, x0, restart, RTOL, 300)
    fresh2 = eager_run(A, M, b2, x0, restart, RTOL, 300)
    assert fresh1[2] == 1 and fresh2[2] == 1 and fresh1[0] > 1
    S = mpk.gmres_solver(A, M, restart)
    b, x = b1.clone(), x0.clone()
    P = S.plan(b, x, rtol=RTOL, maxiter=300, segment=segment)
    assert P.info()["graphs"] == 3 + math.ceil(restart / segment)

    def solved(fresh, what):
        its, hist, reason = P.solve()
        torch.cuda.current_stream().synchronize()
        info = P.info()
        assert (its, reason) == (fresh[0], fresh[2]), (what, its, reason)
        assert_bit_equal(hist, fresh[1], f"{what}: history")
        assert_bit_equal(x.cpu().numpy(), fresh[3], f"{what}: x")
        k, hraw, y, beta = S.fetch_cycle()
        assert k == fresh[4][0]
        assert_bit_equal(y, fresh[4][2], f"{what}: y of the last cycle")
        assert 0 <= info["wasted_steps_last"] <= 2 * segment - 1, info
        cycles = -(-its // restart)
        assert info["readbacks_last"] <= -(-its // segment) + 2 * cycles + 1, info
        assert info["replays_last"] <= info["readbacks_last"] + 2 * cycles + 1, info

    solved(fresh1, "the plan's first solve")
    b.copy_(b2), x.copy_(x0)  # refilled in place: the plan names the same memory
    solved(fresh2, "the plan's second solve")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b.copy_(b1), x.copy_(x0)
        solved(fresh1, "on a non-default stream")
    side.synchronize()
    # a capturing stream: refused, nothing enqueued, the stream stays usable
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        x.fill_(0.0)  # (so that the graph is not empty)
        with pytest.raises(mpk.MiError) as e:
            P.solve()
        with pytest.raises(mpk.MiError) as e2:
            S.state()
    assert e.value.status == 6 and "captur" in str(e.value)
    assert e2.value.status == 6 and "captur" in str(e2.value)
    with torch.cuda.stream(side):
        x.copy_(x0)  # (the captured fill never ran)
        solved(fresh1, "after the refused capture")
    side.synchronize()
    # any mi_gmres_set_* makes the plan stale; the eager solve does not care
    mpk.check(mpk.lib().mi_gmres_set_precond(S.handle, F.handle, mpk.GMRES_PC_EXACT, 0, 0))
    with pytest.raises(mpk.MiError) as e:
        P.solve()
    assert e.value.status == 6 and "plan" in str(e.value)
    x.copy_(x0)
    P2 = S.plan(b, x, rtol=RTOL, maxiter=300, segment=segment)
    its, hist, reason = P2.solve()
    torch.cuda.synchronize()
    assert (its, reason) == (fresh1[0], fresh1[2])
    assert_bit_equal(x.cpu().numpy(), fresh1[3], "a new plan after the setting: x")
    _close(P2, P, S, F, A)


# ---------------------------------------------------------------- the raw cycle in the caller's own graphs

@pytest.mark.parametrize("basis", ["f64", "f32"])
def test_raw_cycles_replayed_from_two_graphs(basis):
    import torch
    from navierstokes_amd import mpk
    name, restart, maxiter = "random:31", 5, 300
    A, M, F, n = _system(name, "sweeps")
    b, x0 = _dev(_rhs(n)), _dev(np.zeros(n))
    want = eager_run(A, M, b, x0, restart, RTOL, maxiter, basis=basis)
    assert want[2] == 1
    S = mpk.gmres_solver(A, M, restart, basis=basis)
    x = x0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    # not prepared: refused with status 6, nothing enqueued, the capture stays valid and its other node replays
    probe = torch.zeros(4, dtype=torch.float64, device="cuda")
    g_bad = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_bad, stream=side):
        probe.add_(1.0)
        with pytest.raises(mpk.MiError) as e:
            S.cycle(b, x, True, RTOL, maxiter)
    assert e.value.status == 6 and "not prepared" in str(e.value)
    g_bad.replay()
    torch.cuda.synchronize()
    assert probe.cpu().tolist() == [1.0] * 4 and not x.cpu().numpy().any()
    with torch.cuda.stream(side):
        S.prepare_stream()
        S.prepare_stream()  # idempotent
    side.synchronize()
    g_first, g_next = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_first, stream=side):
        S.cycle(b, x, True, RTOL, maxiter)
    with torch.cuda.graph(g_next, stream=side):
        S.cycle(b, x, False, RTOL, maxiter)
    # the caller's loop: mi_gmres_solve_dev's rule between cycles
    hist, claimed, refused, cycles = [], False, 0, 0
    g_first.replay()
    while True:
        cycles += 1
        st = S.state()
        if cycles == 1:
            hist.append(None)  # (history[0] is not part of the record's cycle entries)
        hist += st["history"]
        if claimed and not (st["reason"] == 1 and st["done"] and st["k"] == 0):
            refused += 1
        claimed = basis == "f32" and st["done"] and st["reason"] == 1 and st["k"] > 0
        if not claimed and (st["done"] or st["its"] >= maxiter):
            break
        assert cycles < 100
        g_next.replay()
    torch.cuda.synchronize()
    assert (st["its"], st["reason"], refused) == (want[0], want[2], want[5]), (st, want[:3], refused)
    assert_bit_equal(hist[1:], want[1][1:], "raw cycles: history")
    assert_bit_equal(x.cpu().numpy(), want[3], "raw cycles: x")
    k, hraw, y, beta = S.fetch_cycle()
    assert k == want[4][0]
    assert_bit_equal(hraw, want[4][1], "raw cycles: raw columns of the last cycle")
    assert_bit_equal(y, want[4][2], "raw cycles: y of the last cycle")
    assert_bit_equal([beta, st["beta"]], [want[4][3]] * 2, "raw cycles: beta of the last cycle")
    # the graphs are reusable: the whole solve again from x0
    x.copy_(x0)
    g_first.replay()
    for _ in range(cycles - 1):
        g_next.replay()
    torch.cuda.synchronize()
    assert_bit_equal(x.cpu().numpy(), want[3], "raw cycles, replayed without looking: x")
    _close(S, F, A)


# ---------------------------------------------------------------- a Newton step as one graph

def test_value_refresh_refactor_and_cycle_as_one_graph():
    import torch
    from navierstokes_amd import mpk
    L = mpk.lib()
    name, restart, maxiter = "fe:6", 5, 300
    mat = C.matrix(name)
    n = 4 * mat[0]
    A = mpk.bcsr4x4_matrix(*mat)
    F = mpk.bilu4(*mat, fill=0).prepare_dev()
    S = mpk.gmres_solver(A, F, restart)
    values = [_dev(np.asarray(mat[3]).reshape(-1)), _dev(C.new_values(name, 1))]
    coef = torch.empty_like(values[0])  # what the graph reads
    b, x0 = _dev(_rhs(n)), _dev(0.01 * np.cos(0.3 * np.arange(n)))
    x = x0.clone()
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def step():
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        mpk.check(L.mi_bcsr4_update_values_dev(A.handle, p(coef), s))
        mpk.check(L.mi_bilu4dev_refactor(F.handle, p(coef), 0, s))
        S.cycle(b, x, True, RTOL, maxiter)

    def record():
        st = S.state()
        return (st["its"], st["k"], st["done"], st["reason"]), [st["last"], st["beta"]] + st["history"]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    eager = []
    with torch.cuda.stream(side):
        S.prepare_stream()
        for v in values:  # the three calls made eagerly, once per set of values
            coef.copy_(v), x.copy_(x0)
            step()
            eager.append(record() + (x.cpu().numpy(),))
        F.factor_status()
    side.synchronize()
    assert eager[0][0][1] >= 1 and not np.array_equal(eager[0][2], eager[1][2])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step()
    for which in (1, 0, 1):
        coef.copy_(values[which]), x.copy_(x0)
        g.replay()
        ints, floats = record()
        torch.cuda.synchronize()
        assert ints == eager[which][0], (which, ints, eager[which][0])
        assert_bit_equal(floats, eager[which][1], f"values {which}: the record")
        assert_bit_equal(x.cpu().numpy(), eager[which][2], f"values {which}: x")
    F.factor_status()
    _close(S, F, A)
