"""The float Krylov basis on the GPU (MI_BASIS_F32: mi_gmres_create_ex, mi_round_f32_dev, mi_mdot_f32_dev, mi_maxpy_f32_dev,
mi_cgs_f32_dev; include/mi355_spmv.h).  Every comparison is bit for bit.

  primitives   mdot / maxpy (y and norm, negate 0 and 1) / cgs (passes 1 and 2) on a float32 basis against the double entry points
               on the widened basis: n in {1, 2, 3, 511, 512, 513, 1025, 524 289} x m in {1, 7, 8, 9, 16, 17, 64} (the tile
               edges, one and two segments, the first n whose segment exceeds 512), y 16-byte aligned and offset by one double,
               a non-default stream, n = 2 000 001 with m = 3 (the non-temporal path); a float vector offset by one float is
               MI_ERR_ARG
  round        mi_round_f32_dev against numpy's astype(float32) at the edge values of tests/gmres_f32_model.py scattered through
               vectors of n in {1, 2, 3, 5, 513}, with and without a divisor, out64 null, separate and aliasing x
  composed     the solver against the loop of tests/test_gpu_gmres_dev.py with the basis rounded on the host and the projections
               through the DOUBLE public pieces on widened rows: history, count, reason, x, fetch_cycle and refused_last, on fe:3,
               chain and random:31, each with none, ilu0, sweeps and sweeps_f32, restart 5, maxiter 12
  confirmed    the refusal case of tests/gmres_f32_model.py: refused_last >= 1 (asserted: the path cannot be skipped silently),
               bit-equal to the composed loop, and whenever the reason is 1 the residual recomputed from public pieces is <= rtol
  check_every  the same bits for {1, 2, 3, 7, restart, restart + 9}, on the refusal case and on a solve clipped by maxiter
  limits       restart 1; restart 64 on random:62; n = 4; b = 0; x0 the solution; NaN in b; maxiter 0 and 1; the residual sizes
               n in {1, 2, 511, 513, 1025} with aligned and offset vectors
  unmoved      mi_gmres_create_ex(.., MI_BASIS_F64) gives the bits and the device_bytes of mi_gmres_create; basis_bytes of an F32
               handle is 4 (m + 1) ldv32 + 8 ldv; two solves on one handle equal two fresh handles; a capturing stream is still
               refused with MI_ERR_STATE and stays usable"""
import ctypes
import functools

import numpy as np
import pytest

import bilu4_cases as C
import gmres_dev_model as D
import gmres_f32_model as F
import gmres_model as G
import test_gpu_gmres_dev as T
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

RTOL = 1e-8
NS = (1, 2, 3, 511, 512, 513, 1025, 524_289)
MS = (1, 7, 8, 9, 16, 17, 64)
_dev, _rhs, _precond = T._dev, T._rhs, T._precond


# ---------------------------------------------------------------- primitives against the double entry points

def _basis(n, m, seed):
    """(rows32, rows64, y values): m float32 rows of n, each 8-byte aligned (the leading dimension is even), their exact widening,
    and a float64 vector with entries of mixed magnitude."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    ld = n + (n & 1)
    V32 = torch.randn((m, ld), dtype=torch.float32, device="cuda", generator=g)
    V64 = V32.double()
    y = torch.randn(n, dtype=torch.float64, device="cuda", generator=g) * torch.exp(3.0 * torch.randn(n, dtype=torch.float64, device="cuda", generator=g))
    rows32, rows64 = [V32[j, :n] for j in range(m)], [V64[j, :n] for j in range(m)]
    assert all(r.data_ptr() % 8 == 0 for r in rows32)
    return rows32, rows64, y


def _placed(y, offset):
    """A copy of y that is 16-byte aligned (offset 0) or offset by one double."""
    import torch
    buf = torch.zeros(y.numel() + 2, dtype=torch.float64, device="cuda")
    out = buf[offset: offset + y.numel()]
    assert out.data_ptr() % 16 == 8 * offset
    out.copy_(y)
    return out


def _primitives(n, ms, seed):
    from navierstokes_amd import mpk
    rows32, rows64, y0 = _basis(n, max(ms), seed)
    for m in ms:
        r32, r64 = rows32[:m], rows64[:m]
        for offset in (0, 1):
            what = f"n {n} m {m} y offset {offset}"
            y = _placed(y0, offset)
            got, want = mpk.mdot(r32, y), mpk.mdot(r64, y)
            assert_bit_equal(got.cpu().numpy(), want.cpu().numpy(), f"mdot {what}")
            coef = want.clone()
            for negate in (False, True):
                ya, yb = _placed(y0, offset), _placed(y0, offset)
                _, na = mpk.maxpy(coef, r32, ya, negate=negate, norm=True)
                _, nb = mpk.maxpy(coef, r64, yb, negate=negate, norm=True)
                assert_bit_equal(ya.cpu().numpy(), yb.cpu().numpy(), f"maxpy {what} negate {negate}: y")
                assert_bit_equal(na.cpu().numpy(), nb.cpu().numpy(), f"maxpy {what} negate {negate}: norm")
                yc = _placed(y0, offset)
                mpk.maxpy(coef, r32, yc, negate=negate)  # without the norm: another instantiation of the last chunk
                assert_bit_equal(yc.cpu().numpy(), yb.cpu().numpy(), f"maxpy {what} negate {negate}, no norm: y")
            for passes in (1, 2):
                ya, yb = _placed(y0, offset), _placed(y0, offset)
                ha, na = mpk.cgs(r32, ya, passes=passes)
                hb, nb = mpk.cgs(r64, yb, passes=passes)
                assert_bit_equal(ha.cpu().numpy(), hb.cpu().numpy(), f"cgs {what} passes {passes}: h")
                assert_bit_equal(na.cpu().numpy(), nb.cpu().numpy(), f"cgs {what} passes {passes}: norm")
                assert_bit_equal(ya.cpu().numpy(), yb.cpu().numpy(), f"cgs {what} passes {passes}: y")


@pytest.mark.parametrize("n", NS)
def test_float_basis_primitives_equal_the_double_ones_on_the_widened_basis(n):
    _primitives(n, MS, 100 + n % 97)


def test_float_basis_primitives_on_a_non_default_stream():
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _primitives(1025, (9, 17), 7)
    side.synchronize()


def test_float_basis_primitives_non_temporal_path():
    _primitives(2_000_001, (3,), 8)


def test_a_float_vector_offset_by_one_float_is_refused():
    import torch
    from navierstokes_amd import mpk
    n = 64
    buf = torch.ones(2 * n + 2, dtype=torch.float32, device="cuda")
    good, odd = buf[:n], buf[n + 1: 2 * n + 1]
    assert good.data_ptr() % 8 == 0 and odd.data_ptr() % 8 == 4
    y = torch.ones(n, dtype=torch.float64, device="cuda")
    for call in (lambda: mpk.mdot([good, odd], y), lambda: mpk.maxpy(np.ones(2), [good, odd], y), lambda: mpk.maxpy(np.ones(2), [odd, good], y, norm=True),
                 lambda: mpk.cgs([good, odd], y), lambda: mpk.cgs([odd], y, passes=1)):
        with pytest.raises(mpk.MiError) as e:
            call()
        assert e.value.status == 1 and "8-byte aligned" in str(e.value), e.value
    torch.cuda.synchronize()
    assert bool((y == 1.0).all()), "a refused call wrote y"
    assert float(mpk.mdot([good], y).item()) == float(n)  # the stream is as usable as before


# ---------------------------------------------------------------- mi_round_f32_dev against numpy

def _same32(got, want, what):
    """float32 arrays: NaN where NaN is wanted, the same bits everywhere else."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN in other places"
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)) & ~nan)[0]
    assert bad.size == 0, f"{what}: {bad.size} entries differ, first at {bad[:5]}: {got[bad[:5]]} vs {want[bad[:5]]}"


def _nn(a):
    """NaN replaced by a marker (Inf and -0 stay): for assert_bit_equal where only the place of a NaN is held."""
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), 7.0, a)


def _edge_vector(n, shift):
    """n values: a smooth background with the edge values scattered through it (all of them from n = 513 on, a window of them below)."""
    x = np.sin(0.7 * np.arange(n) + shift) * 10.0 ** ((np.arange(n) * 7 + shift) % 23 - 11)
    edges = F.EDGE_VALUES
    if n >= 8 * len(edges):
        x[(np.arange(len(edges)) * 13 + shift) % n] = edges  # (13 and 513 are coprime: distinct places, odd and even, the last one among them)
        x[n - 1] = edges[(shift + 3) % len(edges)]
    else:
        for i in range(n):
            x[i] = edges[(shift * n + i) % len(edges)]
    return x


@pytest.mark.parametrize("n", [1, 2, 3, 5, 513])
def test_round_f32_against_numpy(n):
    import torch
    from navierstokes_amd import mpk
    L = mpk.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    shifts = range(len(F.EDGE_VALUES)) if n < 8 else range(3)  # short vectors: every window of the edge values
    for shift in shifts:
        for div in (None, 0.125, 3.0):
            x = _edge_vector(n, shift)
            if div == 0.125:
                x = x * div  # (exact but for what underflows: the quotient is the edge value again)
            with np.errstate(all="ignore"):
                want32 = (x if div is None else x / div).astype(np.float32)
            want64 = want32.astype(np.float64)
            what = f"n {n} shift {shift} div {div}"
            dx = _dev(x)
            dd = None if div is None else _dev(np.array([div]))
            # the wrapper: out64 separate, x left alone
            x32, x64 = mpk.round_f32(dx, dd)
            _same32(x32.cpu().numpy(), want32, f"{what}: out32")
            _same32(x64.cpu().numpy().astype(np.float32), want32, f"{what}: out64 as float")
            assert_bit_equal(_nn(x64.cpu().numpy()), _nn(want64), f"{what}: out64")
            assert_bit_equal(_nn(dx.cpu().numpy()), _nn(x), f"{what}: x was written")
            # out64 null, and vectors that are only 8-byte (double) and 4-byte (float) aligned: the scalar path
            for off in (0, 1):
                xb = torch.zeros(n + 2, dtype=torch.float64, device="cuda")
                ob = torch.full((n + 3,), 9.0, dtype=torch.float32, device="cuda")
                xo, oo = xb[off: off + n], ob[off: off + n]
                xo.copy_(dx)
                mpk.check(L.mi_round_f32_dev(n, p(xo), p(dd) if dd is not None else None, p(oo), None, mpk._stream_ptr()))
                _same32(oo.cpu().numpy(), want32, f"{what} offset {off}, out64 null: out32")
                assert bool((ob[off + n:] == 9.0).all()) and bool((ob[:off] == 9.0).all()), f"{what}: written past the vector"
                # out64 aliasing x: in place
                mpk.check(L.mi_round_f32_dev(n, p(xo), p(dd) if dd is not None else None, p(oo), p(xo), mpk._stream_ptr()))
                _same32(oo.cpu().numpy(), want32, f"{what} offset {off}, in place: out32")
                assert_bit_equal(_nn(xo.cpu().numpy()), _nn(want64), f"{what} offset {off}, in place: out64")
                assert not xb[:off].any() and not xb[off + n:].any(), f"{what}: written past the vector"


# ---------------------------------------------------------------- the solver against a composed loop

def composed_f32(A, M, b, x0, restart, rtol, maxiter):
    """The float-basis GMRES of include/mi355_spmv.h from the library's public pieces: the loop of tests/test_gpu_gmres_dev.py with
    the basis rounded on the HOST (numpy's division and astype(float32)) and every projection through the DOUBLE entry points
    (cgs, maxpy) on the widened rows; the small problem in tests/gmres_dev_model.py; a step's reason 1 is a claim that the next
    start confirms or refuses.  Returns (iterations, history, reason, x, (k, hraw, y, beta), refused)."""
    import torch
    from navierstokes_amd import mpk
    mult = mpk.SpMV_BCSR if isinstance(A, mpk.bcsr4x4_matrix) else mpk.SpMV_CSR
    n = int(b.numel())
    x = x0.clone()
    W = torch.empty((restart + 1, n), dtype=torch.float64, device=b.device)  # widen(V32): what the next product and the projections read
    w, z, r = torch.empty_like(b), torch.empty_like(b), torch.empty_like(b)
    bnorm = D.bnorm_of(float(mpk.norm2(b).item()))
    its, hist, refused, claimed = 0, [], 0, False

    def stored(v, d):
        with np.errstate(all="ignore"):
            return _dev(F.widen(F.round32(v.cpu().numpy() / d)))

    while True:
        mult(w, x, A)
        r.copy_(b)
        mpk.axpy(-1.0, w, r)
        beta = float(mpk.norm2(r).item())
        rel, reason = D.cycle_start(beta, bnorm, its, rtol, maxiter)
        if not hist:
            hist.append(rel)
        if claimed and reason != 1:
            refused += 1
        claimed = False
        if reason is not None:
            return its, hist, reason, x.cpu().numpy(), (0, np.zeros((restart, restart + 2)), np.zeros(0), beta), refused
        W[0].copy_(stored(r, beta))
        cyc = D.Cycle(restart, beta, bnorm, rtol)
        hraw = np.zeros((restart, restart + 2))
        while cyc.k < restart and its < maxiter and not cyc.reason:
            k = cyc.k
            if M is not None:
                M.solve(z, W[k])
                mult(w, z, A)
            else:
                mult(w, W[k], A)
            h, nrm = mpk.cgs([W[j] for j in range(k + 1)], w, passes=2)
            col = torch.cat([h, nrm]).cpu().numpy()
            entry = cyc.step(col)
            if entry is None:
                break
            hraw[k, : k + 2] = col
            its += 1
            hist.append(entry)
            W[k + 1].copy_(stored(w, col[-1]))
        k = cyc.k
        y = np.array(cyc.solve())
        if k:
            if M is not None:
                w.zero_()
                mpk.maxpy(y, [W[j] for j in range(k)], w)
                M.solve(z, w)
                mpk.axpy(1.0, z, x)
            else:
                mpk.maxpy(y, [W[j] for j in range(k)], x)
        if cyc.reason == 1:
            claimed = True  # the update has run: the next cycle's start confirms or refuses
            continue
        if cyc.reason:
            return its, hist, cyc.reason, x.cpu().numpy(), (k, hraw, y, beta), refused
        if its >= maxiter:
            return its, hist, 2, x.cpu().numpy(), (k, hraw, y, beta), refused


def solver_run(A, M, b, x0, restart, rtol, maxiter, check_every=5, basis="f32"):
    """(iterations, history, reason, x, fetch_cycle(), refused_last, info(), basis_info()) of a fresh gmres_solver."""
    import torch
    from navierstokes_amd import mpk
    S = mpk.gmres_solver(A, M, restart, basis=basis)
    x = x0.clone()
    its, hist, reason = S.solve(b, x, rtol=rtol, maxiter=maxiter, check_every=check_every)
    torch.cuda.synchronize()
    binfo = S.basis_info()
    out = its, hist, reason, x.cpu().numpy(), S.fetch_cycle(), binfo["refused_last"], S.info(), binfo
    S.close()
    return out


def assert_same_solve(got, want, what):
    T.assert_same_solve(got, want, what)
    assert got[5] == want[5], (what, "refused", got[5], want[5])


def _true_residual_from_public_pieces(A, b, x):
    """||b - A x|| / ||b|| with the library's product, axpy and norm: what the solver's start check computes."""
    from navierstokes_amd import mpk
    mult = mpk.SpMV_BCSR if isinstance(A, mpk.bcsr4x4_matrix) else mpk.SpMV_CSR
    w, r = _dev(np.zeros(len(x))), b.clone()
    mult(w, _dev(x), A)
    mpk.axpy(-1.0, w, r)
    return float(mpk.norm2(r).item()) / D.bnorm_of(float(mpk.norm2(b).item()))


@pytest.mark.parametrize("kind", T.PRECONDS)
@pytest.mark.parametrize("name", ["fe:3", "chain", "random:31"])
def test_bit_equal_to_the_loop_composed_from_public_pieces(name, kind):
    from navierstokes_amd import mpk
    mat = C.matrix(name)
    A = mpk.bcsr4x4_matrix(*mat)
    M, Fh = _precond(kind, mat)
    n = 4 * mat[0]
    b, x0 = _dev(_rhs(n)), _dev(np.zeros(n))
    want = composed_f32(A, M, b, x0, 5, 1e-30, 12)
    got = solver_run(A, M, b, x0, 5, 1e-30, 12)
    if name != "chain" or kind == "none":  # (on the chain ILU(0) is exact: the solve ends early)
        assert want[0] == 12 and want[2] == 2 and want[4][0] == 2  # three cycles, the last of two steps
    print(f"{name} {kind}: {got[0]} iterations, reason {got[2]}, refused {got[5]}, last {got[1][-1]:.3e}")
    assert_same_solve(got, want, f"{name} {kind}")
    assert got[6]["restart"] == 5 and got[7]["basis"] == "f32"
    if Fh is not None:
        Fh.close()
    A.close()


# ---------------------------------------------------------------- confirmation

@functools.lru_cache(maxsize=None)
def _refusal_setup():
    name, fill, restart, rtol = F.REFUSAL_CASE
    assert fill is None
    mat = C.matrix(name)
    n = 4 * mat[0]
    return mat, n, restart, rtol


def test_refused_claim_on_the_refusal_case():
    from navierstokes_amd import mpk
    mat, n, restart, rtol = _refusal_setup()
    A = mpk.bcsr4x4_matrix(*mat)
    b, x0 = _dev(_rhs(n)), _dev(np.zeros(n))
    want = composed_f32(A, None, b, x0, restart, rtol, 300)
    got = solver_run(A, None, b, x0, restart, rtol, 300)
    print(f"refusal case: {got[0]} iterations, reason {got[2]}, refused {got[5]}, history tail {got[1][-3:]}, beta {got[4][3]:.3e}")
    assert got[5] >= 1, "the recurrence's first claim was not refused: the confirming path did not run"
    assert_same_solve(got, want, "refusal case")
    assert got[2] == 1 and got[4][0] == 0  # confirmed: the last cycle is the confirming start, k = 0
    true = _true_residual_from_public_pieces(A, b, got[3])
    assert true <= rtol, true
    assert_bit_equal([got[4][3] / D.bnorm_of(float(mpk.norm2(b).item()))], [true], "beta of the confirming start is the true residual norm")
    # the double basis on the same system: no confirmation, nothing refused, its own bits
    dbl = solver_run(A, None, b, x0, restart, rtol, 300, basis="f64")
    assert dbl[2] == 1 and dbl[5] == 0 and dbl[4][0] > 0 and dbl[0] <= got[0] <= dbl[0] + 11
    A.close()


@pytest.mark.parametrize("kind", ["none", "ilu0", "sweeps_f32"])
@pytest.mark.parametrize("name,restart", [("random:31", 5), ("fe:3", 30), ("chain", 30)])
def test_every_reason_one_is_a_true_residual(name, restart, kind):
    from navierstokes_amd import mpk
    mat = C.matrix(name)
    A = mpk.bcsr4x4_matrix(*mat)
    M, Fh = _precond(kind, mat)
    n = 4 * mat[0]
    b, x0 = _dev(_rhs(n)), _dev(np.zeros(n))
    want = composed_f32(A, M, b, x0, restart, RTOL, 300)
    got = solver_run(A, M, b, x0, restart, RTOL, 300)
    assert_same_solve(got, want, f"{name} {kind} restart {restart}")
    true = _true_residual_from_public_pieces(A, b, got[3])
    print(f"{name} {kind} restart {restart}: {got[0]} iterations, reason {got[2]}, refused {got[5]}, true {true:.3e}")
    assert got[2] == 1 and true <= RTOL and got[4][0] == 0 and len(got[1]) == got[0] + 1
    if Fh is not None:
        Fh.close()
    A.close()


# ---------------------------------------------------------------- independence of check_every

@pytest.mark.parametrize("case", ["refusal", "maxiter"])
def test_result_does_not_depend_on_check_every(case):
    from navierstokes_amd import mpk
    mat, n, restart, rtol = _refusal_setup()
    maxiter = 300
    if case == "maxiter":
        mat, restart, rtol, maxiter = C.matrix("random:31"), 5, 1e-30, 12
        n = 4 * mat[0]
    A = mpk.bcsr4x4_matrix(*mat)
    b, x0 = _dev(_rhs(n)), _dev(np.zeros(n))
    runs = {ce: solver_run(A, None, b, x0, restart, rtol, maxiter, check_every=ce) for ce in (1, 2, 3, 7, restart, restart + 9)}
    first = runs[1]
    if case == "refusal":
        assert first[2] == 1 and first[5] >= 1
    else:
        assert (first[0], first[2], first[5]) == (12, 2, 0)
    for ce, run in runs.items():
        assert (run[0], run[2], run[5], run[4][0]) == (first[0], first[2], first[5], first[4][0]), (ce, run[0], run[2], run[5])
        assert_bit_equal(run[1], first[1], f"check_every {ce}: history")
        assert_bit_equal(run[3], first[3], f"check_every {ce}: x")
        assert_bit_equal(run[4][1], first[4][1], f"check_every {ce}: raw columns")
        assert_bit_equal(run[4][2], first[4][2], f"check_every {ce}: y")
        assert_bit_equal([run[4][3]], [first[4][3]], f"check_every {ce}: beta")
        print(f"check_every {ce}: {run[0]} iterations, {run[6]}")
    A.close()


# ---------------------------------------------------------------- limits

@pytest.mark.parametrize("name,restart,maxiter", [("chain", 1, 7), ("random:62", 64, 64)])
def test_restart_one_and_restart_sixty_four(name, restart, maxiter):
    from navierstokes_amd import mpk
    mat = C.matrix(name)
    A = mpk.bcsr4x4_matrix(*mat)
    n = 4 * mat[0]
    assert n >= restart + 1
    b, x0 = _dev(_rhs(n)), _dev(np.zeros(n))
    want = composed_f32(A, None, b, x0, restart, 1e-300, maxiter)
    got = solver_run(A, None, b, x0, restart, 1e-300, maxiter, check_every=7)
    assert want[0] == maxiter and want[4][0] == min(restart, maxiter), want[:3]  # (restart 64: step k = 63 ran)
    assert_same_solve(got, want, f"{name} restart {restart}")
    A.close()


def test_one_block():
    """n = 4, restart 30: bit-equal to the composed loop, at most a handful of iterations, a finite x that solves the system."""
    from navierstokes_amd import mpk
    one = T._one_block()
    A = mpk.bcsr4x4_matrix(*one)
    Ad = np.asarray(one[3]).reshape(4, 4)
    b = np.array([1.0, -2.0, 0.5, 3.0])
    want = composed_f32(A, None, _dev(b), _dev(np.zeros(4)), 30, 1e-13, 300)
    got = solver_run(A, None, _dev(b), _dev(np.zeros(4)), 30, 1e-13, 300)
    print(f"one block: {got[0]} iterations, reason {got[2]}, refused {got[5]}, history {got[1]}")
    assert_same_solve(got, want, "one block")
    assert np.isfinite(got[3]).all()
    if got[2] == 1:
        assert G.true_residual(Ad, got[3], b) <= 2e-13
    A.close()


@pytest.mark.parametrize("kind", ["none", "ilu0"])
def test_exits_without_iterating(kind):
    from navierstokes_amd import mpk
    name = "random:31"
    mat = C.matrix(name)
    Ad, _, b = G.problem(name, None)
    n = len(b)
    A = mpk.bcsr4x4_matrix(*mat)
    M, Fh = _precond(kind, mat)
    its, hist, reason, x, cyc, refused, info, _ = solver_run(A, M, _dev(np.zeros(n)), _dev(np.zeros(n)), 30, RTOL, 300)
    assert (its, hist, reason, refused) == (0, [0.0], 0, 0) and not x.any() and cyc[0] == 0
    x0 = np.linalg.solve(Ad, b)
    its, hist, reason, x, _, refused, _, _ = solver_run(A, M, _dev(b), _dev(x0), 30, RTOL, 300)
    assert (its, reason, refused) == (0, 0, 0) and len(hist) == 1 and hist[0] <= 1e-14
    assert_bit_equal(x, x0, "x0 was already the solution")
    bad = b.copy()
    bad[n // 2] = np.nan
    x0 = np.arange(n) * 0.5
    its, hist, reason, x, _, refused, _, _ = solver_run(A, M, _dev(bad), _dev(x0), 30, RTOL, 300)
    assert (its, reason, refused) == (0, 4, 0) and len(hist) == 1 and np.isnan(hist[0])
    assert_bit_equal(x, x0, "NaN in b: x unchanged")
    its, hist, reason, x, _, refused, _, _ = solver_run(A, M, _dev(b), _dev(x0), 30, RTOL, 0)
    assert (its, reason, refused) == (0, 2, 0) and len(hist) == 1
    assert_bit_equal(x, x0, "maxiter 0: x unchanged")
    want = composed_f32(A, M, _dev(b), _dev(x0), 30, RTOL, 1)
    got = solver_run(A, M, _dev(b), _dev(x0), 30, RTOL, 1)
    assert_same_solve(got, want, f"maxiter 1 {kind}")
    assert (got[0], got[2]) == (1, 2)
    if Fh is not None:
        Fh.close()
    A.close()


def _residual_case(n, offset):
    import torch
    from navierstokes_amd import mpk
    A = mpk.csrmatrix(n, *T._tridiagonal(n))
    bfull = torch.zeros(n + 2, dtype=torch.float64, device="cuda")
    xfull = torch.zeros(n + 2, dtype=torch.float64, device="cuda")
    b, x0 = bfull[offset: offset + n], xfull[offset: offset + n]
    assert b.data_ptr() % 16 == 8 * offset and x0.data_ptr() % 16 == 8 * offset
    b.copy_(_dev(_rhs(n)))
    x0.copy_(_dev(0.01 * np.cos(0.3 * np.arange(n))))
    want = composed_f32(A, None, b, x0, 2, 1e-30, 2)
    got = solver_run(A, None, b, x0, 2, 1e-30, 2)
    assert_same_solve(got, want, f"tridiagonal n {n} offset {offset}")
    assert want[0] == (1 if n == 1 else 2)
    A.close()


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("n", [1, 2, 511, 513, 1025])
def test_residual_sizes_with_offset_vectors(n, offset):
    _residual_case(n, offset)


# ---------------------------------------------------------------- nothing else moved

def test_create_ex_f64_is_create_and_the_basis_bytes():
    from navierstokes_amd import mpk
    L = mpk.lib()
    name, restart = "random:31", 5
    mat = C.matrix(name)
    n = 4 * mat[0]
    A = mpk.bcsr4x4_matrix(*mat)
    Fh = mpk.bilu4(*mat, fill=0)
    b, x0 = _dev(_rhs(n)), _dev(np.zeros(n))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    outs = []
    for create in (lambda h: L.mi_gmres_create(n, restart, ctypes.byref(h)), lambda h: L.mi_gmres_create_ex(n, restart, 0, ctypes.byref(h))):
        h = ctypes.c_void_p()
        mpk.check(create(h))
        mpk.check(L.mi_gmres_set_operator_bcsr4(h, A.handle))
        mpk.check(L.mi_gmres_set_precond(h, Fh.handle, 0, 0, 0))
        x, hist = x0.clone(), np.zeros(301)
        its, why, kind, refused = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(-1), ctypes.c_int(-1)
        by, bb = ctypes.c_longlong(), ctypes.c_longlong()
        mpk.check(L.mi_gmres_solve_dev(h, p(b), p(x), RTOL, 300, 3, ctypes.byref(its), ctypes.byref(why), hist.ctypes.data, mpk._stream_ptr()))
        mpk.check(L.mi_gmres_info(h, None, ctypes.byref(by), None, None, None))
        mpk.check(L.mi_gmres_basis_info(h, ctypes.byref(kind), ctypes.byref(bb), ctypes.byref(refused)))
        import torch
        torch.cuda.synchronize()
        outs.append((its.value, why.value, hist.copy(), x.cpu().numpy(), by.value, kind.value, bb.value, refused.value))
        mpk.check(L.mi_gmres_destroy(h))
    a, c = outs
    assert a[:2] == c[:2] and a[1] == 1 and a[4:] == c[4:]
    assert_bit_equal(a[2], c[2], "create_ex(F64): history")
    assert_bit_equal(a[3], c[3], "create_ex(F64): x")
    ldv = n + (n & 1)
    small = 8 + restart + restart * (restart + 2) + restart * restart + 4 * restart + 3
    assert a[4] == 8 * ((restart + 3) * ldv + small) and a[5:] == (0, 8 * (restart + 1) * ldv, 0)
    # the float basis: what the handle really owns
    for nn, m in ((n, restart), (n, 30), (1, 1), (5, 64), (1027, 30)):
        S = mpk.gmres_solver(mpk.csrmatrix(nn, *T._tridiagonal(nn)), None, m, basis="f32")
        ldv, ldv32 = nn + (nn & 1), (nn + 3) // 4 * 4
        small = 8 + m + m * (m + 2) + m * m + 4 * m + 3
        info = S.basis_info()
        assert info == dict(basis="f32", basis_bytes=4 * (m + 1) * ldv32 + 8 * ldv, refused_last=0), info
        assert S.info()["device_bytes"] == info["basis_bytes"] + 8 * (2 * ldv + small), S.info()
        S.close()
    Fh.close()
    A.close()


def test_reuse_streams_and_capture():
    import torch
    from navierstokes_amd import mpk
    mat, n, restart, rtol = _refusal_setup()
    A = mpk.bcsr4x4_matrix(*mat)
    b1, b2, x0 = _dev(_rhs(n)), _dev(np.cos(0.21 * np.arange(n)) - 0.5), _dev(np.zeros(n))
    fresh1 = solver_run(A, None, b1, x0, restart, rtol, 300)
    fresh2 = solver_run(A, None, b2, x0, restart, rtol, 300)
    assert fresh1[2] == 1 and fresh2[2] == 1 and fresh1[5] >= 1
    S = mpk.gmres_solver(A, None, restart, basis="f32")
    for b, fresh in ((b1, fresh1), (b2, fresh2), (b1, fresh1)):
        x = x0.clone()
        its, hist, reason = S.solve(b, x, rtol=rtol, maxiter=300, check_every=5)
        assert (its, reason, S.basis_info()["refused_last"]) == (fresh[0], fresh[2], fresh[5])
        assert_bit_equal(hist, fresh[1], "a reused handle: history")
        assert_bit_equal(x.cpu().numpy(), fresh[3], "a reused handle: x")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        x = x0.clone()
        its, hist, reason = S.solve(b1, x, rtol=rtol, maxiter=300, check_every=3)
    side.synchronize()
    assert (its, reason) == (fresh1[0], fresh1[2])
    assert_bit_equal(hist, fresh1[1], "non-default stream: history")
    assert_bit_equal(x.cpu().numpy(), fresh1[3], "non-default stream: x")
    # a capturing stream: refused, nothing enqueued, the stream stays usable
    x = x0.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        x.fill_(0.0)  # (so that the graph is not empty)
        with pytest.raises(mpk.MiError) as e:
            S.solve(b1, x, rtol=rtol, maxiter=300)
    assert e.value.status == 6 and "captur" in str(e.value)
    with torch.cuda.stream(side):
        its, hist, reason = S.solve(b1, x, rtol=rtol, maxiter=300)
    side.synchronize()
    assert (its, reason) == (fresh1[0], fresh1[2])
    assert_bit_equal(x.cpu().numpy(), fresh1[3], "after the refused capture: x")
    # host vectors, and GMRES_dev
    xh = np.zeros(n)
    its, hist, reason = S.solve(_rhs(n), xh, rtol=rtol, maxiter=300)
    assert (its, reason) == (fresh1[0], fresh1[2])
    assert_bit_equal(xh, fresh1[3], "host vectors: x")
    its2, hist2 = mpk.GMRES_dev(A, b1, x0.clone(), restart=restart, rtol=rtol, maxiter=300, basis="f32")
    assert its2 == fresh1[0]
    assert_bit_equal(hist2, fresh1[1], "GMRES_dev: history")
    S.close()
    A.close()


def test_primitives_can_be_captured():
    """mi_round_f32_dev and mi_cgs_f32_dev inside a graph: replayed, they give the bits of the direct calls."""
    import torch
    from navierstokes_amd import mpk
    n, m = 1025, 9
    rows32, _, y0 = _basis(n, m, 21)
    ya = y0.clone()
    ha, na = mpk.cgs(rows32, ya, passes=2)
    a32, a64 = mpk.round_f32(ya, na)
    yb = y0.clone()
    mpk.cgs(rows32, yb.clone(), passes=2)  # (the side stream's workspace exists before the capture)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mpk.cgs(rows32, yb.clone(), passes=2)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        hb, nb = mpk.cgs(rows32, yb, passes=2)
        b32, b64 = mpk.round_f32(yb, nb)
    yb.copy_(y0)
    g.replay()
    torch.cuda.synchronize()
    assert_bit_equal(hb.cpu().numpy(), ha.cpu().numpy(), "captured cgs: h")
    assert_bit_equal(yb.cpu().numpy(), ya.cpu().numpy(), "captured cgs: y")
    assert_bit_equal(b32.cpu().numpy(), a32.cpu().numpy(), "captured round: out32")
    assert_bit_equal(b64.cpu().numpy(), a64.cpu().numpy(), "captured round: out64")
