"""VecMDot / VecMAXPY, the classical Gram-Schmidt pass and the CGS Arnoldi basis (mi_mdot*, mi_maxpy*, mi_cgs_dev,
mi_krylov_basis_cgs_dev; blas1_multi.hpp) held bit for bit to models the oracle already had: every dot is O.tree_dot, the update
is the chain of O.axpy in basis order, the norm that rides on the update is O.tree_norm2 of the new vector, a Hessenberg entry
of two passes is one numpy add, and the basis is tests/test_cgs_model._replay_krylov_cgs.

Sizes are those of the reduction suite (every regime of red_geometry, both sides of the non-temporal switch), largest first so
that partials left by a larger call would show; basis counts sit on both sides of every compiled tile (4, 8, 16) and reach the
limit of 64; basis rows lie at odd 8-byte offsets of one buffer, y aligned and odd; host and device forms.

Comparison is bitwise (signed zeros included) except that a NaN matches any NaN (test_gpu_edges.assert_same)."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from navierstokes_amd import mpk, synth
from oracle import oracle as O
from test_cgs_model import _replay_krylov_cgs, cgs_model, loss
from test_gpu_edges import assert_same
from test_gpu_reductions import dev, odd_view, val
from test_oracle_vs_reference import ieee_inputs
from test_reduction_model import DATA, GPU_SIZES

pytestmark = pytest.mark.gpu

M_ALL = (1, 2, 7, 8, 9, 17, 64)
M_LARGE = (1, 9)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    mpk.lib()
    yield


def counts(n):
    return M_ALL if n <= 1_048_577 else M_LARGE


def make(kind, n, m, seed):
    """y and m basis rows of one data kind; (y, row 0) is the kind's own pair (cancelling, all products -0, ...)."""
    rng = np.random.default_rng(seed)
    y, v0 = DATA[kind](n, rng)
    basis = np.empty((m, n))
    basis[0] = v0
    for j in range(1, m):
        basis[j] = DATA[kind](n, rng)[1]
    return basis, y


def dev_rows(basis):
    """The rows in one device buffer, n + 1 apart from offset 1: every row (n odd) or every other row (n even) only 8-byte aligned."""
    m, n = basis.shape
    buf = torch.full((m * (n + 1) + 1,), float("nan"), dtype=torch.float64, device="cuda")
    rows = []
    for j in range(m):
        rows.append(buf[1 + j * (n + 1):1 + j * (n + 1) + n])
        rows[-1].copy_(dev(basis[j]))
    return rows


def coefs(m, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(m) * np.exp2(rng.integers(-8, 9, m))


def axpy_chain(c, basis, y, negate):
    for j in range(len(c)):
        y = O.axpy(-c[j] if negate else c[j], basis[j], y)
    return np.asarray(y, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------ mdot

@pytest.mark.parametrize("n", sorted(GPU_SIZES, reverse=True))
def test_mdot_bitwise(n):
    ms = counts(n)
    for kind in DATA:
        basis, y = make(kind, n, max(ms), n + 17)
        want = np.array([O.tree_dot(y, v) for v in basis], dtype=np.float64).reshape(len(basis))
        rows = dev_rows(basis)
        ys = (dev(y), odd_view(y))
        for j, r in enumerate(rows):  # the device's own dot: the same tree
            assert_same(np.float64(val(mpk.dot(ys[0], r))), want[j], f"mpk.dot n={n} {kind} column {j}")
        for m in ms:
            what = f"n={n} m={m} {kind}"
            assert_same(mpk.mdot(list(basis[:m]), y), want[:m], f"host dots {what}")
            for dy in ys:
                assert_same(mpk.mdot(rows[:m], dy), want[:m], f"device dots {what}")
            assert_same(mpk.mdot([dev(b) for b in basis[:m]], ys[0]), want[:m], f"device dots, aligned rows {what}")
        assert_same(ys[0], y, "y is read only")
        assert_same(ys[1], y, "y is read only")


def test_mdot_ieee_data_sets():
    """x and A x of every IEEE case (non-finite entries, signed zeros, subnormal products, order-dependent overflow)."""
    for pat, name, p, c, v, x, block, pins in ieee_inputs():
        ax = O.spmv(p, c, v, x)
        basis = np.stack([x, ax, x])
        for y in (x, ax):
            want = np.array([O.tree_dot(y, b) for b in basis], dtype=np.float64)
            assert_same(mpk.mdot(list(basis), y.copy()), want, f"{pat}/{name} host")
            assert_same(mpk.mdot(dev_rows(basis), dev(y)), want, f"{pat}/{name} device")
            assert_same(mpk.mdot([dev(b) for b in basis], odd_view(y)), want, f"{pat}/{name} device, odd y")


def test_mdot_of_nothing():
    y = dev(np.ones(5))
    assert mpk.mdot([], y).numel() == 0 and mpk.mdot([], np.ones(5)).size == 0


# ----------------------------------------------------------------------------------------------------------------- maxpy

@pytest.mark.parametrize("n", sorted(GPU_SIZES, reverse=True))
def test_maxpy_bitwise(n):
    """y against the axpy chain for both signs; the norm from the update against the tree of that y.  The norm is asked for on
    the aligned y with negate = 1 and on the odd y with negate = 0, so both variants of the last launch run on both branches."""
    ms = counts(n)
    for kind in DATA:
        basis, y0 = make(kind, n, max(ms), n + 29)
        rows = dev_rows(basis)
        for m in ms:
            c = coefs(m, n + m)
            dc = dev(c)
            for negate in (0, 1):
                what = f"n={n} m={m} {kind} negate={negate}"
                want = axpy_chain(c, basis, y0, negate)
                yh = y0.copy()
                mpk.maxpy(c, list(basis[:m]), yh, negate=bool(negate))
                assert_same(yh, want, f"host y {what}")
                for odd, dy in enumerate((dev(y0), odd_view(y0))):
                    if odd != negate:
                        _, nrm = mpk.maxpy(dc, rows[:m], dy, negate=bool(negate), norm=True)
                        assert_same(np.float64(val(nrm)), np.float64(O.tree_norm2(want)), f"norm {what} odd={odd}")
                    else:
                        mpk.maxpy(dc, rows[:m], dy, negate=bool(negate))
                    assert_same(dy, want, f"device y {what} odd={odd}")
        if n:
            assert_same(torch.stack(rows), basis, "the basis is read only")


def test_maxpy_host_norm_and_empty_basis():
    """norm=True on the host form; m = 0 with a norm leaves y alone and still gives its norm."""
    n = 3001
    basis, y0 = make("mixed", n, 3, 5)
    c = coefs(3, 6)
    want = axpy_chain(c, basis, y0, 1)
    yh = y0.copy()
    _, nrm = mpk.maxpy(c, list(basis), yh, negate=True, norm=True)
    assert_same(yh, want)
    assert_same(np.float64(nrm), np.float64(O.tree_norm2(want)))
    for dy in (dev(y0), odd_view(y0)):
        _, nrm = mpk.maxpy(torch.empty(0, dtype=torch.float64, device="cuda"), [], dy, norm=True)
        assert_same(dy, y0, "m = 0: y untouched")
        assert_same(np.float64(val(nrm)), np.float64(O.tree_norm2(y0)), "m = 0: the norm of y")
        mpk.maxpy([], [], dy)
        assert_same(dy, y0, "m = 0, no norm: nothing happens")


def test_maxpy_ieee_data_sets():
    for pat, name, p, c, v, x, block, pins in ieee_inputs():
        ax = O.spmv(p, c, v, x)
        basis = np.stack([x, ax])
        co = np.array([0.5, -2.0])
        for y0 in (x, ax):
            want = axpy_chain(co, basis, y0, 0)
            for dy in (dev(y0), odd_view(y0)):
                _, nrm = mpk.maxpy(dev(co), dev_rows(basis), dy, norm=True)
                assert_same(dy, want, f"{pat}/{name} y")
                assert_same(np.float64(val(nrm)), np.float64(O.tree_norm2(want)), f"{pat}/{name} norm")


# ------------------------------------------------------------------------------------------------------------------- cgs

@pytest.mark.parametrize("n,m", [(1_048_577, 9), (3001, 64)])
@pytest.mark.parametrize("passes", [1, 2])
def test_cgs_bitwise(n, m, passes):
    for kind in DATA:
        basis, y0 = make(kind, n, m, n + m + passes)
        y_want, h_want, nrm_want = cgs_model(basis, y0, passes)
        rows = dev_rows(basis)
        for dy in (dev(y0), odd_view(y0)):
            h, nrm = mpk.cgs(rows, dy, passes=passes)
            what = f"n={n} m={m} passes={passes} {kind}"
            assert_same(h, h_want, f"h {what}")
            assert_same(dy, y_want, f"y {what}")
            assert_same(np.float64(val(nrm)), np.float64(nrm_want), f"norm {what}")
        if n == 3001:  # the host form composes the host calls
            yh = y0.copy()
            h, nrm = mpk.cgs(list(basis), yh, passes=passes)
            assert_same(h, h_want, f"host h {kind}")
            assert_same(yh, y_want, f"host y {kind}")
            assert_same(np.float64(nrm), np.float64(nrm_want), f"host norm {kind}")


def test_cgs_against_nothing_and_of_nothing():
    y0 = make("mixed", 513, 1, 1)[1]
    dy = dev(y0)
    h, nrm = mpk.cgs([], dy)
    assert h.numel() == 0
    assert_same(dy, y0)
    assert_same(np.float64(val(nrm)), np.float64(O.tree_norm2(y0)))
    e = torch.empty(0, dtype=torch.float64, device="cuda")
    h, nrm = mpk.cgs([e, e.clone()], torch.empty(0, dtype=torch.float64, device="cuda"))
    assert_same(h, np.zeros(2), "n = 0: h = 0")
    assert_same(np.float64(val(nrm)), np.float64(0.0), "n = 0: norm = 0")


# --------------------------------------------------------------------------------------------------------- Krylov basis

def _basis_call(A, s, dv0, ldv, passes):
    n = A.n
    V = torch.full(((s + 1) * ldv,), float("nan"), dtype=torch.float64, device="cuda")
    coef = torch.zeros(s * (s + 2) + 1, dtype=torch.float64, device="cuda")
    mpk.check(mpk.lib().mi_krylov_basis_cgs_dev(A.handle, s, ctypes.c_void_p(dv0.data_ptr()), ctypes.c_void_p(V.data_ptr()), ldv, passes,
                                                ctypes.c_void_p(coef.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    Vh = V.cpu().numpy()
    return np.stack([Vh[k * ldv:k * ldv + n] for k in range(s + 1)]), coef[:s * (s + 2)].reshape(s, s + 2), coef[s * (s + 2)]


@pytest.mark.parametrize("n", [20_001, 20_000])
@pytest.mark.parametrize("passes", [1, 2])
def test_krylov_basis_cgs_bitwise_and_independent_of_ldv(n, passes):
    s = 5
    p, c, v = synth.rows("s15", n)
    A = mpk.csrmatrix(n, p, c, v)
    v0 = synth.x_sin(0, n)
    V_want, H_want, nrm_want = _replay_krylov_cgs(p, c, v, v0, s, passes)
    V, H, nrm0 = mpk.BuildKrylovBasis(A, dev(v0), s, orth="cgs2" if passes == 2 else "cgs")
    assert_same(np.float64(val(nrm0)), np.float64(nrm_want), "||v0||")
    assert_same(V, V_want, f"V, ldv = n = {n}")
    assert_same(H, H_want, f"H, ldv = n = {n}")
    for ldv in (n, n + 1):
        V2, H2, nrm2 = _basis_call(A, s, dev(v0), ldv, passes)
        assert_same(V2, V_want, f"V, ldv = {ldv}")
        assert_same(H2, H_want, f"H, ldv = {ldv}")
        assert_same(nrm2, np.float64(nrm_want))
    A.close()


def test_krylov_basis_cgs2_stays_orthonormal_at_restart_length():
    """s = 30 on the headline family, where the sweep of orth=True ends 0.7 away from orthonormal (tests/test_cgs_model.py)."""
    n, s = 20_001, 30
    p, c, v = synth.rows("s15", n)
    A = mpk.csrmatrix(n, p, c, v)
    v0 = synth.x_sin(0, n)
    V_want, H_want, nrm_want = _replay_krylov_cgs(p, c, v, v0, s, 2)
    V, H, nrm0 = mpk.BuildKrylovBasis(A, dev(v0), s, orth="cgs2")
    assert_same(np.float64(val(nrm0)), np.float64(nrm_want), "||v0||")
    assert_same(V, V_want, "V")
    assert_same(H, H_want, "H")
    e = loss(V.cpu().numpy())
    print(f"device CGS2 basis, s15 n={n} s={s}: max |V^T V - I| = {e:.3e}")
    assert e <= 1e-14, e
    A.close()


def test_krylov_basis_cgs_arguments():
    """The argument rules that need a handle (the others: tests/test_multi_blas1_abi.py)."""
    L = mpk.lib()
    A = mpk.csrmatrix(2, [0, 1, 2], [0, 1], [1.0, 2.0])
    v0, V, coef = dev(np.ones(2)), torch.zeros(6, dtype=torch.float64, device="cuda"), torch.zeros(9, dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def refused(status, word):
        assert status == 1 and word in L.mi_last_error().decode(), (status, L.mi_last_error())
    for passes in (0, 3):
        refused(L.mi_krylov_basis_cgs_dev(A.handle, 2, p(v0), p(V), 2, passes, p(coef), None), "passes")
    for s in (-1, 65):
        refused(L.mi_krylov_basis_cgs_dev(A.handle, s, p(v0), p(V), 2, 2, p(coef), None), "s must be")
    refused(L.mi_krylov_basis_cgs_dev(A.handle, 2, p(v0), p(V), 2, 2, None, None), "bad argument")
    refused(L.mi_krylov_basis_cgs_dev(A.handle, 2, p(v0), p(V), 1, 2, p(coef), None), "bad argument")
    R = mpk.csrmatrix(2, [0, 1, 2], [0, 2], [1.0, 2.0], ncols=3)
    refused(L.mi_krylov_basis_cgs_dev(R.handle, 2, p(v0), p(V), 2, 2, p(coef), None), "square")
    torch.cuda.synchronize()
    assert not V.cpu().numpy().any() and not coef.cpu().numpy().any(), "a refused call wrote something"
    A.close()
    R.close()


# --------------------------------------------------------------------------------------------------------------- streams

def test_fresh_non_blocking_stream():
    """The first calls on a stream that never reduced (its workspace is allocated there), then the same again; results equal
    the default stream's."""
    n, m = 1_048_577, 9
    basis, y0 = make("cancel", n, m, 77)
    rows = dev_rows(basis)
    y_want, h_want, nrm_want = cgs_model(basis, y0, 2)
    dots_want = np.array([O.tree_dot(y0, b) for b in basis], dtype=np.float64)
    torch.cuda.synchronize()
    s1 = torch.cuda.Stream()
    for rep in range(2):
        dy = odd_view(y0)
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            dots = mpk.mdot(rows, dy)
            h, nrm = mpk.cgs(rows, dy)
        s1.synchronize()
        assert_same(dots, dots_want, f"dots, non-blocking stream, call {rep}")
        assert_same(h, h_want, f"h, non-blocking stream, call {rep}")
        assert_same(dy, y_want, f"y, non-blocking stream, call {rep}")
        assert_same(np.float64(val(nrm)), np.float64(nrm_want), f"norm, non-blocking stream, call {rep}")
    dy = dev(y0)
    h, nrm = mpk.cgs(rows, dy)
    assert_same(h, h_want, "h, default stream")
    assert_same(dy, y_want, "y, default stream")


# ------------------------------------------------------------------------------------------------------------- the tile

_CHILD = r"""
import hashlib
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
from navierstokes_amd import mpk
from test_gpu_multi_blas1 import coefs, dev_rows, make
import torch
n, m = int(sys.argv[2]), int(sys.argv[3])
bits = lambda a: " ".join(str(int(b)) for b in np.ascontiguousarray(a.cpu().numpy().reshape(-1)).view(np.uint64))
sha = lambda t: hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()
for kind in ("mixed", "cancel"):
    basis, y0 = make(kind, n, m, n + m)
    rows = dev_rows(basis)
    dy = torch.from_numpy(y0).cuda()
    print("R", kind, "dots", bits(mpk.mdot(rows, dy)), flush=True)
    _, nrm = mpk.maxpy(torch.from_numpy(coefs(m, m)).cuda(), rows, dy, negate=True, norm=True)
    print("R", kind, "maxpy", sha(dy), bits(nrm), flush=True)
    dy = torch.from_numpy(y0).cuda()
    h, nrm = mpk.cgs(rows, dy, passes=2)
    print("R", kind, "cgs", sha(dy), bits(nrm), bits(h), flush=True)
"""


@pytest.mark.parametrize("tile", ["4", "8", "16"])
def test_bits_do_not_depend_on_the_tile(tile):
    """MI355_MDOT_TILE is read once per process: each compiled value in a fresh child; m = 17 is a full tile plus one for 16,
    two plus one for 8, four plus one for 4."""
    n, m = 300_001, 17
    env = dict(os.environ, MI355_MDOT_TILE=tile)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(n), str(m)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("R ")]
    assert len(lines) == 6, r.stdout
    f64 = lambda toks: np.array([int(t) for t in toks], dtype=np.uint64).view(np.float64)  # noqa: E731
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()  # noqa: E731
    for kind in ("mixed", "cancel"):
        basis, y0 = make(kind, n, m, n + m)
        got = {ln[2]: ln[3:] for ln in lines if ln[1] == kind}
        assert_same(f64(got["dots"]), np.array([O.tree_dot(y0, b) for b in basis], dtype=np.float64), f"tile {tile} {kind} dots")
        want = axpy_chain(coefs(m, m), basis, y0, 1)
        assert got["maxpy"][0] == sha(want), f"tile {tile} {kind}: y of maxpy"
        assert_same(f64(got["maxpy"][1:]), np.array([O.tree_norm2(want)]), f"tile {tile} {kind} norm of maxpy")
        y_want, h_want, nrm_want = cgs_model(basis, y0, 2)
        assert got["cgs"][0] == sha(y_want), f"tile {tile} {kind}: y of cgs"
        assert_same(f64(got["cgs"][1:2]), np.array([nrm_want]), f"tile {tile} {kind} norm of cgs")
        assert_same(f64(got["cgs"][2:]), h_want, f"tile {tile} {kind} h")
