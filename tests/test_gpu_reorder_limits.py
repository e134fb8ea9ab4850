"""The relabelled twin (reorder.hpp; maybe_reorder in capi_csr.hip) at every limit of its construction and through every entry point that
takes a relabelled handle.  mi_csr_create keeps no natural-order arrays on such a handle: whatever does not go through the twin reads a
null pointer.  The patterns are the families of tests/reorder_cases.py; tests/test_reorder_cases.py shows on the CPU that each reaches what
it is for (the identity that gives the twin the OFFSET form of its row map, disconnected graphs, rows of more than 256 and more than 2048
nonzeros, n on both sides of the 64-row groups of the refresh kernel and past its grid cap, a twin eligible for the one-launch powers step
and one for the sliced stream).

Every test forces the relabelling (MI355_REORDER=1), asserts that the handle reports it with the expected block, and compares BITWISE with
the oracle on the matrix as delivered (the relabelling keeps each row's terms in the caller's order): O.spmv, O.spmk_chain, O.tree_dot,
O.tree_ortho_update, O.tree_mgs, O.tree_norm2.  A NaN matches any NaN (test_gpu_edges.assert_same).  Outputs start as NaN and are followed by
NaN guard entries that must stay NaN.  The one comparison that is not against the oracle is the GMRES one: it is bitwise between two paths of
the library that evaluate the same chains by construction, and says so."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import reorder_cases as RC
from navierstokes_amd import mpk, synth
from oracle import oracle as O
from test_cgs_model import _replay_krylov_cgs
from test_gpu_edges import HIP_STREAM_NON_BLOCKING, assert_same, stream_flags
from test_gpu_reductions import _replay_krylov, val
from test_reorder_cases import reorder_probe

pytestmark = pytest.mark.gpu

GUARD = 8
MI_MAX_POWERS = 16   # include/mi355_spmv.h
MI_ERR_STATE = 6
ALPHA = 1e-8
BLOCK_CASES = [name for name in RC.NAMES if RC.BLOCK[name] == 4]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    mpk.lib()
    yield


@pytest.fixture(autouse=True)
def _forced(monkeypatch):
    monkeypatch.setenv("MI355_REORDER", "1")


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()   # (a copy: the cases' arrays are shared and read-only)


def view(a, off):
    """a device copy of a that starts `off` doubles into its (256-byte aligned) allocation: off = 1 is 8 bytes off a 16-byte boundary"""
    a = np.asarray(a)
    buf = torch.full((len(a) + 2,), float("nan"), dtype=torch.float64, device="cuda")
    buf[off:off + len(a)] = dev(a)
    out = buf[off:off + len(a)]
    assert len(a) == 0 or out.data_ptr() % 16 == 8 * off
    return out


class Out:
    """an output of n doubles, `off` doubles into its allocation, NaN everywhere, GUARD entries behind it that must stay NaN"""

    def __init__(self, n, off=0):
        self.n, self.off = n, off
        self.buf = torch.full((off + n + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
        self.t = self.buf[off:off + n]
        assert n == 0 or self.t.data_ptr() % 16 == 8 * off

    def check(self, want, what):
        h = self.buf.cpu().numpy()
        assert_same(h[self.off:self.off + self.n], want, what)
        assert np.isnan(h[:self.off]).all() and np.isnan(h[self.off + self.n:]).all(), f"{what}: wrote outside y"
        self.buf.fill_(float("nan"))


@functools.lru_cache(maxsize=None)
def xvec(name, j=0):
    """seeded x from (-1, 1); `components`: +Inf at the column no row names"""
    n, p, c, _ = RC.case(name)
    x = np.random.default_rng([RC.seed(name), 100 + j]).uniform(-1, 1, n)
    if name == "components":
        (unnamed,) = np.setdiff1d(np.arange(n), c)
        x[unnamed] = np.inf
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def want_spmv(name, k=0, j=0):
    n, p, c, values = RC.case(name)
    y = O.spmv(p, c, values(k), xvec(name, j))
    assert np.isfinite(y).all()                               # (the Inf of `components` reaches no row)
    y.setflags(write=False)
    return y


def handle(name, v=None):
    """the case as a handle, with what every test asserts first: relabelled, by the expected block (tridiag:7: not relabelled)"""
    n, p, c, values = RC.case(name)
    A = mpk.csrmatrix(n, p, c, values(0) if v is None else v)
    info = A.reorder_info()
    if RC.BLOCK[name] is None:
        assert info["reordered"] is False, info
    else:
        assert info["reordered"] is True and info["block"] == RC.BLOCK[name], (name, info)
    return A


def sell_env(name, monkeypatch):
    """block cases: the blocked copy of the twin in its sliced form, the four variants dealt out over the cases"""
    if name in BLOCK_CASES:
        monkeypatch.setenv("MI355_BCSR_SELL", "1")
        monkeypatch.setenv("MI355_BCSR_SELL_FORM", str(BLOCK_CASES.index(name) % 4))


KERNEL_NAMES = {"stream": "spmv_csr_stream<", "ring": "spmv_csr_ring<", "rowpar": "spmv_csr_rowpar", "tile": "spmv_csr_tile<",
                "mring": "spmv_csr_mring<", "bcsr4": "spmv_bcsr4_sell<", "sstream": "spmv_sstream<"}


def force(A, kern):
    A.set_kernel(kern)
    assert A.kernel_name().startswith(KERNEL_NAMES[kern]), f"asked for {kern}, the handle runs {A.kernel_name()}"


# ------------------------------------------------------------------------------------------------------------ every kernel

@pytest.mark.parametrize("name", [nm for nm in RC.NAMES if nm != "stride"])
def test_every_kernel(name, monkeypatch):
    """The permutation is the probe's; host and device products; then every kernel of the twin forced and NAMED (a fallback fails), with x
    and y aligned and 8 bytes off a 16-byte boundary in all four combinations.  include/mi355_spmv.h documents no refusal of an 8-byte
    aligned vector for a CSR handle, so every combination must give the oracle's bits."""
    sell_env(name, monkeypatch)
    if name == "sliced":
        monkeypatch.setenv("MI355_SSTREAM", "1")
        monkeypatch.setenv(*RC.SLICED_ENV)
    n, p, c, values = RC.case(name)
    x, yo = xvec(name), want_spmv(name)
    A = handle(name)
    reordered, perm = A.perm()
    if RC.BLOCK[name] is None:
        assert not reordered and np.array_equal(perm, np.arange(n))
    else:
        assert reordered and np.array_equal(perm, reorder_probe(p, c)[1]), "mi_csr_perm is not mi_reorder_probe's permutation"
    y = np.full(n, np.nan)
    mpk.SpMV_CSR(y, x, A)
    assert_same(y, yo, f"{name}: host SpMV_CSR ({A.kernel_name()})")
    kernels = ["auto", "stream", "ring", "rowpar", "tile", "mring"]
    if name in BLOCK_CASES:
        kernels.append("bcsr4")
    if name == "sliced":
        kernels.append("sstream")
    for xoff, yoff in ((0, 0), (1, 1), (1, 0), (0, 1)):
        xd, out = view(x, xoff), Out(n, yoff)
        for kern in kernels:
            if kern == "auto":
                A.set_kernel("auto")
            else:
                force(A, kern)
            mpk.SpMV_CSR(out.t, xd, A)
            out.check(yo, f"{name}: {kern} -> {A.kernel_name()}, x {8 * xoff} and y {8 * yoff} bytes off")
    A.close()


# ------------------------------------------------------------------------------------------------------------ value refresh

@pytest.mark.parametrize("name", ["tridiag:63", "tridiag:64", "tridiag:65", "tridiag:129", "blocktridiag:17", "fe:4", "hub", "long:2500",
                                  "unsorted", "stride"])
def test_value_refresh(name, monkeypatch):
    """permute_values_kernel (64 new rows per workgroup, bisection over 65 row pointers, 256 elements per pass, at most 4096 groups) and what
    follows it on the twin: a host refresh; a device refresh on one stream with the product on a second behind wait_stream; a device
    refresh from an array 8 bytes off alignment.  The block cases run the product through the blocked sliced copy, then through the stream
    kernel, which reads the twin's CSR values.  `stride` (262 209 rows: the grid's second turn) runs one device refresh and one product."""
    sell_env(name, monkeypatch)
    n, p, c, values = RC.case(name)
    A = handle(name)
    x = xvec(name)
    xd = dev(x)
    kernels = ["bcsr4", "stream"] if name in BLOCK_CASES else ["auto"]

    def products(k, what):
        for kern in kernels:
            if kern == "auto":
                A.set_kernel("auto")
            else:
                force(A, kern)
            out = Out(n)
            mpk.SpMV_CSR(out.t, xd, A)
            out.check(want_spmv(name, k), f"{name}: {what} ({kern} -> {A.kernel_name()})")

    if name == "stride":
        A.update_values(dev(values(1)))
        products(1, "device refresh past the grid cap")
        A.close()
        return
    products(0, "as created")
    A.update_values(values(1))
    products(1, "host refresh")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    assert all(stream_flags(s) & HIP_STREAM_NON_BLOCKING for s in (s1, s2))
    v2 = dev(values(2))
    outs = [Out(n) for _ in kernels]
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        A.update_values(v2)
    s2.wait_stream(s1)
    for kern, out in zip(kernels, outs):
        if kern != "auto":
            force(A, kern)   # (set outside the stream context: mi_csr_set_kernel synchronises the null stream only)
        with torch.cuda.stream(s2):
            mpk.SpMV_CSR(out.t, xd, A)
    torch.cuda.synchronize()
    for kern, out in zip(kernels, outs):
        out.check(want_spmv(name, 2), f"{name}: device refresh on s1, product on s2 ({kern})")
    v0 = view(values(0), 1)
    A.update_values(v0)
    products(0, "device refresh from an 8-byte aligned array")
    A.close()


# ------------------------------------------------------------------------------------------------------------------ powers

def _power_scale(name):
    """1 / (longest row): |A x|_inf <= |x|_inf, so sixteen powers stay finite"""
    return 1.0 / float(max(1, np.diff(RC.case(name)[1]).max()))


@pytest.mark.parametrize("name", ["tridiag:64", "band:1000", "components", "fe:4", "long:2500"])
def test_powers(name):
    """mi_spmk_dev on a relabelled handle at k = 1, 2, MI_MAX_POWERS and back (the power buffers d_pp grow, then are reused);
    mi_spmk_internal_dev un-permuted; to_internal / from_internal against perm; the product in the internal numbering."""
    n, p, c, values = RC.case(name)
    scale = _power_scale(name)
    v = values(0) * scale
    A = handle(name, v)
    x = xvec(name)
    xd = dev(x)
    Y = O.spmk_chain(MI_MAX_POWERS, p, c, v, x)
    assert np.isfinite(Y).all()
    for k in (1, 2, MI_MAX_POWERS, 2, 1):
        outs = [Out(n) for _ in range(k)]
        mpk.SpMkV([o.t for o in outs], xd, A)
        for q, o in enumerate(outs):
            o.check(Y[q], f"{name}: k = {k}, power {q + 1}")
    hy = [np.full(n, np.nan) for _ in range(MI_MAX_POWERS)]
    mpk.SpMkV(hy, x, A)
    for q in range(MI_MAX_POWERS):
        assert_same(hy[q], Y[q], f"{name}: host k = {MI_MAX_POWERS}, power {q + 1}")
    # the library's numbering: x_int[perm[i]] = x[i]
    _, perm = A.perm()
    xf = np.where(np.isfinite(x), x, 0.5)      # (`components`: the internal calls below are checked against a finite x as well as the Inf one)
    for xx in (x, xf):
        for off in (0, 1):                     # (gather_perm and scatter_perm: the node form of a block-4 handle needs 16-byte aligned vectors)
            xi = Out(n, off)
            A.to_internal(view(xx, off), xi.t)
            xi.check(xx[np.argsort(perm)], f"{name}: to_internal, {8 * off} bytes off")
            A.to_internal(view(xx, off), xi.t)
            back = Out(n, off)
            A.from_internal(xi.t, back.t)
            back.check(xx, f"{name}: from_internal undoes to_internal, {8 * off} bytes off")
    xi = A.to_internal(xd)
    outs = [torch.full((n,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(3)]
    ptrs = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in outs])
    mpk.check(mpk.lib().mi_spmk_internal_dev(A.handle, 3, ctypes.c_void_p(xi.data_ptr()), ptrs, mpk._stream_ptr()))
    for q in range(3):
        back = Out(n)
        A.from_internal(outs[q], back.t)
        back.check(Y[q], f"{name}: mi_spmk_internal_dev, power {q + 1}, un-permuted")
    yi = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    mpk.SpMV_CSR_internal(yi, xi, A)
    assert_same(yi.cpu().numpy()[perm], Y[0], f"{name}: SpMV_CSR_internal")
    A.close()


def test_one_launch_powers_on_a_twin(monkeypatch):
    """The twin itself is what spmk_setup judges (launch_spmk.hip tests H->inner on the TWIN, where it is null), so a relabelled band runs
    the one-launch step.  Asserted, not assumed: spmk_info says which form ran.  k = 4, 2, 8, 4 on one handle with a different x each time
    (the flags' epoch counts on from step to step), then MI355_SPMK_FUSED=0 gives the same bits."""
    name = "powers"
    n, p, c, values = RC.case(name)
    assert n == RC.powers_size()
    v = values(0) * _power_scale(name)
    monkeypatch.setenv("MI355_SPMK_FUSED", "1")
    A = handle(name, v)
    force(A, "ring")
    steps = [(4, 0), (2, 1), (8, 2), (4, 3)]
    got = []
    for k, j in steps:
        outs = [Out(n) for _ in range(k)]
        mpk.SpMkV([o.t for o in outs], dev(xvec(name, j)), A)
        assert A.spmk_info(k)["one_launch"] is True, (k, A.spmk_info(k), A.kernel_name())
        Y = O.spmk_chain(k, p, c, v, xvec(name, j))
        for q, o in enumerate(outs):
            got.append(o.t.cpu().numpy().copy())
            o.check(Y[q], f"one launch, k = {k}, x {j}, power {q + 1}")
    monkeypatch.setenv("MI355_SPMK_FUSED", "0")
    i = 0
    for k, j in steps:
        outs = [Out(n) for _ in range(k)]
        mpk.SpMkV([o.t for o in outs], dev(xvec(name, j)), A)
        assert A.spmk_info(k)["one_launch"] is False
        for q, o in enumerate(outs):
            o.check(got[i], f"k launches, k = {k}, x {j}, power {q + 1}")
            i += 1
    A.close()


# -------------------------------------------------------------------------------------------------- product with dot and update

@pytest.mark.parametrize("name", ["tridiag:65", "components", "fe:3"])
def test_product_with_dot_and_update(name):
    """mi_spmv_dot_dev / mi_spmv_orthogonalize_dev on a relabelled handle: no epilogue (the header: "relabelled or blocked matrices run
    product and dot as separate launches"), so beta is mi_dot_dev's tree over (b, y) in the CALLER's numbering."""
    n, p, c, values = RC.case(name)
    A = handle(name)
    assert A.dot_in_epilogue() is False
    with pytest.raises(mpk.MiError):
        A.dot_epilogue_layout()
    x, yo = xvec(name), want_spmv(name)
    b = np.random.default_rng([RC.seed(name), 7]).uniform(-1, 1, n)
    want = O.tree_dot(b, yo)
    xd, bd = dev(x), dev(b)
    y = Out(n)
    beta = mpk.SpMV_CSR_dot(y.t, xd, A, bd)
    y.check(yo, f"{name}: y of mi_spmv_dot_dev")
    assert_same(np.float64(val(beta)), np.float64(want), f"{name}: beta")
    x1, x3 = Out(n), Out(n)
    beta3 = mpk.SpMV_CSR_orthogonalize(x1.t, xd, A, bd, x3.t, ALPHA)
    assert_same(np.float64(val(beta3)), np.float64(want), f"{name}: beta of mi_spmv_orthogonalize_dev")
    x1.check(yo, f"{name}: x1")
    x3.check(O.tree_ortho_update(ALPHA, want, b, yo), f"{name}: x3")
    A.close()


# ------------------------------------------------------------------------------------------------------------ multi-vector

@pytest.mark.parametrize("name", ["fe:4", "band:1000"])
def test_multi_vector(name):
    """mi_spmm_dev at s = 1, 3, 4, 8: X 16-byte aligned with even ldx (fe:4: the s columns gathered, one launch over the blocked twin);
    X one double off, and an odd ldx (column by column through launch_spmv and the per-stream gather buffer); a padded ldy."""
    n, p, c, values = RC.case(name)
    assert n % 2 == 0
    A = handle(name)
    S = 8
    X = np.stack([xvec(name, j) for j in range(S)])
    want = np.stack([want_spmv(name, 0, j) for j in range(S)])
    vp = ctypes.c_void_p
    for s in (1, 3, 4, 8):
        for what, xoff, ldx, ldy in (("aligned X, even ldx", 0, n, n), ("X one double off", 1, n, n), ("odd ldx", 0, n + 1, n),
                                     ("padded ldy", 0, n, n + 3), ("X one double off, odd ldx, padded ldy", 1, n + 1, n + 3)):
            bx = torch.full((xoff + s * ldx + 1,), float("nan"), dtype=torch.float64, device="cuda")
            for j in range(s):
                bx[xoff + j * ldx:xoff + j * ldx + n] = dev(X[j])
            by = torch.full((s * ldy + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
            mpk.check(mpk.lib().mi_spmm_dev(A.handle, s, vp(bx.data_ptr() + 8 * xoff), ldx, vp(by.data_ptr()), ldy, mpk._stream_ptr()))
            h = by.cpu().numpy()
            written = np.zeros(len(h), bool)
            for j in range(s):
                assert_same(h[j * ldy:j * ldy + n], want[j], f"{name}: s = {s}, {what}, column {j}")
                written[j * ldy:j * ldy + n] = True
            assert np.isnan(h[~written]).all(), f"{name}: s = {s}, {what}: wrote outside the columns of Y"
    A.close()


# ------------------------------------------------------------------------------------------------------------ Krylov bases

def _basis_start(name):
    """v0 for the bases: a seeded draw with every entry nonzero, so that every component of `components` (its empty rows aside) takes part;
    that the basis does not break down in the steps taken is asserted on the model in the test"""
    n = RC.case(name)[0]
    return np.random.default_rng([RC.seed(name), 9]).uniform(-1, 1, n)


@pytest.mark.parametrize("name", ["fe:3", "components"])
def test_krylov_bases(name):
    """mi_krylov_basis_dev (monomial and orthonormal) and mi_krylov_basis_cgs_dev (one and two passes) on a relabelled handle, replayed with
    the oracle's product and trees exactly as tests/test_gpu_reductions.py and tests/test_gpu_multi_blas1.py replay them on natural handles."""
    s = 3
    n, p, c, values = RC.case(name)
    v = values(0)
    v0 = _basis_start(name)
    A = handle(name)
    V, _, _ = mpk.BuildKrylovBasis(A, dev(v0), s, orth=False)
    assert_same(V[0], v0, f"{name}: monomial basis, column 0")
    assert_same(V[1:], O.spmk_chain(s, p, c, v, v0), f"{name}: monomial basis = the powers chain")
    V_want, H_want, nrm_want = _replay_krylov(p, c, v, v0, s)
    # no breakdown: every norm the basis divides by is far from zero next to the vector it came from
    assert np.isfinite(V_want).all() and nrm_want > 0 and (H_want[np.arange(s), np.arange(s) + 1] > 1e-3).all(), H_want
    V, H, nrm0 = mpk.BuildKrylovBasis(A, dev(v0), s, orth=True)
    assert_same(np.float64(val(nrm0)), np.float64(nrm_want), f"{name}: ||v0||")
    assert_same(V, V_want, f"{name}: orthonormal basis")
    assert_same(H, H_want, f"{name}: its coefficients")
    for passes in (1, 2):
        V_want, H_want, nrm_want = _replay_krylov_cgs(p, c, v, v0, s, passes)
        assert np.isfinite(V_want).all() and (H_want[np.arange(s), np.arange(s) + 1] > 1e-3).all(), H_want
        V, H, nrm0 = mpk.BuildKrylovBasis(A, dev(v0), s, orth="cgs2" if passes == 2 else "cgs")
        assert_same(np.float64(val(nrm0)), np.float64(nrm_want), f"{name}: CGS{passes} ||v0||")
        assert_same(V, V_want, f"{name}: CGS basis, {passes} passes")
        assert_same(H, H_want, f"{name}: CGS coefficients, {passes} passes")
    A.close()


# ------------------------------------------------------------------------------------------------------------------- GMRES

@pytest.mark.parametrize("name", ["fe:3"])
def test_gmres_operator(name):
    """mi_gmres_set_operator_csr with a relabelled operator: GMRES(5), 12 iterations, without M and with bilu4(fill = 0) built from the same
    delivered blocks.  NOT against the oracle: history, count, reason and x are bit-equal to the solver on a bcsr4x4_matrix of the same
    matrix — both operators evaluate every row as the same fma chain (block columns ascending = CSR order), everything else is shared."""
    n, p, c, values = RC.case(name)
    v = values(0).copy()
    v[c == np.repeat(np.arange(n), np.diff(p))] += 4.0   # a dominant diagonal: ILU(0) exists and the iteration moves
    bp, bc, bv = synth.csr_to_bcsr4(p, c, v)
    nb = n // 4
    A = handle(name, v)
    B = mpk.bcsr4x4_matrix(nb, bp, bc, bv)
    F = mpk.bilu4(nb, bp, bc, bv, fill=0)
    b = dev(np.random.default_rng([RC.seed(name), 11]).uniform(-1, 1, n))
    for M in (None, F):
        runs = []
        for op in (A, B):
            S = mpk.gmres_solver(op, M, restart=5)
            x = torch.zeros(n, dtype=torch.float64, device="cuda")
            its, hist, reason = S.solve(b, x, rtol=1e-30, maxiter=12)
            runs.append((its, hist, reason, x.cpu().numpy()))
            S.close()
        (its, hist, reason, x), (its_b, hist_b, reason_b, x_b) = runs
        what = f"{name}, M = {'bilu4' if M else 'none'}"
        assert (its, reason) == (its_b, reason_b) and its == 12, (what, its, reason, its_b, reason_b)
        assert_same(np.array(hist), np.array(hist_b), f"{what}: residual history")
        assert_same(x, x_b, f"{what}: x")
        assert np.isfinite(x).all() and hist[-1] < hist[0]
    F.close(), B.close(), A.close()


# ------------------------------------------------------------------------------------------------------ streams and capture

def test_streams_and_capture():
    """One gather buffer per stream: concurrent products on two streams; the first product on a third, fresh stream INSIDE capture is
    refused with MI_ERR_STATE (reorder_scratch would have to allocate) and the handle stays usable; after one product on that stream outside
    capture a captured product replays with new x and, after a device refresh on that stream, with new values."""
    name = "band:1000"
    n, p, c, values = RC.case(name)
    A = handle(name)
    s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    assert all(stream_flags(s) & HIP_STREAM_NON_BLOCKING for s in (s1, s2, s3))
    xa, xb = dev(xvec(name, 0)), dev(xvec(name, 1))
    ya, yb = Out(n), Out(n)
    torch.cuda.synchronize()
    for _ in range(20):
        with torch.cuda.stream(s1):
            mpk.SpMV_CSR(ya.t, xa, A)
        with torch.cuda.stream(s2):
            mpk.SpMV_CSR(yb.t, xb, A)
    torch.cuda.synchronize()
    ya.check(want_spmv(name, 0, 0), "stream 1")
    yb.check(want_spmv(name, 0, 1), "stream 2")
    # a third stream, never used with this handle: its first product under capture has no gather buffer
    xc, yc = dev(xvec(name, 2)), Out(n)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s3):
        yc.t.fill_(0.0)   # (so that the graph is not empty)
        with pytest.raises(mpk.MiError) as e:
            mpk.SpMV_CSR(yc.t, xc, A)
    assert e.value.status == MI_ERR_STATE and "captur" in str(e.value), str(e.value)
    del g
    yc.buf.fill_(float("nan"))
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        mpk.SpMV_CSR(ya.t, xb, A)
    torch.cuda.synchronize()
    ya.check(want_spmv(name, 0, 1), "the handle after the refusal")
    with torch.cuda.stream(s3):
        mpk.SpMV_CSR(yc.t, xc, A)
    torch.cuda.synchronize()
    yc.check(want_spmv(name, 0, 2), "stream 3, outside capture")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s3):
        mpk.SpMV_CSR(yc.t, xc, A)
    v1 = dev(values(1))
    torch.cuda.synchronize()
    for k, j in ((0, 0), (0, 1), (1, 1), (1, 2)):
        with torch.cuda.stream(s3):
            xc.copy_(dev(xvec(name, j)), non_blocking=False)
            if k == 1:
                A.update_values(v1)
            g.replay()
        torch.cuda.synchronize()
        yc.check(want_spmv(name, k, j), f"replay with x {j}, values {k}")
    A.close()
