"""Every reduction of the library held bit for bit to the oracle's model of its fixed summation tree (oracle/cpu_ref.c, "BITWISE
MODELS"; checked against an exact restatement in tests/test_reduction_model.py): dot / norm2 / rel_error, the orthogonalize beta and
update, the Gram-Schmidt sweep, the dot in the ring kernel's epilogue and the separate dot of other handles, the orthonormal Krylov
basis, the distributed dot and orthogonalize, and the shim's BLAS-1 symbols.

Sizes cover every regime of red_geometry (one segment; np reaching 1024, then seg growing), the switch to non-temporal loads and
byte offsets past 2^31.  Views at odd offsets (only 8-byte aligned) must give the bits of contiguous copies, on any stream.

Comparison is bitwise (signed zeros included) except that a NaN matches any NaN (test_gpu_edges.assert_same)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from navierstokes_amd import mpk, synth
from oracle import oracle as O
from test_gpu_edges import assert_same
from test_oracle_vs_reference import ieee_inputs
from test_reduction_model import DATA, GPU_SIZES

pytestmark = pytest.mark.gpu

ALPHA = 1e-8


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    mpk.lib()
    yield


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def odd_view(a):
    """A device copy of a that starts 8 bytes into its allocation (only 8-byte aligned when n > 0)."""
    buf = torch.full((len(a) + 1,), float("nan"), dtype=torch.float64, device="cuda")
    buf[1:] = dev(a)
    return buf[1:]


def val(r):
    return float(r.cpu()) if torch.is_tensor(r) else float(r)


def models(a, b):
    return dict(dot=O.tree_dot(a, b), norm2=O.tree_norm2(a), rel_error=O.tree_rel_error(a, b))


def device_results(da, db):
    return dict(dot=val(mpk.dot(da, db)), norm2=val(mpk.norm2(da)), rel_error=val(mpk.rel_error(da, db)))


def check_all(got, want, what):
    for k in want:
        assert_same(np.float64(got[k]), np.float64(want[k]), f"{what} {k}")


# ------------------------------------------------------------------------------------------------- dot, norm2, rel_error

@pytest.mark.parametrize("n", sorted(GPU_SIZES, reverse=True))
def test_dot_norm2_rel_error_bitwise(n):
    """Host and device forms, contiguous and odd-offset views, four data sets; sizes largest first, so a reduction that read
    partials left over by a larger one would show."""
    for kind in DATA:
        a, b = DATA[kind](n, np.random.default_rng(n + 11))
        want = models(a, b)
        check_all(dict(dot=mpk.dot(a, b), norm2=mpk.norm2(a), rel_error=mpk.rel_error(a, b)), want, f"host n={n} {kind}")
        check_all(device_results(dev(a), dev(b)), want, f"device n={n} {kind}")
        check_all(device_results(odd_view(a), odd_view(b)), want, f"odd views n={n} {kind}")
        check_all(device_results(odd_view(a), dev(b)), want, f"one odd view n={n} {kind}")


def test_ieee_data_sets():
    """x and A x of every IEEE case (non-finite entries, signed zeros, subnormal products, overflow whose class depends on the
    order): the model is the same tree, so even the class and sign of every result must match."""
    for pat, name, p, c, v, x, block, pins in ieee_inputs():
        y = O.spmv(p, c, v, x)
        for a, b in ((x, y), (y, x), (x, x)):
            want = models(a, b)
            check_all(device_results(dev(a), dev(b)), want, f"{pat}/{name}")
            check_all(device_results(odd_view(a), odd_view(b)), want, f"{pat}/{name} odd views")


def test_offsets_past_2_to_the_31_bytes():
    """One odd n above 2^28 elements: element offsets times 8 pass 2^31."""
    n = (1 << 28) + 3
    buf = torch.empty(n + 1, dtype=torch.float64, device="cuda")
    buf.uniform_(-1.0, 1.0, generator=torch.Generator(device="cuda").manual_seed(28))
    h = buf.cpu().numpy()
    a, b = h[:n], h[1:]
    assert_same(np.float64(val(mpk.dot(buf[:n], buf[1:]))), np.float64(O.tree_dot(a, b)), "dot, one view 8-byte aligned")
    assert_same(np.float64(val(mpk.norm2(buf[1:]))), np.float64(O.tree_norm2(b)), "norm2 of the odd view")
    assert_same(np.float64(val(mpk.norm2(buf[:n]))), np.float64(O.tree_norm2(a)), "norm2 of the aligned view")
    del buf


def test_streams():
    """The default stream, a non-blocking stream, and two non-blocking streams at once on different data."""
    n = 1_048_577
    sets = [DATA[k](n, np.random.default_rng(40 + i)) for i, k in enumerate(("mixed", "cancel"))]
    want = [models(a, b) for a, b in sets]
    views = [(odd_view(a), odd_view(b)) for a, b in sets]
    torch.cuda.synchronize()
    check_all(device_results(*views[0]), want[0], "default stream")
    s1 = torch.cuda.Stream()
    with torch.cuda.stream(s1):
        outs = [mpk.dot(*views[1]), mpk.norm2(views[1][0]), mpk.rel_error(*views[1])]
    s1.synchronize()
    check_all(dict(zip(("dot", "norm2", "rel_error"), map(val, outs))), want[1], "non-blocking stream")
    s2 = torch.cuda.Stream()
    got = [[], []]
    for _ in range(3):  # interleaved launches on both streams
        for j, s in enumerate((s1, s2)):
            with torch.cuda.stream(s):
                got[j].append((mpk.dot(*views[j]), mpk.norm2(views[j][0]), mpk.rel_error(*views[j])))
    torch.cuda.synchronize()
    for j in range(2):
        for triple in got[j]:
            check_all(dict(zip(("dot", "norm2", "rel_error"), map(val, triple))), want[j], f"stream {j + 1} of two")


_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
from navierstokes_amd import mpk
from test_reduction_model import DATA
import torch
n = int(sys.argv[2])
for kind in ("mixed", "cancel"):
    a, b = DATA[kind](n, np.random.default_rng(n))
    buf = torch.zeros(2 * n + 2, dtype=torch.float64, device="cuda")
    buf[1:n + 1] = torch.from_numpy(a).cuda()
    buf[n + 2:] = torch.from_numpy(b).cuda()
    for da, db in ((buf[1:n + 1], buf[n + 2:]), (torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())):
        r = [float(mpk.dot(da, db).cpu()), float(mpk.norm2(da).cpu()), float(mpk.rel_error(da, db).cpu())]
        x3 = torch.empty_like(da)
        beta = float(mpk.orthogonalize(n, da, db, x3, 1e-8).cpu())
        r.append(beta)
        print("R", kind, " ".join(str(int(np.float64(v).view(np.uint64))) for v in r), flush=True)
    print("R", kind, "host", " ".join(str(int(np.float64(v).view(np.uint64))) for v in (mpk.dot(a, b), mpk.norm2(a), mpk.rel_error(a, b))), flush=True)
"""


@pytest.mark.parametrize("nt", ["0", "1"])
def test_non_temporal_loads_on_and_off(nt):
    """MI355_BLAS1_NT is read once per process: each setting in a fresh child, at n = 3 000 000, views and copies."""
    n = 3_000_000
    env = dict(os.environ, MI355_BLAS1_NT=nt)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(n)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("R ")]
    assert len(lines) == 6, r.stdout
    for kind in ("mixed", "cancel"):
        a, b = DATA[kind](n, np.random.default_rng(n))
        m = models(a, b)
        beta, x3 = O.tree_orthogonalize(a, b, 1e-8)
        want_dev = [m["dot"], m["norm2"], m["rel_error"], beta]
        got = [ln for ln in lines if ln[1] == kind]
        for ln in got:
            vals = np.array([int(t) for t in ln[2:] if t != "host"], dtype=np.uint64).view(np.float64)
            want = want_dev[:3] if ln[2] == "host" else want_dev
            assert_same(vals[:len(want)], np.array(want), f"MI355_BLAS1_NT={nt} {kind} {ln[2] == 'host' and 'host' or 'device'}")


# -------------------------------------------------------------------------------------------------------- orthogonalize

@pytest.mark.parametrize("n", [2_000_001, 1_048_577, 524_289, 513, 2])
def test_orthogonalize_beta_and_update(n):
    """beta, and x3 elementwise from the model's beta: a workgroup of the update that finished beta from stale partials would
    leave a stretch of x3 with other bits.  Sizes run largest first on one stream."""
    for kind in ("mixed", "cancel"):
        b, x1 = DATA[kind](n, np.random.default_rng(n + 5))
        beta, want = O.tree_orthogonalize(b, x1, ALPHA)
        x3 = np.full(n, np.nan)
        assert_same(np.float64(mpk.orthogonalize(n, b, x1, x3, ALPHA)), np.float64(beta), f"host beta n={n} {kind}")
        assert_same(x3, want, f"host x3 n={n} {kind}")
        for db, dx1 in ((dev(b), dev(x1)), (odd_view(b), odd_view(x1))):
            dx3 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
            assert_same(np.float64(val(mpk.orthogonalize(n, db, dx1, dx3, ALPHA))), np.float64(beta), f"device beta n={n} {kind}")
            assert_same(dx3, want, f"device x3 n={n} {kind}")
        inplace = odd_view(x1)  # the in-place form (x3 == x1)
        assert_same(np.float64(val(mpk.orthogonalize(n, odd_view(b), inplace, inplace, ALPHA))), np.float64(beta))
        assert_same(inplace, want, f"in-place x3 n={n} {kind}")


@pytest.mark.parametrize("n", [1_048_577, 3001])
@pytest.mark.parametrize("m", [1, 2, 8])
def test_orthonormalize_against_basis(n, m):
    """Every dot and the final y, host and device forms; device basis rows at odd offsets of one buffer.  Two data sets: in a
    sum dominated by a few products two trees often agree (mixed data at m = 1), in a sum of many similar ones often not."""
    rng = np.random.default_rng(n + m)
    for kind in ("mixed", "normal"):
        if kind == "mixed":
            basis = np.stack([DATA["mixed"](n, rng)[0] for _ in range(m)])
            y0 = DATA["mixed"](n, rng)[1]
        else:
            basis, y0 = rng.standard_normal((m, n)), rng.standard_normal(n)
        _check_sweep(basis, y0, f"n={n} m={m} {kind}")


def _check_sweep(basis, y0, what):
    m, n = basis.shape
    y_want, dots_want = O.tree_mgs(basis, y0)
    yh = y0.copy()
    assert_same(mpk.orthonormalize_against_basis(list(basis), yh), dots_want, f"host dots {what}")
    assert_same(yh, y_want, f"host y {what}")
    buf = torch.full((m * (n + 1) + 1,), float("nan"), dtype=torch.float64, device="cuda")
    rows = []
    for j in range(m):  # n odd: every row starts at an odd offset
        rows.append(buf[1 + j * (n + 1):1 + j * (n + 1) + n])
        rows[-1].copy_(dev(basis[j]))
    for dy in (dev(y0), odd_view(y0)):
        dots = mpk.orthonormalize_against_basis(rows, dy)
        assert_same(dots, dots_want, f"device dots {what}")
        assert_same(dy, y_want, f"device y {what}")


# ------------------------------------------------------------------------------------------------ product with its dot

def _handle(name, n, monkeypatch):
    SS = {"MI355_SSTREAM": "1", "MI355_SSTREAM_MAX_PADDING": "1e9"}
    if name.startswith("ring"):
        kind = name.split("-")[1]
        p, c, v = synth.rows(kind, n)
        return p, c, v, mpk.csrmatrix(n, p, c, v).set_kernel("ring"), True
    if name == "stream":
        p, c, v = synth.rows("s15", n)
        return p, c, v, mpk.csrmatrix(n, p, c, v).set_kernel("stream"), False
    if name == "sstream":
        for k, e in SS.items():
            monkeypatch.setenv(k, e)
        p, c, v = synth.rows("s15", n, w=min(2000, max(8, n // 8)))
        return p, c, v, mpk.csrmatrix(n, p, c, v).set_kernel("sstream"), False
    if name == "relabelled":
        monkeypatch.setenv("MI355_REORDER", "1")
        p, c, v = synth.fe_matrix(14)
        p, c, v, _ = synth.permute_nodes(p, c, v, block=4)
        A = mpk.csrmatrix(len(p) - 1, p, c, v)
        assert A.perm()[0], "the scrambled numbering was relabelled"
        return p, c, v, A, False
    raise KeyError(name)


@pytest.mark.parametrize("name,n", [("ring-s15", 3_000), ("ring-s15", 300_000), ("ring-svar", 3_000), ("ring-svar", 300_000),
                                    ("stream", 300_000), ("sstream", 300_000), ("relabelled", None)])
def test_product_with_its_dot(name, n, monkeypatch):
    """beta of mi_spmv_dot_dev / mi_spmv_orthogonalize_dev against the tree the handle's launch takes: the ring epilogue's model
    on the layout the handle reports, or the stage-1 tree on (b, y).  x3 from the MODEL's beta."""
    p, c, v, A, fused = _handle(name, n, monkeypatch)
    n = A.n
    assert A.dot_in_epilogue() == fused, (name, A.kernel_name())
    x = synth.x_sin(0, n)
    rng = np.random.default_rng(n)
    yo = O.spmv(p, c, v, x)
    for kind in ("mixed", "cancel"):
        b = DATA["mixed"](n, rng)[0]
        if kind == "cancel":  # b chosen so that b . y cancels to ~1e-12 of sum |b_i y_i|
            h = n // 2
            b[h:2 * h] = -yo[:h] * (1 + 1e-12 * rng.standard_normal(h))
            b[:h] = yo[h:2 * h]
        if fused:
            layout = A.dot_epilogue_layout()
            assert layout["threads"] == 256 and int(np.sum(layout["block_rows"])) == n, layout["threads"]
            want = O.tree_ring_dot(layout, b, yo)
        else:
            with pytest.raises(mpk.MiError):
                A.dot_epilogue_layout()
            want = O.tree_dot(b, yo)
        y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        beta = mpk.SpMV_CSR_dot(y, dev(x), A, dev(b))
        assert_same(y, yo, f"{name} y")
        assert_same(np.float64(val(beta)), np.float64(want), f"{name} {kind} beta ({A.kernel_name()})")
        x1 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        x3 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        beta3 = mpk.SpMV_CSR_orthogonalize(x1, dev(x), A, dev(b), x3, ALPHA)
        assert_same(np.float64(val(beta3)), np.float64(want), f"{name} {kind} orthogonalize beta")
        assert_same(x1, yo, f"{name} x1")
        assert_same(x3, O.tree_ortho_update(ALPHA, want, b, yo), f"{name} {kind} x3")


# --------------------------------------------------------------------------------------------------------- Krylov basis

def _replay_krylov(p, c, v, v0, s):
    n = len(v0)
    V = np.zeros((s + 1, n))
    H = np.zeros((s, s + 2))
    nrm0 = O.tree_norm2(v0)
    V[0] = v0 / nrm0
    for k in range(s):
        w, dots = O.tree_mgs(V[:k + 1], O.spmv(p, c, v, V[k]))
        nr = O.tree_norm2(w)
        V[k + 1] = w / nr
        H[k, :k + 1] = dots
        H[k, k + 1] = nr
    return V, H, nrm0


@pytest.mark.parametrize("n", [20_001, 20_000])
def test_krylov_basis_bitwise_and_independent_of_ldv(n):
    """mi_krylov_basis_dev with orth=1: V and H from v0 alone (the oracle's product, the model's sweep and norm2, IEEE division),
    for ldv = n and ldv = n + 1 — one of the two leaves every other column only 8-byte aligned."""
    s = 5
    p, c, v = synth.rows("s15", n)
    A = mpk.csrmatrix(n, p, c, v)
    v0 = synth.x_sin(0, n)
    V_want, H_want, nrm_want = _replay_krylov(p, c, v, v0, s)
    V, H, nrm0 = mpk.BuildKrylovBasis(A, dev(v0), s, orth=True)
    assert_same(np.float64(val(nrm0)), np.float64(nrm_want), "||v0||")
    assert_same(V, V_want, f"V, ldv = n = {n}")
    assert_same(H, H_want, f"H, ldv = n = {n}")
    ldv = n + 1
    V2 = torch.full(((s + 1) * ldv,), float("nan"), dtype=torch.float64, device="cuda")
    coef = torch.zeros(s * (s + 2) + 1, dtype=torch.float64, device="cuda")
    dv0 = dev(v0)
    mpk.check(mpk.lib().mi_krylov_basis_dev(A.handle, s, ctypes.c_void_p(dv0.data_ptr()), ctypes.c_void_p(V2.data_ptr()), ldv, 1,
                                            ctypes.c_void_p(coef.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    V2h = V2.cpu().numpy()
    for k in range(s + 1):
        assert_same(V2h[k * ldv:k * ldv + n], V_want[k], f"column {k}, ldv = {ldv}")
    assert_same(coef[:s * (s + 2)].reshape(s, s + 2), H_want, f"H, ldv = {ldv}")
    assert_same(coef[s * (s + 2)], np.float64(nrm_want))


# ----------------------------------------------------------------------------------------------------------- distributed

@pytest.mark.parametrize("ranks", [2, 3])
def test_distributed_dot_and_orthogonalize(ranks):
    """mi_dist_dot / mi_dist_orthogonalize with the ranks on one card: the rank-order sum of every rank's model dot over its slice
    (mi_dist_rank_info), and x3 from that beta."""
    n = 200_003
    p, c, v = synth.rows("s15", n)
    D = mpk.DistMatrix(ranks, n, p, c, v)
    try:
        slices = [(r["row_start"], r["row_start"] + r["n_local"]) for r in D.info()["ranks"]]
        assert len(slices) == ranks and slices[0][0] == 0 and slices[-1][1] == n
        for kind in ("mixed", "cancel"):
            a, b = DATA[kind](n, np.random.default_rng(ranks + len(kind)))
            want = O.tree_rank_sum([O.tree_dot(a[s:e], b[s:e]) for s, e in slices])
            assert_same(np.float64(D.dot(a, b)), np.float64(want), f"dist dot, {ranks} ranks, {kind}")
            x3 = np.full(n, np.nan)
            beta = D.orthogonalize(a, b, x3, ALPHA)
            assert_same(np.float64(beta), np.float64(want), f"dist orthogonalize beta, {ranks} ranks, {kind}")
            assert_same(x3, O.tree_ortho_update(ALPHA, want, a, b), f"dist x3, {ranks} ranks, {kind}")
    finally:
        D.close()


# ------------------------------------------------------------------------------------------------------------------ shim

def test_shim_blas1_symbols():
    """norm2, rel_error, both orthogonalize forms (their dot) and orthonormalize_against_basis under the reference's names."""
    import shim
    if not os.path.exists(shim.SHIM):
        pytest.fail("libmpk_mi355.so not built")
    L = shim.lib()
    for n in (1001, 524_289):
        a, b = DATA["mixed"](n, np.random.default_rng(n))
        assert_same(np.float64(L.shim_norm2(n, a)), np.float64(O.tree_norm2(a)), f"norm2 n={n}")
        assert_same(np.float64(L.shim_rel_error(n, a, b)), np.float64(O.tree_rel_error(a, b)), f"rel_error n={n}")
        beta, want = O.tree_orthogonalize(a, b, ALPHA)
        assert_same(shim.orthogonalize3(a, b, ALPHA), want, f"orthogonalize (3-vector form) n={n}")
        assert_same(shim.orthogonalize_inplace(a, b, ALPHA), want, f"orthogonalize (in-place form) n={n}")
        basis = np.stack([DATA["mixed"](n, np.random.default_rng(n + j))[0] for j in range(3)])
        assert_same(shim.orthonormalize_against_basis(basis, b), O.tree_mgs(basis, b)[0], f"orthonormalize_against_basis n={n}")
