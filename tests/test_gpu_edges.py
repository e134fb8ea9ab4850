"""Every product path of the library in one table, held to the oracle's fma chain where callers break the two conditions the rest
of the GPU suite shares: values drawn from (-1, 1), and products on torch's default (legacy null) stream.

- The path table (PATHS): how each path is built, the environment that forces it, the product call, the oracle and the kernel it
  must report.  Every use of a row asserts the kernel that served it, so a silent fallback fails instead of testing nothing.
- IEEE values (CASES): non-finite x where rows look and where no row looks, stored zeros facing Inf, signed zeros and empty rows,
  subnormal products and partial sums, overflow whose class depends on the summation order.
- Stream order: a handle's first product on a fresh non-blocking stream right after create; the null stream idle when every
  create / set-kernel / host-refresh entry point returns; a device-side refresh on one stream and the product on another; one
  handle on two non-blocking streams at once; the one-launch k-step moved from one stream to another.
- Views that are only 8-byte aligned: bitwise results through whatever kernel takes them, or the documented refusal (MiError);
  never a write outside the view.

Comparison is bitwise (the sign of a zero and of an infinity included) except that a NaN matches any NaN: IEEE 754 does not say
which payload an fma propagates, and the CPU and the GPU need not agree."""
import ctypes

import numpy as np
import pytest
import torch

from navierstokes_amd import mpk, synth
from oracle import oracle as O
from test_oracle_vs_reference import IEEE_CASES as CASES

pytestmark = pytest.mark.gpu

def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nans(n):
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def host(t):
    return t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def assert_same(got, want, what=""):
    """Bitwise, except that any NaN matches any NaN (sign and payload free)."""
    got = np.ascontiguousarray(host(got), dtype=np.float64)
    want = np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    both_nan = np.isnan(got) & np.isnan(want)
    bad = np.nonzero((got.view(np.uint64) != want.view(np.uint64)) & ~both_nan)[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} entries differ, first at {bad[:5]}: "
                           f"{got[bad[:5]]} vs {want[bad[:5]]}")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    mpk.lib()
    yield


# ------------------------------------------------------------------------------------------------ base patterns (seeded, cached)

_BASES = {}


def base(name):
    """(ptrow, indcol, coef, block): block = 4 for node-block (FE) patterns, whose edits keep whole 4x4 blocks."""
    if name not in _BASES:
        if name == "s15":
            p, c, v = synth.rows("s15", 300_000, w=2000)
            _BASES[name] = (p, c, v, 1)
        elif name == "s15_small":
            p, c, v = synth.rows("s15", 70_001, w=900)
            _BASES[name] = (p, c, v, 1)
        elif name == "mesh62":
            p, c, v = synth.pressure_matrix(62)
            _BASES[name] = (p, c, v, 1)
        elif name == "fe14":
            p, c, v = synth.fe_matrix(14)
            _BASES[name] = (p, c, v, 4)
        elif name == "fe14_scrambled":
            p, c, v = synth.fe_matrix(14)
            p, c, v, _ = synth.permute_nodes(p, c, v, block=4)
            _BASES[name] = (p, c, v, 4)
        else:
            raise KeyError(name)
    return _BASES[name]


# ------------------------------------------------------------------------------------------------------------------ path table

def _sell_form(B):
    b, f = ctypes.c_int(), ctypes.c_int()
    mpk.check(mpk.lib().mi_bcsr4_sell_info(B.handle, ctypes.byref(b), ctypes.byref(f), None, None, None))
    return b.value, f.value


class Path:
    """One product path.  make(p, c, v) -> handle; run(H, x_dev, outs) queues the product on the current stream;
    want(p, c, v, x) -> list of expected arrays; check(H) asserts the kernel that serves the handle."""
    kind = "spmv"    # "spmv" (one y), "spmk" (k outputs), "spmm" (s columns), "dot" (y and beta), "dist" (host vectors)
    k = 1
    ny_extra = 0     # y is longer than n (row-mapped pieces): the rows outside the map keep their sentinel

    def __init__(self, pid, pattern, env=None):
        self.id, self.pattern, self.env = pid, pattern, dict(env or {})

    def n_out(self, n):
        return n + self.ny_extra

    def want(self, p, c, v, x):
        return [O.spmv(p, c, v, x)]

    def pick(self, outs):
        return [host(o) for o in outs]

    def update(self, H, p, c, v):
        """New values from a device array, queued on the current stream."""
        H.update_values(dev(v))


class Csr(Path):
    def __init__(self, pid, pattern, kernel, prefix, env=None, extra=None):
        super().__init__(pid, pattern, env)
        self.kernel, self.prefix, self.extra = kernel, prefix, extra

    def make(self, p, c, v):
        A = mpk.csrmatrix(len(p) - 1, p, c, v)
        if self.kernel != "auto":
            A.set_kernel(self.kernel)
        _ = A.handle
        return A

    def check(self, A):
        name = A.kernel_name()
        assert name.startswith(self.prefix), (self.id, name)
        if self.extra:
            self.extra(A)

    def run(self, A, x, outs):
        mpk.SpMV_CSR(outs[0], x, A)


def _sstream_form(form):
    def check(A):
        assert A.sstream_info()["form"] == form, A.sstream_info()
    return check


def _ring_config(cfg):
    def check(A):
        assert A.ring_info()[0] == cfg, A.ring_info()
    return check


class CsrBlocked(Csr):
    """The blocked copy of an FE matrix, through the CSR API."""

    def __init__(self, pid, form):
        env = {"MI355_BCSR_SELL": "0"} if form is None else {"MI355_BCSR_SELL": "1", "MI355_BCSR_SELL_FORM": str(form)}
        super().__init__(pid, "fe14", "bcsr4", "spmv_bcsr4<2>" if form is None else "spmv_bcsr4_sell<", env)


class BcsrApi(Path):
    def __init__(self, pid, form):
        super().__init__(pid, "fe14", {"MI355_BCSR_SELL": "1", "MI355_BCSR_SELL_FORM": str(form)})
        self.form = form

    def make(self, p, c, v):
        n = len(p) - 1
        bp, bc, bv = synth.csr_to_bcsr4(p, c, v)
        B = mpk.bcsr4x4_matrix(n // 4, bp, bc, bv, nbcols=n // 4)
        _ = B.handle
        return B

    def update(self, B, p, c, v):
        B.update_values(dev(synth.csr_to_bcsr4(p, c, v)[2]))  # the handle takes its values in block order

    def check(self, B):
        assert _sell_form(B) == (1, self.form), (self.id, _sell_form(B))

    def run(self, B, x, outs):
        mpk.SpMV_BCSR(outs[0], x, B)

    def want(self, p, c, v, x):
        bp, bc, bv = synth.csr_to_bcsr4(p, c, v)
        return [O.spmv_bcsr4(bp, bc, bv, x)]


class Mapped(Csr):
    """A partition piece: row r writes y[rowmap[r]]; y is n + 9 long and the rows outside the map keep their NaN sentinel."""
    ny_extra = 9

    def __init__(self, pid, how, kernel, prefix, env=None):
        super().__init__(pid, "s15_small", kernel, prefix, env)
        self.how = how

    def rowmap(self, n):
        if self.how == "scattered":
            return np.random.default_rng(9).permutation(n + 9)[:n].astype(np.int32)
        return (np.arange(n) + 5).astype(np.int32)  # odd offset: the rows' pairs are no longer 16-byte aligned

    def make(self, p, c, v):
        n = len(p) - 1
        A = mpk.csrmatrix(n, p, c, v, rowmap=self.rowmap(n))
        A.set_kernel(self.kernel)
        _ = A.handle
        return A

    def pick(self, outs):
        got = host(outs[0])
        n = len(got) - self.ny_extra
        rm = self.rowmap(n)
        rest = np.ones(len(got), bool)
        rest[rm] = False
        assert np.isnan(got[rest]).all(), f"{self.id}: wrote rows outside the map"
        return [got[rm]]


class Relabelled(Csr):
    """A scrambled (mesher-like) numbering that mi_csr_create relabels (forced); checked in the caller's numbering."""

    def __init__(self, pid):
        super().__init__(pid, "fe14_scrambled", "auto", "", {"MI355_REORDER": "1"})

    def check(self, A):
        assert A.reorder_info()["reordered"] and A.kernel_name(), (A.reorder_info(), A.kernel_name())


class Spmk(Csr):
    kind = "spmk"

    def __init__(self, pid, k, fused):
        super().__init__(pid, "s15", "ring", "spmv_csr_ring<", {"MI355_SPMK_FUSED": "1" if fused else "0"})
        self.k, self.fused = k, fused

    def check(self, A):
        super().check(A)
        info = A.spmk_info(self.k)
        assert info["one_launch"] == self.fused and (info["eligible"] or not self.fused), (self.id, info)

    def run(self, A, x, outs):
        mpk.SpMkV(outs, x, A)

    def want(self, p, c, v, x):
        return list(O.spmk_chain(self.k, p, c, v, x))


S_COLS = 3


def _columns(x, s=S_COLS):
    """s columns of X: the case's x, and others that move its special entries to other rows."""
    return np.stack([x, np.roll(x, 4) * 0.5, -np.roll(x, -4), np.roll(x, 8) * -0.25][:s])


class Spmm(Path):
    kind = "spmm"

    def __init__(self, pid, api, form=None, s=S_COLS):
        """form: a tile form of the multi-vector product forced on (MI355_SPMM_TILE), which check() then requires; s: the columns."""
        super().__init__(pid, "fe14", {"MI355_BCSR_SELL": "1", "MI355_BCSR_SELL_FORM": "0"})
        if form is not None:
            self.env["MI355_SPMM_TILE"] = str(form)
        self.api, self.form, self.s = api, form, s

    def make(self, p, c, v):
        n = len(p) - 1
        if self.api == "bcsr":
            bp, bc, bv = synth.csr_to_bcsr4(p, c, v)
            H = mpk.bcsr4x4_matrix(n // 4, bp, bc, bv, nbcols=n // 4)
        else:
            H = mpk.csrmatrix(n, p, c, v).set_kernel("bcsr4")
        _ = H.handle
        return H

    def check(self, H):
        if self.api == "bcsr":
            tb, form = ctypes.c_int(), ctypes.c_int()
            mpk.check(mpk.lib().mi_bcsr4_spmm_info(H.handle, self.s, ctypes.byref(tb), ctypes.byref(form), None, None))
            assert form.value >= 0, form.value
            if self.form is not None:  # asked after a product: the lists are built at the first one
                assert (tb.value, form.value) == (1, self.form), (self.id, tb.value, form.value)
        else:  # the multi-vector product of a CSR handle reads its blocked copy
            assert H.kernel_name().startswith("spmv_bcsr4"), H.kernel_name()

    def run(self, H, X, outs):
        mpk.MatMatMult_SeqBAIJ_4(H, X, outs[0], "chain")

    def run_ld(self, H, X_ptr, ldx, Y_ptr, ldy):
        """The C-ABI call with explicit leading dimensions (the torch wrapper passes contiguous (s, n) tensors only)."""
        L, vp = mpk.lib(), ctypes.c_void_p
        if self.api == "bcsr":
            mpk.check(L.mi_bcsr4_spmm_dev(H.handle, self.s, vp(X_ptr), ldx, vp(Y_ptr), ldy, mpk.ARITH["chain"], mpk._stream_ptr()))
        else:
            mpk.check(L.mi_spmm_dev(H.handle, self.s, vp(X_ptr), ldx, vp(Y_ptr), ldy, mpk._stream_ptr()))

    def want(self, p, c, v, x):
        return [np.stack([O.spmv(p, c, v, col) for col in _columns(x, self.s)])]


class Dot(Csr):
    kind = "dot"

    def __init__(self, pid):
        super().__init__(pid, "s15", "ring", "spmv_csr_ring<")

    def check(self, A):
        super().check(A)
        assert A.dot_in_epilogue(), (A.kernel_name(), A.ring_shape_info())

    def run(self, A, x, outs):
        outs[1].copy_(mpk.SpMV_CSR_dot(outs[0], x, A, self.b))

    def b_for(self, n):
        return np.cos(0.002 * np.arange(n))


class Dist(Path):
    kind = "dist"

    def __init__(self, pid):
        super().__init__(pid, "s15_small", {"MI355_DIST_EXCHANGE": "event"})

    def make(self, p, c, v):
        return mpk.DistMatrix(2, len(p) - 1, p, c, v)

    def check(self, D):
        info = D.info()
        assert info["nranks"] == 2 and info["exchange"].split("-")[0] == "event", info

    def run(self, D, x, outs):
        D.spmv(outs[0], x)


SS = {"MI355_SSTREAM": "1", "MI355_SSTREAM_MAX_PADDING": "1e9"}
PATHS = (
    [Csr("stream", "s15", "stream", "spmv_csr_stream<"),
     Csr("ring-cfg4", "s15", "ring", "spmv_csr_ring<", {"MI355_RING_CONFIG": "4"}, _ring_config(4)),
     Csr("ring-cfg2", "s15", "ring", "spmv_csr_ring<", {"MI355_RING_CONFIG": "2"}, _ring_config(2)),
     Csr("rowpar", "s15", "rowpar", "spmv_csr_rowpar"),
     Csr("tile", "s15", "tile", "spmv_csr_tile<"),
     Csr("mring", "s15", "mring", "spmv_csr_mring<"),
     Csr("auto", "s15", "auto", "spmv_")]
    + [Csr(f"sstream-form{f}", "s15", "sstream", "spmv_sstream<", dict(SS, MI355_SSTREAM_FORM=str(f)), _sstream_form(f)) for f in range(4)]
    + [Csr("sstream-cut-ring", "mesh62", "sstream", "spmv_sstream_mw<", dict(SS, MI355_SSTREAM_FORM="0"), _sstream_form(0)),
       CsrBlocked("csr-bcsr4-quad", None)]
    + [CsrBlocked(f"csr-bcsr4-sell{f}", f) for f in range(4)]
    + [BcsrApi(f"bcsr-api-sell{f}", f) for f in (0, 3)]
    + [Mapped("mapped-scattered", "scattered", "sstream", "spmv_sstream<", SS),
       Mapped("mapped-odd-offset", "offset", "ring", "spmv_csr_ring<"),
       Relabelled("relabelled")]
    + [Spmk(f"spmk{k}-one-launch", k, True) for k in (2, 3, 4)]
    + [Spmk("spmk3-k-launches", 3, False),
       Spmm("spmm-bcsr", "bcsr"), Spmm("spmm-csr", "csr"),
       Spmm("spmm-bcsr-tile", "bcsr", form=1), Spmm("spmm-bcsr-otile", "bcsr", form=2, s=4), Spmm("spmm-bcsr-otile-nt", "bcsr", form=3, s=4),
       Dot("dot-epilogue"),
       Dist("dist-n2")]
)
PATH_IDS = [P.id for P in PATHS]
SINGLE = [P for P in PATHS if P.kind in ("spmv", "dot")]


def _force(P, monkeypatch):
    for k, val in P.env.items():
        monkeypatch.setenv(k, val)


def _outputs(P, n):
    """Fresh NaN-filled device outputs of the path (or host arrays for the host-vector API)."""
    if P.kind == "dist":
        return [np.full(n, np.nan)]
    if P.kind == "spmk":
        return [nans(n) for _ in range(P.k)]
    if P.kind == "spmm":
        return [torch.full((P.s, n), float("nan"), dtype=torch.float64, device="cuda")]
    if P.kind == "dot":
        return [nans(n), nans(1)]
    return [nans(P.n_out(n))]


def _x_arg(P, x):
    if P.kind == "dist":
        return x
    if P.kind == "spmm":
        return dev(_columns(x, P.s))
    return dev(x)


def _run_and_check(P, H, p, c, v, x, what):
    n = len(p) - 1
    outs = _outputs(P, n)
    if P.kind == "dot":
        P.b = dev(P.b_for(n))
    P.run(H, _x_arg(P, x), outs)
    torch.cuda.synchronize()
    P.check(H)
    want = P.want(p, c, v, x)
    got = P.pick(outs[:len(want)])
    for q, (g, w) in enumerate(zip(got, want)):
        assert_same(g, w, f"{P.id} [{what}] output {q}")
    if P.kind == "dot":
        beta, ref = float(outs[1].cpu()), O.dot(P.b_for(n), want[0])
        assert _cls(beta) == _cls(ref), (P.id, what, beta, ref)
    return got


# ----------------------------------------------------------------------------------------------------------- IEEE value cases

@pytest.mark.parametrize("path", PATHS, ids=PATH_IDS)
def test_ieee_values_on_every_path(path, monkeypatch):
    """Each IEEE case on each path, bitwise against the oracle (NaN matches NaN), plus what the case pins by itself."""
    _force(path, monkeypatch)
    p0, c0, _, block = base(path.pattern)
    for ci, (name, make_case) in enumerate(CASES.items()):
        rng = np.random.default_rng(1000 + ci)
        p, c, v, x, pins = make_case(p0, c0, block, rng)
        H = path.make(p, c, v)
        try:
            got = _run_and_check(path, H, p, c, v, x, name)
        finally:
            H.close()
        y = got[0][0] if path.kind == "spmm" else got[0]
        if pins.get("finite"):
            assert np.isfinite(y).all(), f"{path.id} [{name}]: an unreferenced NaN / Inf reached y"
        if "plus_zero" in pins:
            z = y[pins["plus_zero"]]
            assert (z.view(np.uint64) == 0).all(), f"{path.id} [{name}]: rows of -0.0 products / empty rows are not +0.0"
        if pins.get("subnormal"):
            assert (np.abs(y[y != 0]) < np.finfo(np.float64).tiny).any(), f"{path.id} [{name}]: no subnormal result"


# ---------------------------------------------------------------------------------------------------- 8-byte aligned views

@pytest.mark.parametrize("path", [P for P in PATHS if P.kind != "dist"], ids=[P.id for P in PATHS if P.kind != "dist"])
def test_views_that_are_only_8_byte_aligned(path, monkeypatch):
    """x alone and y alone as views one element into a larger tensor (data_ptr % 16 == 8): bitwise, or MiError where the C-ABI
    documents a refusal.  NaN sentinels on both sides of y must survive.  k-step: the outputs; multi-vector: an odd leading dimension."""
    _force(path, monkeypatch)
    p, c, v, _ = base(path.pattern)
    n = len(p) - 1
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, n)
    H = path.make(p, c, v)
    want = path.want(p, c, v, x)
    try:
        if path.kind == "spmm":
            ld = n + 1  # odd: every other column starts 8 bytes off a 16-byte boundary
            S = path.s
            X = _columns(x, S)
            for odd in ("X", "Y"):
                bx = nans(S * ld + 2)
                by = nans(S * ld + 2)
                if odd == "X":
                    bx[:S * ld].view(S, ld)[:, :n] = dev(X)
                    xp, ldx, yp, ldy = bx.data_ptr(), ld, by.data_ptr() + 8, n
                else:
                    bx[:S * n] = dev(X.reshape(-1))
                    xp, ldx, yp, ldy = bx.data_ptr(), n, by.data_ptr() + 8, ld
                try:
                    path.run_ld(H, xp, ldx, yp, ldy)
                    torch.cuda.synchronize()
                except mpk.MiError:
                    assert path.api == "bcsr" and odd == "X", f"{path.id}: refused an odd leading dimension of {odd}"
                    continue
                path.check(H)
                b = by.cpu().numpy()
                Y = np.stack([b[1 + j * ldy:1 + j * ldy + n] for j in range(S)])
                assert_same(Y, want[0], f"{path.id} odd leading dimension of {odd}")
                written = np.zeros(len(b), bool)
                for j in range(S):
                    written[1 + j * ldy:1 + j * ldy + n] = True
                assert np.isnan(b[~written]).all(), f"{path.id}: wrote outside the columns of Y"
            return
        ny = path.n_out(n)
        for which in ("x", "y"):
            bx = nans(n + 2)
            if which == "x":
                bx[1:n + 1] = dev(x)
                xv = bx[1:n + 1]
                assert xv.data_ptr() % 16 == 8
            else:
                xv = dev(x)
            outs, bufs = [], []
            for _ in range(path.k if path.kind == "spmk" else 1):
                if which == "y":
                    b = nans(ny + 2)
                    bufs.append(b)
                    outs.append(b[1:ny + 1])
                    assert outs[-1].data_ptr() % 16 == 8
                else:
                    outs.append(nans(ny))
            if path.kind == "dot":
                path.b = dev(path.b_for(n))
                outs.append(nans(1))
            try:
                path.run(H, xv, outs)
                torch.cuda.synchronize()
            except mpk.MiError:
                assert isinstance(path, BcsrApi) and which == "x", f"{path.id}: refused an 8-byte aligned {which}"
                continue
            path.check(H)
            got = path.pick(outs[:len(want)])
            for q, (g, w) in enumerate(zip(got, want)):
                assert_same(g, w, f"{path.id}, 8-byte aligned {which}, output {q}")
            for b in bufs:
                bh = b.cpu().numpy()
                assert np.isnan(bh[0]) and np.isnan(bh[-1]), f"{path.id}: wrote outside the y view"
            assert np.isnan(bx[0].item()) and np.isnan(bx[-1].item())
    finally:
        H.close()


# ------------------------------------------------------------------------------------------------------------- stream order

_HIP = None


def stream_flags(s):
    global _HIP
    if _HIP is None:
        _HIP = ctypes.CDLL("libamdhip64.so")
        _HIP.hipStreamGetFlags.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint)]
    f = ctypes.c_uint()
    assert _HIP.hipStreamGetFlags(ctypes.c_void_p(s.cuda_stream), ctypes.byref(f)) == 0
    return f.value


HIP_STREAM_NON_BLOCKING = 0x01


def _first_product_on_a_fresh_stream(make, check, prod, want, what):
    """Create (touching the handle), ask whether the null stream is idle, then with no synchronisation the first product on a new
    non-blocking stream.  Returns whether the null stream was idle when create returned."""
    torch.cuda.synchronize()
    H = make()
    idle = torch.cuda.default_stream().query()
    check(H)
    s = torch.cuda.Stream()
    assert stream_flags(s) & HIP_STREAM_NON_BLOCKING, "the side stream must be non-blocking, or this proves nothing"
    with torch.cuda.stream(s):
        y = prod(H)
    torch.cuda.synchronize()
    assert_same(y, want(), what)
    H.close()
    return idle


@pytest.mark.parametrize("which", ["sstream-c4", "bcsr-sell-fe68", "cut-ring-mesh100"])
def test_first_product_on_a_fresh_non_blocking_stream(which, monkeypatch):
    """The headline-sized fills (sliced values of spmv_sstream, of spmv_bcsr4_sell) take hundreds of microseconds; with the measurement
    skipped (forced kernel) nothing used to wait for them.  The product on a fresh non-blocking stream must see complete values, and
    create must leave the null stream idle.  Coefficients are seeded here, so a recycled buffer cannot hold the right values by chance."""
    rng = np.random.default_rng(77)
    if which == "bcsr-sell-fe68":
        monkeypatch.setenv("MI355_BCSR_SELL", "1")
        monkeypatch.setenv("MI355_BCSR_SELL_FORM", "0")
        p, c, _ = synth.fe_matrix(68)
        n = len(p) - 1
        bp, bc, _ = synth.csr_to_bcsr4(p, c, np.zeros(len(c)))
        del p, c
        bv = rng.uniform(-1, 1, 16 * len(bc))
        x = rng.uniform(-1, 1, n)

        def make():
            B = mpk.bcsr4x4_matrix(n // 4, bp, bc, bv, nbcols=n // 4)
            _ = B.handle
            return B

        def check(B):
            assert _sell_form(B) == (1, 0), _sell_form(B)

        def prod(B):
            y = torch.empty(n, dtype=torch.float64, device="cuda")
            mpk.SpMV_BCSR(y, dev(x), B)
            return y

        want = lambda: O.spmv_bcsr4(bp, bc, bv, x)
    else:
        monkeypatch.setenv("MI355_SPMV_KERNEL", "sstream")
        monkeypatch.setenv("MI355_SSTREAM", "1")
        p, c, _ = synth.rows("s15", 5_000_000) if which == "sstream-c4" else synth.pressure_matrix(100)
        n = len(p) - 1
        v = rng.uniform(-1, 1, len(c))
        x = rng.uniform(-1, 1, n)
        prefix = "spmv_sstream<" if which == "sstream-c4" else "spmv_sstream_mw<"

        def make():
            A = mpk.csrmatrix(n, p, c, v)
            _ = A.handle
            return A

        def check(A):
            assert A.kernel_name().startswith(prefix), A.kernel_name()

        def prod(A):
            y = torch.empty(n, dtype=torch.float64, device="cuda")
            mpk.SpMV_CSR(y, dev(x), A)
            return y

        want = lambda: O.spmv(p, c, v, x)
    idle = _first_product_on_a_fresh_stream(make, check, prod, want, which)
    assert idle, f"{which}: create returned with work still queued on the null stream"


def _idle(what):
    assert torch.cuda.default_stream().query(), f"{what} returned with work still queued on the null stream"


def test_entry_points_return_with_the_null_stream_idle(monkeypatch):
    """Deterministic companion of the fresh-stream case: right after each create, set-kernel and host-array refresh returns, the null
    stream has nothing left to do.  (Forced kernels: the create-time measurement, whose events used to drain the fills, is skipped.)"""
    monkeypatch.setenv("MI355_SSTREAM", "1")
    monkeypatch.setenv("MI355_BCSR_SELL", "1")
    monkeypatch.setenv("MI355_BCSR_SELL_FORM", "0")
    p, c, v = synth.rows("s15", 300_000, w=2000)
    n = len(p) - 1
    for env, what in (({"MI355_SPMV_KERNEL": "sstream"}, "mi_csr_create (forced sstream)"), ({"MI355_SPMV_AUTOTUNE": "0"}, "mi_csr_create (no measurement)"),
                      ({}, "mi_csr_create (measured)")):
        with monkeypatch.context() as m:
            for k, val in env.items():
                m.setenv(k, val)
            torch.cuda.synchronize()
            A = mpk.csrmatrix(n, p, c, v)
            _ = A.handle
            _idle(what)
            A.update_values(v * 0.5)
            _idle("mi_csr_update_values (host array)")
            for kernel in ("tile", "mring", "sstream", "ring"):
                A.set_kernel(kernel)
                _idle(f"mi_csr_set_kernel({kernel})")
            A.close()
    monkeypatch.setenv("MI355_SPMV_KERNEL", "sstream")
    torch.cuda.synchronize()
    A = mpk.csrmatrix(n, p, c, v, rowmap=(np.arange(n) + 6).astype(np.int32))
    _ = A.handle
    _idle("mi_csr_create_mapped (forced sstream)")
    A.close()
    monkeypatch.delenv("MI355_SPMV_KERNEL")
    pf, cf, vf = synth.fe_matrix(20)
    ps, cs, vs, _ = synth.permute_nodes(pf, cf, vf, block=4)
    nf = len(pf) - 1
    with monkeypatch.context() as m:
        m.setenv("MI355_REORDER", "1")
        torch.cuda.synchronize()
        A = mpk.csrmatrix(nf, ps, cs, vs)
        _ = A.handle
        _idle("mi_csr_create (relabelled twin)")
        assert A.reorder_info()["reordered"]
        A.update_values(vs * 0.5)
        _idle("mi_csr_update_values (relabelled, host array)")
        A.close()
    with monkeypatch.context() as m:
        m.setenv("MI355_SPMV_KERNEL", "bcsr4")
        torch.cuda.synchronize()
        A = mpk.csrmatrix(nf, pf, cf, vf)
        _ = A.handle
        _idle("mi_csr_create (forced bcsr4, sliced blocked copy)")
        assert "sell" in A.kernel_name(), A.kernel_name()
        A.close()
    bp, bc, bv = synth.csr_to_bcsr4(pf, cf, vf)
    torch.cuda.synchronize()
    B = mpk.bcsr4x4_matrix(nf // 4, bp, bc, bv, nbcols=nf // 4)
    _ = B.handle
    _idle("mi_bcsr4_create (forced sliced form)")
    assert _sell_form(B) == (1, 0)
    B.update_values(bv * 0.5)
    _idle("mi_bcsr4_update_values (host array)")
    B.close()


@pytest.mark.parametrize("path", [P for P in PATHS if P.kind in ("spmv", "dot", "spmk")], ids=[P.id for P in PATHS if P.kind in ("spmv", "dot", "spmk")])
def test_device_update_on_one_stream_product_on_another(path, monkeypatch):
    """update_values(dev(v2)) on s1, s2.wait_stream(s1), the product on s2: bitwise A_new x — every part of a value refresh is queued
    on the caller's stream."""
    _force(path, monkeypatch)
    p, c, v, _ = base(path.pattern)
    n = len(p) - 1
    x = np.random.default_rng(4).uniform(-1, 1, n)
    v2 = v * np.cos(np.arange(len(v)))
    H = path.make(p, c, v)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = _outputs(path, n)
    if path.kind == "dot":
        path.b = dev(path.b_for(n))
    xd = dev(x)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        path.update(H, p, c, v2)
    s2.wait_stream(s1)
    with torch.cuda.stream(s2):
        path.run(H, xd, outs)
    torch.cuda.synchronize()
    path.check(H)
    want = path.want(p, c, v2, x)
    for q, (g, w) in enumerate(zip(path.pick(outs[:len(want)]), want)):
        assert_same(g, w, f"{path.id}: refresh on s1, product on s2, output {q}")
    H.close()


@pytest.mark.parametrize("path", SINGLE, ids=[P.id for P in SINGLE])
def test_one_handle_on_two_non_blocking_streams(path, monkeypatch):
    """Products with different x queued on two non-blocking streams before waiting on either: both bitwise (scratch per stream —
    the relabelled gather buffer, the dot's reduction workspace)."""
    _force(path, monkeypatch)
    p, c, v, _ = base(path.pattern)
    n = len(p) - 1
    rng = np.random.default_rng(5)
    xs = [rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)]
    H = path.make(p, c, v)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    assert all(stream_flags(s) & HIP_STREAM_NON_BLOCKING for s in streams)
    xd = [dev(x) for x in xs]
    outs = [_outputs(path, n) for _ in streams]
    b = path.b_for(n) if path.kind == "dot" else None
    if b is not None:
        path.b = dev(b)
    torch.cuda.synchronize()
    for _ in range(3):
        for s, x, o in zip(streams, xd, outs):
            with torch.cuda.stream(s):
                path.run(H, x, o)
    torch.cuda.synchronize()
    path.check(H)
    for k, (x, o) in enumerate(zip(xs, outs)):
        want = path.want(p, c, v, x)
        assert_same(path.pick(o[:1])[0], want[0], f"{path.id}: stream {k}")
        if b is not None:
            ref = O.dot(b, want[0])
            assert abs(float(o[1].cpu()) - ref) <= 1e-13 * float(np.abs(b * want[0]).sum()), (path.id, k)
    H.close()


def test_one_launch_k_step_moved_between_streams(monkeypatch):
    """The one-launch k-step on s1, then (s2 waits for s1) on s2: both bitwise; the flags it counts on are per handle, not per stream."""
    P = Spmk("spmk4", 4, True)
    _force(P, monkeypatch)
    p, c, v, _ = base(P.pattern)
    n = len(p) - 1
    rng = np.random.default_rng(6)
    xs = [rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)]
    A = P.make(p, c, v)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    o1, o2 = _outputs(P, n), _outputs(P, n)
    x1, x2 = dev(xs[0]), dev(xs[1])
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        P.run(A, x1, o1)
    s2.wait_stream(s1)
    with torch.cuda.stream(s2):
        P.run(A, x2, o2)
    torch.cuda.synchronize()
    P.check(A)
    for x, o, tag in ((xs[0], o1, "s1"), (xs[1], o2, "s2")):
        for q, (g, w) in enumerate(zip(P.pick(o), P.want(p, c, v, x))):
            assert_same(g, w, f"one-launch k-step on {tag}, power {q + 1}")
    A.close()


# --------------------------------------------------------------------------------------------------------------- reductions

def _cls(a):
    return "nan" if np.isnan(a) else "+inf" if a == np.inf else "-inf" if a == -np.inf else "finite"


def test_reductions_keep_the_class_of_their_result():
    """dot, norm2 and rel_error on inputs whose class (NaN, +-Inf, finite) does not depend on the summation order: one Inf, one NaN,
    all entries huge and of one sign (norm2 overflows), all tiny (norm2 underflows to 0).  Finite results within test_blas1's bounds."""
    rng = np.random.default_rng(12)
    for n in (3, 513, 100_003):
        base_a = rng.uniform(0.5, 1, n)
        base_b = rng.uniform(0.5, 1, n)
        cases = []
        a = base_a.copy(); a[n // 2] = np.inf
        cases.append(("one inf", a, base_b))
        a = base_a.copy(); a[n // 3] = np.nan
        cases.append(("one nan", a, base_b))
        cases.append(("huge", base_a * 1e200, base_b * 1e200))
        cases.append(("tiny", base_a * 1e-200, base_b * 1e-200))
        for what, a, b in cases:
            for form in ("host", "device"):
                arg = (lambda t: t) if form == "host" else dev
                out = lambda r: float(r.cpu()) if torch.is_tensor(r) else float(r)
                d, want = out(mpk.dot(arg(a), arg(b))), O.dot(a, b)
                assert _cls(d) == _cls(want), (n, what, form, "dot", d, want)
                if _cls(want) == "finite":
                    assert abs(d - want) <= 1e-13 * float(np.abs(a * b).sum()), (n, what, form, d, want)
                nm, want = out(mpk.norm2(arg(a))), O.norm2(a)
                assert _cls(nm) == _cls(want), (n, what, form, "norm2", nm, want)
                if _cls(want) == "finite":
                    assert abs(nm - want) <= 1e-14 * want, (n, what, form, nm, want)
                t = b if what in ("one inf", "one nan") else a * (1 + 1e-9 * rng.standard_normal(n))
                r, want = out(mpk.rel_error(arg(a), arg(t))), O.rel_error(a, t)
                assert _cls(r) == _cls(want), (n, what, form, "rel_error", r, want)
                if _cls(want) == "finite" and want > 0:
                    assert abs(r - want) <= 1e-9 * want + 1e-25, (n, what, form, r, want)
