"""The multi-vector product's tile forms (spmm_tile.hpp: form 1 spmm_bcsr4_tile, forms 2 / 3 spmm_bcsr4_otile) at every limit of their
plan (spmm_tile_plan.hpp), on the patterns of tests/spmm_tile_cases.py; the plan itself is held to its invariants in
tests/test_spmm_tile_plan.py.

The oracle is one throughout: per column O.spmv_bcsr4 for "chain" and O.spmv_bcsr4_blockacc for "blockacc", compared bit for bit (a NaN
matches any NaN: test_gpu_edges.assert_same).  Y is pre-filled with NaN, its leading dimension is 4 nbrows + 6, and everything behind a
column must still be NaN afterwards.  Every product is followed by mi_bcsr4_spmm_info: the form in use must be the forced one wherever
the rule restated in spmm_tile_cases.expected_form allows it (4 096 blocks, the column count, umax (4 s + 2) 8 <= 160 KiB) and 0
elsewhere, and longest_list must be the probe's umax — so no case passes through a fallback unnoticed.

  limits         every pattern, forms 1-3, both associations, twice per handle: form 1 at s = 1-4, forms 2 / 3 at s = 2, 4, 6, 8; on `grid`
                 also s = 9, 11, 16 (batches of eight and a remainder); `grid` and `components` also under the small list caps
  LDS boundary   each long:L on one handle through all twelve (form, s) pairs: the pairs that fit run the tile (launches of up to
                 163 840 bytes of dynamic LDS), the others form 0
  block-row map  `grid` as a relabelled CSR handle (mi_spmm_dev; the tile stores through browmap)
  IEEE values    the six builders of test_oracle_vs_reference.IEEE_CASES on `grid` and `empty`, forms 1-3 at four columns
  streams        first product on a fresh non-blocking stream; one handle on two streams; a value refresh and the product on one stream
  capture        a captured product replayed with a changed X and after a device-side value refresh, whatever form was chosen

Wall time of the file on an MI355X: 4 s (78 tests)."""
import ctypes

import numpy as np
import pytest
import torch

import spmm_tile_cases as TC
from navierstokes_amd import mpk, synth
from oracle import oracle as O
from test_gpu_edges import HIP_STREAM_NON_BLOCKING, assert_same, stream_flags
from test_oracle_vs_reference import IEEE_CASES

pytestmark = pytest.mark.gpu

ORACLE = {"chain": O.spmv_bcsr4, "blockacc": O.spmv_bcsr4_blockacc}
FORM_COLUMNS = {1: (1, 2, 3, 4), 2: (2, 4, 6, 8), 3: (2, 4, 6, 8)}
PAD = 6   # doubles of Y behind every column


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    mpk.lib()
    yield


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Handle:
    """mi_bcsr4_create on a case's arrays as they are (mpk.bcsr4x4_matrix widens nbcols to nbrows, which rect_tall must not be)."""

    def __init__(self, C, bv=None):
        self.C = C
        self.bv = np.ascontiguousarray(C.bv if bv is None else bv)
        h = ctypes.c_void_p()
        mpk.check(mpk.lib().mi_bcsr4_create(C.nbrows, C.nbcols, C.bp.ctypes.data, C.bc.ctypes.data, self.bv.ctypes.data, ctypes.byref(h)))
        self.h = h

    def info(self, s):
        tb, form, ll = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
        mpk.check(mpk.lib().mi_bcsr4_spmm_info(self.h, s, ctypes.byref(tb), ctypes.byref(form), ctypes.byref(ll), None))
        return tb.value, form.value, ll.value

    def spmm(self, Xd, s, Yd, arith):
        """s columns of Xd (rows of a contiguous (S, 4 nbcols) tensor) into Yd (flat; column j at j * ldy), on torch's current stream."""
        ldy = 4 * self.C.nbrows + PAD
        assert Xd.shape[1] == 4 * self.C.nbcols and Xd.shape[0] >= s and Yd.numel() >= s * ldy
        mpk.check(mpk.lib().mi_bcsr4_spmm_dev(self.h, s, ctypes.c_void_p(Xd.data_ptr()), Xd.shape[1], ctypes.c_void_p(Yd.data_ptr()), ldy,
                                              mpk.ARITH[arith], mpk._stream_ptr()))

    def update_dev(self, vd):
        mpk.check(mpk.lib().mi_bcsr4_update_values_dev(self.h, ctypes.c_void_p(vd.data_ptr()), mpk._stream_ptr()))

    def close(self):
        if self.h is not None:
            mpk.lib().mi_bcsr4_destroy(self.h)
            self.h = None


def new_y(C, s):
    return torch.full((s * (4 * C.nbrows + PAD) + 3,), float("nan"), dtype=torch.float64, device="cuda")


def check_y(C, Yd, refs, s, what):
    """Columns bit-equal to refs[j]; everything else of the buffer still NaN."""
    n, ldy = 4 * C.nbrows, 4 * C.nbrows + PAD
    y = Yd.cpu().numpy()
    written = np.zeros(len(y), bool)
    for j in range(s):
        assert_same(y[j * ldy:j * ldy + n], refs[j], f"{what} column {j}")
        written[j * ldy:j * ldy + n] = True
    assert np.isnan(y[~written]).all(), f"{what}: wrote behind a column of Y"


_REFS = {}


def refs_of(C, X, arith, s, key="seeded", bv=None):
    """Oracle columns 0 .. s - 1 for the case's seeded values and X (computed once per case, association and column)."""
    R = _REFS.setdefault((C.name, arith, key, len(X)), {})
    for j in range(s):
        if j not in R:
            R[j] = ORACLE[arith](C.bp, C.bc, C.bv if bv is None else bv, X[j])
    return [R[j] for j in range(s)]


def plans_of(C, ucap=None):
    c128, c64 = TC.caps_of(ucap)
    return mpk.bcsr4_spmm_plan_probe(C.nbrows, C.bp, C.bc, 128, c128), mpk.bcsr4_spmm_plan_probe(C.nbrows, C.bp, C.bc, 64, c64)


def check_info(H, plans, form, s, what):
    """After a product of s columns: the form of every batch of at most eight, and the longest list."""
    C = H.C
    got = {}
    for m in sorted({min(8, s - j0) for j0 in range(0, s, 8)}):
        tb, fi, ll = H.info(m)
        want = TC.expected_form(C, *plans, form, m)
        assert tb == int(C.nblocks >= TC.MIN_BLOCKS and not plans[0]["refused"]), f"{what}: tile_built {tb}"
        assert fi == want, f"{what}: {m} columns run form {fi}, expected {want}"
        assert ll == TC.expected_longest_list(C, *plans, m), f"{what}: longest_list {ll} at {m} columns"
        got[m] = fi
    return got


LIMIT_RUNS = [(n, None) for n in TC.NAMES] + TC.CAPPED


@pytest.mark.parametrize("name,ucap", LIMIT_RUNS, ids=[f"{n}{'' if u is None else '-ucap' + u}" for n, u in LIMIT_RUNS])
def test_limits(name, ucap, monkeypatch):
    C = TC.case(name)
    if ucap is not None:
        monkeypatch.setenv("MI355_SPMM_TILE_UCAP", ucap)
    plans = plans_of(C, ucap)
    extra = (9, 11, 16) if name == "grid" and ucap is None else ()
    X = C.x(max((8,) + extra))
    Xd = dev(X)
    H = Handle(C)
    ran = set()
    try:
        for form in (1, 2, 3):
            monkeypatch.setenv("MI355_SPMM_TILE", str(form))
            for s in FORM_COLUMNS[form] + extra:
                for arith in ("chain", "blockacc"):
                    refs = refs_of(C, X, arith, s)
                    for rep in range(2):
                        what = f"{name} ucap {ucap} form {form} s={s} {arith} rep {rep}"
                        Yd = new_y(C, s)
                        H.spmm(Xd, s, Yd, arith)
                        torch.cuda.synchronize()
                        ran.update((form, m, f) for m, f in check_info(H, plans, form, s, what).items())
                        check_y(C, Yd, refs, s, what)
    finally:
        H.close()
    # what this case is for did run: every (form, s <= 8) pair through the tile unless the restated rule forbids it
    if name == "below:4095":
        assert {f for _, _, f in ran} == {0}
    elif not name.startswith(("long:", "rowsdiag:")):
        assert {(f, m, f) for f in (1, 2, 3) for m in FORM_COLUMNS[f]} <= ran, sorted(ran)


@pytest.mark.parametrize("L", TC.LONG)
def test_lds_boundary(L, monkeypatch):
    """One handle through all (form, s) pairs, the Y buffers made before the handle so that nothing else is launched in between: the pairs
    whose umax (4 s + 2) 8 bytes fit 160 KiB run the tile — L = 1137 at s = 4 asks for 163 728 bytes, 1462 at 3 and 602 at 8 for 163 744,
    787 at 6 for 163 696, 2048 at 2 for all 163 840 — and the pairs that do not fit run form 0; all bit-equal."""
    C = TC.case(f"long:{L}")
    plans = plans_of(C)
    assert plans[0]["umax"] == plans[1]["umax"] == L
    pairs = [(f, s) for f in (1, 2, 3) for s in FORM_COLUMNS[f]]
    fits = [(f, s) for f, s in pairs if TC.lds_bytes(L, s) <= TC.LDS_BYTES]
    assert [TC.expected_form(C, *plans, f, s) for f, s in pairs] == [f if (f, s) in fits else 0 for f, s in pairs]
    X = C.x(8)
    Xd = dev(X)
    Ys = {(f, s, a): new_y(C, s) for f, s in pairs for a in ORACLE}
    torch.cuda.synchronize()
    H = Handle(C)
    try:
        for f, s in pairs:
            monkeypatch.setenv("MI355_SPMM_TILE", str(f))
            for a in ORACLE:
                H.spmm(Xd, s, Ys[f, s, a], a)
                _, fi, ll = H.info(s)
                assert fi == (f if (f, s) in fits else 0), f"long:{L} form {f} s={s}: runs form {fi} ({TC.lds_bytes(L, s)} bytes of LDS)"
                assert ll == L
        torch.cuda.synchronize()
        for (f, s, a), Yd in Ys.items():
            check_y(C, Yd, refs_of(C, X, a, s), s, f"long:{L} form {f} s={s} {a} ({TC.lds_bytes(L, s)} bytes of LDS)")
    finally:
        H.close()


def test_block_row_map(monkeypatch):
    """`grid` written out as CSR under a scrambled node numbering, the relabelling forced: mi_spmm_dev gathers the columns into the new
    numbering and the tile stores through the block-row map.  (A CSR handle has no mi_bcsr4_spmm_info; that its blocked copy exists is
    what set_kernel("bcsr4") proves, and the same pattern's forms are asserted in test_limits.)"""
    C = TC.case("grid")
    p, c, v = TC.to_csr(C)
    p, c, v, _ = synth.permute_nodes(p, c, v, block=4, seed=5)
    n = len(p) - 1
    monkeypatch.setenv("MI355_REORDER", "1")
    X = np.random.default_rng(8).uniform(-1, 1, (4, n))
    refs = [O.spmv(p, c, v, x) for x in X]
    Xd = dev(X)
    A = mpk.csrmatrix(n, p, c, v)
    try:
        A.set_kernel("bcsr4")
        assert A.reorder_info()["reordered"], A.reorder_info()
        assert A.kernel_name().startswith("spmv_bcsr4"), A.kernel_name()
        ldy = n + PAD
        for form in (1, 2, 3):
            monkeypatch.setenv("MI355_SPMM_TILE", str(form))
            for s in (2, 4):
                for rep in range(2):
                    Yd = torch.full((s * ldy + 3,), float("nan"), dtype=torch.float64, device="cuda")
                    mpk.check(mpk.lib().mi_spmm_dev(A.handle, s, ctypes.c_void_p(Xd.data_ptr()), n, ctypes.c_void_p(Yd.data_ptr()), ldy, mpk._stream_ptr()))
                    torch.cuda.synchronize()
                    check_y(C, Yd, refs, s, f"relabelled grid form {form} s={s} rep {rep}")
    finally:
        A.close()


def _four_columns(x):
    """test_gpu_edges._columns extended to four: the case's x, and three others that move its special entries to other rows."""
    return np.stack([x, np.roll(x, 4) * 0.5, -np.roll(x, -4), np.roll(x, 8) * -0.25])


@pytest.mark.parametrize("case", list(IEEE_CASES), ids=list(IEEE_CASES))
@pytest.mark.parametrize("pattern", ["grid", "empty"])
def test_ieee_values(pattern, case, monkeypatch):
    """Non-finite x where rows look and at nodes in no tile's list, stored zeros against Inf, rows of -0.0 products and empty rows (+0.0),
    subnormal partial sums, and the overflow whose class depends on the order — each association against its own oracle."""
    base = TC.case(pattern)
    p0, c0, _ = TC.to_csr(base)
    p, c, v, x, pins = IEEE_CASES[case](p0, c0, 4, np.random.default_rng(3000 + list(IEEE_CASES).index(case)))
    bp, bc, bv = synth.csr_to_bcsr4(p, c, v)
    C = TC.Case(f"{pattern}/{case}", base.nbrows, base.nbcols, [bc[bp[r]:bp[r + 1]] for r in range(base.nbrows)], 0)
    assert C.nblocks >= TC.MIN_BLOCKS
    plans = plans_of(C)
    X = _four_columns(x)
    Xd = dev(X)
    H = Handle(C, bv)
    try:
        for arith in ORACLE:
            refs = [ORACLE[arith](bp, bc, bv, xc) for xc in X]
            for form in (1, 2, 3):
                monkeypatch.setenv("MI355_SPMM_TILE", str(form))
                Yd = new_y(C, 4)
                H.spmm(Xd, 4, Yd, arith)
                torch.cuda.synchronize()
                what = f"{pattern} [{case}] form {form} {arith}"
                assert check_info(H, plans, form, 4, what) == {4: form}, what
                check_y(C, Yd, refs, 4, what)
                y = Yd.cpu().numpy()[:4 * C.nbrows]
                if pins.get("finite"):
                    assert np.isfinite(y).all(), f"{what}: an unreferenced NaN / Inf reached y"
                if "plus_zero" in pins:
                    assert (y[pins["plus_zero"]].view(np.uint64) == 0).all(), f"{what}: rows of -0.0 products / empty rows are not +0.0"
                if pins.get("subnormal"):
                    assert (np.abs(y[y != 0]) < np.finfo(np.float64).tiny).any(), f"{what}: no subnormal result"
            if case == "overflow-order":
                assert np.isinf(refs[0]).any() or np.isnan(refs[0]).any()
    finally:
        H.close()


@pytest.mark.parametrize("form", [1, 2, 3])
def test_first_product_on_a_fresh_non_blocking_stream(form, monkeypatch):
    """Create, then with no synchronisation the handle's first product — the one that builds and uploads the lists — on a new non-blocking
    stream."""
    monkeypatch.setenv("MI355_SPMM_TILE", str(form))
    C = TC.case("grid")
    plans = plans_of(C)
    X = C.x(4)
    Xd, Yd = dev(X), new_y(C, 4)
    torch.cuda.synchronize()
    H = Handle(C)
    try:
        st = torch.cuda.Stream()
        assert stream_flags(st) & HIP_STREAM_NON_BLOCKING, "the side stream must be non-blocking, or this proves nothing"
        with torch.cuda.stream(st):
            H.spmm(Xd, 4, Yd, "chain")
        torch.cuda.synchronize()
        assert check_info(H, plans, form, 4, f"fresh stream form {form}") == {4: form}
        check_y(C, Yd, refs_of(C, X, "chain", 4), 4, f"first product on a fresh stream, form {form}")
    finally:
        H.close()


@pytest.mark.parametrize("form", [1, 2, 3])
def test_one_handle_on_two_non_blocking_streams(form, monkeypatch):
    """s = 4 on one stream and s = 2 on another, queued three times each before waiting on either."""
    monkeypatch.setenv("MI355_SPMM_TILE", str(form))
    C = TC.case("grid")
    plans = plans_of(C)
    Xa, Xb = C.x(4), C.x(2, seed=1)
    Xad, Xbd = dev(Xa), dev(Xb)
    Ya, Yb = new_y(C, 4), new_y(C, 2)
    H = Handle(C)
    try:
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        assert all(stream_flags(st) & HIP_STREAM_NON_BLOCKING for st in streams)
        torch.cuda.synchronize()
        for _ in range(3):
            with torch.cuda.stream(streams[0]):
                H.spmm(Xad, 4, Ya, "chain")
            with torch.cuda.stream(streams[1]):
                H.spmm(Xbd, 2, Yb, "chain")
        torch.cuda.synchronize()
        assert check_info(H, plans, form, 4, "two streams") == {4: form} and check_info(H, plans, form, 2, "two streams") == {2: form}
        check_y(C, Ya, refs_of(C, Xa, "chain", 4), 4, f"form {form}: four columns on stream 0")
        check_y(C, Yb, [O.spmv_bcsr4(C.bp, C.bc, C.bv, x) for x in Xb], 2, f"form {form}: two columns on stream 1")
    finally:
        H.close()


@pytest.mark.parametrize("form", [1, 2])
def test_value_refresh_and_product_on_one_stream(form, monkeypatch):
    """update_values from a device array on a stream, the product behind it on the same stream: the new values (the tile kernels read the
    handle's block array directly)."""
    monkeypatch.setenv("MI355_SPMM_TILE", str(form))
    C = TC.case("grid")
    plans = plans_of(C)
    X = C.x(4)
    Xd, Y0, Y1 = dev(X), new_y(C, 4), new_y(C, 4)
    v2 = C.values(991)
    v2d = dev(v2)
    H = Handle(C)
    try:
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            H.spmm(Xd, 4, Y0, "chain")
            H.update_dev(v2d)
            H.spmm(Xd, 4, Y1, "chain")
        torch.cuda.synchronize()
        assert check_info(H, plans, form, 4, "refresh") == {4: form}
        check_y(C, Y0, refs_of(C, X, "chain", 4), 4, f"form {form}: before the refresh")
        check_y(C, Y1, [O.spmv_bcsr4(C.bp, C.bc, v2, x) for x in X], 4, f"form {form}: after the refresh on the same stream")
        assert not np.array_equal(Y0.cpu().numpy()[:8], Y1.cpu().numpy()[:8])
    finally:
        H.close()


@pytest.mark.parametrize("measured_first", [True, False], ids=["after-the-choice", "fresh-handle"])
def test_captured_product(measured_first, capsys):
    """No form forced.  after-the-choice: one product outside capture (the forms are timed and one is kept), then a captured product replayed
    with a changed X and after a device-side value refresh.  fresh-handle: the capture is the handle's first product (the gather kernels
    are recorded: no measurement and no upload under capture).  Whatever form was captured, all results are bit-equal."""
    C = TC.case("grid")
    s = 4
    X, X2 = C.x(s), C.x(s, seed=2)
    v2 = C.values(992)
    Xd, v2d, Yd = dev(X), dev(v2), new_y(C, s)
    H = Handle(C)
    side = torch.cuda.Stream()
    try:
        form = "gather (nothing measured)"
        if measured_first:
            H.spmm(Xd, s, Yd, "chain")
            torch.cuda.synchronize()
            check_y(C, Yd, refs_of(C, X, "chain", s), s, "eager product")
            tb, fi, _ = H.info(s)
            assert tb == 1 and 0 <= fi <= 4
            form = f"form {fi}"
            with capsys.disabled():
                print(f"\n  multi-vector product on grid, {s} columns, no form forced: form_in_use {fi}")
        Yd.fill_(float("nan"))
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                H.spmm(Xd, s, Yd, "chain")
        with torch.cuda.stream(side):
            Yd.fill_(float("nan"))
            g.replay()
        torch.cuda.synchronize()
        check_y(C, Yd, refs_of(C, X, "chain", s), s, f"replay, captured {form}")
        with torch.cuda.stream(side):
            Yd.fill_(float("nan"))
            Xd.copy_(dev(X2))
            g.replay()
        torch.cuda.synchronize()
        check_y(C, Yd, [O.spmv_bcsr4(C.bp, C.bc, C.bv, x) for x in X2], s, f"replay with a changed X, captured {form}")
        with torch.cuda.stream(side):
            Yd.fill_(float("nan"))
            H.update_dev(v2d)
            g.replay()
        torch.cuda.synchronize()
        check_y(C, Yd, [O.spmv_bcsr4(C.bp, C.bc, v2, x) for x in X2], s, f"replay after a device-side value refresh, captured {form}")
    finally:
        H.close()
