"""The blocked sliced-stream kernels (spmv_bcsr_sell.hpp) at every limit of their plan.

CPU part (unmarked): for every case of tests/bsell_cases.py (the limit table and 100 seeded patterns) mi_bcsr4_sell_plan_probe must
agree EXACTLY with the plain restatement — every integer of sptr, of the wave ranges at both caps and of the column stream with its
tail; every tag a case carries is checked against the restatement; every limit has a case on each of its sides.

GPU part (gpu), everything bit for bit against the oracle's SpMV_BCSR_FMA restatement (there is no tolerance to choose):
  the product      every case forced onto the sliced copy (MI355_BCSR_SELL=1) in each variant (MI355_BCSR_SELL_FORM 0-3; seeded cases two
                   variants each, all four over the set), mi_bcsr4_sell_info confirming variant, steps and padding; y pre-filled with NaN
                   and a NaN guard behind it; x infinite at node 0 and at every block column no block names, so that a padding place that
                   were multiplied would show.  The (case, variant) pairs are counted and the total is asserted.
  refreshes        update_values from a host array, from a device array on a second stream, and from column-major blocks, on a case of
                   each refresh tier; after each, the handle's row-major blocks are read back through the row-per-quad kernel.
  the CSR handle   the same patterns as CSR matrices with the blocked copy forced (one variant per case, rotating); value refreshes
                   from the host and from the device on a case of each tier: the product, and the CSR copy through a CSR kernel.
  multi-vector     MatMatMult_SeqBAIJ_4 with the sliced form forced (MI355_SPMM_TILE=4) at s = 4, 8, 11, both associations, padded
                   leading dimensions with NaN guards, on the cases that fill the parks of 16 and of 8 slices.
  powers, row map  mi_bcsr4_spmk with k = 3 on a square park-filling case; the same pattern under a scrambled node numbering with the
                   relabelling forced (the stores go through the block-row map).
  no block column  a matrix with block rows and no block columns never gets a sliced copy: y = +0.0 through the row-per-quad kernel."""
import ctypes

import numpy as np
import pytest

import bsell_cases as BC
from conftest import assert_bit_equal
from navierstokes_amd import mpk
from oracle import oracle as O

TABLE = BC.table()
SEEDED = BC.seeded_cases()
BY_NAME = {c.name: c for c in TABLE}
TIER_CASES = ("tier_4096", "tier_4112", "tier_16384", "tier_16400")
MM_CASES = ("park_7", "park_8", "park_9", "park_15", "park_16", "park_17", "park_32", "park_33")


def restated(case):
    return BC.restate(case.nbrows, case.ptrow, case.indcol)


def check_against_restatement(case):
    R = restated(case)
    for cap in BC.CAPS:
        P = mpk.bcsr4_sell_plan_probe(case.nbrows, case.ptrow, case.indcol, cap)
        what = f"{case.name} cap {cap}"
        assert (P["nslices"], P["nsteps"], P["nwaves"]) == (R["nslices"], R["nsteps"], R[cap]["nwaves"]), what
        assert np.array_equal(P["sptr"], R["sptr"]), f"{what}: sptr"
        assert np.array_equal(P["wrng"], R[cap]["wrng"]), f"{what}: wave ranges"
        assert P["col"].dtype == R["col"].dtype and np.array_equal(P["col"], R["col"]), f"{what}: column stream"
    return R


@pytest.mark.parametrize("case", TABLE, ids=lambda c: c.name)
def test_table_case_plans(case):
    """The limit table: the probe against the restatement at both caps; the case's tags and pinned wave counts against the restatement."""
    R = check_against_restatement(case)
    if case.waves is not None:
        assert (R[1024]["nwaves"], R[2048]["nwaves"]) == case.waves, (case.name, R[1024]["nwaves"], R[2048]["nwaves"])
    for t in case.tags:
        assert BC.claim_holds(t, case, R), f"{case.name}: tagged {t}, which the restatement does not confirm"
        assert t not in BC.NOT_REACHED
    assert case.nblocks <= BC.MAX_BLOCKS


@pytest.mark.parametrize("chunk", range(4))
def test_seeded_case_plans(chunk):
    for case in SEEDED[chunk::4]:
        check_against_restatement(case)


def test_restatement_on_a_pattern_written_out_by_hand():
    """17 block rows: row 0 holds blocks at columns 5, 2; row 3 one at column 7; row 16 none.  Two slices of 2 and 1 steps."""
    lens = np.zeros(17, np.int64)
    lens[0], lens[3] = 2, 1
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    R = BC.restate(17, p, np.array([5, 2, 7], np.int32))
    assert R["sptr"].tolist() == [0, 2, 3, 3, 3] and R["nsteps"] == 3 and R["col"].shape == (51, 16)
    F, P = BC.FIRST, BC.PAD
    assert R["col"][0].tolist() == [F | 5, F | P, F | P, F | 7] + [F | P] * 12
    assert R["col"][1].tolist() == [2] + [P] * 15
    assert R["col"][2].tolist() == [F | P] * 16 and R["col"][3].tolist() == [F | P] * 16 and (R["col"][4:] == P).all()
    assert R[1024]["nwaves"] == 32 and R[1024]["wrng"].tolist() == [0] * 11 + [1] * 21 + [2]  # targets 3 w / 32: 0 up to w = 10, then 1 or 2 — slice 1 starts at step 2
    assert R["max_slice_vals"] == 48 and R["padding"] == 3 * 16 / 3 - 1.0
    assert [BC.wave_count(n, 1024) for n in (0, 65, 66, 1985, 1986, 4098)] == [32, 32, 64, 992, 1024, 1024]
    assert [BC.wave_count(n, 2048) for n in (2049, 2050, 4033, 4034, 4098)] == [1024, 1056, 2016, 2048, 2048]


def test_every_limit_has_a_case_on_each_side(capsys):
    sides = {lim: {s: [] for s in LIM[0]} for lim, LIM in BC.LIMITS.items()}
    feats = {f: [] for f in BC.FEATURES}
    for case in TABLE:
        for t in case.tags:
            if ":" in t:
                lim, side = t.split(":")
                sides[lim][side].append(case.name)
            else:
                feats[t].append(case.name)
    with capsys.disabled():
        print("\nblocked sliced stream: cases per side of every limit")
        for lim, s in sides.items():
            print(f"  {lim:16s} " + "  ".join(f"{k}: {len(v)}" for k, v in s.items()))
    for lim, s in sides.items():
        for side, names in s.items():
            assert names or f"{lim}:{side}" in BC.NOT_REACHED, f"limit {lim}: no case on side {side}"
            assert not (names and f"{lim}:{side}" in BC.NOT_REACHED), f"{lim}:{side} is listed as not reached, but {names} reach it"
    for f, names in feats.items():
        assert names or f in BC.NOT_REACHED, f"no case carries {f}"
    # each refresh tier: a case with more slices than its grid; each (tier, case) the GPU part refreshes lies where its name says
    assert [BC.refresh_tier(restated(BY_NAME[n])["max_slice_vals"])[0] for n in TIER_CASES] == [4096, 16384, 16384, 0]
    assert [restated(BY_NAME[n])["max_slice_vals"] for n in TIER_CASES] == [4096, 4112, 16384, 16400]


def test_signed_zero_case_sums_to_minus_zero_in_front_of_padding():
    case = BY_NAME["neg_zero"]
    y = O.spmv_bcsr4(case.ptrow, case.indcol, case.values(), case.x(inf=False))
    lens = np.diff(case.ptrow)
    R = restated(case)
    minus = np.signbit(y) & (y == 0)
    rows = np.nonzero(minus.reshape(-1, 4).all(axis=1))[0]
    assert len(rows) >= 10 and (lens[rows] > 0).all()
    assert (lens[rows] < R["slice_len"][rows // BC.ROWS]).any(), "no -0.0 row with padding steps behind it"


def _block_perm(case):
    """block-row relabelling mi_csr_create would apply to the case's CSR form: perm[old block row] = new"""
    n, _, p, c = case.csr()
    perm = np.zeros(n, np.int32)
    blk = ctypes.c_int()
    sb, sa = ctypes.c_double(), ctypes.c_double()
    mpk.check(mpk.lib().mi_reorder_probe(n, p.ctypes.data, c.ctypes.data, ctypes.byref(blk), perm.ctypes.data, ctypes.byref(sb), ctypes.byref(sa)))
    assert blk.value == 4 and (perm[0::4] % 4 == 0).all()
    return perm[0::4] // 4


def _scrambled(case, seed=3):
    """the case under a random numbering of its nodes: (ptrow, indcol, the block permutation old -> new)"""
    rng = np.random.default_rng(seed)
    new_of_old = rng.permutation(case.nbrows)
    old_of_new = np.argsort(new_of_old)
    lens = np.diff(case.ptrow)[old_of_new]
    p2 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = np.repeat(case.ptrow[:-1][old_of_new].astype(np.int64) - p2[:-1], lens) + np.arange(p2[-1])
    return p2, new_of_old[case.indcol[idx]].astype(np.int32), idx


def test_relabelled_park_case_still_fills_the_park():
    """The square park-filling case under a scrambled numbering, relabelled as mi_csr_create relabels it: one wave of the twin's
    blocked copy still owns more slices than the park holds (else the GPU part's row-map product would not reach the flush)."""
    case = BY_NAME["park_square"]
    p2, c2, _ = _scrambled(case)
    S = BC.Case("scrambled", np.diff(p2), nbcols=case.nbcols)
    S.indcol = c2
    perm = _block_perm(S)
    inv = np.argsort(perm)
    lens = np.diff(p2)[inv]
    p3 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = np.repeat(p2[:-1][inv].astype(np.int64) - p3[:-1], lens) + np.arange(p3[-1])
    R = BC.restate(case.nbrows, p3, perm[c2[idx]])
    assert R[1024]["spw"].max() > BC.PARK["w1"], R[1024]["spw"].max()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
GUARD = 9
RAN = {"pairs": 0, "table": set(), "seeded": set()}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def _sell_info(handle):
    b, f, st, pad = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong(), ctypes.c_double()
    mpk.check(mpk.lib().mi_bcsr4_sell_info(handle, ctypes.byref(b), ctypes.byref(f), ctypes.byref(st), ctypes.byref(pad), None))
    return dict(built=b.value, form=f.value, steps=st.value, padding=pad.value)


def _product(B, case, x, what, v):
    n = 4 * case.nbrows
    y = _nan(n + GUARD)
    mpk.SpMV_BCSR(y[:n], _dev(x), B)
    got = y.cpu().numpy()
    assert_bit_equal(got[:n], O.spmv_bcsr4(case.ptrow, case.indcol, v, x), what)
    assert np.isnan(got[n:]).all(), f"{what}: written behind y"


def _run_forms(case, forms, monkeypatch):
    R = restated(case)
    v = case.values()
    for f in forms:
        monkeypatch.setenv("MI355_BCSR_SELL_FORM", str(f))
        B = _make(case, v)
        info = _sell_info(B.handle)
        what = f"{case.name} variant {f}"
        assert info == dict(built=1, form=f, steps=R["nsteps"], padding=R["padding"]), (what, info, R["nsteps"], R["padding"])
        _product(B, case, case.x(inf=True), f"{what}: y = A x", v)
        if case.special == "neg_zero":
            _product(B, case, case.x(inf=False), f"{what}: y = A x, x finite at node 0", v)
        if case.nblocks == 0 and case.nbrows:
            y = _nan(4 * case.nbrows)
            mpk.SpMV_BCSR(y, _dev(case.x(inf=True)), B)
            assert (y.cpu().numpy().view(np.uint64) == 0).all(), f"{what}: y is not +0.0"
        B.close()
        RAN["pairs"] += 1


def _seeded_forms(q):
    return q % 4, (q % 4 + 1 + (q // 4) % 3) % 4  # two different variants; every pair of variants occurs


@pytest.fixture
def forced(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    mpk.lib()
    monkeypatch.setenv("MI355_BCSR_SELL", "1")
    monkeypatch.setenv("MI355_REORDER", "0")
    return monkeypatch


def _make(case, v, nbcols=None, layout="row"):
    B = mpk.bcsr4x4_matrix(case.nbrows, case.ptrow, case.indcol, v, nbcols=case.nbcols if nbcols is None else nbcols, layout=layout)
    B.nbcols = case.nbcols if nbcols is None else nbcols  # (the class widens nbcols to the row count; the handle, made lazily, takes the case's)
    return B


@pytest.mark.gpu
@pytest.mark.parametrize("case", TABLE, ids=lambda c: c.name)
def test_gpu_table_case(case, forced):
    _run_forms(case, (0, 1, 2, 3), forced)
    RAN["table"].add(case.name)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(4))
def test_gpu_seeded_cases(chunk, forced):
    for q, case in enumerate(SEEDED):
        if q % 4 == chunk:
            _run_forms(case, _seeded_forms(q), forced)
            RAN["seeded"].add(case.name)


@pytest.mark.gpu
def test_gpu_every_pair_ran(forced):
    """Runs after the two tests above (file order): four variants of every table case, two of every seeded case; all four variants
    occur among the seeded pairs."""
    assert RAN["table"] == {c.name for c in TABLE} and RAN["seeded"] == {c.name for c in SEEDED}
    assert RAN["pairs"] == 4 * len(TABLE) + 2 * len(SEEDED), RAN["pairs"]
    assert {f for q in range(len(SEEDED)) for f in _seeded_forms(q)} == {0, 1, 2, 3}


def _transposed(v):
    return np.ascontiguousarray(v.reshape(-1, 4, 4).transpose(0, 2, 1)).reshape(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", TIER_CASES)
@pytest.mark.parametrize("layout", ["row", "col"])
def test_gpu_bcsr_refreshes(name, layout, forced):
    """mi_bcsr4_update_values_layout{,_dev}: host array, device array on a second stream; row-major and column-major blocks."""
    import torch
    case = BY_NAME[name]
    x = case.x(inf=True)
    give = (lambda v: v) if layout == "row" else _transposed
    forced.setenv("MI355_BCSR_SELL_FORM", "0" if layout == "row" else "3")
    B = _make(case, give(case.values(0)), layout=layout)
    assert _sell_info(B.handle)["built"] == 1
    _product(B, case, x, f"{name} {layout}: as created", case.values(0))
    v1 = case.values(1)
    B.update_values(give(v1))
    _product(B, case, x, f"{name} {layout}: after a host refresh", v1)
    v2 = case.values(2)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        d2 = _dev(give(v2))
        B.update_values(d2)
    s2.wait_stream(s1)
    n = 4 * case.nbrows
    with torch.cuda.stream(s2):
        y = _nan(n + GUARD)
        mpk.SpMV_BCSR(y[:n], _dev(x), B)
    s2.synchronize()
    got = y.cpu().numpy()
    y2 = O.spmv_bcsr4(case.ptrow, case.indcol, v2, x)
    assert_bit_equal(got[:n], y2, f"{name} {layout}: after a device refresh on another stream")
    assert np.isnan(got[n:]).all()
    # the handle's row-major blocks followed: a second handle without the sliced copy, refreshed the same way, reads them
    forced.setenv("MI355_BCSR_SELL", "0")
    C = _make(case, give(case.values(0)), layout=layout)
    assert _sell_info(C.handle)["built"] == 0
    C.update_values(_dev(give(v2)))
    _product(C, case, x, f"{name} {layout}: the blocks after a device refresh (row-per-quad kernel)", v2)
    C.update_values(give(v1))
    _product(C, case, x, f"{name} {layout}: the blocks after a host refresh (row-per-quad kernel)", v1)
    B.close()
    C.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", TIER_CASES)
def test_gpu_refreshed_blocks_of_a_sliced_handle(name, forced):
    """bcsr4_blocks_refresh_kernel writes the row-major blocks AND the sliced values; the products above read the sliced values only.
    Here the blocks of the same (sliced) handle are read: the multi-vector product at three columns runs the gather kernels on them."""
    case = BY_NAME[name]
    for layout in ("row", "col"):
        give = (lambda v: v) if layout == "row" else _transposed
        B = _make(case, give(case.values(0)), layout=layout)
        assert _sell_info(B.handle)["built"] == 1
        v2 = case.values(2)
        B.update_values(_dev(give(v2)))
        X = np.stack([case.x(inf=True)] * 3)
        X[1:, :] = np.where(np.isfinite(X[1:, :]), 0.5 * X[1:, :], X[1:, :])
        Y = _nan(3, 4 * case.nbrows)
        mpk.MatMatMult_SeqBAIJ_4(B, _dev(X), Y, "chain")
        for j in range(3):
            assert_bit_equal(Y[j].cpu().numpy(), O.spmv_bcsr4(case.ptrow, case.indcol, v2, X[j]), f"{name} {layout}: blocks after a device refresh, column {j}")
        B.close()


def _csr_cases():
    return [c for c in TABLE if c.nblocks > 0]


@pytest.mark.gpu
@pytest.mark.parametrize("case", _csr_cases(), ids=lambda c: c.name)
def test_gpu_csr_handle(case, forced):
    """The pattern as a CSR matrix whose blocked copy (sliced) is forced; refreshes on the tier cases."""
    import torch
    f = sum(map(ord, case.name)) % 4
    forced.setenv("MI355_BCSR_SELL_FORM", str(f))
    v = case.values()
    n, ncols, p, c, cv = case.csr(v)
    x = case.x(inf=True)
    A = mpk.csrmatrix(n, p, c, cv, ncols=ncols).set_kernel("bcsr4")
    what = f"{case.name} as CSR, variant {f}"
    assert "spmv_bcsr4_sell" in A.kernel_name(), (what, A.kernel_name())

    def product(vals, tag):
        y = _nan(n + GUARD)
        mpk.SpMV_CSR(y[:n], _dev(x), A)
        got = y.cpu().numpy()
        assert_bit_equal(got[:n], O.spmv(p, c, vals, x), f"{what}: {tag} ({A.kernel_name()})")
        assert np.isnan(got[n:]).all(), f"{what}: written behind y"

    product(cv, "y = A x")
    if case.name in TIER_CASES or case.name == "park_big":
        if case.name != "park_big":
            cv1 = case.csr(case.values(1))[4]
            A.update_values(cv1)
            product(cv1, "after a host refresh")
        cv2 = case.csr(case.values(2))[4]
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            d2 = _dev(cv2)
            A.update_values(d2)
        s2.wait_stream(s1)
        with torch.cuda.stream(s2):
            product(cv2, "after a device refresh on another stream")
        s2.synchronize()
        A.set_kernel("stream")  # the CSR copy followed too
        assert "sell" not in A.kernel_name()
        product(cv2, "the CSR values after the device refresh")
        if case.name != "park_big":
            A.set_kernel("bcsr4")
            A.update_values(cv1)
            A.set_kernel("stream")
            product(cv1, "the CSR values after a host refresh")
    A.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", MM_CASES)
def test_gpu_multi_vector(name, forced):
    """spmm_bcsr4_sell at four and eight columns (and eleven: eight through it, three through the gather kernel), both associations."""
    case = BY_NAME[name]
    forced.setenv("MI355_SPMM_TILE", "4")
    v = case.values()
    B = _make(case, v)
    n, nc = 4 * case.nbrows, 4 * case.nbcols
    x0 = case.x(inf=True)
    for s in (4, 8, 11):
        if s <= 8:
            form = ctypes.c_int()
            mpk.check(mpk.lib().mi_bcsr4_spmm_info(B.handle, s, None, ctypes.byref(form), None, None))
            assert form.value == 4, (name, s, form.value)
        X = np.stack([np.where(np.isfinite(x0), x0 * (1.0 + 0.25 * j), x0) for j in range(s)])
        Xd = _nan(s, nc + 6)
        Xd[:, :nc] = _dev(X)
        for arith, orc in (("chain", O.spmv_bcsr4), ("blockacc", O.spmv_bcsr4_blockacc)):
            Yd = _nan(s, n + GUARD)
            mpk.MatMatMult_SeqBAIJ_4(B, Xd, Yd, arith)
            got = Yd.cpu().numpy()
            for j in range(s):
                assert_bit_equal(got[j, :n], orc(case.ptrow, case.indcol, v, X[j]), f"{name} s = {s} {arith} column {j}")
            assert np.isnan(got[:, n:]).all(), f"{name} s = {s} {arith}: written behind a column"
    B.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_gpu_powers_on_a_park_filling_case(form, forced):
    import torch
    case = BY_NAME["park_square"]
    forced.setenv("MI355_BCSR_SELL_FORM", str(form))
    v = 0.01 * case.values()
    B = _make(case, v)
    assert _sell_info(B.handle)["form"] == form
    n = 4 * case.nbrows
    x = case.x(inf=True)
    outs = [_nan(n) for _ in range(3)]
    ptrs = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in outs])
    dx = _dev(x)
    mpk.check(mpk.lib().mi_bcsr4_spmk_dev(B.handle, 3, ctypes.c_void_p(dx.data_ptr()), ptrs, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    src = x
    for k in range(3):
        src = O.spmv_bcsr4(case.ptrow, case.indcol, v, src)
        assert_bit_equal(outs[k].cpu().numpy(), src, f"power {k + 1}, variant {form}")
    B.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", [0, 2])
def test_gpu_park_flush_through_the_block_row_map(form, forced):
    """The square park-filling case under a scrambled node numbering, relabelled at create (MI355_REORDER=1): the twin's blocked copy
    stores through its block-row map, from a park that fills (test_relabelled_park_case_still_fills_the_park)."""
    case = BY_NAME["park_square"]
    forced.setenv("MI355_REORDER", "1")
    forced.setenv("MI355_BCSR_SELL_FORM", str(form))
    p2, c2, idx = _scrambled(case)
    S = BC.Case("scrambled", np.diff(p2), nbcols=case.nbcols)
    S.indcol = c2
    v = S.values()
    n, ncols, p, c, cv = S.csr(v)
    A = mpk.csrmatrix(n, p, c, cv, ncols=ncols).set_kernel("bcsr4")
    assert A.reorder_info()["reordered"] and "spmv_bcsr4_sell" in A.kernel_name(), (A.reorder_info(), A.kernel_name())
    x = S.x(inf=False)
    y = _nan(n + GUARD)
    mpk.SpMV_CSR(y[:n], _dev(x), A)
    got = y.cpu().numpy()
    assert_bit_equal(got[:n], O.spmv(p, c, cv, x), f"relabelled, variant {form}")
    assert np.isnan(got[n:]).all()
    cv2 = S.csr(S.values(2))[4]
    A.update_values(_dev(cv2))
    mpk.SpMV_CSR(y[:n], _dev(x), A)
    assert_bit_equal(y[:n].cpu().numpy(), O.spmv(p, c, cv2, x), f"relabelled, variant {form}, after a device refresh")
    A.close()


@pytest.mark.gpu
def test_gpu_no_block_columns_never_takes_the_sliced_copy(forced):
    """nbrows > 0, nbcols = 0 with the sliced copy forced: every slice would be one padding step, which reads x at node 0 — of an x without
    elements.  mi_bcsr4_create builds no sliced copy there; y = +0.0 through the row-per-quad kernel."""
    L = mpk.lib()
    nbr = 100
    p = np.zeros(nbr + 1, np.int32)
    h = ctypes.c_void_p()
    mpk.check(L.mi_bcsr4_create(nbr, 0, p.ctypes.data, None, None, ctypes.byref(h)))
    info = _sell_info(h)
    assert info["built"] == 0 and info["form"] == -1, info
    y = np.full(4 * nbr, np.nan)
    x = np.zeros(1)
    mpk.check(L.mi_bcsr4_spmv(h, x.ctypes.data, y.ctypes.data))
    assert (y.view(np.uint64) == 0).all()
    L.mi_bcsr4_destroy(h)
