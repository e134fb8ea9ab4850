"""The C-ABI of the block DILU's device refactor (mi_dilu4dev_*) on a box without a GPU: the six exports are declared, exported and
bound; the argument rules hold before the device is touched; the plan probe — which builds the plan AND replays it against the
pattern — counts the pivot pairs worked out in Python from the pattern in the handle's numbering, on every pattern of
tests/bilu4_order_cases.py (the fe: ones are left to tests/test_gpu_dilu4dev.py), every case of tests/dilu4_limit_cases.py and the
three dropped cases of tests/dilu4dev_cases.py, whose own properties (all factor in the model, level widths, census) are checked
here too."""
import ctypes
import os
import re

import numpy as np
import pytest

import bilu4_cases as C
import bilu4_order_cases as OC
import bilu4_wide_cases as W
import dilu4_limit_cases as LC
import dilu4dev_cases as DC
from conftest import ROOT, assert_bit_equal

LIB = os.path.join(ROOT, "navierstokes_amd", "csrc", "libmi355spmv.so")
SYMBOLS = ("mi_dilu4dev_plan_probe", "mi_dilu4dev_prepare", "mi_dilu4dev_refactor", "mi_dilu4dev_status", "mi_dilu4dev_fetch",
           "mi_dilu4dev_info")
FIXED_LAUNCHES = 1  # include/mi355_spmv.h: "launches per refactor = forward launches + 1"
MI_ERR_ARG, MI_ERR_STATE = 1, 6
ORDERS = ("natural", "colour")
PROBE_CASES = ([("order", n) for n in OC.PATTERNS if not n.startswith("fe:")] + [("limit", n) for n in LC.NAMES] +
               [("dropped", n) for n in DC.NAMES])


def _matrix(kind, name):
    return {"order": OC.matrix, "limit": LC.matrix, "dropped": DC.dropped}[kind](name)


def test_exports_are_declared_and_bound():
    assert os.path.exists(LIB), "libmi355spmv.so not built (run __graft_entry__.build())"
    raw = ctypes.CDLL(LIB)
    src = open(os.path.join(ROOT, "include", "mi355_spmv.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mi_dilu4dev_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(SYMBOLS), declared ^ set(SYMBOLS)
    from navierstokes_amd import mpk
    L = mpk.lib()
    for s in SYMBOLS:
        assert hasattr(raw, s), f"{s} is not exported"
        assert getattr(L, s).argtypes, f"{s} is not bound in mpk.py"
    for name in ("prepare_dev", "refactor_dev", "factor_status", "fetch_dev", "info_dev"):
        assert hasattr(mpk.dilu4, name), name
    assert hasattr(mpk, "dilu4dev_plan_probe")
    assert L.mi_version() == 501
    assert "forward launches + 1" in src[src.index("mi_dilu4dev_*) ----"):] and "mi_dilu4dev_* (the device refactor of the block DILU)" in src
    # every entry cites the Newton step that refactors, like its neighbours
    for s in SYMBOLS:
        comment = src[:src.index(f"int {s}(")].rsplit("/*", 1)[1]
        assert "src/solve_newton.c:1245-1265" in comment, f"{s}: the header does not cite the Newton step"
    # the DILU section still says what is NOT built, less the device refactor
    dilu = src[src.index("EISENSTAT"):src.index("typedef struct mi_dilu4_s")]
    not_built = dilu[dilu.index("NOT built"):]
    for word in ("single-precision copy", "Jacobi sweeps", "one-launch form", "automatic", "mi_dist", "symbolic phase on the device"):
        assert word in not_built, word
    assert "NOT built: a refactorisation on the device" not in dilu


def _host_handle(order="natural"):
    from navierstokes_amd import mpk
    eye, off = np.eye(4).reshape(-1) * 2, np.ones(16) * 0.1
    return mpk.dilu4(2, [0, 2, 4], [0, 1, 0, 1], np.concatenate([eye, off, off, eye]), host_only=True, order=order)


def test_argument_rules_hold_before_the_device_is_touched():
    from navierstokes_amd import mpk
    L = mpk.lib()
    E = _host_handle()
    v = np.ones(64)
    vp = v.ctypes.data
    bad = ctypes.c_int(5)
    for call, word in ((lambda: L.mi_dilu4dev_prepare(None), "null handle"), (lambda: L.mi_dilu4dev_refactor(None, vp, 0, None), "null handle"),
                       (lambda: L.mi_dilu4dev_refactor(E.handle, None, 0, None), "null coef"),
                       (lambda: L.mi_dilu4dev_refactor(E.handle, vp, 7, None), "layout"), (lambda: L.mi_dilu4dev_refactor(E.handle, vp, -1, None), "layout"),
                       (lambda: L.mi_dilu4dev_status(None, ctypes.byref(bad)), "null handle"), (lambda: L.mi_dilu4dev_fetch(None), "null handle"),
                       (lambda: L.mi_dilu4dev_info(None, None, None, None), "null handle")):
        assert call() == MI_ERR_ARG, word
        assert word in L.mi_last_error().decode(), (word, L.mi_last_error())
    assert bad.value == 5 and (v == 1.0).all()
    E.close()


@pytest.mark.parametrize("order", ORDERS)
def test_a_host_only_handle_has_no_device_refactor(order):
    from navierstokes_amd import mpk
    L = mpk.lib()
    E = _host_handle(order)
    before = [a.copy() for a in E.fetch()]
    v = np.ones(64)
    bad = ctypes.c_int(5)
    for call in (lambda: L.mi_dilu4dev_prepare(E.handle), lambda: L.mi_dilu4dev_refactor(E.handle, v.ctypes.data, 0, None),
                 lambda: L.mi_dilu4dev_status(E.handle, ctypes.byref(bad)), lambda: L.mi_dilu4dev_fetch(E.handle)):
        assert call() == MI_ERR_STATE
        assert "host-only" in L.mi_last_error().decode()
    for method in (E.prepare_dev, E.factor_status, E.fetch_dev):
        with pytest.raises(mpk.MiError) as e:
            method()
        assert e.value.status == MI_ERR_STATE
    assert E.info_dev() == dict(prepared=False, launches=1 + FIXED_LAUNCHES, plan_bytes=0)  # two block rows: one folded launch
    assert L.mi_dilu4dev_info(E.handle, None, None, None) == 0
    for got, want in zip(E.fetch(), before):
        assert_bit_equal(got, want, "the host copies were written")
    assert (v == 1.0).all()
    E.close()
    with pytest.raises(ValueError):
        E.prepare_dev()


def test_an_empty_matrix_makes_every_call_a_no_op():
    from navierstokes_amd import mpk
    L = mpk.lib()
    for order in ORDERS:
        E = mpk.dilu4(0, [0], [], [], host_only=True, order=order)
        bad = ctypes.c_int(5)
        assert L.mi_dilu4dev_prepare(E.handle) == 0 and L.mi_dilu4dev_refactor(E.handle, None, 0, None) == 0
        assert L.mi_dilu4dev_status(E.handle, ctypes.byref(bad)) == 0 and bad.value == -1
        assert L.mi_dilu4dev_fetch(E.handle) == 0
        assert E.info_dev()["prepared"] is False
        assert mpk.dilu4dev_plan_probe(0, [0], [], order)["pivot_pairs"] == 0
        E.close()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kind,name", PROBE_CASES, ids=[f"{k}-{n}" for k, n in PROBE_CASES])
def test_plan_probe_counts_equal_the_pattern_s(kind, name, order):
    from navierstokes_amd import mpk
    nb, bp, bc, _ = _matrix(kind, name)
    got = mpk.dilu4dev_plan_probe(nb, bp, bc, order)  # (the library replays the plan against the pattern before it answers)
    bptr, bcol = DC.permuted_pattern(nb, bp, bc, order)
    want = DC.pivot_pairs(nb, bptr, bcol)
    assert got["pivot_pairs"] == want
    nl = sum(int((bcol[bptr[i]:bptr[i + 1]] < i).sum()) for i in range(nb))
    if kind == "dropped":
        assert 0 < want < nl, "a dropped case has mated and unmated L blocks"
    elif kind == "limit" or name in ("chain", "arrow"):
        assert want == nl, "a symmetric pattern has a mate for every L block"  # (the random patterns and unsym are not symmetric)
    assert got["launches"] == mpk.bilu4_plan_probe(nb, bptr, bcol, 0)["fwd_launches"] + FIXED_LAUNCHES
    assert got["plan_bytes"] == 4 * (nb + len(bc) + nl + 1)  # fpos, gather, mate and the refusal word
    assert got["plan_bytes"] > 0


def test_bad_patterns_are_refused_with_the_messages_of_create():
    from navierstokes_amd import mpk
    L = mpk.lib()
    i32 = lambda a: np.array(a, np.int32)
    coef = np.ones(16 * 4)
    cases = [(-1, i32([0]), i32([0])), (2, i32([1, 2, 3]), i32([0, 0, 1])), (2, i32([0, 2, 1]), i32([0, 1])), (2, i32([0, 1, 2]), i32([0, 2])),
             (2, i32([0, 2, 3]), i32([1, 0, 1])), (2, i32([0, 2, 3]), i32([0, 0, 1])), (2, i32([0, 1, 2]), i32([0, 0]))]
    for order in (0, 1):
        for nb, p, c in cases:
            h = ctypes.c_void_p()
            assert L.mi_dilu4_create_host(nb, p.ctypes.data, c.ctypes.data, coef.ctypes.data, 0, order, ctypes.byref(h)) == MI_ERR_ARG
            want = L.mi_last_error().decode()
            assert L.mi_dilu4dev_plan_probe(nb, p.ctypes.data, c.ctypes.data, order, None, None, None) == MI_ERR_ARG
            assert L.mi_last_error().decode() == want and want
    assert L.mi_dilu4dev_plan_probe(2, None, None, 0, None, None, None) == MI_ERR_ARG and "null ptrow" in L.mi_last_error().decode()
    good = i32([0, 1, 2]), i32([0, 1])
    for ordering in (2, -1):
        assert L.mi_dilu4dev_plan_probe(2, good[0].ctypes.data, good[1].ctypes.data, ordering, None, None, None) == MI_ERR_ARG
        assert "unknown ordering" in L.mi_last_error().decode()
    assert L.mi_dilu4dev_plan_probe(2, good[0].ctypes.data, good[1].ctypes.data, 1, None, None, None) == 0
    with pytest.raises(mpk.MiError):
        mpk.dilu4dev_plan_probe(2, [0, 1, 2], [0, 0])
    with pytest.raises(ValueError):
        mpk.dilu4dev_plan_probe(2, [0, 1, 2], [0, 1], order="rcm")


# ---------------------------------------------------------------- the dropped cases are what they are there for

@pytest.mark.parametrize("name", DC.NAMES)
def test_a_dropped_case_loses_u_blocks_only_and_keeps_its_forward_schedule(name):
    from navierstokes_amd import mpk
    nb, bp, bc, bv = LC.matrix(name)
    db, dp, dc, dv = DC.dropped(name)
    assert db == nb and len(dc) < len(bc) and dv.size == 16 * len(dc)
    kept = {(i, int(dc[k])): k for i in range(nb) for k in range(dp[i], dp[i + 1])}
    blocks = np.asarray(bv).reshape(-1, 16)
    for i in range(nb):
        for k in range(bp[i], bp[i + 1]):
            j = int(bc[k])
            gone = j > i and (i + j) % 3 == 0
            assert ((i, j) in kept) != gone, (i, j)
            if not gone:
                assert_bit_equal(dv.reshape(-1, 16)[kept[(i, j)]], blocks[k], f"block ({i}, {j})")
    full, drop = mpk.bilu4_plan_probe(nb, bp, bc, 0), mpk.bilu4_plan_probe(nb, dp, dc, 0)
    assert list(drop["fwd_sizes"]) == list(full["fwd_sizes"]) and drop["fwd_launches"] == full["fwd_launches"]
    if name == "wide":
        assert list(drop["fwd_sizes"]) == list(W.WIDTHS) and (min(W.WIDTHS), max(W.WIDTHS)) == (63, 129)
    if name == "alternating":
        assert list(drop["fwd_sizes"]) == list(C.ALTERNATING_WIDTHS) and drop["fwd_launches"] == len(C.ALTERNATING_WIDTHS)
    DC.assert_census(name)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", DC.NAMES)
def test_a_dropped_case_factors_with_both_value_sets(name, order):
    """The model's pivots exist (no refusal) and the host handle's are the model's, bit for bit, for values 0 and 1."""
    from navierstokes_amd import mpk
    nb, bp, bc, _ = DC.dropped(name)
    E = mpk.dilu4(nb, bp, bc, DC.values(name), host_only=True, order=order)
    for variant in (0, 1):
        if variant:
            E.refactor(DC.values(name, variant))
        einv, k = E.fetch()
        weinv, wk = DC.model(name, order, variant).fetch()
        assert_bit_equal(einv, weinv, f"{name} {order} values {variant}: Einv")
        assert_bit_equal(k, wk, f"{name} {order} values {variant}: K")
    assert not np.array_equal(DC.model(name, order, 0).fetch()[0], DC.model(name, order, 1).fetch()[0])
    E.close()


def test_an_unmated_block_changes_the_pivots():
    """Were the `mate < 0` term not skipped but taken with SOME U block, or a mated term skipped, the pivots would differ: the
    model of the dropped pattern differs from the model of the full one on rows that lost a mate, and only there and downstream."""
    name = "wide"
    full, drop = LC.model(name, "natural").B, DC.model(name, "natural").B
    rows = DC.mated(drop.nb, drop.ptr, drop.col)
    lost = np.array([bool(m) and not all(m) for m in rows])
    differs = (full.einv.reshape(drop.nb, -1).view(np.uint64) != drop.einv.reshape(drop.nb, -1).view(np.uint64)).any(axis=1)
    assert differs[lost].all()
