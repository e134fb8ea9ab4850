"""The C-ABI of the block ILU's device refactor (mi_bilu4dev_*) on a box without a GPU: the six exports are declared, exported
and bound; the argument rules hold before the device is touched; the plan probe's counts equal those worked out in Python from
the model's pattern (tests/bilu4_model.py), for every small case of tests/bilu4_cases.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import bilu4_cases as C
import bilu4_model as M
from conftest import ROOT

LIB = os.path.join(ROOT, "navierstokes_amd", "csrc", "libmi355spmv.so")
SYMBOLS = ("mi_bilu4dev_plan_probe", "mi_bilu4dev_prepare", "mi_bilu4dev_refactor", "mi_bilu4dev_status", "mi_bilu4dev_fetch",
           "mi_bilu4dev_info")
FIXED_LAUNCHES = 1  # include/mi355_spmv.h: "launches per refactor = forward launches + 1"
MI_ERR_ARG, MI_ERR_STATE = 1, 6
PROBE_CASES = C.SHAPE_CASES + C.RANDOM_CASES + C.LAYERED_CASES + C.WIDE_CASES + [(f"fe:{nx}", fill) for nx in (3, 6) for fill in (0, 1, 2)]


def test_exports_are_declared_and_bound():
    assert os.path.exists(LIB), "libmi355spmv.so not built (run __graft_entry__.build())"
    raw = ctypes.CDLL(LIB)
    src = open(os.path.join(ROOT, "include", "mi355_spmv.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mi_bilu4dev_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(SYMBOLS), declared ^ set(SYMBOLS)
    from navierstokes_amd import mpk
    L = mpk.lib()
    for s in SYMBOLS:
        assert hasattr(raw, s), f"{s} is not exported"
        assert getattr(L, s).argtypes, f"{s} is not bound in mpk.py"
    for name in ("prepare_dev", "refactor_dev", "factor_status", "fetch_factor", "info_dev"):
        assert hasattr(mpk.bilu4, name), name
    assert hasattr(mpk, "bilu4dev_plan_probe")
    assert L.mi_version() == 501
    assert "forward launches + 1" in src and "mi_bilu4dev_* (the" in src
    # every entry cites the reference's factorisation and the Newton step that calls it, like its neighbours
    for s in SYMBOLS:
        comment = src[:src.index(f"int {s}(")].rsplit("/*", 1)[1]
        for cite in ("baij4_factor_avx2.c:114-170", "solve_newton.c:1257"):
            assert cite in comment, f"{s}: the header does not cite {cite}"


def _host_handle():
    from navierstokes_amd import mpk
    eye, off = np.eye(4).reshape(-1) * 2, np.ones(16) * 0.1
    return mpk.bilu4(2, [0, 2, 4], [0, 1, 0, 1], np.concatenate([eye, off, off, eye]), host_only=True)


def test_argument_rules_hold_before_the_device_is_touched():
    from navierstokes_amd import mpk
    L = mpk.lib()
    F = _host_handle()
    v = np.ones(64)
    vp = v.ctypes.data
    bad = ctypes.c_int(5)
    for call, word in ((lambda: L.mi_bilu4dev_prepare(None), "null handle"), (lambda: L.mi_bilu4dev_refactor(None, vp, 0, None), "null handle"),
                       (lambda: L.mi_bilu4dev_refactor(F.handle, None, 0, None), "null coef"),
                       (lambda: L.mi_bilu4dev_refactor(F.handle, vp, 7, None), "layout"), (lambda: L.mi_bilu4dev_refactor(F.handle, vp, -1, None), "layout"),
                       (lambda: L.mi_bilu4dev_status(None, ctypes.byref(bad)), "null handle"), (lambda: L.mi_bilu4dev_fetch(None), "null handle"),
                       (lambda: L.mi_bilu4dev_info(None, None, None, None), "null handle")):
        assert call() == MI_ERR_ARG, word
        assert word in L.mi_last_error().decode(), (word, L.mi_last_error())
    F.close()


def test_a_host_only_handle_has_no_device_refactor():
    from navierstokes_amd import mpk
    L = mpk.lib()
    F = _host_handle()
    before = F.factor_host()[3].copy()
    v = np.ones(64)
    bad = ctypes.c_int(5)
    for call in (lambda: L.mi_bilu4dev_prepare(F.handle), lambda: L.mi_bilu4dev_refactor(F.handle, v.ctypes.data, 0, None),
                 lambda: L.mi_bilu4dev_status(F.handle, ctypes.byref(bad)), lambda: L.mi_bilu4dev_fetch(F.handle)):
        assert call() == MI_ERR_STATE
        assert "host-only" in L.mi_last_error().decode()
    for method in (F.prepare_dev, F.factor_status, F.fetch_factor):
        with pytest.raises(mpk.MiError) as e:
            method()
        assert e.value.status == MI_ERR_STATE
    info = F.info_dev()
    assert info == dict(prepared=False, launches=1 + FIXED_LAUNCHES, plan_bytes=0)  # two block rows: one folded launch
    assert L.mi_bilu4dev_info(F.handle, None, None, None) == 0
    assert np.array_equal(F.factor_host()[3], before) and (v == 1.0).all()
    F.close()
    with pytest.raises(ValueError):
        F.prepare_dev()


def test_an_empty_matrix_makes_every_call_a_no_op():
    from navierstokes_amd import mpk
    L = mpk.lib()
    F = mpk.bilu4(0, [0], [], [], host_only=True)
    bad = ctypes.c_int(5)
    assert L.mi_bilu4dev_prepare(F.handle) == 0 and L.mi_bilu4dev_refactor(F.handle, None, 0, None) == 0
    assert L.mi_bilu4dev_status(F.handle, ctypes.byref(bad)) == 0 and bad.value == -1
    assert L.mi_bilu4dev_fetch(F.handle) == 0
    assert F.info_dev()["prepared"] is False
    assert mpk.bilu4dev_plan_probe(0, [0], [], 0)["update_pairs"] == 0
    F.close()


def _update_pairs(nb, ptr, col, diag):
    """Sum over rows i and L blocks k of row i of the U columns of row col[k] that occur in row i."""
    rows = [set(col[ptr[i]:ptr[i + 1]].tolist()) for i in range(nb)]
    upper = [col[diag[i] + 1:ptr[i + 1]].tolist() for i in range(nb)]
    return sum(sum(j in rows[i] for j in upper[p]) for i in range(nb) for p in col[ptr[i]:diag[i]].tolist())


@pytest.mark.parametrize("case", PROBE_CASES, ids=C.case_id)
def test_plan_probe_counts_equal_the_model_pattern(case):
    from navierstokes_amd import mpk
    name, fill = case
    nb, bp, bc, _ = C.matrix(name)
    got = mpk.bilu4dev_plan_probe(nb, bp, bc, fill)
    ptr, col, diag = M.symbolic(nb, bp, bc, fill)
    assert got["update_pairs"] == _update_pairs(nb, np.asarray(ptr), np.asarray(col), np.asarray(diag))
    assert got["launches"] == mpk.bilu4_plan_probe(nb, bp, bc, fill)["fwd_launches"] + FIXED_LAUNCHES
    assert got["plan_bytes"] > 0


def test_bad_patterns_are_refused_with_the_plan_probe_s_messages():
    from navierstokes_amd import mpk
    L = mpk.lib()
    i32 = lambda a: np.array(a, np.int32)
    cases = [(2, i32([0, 1, 2]), i32([0, 1]), -1), (-1, i32([0]), i32([0]), 0), (2, i32([1, 2, 3]), i32([0, 0, 1]), 0), (2, i32([0, 2, 1]), i32([0, 1]), 0),
             (2, i32([0, 1, 2]), i32([0, 2]), 0), (2, i32([0, 2, 3]), i32([1, 0, 1]), 0), (2, i32([0, 2, 3]), i32([0, 0, 1]), 0),
             (2, i32([0, 1, 2]), i32([0, 0]), 0)]
    for nb, p, c, fill in cases:
        assert L.mi_bilu4_plan_probe(nb, p.ctypes.data, c.ctypes.data, fill, *([None] * 7), 0) == MI_ERR_ARG
        want = L.mi_last_error().decode()
        assert L.mi_bilu4dev_plan_probe(nb, p.ctypes.data, c.ctypes.data, fill, None, None, None) == MI_ERR_ARG
        assert L.mi_last_error().decode() == want and want
    assert L.mi_bilu4dev_plan_probe(2, None, None, 0, None, None, None) == MI_ERR_ARG and "null ptrow" in L.mi_last_error().decode()
    with pytest.raises(mpk.MiError):
        mpk.bilu4dev_plan_probe(2, [0, 1, 2], [0, 0], 0)
