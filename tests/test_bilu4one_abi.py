"""The C-ABI of the one-launch block ILU solve on a box without a GPU: the five exports are declared, exported and bound; the
argument rules hold before the device is touched; a host-only handle has no device form; an empty matrix makes every call a no-op."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "navierstokes_amd", "csrc", "libmi355spmv.so")
SYMBOLS = ("mi_bilu4one_plan_probe", "mi_bilu4one_prepare", "mi_bilu4_set_solve_form", "mi_bilu4one_status", "mi_bilu4one_info")
MI_ERR_ARG, MI_ERR_STATE = 1, 6


def test_exports_are_declared_and_bound():
    assert os.path.exists(LIB), "libmi355spmv.so not built (run __graft_entry__.build())"
    raw = ctypes.CDLL(LIB)
    src = open(os.path.join(ROOT, "include", "mi355_spmv.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\bint\s*\(?\s*%s\s*\)?\s*\(" % s, hdr), f"{s} is not declared in include/mi355_spmv.h"
        assert hasattr(raw, s), f"{s} is not exported"
    assert set(re.findall(r"\b(mi_bilu4one_[a-z0-9_]+)\s*\(", hdr)) == {s for s in SYMBOLS if s.startswith("mi_bilu4one_")}
    assert re.search(r"MI_BILU_FORM_LEVELS = 0, MI_BILU_FORM_ONE = 1, MI_BILU_FORM_AUTO = -1", hdr)
    from navierstokes_amd import mpk
    L = mpk.lib()
    for s in SYMBOLS:
        assert getattr(L, s).argtypes, f"{s} is not bound in mpk.py"
    for name in ("set_form", "info_one", "prepare_one", "one_status"):
        assert hasattr(mpk.bilu4, name), name
    assert hasattr(mpk, "bilu4one_plan_probe")
    assert L.mi_version() == 501  # additive: nothing changed for a caller built against 0.5.1
    assert "baij4_solve.c:4-93" in src[src.index("mi_bilu4one_*, mi_bilu4_set_solve_form"):src.index("enum { MI_BILU_FORM_LEVELS")]


def _host_handle():
    from navierstokes_amd import mpk
    eye, off = np.eye(4).reshape(-1) * 2, np.ones(16) * 0.1
    return mpk.bilu4(2, [0, 2, 4], [0, 1, 0, 1], np.concatenate([eye, off, off, eye]), host_only=True)


def test_argument_rules_hold_before_the_device_is_touched():
    from navierstokes_amd import mpk
    L = mpk.lib()
    F = _host_handle()
    for call, word in ((lambda: L.mi_bilu4one_prepare(None), "null handle"), (lambda: L.mi_bilu4_set_solve_form(None, 0), "null handle"),
                       (lambda: L.mi_bilu4_set_solve_form(None, 1), "null handle"), (lambda: L.mi_bilu4one_status(None), "null handle"),
                       (lambda: L.mi_bilu4one_info(None, *([None] * 6)), "null handle"),
                       (lambda: L.mi_bilu4_set_solve_form(F.handle, 2), "unknown solve form"), (lambda: L.mi_bilu4_set_solve_form(F.handle, -2), "unknown solve form"),
                       (lambda: L.mi_bilu4_set_solve_form(F.handle, 7), "unknown solve form")):
        assert call() == MI_ERR_ARG, word
        assert word in L.mi_last_error().decode(), (word, L.mi_last_error())
    with pytest.raises(mpk.MiError) as e:
        F.set_form(2)
    assert e.value.status == MI_ERR_ARG
    F.close()


def test_a_host_only_handle_has_no_one_launch_form():
    from navierstokes_amd import mpk
    L = mpk.lib()
    F = _host_handle()
    before = F.factor_host()[3].copy()
    for call in (lambda: L.mi_bilu4one_prepare(F.handle), lambda: L.mi_bilu4_set_solve_form(F.handle, 0), lambda: L.mi_bilu4_set_solve_form(F.handle, 1),
                 lambda: L.mi_bilu4_set_solve_form(F.handle, -1), lambda: L.mi_bilu4one_status(F.handle)):
        assert call() == MI_ERR_STATE
        assert "host-only" in L.mi_last_error().decode()
    for method in (lambda: F.set_form(1), F.one_status):
        with pytest.raises(mpk.MiError) as e:
            method()
        assert e.value.status == MI_ERR_STATE
    assert F.info_one() == dict(prepared=False, eligible=False, workgroups=0, nchunks=(0, 0), max_deps=(0, 0), plan_bytes=0)
    assert L.mi_bilu4one_info(F.handle, *([None] * 6)) == 0
    info = F.info()
    assert info["form"] == 0 and info["launches"] == 2 and info["us_one_launch"] == 0.0  # untouched: one folded launch per sweep
    assert np.array_equal(F.factor_host()[3], before)
    F.close()
    with pytest.raises(ValueError):
        F.set_form(0)


def test_an_empty_matrix_makes_every_call_a_no_op():
    from navierstokes_amd import mpk
    L = mpk.lib()
    F = mpk.bilu4(0, [0], [], [], host_only=True)
    assert L.mi_bilu4one_prepare(F.handle) == 0 and L.mi_bilu4one_status(F.handle) == 0
    for form in (0, 1, -1):
        assert L.mi_bilu4_set_solve_form(F.handle, form) == 0
        assert F.info()["form"] == 0
    assert L.mi_bilu4_set_solve_form(F.handle, 2) == MI_ERR_ARG
    assert F.info_one()["prepared"] is False
    assert mpk.bilu4one_plan_probe(0, [0], [], 0)["nchunks"] == (0, 0)
    F.close()
