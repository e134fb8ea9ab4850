"""The C-ABI of the sweep solve of the block ILU (mi_bilu4sw_*) on a box without a GPU: the four exports are declared, exported and
bound; the argument rules hold before the device is touched; a host-only handle (the only kind such a box can make) is refused with
MI_ERR_NODEVICE: there is no CPU fallback; an empty matrix makes every call a no-op."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "navierstokes_amd", "csrc", "libmi355spmv.so")
SYMBOLS = ("mi_bilu4sw_prepare", "mi_bilu4sw_solve_dev", "mi_bilu4sw_solve", "mi_bilu4sw_info")
MI_ERR_ARG, MI_ERR_NODEVICE = 1, 2


def test_exports_are_declared_and_bound():
    assert os.path.exists(LIB), "libmi355spmv.so not built (run __graft_entry__.build())"
    raw = ctypes.CDLL(LIB)
    src = open(os.path.join(ROOT, "include", "mi355_spmv.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert set(re.findall(r"\b(mi_bilu4sw_[a-z0-9_]+)\s*\(", hdr)) == set(SYMBOLS)
    from navierstokes_amd import mpk
    L = mpk.lib()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), f"{s} is not declared in include/mi355_spmv.h"
        assert hasattr(raw, s), f"{s} is not exported"
        assert getattr(L, s).argtypes, f"{s} is not bound in mpk.py"
    for name in ("sweeps", "sweep_info", "prepare_sweeps"):
        assert hasattr(mpk.bilu4, name), name
    assert L.mi_version() == 501  # additive: nothing changed for a caller built against 0.5.1
    # the definition is part of the interface: it stands in the header
    doc = src[src.index("(mi_bilu4sw_*) ----"):src.index("int mi_bilu4sw_prepare")]
    for word in ("t^0 = b", "x^0_i = Dinv_i . t^{sf}_i", "CLAMPED", "BIT FOR BIT", "ONE sweep solve at a time per handle", "MI_ERR_NODEVICE"):
        assert word in doc, word


def _host_handle():
    from navierstokes_amd import mpk
    eye, off = np.eye(4).reshape(-1) * 2, np.ones(16) * 0.1
    return mpk.bilu4(2, [0, 2, 4], [0, 1, 0, 1], np.concatenate([eye, off, off, eye]), host_only=True)


def test_argument_rules_hold_before_the_device_is_touched():
    from navierstokes_amd import mpk
    L = mpk.lib()
    F = _host_handle()
    v = np.ones(8)
    vp = v.ctypes.data
    for call, word in ((lambda: L.mi_bilu4sw_prepare(None), "null handle"), (lambda: L.mi_bilu4sw_solve_dev(None, vp, vp, 1, 1, None), "null handle"),
                       (lambda: L.mi_bilu4sw_solve(None, vp, vp, 1, 1), "null handle"), (lambda: L.mi_bilu4sw_info(None, *([None] * 5)), "null handle"),
                       (lambda: L.mi_bilu4sw_solve_dev(F.handle, vp, vp, -1, 1, None), "negative sweep count"),
                       (lambda: L.mi_bilu4sw_solve_dev(F.handle, vp, vp, 1, -1, None), "negative sweep count"),
                       (lambda: L.mi_bilu4sw_solve(F.handle, vp, vp, -(2 ** 31), 0), "negative sweep count"),
                       (lambda: L.mi_bilu4sw_solve(F.handle, vp, vp, 0, -1), "negative sweep count"),
                       (lambda: L.mi_bilu4sw_solve_dev(F.handle, None, vp, 1, 1, None), "null vector"),
                       (lambda: L.mi_bilu4sw_solve_dev(F.handle, vp, None, 1, 1, None), "null vector"),
                       (lambda: L.mi_bilu4sw_solve(F.handle, None, vp, 1, 1), "null vector"), (lambda: L.mi_bilu4sw_solve(F.handle, vp, None, 1, 1), "null vector")):
        assert call() == MI_ERR_ARG, word
        assert word in L.mi_last_error().decode(), (word, L.mi_last_error())
    with pytest.raises(ValueError):
        F.sweeps(-1)
    with pytest.raises(ValueError):
        F.sweeps(1, -2)
    assert (v == 1.0).all()
    F.close()


def test_a_host_only_handle_is_refused_with_nodevice():
    from navierstokes_amd import mpk
    L = mpk.lib()
    F = _host_handle()
    v, x = np.ones(8), np.full(8, 7.0)
    for call in (lambda: L.mi_bilu4sw_prepare(F.handle), lambda: L.mi_bilu4sw_solve_dev(F.handle, v.ctypes.data, x.ctypes.data, 1, 1, None),
                 lambda: L.mi_bilu4sw_solve(F.handle, v.ctypes.data, x.ctypes.data, 0, 0), lambda: L.mi_bilu4sw_solve(F.handle, v.ctypes.data, x.ctypes.data, 10 ** 6, 3)):
        assert call() == MI_ERR_NODEVICE
        assert "host-only" in L.mi_last_error().decode() and "no CPU fallback" in L.mi_last_error().decode()
    for method in (lambda: F.sweeps(2).solve(x, v), lambda: F.sweeps(0, 3).solve(x, v), F.prepare_sweeps):
        with pytest.raises(mpk.MiError) as e:
            method()
        assert e.value.status == MI_ERR_NODEVICE
    assert (x == 7.0).all() and (v == 1.0).all(), "a refused solve wrote"
    # two block rows, each depending on the other in one sweep: two levels per sweep, so one sweep per triangle is exact
    assert F.sweep_info() == dict(prepared=False, max_fwd=1, max_bwd=1, launches_last=0, work_bytes=0)
    assert L.mi_bilu4sw_info(F.handle, *([None] * 5)) == 0
    view = F.sweeps(3)
    assert (view.fwd, view.bwd) == (3, 3) and (F.sweeps(3, 0).fwd, F.sweeps(3, 0).bwd) == (3, 0)
    assert F.info()["form"] == 0
    F.close()
    with pytest.raises(ValueError):
        view.solve(x, v)


def test_an_empty_matrix_makes_every_call_a_no_op():
    from navierstokes_amd import mpk
    L = mpk.lib()
    F = mpk.bilu4(0, [0], [], [], host_only=True)
    e = np.zeros(0)
    assert L.mi_bilu4sw_prepare(F.handle) == 0
    assert L.mi_bilu4sw_solve(F.handle, e.ctypes.data, e.ctypes.data, 2, 2) == 0
    assert L.mi_bilu4sw_solve_dev(F.handle, None, None, 2, 2, None) == 0
    assert L.mi_bilu4sw_solve_dev(F.handle, None, None, -2, 2, None) == MI_ERR_ARG
    assert F.sweep_info() == dict(prepared=False, max_fwd=0, max_bwd=0, launches_last=0, work_bytes=0)
    F.close()
