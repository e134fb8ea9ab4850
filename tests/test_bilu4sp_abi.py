"""The C-ABI of the sweeps over the single-precision copy of the block ILU factor (mi_bilu4sp_*) on a box without a GPU: the six
exports are declared, exported and bound; the argument rules hold before the device is touched; a host-only handle (the only kind
such a box can make) is refused with MI_ERR_NODEVICE: there is no CPU fallback; an empty matrix makes every call a no-op."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "navierstokes_amd", "csrc", "libmi355spmv.so")
SYMBOLS = ("mi_bilu4sp_prepare", "mi_bilu4sp_solve_dev", "mi_bilu4sp_solve", "mi_bilu4sp_status", "mi_bilu4sp_fetch", "mi_bilu4sp_info")
MI_ERR_ARG, MI_ERR_NODEVICE = 1, 2


def test_exports_are_declared_and_bound():
    assert os.path.exists(LIB), "libmi355spmv.so not built (run __graft_entry__.build())"
    raw = ctypes.CDLL(LIB)
    src = open(os.path.join(ROOT, "include", "mi355_spmv.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert set(re.findall(r"\b(mi_bilu4sp_[a-z0-9_]+)\s*\(", hdr)) == set(SYMBOLS)
    from navierstokes_amd import mpk
    L = mpk.lib()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), f"{s} is not declared in include/mi355_spmv.h"
        assert hasattr(raw, s), f"{s} is not exported"
        assert getattr(L, s).argtypes, f"{s} is not bound in mpk.py"
    for name in ("sweep_status_f32", "fetch_f32", "sweep_info_f32"):
        assert hasattr(mpk.bilu4, name), name
    assert L.mi_version() == 501  # additive: nothing changed for a caller built against 0.5.1
    # the definition is part of the interface: it stands in the header
    doc = src[src.index("(mi_bilu4sp_*) ----"):src.index("int mi_bilu4sp_prepare")]
    for word in ("v32 = (double)(float)v", "ties to EVEN", "SUBNORMALS are kept", "+-Inf", "CLAMPED", "BIT FOR BIT", "64 bytes per block", "never read it",
                 "ONE sweep solve of EITHER precision at a time per handle", "MI_ERR_NODEVICE"):
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
    f32 = np.zeros(4 * 16, np.float32)
    for call, word in ((lambda: L.mi_bilu4sp_prepare(None), "null handle"), (lambda: L.mi_bilu4sp_solve_dev(None, vp, vp, 1, 1, None), "null handle"),
                       (lambda: L.mi_bilu4sp_solve(None, vp, vp, 1, 1), "null handle"), (lambda: L.mi_bilu4sp_info(None, *([None] * 4)), "null handle"),
                       (lambda: L.mi_bilu4sp_status(None, None, None), "null handle"), (lambda: L.mi_bilu4sp_fetch(None, f32.ctypes.data, 4), "null handle"),
                       (lambda: L.mi_bilu4sp_solve_dev(F.handle, vp, vp, -1, 1, None), "negative sweep count"),
                       (lambda: L.mi_bilu4sp_solve_dev(F.handle, vp, vp, 1, -1, None), "negative sweep count"),
                       (lambda: L.mi_bilu4sp_solve(F.handle, vp, vp, -(2 ** 31), 0), "negative sweep count"),
                       (lambda: L.mi_bilu4sp_solve(F.handle, vp, vp, 0, -1), "negative sweep count"),
                       (lambda: L.mi_bilu4sp_solve_dev(F.handle, None, vp, 1, 1, None), "null vector"),
                       (lambda: L.mi_bilu4sp_solve_dev(F.handle, vp, None, 1, 1, None), "null vector"),
                       (lambda: L.mi_bilu4sp_solve(F.handle, None, vp, 1, 1), "null vector"), (lambda: L.mi_bilu4sp_solve(F.handle, vp, None, 1, 1), "null vector"),
                       (lambda: L.mi_bilu4sp_fetch(F.handle, None, 4), "null val")):
        assert call() == MI_ERR_ARG, word
        assert word in L.mi_last_error().decode(), (word, L.mi_last_error())
    with pytest.raises(ValueError):
        F.sweeps(-1, precision="f32")
    with pytest.raises(ValueError):
        F.sweeps(1, -2, precision="f32")
    for bad in ("f16", "F32", "double", "", None):
        with pytest.raises(ValueError):
            F.sweeps(1, precision=bad)
        with pytest.raises(ValueError):
            F.prepare_sweeps(precision=bad)
    assert (v == 1.0).all()
    F.close()


def test_a_host_only_handle_is_refused_with_nodevice():
    from navierstokes_amd import mpk
    L = mpk.lib()
    F = _host_handle()
    v, x = np.ones(8), np.full(8, 7.0)
    f32 = np.full(4 * 16, 7.0, np.float32)
    bad, cnt = ctypes.c_int(5), ctypes.c_longlong(5)
    for call in (lambda: L.mi_bilu4sp_prepare(F.handle), lambda: L.mi_bilu4sp_solve_dev(F.handle, v.ctypes.data, x.ctypes.data, 1, 1, None),
                 lambda: L.mi_bilu4sp_solve(F.handle, v.ctypes.data, x.ctypes.data, 0, 0), lambda: L.mi_bilu4sp_solve(F.handle, v.ctypes.data, x.ctypes.data, 10 ** 6, 3),
                 lambda: L.mi_bilu4sp_status(F.handle, ctypes.byref(bad), ctypes.byref(cnt)), lambda: L.mi_bilu4sp_fetch(F.handle, f32.ctypes.data, 4)):
        assert call() == MI_ERR_NODEVICE
        assert "host-only" in L.mi_last_error().decode() and "no CPU fallback" in L.mi_last_error().decode()
    assert (bad.value, cnt.value) == (-1, 0)
    for method in (lambda: F.sweeps(2, precision="f32").solve(x, v), lambda: F.sweeps(0, 3, precision="f32").solve(x, v), lambda: F.prepare_sweeps(precision="f32"),
                   F.sweep_status_f32, F.fetch_f32):
        with pytest.raises(mpk.MiError) as e:
            method()
        assert e.value.status == MI_ERR_NODEVICE
    assert (x == 7.0).all() and (v == 1.0).all() and (f32 == 7.0).all(), "a refused call wrote"
    assert F.sweep_info_f32() == dict(prepared=False, convert_launches=0, launches_last=0, copy_bytes=0)
    assert F.sweep_info() == dict(prepared=False, max_fwd=1, max_bwd=1, launches_last=0, work_bytes=0)
    assert L.mi_bilu4sp_info(F.handle, *([None] * 4)) == 0
    view = F.sweeps(3, precision="f32")
    assert (view.fwd, view.bwd, view.precision) == (3, 3, "f32") and F.sweeps(3, 0).precision == "f64"
    F.close()
    with pytest.raises(ValueError):
        view.solve(x, v)


def test_an_empty_matrix_makes_every_call_a_no_op():
    from navierstokes_amd import mpk
    L = mpk.lib()
    F = mpk.bilu4(0, [0], [], [], host_only=True)
    e = np.zeros(0)
    assert L.mi_bilu4sp_prepare(F.handle) == 0
    assert L.mi_bilu4sp_solve(F.handle, e.ctypes.data, e.ctypes.data, 2, 2) == 0
    assert L.mi_bilu4sp_solve_dev(F.handle, None, None, 2, 2, None) == 0
    assert L.mi_bilu4sp_solve_dev(F.handle, None, None, -2, 2, None) == MI_ERR_ARG
    assert L.mi_bilu4sp_status(F.handle, None, None) == 0
    assert L.mi_bilu4sp_fetch(F.handle, None, 0) == 0
    assert F.fetch_f32().shape == (0, 4, 4) and F.sweep_status_f32() is F
    assert F.sweep_info_f32() == dict(prepared=False, convert_launches=0, launches_last=0, copy_bytes=0)
    F.close()
