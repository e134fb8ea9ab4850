"""The C-ABI of the exact block ILU solve over the single-precision copy of the factor (mi_bilu4spx_*) and of
mi_gmres_set_precond_ex on a box without a GPU: the exports are declared, exported and bound; the three mi_bilu4spx_* names are a
closed set; the argument rules hold before the device is touched; a host-only handle (the only kind such a box can make) is refused
with MI_ERR_NODEVICE; an empty matrix makes every call a no-op."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "navierstokes_amd", "csrc", "libmi355spmv.so")
SPX = ("mi_bilu4spx_solve_dev", "mi_bilu4spx_solve", "mi_bilu4spx_info")
SYMBOLS = SPX + ("mi_gmres_set_precond_ex",)
MI_ERR_ARG, MI_ERR_NODEVICE = 1, 2


def test_exports_are_declared_and_bound():
    assert os.path.exists(LIB), "libmi355spmv.so not built (run __graft_entry__.build())"
    raw = ctypes.CDLL(LIB)
    src = open(os.path.join(ROOT, "include", "mi355_spmv.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert set(re.findall(r"\b(mi_bilu4spx_[a-z0-9_]+)\s*\(", hdr)) == set(SPX)
    from navierstokes_amd import mpk
    L = mpk.lib()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), f"{s} is not declared in include/mi355_spmv.h"
        assert hasattr(raw, s), f"{s} is not exported"
        assert getattr(L, s).argtypes, f"{s} is not bound in mpk.py"
    assert re.search(r"\bMI_GMRES_PC_EXACT_F32\s*=\s*3\b", hdr), "MI_GMRES_PC_EXACT_F32 = 3 is not in the header"
    assert mpk.GMRES_PC_EXACT_F32 == 3
    for name in ("exact", "exact_info_f32"):
        assert hasattr(mpk.bilu4, name), name
    assert L.mi_version() == 501  # additive: nothing changed for a caller built against 0.5.1
    # the definition is part of the interface: it stands in the header
    doc = src[src.index("(mi_bilu4spx_*) ----"):src.index("int mi_bilu4spx_solve_dev")]
    for word in ("v32 = (double)(float)v", "L, U and the inverted diagonal blocks", "BIT FOR BIT", "level by level", "MI_ERR_STATE", "MI_ERR_NODEVICE",
                 "d_x == d_b is allowed", "8-byte alignment"):
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
    for call, word in ((lambda: L.mi_bilu4spx_solve_dev(None, vp, vp, None), "null handle"), (lambda: L.mi_bilu4spx_solve(None, vp, vp), "null handle"),
                       (lambda: L.mi_bilu4spx_info(None, None, None), "null handle"),
                       (lambda: L.mi_bilu4spx_solve_dev(F.handle, None, vp, None), "null vector"), (lambda: L.mi_bilu4spx_solve_dev(F.handle, vp, None, None), "null vector"),
                       (lambda: L.mi_bilu4spx_solve(F.handle, None, vp), "null vector"), (lambda: L.mi_bilu4spx_solve(F.handle, vp, None), "null vector"),
                       (lambda: L.mi_gmres_set_precond_ex(None, F.handle, 3, 0, 0), "null handle")):
        assert call() == MI_ERR_ARG, word
        assert word in L.mi_last_error().decode(), (word, L.mi_last_error())
    for bad in ("f16", "F32", "double", "", None):
        with pytest.raises(ValueError):
            F.exact(bad)
    assert F.exact("f64") is F and F.exact() is F
    view = F.exact("f32")
    assert view.F is F and not hasattr(view, "close"), "the view shares the handle and owns nothing"
    assert (v == 1.0).all()
    F.close()
    with pytest.raises(ValueError):
        view.solve(v, v)


def test_a_host_only_handle_is_refused_with_nodevice():
    from navierstokes_amd import mpk
    L = mpk.lib()
    F = _host_handle()
    v, x = np.ones(8), np.full(8, 7.0)
    for call in (lambda: L.mi_bilu4spx_solve_dev(F.handle, v.ctypes.data, x.ctypes.data, None), lambda: L.mi_bilu4spx_solve(F.handle, v.ctypes.data, x.ctypes.data)):
        assert call() == MI_ERR_NODEVICE
        assert "host-only" in L.mi_last_error().decode() and "no CPU fallback" in L.mi_last_error().decode()
    with pytest.raises(mpk.MiError) as e:
        F.exact("f32").solve(x, v)
    assert e.value.status == MI_ERR_NODEVICE
    assert (x == 7.0).all() and (v == 1.0).all(), "a refused call wrote"
    assert F.exact_info_f32() == dict(launches_last=0, wide_launches_last=0)
    assert L.mi_bilu4spx_info(F.handle, None, None) == 0
    assert F.sweep_info_f32() == dict(prepared=False, convert_launches=0, launches_last=0, copy_bytes=0)
    F.close()


def test_set_precond_ex_refuses_what_it_does_not_know():
    """Kind 4, and a negative count for the two sweep kinds: refused before the solver is looked at, so a box that cannot make a
    solver sees it too.  Kinds 0 and 3 ignore the counts; without a preconditioner kind and counts are ignored."""
    from navierstokes_amd import mpk
    L = mpk.lib()
    F = _host_handle()
    for args, word in (((4, 0, 0), "unknown preconditioner kind"), ((-1, 0, 0), "unknown preconditioner kind"), ((2 ** 31 - 1, 0, 0), "unknown preconditioner kind"),
                       ((1, -1, 0), "negative sweep count"), ((1, 0, -1), "negative sweep count"), ((2, -1, 0), "negative sweep count"),
                       ((2, 0, -1), "negative sweep count"), ((0, -1, -1), "null handle"), ((3, -1, -1), "null handle"), ((1, 0, 0), "null handle")):
        assert L.mi_gmres_set_precond_ex(None, F.handle, *args) == MI_ERR_ARG, args
        assert word in L.mi_last_error().decode(), (args, L.mi_last_error())
    assert L.mi_gmres_set_precond_ex(None, None, 4, -1, -1) == MI_ERR_ARG and "null handle" in L.mi_last_error().decode()
    # the function it stands behind refuses in the order it always has: the handle first
    assert L.mi_gmres_set_precond(None, F.handle, 3, 0, 0) == MI_ERR_ARG and "null handle" in L.mi_last_error().decode()
    F.close()


def test_an_empty_matrix_makes_every_call_a_no_op():
    from navierstokes_amd import mpk
    L = mpk.lib()
    F = mpk.bilu4(0, [0], [], [], host_only=True)
    e = np.zeros(0)
    assert L.mi_bilu4spx_solve(F.handle, e.ctypes.data, e.ctypes.data) == 0
    assert L.mi_bilu4spx_solve_dev(F.handle, None, None, None) == 0
    assert F.exact("f32").solve(e, e) is e
    assert F.exact_info_f32() == dict(launches_last=0, wide_launches_last=0)
    F.close()
