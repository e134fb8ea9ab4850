"""The C-ABI of the float Krylov basis (mi_gmres_create_ex, mi_gmres_basis_info, mi_round_f32_dev, mi_mdot_f32_dev, mi_maxpy_f32_dev,
mi_cgs_f32_dev) on a box without a GPU: the library exports the symbols the header declares, the header section holds the
definition, every argument rule is refused with MI_ERR_ARG and a message before the device is touched and with nothing written,
and the compute calls fail with MI_ERR_NODEVICE instead of falling back.  The bits are in tests/test_gpu_gmres_f32.py."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "navierstokes_amd", "csrc", "libmi355spmv.so")
SYMBOLS = ("mi_gmres_create_ex", "mi_gmres_basis_info", "mi_round_f32_dev", "mi_mdot_f32_dev", "mi_maxpy_f32_dev", "mi_cgs_f32_dev")
MI_ERR_ARG, MI_ERR_NODEVICE = 1, 2
MI_BASIS_F64, MI_BASIS_F32 = 0, 1


def test_library_exports_the_symbols_and_the_header_defines_the_basis():
    assert os.path.exists(LIB), "libmi355spmv.so not built (run __graft_entry__.build())"
    L = ctypes.CDLL(LIB)
    missing = [s for s in SYMBOLS if not hasattr(L, s)]
    assert not missing, missing
    hdr = open(os.path.join(ROOT, "include", "mi355_spmv.h")).read()
    for s in SYMBOLS:
        assert f"int {s}(" in hdr, f"{s} is not declared in include/mi355_spmv.h"
    section = hdr[hdr.index("SINGLE-PRECISION KRYLOV BASIS"):]
    for word in ("DEFINITION", "MI_BASIS_F32", "round32", "widen", "refused_last", "COST"):
        assert word in section, word
    assert "enum { MI_BASIS_F64 = 0, MI_BASIS_F32 = 1 };" in section
    from navierstokes_amd import mpk
    assert mpk.GMRES_BASIS == {"f64": MI_BASIS_F64, "f32": MI_BASIS_F32}
    L.mi_version.restype = ctypes.c_int
    assert L.mi_version() == 501  # nothing existing changed


def _ptrs(rows):
    return (ctypes.c_void_p * max(len(rows), 1))(*[r.ctypes.data for r in rows])


def _refused(status, word):
    from navierstokes_amd import mpk
    assert status == MI_ERR_ARG, status
    msg = mpk.lib().mi_last_error().decode()
    assert word in msg, msg


def test_bad_arguments_are_refused_before_the_device_is_touched():
    """Host pointers stand in for device pointers: a refused call never looks behind them."""
    from navierstokes_amd import mpk
    L = mpk.lib()
    n = 8
    whole = np.ones(66 * n + 5, np.float32)
    store = whole[(-whole.ctypes.data % 16) // 4:]  # 16-byte aligned: row j at j n floats is 8-byte aligned for even n
    assert store.ctypes.data % 16 == 0
    rows = [store[j * n:(j + 1) * n] for j in range(65)]
    y, out, nrm = np.ones(n), np.zeros(65), np.zeros(1)
    yp, op, np_ = y.ctypes.data, out.ctypes.data, nrm.ctypes.data
    two = _ptrs(rows[:2])
    with_null = (ctypes.c_void_p * 2)(rows[0].ctypes.data, None)
    with_y = (ctypes.c_void_p * 2)(rows[0].ctypes.data, yp)
    odd = store[1:1 + n]  # offset by one float: 4-byte aligned only
    assert odd.ctypes.data % 8 == 4
    with_odd = (ctypes.c_void_p * 2)(rows[2].ctypes.data, odd.ctypes.data)
    # m outside 0..64, negative n
    for m in (-1, 65):
        _refused(L.mi_mdot_f32_dev(n, m, _ptrs(rows), yp, op, None), "m must be")
        _refused(L.mi_maxpy_f32_dev(n, m, op, 0, _ptrs(rows), yp, None, None), "m must be")
        _refused(L.mi_cgs_f32_dev(n, m, _ptrs(rows), yp, 2, op, np_, None), "m must be")
    _refused(L.mi_mdot_f32_dev(-1, 2, two, yp, op, None), "negative")
    _refused(L.mi_maxpy_f32_dev(-1, 2, op, 0, two, yp, None, None), "negative")
    _refused(L.mi_cgs_f32_dev(-1, 2, two, yp, 2, op, np_, None), "negative")
    # null vectors
    _refused(L.mi_mdot_f32_dev(n, 2, two, None, op, None), "null")
    _refused(L.mi_mdot_f32_dev(n, 2, with_null, yp, op, None), "null")
    _refused(L.mi_mdot_f32_dev(n, 2, None, yp, op, None), "null")
    _refused(L.mi_mdot_f32_dev(n, 2, two, yp, None, None), "null")
    _refused(L.mi_maxpy_f32_dev(n, 2, op, 0, two, None, None, None), "null")
    _refused(L.mi_maxpy_f32_dev(n, 2, op, 0, with_null, yp, None, None), "null")
    _refused(L.mi_maxpy_f32_dev(n, 2, None, 0, two, yp, None, None), "null")
    _refused(L.mi_cgs_f32_dev(n, 2, two, None, 2, op, np_, None), "null")
    _refused(L.mi_cgs_f32_dev(n, 2, with_null, yp, 2, op, np_, None), "null")
    _refused(L.mi_cgs_f32_dev(n, 2, two, yp, 2, None, np_, None), "null")
    _refused(L.mi_cgs_f32_dev(n, 2, two, yp, 2, op, None, None), "null")
    # y is a basis vector
    _refused(L.mi_mdot_f32_dev(n, 2, with_y, yp, op, None), "basis")
    _refused(L.mi_maxpy_f32_dev(n, 2, op, 0, with_y, yp, None, None), "basis")
    _refused(L.mi_cgs_f32_dev(n, 2, with_y, yp, 1, op, np_, None), "basis")
    # a float vector that is not 8-byte aligned
    _refused(L.mi_mdot_f32_dev(n, 2, with_odd, yp, op, None), "8-byte aligned")
    _refused(L.mi_maxpy_f32_dev(n, 2, op, 1, with_odd, yp, np_, None), "8-byte aligned")
    _refused(L.mi_cgs_f32_dev(n, 2, with_odd, yp, 2, op, np_, None), "8-byte aligned")
    # passes outside {1, 2}
    for passes in (0, 3, -1):
        _refused(L.mi_cgs_f32_dev(n, 2, two, yp, passes, op, np_, None), "passes")
    # mi_round_f32_dev
    x64, o32 = np.ones(n + 1), np.zeros(n + 2, np.float32)
    _refused(L.mi_round_f32_dev(-1, yp, None, o32.ctypes.data, None, None), "negative")
    _refused(L.mi_round_f32_dev(n, None, None, o32.ctypes.data, None, None), "null")
    _refused(L.mi_round_f32_dev(n, yp, None, None, x64.ctypes.data, None), "null")
    _refused(L.mi_round_f32_dev(n, yp, None, o32.ctypes.data + 2, None, None), "misaligned")
    _refused(L.mi_round_f32_dev(n, yp + 4, None, o32.ctypes.data, None, None), "misaligned")
    _refused(L.mi_round_f32_dev(n, yp, None, o32.ctypes.data, x64.ctypes.data + 4, None), "misaligned")
    _refused(L.mi_round_f32_dev(n, yp, None, ctypes.c_void_p(yp), None, None), "out32")
    # mi_gmres_create_ex: an unknown basis, and the rules of mi_gmres_create
    h = ctypes.c_void_p()
    for basis in (-1, 2, 32):
        _refused(L.mi_gmres_create_ex(8, 30, basis, ctypes.byref(h)), "basis")
        assert not h.value
    for basis in (MI_BASIS_F64, MI_BASIS_F32):
        for restart in (0, -1, 65):
            _refused(L.mi_gmres_create_ex(8, restart, basis, ctypes.byref(h)), "restart")
        for nn in (0, -4):
            _refused(L.mi_gmres_create_ex(nn, 30, basis, ctypes.byref(h)), "n must be")
        _refused(L.mi_gmres_create_ex(8, 30, basis, None), "null")
        assert not h.value
    _refused(L.mi_gmres_basis_info(None, None, None, None), "null handle")
    assert np.all(y == 1.0) and not out.any() and not nrm.any() and np.all(store == 1.0) and not o32.any() and np.all(x64 == 1.0), \
        "a refused call wrote something"


def test_wrappers_refuse_what_the_library_would():
    from navierstokes_amd import mpk
    A = mpk.csrmatrix(2, [0, 1, 2], [0, 1], [1.0, 2.0])
    with pytest.raises(ValueError):
        mpk.gmres_solver(A, restart=2, basis="f16")
    with pytest.raises(ValueError):
        mpk.GMRES_dev(A, np.ones(2), np.zeros(2), restart=2, basis="single")


def test_no_cpu_fallback_without_gpu():
    """Status 2 (MI_ERR_NODEVICE) from every new entry point that computes, and from the Python solver: nothing runs on the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("this box has a GPU")
    from navierstokes_amd import mpk
    L = mpk.lib()
    n = 8
    store = np.ones(2 * n, np.float32)
    rows = [store[:n], store[n:]]
    y, out, nrm, o32 = np.ones(n), np.zeros(2), np.zeros(1), np.zeros(n, np.float32)
    for status in (L.mi_mdot_f32_dev(n, 2, _ptrs(rows), y.ctypes.data, out.ctypes.data, None),
                   L.mi_maxpy_f32_dev(n, 2, out.ctypes.data, 1, _ptrs(rows), y.ctypes.data, nrm.ctypes.data, None),
                   L.mi_maxpy_f32_dev(n, 0, None, 0, None, y.ctypes.data, nrm.ctypes.data, None),
                   L.mi_cgs_f32_dev(n, 2, _ptrs(rows), y.ctypes.data, 2, out.ctypes.data, nrm.ctypes.data, None),
                   L.mi_round_f32_dev(n, y.ctypes.data, None, o32.ctypes.data, None, None)):
        assert status == MI_ERR_NODEVICE, (status, L.mi_last_error())
    assert np.all(y == 1.0) and not out.any() and not nrm.any() and not o32.any()
    h = ctypes.c_void_p()
    for basis in (MI_BASIS_F64, MI_BASIS_F32):
        assert L.mi_gmres_create_ex(8, 30, basis, ctypes.byref(h)) == MI_ERR_NODEVICE and not h.value
    A = mpk.csrmatrix(2, [0, 1, 2], [0, 1], [1.0, 2.0])
    for call in (lambda: mpk.gmres_solver(A, restart=2, basis="f32").solve(np.ones(2), np.zeros(2)),
                 lambda: mpk.GMRES_dev(A, np.ones(2), np.zeros(2), restart=2, basis="f32")):
        with pytest.raises(mpk.MiError) as e:
            call()
        assert e.value.status == MI_ERR_NODEVICE, e.value
