"""The C-ABI of the multi-vector BLAS-1 (mi_mdot*, mi_maxpy*, mi_cgs_dev, mi_krylov_basis_cgs_dev) on a box without a GPU: the
library exports the symbols, every bad argument is refused with MI_ERR_ARG and a message before the device is touched, and the
compute calls fail with MI_ERR_NODEVICE instead of falling back.  No compute here; tests/test_gpu_multi_blas1.py has the bits."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "navierstokes_amd", "csrc", "libmi355spmv.so")
SYMBOLS = ("mi_mdot", "mi_mdot_dev", "mi_maxpy", "mi_maxpy_dev", "mi_cgs_dev", "mi_krylov_basis_cgs_dev")
MI_ERR_ARG, MI_ERR_NODEVICE = 1, 2


def test_library_exports_the_six_symbols():
    assert os.path.exists(LIB), "libmi355spmv.so not built (run __graft_entry__.build())"
    L = ctypes.CDLL(LIB)
    missing = [s for s in SYMBOLS if not hasattr(L, s)]
    assert not missing, missing
    hdr = open(os.path.join(ROOT, "include", "mi355_spmv.h")).read()
    for s in SYMBOLS:
        assert f"int {s}(" in hdr, f"{s} is not declared in include/mi355_spmv.h"


def _ptrs(rows):
    return (ctypes.c_void_p * max(len(rows), 1))(*[r.ctypes.data for r in rows])


def _refused(status, word):
    from navierstokes_amd import mpk
    assert status == MI_ERR_ARG, status
    msg = mpk.lib().mi_last_error().decode()
    assert word in msg, msg


def test_bad_arguments_are_refused_before_the_device_is_touched():
    """Host pointers stand in for device pointers in the *_dev calls: a refused call never looks behind them."""
    from navierstokes_amd import mpk
    L = mpk.lib()
    n = 8
    rows = [np.ones(n) for _ in range(65)]
    y, out, nrm = np.ones(n), np.zeros(65), np.zeros(1)
    yp, op, np_ = y.ctypes.data, out.ctypes.data, nrm.ctypes.data
    two = _ptrs(rows[:2])
    with_null = (ctypes.c_void_p * 2)(rows[0].ctypes.data, None)
    with_y = (ctypes.c_void_p * 2)(rows[0].ctypes.data, yp)
    # m outside 0..64
    for m in (-1, 65):
        _refused(L.mi_mdot_dev(n, m, _ptrs(rows), yp, op, None), "m must be")
        _refused(L.mi_mdot(n, m, _ptrs(rows), yp, op), "m must be")
        _refused(L.mi_maxpy_dev(n, m, op, 0, _ptrs(rows), yp, None, None), "m must be")
        _refused(L.mi_maxpy(n, m, op, 0, _ptrs(rows), yp), "m must be")
        _refused(L.mi_cgs_dev(n, m, _ptrs(rows), yp, 2, op, np_, None), "m must be")
    _refused(L.mi_mdot_dev(-1, 2, two, yp, op, None), "negative")
    # null vectors
    _refused(L.mi_mdot_dev(n, 2, two, None, op, None), "null")
    _refused(L.mi_mdot_dev(n, 2, with_null, yp, op, None), "null")
    _refused(L.mi_mdot_dev(n, 2, None, yp, op, None), "null")
    _refused(L.mi_mdot_dev(n, 2, two, yp, None, None), "null")
    _refused(L.mi_mdot(n, 2, with_null, yp, op), "null")
    _refused(L.mi_mdot(n, 2, two, yp, None), "null")
    _refused(L.mi_maxpy_dev(n, 2, op, 0, two, None, None, None), "null")
    _refused(L.mi_maxpy_dev(n, 2, op, 0, with_null, yp, None, None), "null")
    _refused(L.mi_maxpy_dev(n, 2, None, 0, two, yp, None, None), "null")
    _refused(L.mi_maxpy(n, 2, op, 1, with_null, yp), "null")
    _refused(L.mi_maxpy(n, 2, None, 1, two, yp), "null")
    _refused(L.mi_cgs_dev(n, 2, two, None, 2, op, np_, None), "null")
    _refused(L.mi_cgs_dev(n, 2, with_null, yp, 2, op, np_, None), "null")
    _refused(L.mi_cgs_dev(n, 2, two, yp, 2, None, np_, None), "null")
    _refused(L.mi_cgs_dev(n, 2, two, yp, 2, op, None, None), "null")
    # y is a basis vector
    _refused(L.mi_mdot_dev(n, 2, with_y, yp, op, None), "basis")
    _refused(L.mi_mdot(n, 2, with_y, yp, op), "basis")
    _refused(L.mi_maxpy_dev(n, 2, op, 0, with_y, yp, None, None), "basis")
    _refused(L.mi_maxpy(n, 2, op, 0, with_y, yp), "basis")
    _refused(L.mi_cgs_dev(n, 2, with_y, yp, 1, op, np_, None), "basis")
    # passes outside {1, 2}
    for passes in (0, 3, -1):
        _refused(L.mi_cgs_dev(n, 2, two, yp, passes, op, np_, None), "passes")
    assert np.all(y == 1.0) and not out.any() and not nrm.any(), "a refused call wrote something"


def test_krylov_cgs_refuses_a_null_handle():
    """The other argument rules of mi_krylov_basis_cgs_dev need a handle, hence a device: tests/test_gpu_multi_blas1.py."""
    from navierstokes_amd import mpk
    v0, V, coef = np.ones(2), np.zeros(6), np.zeros(9)
    _refused(mpk.lib().mi_krylov_basis_cgs_dev(None, 2, v0.ctypes.data, V.ctypes.data, 2, 2, coef.ctypes.data, None), "null handle")


def test_wrappers_refuse_what_the_library_would():
    from navierstokes_amd import mpk
    with pytest.raises(ValueError):
        mpk.cgs([np.ones(4)], np.ones(4), passes=3)
    with pytest.raises(ValueError):
        mpk.BuildKrylovBasis(mpk.csrmatrix(2, [0, 1, 2], [0, 1], [1.0, 2.0]), None, 1, orth="mgs")


def test_no_cpu_fallback_without_gpu():
    """Status 2 (MI_ERR_NODEVICE) from the host forms and from the device forms alike."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("this box has a GPU")
    from navierstokes_amd import mpk
    L = mpk.lib()
    n = 8
    rows = [np.ones(n), np.full(n, 2.0)]
    for call in (lambda: mpk.mdot(rows, np.ones(n)),
                 lambda: mpk.maxpy(np.ones(2), rows, np.ones(n)),
                 lambda: mpk.maxpy(np.ones(2), rows, np.ones(n), negate=True, norm=True),
                 lambda: mpk.cgs(rows, np.ones(n)),
                 lambda: mpk.cgs(rows, np.ones(n), passes=1)):
        with pytest.raises(mpk.MiError) as e:
            call()
        assert e.value.status == MI_ERR_NODEVICE, e.value
    y, out, nrm = np.ones(n), np.zeros(2), np.zeros(1)
    for status in (L.mi_mdot_dev(n, 2, _ptrs(rows), y.ctypes.data, out.ctypes.data, None),
                   L.mi_maxpy_dev(n, 2, out.ctypes.data, 1, _ptrs(rows), y.ctypes.data, nrm.ctypes.data, None),
                   L.mi_maxpy_dev(n, 0, None, 0, None, y.ctypes.data, nrm.ctypes.data, None),
                   L.mi_cgs_dev(n, 2, _ptrs(rows), y.ctypes.data, 2, out.ctypes.data, nrm.ctypes.data, None)):
        assert status == MI_ERR_NODEVICE, (status, L.mi_last_error())
    assert np.all(y == 1.0) and not out.any() and not nrm.any()
