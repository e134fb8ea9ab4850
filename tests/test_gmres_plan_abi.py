"""The C-ABI of the capturable GMRES (mi_maxpy_upto_dev, mi_maxpy_upto_f32_dev, mi_gmres_prepare_stream, mi_gmres_cycle_dev,
mi_gmres_state, mi_gmres_plan_*) on a box without a GPU: the library exports the symbols the header declares, the header section
keeps its words, every argument rule is refused with MI_ERR_ARG and a message before the device is touched and with nothing
written, and the compute calls fail with MI_ERR_NODEVICE instead of falling back.  The bits are in tests/test_gpu_maxpy_upto.py
and tests/test_gpu_gmres_plan.py."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "navierstokes_amd", "csrc", "libmi355spmv.so")
SYMBOLS = ("mi_maxpy_upto_dev", "mi_maxpy_upto_f32_dev", "mi_gmres_prepare_stream", "mi_gmres_cycle_dev", "mi_gmres_state",
           "mi_gmres_plan_create", "mi_gmres_plan_solve", "mi_gmres_plan_info", "mi_gmres_plan_destroy")
MI_ERR_ARG, MI_ERR_NODEVICE = 1, 2


def test_library_exports_the_symbols_and_the_header_keeps_its_words():
    assert os.path.exists(LIB), "libmi355spmv.so not built (run __graft_entry__.build())"
    L = ctypes.CDLL(LIB)
    missing = [s for s in SYMBOLS if not hasattr(L, s)]
    assert not missing, missing
    hdr = open(os.path.join(ROOT, "include", "mi355_spmv.h")).read()
    for s in SYMBOLS:
        assert f"int {s}(" in hdr, f"{s} is not declared in include/mi355_spmv.h"
    section = hdr[hdr.index("capturable GMRES"):]
    for word in ("DEFINITION", "CAPTURE", "WASTE", "2 segment - 1", "not prepared", "CLAIM", "thread-local"):
        assert word in section, word
    assert "typedef struct mi_gmres_plan_s* mi_gmres_plan_t;" in section
    L.mi_version.restype = ctypes.c_int
    assert L.mi_version() == 501  # nothing existing changed
    from navierstokes_amd import mpk
    for name in ("maxpy_upto", "gmres_plan"):
        assert hasattr(mpk, name), name
    for name in ("prepare_stream", "cycle", "state", "plan"):
        assert hasattr(mpk.gmres_solver, name), name


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
    rows32 = [store[j * n:(j + 1) * n] for j in range(65)]
    rows64 = [np.ones(n) for _ in range(65)]
    y, coef = np.ones(n), np.full(65, 2.0)
    count = np.array([2], np.int32)
    yp, cp, kp = y.ctypes.data, coef.ctypes.data, count.ctypes.data
    odd = store[1:1 + n]  # offset by one float: 4-byte aligned only
    assert odd.ctypes.data % 8 == 4
    for call, rows in ((L.mi_maxpy_upto_dev, rows64), (L.mi_maxpy_upto_f32_dev, rows32)):
        two = _ptrs(rows[:2])
        for m in (-1, 65):
            _refused(call(n, m, kp, cp, 0, _ptrs(rows), yp, None), "m must be")
        _refused(call(-1, 2, kp, cp, 0, two, yp, None), "negative")
        _refused(call(n, 2, kp, cp, 0, two, None, None), "null")
        _refused(call(n, 2, kp, cp, 0, None, yp, None), "null")
        _refused(call(n, 2, kp, cp, 0, (ctypes.c_void_p * 2)(rows[0].ctypes.data, None), yp, None), "null basis vector")
        _refused(call(n, 2, kp, None, 0, two, yp, None), "null coefficients")
        _refused(call(n, 2, None, cp, 1, two, yp, None), "null count")
        _refused(call(n, 0, None, None, 0, None, yp, None), "null count")  # (even with nothing to add)
        _refused(call(n, 2, kp, cp, 0, (ctypes.c_void_p * 2)(rows[0].ctypes.data, yp), yp, None), "basis")
    _refused(L.mi_maxpy_upto_f32_dev(n, 2, kp, cp, 0, (ctypes.c_void_p * 2)(rows32[2].ctypes.data, odd.ctypes.data), yp, None), "8-byte aligned")
    # the solver's new entry points: a null handle (no handle can exist without a GPU), and the plan's own rules before it
    b, x = np.ones(n), np.zeros(n)
    bp, xp = b.ctypes.data, x.ctypes.data
    _refused(L.mi_gmres_prepare_stream(None, None), "null handle")
    _refused(L.mi_gmres_cycle_dev(None, bp, xp, 1, 1e-8, 10, None), "null handle")
    _refused(L.mi_gmres_cycle_dev(None, bp, xp, 1, 1e-8, -1, None), "negative maxiter")
    _refused(L.mi_gmres_state(None, None, None, None, None, None, None, None, None), "null handle")
    h = ctypes.c_void_p(1234)
    for segment in (0, -3):
        _refused(L.mi_gmres_plan_create(None, bp, xp, 1e-8, 10, segment, ctypes.byref(h)), "segment")
        assert not h.value  # (the output is cleared first)
    _refused(L.mi_gmres_plan_create(None, bp, xp, 1e-8, -1, 5, ctypes.byref(h)), "negative maxiter")
    _refused(L.mi_gmres_plan_create(None, bp, xp, 1e-8, 10, 5, ctypes.byref(h)), "null handle")
    _refused(L.mi_gmres_plan_create(None, bp, xp, 1e-8, 10, 5, None), "null output")
    _refused(L.mi_gmres_plan_solve(None, None, None, None, None), "null handle")
    _refused(L.mi_gmres_plan_info(None, None, None, None, None, None), "null handle")
    assert L.mi_gmres_plan_destroy(None) == 0
    assert np.all(y == 1.0) and np.all(store == 1.0) and all(np.all(r == 1.0) for r in rows64) and not x.any() and count[0] == 2, \
        "a refused call wrote something"


def test_wrappers_raise_what_the_library_would():
    """The Python forms hand the library's refusal on as MiError with its status; what they refuse themselves is a type."""
    from navierstokes_amd import mpk
    with pytest.raises(TypeError):
        mpk.maxpy_upto(np.array([1], np.int32), np.ones(2), [np.ones(4), np.ones(4)], np.ones(4))  # no host form
    L = mpk.lib()
    with pytest.raises(mpk.MiError) as e:
        mpk.check(L.mi_gmres_plan_create(None, None, None, 1e-8, 10, 0, ctypes.byref(ctypes.c_void_p())))
    assert e.value.status == MI_ERR_ARG and "segment" in str(e.value)
    with pytest.raises(mpk.MiError) as e:
        mpk.check(L.mi_maxpy_upto_dev(4, 65, None, None, 0, None, None, None))
    assert e.value.status == MI_ERR_ARG and "m must be" in str(e.value)


def test_no_cpu_fallback_without_gpu():
    """Status 2 (MI_ERR_NODEVICE) from every new entry point that computes and can be reached without a handle, and from the
    Python solver on the way to a plan: nothing runs on the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("this box has a GPU")
    from navierstokes_amd import mpk
    L = mpk.lib()
    n = 8
    rows64 = [np.ones(n), np.ones(n)]
    rows32 = [np.ones(n, np.float32), np.ones(n, np.float32)]
    y, coef, count = np.ones(n), np.full(2, 2.0), np.array([2], np.int32)
    for call, rows in ((L.mi_maxpy_upto_dev, rows64), (L.mi_maxpy_upto_f32_dev, rows32)):
        status = call(n, 2, count.ctypes.data, coef.ctypes.data, 0, _ptrs(rows), y.ctypes.data, None)
        assert status == MI_ERR_NODEVICE, (status, L.mi_last_error())
    assert np.all(y == 1.0)
    A = mpk.csrmatrix(2, [0, 1, 2], [0, 1], [1.0, 2.0])
    with pytest.raises(mpk.MiError) as e:  # (a plan, a cycle and a state need a solver, and a solver needs a GPU)
        mpk.gmres_solver(A, restart=2).plan(np.ones(2), np.zeros(2), segment=1)
    assert e.value.status == MI_ERR_NODEVICE, e.value
