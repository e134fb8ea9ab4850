"""The C-ABI of mi_gmres_* on a box without a GPU: the library exports the symbols the header declares, every bad argument that can
be told without a handle is refused with MI_ERR_ARG and a message before the device is touched, and mi_gmres_create fails with
MI_ERR_NODEVICE instead of falling back.  The rules that need a handle (row counts, the kind of preconditioner, the capture rule)
are in tests/test_gpu_gmres_dev.py."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "navierstokes_amd", "csrc", "libmi355spmv.so")
SYMBOLS = ("mi_gmres_create", "mi_gmres_set_operator_csr", "mi_gmres_set_operator_bcsr4", "mi_gmres_set_precond", "mi_gmres_solve_dev",
           "mi_gmres_solve", "mi_gmres_fetch_cycle", "mi_gmres_info", "mi_gmres_destroy")
MI_ERR_ARG, MI_ERR_NODEVICE = 1, 2


def test_library_exports_the_symbols():
    assert os.path.exists(LIB), "libmi355spmv.so not built (run __graft_entry__.build())"
    L = ctypes.CDLL(LIB)
    missing = [s for s in SYMBOLS if not hasattr(L, s)]
    assert not missing, missing
    hdr = open(os.path.join(ROOT, "include", "mi355_spmv.h")).read()
    for s in SYMBOLS:
        assert f"int {s}(" in hdr, f"{s} is not declared in include/mi355_spmv.h"
    for word in ("DEFINITION", "ARITHMETIC", "MI_GMRES_PC_EXACT", "MI_GMRES_PC_SWEEPS_F32"):
        assert word in hdr[hdr.index("mi_gmres_*"):]


def _refused(status, word):
    from navierstokes_amd import mpk
    assert status == MI_ERR_ARG, status
    msg = mpk.lib().mi_last_error().decode()
    assert word in msg, msg


def test_bad_arguments_are_refused_before_the_device_is_touched():
    """Host pointers stand in for device pointers and for handles' vectors: a refused call never looks behind them."""
    from navierstokes_amd import mpk
    L = mpk.lib()
    h = ctypes.c_void_p()
    for restart in (0, -1, 65):
        _refused(L.mi_gmres_create(8, restart, ctypes.byref(h)), "restart")
        assert not h.value
    for n in (0, -4):
        _refused(L.mi_gmres_create(n, 30, ctypes.byref(h)), "n must be")
    _refused(L.mi_gmres_create(8, 30, None), "null")
    b, x, hist = np.ones(8), np.zeros(8), np.zeros(11)
    its, why = ctypes.c_int(-7), ctypes.c_int(-7)
    bp, xp = b.ctypes.data, x.ctypes.data
    args = (ctypes.byref(its), ctypes.byref(why), hist.ctypes.data)
    fake = ctypes.c_void_p(bp)  # never dereferenced: the scalar rules come first
    for ce in (0, -3):
        _refused(L.mi_gmres_solve_dev(fake, bp, xp, 1e-8, 10, ce, *args, None), "check_every")
        _refused(L.mi_gmres_solve(fake, bp, xp, 1e-8, 10, ce, *args), "check_every")
    _refused(L.mi_gmres_solve_dev(fake, bp, xp, 1e-8, -1, 5, *args, None), "maxiter")
    _refused(L.mi_gmres_solve(fake, bp, xp, 1e-8, -1, 5, *args), "maxiter")
    _refused(L.mi_gmres_solve_dev(None, bp, xp, 1e-8, 10, 5, *args, None), "null handle")
    _refused(L.mi_gmres_solve(None, bp, xp, 1e-8, 10, 5, *args), "null handle")
    _refused(L.mi_gmres_set_operator_csr(None, None), "null handle")
    _refused(L.mi_gmres_set_operator_bcsr4(None, None), "null handle")
    _refused(L.mi_gmres_set_precond(None, None, 0, 0, 0), "null handle")
    _refused(L.mi_gmres_fetch_cycle(None, None, None, None, None), "null handle")
    _refused(L.mi_gmres_info(None, None, None, None, None, None), "null handle")
    assert L.mi_gmres_destroy(None) == 0
    assert (its.value, why.value) == (-7, -7) and not x.any() and not hist.any() and np.all(b == 1.0), "a refused call wrote something"


def test_no_cpu_fallback_without_gpu():
    """Status 2 (MI_ERR_NODEVICE) from mi_gmres_create, hence from the Python solver and from GMRES_dev: nothing is solved on the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("this box has a GPU")
    from navierstokes_amd import mpk
    h = ctypes.c_void_p()
    assert mpk.lib().mi_gmres_create(8, 30, ctypes.byref(h)) == MI_ERR_NODEVICE and not h.value
    A = mpk.csrmatrix(2, [0, 1, 2], [0, 1], [1.0, 2.0])
    for call in (lambda: mpk.gmres_solver(A, restart=2).solve(np.ones(2), np.zeros(2)), lambda: mpk.GMRES_dev(A, np.ones(2), np.zeros(2), restart=2)):
        with pytest.raises(mpk.MiError) as e:
            call()
        assert e.value.status == MI_ERR_NODEVICE, e.value
