"""The C-ABI of the block ILU preconditioner on a box without a GPU: every mi_bilu4_* export is declared in the header and bound in
mpk.py, the argument rules hold before the device is touched, and the solve refuses instead of falling back."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "navierstokes_amd", "csrc", "libmi355spmv.so")
SYMBOLS = ("mi_bilu4_create", "mi_bilu4_create_host", "mi_bilu4_destroy", "mi_bilu4_refactor", "mi_bilu4_solve_dev", "mi_bilu4_solve",
           "mi_bilu4_info", "mi_bilu4_factor_host", "mi_bilu4_plan_probe")
MI_ERR_ARG, MI_ERR_NODEVICE, MI_ERR_STATE = 1, 2, 6


def test_exports_are_declared_and_bound():
    assert os.path.exists(LIB), "libmi355spmv.so not built (run __graft_entry__.build())"
    raw = ctypes.CDLL(LIB)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355_spmv.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mi_bilu4_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(SYMBOLS), declared ^ set(SYMBOLS)
    from navierstokes_amd import mpk
    L = mpk.lib()
    for s in SYMBOLS:
        assert hasattr(raw, s), f"{s} is not exported"
        assert getattr(L, s).argtypes, f"{s} is not bound in mpk.py"
    for name in ("bilu4", "bilu4_plan_probe", "MatSolve_SeqBAIJ_4", "GMRES"):
        assert hasattr(mpk, name), name
    src = open(os.path.join(ROOT, "include", "mi355_spmv.h")).read()
    for cite in ("baij4_solve.c:4-93", "baij4_factor_avx2.c:114-170", "solve_newton.c:1156-1164"):
        assert cite in src, f"the header does not cite {cite}"


def test_argument_rules_on_a_handle():
    from navierstokes_amd import mpk
    L = mpk.lib()
    F = mpk.bilu4(2, [0, 2, 4], [0, 1, 0, 1], np.concatenate([np.eye(4).reshape(-1) * 2, np.ones(16) * 0.1, np.ones(16) * 0.1, np.eye(4).reshape(-1) * 2]),
                  host_only=True)
    v = np.ones(8)
    vp = v.ctypes.data
    for call, word in ((lambda: L.mi_bilu4_refactor(None, vp, 0), "null handle"), (lambda: L.mi_bilu4_refactor(F.handle, None, 0), "null coef"),
                       (lambda: L.mi_bilu4_refactor(F.handle, vp, 7), "layout"), (lambda: L.mi_bilu4_solve_dev(None, vp, vp, None), "null handle"),
                       (lambda: L.mi_bilu4_solve_dev(F.handle, None, vp, None), "null vector"), (lambda: L.mi_bilu4_solve(F.handle, vp, None), "null vector"),
                       (lambda: L.mi_bilu4_info(None, *([None] * 9)), "null handle"), (lambda: L.mi_bilu4_factor_host(None, None, None, None, None, 0), "null handle"),
                       (lambda: L.mi_bilu4_factor_host(F.handle, None, vp, None, None, 1), "too short")):
        assert call() == MI_ERR_ARG, word
        assert word in L.mi_last_error().decode(), (word, L.mi_last_error())
    # a host-only handle has no device factor: the solve says so, whatever the box
    assert L.mi_bilu4_solve_dev(F.handle, v.ctypes.data, v.ctypes.data, None) == MI_ERR_STATE
    with pytest.raises(mpk.MiError) as e:
        F.solve(np.zeros(8), v)
    assert e.value.status == MI_ERR_STATE
    assert (v == 1.0).all()
    info = F.info()
    assert info["nbrows"] == 2 and info["nblocks"] == 4 and info["form"] == 0 and info["us_one_launch"] == 0.0 and info["factor_bytes"] > 0
    F.close()
    with pytest.raises(ValueError):
        F.solve(np.zeros(8), v)
    with pytest.raises(ValueError):
        mpk.bilu4(2, [0, 2], [0, 1], np.ones(32), host_only=True)


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("this box has a GPU")
    from navierstokes_amd import mpk
    with pytest.raises(mpk.MiError) as e:
        mpk.bilu4(1, [0, 1], [0], np.eye(4).reshape(-1))
    assert e.value.status == MI_ERR_NODEVICE
