"""mi_dilu4_* without a GPU (mi_dilu4_create_host): the pivots against the model, and the model's algebra against dense longdouble.

  fetch      mi_dilu4_fetch (Einv and K by the caller's block row) is BIT-equal to tests/dilu4_model.py on fe:3, a scrambled-numbering
             FE matrix (fe_perm:3), the chain and arrow patterns of the bilu4 tests, the unsymmetric seven-row pattern and 50
             random patterns — most of them unsymmetric, where a missing (j, i) block skips the term — in both orderings, both block
             layouts, and after refactor with other values; and with 1 and 4 host threads on patterns with levels of 64 rows and more
  refused    a refused pivot is reported by the caller's block row, at create and at refactor
  algebra    the model's A^ u against (E + L)^-1 B (E + U)^-1 E u, and the model's from_hat(to_hat(r)) against M^-1 r, both formed
             densely in longdouble.  e = max|v - v_ld| / max|v_ld| <= ALGEBRA_TOL.  Where the number comes from:
             tests/test_ref_baij.py allows the bilu4 model, against its longdouble solve, ten times the reference kernels' own error;
             the largest bound that gave on its recorded cases is 10 x 1.067e-15 (profiles/NOTES.md, "Solve: measured errors",
             fe:3-fill4 random, e_avx2), and that is the tolerance here.  Each comparison also rejects a wrong input on the model's
             side: Einv transposed (both), K replaced by E (A^, the only one that reads K).
  interface  the entry points are declared, exported and bound; argument rules; an empty matrix; a host-only handle refuses the
             three operations with MI_ERR_STATE"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import bilu4_cases as C
import bilu4_model as M
import bilu4_order_cases as OC
import dilu4_model as DM
from conftest import ROOT, assert_bit_equal

MI_ERR_ARG, MI_ERR_STATE = 1, 6
ALGEBRA_TOL = 10 * 1.067e-15
ORDERS = ("natural", "colour")
SYMBOLS = ("mi_dilu4_create", "mi_dilu4_create_host", "mi_dilu4_destroy", "mi_dilu4_refactor", "mi_dilu4_fetch", "mi_dilu4_info",
           "mi_dilu4_to_hat_dev", "mi_dilu4_from_hat_dev", "mi_dilu4_apply_hat_dev")
FETCH_PATTERNS = ["fe:3", "fe_perm:3", "chain", "arrow", "unsym"] + [f"random:{s}" for s in range(50)]


def _as_layout(blocks, layout):
    """(nblocks, 4, 4) row-major blocks as the flat array a handle of that layout is given."""
    blocks = np.asarray(blocks, np.float64).reshape(-1, 4, 4)
    return (blocks.transpose(0, 2, 1) if layout == "col" else blocks).reshape(-1).copy()


@functools.lru_cache(maxsize=None)
def model(name, order, variant=0):
    """The model of a handle on OC.matrix(name) (computed once per process, read-only)."""
    nb, bp, bc, _ = OC.matrix(name)
    return DM.Ordered(nb, bp, bc, OC.values(name, variant), order)


def _assert_fetch(E, want, what):
    einv, k = E.fetch()
    weinv, wk = want.fetch()
    assert_bit_equal(einv, weinv, f"{what}: Einv")
    assert_bit_equal(k, wk, f"{what}: K")


# ---------------------------------------------------------------- fetch

@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", FETCH_PATTERNS)
def test_fetch_is_the_models_pivots(name, order):
    from navierstokes_amd import mpk
    nb, bp, bc, _ = OC.matrix(name)
    for layout in ("row", "col"):
        E = mpk.dilu4(nb, bp, bc, _as_layout(OC.values(name), layout), layout=layout, host_only=True, order=order)
        info = E.info()
        assert info["order"] == order and np.array_equal(info["perm"], model(name, order).perm), name
        assert info["nbrows"] == nb and info["nblocks"] == len(bc) and info["device_bytes"] == 0
        for variant in (0, 1):
            if variant:
                E.refactor(_as_layout(OC.values(name, variant), layout))
            _assert_fetch(E, model(name, order, variant), f"{name} {order} layout {layout} variant {variant}")
        E.close()


def test_some_random_patterns_are_unsymmetric_and_skip_terms():
    """What the random cases are for: block (i, j), j < i, without its mirror (j, i)."""
    skipping = 0
    for name in FETCH_PATTERNS:
        nb, bp, bc, _ = OC.matrix(name)
        have = {(i, int(j)) for i in range(nb) for j in bc[bp[i]:bp[i + 1]]}
        skipping += any((j, i) not in have for (i, j) in have if j < i)
    assert skipping >= 25, skipping


@pytest.mark.parametrize("name,order", [("limits:0", "natural"), ("fe:6", "colour"), ("fe:6", "natural")])
def test_the_bits_do_not_depend_on_the_thread_count(name, order, monkeypatch):
    from navierstokes_amd import mpk
    nb, bp, bc, bv = C.matrix(name)
    want = DM.Ordered(nb, bp, bc, bv, order)
    if name == "limits:0":
        assert max(C.LIMITS_WIDTHS) >= 64  # levels wide enough to be dealt to threads
    for threads in ("1", "4"):
        monkeypatch.setenv("MI355_BILU_THREADS", threads)
        E = mpk.dilu4(nb, bp, bc, bv, host_only=True, order=order)
        _assert_fetch(E, want, f"{name} {order} {threads} threads")
        E.close()


# ---------------------------------------------------------------- a refused pivot

@pytest.mark.parametrize("order", ORDERS)
def test_a_refused_pivot_names_the_callers_block_row(order):
    from navierstokes_amd import mpk
    nb, bp, bc, bv = OC.matrix("chain")
    # a row from whose diagonal block nothing is subtracted, so that zeroing the block zeroes the pivot: colour 0 of the chain (an
    # even row, not its own number under the ordering); in natural order only row 0 has no L block
    bad = 44 if order == "colour" else 0
    assert order == "natural" or OC.ordered("chain")[1][bad] != bad
    v = np.array(bv, np.float64).reshape(-1, 4, 4)
    v[bp[bad] + list(bc[bp[bad]:bp[bad + 1]]).index(bad)] = 0.0
    if order == "colour":
        with pytest.raises(M.ZeroPivot) as z:
            DM.Ordered(nb, bp, bc, v, order)
        assert z.value.row == bad
    with pytest.raises(mpk.MiError) as e:
        mpk.dilu4(nb, bp, bc, v.reshape(-1), host_only=True, order=order)
    assert e.value.status == MI_ERR_ARG and f"block row {bad}" in str(e.value), str(e.value)
    E = mpk.dilu4(nb, bp, bc, bv, host_only=True, order=order)
    with pytest.raises(mpk.MiError) as e:
        E.refactor(v.reshape(-1))
    assert e.value.status == MI_ERR_ARG and f"block row {bad}" in str(e.value), str(e.value)
    E.refactor(bv)  # ... and is usable again after a refactor that succeeds
    _assert_fetch(E, model("chain", order), f"chain {order} after a refused refactor")
    E.close()


# ---------------------------------------------------------------- the algebra

# (each has a block (i, j) with its mirror (j, i), so that E is not D and "K replaced by E" is a wrong input)
ALGEBRA_CASES = [("fe:3", "colour"), ("fe:3", "natural"), ("chain", "natural"), ("random:7", "natural"), ("arrow", "colour")]


def _err(v, v_ld):
    return float(np.max(np.abs(np.asarray(v, np.longdouble) - v_ld)) / np.max(np.abs(v_ld)))


def _vector(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)


class _Wrong:
    """A Dilu with einv / kmat replaced: the model's operations over a deliberately wrong input."""

    def __init__(self, D, einv=None, kmat=None):
        self.__dict__.update(D.__dict__)
        if einv is not None:
            self.einv = einv
        if kmat is not None:
            self.kmat = kmat

    to_hat, from_hat, apply_hat = DM.Dilu.to_hat, DM.Dilu.from_hat, DM.Dilu.apply_hat


@pytest.mark.parametrize("name,order", ALGEBRA_CASES)
def test_apply_hat_is_the_split_preconditioned_operator(name, order):
    D = model(name, order).B
    u = _vector(4 * D.nb, 3)
    assert (D.E != D.val[D.diag]).any()
    want = DM.dense_apply_hat(D, u)
    e = _err(D.apply_hat(u), want)
    transposed = _err(_Wrong(D, einv=D.einv.transpose(0, 2, 1).copy()).apply_hat(u), want)
    k_is_e = _err(_Wrong(D, kmat=D.E.copy()).apply_hat(u), want)
    print(f"dilu4 algebra {name} {order}: A^ u e={e:.3e}; Einv transposed {transposed:.3e}; K = E {k_is_e:.3e}; bound {ALGEBRA_TOL:.3e}")
    assert np.isfinite(e) and e <= ALGEBRA_TOL, e
    assert transposed > ALGEBRA_TOL and k_is_e > ALGEBRA_TOL, (transposed, k_is_e)


@pytest.mark.parametrize("name,order", ALGEBRA_CASES)
def test_from_hat_of_to_hat_is_the_preconditioner(name, order):
    D = model(name, order).B
    r = _vector(4 * D.nb, 4)
    want = DM.dense_minv(D, r)
    e = _err(D.from_hat(D.to_hat(r)), want)
    W = _Wrong(D, einv=D.einv.transpose(0, 2, 1).copy())
    transposed = _err(W.from_hat(W.to_hat(r)), want)
    print(f"dilu4 algebra {name} {order}: M^-1 r e={e:.3e}; Einv transposed {transposed:.3e}; bound {ALGEBRA_TOL:.3e}")
    assert np.isfinite(e) and e <= ALGEBRA_TOL, e
    assert transposed > ALGEBRA_TOL, transposed


def test_the_identity_behind_the_trick():
    """B = (E + L) + (E + U) - (2E - D) with the model's K: exactly, entry by entry, wherever 2E - D was exact."""
    D = model("fe:3", "colour").B
    B, E, L, U = DM.dense_parts(D)
    K = np.zeros_like(B)
    for i in range(D.nb):
        K[4 * i:4 * i + 4, 4 * i:4 * i + 4] = D.kmat[i]
    resid = np.max(np.abs((E + L) + (E + U) - K - B)) / np.max(np.abs(B))
    assert resid <= 2.0 ** -52, resid  # K is one rounding away from 2E - D


# ---------------------------------------------------------------- the interface

def test_the_entry_points_are_declared_exported_and_bound():
    from navierstokes_amd import mpk
    hdr = open(os.path.join(ROOT, "include", "mi355_spmv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(mi_dilu4_[a-z0-9_]+)\s*\(", code)) == set(SYMBOLS)
    assert "int mi_gmres_set_operator_dilu4(" in code and "typedef struct mi_dilu4_s* mi_dilu4_t;" in code
    L = mpk.lib()
    for s in SYMBOLS + ("mi_gmres_set_operator_dilu4",):
        assert getattr(L, s).argtypes is not None, s
    for word in ("HAT NORM", "EISENSTAT", "K_i = (2 E_i) - D_i", "NOT built"):
        assert word in hdr[hdr.index("EISENSTAT"):], word
    L.mi_version.restype = ctypes.c_int
    assert L.mi_version() == 501  # nothing existing changed
    for name in ("to_hat", "from_hat", "apply_hat", "refactor", "fetch", "info", "gmres"):
        assert hasattr(mpk.dilu4, name), name


def test_argument_rules_and_the_host_only_handle():
    from navierstokes_amd import mpk
    L = mpk.lib()
    nb, bp, bc, bv = OC.matrix("chain")
    bp, bc, bv = np.ascontiguousarray(bp, np.int32), np.ascontiguousarray(bc, np.int32), np.ascontiguousarray(bv, np.float64)
    h = ctypes.c_void_p()

    def refused(status, word):
        assert status == MI_ERR_ARG and word in L.mi_last_error().decode(), (status, L.mi_last_error())

    for make in (L.mi_dilu4_create, L.mi_dilu4_create_host):
        refused(make(nb, bp.ctypes.data, bc.ctypes.data, bv.ctypes.data, 0, 0, None), "null output")
        refused(make(nb, bp.ctypes.data, bc.ctypes.data, bv.ctypes.data, 2, 0, ctypes.byref(h)), "layout")
        refused(make(nb, bp.ctypes.data, bc.ctypes.data, bv.ctypes.data, 0, 2, ctypes.byref(h)), "ordering")
        refused(make(-1, bp.ctypes.data, bc.ctypes.data, bv.ctypes.data, 0, 0, ctypes.byref(h)), "negative")
        refused(make(nb, None, bc.ctypes.data, bv.ctypes.data, 0, 0, ctypes.byref(h)), "ptrow")
        refused(make(nb, bp.ctypes.data, bc.ctypes.data, None, 0, 0, ctypes.byref(h)), "coef")
        rev = bc.copy()
        rev[0], rev[1] = bc[1], bc[0]
        refused(make(nb, bp.ctypes.data, rev.ctypes.data, bv.ctypes.data, 0, 1, ctypes.byref(h)), "unsorted")
        assert not h.value
    nodiag = np.array([1, 0], np.int32)
    refused(L.mi_dilu4_create_host(2, np.array([0, 1, 2], np.int32).ctypes.data, nodiag.ctypes.data, bv.ctypes.data, 0, 0, ctypes.byref(h)), "diagonal")
    for call in (lambda: L.mi_dilu4_refactor(None, bv.ctypes.data, 0), lambda: L.mi_dilu4_fetch(None, None, None),
                 lambda: L.mi_dilu4_info(None, *[None] * 10), lambda: L.mi_dilu4_apply_hat_dev(None, None, None, None),
                 lambda: L.mi_dilu4_to_hat_dev(None, None, None, None), lambda: L.mi_dilu4_from_hat_dev(None, None, None, None),
                 lambda: L.mi_gmres_set_operator_dilu4(None, None)):
        refused(call(), "null handle")
    assert L.mi_dilu4_destroy(None) == 0
    E = mpk.dilu4(nb, bp, bc, bv, host_only=True)
    refused(L.mi_dilu4_refactor(E.handle, bv.ctypes.data, 7), "layout")
    refused(L.mi_dilu4_refactor(E.handle, None, 0), "coef")
    fake = ctypes.c_void_p(64)
    for fn in (L.mi_dilu4_to_hat_dev, L.mi_dilu4_from_hat_dev, L.mi_dilu4_apply_hat_dev):
        refused(fn(E.handle, None, fake, None), "null vector")
        assert fn(E.handle, fake, fake, None) == MI_ERR_STATE and "host-only" in L.mi_last_error().decode()
    info = E.info()
    plan = mpk.bilu4_plan_probe(nb, *OC.ordered("chain")[3:5], 0)
    assert (info["fwd_levels"], info["bwd_levels"]) == (plan["fwd_levels"], plan["bwd_levels"]) and info["ncolours"] == 2
    assert info["launches"] == plan["fwd_launches"] + plan["bwd_launches"] + 2  # the schedule of bilu4 at fill 0 on B, and the two boundary launches
    E.close()


def test_an_empty_matrix_is_a_no_op():
    from navierstokes_amd import mpk
    L = mpk.lib()
    E = mpk.dilu4(0, [0], [], [], host_only=True, order="colour")
    info = E.info()
    assert info["nbrows"] == 0 and info["nblocks"] == 0 and info["order"] == "colour" and info["launches"] == 2
    assert L.mi_dilu4_apply_hat_dev(E.handle, None, None, None) == 0 and L.mi_dilu4_refactor(E.handle, None, 0) == 0
    einv, k = E.fetch()
    assert einv.shape == (0, 4, 4) and k.shape == (0, 4, 4)
    E.close()
