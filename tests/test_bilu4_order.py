"""The multicolour ordering behind a block ILU handle (mi_bilu4_create_host_ordered, mi_bilu4_order_probe, mi_bilu4_order_info) on a
box without a GPU: host-only handles and probes.

  rule       the probe's perm and colours are those of the plain-Python model of tests/bilu4_order_cases.py, on fe:3, fe:4, a
             chain, an arrow, 20 seeded random patterns and an unsymmetric pattern that the upper triangle alone would colour
             differently; every colour is independent; ncolours <= 1 + the largest degree
  levels     at fill 0 fwd_levels and bwd_levels of mi_bilu4_info are both <= ncolours
  factor     the host factor of an ordered handle is, bit for bit, tests/bilu4_model.py's factor of the matrix permuted in numpy:
             fill 0, 1 and 2, both layouts; again after mi_bilu4_refactor with new values
  natural    mi_bilu4_create_host_ordered(.., NATURAL) gives the factor and the info of mi_bilu4_create_host
  pivot      a refused pivot names the caller's block row
"""
import ctypes

import numpy as np
import pytest

import bilu4_order_cases as OC
from conftest import assert_bit_equal

MI_ERR_ARG, MI_ERR_STATE = 1, 6


@pytest.mark.parametrize("name", OC.PATTERNS)
def test_the_probe_follows_the_rule(name):
    from navierstokes_amd import mpk
    nb, bp, bc, _ = OC.matrix(name)
    perm, colour = OC.colour_model(nb, bp, bc)
    got = mpk.bilu4_order_probe(nb, bp, bc, "colour")
    assert np.array_equal(got["perm"], perm), name
    ncol = int(colour.max()) + 1
    assert got["ncolours"] == ncol
    assert np.array_equal(got["colour_sizes"], np.bincount(colour, minlength=ncol))
    assert sorted(got["perm"].tolist()) == list(range(nb))
    # every colour is an independent set of the symmetrised graph: the colour of a new number, from the probe's own sizes
    first = np.concatenate([[0], np.cumsum(got["colour_sizes"])])
    col_of = np.searchsorted(first, got["perm"], side="right") - 1
    for i in range(nb):
        for j in bc[bp[i]:bp[i + 1]]:
            assert int(j) == i or col_of[i] != col_of[int(j)], (name, i, int(j))
    assert ncol <= 1 + OC.max_degree(nb, bp, bc)
    nat = mpk.bilu4_order_probe(nb, bp, bc, "natural")
    assert nat["ncolours"] == 0 and np.array_equal(nat["perm"], np.arange(nb)) and len(nat["colour_sizes"]) == 0


def test_the_unsymmetric_pattern_needs_the_symmetrised_graph():
    nb, bp, bc, _ = OC.matrix("unsym")
    full, _ = OC.colour_model(nb, bp, bc)
    upper, _ = OC.colour_model(nb, bp, bc, symmetrise=False)
    assert not np.array_equal(full, upper)


@pytest.mark.parametrize("name", OC.PATTERNS)
def test_fill_zero_has_at_most_ncolours_levels_per_sweep(name):
    from navierstokes_amd import mpk
    nb, bp, bc, bv = OC.matrix(name)
    F = mpk.bilu4(nb, bp, bc, bv, fill=0, host_only=True, order="colour")
    info, oinfo = F.info(), F.order_info()
    F.close()
    # the launches of a solve that take the wide-level kernel: every unfolded level (one level of at least 64 block rows)
    plan = mpk.bilu4_plan_probe(nb, *OC.ordered(name)[3:5], 0)
    assert oinfo["order"] == "colour" and oinfo["wide_launches"] == int((plan["fwd_sizes"] >= 64).sum() + (plan["bwd_sizes"] >= 64).sum())
    assert np.array_equal(oinfo["perm"], OC.ordered(name)[1])
    assert 1 <= info["fwd_levels"] <= oinfo["ncolours"] and 1 <= info["bwd_levels"] <= oinfo["ncolours"], (info, oinfo)


def _as_layout(blocks, layout):
    """(nblocks, 4, 4) row-major blocks as the flat array a handle of that layout is given."""
    return (blocks.transpose(0, 2, 1) if layout == "col" else blocks).reshape(-1).copy()


@pytest.mark.parametrize("fill", [0, 1, 2])
@pytest.mark.parametrize("name", OC.PATTERNS)
def test_the_host_factor_is_the_models_factor_of_the_permuted_matrix(name, fill):
    from navierstokes_amd import mpk
    nb, bp, bc, _ = OC.matrix(name)
    for layout in ("row", "col"):
        F = mpk.bilu4(nb, bp, bc, _as_layout(OC.values(name).reshape(-1, 4, 4), layout), fill=fill, layout=layout, host_only=True, order="colour")
        for variant in (0, 1):
            if variant:
                F.refactor(_as_layout(OC.values(name, variant).reshape(-1, 4, 4), layout))
            ptr, col, diag, val = F.factor_host()
            wptr, wcol, wdiag, wval = OC.model_factor(name, fill, variant)
            what = f"{name} fill {fill} layout {layout} variant {variant}"
            assert np.array_equal(ptr, wptr) and np.array_equal(col, wcol) and np.array_equal(diag, wdiag), what
            assert_bit_equal(val, wval, what)
        F.close()


@pytest.mark.parametrize("name", ["fe:3", "arrow", "unsym", "random:7"])
def test_natural_through_the_ordered_entry_point_is_create_host(name):
    from navierstokes_amd import mpk
    L = mpk.lib()
    nb, bp, bc, bv = OC.matrix(name)
    bp, bc, bv = np.ascontiguousarray(bp, np.int32), np.ascontiguousarray(bc, np.int32), np.ascontiguousarray(bv, np.float64)
    for fill in (0, 1):
        ref = mpk.bilu4(nb, bp, bc, bv, fill=fill, host_only=True)
        F = mpk.bilu4(nb, bp, bc, bv, fill=fill, host_only=True)  # a second handle, whose own handle is swapped for the ordered entry point's
        h = ctypes.c_void_p()
        mpk.check(L.mi_bilu4_create_host_ordered(nb, bp.ctypes.data, bc.ctypes.data, bv.ctypes.data, 0, fill, 0, ctypes.byref(h)))
        L.mi_bilu4_destroy(F._h)
        F._h = h
        for a, b in zip(F.factor_host(), ref.factor_host()):
            assert_bit_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), f"{name} fill {fill}")
        ia, ib = F.info(), ref.info()
        for key in ("nbrows", "nblocks", "fwd_levels", "bwd_levels", "launches", "form", "factor_bytes"):
            assert ia[key] == ib[key], (key, ia, ib)
        assert F.order_info()["order"] == "natural" and F.order_info()["ncolours"] == 0 and F.order_info()["wide_launches"] == 0
        assert np.array_equal(F.order_info()["perm"], np.arange(nb))
        F.close()
        ref.close()


def test_a_refused_pivot_names_the_callers_block_row():
    from navierstokes_amd import mpk
    nb, bp, bc, bv = OC.matrix("chain")
    perm = OC.ordered("chain")[1]
    bad = 44  # an even row of the chain: colour 0, so nothing is subtracted from its diagonal block before it is inverted
    assert perm[bad] != bad and perm[bad] < nb // 2 + 1
    v = np.array(bv, np.float64).reshape(-1, 4, 4)
    v[bp[bad] + list(bc[bp[bad]:bp[bad + 1]]).index(bad)] = 0.0
    with pytest.raises(mpk.MiError) as e:
        mpk.bilu4(nb, bp, bc, v.reshape(-1), host_only=True, order="colour")
    assert e.value.status == MI_ERR_ARG and f"block row {bad}" in str(e.value), str(e.value)
    F = mpk.bilu4(nb, bp, bc, bv, host_only=True, order="colour")
    with pytest.raises(mpk.MiError) as e:
        F.refactor(v.reshape(-1))
    assert f"block row {bad}" in str(e.value), str(e.value)
    F.close()


def test_argument_rules():
    from navierstokes_amd import mpk
    L = mpk.lib()
    nb, bp, bc, bv = OC.matrix("unsym")
    bp, bc, bv = np.ascontiguousarray(bp, np.int32), np.ascontiguousarray(bc, np.int32), np.ascontiguousarray(bv, np.float64)
    h = ctypes.c_void_p()
    assert L.mi_bilu4_create_host_ordered(nb, bp.ctypes.data, bc.ctypes.data, bv.ctypes.data, 0, 0, 7, ctypes.byref(h)) == MI_ERR_ARG
    assert "ordering" in L.mi_last_error().decode()
    assert L.mi_bilu4_order_probe(nb, bp.ctypes.data, bc.ctypes.data, 7, None, None, None, 0) == MI_ERR_ARG
    sizes, nc = np.zeros(1, np.int32), ctypes.c_int()
    assert L.mi_bilu4_order_probe(nb, bp.ctypes.data, bc.ctypes.data, 1, None, ctypes.byref(nc), sizes.ctypes.data, 1) == MI_ERR_ARG
    assert "too short" in L.mi_last_error().decode() and nc.value == 3
    assert L.mi_bilu4_order_info(None, None, None, None, None) == MI_ERR_ARG
    with pytest.raises(ValueError):
        mpk.bilu4(nb, bp, bc, bv, host_only=True, order="rcm")
    # an ordered host-only handle refuses the solve like any host-only handle
    F = mpk.bilu4(nb, bp, bc, bv, host_only=True, order="colour")
    with pytest.raises(mpk.MiError) as e:
        F.solve(np.zeros(4 * nb), np.ones(4 * nb))
    assert e.value.status == MI_ERR_STATE
    F.close()


ORDER_SYMBOLS = ("mi_bilu4_create_ordered", "mi_bilu4_create_host_ordered", "mi_bilu4_order_info", "mi_bilu4_order_probe")


def test_the_order_entry_points_are_a_closed_list_declared_and_bound():
    """The ordering's exports are exactly ORDER_SYMBOLS: each declared in the header (with a parenthesised declarator, beside the
    closed list of tests/test_bilu4_abi.py), exported, and bound in mpk.py; the library exports no other symbol that names an ordering."""
    import os
    import re
    import subprocess
    from conftest import ROOT
    from navierstokes_amd import mpk
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355_spmv.h")).read(), flags=re.S)
    declared = set(re.findall(r"\bint\s+\((mi_bilu4_[a-z0-9_]*order[a-z0-9_]*)\)\s*\(", hdr))
    assert declared == set(ORDER_SYMBOLS), declared ^ set(ORDER_SYMBOLS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", mpk.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert {s for s in exported if s.startswith("mi_bilu4") and "order" in s} == set(ORDER_SYMBOLS)
    for s in ORDER_SYMBOLS:
        assert getattr(mpk.lib(), s).argtypes, f"{s} is not bound in mpk.py"
    assert "MI_BILU_ORDER_NATURAL = 0" in hdr and "MI_BILU_ORDER_COLOUR = 1" in hdr
    for name in ("bilu4_order_probe", "BILU_ORDERS"):
        assert hasattr(mpk, name), name


def test_an_empty_matrix_keeps_the_ordering_it_was_asked_for():
    from navierstokes_amd import mpk
    L = mpk.lib()
    p0 = np.zeros(1, np.int32)
    for ordering in (0, 1):
        h = ctypes.c_void_p()
        mpk.check(L.mi_bilu4_create_host_ordered(0, p0.ctypes.data, None, None, 0, 0, ordering, ctypes.byref(h)))
        o, nc, wl = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
        mpk.check(L.mi_bilu4_order_info(h, ctypes.byref(o), ctypes.byref(nc), ctypes.byref(wl), None))
        assert (o.value, nc.value, wl.value) == (ordering, 0, 0)
        L.mi_bilu4_destroy(h)
    got = mpk.bilu4_order_probe(0, p0, np.zeros(0, np.int32), "colour")
    assert got["ncolours"] == 0 and len(got["perm"]) == 0 and len(got["colour_sizes"]) == 0
