"""The wide-level kernel of the ordered block ILU solve (bilu4_level_wide) at the limits of its launch rule and of its pipeline, on
the hand-built pattern of tests/bilu4_wide_cases.py, bit for bit (uint64 views) against tests/bilu4_model.py.

  pattern    already in colour order (the library's perm is the identity, one colour per layer); level widths 63, 64, 65, 127, 128,
             129 in both sweeps: both sides of the folded / wide switch at MI355_BILU_WIDE_MIN=64 and of a threshold of 128, and last
             workgroups with one quad
  rows       rows of wide levels with 0, 1, P - 1, P, P + 1 and 2 P + 1 off-diagonal blocks in each triangle (P = 4): the
             pipeline's prologue, its clamp and the round boundary; the rows with ONE block — every stage of the pipeline clamps to it
             and names the same neighbour; block row 64, whose only (hence last) block left of the diagonal names block row 0
  switch     kBiluWideMin was MEASURED to be 64, the narrowest unfolded level (profiles/NOTES.md R15.1), so the handle on which the
             wide kernel does not run is the one created with MI355_BILU_WIDE_MIN above every width (mi_bilu4_order_info's
             wide_launches == 0); with MI355_BILU_WIDE_MIN=64, and by default, every level of at least 64 rows takes it, with 128 the
             levels of at least 128; mi_bilu4_info's launches are the same throughout: the rule only picks a kernel
  bits       all handles give each other's bits and the model's (x = U^-1 L^-1 b pins the forward sweep and the backward one:
             t is what the backward sweep starts from), with b and x 16-byte aligned and offset by 8 bytes, and x == b.  The
             caller's alignment reaches the two boundary kernels only (their 16-byte and scalar forms): the level kernels of an
             ordered handle always run on the handle's own aligned vectors
"""
import functools
import os

import numpy as np
import pytest

import bilu4_model as M
import bilu4_order_cases as OC
import bilu4_wide_cases as W
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


@functools.lru_cache(maxsize=None)
def _model():
    """(b, the model's x): factored and solved once for the file."""
    nb, bp, bc, bv = W.matrix()
    ptr, col, diag, val = M.factor(nb, bp, bc, bv, 0)
    b = np.random.default_rng(61).standard_normal(4 * nb)
    sched = (M.schedule(nb, ptr, col, diag, False), M.schedule(nb, ptr, col, diag, True))
    return b, M.solve(nb, ptr, col, diag, val, b, sched)


def _handle(wide_min):
    from navierstokes_amd import mpk
    old = os.environ.pop("MI355_BILU_WIDE_MIN", None)
    if wide_min is not None:
        os.environ["MI355_BILU_WIDE_MIN"] = str(wide_min)
    try:
        return mpk.bilu4(*W.matrix(), fill=0, order="colour")
    finally:
        os.environ.pop("MI355_BILU_WIDE_MIN", None)
        if old is not None:
            os.environ["MI355_BILU_WIDE_MIN"] = old


def test_the_pattern_has_the_limits_it_was_built_for():
    from navierstokes_amd import mpk
    nb, bp, bc, _ = W.matrix()
    perm, colour = OC.colour_model(nb, bp, bc)
    assert np.array_equal(perm, np.arange(nb)) and np.array_equal(colour, W.layer_of())
    plan = mpk.bilu4_plan_probe(nb, bp, bc, 0)
    assert list(plan["fwd_sizes"]) == list(W.WIDTHS)
    assert sorted(plan["bwd_sizes"]) == sorted(W.WIDTHS) and set(W.WIDTHS) == {63, 64, 65, 127, 128, 129}
    wide = np.asarray(W.WIDTHS)[W.layer_of()] >= W.WIDE_MIN
    lower, upper = W.offdiag_counts()
    for counts in (lower, upper):
        assert set(W.WANTED_COUNTS) <= set(counts[wide].tolist()), sorted(set(counts[wide].tolist()))
    assert lower[64] == 1 and bc[bp[64]] == 0  # the first row of layer 1: its one block left of the diagonal is block row 0


NEVER = 2 ** 31 - 1  # a threshold above every width: bilu4_level computes every unfolded level


def test_the_switch_picks_the_kernel_and_nothing_else():
    b, want = _model()
    got = {}
    for wide_min in (NEVER, W.WIDE_MIN, 128, None):
        F = _handle(wide_min)
        oinfo, info = F.order_info(), F.info()
        assert oinfo["order"] == "colour" and oinfo["ncolours"] == len(W.WIDTHS) and np.array_equal(oinfo["perm"], np.arange(len(b) // 4))
        assert oinfo["wide_launches"] == 2 * sum(w >= (W.WIDE_MIN if wide_min is None else wide_min) for w in W.WIDTHS), (wide_min, oinfo)
        assert info["fwd_levels"] == info["bwd_levels"] == len(W.WIDTHS)
        x = _dev(np.full(len(b), np.nan))
        F.solve(x, _dev(b))
        got[wide_min] = (x.cpu().numpy(), info["launches"])
        F.close()
    assert len({launches for _, launches in got.values()}) == 1
    assert_bit_equal(got[NEVER][0], want, "no wide launch (bilu4_level) against the model")
    assert_bit_equal(got[W.WIDE_MIN][0], want, "MI355_BILU_WIDE_MIN=64 (bilu4_level_wide) against the model")
    for wide_min in (W.WIDE_MIN, 128, None):
        assert_bit_equal(got[wide_min][0], got[NEVER][0], f"the two kernels, MI355_BILU_WIDE_MIN={wide_min}")


@pytest.mark.parametrize("offset", [0, 1], ids=["16-byte aligned", "offset by 8 bytes"])
def test_wide_levels_with_either_alignment_and_in_place(offset):
    import torch
    b, want = _model()
    n = len(b)
    F = _handle(W.WIDE_MIN)
    assert F.order_info()["wide_launches"] > 0
    buf_b = torch.zeros(n + 2, dtype=torch.float64, device="cuda")
    buf_x = torch.full((n + 2,), float("nan"), dtype=torch.float64, device="cuda")
    db, dx = buf_b[offset:offset + n], buf_x[offset:offset + n]
    assert db.data_ptr() % 16 == 8 * offset and dx.data_ptr() % 16 == 8 * offset
    db.copy_(_dev(b))
    F.solve(dx, db)
    assert_bit_equal(dx.cpu().numpy(), want, "x")
    assert_bit_equal(db.cpu().numpy(), b, "b was written")
    F.solve(db, db)
    assert_bit_equal(db.cpu().numpy(), want, "x == b")
    F.close()
