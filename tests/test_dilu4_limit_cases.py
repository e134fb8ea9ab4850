"""The patterns of tests/dilu4_limit_cases.py have the limits they are there for, and a comparison on them can fail — without a GPU
(mi_dilu4_create_host, mi_bilu4_plan_probe and tests/dilu4_model.py).

  counts     in natural order every count of WANTED (0, 1, P-1, P, P+1, 2P-1, 2P, 2P+1, 3P, 3P+1 off-diagonal blocks in a row)
             occurs among the rows of UNFOLDED levels of `wide` in each triangle, among the rows of FOLDED levels of limits:3~
             left of the diagonal and of limits:3 right of it.  The sets, as printed by the test:
               wide, unfolded, left        0, 1, 3, 4, 5, 7..13
               wide, unfolded, right       0..15, 17, 18, 22
               limits:3~, folded, left     0..16, 19, 31, 34, 135
               limits:3, folded, right     0..16, 19, 31, 34, 135
  schedules  the level widths, launches and orderings each case is named for; a host-only handle's launches are the plan probe's
  fetch      mi_dilu4_fetch is BIT-equal to the model on every case in both orders, before and after refactor to the second values
  sensitive  with the pivots kept, zeroing the LAST block of every row with c blocks in a triangle (c in WANTED, c >= 1), or block
             P of every row with more than P, changes the model's sweep on every such row: a test vector could not hide the term
             that a pipeline stage drops, so the bit comparison on the GPU fails if one is dropped"""
import numpy as np
import pytest

import bilu4_wide_cases as W
import dilu4_limit_cases as LC
import dilu4_model as DM
from conftest import assert_bit_equal

ORDERS = ("natural", "colour")
# (case, kernel, triangle): where every count of WANTED must occur, in natural order
PLACES = [("wide", "unfolded", "left"), ("wide", "unfolded", "right"), ("limits:3~", "folded", "left"), ("limits:3", "folded", "right")]


def _probe(name, order):
    from navierstokes_amd import mpk
    B = LC.model(name, order).B
    return mpk.bilu4_plan_probe(B.nb, B.ptr, B.col, 0)


def test_mirror_swaps_the_triangles():
    nb, bp, bc, bv = LC.matrix("limits:3")
    mb, mp, mc, mv = LC.matrix("limits:3~")
    assert mb == nb and len(mc) == len(bc)
    blocks, mblocks = np.asarray(bv).reshape(-1, 16), np.asarray(mv).reshape(-1, 16)
    was = {(i, int(bc[k])): k for i in range(nb) for k in range(bp[i], bp[i + 1])}
    for i in range(nb):
        cols = mc[mp[i]:mp[i + 1]]
        assert (np.diff(cols) > 0).all()
        for k in range(mp[i], mp[i + 1]):
            assert_bit_equal(mblocks[k], blocks[was[(nb - 1 - i, nb - 1 - int(mc[k]))]], f"block ({i}, {mc[k]})")
    back = LC.mirror(mb, mp, mc, mv)
    assert np.array_equal(back[1], bp) and np.array_equal(back[2], bc)
    assert_bit_equal(back[3], bv, "mirrored twice")


@pytest.mark.parametrize("name,kernel,triangle", PLACES, ids=[f"{n}-{k}-{t}" for n, k, t in PLACES])
def test_every_wanted_count_occurs(name, kernel, triangle):
    counts = LC.counts_by_kernel(LC.model(name, "natural"))
    for key, have in sorted(counts.items()):
        print(f"dilu4 limit counts {name} natural {key[1]} {key[0]}: {sorted(have)}")
    assert set(LC.WANTED) <= counts[(triangle, kernel)], sorted(counts[(triangle, kernel)])


def test_the_stated_sets():
    """The sets this file's docstring quotes."""
    wide, lim, mir = (LC.counts_by_kernel(LC.model(n, "natural")) for n in ("wide", "limits:3", "limits:3~"))
    assert wide[("left", "unfolded")] == {0, 1, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13}
    assert wide[("right", "unfolded")] == set(range(16)) | {17, 18, 22}
    assert mir[("left", "folded")] == lim[("right", "folded")] == set(range(17)) | {19, 31, 34, 135}
    assert mir[("right", "folded")] == lim[("left", "folded")] and mir[("left", "unfolded")] == lim[("right", "unfolded")]


def test_schedules_and_orderings():
    nb = LC.matrix("wide")[0]
    assert list(_probe("wide", "natural")["fwd_sizes"]) == list(W.WIDTHS)
    assert np.array_equal(LC.model("wide", "colour").perm, np.arange(nb))
    assert {127, 128, 129} <= set(W.WIDTHS)  # two workgroups less a quad, exactly two, and a third holding one quad
    lim, mir = _probe("limits:3", "natural"), _probe("limits:3~", "natural")
    assert list(mir["fwd_sizes"]) == list(lim["bwd_sizes"]) and list(mir["bwd_sizes"]) == list(lim["fwd_sizes"])
    deep = _probe("fold_deep", "natural")
    assert (deep["fwd_launches"], deep["bwd_launches"], deep["fwd_levels"], deep["bwd_levels"]) == (1, 1, 252, 252), deep
    alt = _probe("alternating", "natural")
    assert alt["fwd_launches"] == alt["fwd_levels"] == 48 and alt["bwd_launches"] == alt["bwd_levels"] == 48, alt
    for n, folded in ((63, True), (64, False), (65, False)):
        one = _probe(f"wide:{n}", "natural")
        assert list(one["fwd_sizes"]) == list(one["bwd_sizes"]) == [n] and (n < LC.FOLD_BELOW) == folded
    for n in (1, 16, 17):
        assert LC.matrix(f"tiny:{n}")[0] == n


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", LC.NAMES)
def test_host_handle_launches_and_fetch(name, order):
    from navierstokes_amd import mpk
    nb, bp, bc, _ = LC.matrix(name)
    E = mpk.dilu4(nb, bp, bc, LC.values(name), host_only=True, order=order)
    info, plan = E.info(), _probe(name, order)
    assert info["order"] == order and np.array_equal(info["perm"], LC.model(name, order).perm)
    assert info["launches"] == plan["fwd_launches"] + plan["bwd_launches"] + (2 if order == "colour" else 0), (info, plan)
    assert (info["fwd_levels"], info["bwd_levels"]) == (plan["fwd_levels"], plan["bwd_levels"])
    for step, variant in enumerate((0, 1, 0)):  # as created, after refactor to the second values, and back
        if step:
            E.refactor(LC.values(name, variant))
        einv, k = E.fetch()
        weinv, wk = LC.model(name, order, variant).fetch()
        assert_bit_equal(einv, weinv, f"{name} {order} variant {variant}: Einv")
        assert_bit_equal(k, wk, f"{name} {order} variant {variant}: K")
    assert not np.array_equal(LC.model(name, order, 0).fetch()[0], LC.model(name, order, 1).fetch()[0])
    E.close()


# ---------------------------------------------------------------- a dropped term shows

class _OtherBlocks:
    """A Dilu with val replaced AFTER construction: the pivots (einv, kmat) stay those of the true values."""

    def __init__(self, D, val):
        self.__dict__.update(D.__dict__)
        self.val = val

    to_hat, from_hat, apply_hat = DM.Dilu.to_hat, DM.Dilu.from_hat, DM.Dilu.apply_hat


def _rows_differ(a, b):
    return (np.asarray(a).reshape(-1, 4).view(np.uint64) != np.asarray(b).reshape(-1, 4).view(np.uint64)).any(axis=1)


@pytest.mark.parametrize("name,kernel,triangle", PLACES, ids=[f"{n}-{k}-{t}" for n, k, t in PLACES])
def test_a_dropped_block_changes_its_row(name, kernel, triangle):
    D = LC.model(name, "natural").B
    u = np.random.default_rng(5).uniform(-1.0, 1.0, 4 * D.nb)
    op = "to_hat" if triangle == "left" else "from_hat"
    first = D.ptr[:-1] if triangle == "left" else D.diag + 1  # the row's first block in the triangle
    count = (D.diag - D.ptr[:-1]) if triangle == "left" else (D.ptr[1:] - D.diag - 1)
    want = getattr(D, op)(u)

    def check(rows, at, what):
        assert rows.size, what
        val = D.val.copy()
        val[at] = 0.0
        got = getattr(_OtherBlocks(D, val), op)(u)
        same = rows[~_rows_differ(got, want)[rows]]
        assert same.size == 0, (what, same[:8])

    for c in LC.WANTED:
        if c >= 1:
            rows = np.nonzero(count == c)[0]
            check(rows, first[rows] + c - 1, f"{name} {triangle}: the last block of the rows with {c}")
    rows = np.nonzero(count >= LC.P + 1)[0]
    check(rows, first[rows] + LC.P, f"{name} {triangle}: block {LC.P} of the rows with more")
