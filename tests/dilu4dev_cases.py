"""The matrices that tests/test_dilu4dev_abi.py and tests/test_gpu_dilu4dev.py add to those of tests/dilu4_limit_cases.py: patterns on
which an L block (i, j) has NO block (j, i), so that the device refactor of the block DILU (mi_dilu4dev_*, dilu4_factor.hpp) meets
the `mate < 0` path of its row loop.  Every symmetric case has a mate for every L block.

dropped(name), name in NAMES: the matrix of dilu4_limit_cases.matrix(name) and its two value sets with every block (i, j), j > i,
(i + j) % 3 == 0 removed.  Only U blocks go: the L blocks, hence the forward schedule, and the diagonal dominance are untouched.

census(name, order): per block row of B (the handle's numbering) how many L blocks it has and which of them are mated.  This file
asserts at import time that in NATURAL order every case holds
  * rows whose ONLY mated block is the first of at least two, rows whose ONLY mated block is the last of at least two, and rows
    with L blocks and no mate at all (the first stage of the look-ahead, the last, and a row that subtracts nothing);
  * rows with every L count 0..13 (0..3 for `alternating`, whose rows have no more; `wide` has no row with exactly 6 L blocks,
    dropped or not — its generator, tests/bilu4_wide_cases.py, makes none — so it is held to 0..5 and 7..13 and limits:3~
    supplies the 6);
and for `wide` and `limits:3~` the numbers of such rows, so that a changed generator cannot silently stop meeting a limit."""
import functools

import numpy as np

import bilu4_order_cases as OC
import dilu4_limit_cases as LC
import dilu4_model as DM

NAMES = ("wide", "limits:3~", "alternating")
L_COUNTS = {"wide": set(range(14)) - {6}, "limits:3~": set(range(14)), "alternating": set(range(4))}
# natural order: (rows with an unmated block, only the first mated, only the last mated, L blocks but none mated)
CENSUS = {"wide": (876, 21, 41, 21), "limits:3~": (519, 27, 19, 101)}


@functools.lru_cache(maxsize=None)
def _keep(name):
    nb, bp, bc, _ = LC.matrix(name)
    rows = np.repeat(np.arange(nb), np.diff(bp))
    cols = np.asarray(bc)
    return ~((cols > rows) & ((rows + cols) % 3 == 0))


@functools.lru_cache(maxsize=None)
def dropped(name):
    """(nb, ptrow, indcol, coef) of the case, blocks row-major."""
    if name not in NAMES:
        raise KeyError(name)
    nb, bp, bc, _ = LC.matrix(name)
    keep = _keep(name)
    ptr = np.concatenate([[0], np.cumsum(np.add.reduceat(keep, bp[:-1]))]).astype(np.int32)
    return nb, ptr, np.asarray(bc)[keep].astype(np.int32), values(name)


@functools.lru_cache(maxsize=None)
def values(name, variant=0):
    v = np.ascontiguousarray(np.asarray(LC.values(name, variant), np.float64).reshape(-1, 16)[_keep(name)]).reshape(-1)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def model(name, order, variant=0):
    """tests/dilu4_model.py's model of a handle on dropped(name) with values(name, variant): computed once, read-only."""
    nb, bp, bc, _ = dropped(name)
    return DM.Ordered(nb, bp, bc, values(name, variant), order)


def permuted_pattern(nb, ptr, col, order):
    """(bptr, bcol) of B: the pattern in the handle's numbering."""
    if order == "natural":
        return np.asarray(ptr), np.asarray(col)
    perm, _ = OC.colour_model(nb, ptr, col)
    bptr, bcol, _, _ = OC.permute(nb, ptr, col, np.zeros(16 * len(col)), perm)
    return bptr, bcol


def mated(nb, bptr, bcol):
    """Per block row of B: the list, over its L blocks in ascending column, of whether block (j, i) exists."""
    have = {(i, int(bcol[k])) for i in range(nb) for k in range(bptr[i], bptr[i + 1])}
    return [[(int(j), i) in have for j in bcol[bptr[i]:bptr[i + 1]] if j < i] for i in range(nb)]


def pivot_pairs(nb, bptr, bcol):
    return sum(sum(m) for m in mated(nb, bptr, bcol))


@functools.lru_cache(maxsize=None)
def census(name, order="natural"):
    """dict(unmated, only_first, only_last, none, l_counts) of dropped(name) in the handle's numbering."""
    nb, bp, bc, _ = dropped(name)
    rows = mated(nb, *permuted_pattern(nb, bp, bc, order))
    return dict(unmated=sum(1 for m in rows if not all(m)),
                only_first=sum(1 for m in rows if len(m) >= 2 and m[0] and not any(m[1:])),
                only_last=sum(1 for m in rows if len(m) >= 2 and m[-1] and not any(m[:-1])),
                none=sum(1 for m in rows if m and not any(m)),
                l_counts={len(m) for m in rows})


def assert_census(name):
    c = census(name)
    assert c["only_first"] > 0 and c["only_last"] > 0 and c["none"] > 0, (name, c)
    assert set(L_COUNTS[name]) <= c["l_counts"], (name, sorted(c["l_counts"]))
    if name in CENSUS:
        assert (c["unmated"], c["only_first"], c["only_last"], c["none"]) == CENSUS[name], (name, c)


for _name in NAMES:
    assert_census(_name)
