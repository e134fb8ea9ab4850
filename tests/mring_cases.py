"""Matrices at the limits of the multi-window ring kernel's plan (spmv_mring.hpp, mring_plan.hpp) — TEST INFRASTRUCTURE, not a
conftest.  Deterministic numpy, no GPU; shared by tests/test_mring_limits.py (census) and tests/test_gpu_mring_limits.py (bits).

case(name) -> Case(n, ncols, ptrow, indcol, coef, want) as in tests/ring_cases.py, `want` over navierstokes_amd.mpk.MRING_CENSUS.

The planner gives a block at most T = 256 rows, so with few nonzeros per row block b is rows [256 b, 256 b + 256): the cases are
written block by block.  The base is the diagonal (one cluster that slides by four groups of 64 columns a block, the window a
further four groups ahead); special blocks name up to eight columns a row."""
import functools

import numpy as np

from ring_cases import Case, K_RING_MAX_PLAIN, assemble, diagonal, scramble

# ---- constants of mring_plan.hpp -------------------------------------------------------------------------------------------------
K, W, GAP, LEAD, GROUPS = 5, 960, 256, 4, 8            # kMringK, kMringW, kMringGap, kMringLead, kMringGroups
NNZB, T, WG_UNIT, XCDS, MAX_B = 2048, 256, 512, 8, 96  # kMringNnzb, kMringThreads, kMringWgUnit, kMringXcds, kMringMaxB
ROWS = T                                               # rows of a block
NB0 = 2 * WG_UNIT + 80                                 # blocks of the small cases: runs of three blocks (fewer than 513 blocks: one block a run)


def block_rows(special, b, offsets, ncols):
    """block b: row 256 b + i names the columns offsets[j] + i (scrambled), clamped to the matrix"""
    for i in range(ROWS):
        r = b * ROWS + i
        special[r] = scramble(np.minimum(np.asarray(offsets, np.int64) + i, ncols - 1), r)


def wide_row(special, r, ncols):
    """row r with K columns GAP + 40 apart behind its block's diagonal cluster: one cluster too many, the block is PLAIN"""
    c0 = (r // ROWS + 1) * ROWS + GAP + 40
    assert c0 + K * (GAP + 40) < ncols
    special[r] = scramble(c0 + (GAP + 40) * np.arange(K), r)


# ---- M1: clusters -----------------------------------------------------------------------------------------------------------------
def m1():
    n = ROWS * NB0
    sp = {}
    far = 2 * W                                                                        # clusters this far apart are never joined
    block_rows(sp, 10, [10 * ROWS + far * j for j in range(K)], n)                    # K clusters: served
    block_rows(sp, 20, [20 * ROWS - far * 2 + far * j for j in range(K + 1)], n)      # K + 1: PLAIN
    step = (W - 64 - ROWS) // 3
    block_rows(sp, 30, [30 * ROWS + q for q in (0, step, 2 * step, W - 64 - ROWS)], n)          # one cluster W - 64 wide: served
    block_rows(sp, 40, [40 * ROWS + q for q in (0, step, 2 * step, W - 64 - ROWS + 1)], n)      # one column wider: PLAIN
    block_rows(sp, 50, [50 * ROWS, 50 * ROWS + ROWS - 1 + GAP - 1], n)                # neighbours GAP - 1 apart: one cluster
    block_rows(sp, 60, [60 * ROWS, 60 * ROWS + ROWS - 1 + GAP], n)                    # GAP apart: two
    p, c, v = assemble(n, n, diagonal(n), sp, 1001)
    want = dict(served_clusters_k=("==", 1), clusters_max=("==", K), wide_clusters_k1=("==", 1), plain_clusters=("==", 1),
                served_width_limit=("==", 1), width_max=("==", W - 64), wide_width_limit1=("==", 1), plain_width=("==", 1),
                gap_max_joined=("==", GAP - 1), gap_min_split=("==", GAP), plain=("==", 2))
    return Case(n, n, p, c, v, want)


# ---- M2: groups -------------------------------------------------------------------------------------------------------------------
M2_BLOCK = 31      # the middle block of a run of three


def m2(extra=0):
    """On the diagonal the window ends LEAD groups beyond a block's last column.  Block M2_BLOCK reaches GROUPS groups beyond that (+ extra
    columns): with extra = 0 it needs exactly GROUPS groups and stays in its run, with extra = 1 it needs one more and starts a run."""
    n = ROWS * NB0
    sp = {}
    top = M2_BLOCK * ROWS + 64 * (LEAD + GROUPS) - ROWS + extra      # + i, i < ROWS: the block's last column is M2_BLOCK ROWS + 64 (LEAD + GROUPS) - 1 + extra
    block_rows(sp, M2_BLOCK, [M2_BLOCK * ROWS, M2_BLOCK * ROWS + (top - M2_BLOCK * ROWS) // 2, top], n)
    p, c, v = assemble(n, n, diagonal(n), sp, 1002)
    want = dict(groups_max=("==", GROUPS), groups_full=1) if extra == 0 else dict(forced_cuts=1)
    return Case(n, n, p, c, v, want)


# ---- M3: window wrap ----------------------------------------------------------------------------------------------------------------
def m3():
    """the diagonal slides its window across the wrap-around every W columns; two clusters two planes apart do so in two windows"""
    n = ROWS * NB0
    plane = 3 * W + 128
    r = np.arange(n, dtype=np.int64)
    base = np.stack([np.minimum(r + plane, n - 1), r], axis=1)
    p, c, v = assemble(n, n, base, {}, 1003)
    return Case(n, n, p, c, v, dict(group_ends_at_wrap=10, group_starts_at_wrap=10, block_across_wrap=10, groups_full=10, served=100))


# ---- M4: run kinds ------------------------------------------------------------------------------------------------------------------
M4_PERIOD = 100                      # blocks: 3 PLAIN, 20 served, 4 PLAIN, 20 served, 40 PLAIN, 13 served
N_M4 = 2800 * ROWS                   # the smallest size (in steps of 200 blocks) with runs of all three kinds, found with the census


def m4_matrix(nblk, seed=1004):
    n = nblk * ROWS
    sp = {}
    for b0 in range(0, nblk - M4_PERIOD - 10, M4_PERIOD):
        b = b0 + 5
        for m in (K_RING_MAX_PLAIN, K_RING_MAX_PLAIN + 1, 40):
            for q in range(m):
                wide_row(sp, (b + q) * ROWS + 7 + q % 3, n)
            b += m + 20
    return assemble(n, n, diagonal(n), sp, seed)


def m4():
    n = N_M4
    p, c, v = m4_matrix(n // ROWS)
    return Case(n, n, p, c, v, dict(runs_kind0=1, runs_kind1=1, runs_kind3=1, runs_wide3=1, runs_wide4=1, plain_first=1, plain_last=1, plain_middle=1))


def m4_small():
    n = 800 * ROWS
    p, c, v = m4_matrix(n // ROWS)
    return Case(n, n, p, c, v, dict(runs_kind0=("==", 0), runs_kind3=1))


# ---- M5: second round -----------------------------------------------------------------------------------------------------------------
def m5():
    """More than 8 * 512 blocks, so that a run of a block or two counts as SHORT; every 30 blocks two blocks in a row name three fresh
    clusters, more groups than the loop refills: each starts a run, and the first of the two is a run of one block.  The short runs come
    on top of the long ones: more runs than the 512 resident workgroups, dealt out over 8 XCD shares of unequal length."""
    nblk = 9 * WG_UNIT
    n = nblk * ROWS
    sp = {}
    far = 3 * W
    for b in range(45, nblk - 40, 30):
        for q in (0, 1):
            lo = (b + q) * ROWS - far - 300 * q
            block_rows(sp, b + q, [lo, lo + far, lo + 2 * far, lo + 3 * far], n)
    p, c, v = assemble(n, n, diagonal(n), sp, 1005)
    return Case(n, n, p, c, v, dict(runs=WG_UNIT + 1, table_len=WG_UNIT + 8, table_padded=1, forced_cuts=100, run_min=("==", 1), run_max=9))


# ---- M6: matrix end -------------------------------------------------------------------------------------------------------------------
def m6(n=ROWS * NB0 + 37, ncols=None):
    """n not a multiple of 64: the window of the last blocks runs ahead to the last column and its groups reach past it"""
    ncols = n if ncols is None else ncols
    r = np.arange(n, dtype=np.int64)
    base = np.stack([np.minimum(r + 2 * W, ncols - 1), np.minimum(r, ncols - 1)], axis=1)
    p, c, v = assemble(n, ncols, base, {}, 1006)
    want = dict(group_past_end=1) if ncols == n and n > 4 * ROWS else {}
    return Case(n, ncols, p, c, v, want)


BUILDERS = dict(m1=m1, m2=m2, m2_cut=functools.partial(m2, extra=1), m3=m3, m4=m4, m4_small=m4_small, m5=m5, m6=m6,
                m6_tiny=functools.partial(m6, n=40), m6_rect=functools.partial(m6, n=ROWS * NB0 + 37, ncols=ROWS * NB0 - 500),
                m6_wide=functools.partial(m6, n=ROWS * NB0 + 5, ncols=ROWS * NB0 + 4 * W + 3))
NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=4)
def case(name):
    return BUILDERS[name]()
