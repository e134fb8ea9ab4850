"""Matrices at the limits of the row-block kernels — spmv_csr_stream<1024> (spmv_kernels.hpp; the fallback of every CSR handle) and
spmv_csr_tile<2048> (spmv_tile.hpp, tile_plan.hpp) — TEST INFRASTRUCTURE, not a conftest.  Deterministic numpy, no GPU; shared by
tests/test_rowblock_limits.py (census of every case) and tests/test_gpu_rowblock_limits.py (bits).

case(name, nnzb) -> Case(n, ncols, ptrow, indcol, coef, want, want_tile): a case is built for ONE kernel's block size (1024: stream,
2048: tile; both run T = 256 threads and cap a block at 4 T rows) and named after the limits it sits on.  `want` maps a counter of
mi_rowblock_census (navierstokes_amd.mpk.ROWBLOCK_CENSUS) to the smallest value the case must reach, or to ("==", v) for an exact
one; `want_tile` holds the counters only the tile kernel's census fills.

How block contents are known by construction.  The planner (partition.hpp: build_row_blocks) fills a block greedily up to NNZB
nonzeros or 4 T rows, then pulls its end back to a multiple of 64 rows where the shortened block keeps 7/8 of its nonzeros.  So:
  - a SEPARATOR row of exactly NNZB nonzeros ends the block in front of it and is a block of its own (nothing fits beside it,
    and a one-row block is never pulled back);
  - a designed block keeps its rows when it ends on a multiple of 64 rows, or when it starts on one and holds fewer than 64;
    blocks of fewer than 64 rows between separators move the next designed block to the start it needs.
Values are seeded uniform(-1, 1); rows of more than one nonzero name their columns in an order that is not ascending."""
import collections
import functools

import numpy as np

T, ROW_CAP, ROW_ALIGN, KEEP_EIGHTHS = 256, 1024, 64, 7   # kWG / kTileThreads, 4 T, row_block_align, kRowBlockKeepEighths
NNZBS = {"stream": 1024, "tile": 2048}
LIST_LENGTHS = (1, 255, 256, 257, 512, 513, 768, 769, 1024, 1025, 1280, 1281, 1536, 1537, 1792, 1793, 2047, 2048)

Case = collections.namedtuple("Case", "n ncols ptrow indcol coef want want_tile")


def scramble(cols, r):
    """the columns of row r in an order that is not ascending (rotated by a third, every other row reversed as well)"""
    cols = np.asarray(cols, np.int64)
    if len(cols) < 2:
        return cols
    cols = np.roll(cols, len(cols) // 3 + 1)
    return cols[::-1] if r & 1 else cols


def spread(r, k, ncols, step=3):
    """k columns from r on, `step` apart, wrapped into [0, ncols), scrambled"""
    return scramble((r + step * np.arange(k, dtype=np.int64)) % ncols, r)


def assemble(rows, ncols, seed, want, want_tile=None):
    """rows: one array of columns per row"""
    n = len(rows)
    lens = np.array([len(c) for c in rows], np.int64)
    ptrow = np.concatenate([[0], np.cumsum(lens)])
    indcol = np.concatenate([np.asarray(c, np.int64) for c in rows] + [np.zeros(0, np.int64)])
    assert ptrow[-1] < 100_000, "every case stays below 100 000 nonzeros"
    assert len(indcol) == 0 or (indcol.min() >= 0 and indcol.max() < ncols), (indcol.min(), indcol.max(), ncols)
    coef = np.random.default_rng(seed).uniform(-1.0, 1.0, len(indcol))
    out = ptrow.astype(np.int32), indcol.astype(np.int32), coef
    for a in out:
        a.setflags(write=False)
    return Case(n, ncols, *out, want, want_tile or {})


def from_lengths(lens, ncols, seed, want, want_tile=None, special=None):
    """row r holds lens[r] columns spread from r on, unless special[r] names them"""
    special = special or {}
    return assemble([special[r] if r in special else spread(r, int(k), ncols) for r, k in enumerate(lens)], ncols, seed, want, want_tile)


# ---- full blocks, and the launch grid ---------------------------------------------------------------------------------------------
def _full(nnzb, nblk, seed):
    """nblk blocks: 64 equal rows each, one of them 1, 7 or 9 nonzeros short in turn (blocks of NNZB - 1, NNZB - 7, NNZB - 9
    nonzeros: a last 16-byte slot group of the tile kernel with 1 and 7 places of filler; the clamped / unclamped value loads one
    short of the block), then one block of exactly NNZB, then one row of one nonzero as the last block."""
    L = nnzb // 64
    lens, kinds = [], collections.Counter()
    for b in range(nblk - 2):
        short = (1, 7, 9)[b % 3]
        kinds[short] += 1
        blk = [L] * 64
        blk[31] = L - short
        lens += blk
    if nblk >= 2:
        lens += [L] * 64
    lens += [1]
    n = len(lens)
    want = dict(blocks=("==", nblk), idle_wgs=("==", -nblk % 8), pulled_back=("==", 0), full=("==", int(nblk >= 2)), full_less1=("==", kinds[1]),
                nn_mod8_1=("==", kinds[7] + 1), nn_mod8_7=("==", kinds[1] + kinds[9]), nn_1=("==", 1), rows_1=("==", 1), rowlen_1=("==", 1),
                empty=("==", 0), long=("==", 0))
    return from_lengths(lens, max(n, 2 * L), seed, want)


def full_blocks(nnzb):
    return _full(nnzb, 17, 11)                                             # 17 = 1 (mod 8): seven idle workgroups behind the grid


def grid_edges(nnzb, nblk):
    """the same cut to 1 (a matrix of one row and one nonzero), 7, 8 and 9 blocks: xcd_remap over a grid of 8 * ceil(blocks / 8)"""
    return _full(nnzb, nblk, 20 + nblk)


# ---- blocks of more than T rows -----------------------------------------------------------------------------------------------------
def short_rows(nnzb):
    """Rows of 1 and 2 nonzeros between separators, so that blocks hold exactly T, T + 1 and the capped 4 T rows (the second row loop
    of both kernels: no turn, one row, three full turns); 2048 rows of one nonzero with every 16th row empty, so that the row cap and
    not NNZB ends a block (the second such block ends at the cap AND in front of a separator); 280 rows of two nonzeros from a
    multiple of 64 on, which the alignment rule cuts back to 256."""
    sep = [nnzb]
    lens = [1] * T + sep                                                   # [0, 256): T rows; the separator is row 256
    lens += [2] * 61 + sep                                                 # [257, 318) stays: it crosses no multiple of 64; separator 318
    lens += [1] * (T + 1) + sep                                            # [319, 576): T + 1 rows ending on 9 * 64; separator 576
    lens += [2, 1] * 31 + sep                                              # [577, 639); separator 639
    stretch = [0 if i % 16 == 7 else 1 for i in range(2 * ROW_CAP)]        # [640, 1664), [1664, 2688): ended by the row cap
    lens += stretch + sep                                                  # separator 2688
    lens += [1] * 62 + sep                                                 # [2689, 2751); separator 2751
    lens += [2] * 280 + sep                                                # [2752, 3032) is pulled back to [2752, 3008); [3008, 3032); separator 3032
    lens += [1] * 5                                                        # the last block
    n = len(lens)
    want = dict(rows_t=("==", 2), rows_t1=("==", 1), rows_cap=("==", 2), ended_by_cap=("==", 1), pulled_back=("==", 1), rows_max=("==", ROW_CAP),
                full=("==", 7), rows_1=("==", 7), rowlen_1=1000, empty=("==", 0), long=("==", 0))
    special = {r: np.array([(r + 1) % n, r]) for r, k in enumerate(lens) if k == 2}       # descending
    return from_lengths(lens, n, 31, want, special=special)


# ---- blocks and rows without nonzeros -----------------------------------------------------------------------------------------------
def empty(nnzb):
    """1024 empty rows and more at the start, in the middle and at the end: blocks without nonzeros as the first block, an inner one
    and the last (a whole turn of the zero-fill loop and three more); listed blocks whose first rows are empty, and separators that
    take 1023 empty rows with them (a listed block of 4 T rows whose last 1023 are empty)."""
    sep = [nnzb]
    lens = [0] * (ROW_CAP + 10) + [8] * 54 + sep                            # [0, 1024) empty; [1024, 1088): ten empty rows first; separator 1088
    lens += [0] * (ROW_CAP - 1)                                             # ... which takes 1023 empty rows along: [1088, 2112)
    lens += [0] * (ROW_CAP + 5) + [8] * 59 + sep                            # [2112, 3136) empty; [3136, 3200): five empty rows first; separator 3200
    lens += [0] * (ROW_CAP - 1) + [0] * ROW_CAP                             # [3200, 4224); [4224, 5248) empty, the last block
    n = len(lens)
    want = dict(empty=("==", 3), empty_first=("==", 1), empty_last=("==", 1), empty_middle=("==", 1), first_row_empty=("==", 2),
                last_row_empty=("==", 2), rows_cap=("==", 2), rowlen_8=54 + 59, blocks=("==", 7), pulled_back=("==", 0))
    return from_lengths(lens, n, 41, want)


# ---- rows longer than a block -------------------------------------------------------------------------------------------------------
def long_rows(nnzb):
    """Rows of NNZB + 1, 2 NNZB (the chunk loop's last chunk full), 2 NNZB + 1 and 3 NNZB + 5 nonzeros: one as row 0, 2 NNZB + 1 and
    3 NNZB + 5 side by side, one with every column named twice and empty rows behind it, 2 NNZB as the last row of the matrix (its
    last chunk ends where the arrays end).  ncols lets every other long row name distinct columns."""
    ncols = 3 * (3 * nnzb + 5) + 64
    few = [5]
    lens = [nnzb + 1] + few * 40 + [2 * nnzb + 1, 3 * nnzb + 5] + few * 30 + [nnzb + 1] + [0] * 20 + few * 30 + [2 * nnzb]
    n = len(lens)
    special = {}
    for r, k in enumerate(lens):
        if k > nnzb:
            start = (97 * r) % (ncols - 3 * k)
            special[r] = scramble(start + 3 * np.arange(k, dtype=np.int64), r)
            assert len(np.unique(special[r])) == k
    twice = 1 + 40 + 2 + 30
    special[twice] = scramble(7 + 3 * np.repeat(np.arange((nnzb + 2) // 2, dtype=np.int64), 2)[:nnzb + 1], twice)
    want = dict(long=("==", 5), long_plus1=("==", 2), long_2x=("==", 1), long_2x1=("==", 1), long_first_row=("==", 1), long_last_row=("==", 1),
                long_after_long=("==", 1), first_row_empty=("==", 1), empty=("==", 0))
    return from_lengths(lens, ncols, 51, want, special=special)


# ---- row lengths around the batched chain's eight -----------------------------------------------------------------------------------
def row_lengths(nnzb):
    """Rows of 1, 7, 8, 9, 15, 16, 17 nonzeros in turn (row_chain<8> / tile_row_chain<8>: one batch short of, exactly and one past
    full; a cycle holds 73 = 1 (mod 8) nonzeros, so rows start at every offset mod 8 inside their blocks); columns descending,
    every third row names its first column twice; column 0 and column ncols - 1 in one row."""
    n = 7 * 60
    ncols = n
    lens = [(1, 7, 8, 9, 15, 16, 17)[r % 7] for r in range(n)]
    special = {}
    for r, k in enumerate(lens):
        c = (5 * r) % (ncols - k) + np.arange(k, dtype=np.int64)[::-1]
        if r % 3 == 0 and k >= 2:
            c[k // 2] = c[0]
        special[r] = c
    special[8] = np.array([ncols - 1, 0, 3, ncols - 1, 0, 1, 2], np.int64)                # a row of seven
    assert lens[8] == 7
    want = dict(rowlen_1=60, rowlen_8=60, rowlen_9=60, empty=("==", 0), long=("==", 0))
    return from_lengths(lens, ncols, 61, want, special=special)


# ---- rectangular matrices -------------------------------------------------------------------------------------------------------------
def rect_one_column(nnzb):
    """ncols = 1: every nonzero in column 0 — a list of one column per block (U = 1, R = 1, every lane of the list load clamped)"""
    lens = [(3, 8, 5, 0, 12, 1, 9)[r % 7] for r in range(700)]
    return assemble([np.zeros(k, np.int64) for k in lens], 1, 71, dict(rowlen_1=100, rowlen_8=100, rowlen_9=100),
                    dict(u_1=1, r1=1, u_max=("==", 1)))


def rect_wide(nnzb):
    """ncols = 8 n: columns spread over the whole width, the last column named"""
    n = 300
    ncols = 8 * n
    rows = [scramble((8 * r + 267 * np.arange(9, dtype=np.int64)) % ncols, r) for r in range(n)]
    rows[n - 1][4] = ncols - 1
    rows[0][0] = 0
    return assemble(rows, ncols, 72, dict(rowlen_9=("==", n)), dict(u_max=1000))


# ---- the tile kernel's list lengths ---------------------------------------------------------------------------------------------------
def lists(nnzb, skew):
    """Tile only: eighteen consecutive blocks of exactly 2048 nonzeros whose distinct-column counts are LIST_LENGTHS — every
    instantiation tile_block<R>, R = 1..8, with both sides of every boundary U = 256 k | 256 k + 1, U = 1 and U = nn = 2048.  Block b
    names the columns of a range of its own, U_b long, one after the other (descending, wrapping), so it names all of them.
    skew: 128 rows of 16 (every row a multiple of 8 long: the SKEW instantiation), else 64 x (15, 17) (none is: the plain one);
    either way a block is 128 rows and ends on a multiple of 64."""
    assert nnzb == 2048
    per = [16] * 128 if skew else [15, 17] * 64
    rows, off = [], 0
    for U in LIST_LENGTHS:
        k = np.arange(nnzb, dtype=np.int64)
        cols = off + (U - 1 - k % U)
        p = 0
        for ln in per:
            rows.append(cols[p:p + ln])
            p += ln
        assert p == nnzb and len(np.unique(cols)) == U
        off += U
    nb = len(LIST_LENGTHS)
    want = dict(blocks=("==", nb), full=("==", nb), pulled_back=("==", 0), idle_wgs=("==", -nb % 8))
    want_tile = dict(r1=("==", 3), r2=("==", 2), r3=("==", 2), r4=("==", 2), r5=("==", 2), r6=("==", 2), r7=("==", 2), r8=("==", 3), u_1=("==", 1),
                     u_mult=("==", 8), u_mult1=("==", 7), u_eq_nn=("==", 1), u_max=("==", 2048), skew=("==", int(skew)))
    return assemble(rows, off, 80 + int(skew), want, want_tile)


BUILDERS = dict(full_blocks=full_blocks, short_rows=short_rows, empty=empty, long_rows=long_rows, row_lengths=row_lengths,
                rect_one_column=rect_one_column, rect_wide=rect_wide,
                **{f"grid_edges_{k}": functools.partial(grid_edges, nblk=k) for k in (1, 7, 8, 9)},
                lists_skew=functools.partial(lists, skew=True), lists_plain=functools.partial(lists, skew=False))
TILE_ONLY = ("lists_skew", "lists_plain")
ALL = [(name, kern) for name in BUILDERS for kern in ("stream", "tile") if kern == "tile" or name not in TILE_ONLY]


@functools.lru_cache(maxsize=None)
def case(name, kern):
    return BUILDERS[name](NNZBS[kern])


def reversed_row_map(n):
    """(rowmap, length of y): the rows reversed into a longer y, 37 entries in (an odd offset; not a plain offset map, so the kernels
    store through the map)"""
    return (37 + np.arange(n - 1, -1, -1, dtype=np.int64)).astype(np.int32), n + 37 + 11
