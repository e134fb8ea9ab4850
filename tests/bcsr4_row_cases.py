"""Block patterns at the limits of the row-per-quad BCSR 4x4 kernels — spmv_bcsr4<2> and spmv_bcsr4_tile<2> (spmv_kernels.hpp, the x-tile
lists of bcsr4_tile_plan.hpp) — TEST INFRASTRUCTURE, not a conftest.  Deterministic numpy, no GPU; shared by
tests/test_bcsr4_row_limits.py (the probe's answer for every case) and tests/test_gpu_bcsr4_row_limits.py (bits).

case(name) -> Case(nbrows, nbcols, ptrow, indcol, coef, probe): block pattern, 16 seeded values from (-1, 1) per block (row-major),
and what mi_bcsr4_tile_probe must answer.  Block columns inside a block row are not ascending and may repeat."""
import collections
import functools

import numpy as np

TILE_ROWS, TILE_NODES, TILE_MIN_BLOCKS = 64, 1024, 4096                  # kWG / 4, kBtileNodes, kBtileMinBlocks
PIPE_LENGTHS = (0, 1, 2, 3, 4, 5, 9)   # spmv_bcsr4<2>: nothing, half a round, a round, 1.5, two rounds (the last prefetch clamps), 2.5, 4.5
PIPE_ROWS = (1, 63, 64, 65, 129)

Case = collections.namedtuple("Case", "nbrows nbcols ptrow indcol coef probe")


def assemble(rows, nbcols, seed, probe):
    lens = np.array([len(c) for c in rows], np.int64)
    ptrow = np.concatenate([[0], np.cumsum(lens)])
    indcol = np.concatenate([np.asarray(c, np.int64) for c in rows] + [np.zeros(0, np.int64)])
    assert 16 * ptrow[-1] < 100_000, "every case stays below 100 000 nonzeros"
    assert len(indcol) == 0 or (indcol.min() >= 0 and indcol.max() < nbcols)
    coef = np.random.default_rng(seed).uniform(-1.0, 1.0, 16 * len(indcol))
    out = ptrow.astype(np.int32), indcol.astype(np.int32), coef
    for a in out:
        a.setflags(write=False)
    return Case(len(rows), nbcols, *out, probe)


def every_pair(symbols):
    """a sequence in which every ordered pair of symbols (equal ones included) stands side by side: an Euler circuit of the complete
    directed graph with loops (Hierholzer), len(symbols) ** 2 + 1 long"""
    k = len(symbols)
    nxt = [0] * k
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < k:
            stack.append(nxt[v])
            nxt[v] += 1
        else:
            out.append(stack.pop())
    return [symbols[i] for i in out[::-1]]


def block_cols(i, k, nbcols):
    """k block columns for block row i: 5 apart from 3 i on, wrapped, rotated so that they are not ascending; every fourth row
    names its first column twice"""
    c = (3 * i + 5 * np.arange(k, dtype=np.int64)) % nbcols
    c = np.roll(c, k // 3 + 1) if k > 1 else c
    if i % 4 == 1 and k >= 2:
        c[k - 1] = c[0]
    return c


def pipe(nbrows):
    """Block rows of 0, 1, 2, 3, 4, 5 and 9 blocks, every length beside every other (and itself) in both orders — each takes its own
    path through the two-round pipeline of spmv_bcsr4<2>, and four lanes per block row put neighbours into one wave; the first and the
    last block row empty (from two block rows on; one block row alone holds five blocks).  nbrows 63, 64, 65 and 129: one workgroup
    short of full, full, one block row into the second, one into the third.  More block columns than block rows, the last one named."""
    seq = every_pair(PIPE_LENGTHS)
    lens = [seq[i % len(seq)] for i in range(nbrows)]
    if nbrows >= 2:
        lens[0] = lens[-1] = 0
    else:
        lens = [5]
    nbcols = nbrows + 7
    rows = [block_cols(i, k, nbcols) for i, k in enumerate(lens)]
    for i, k in enumerate(lens):
        if k == 9:
            rows[i][4] = nbcols - 1
            break
    return assemble(rows, nbcols, 100 + nbrows, dict(would_build=False, groups=-(-nbrows // TILE_ROWS), max_nodes=0, groups_at_cap=0))


def _xtile(first_group_extra, trim_to=None):
    """Group 0: 64 block rows x 16 blocks, all 1024 block columns distinct (+ first_group_extra further ones in its last row);
    group 1: 1024 blocks that all name block column 7; groups 2 and 3: 17 blocks a row over 600 columns; a last group of ten block
    rows, the last of them empty (its lanes load the padding block behind the arrays).  trim_to: blocks dropped from the ends of
    the rows of group 3 until that many are left."""
    nbcols = 1100
    rows = [16 * i + np.roll(np.arange(16, dtype=np.int64), i % 16) for i in range(64)]
    rows[63] = np.concatenate([rows[63], 1024 + np.arange(first_group_extra, dtype=np.int64)])
    rows += [np.full(16, 7, np.int64) for _ in range(64)]
    rows += [np.roll((5 * i + 3 * np.arange(17, dtype=np.int64)) % 600, i % 17) for i in range(128)]
    rows += [block_cols(i, k, nbcols) for i, k in enumerate((3, 0, 2, 9, 1, 4, 5, 0, 2, 0))]
    total = sum(len(r) for r in rows)
    if trim_to is not None:
        i = 255
        while total > trim_to:
            assert i >= 192
            cut = min(len(rows[i]) - 1, total - trim_to)
            rows[i] = rows[i][:len(rows[i]) - cut]
            total -= cut
            i -= 1
    return rows, nbcols, total


def xtile_cap():
    rows, nbcols, total = _xtile(0)
    assert total >= TILE_MIN_BLOCKS
    return assemble(rows, nbcols, 201, dict(would_build=True, groups=5, max_nodes=TILE_NODES, groups_at_cap=1))


def xtile_over():
    """one block column more in group 0: 1025 — the lists are not built, the plain kernel serves the handle"""
    rows, nbcols, total = _xtile(1)
    return assemble(rows, nbcols, 202, dict(would_build=False, groups=5, max_nodes=TILE_NODES + 1, groups_at_cap=0))


def xtile_small():
    """4095 blocks: one short of the size from which the lists are built"""
    rows, nbcols, total = _xtile(0, trim_to=TILE_MIN_BLOCKS - 1)
    assert total == TILE_MIN_BLOCKS - 1
    return assemble(rows, nbcols, 203, dict(would_build=False, groups=5, max_nodes=0, groups_at_cap=0))


def xtile_exact():
    """4096 blocks: the smallest pattern with lists"""
    rows, nbcols, total = _xtile(0, trim_to=TILE_MIN_BLOCKS)
    assert total == TILE_MIN_BLOCKS
    return assemble(rows, nbcols, 204, dict(would_build=True, groups=5, max_nodes=TILE_NODES, groups_at_cap=1))


BUILDERS = dict(xtile_cap=xtile_cap, xtile_over=xtile_over, xtile_small=xtile_small, xtile_exact=xtile_exact,
                **{f"pipe_{k}": functools.partial(pipe, k) for k in PIPE_ROWS})
ALL = list(BUILDERS)
XTILE = [nm for nm in ALL if nm.startswith("xtile")]


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


def to_csr(K):
    """the block pattern as a CSR matrix (n = 4 nbrows, ncols = 4 nbcols): row 4 i + q holds, block by block, the four entries of row q
    of the block — the order in which csr_to_bcsr4_exact reads them back, so the blocked copy of this matrix is K itself"""
    lens = np.diff(K.ptrow.astype(np.int64))
    ptrow = np.concatenate([[0], np.cumsum(np.repeat(4 * lens, 4))])
    indcol = np.empty(int(ptrow[-1]), np.int64)
    coef = np.empty(int(ptrow[-1]), np.float64)
    v = K.coef.reshape(-1, 4, 4)
    for i in range(K.nbrows):
        b0, b1 = int(K.ptrow[i]), int(K.ptrow[i + 1])
        cols = (4 * K.indcol[b0:b1].astype(np.int64)[:, None] + np.arange(4)[None, :]).ravel()
        for q in range(4):
            a = int(ptrow[4 * i + q])
            indcol[a:a + len(cols)] = cols
            coef[a:a + len(cols)] = v[b0:b1, q, :].ravel()
    return 4 * K.nbrows, 4 * K.nbcols, ptrow.astype(np.int32), indcol.astype(np.int32), coef
