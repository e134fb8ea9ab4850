"""Extra patterns for the one-launch form of the block ILU solve (mi_bilu4one_*): levels wide enough to be cut into chunks.  Every
pattern of tests/bilu4_cases.py that is small enough for the Python factorisation folds into ONE chunk per sweep or has prescribed
layers; these add chunk boundaries inside a level, far dependencies across chunks, and a pattern that is not structurally symmetric.
All diagonally dominant — diagonal blocks 4 I plus small noise, off-diagonal blocks small — so that no pivot is refused.
A case is (nb, ptrow, indcol, coef), blocks row-major, as tests/bilu4_cases.matrix returns them."""
import functools

import numpy as np

import bilu4_model as M

CHUNK = 64   # block rows per chunk of a wide level
MAX_DEPS = 256


def _from_rows(rows, seed):
    nb = len(rows)
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    col = np.array([c for r in rows for c in sorted(r)], np.int32)
    rng = np.random.default_rng(seed)
    row_of = np.repeat(np.arange(nb), np.diff(ptr))
    val = rng.uniform(-1.0, 1.0, (len(col), 4, 4)) / (4.0 * np.diff(ptr)[row_of])[:, None, None]
    on_diag = np.nonzero(col == row_of)[0]
    val[on_diag] = 4.0 * np.eye(4) + rng.uniform(-0.05, 0.05, (nb, 4, 4))
    return nb, ptr, col, val.reshape(-1)


WIDE3_LEVELS = (130, 64, 65)


def wide3():
    """Three forward levels of 130, 64 and 65 block rows (chunks of 64+64+2, 64, 64+1).  Every row of a level names a few seeded rows
    of the level before; every third row of the last level names rows of the first one directly.  Only every other link (i, j),
    j < i, has its mirror (j, i): L(i, j) without U(j, i) is the write-after-read hazard between the sweeps (the backward sweep
    overwrites t_j while a forward row may still have to read it)."""
    rng = np.random.default_rng(51)
    first = np.concatenate([[0], np.cumsum(WIDE3_LEVELS)])
    rows = [{i} for i in range(int(first[-1]))]
    links = []
    for l in (1, 2):
        for i in range(first[l], first[l + 1]):
            for j in rng.choice(np.arange(first[l - 1], first[l]), 3, replace=False):
                links.append((i, int(j)))
            if l == 2 and i % 3 == 0:
                for j in rng.choice(np.arange(first[0], first[1]), 2, replace=False):
                    links.append((i, int(j)))
    for n, (i, j) in enumerate(links):
        rows[i].add(j)
        if n % 2 == 0:
            rows[j].add(i)
    return _from_rows(rows, 52)


def fold_wide_fold():
    """20 single-row levels, one level of 200 rows, 20 single-row levels; structurally symmetric, so the backward sweep is the mirror."""
    nb = 240
    rows = [{i} for i in range(nb)]

    def link(i, j):
        rows[i].add(j)
        rows[j].add(i)

    for i in range(1, 20):
        link(i, i - 1)
    for i in range(20, 220):
        link(i, 19)
        link(220, i)
    for i in range(221, nb):
        link(i, i - 1)
    return _from_rows(rows, 53)


def arrow200():
    """199 diagonal rows and a last row that names all of them: one row that waits for the four chunks of the level before it."""
    nb = 200
    return _from_rows([{i} for i in range(nb - 1)] + [set(range(nb))], 54)


def over_cap():
    """257 x 64 diagonal rows and a last row that names one row of each of their 257 chunks: one dependency more than a workgroup
    has lanes to poll with.  For the plan probe and the refusal only: nobody factors its model."""
    nb = (MAX_DEPS + 1) * CHUNK + 1
    return _from_rows([{i} for i in range(nb - 1)] + [set(range(0, nb - 1, CHUNK)) | {nb - 1}], 55)


_MAKERS = {"wide3": wide3, "fold_wide_fold": fold_wide_fold, "arrow200": arrow200, "over_cap": over_cap}
SOLVE_CASES = [("wide3", 0), ("fold_wide_fold", 0), ("arrow200", 0)]
PROBE_ONLY = ("over_cap", 0)


@functools.lru_cache(maxsize=None)
def matrix(name):
    return _MAKERS[name]()


@functools.lru_cache(maxsize=None)
def model_factor(name, fill, variant=0):
    nb, bp, bc, bv = matrix(name)
    if variant:
        bv = new_values(name, variant)
    return M.factor(nb, bp, bc, bv, fill)


def new_values(name, variant):
    """Other values on the same pattern: every off-diagonal block scaled by a seeded factor in [0.5, 1.5), diagonal blocks by 1.25."""
    nb, bp, bc, bv = matrix(name)
    rng = np.random.default_rng(177 + variant)
    v = np.array(bv, np.float64).reshape(-1, 4, 4) * rng.uniform(0.5, 1.5, (len(bc), 1, 1))
    on_diag = np.nonzero(bc == np.repeat(np.arange(nb), np.diff(bp)))[0]
    v[on_diag] = np.asarray(bv).reshape(-1, 4, 4)[on_diag] * 1.25
    return v.reshape(-1)
