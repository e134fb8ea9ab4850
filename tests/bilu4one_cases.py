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


def fan(k):
    """One consumer per sweep that waits for exactly k chunks.  nb = 64 k + 2; rows 1 .. 64 k are diagonal; row 0 has a U block at
    column 64 c + 6 for every c < k (no mirror), the last row an L block at the same columns.  Forward: level 0 is rows 0 .. 64 k
    (k chunks of 64 and the one-row chunk of row 64 k), level 1 the last row, which names row 64 c + 6 of chunk c.  Backward: level 0
    is rows 1 .. 64 k + 1, where row 64 c + 6 lies at position 64 c + 5 of chunk c, and level 1 is row 0.  So k + 2 chunks per sweep
    and a last chunk with k dependencies, 0 .. k - 1: lane d of the poll waits for chunk d."""
    nb = CHUNK * k + 2
    named = set(range(6, CHUNK * k, CHUNK))
    return _from_rows([{0} | named] + [{i} for i in range(1, nb - 1)] + [named | {nb - 1}], 60 + k)


FAN_LATE_CHAIN = 200  # single-row levels the last-listed dependency of fan_late's consumer has to wait for (profiles/NOTES.md R7.2)


def fan_late(k, chain=None):
    """A consumer with k dependencies whose LAST-listed one is the last to finish.  L links only.  64 (k - 1) diagonal rows (chunks
    0 .. k - 2); a chain of `chain` single-row levels, the first naming diagonal row 7, each later one its predecessor (one folded
    chunk, k - 1); one level of 64 rows that all name the end of the chain (chunk k); a last row (chunk k + 1) that names row 64 c + 9
    of every diagonal chunk and row 11 of the 64-row level.  Its dependency list is 0 .. k - 2, k: lane k - 1 polls the 64-row chunk,
    which cannot finish before the whole chain has, while every other lane's flag is set at once."""
    chain = FAN_LATE_CHAIN if chain is None else chain
    nd = CHUNK * (k - 1)
    rows = [{i} for i in range(nd)]
    rows += [{nd + j, 7 if j == 0 else nd + j - 1} for j in range(chain)]
    wide = nd + chain
    rows += [{wide + r, wide - 1} for r in range(CHUNK)]
    rows.append(set(range(9, nd, CHUNK)) | {wide + 11, wide + CHUNK})
    return _from_rows(rows, 400 + k)


SPREAD_CONSUMERS = CHUNK + 1


def spread_links(k):
    """(consumer row, named diagonal row) of spread(k), in the order they are made."""
    first = CHUNK * k
    return [(first + r, CHUNK * c + (7 * r + r // CHUNK + 3 * (c // CHUNK)) % CHUNK) for r in range(SPREAD_CONSUMERS) for c in range(r, k, CHUNK)]


def spread(k):
    """A chunk with k dependencies none of whose rows has more than 4 off-diagonal blocks: the polling lanes are not the rows' lanes.
    64 k diagonal rows (chunks 0 .. k - 1), then one level of 65 consumer rows (chunks of 64 and 1).  Consumer row r names one row
    of each diagonal chunk r, r + 64, r + 128, r + 192 below k, so the first consumer chunk names every diagonal chunk once and the
    second at most 4.  Every second link has its mirror, as in wide3: the mirrored diagonal rows form the backward sweep's level 1."""
    rows = [{i} for i in range(CHUNK * k + SPREAD_CONSUMERS)]
    for n, (i, j) in enumerate(spread_links(k)):
        rows[i].add(j)
        if n % 2 == 0:
            rows[j].add(i)
    return _from_rows(rows, 700 + k)


_MAKERS = {"wide3": wide3, "fold_wide_fold": fold_wide_fold, "arrow200": arrow200, "over_cap": over_cap}
_FAMILIES = {"fan": fan, "fan_late": fan_late, "spread": spread}
SOLVE_CASES = [("wide3", 0), ("fold_wide_fold", 0), ("arrow200", 0)]
PROBE_ONLY = ("over_cap", 0)
# the limits of the hand-off: 63 / 64 / 65 dependencies (one wave of polling lanes, exactly; one lane of a second wave), 128 / 129
# (two waves, a third), 255 / 256 (one lane short of the workgroup; every lane — the cap)
FAN_KS = (63, 64, 65, 128, 129, 255, 256)
LIMIT_CASES = [(f"fan:{k}", 0) for k in FAN_KS] + [(f"fan_late:{k}", 0) for k in (64, 65, 256)] + [(f"spread:{k}", 0) for k in (65, 256)]
FAN_OVER_CAP = (f"fan:{MAX_DEPS + 1}", 0)  # for the plan probe and the refusal only, as over_cap — but over the cap on BOTH sweeps


def limit_k(name):
    """The k of a LIMIT_CASES name: the number of dependencies of its widest consumer."""
    return int(name.partition(":")[2])


@functools.lru_cache(maxsize=None)
def matrix(name):
    kind, _, arg = name.partition(":")
    if kind in _FAMILIES:
        return _FAMILIES[kind](int(arg))
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
