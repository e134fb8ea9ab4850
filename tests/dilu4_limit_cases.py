"""The matrices of tests/test_dilu4_limit_cases.py and tests/test_gpu_dilu4_limits.py: the patterns on which the block loop of
dilu4_row (dilu4_kernels.hpp), restated from bilu4_level_wide, meets every limit of its four-deep pipeline in BOTH kernels that
have it (dilu4_level, dilu4_folded) and in both triangles, and on which the launcher meets every limit of its rule.

  wide         tests/bilu4_wide_cases.py: levels of 63, 64, 65, 127, 128 and 129 rows, already in colour order; its unfolded levels
               hold rows with every count of WANTED in each triangle
  limits:3     the layered pattern of tests/bilu4_cases.py with three far links per row: its narrow levels (folded) hold rows with
               every count of WANTED RIGHT of the diagonal
  limits:3~    the same matrix with block row i renumbered nb-1-i (mirror): the two triangles and the two schedules change places,
               so the folded rows have every count of WANTED LEFT of the diagonal
  fold_deep    252 narrow levels: in natural order each sweep is ONE folded launch with a barrier per level
  alternating  48 levels of 63, 64, 63, 64, .. rows: in natural order the launcher changes kernel at every level
  wide:N       ONE level of N block rows with no off-diagonal block: N = 63 folds, 64 is one whole workgroup, 65 one quad over
  tiny:N       a chain of N block rows: one quad, exactly one wave of quads, one quad over

matrix(name) is (nb, ptrow, indcol, coef) with the blocks row-major; values(name, 1) is a second set of values on the same pattern
(bilu4_cases._values under another seed), for a refactor."""
import functools

import numpy as np

import bilu4_cases as C
import bilu4_wide_cases as W
import dilu4_model as DM

P = 4  # kDiluDepth: the depth of the block loop's pipeline
FOLD_BELOW = 64  # a level of fewer block rows runs in dilu4_folded, any other in dilu4_level (Bilu4Launch::folded)
# off-diagonal blocks per row.  0: the loop is skipped; 1: every stage of the prologue clamps to the one block; P-1, P: one round, its
# last stage guarded off or not; P+1: a second round, whose one live block came in with the column the PROLOGUE fetched a round
# ahead; 2P-1, 2P: that round guarded in its last stage or whole, every refill clamped; 2P+1: a third round, whose one live block is
# the first to come in with a column of the 2P-ahead refill; 3P, 3P+1: the same one round later, both refills in steady state
WANTED = (0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 3 * P, 3 * P + 1)
REFACTOR_SEED = 977
NAMES = ("wide", "limits:3", "limits:3~", "fold_deep", "alternating", "wide:63", "wide:64", "wide:65", "tiny:1", "tiny:16", "tiny:17")


def mirror(nb, ptr, col, val):
    """The same matrix with block row i renumbered nb-1-i (and block column j renumbered nb-1-j), columns ascending again: what was
    left of the diagonal is right of it, and the forward schedule is the old backward one."""
    ptr, col = np.asarray(ptr), np.asarray(col)
    val = np.asarray(val, np.float64).reshape(-1, 16)
    # new row n is old row nb-1-n; its old columns ascending are its new columns descending: reverse the row
    order = np.concatenate([np.arange(ptr[i + 1] - 1, ptr[i] - 1, -1) for i in range(nb - 1, -1, -1)]) if nb else np.zeros(0, np.int64)
    mptr = np.concatenate([[0], np.cumsum(np.diff(ptr)[::-1])]).astype(np.int32)
    mcol = (nb - 1 - col[order]).astype(np.int32)
    return nb, mptr, mcol, val[order].reshape(-1).copy()


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name not in NAMES:
        raise KeyError(name)
    if name == "wide":
        return W.matrix()
    if name.endswith("~"):
        return mirror(*C.matrix(name[:-1]))
    if name.startswith("tiny:"):
        return C.chain(int(name.partition(":")[2]))
    return C.matrix(name)  # limits:3, fold_deep, alternating, wide:N


@functools.lru_cache(maxsize=None)
def values(name, variant=0):
    nb, bp, bc, bv = matrix(name)
    if not variant:
        return np.asarray(bv, np.float64)
    return C._values(nb, bp, bc, REFACTOR_SEED + variant)


@functools.lru_cache(maxsize=None)
def model(name, order, variant=0):
    """tests/dilu4_model.py's model of a handle on matrix(name) with values(name, variant): computed once per process, read-only
    (fold_deep takes about a second, and each of its sweeps another)."""
    nb, bp, bc, _ = matrix(name)
    return DM.Ordered(nb, bp, bc, values(name, variant), order)


def counts_by_kernel(m):
    """{(triangle, kernel): the set of off-diagonal block counts of its rows}, triangle "left" (the forward sweeps: to_hat and the
    second half of apply_hat) or "right" (the backward sweep: from_hat), kernel "folded" or "unfolded" by the width of the row's
    level in THAT sweep.  m: a dilu4_model.Dilu, or an Ordered (whose B it is)."""
    D = getattr(m, "B", m)
    left = np.asarray(D.diag) - np.asarray(D.ptr[:-1])
    right = np.asarray(D.ptr[1:]) - np.asarray(D.diag) - 1
    out = {(t, k): set() for t in ("left", "right") for k in ("folded", "unfolded")}
    for triangle, S, counts in (("left", D.F, left), ("right", D.Bw, right)):
        for l in range(S["nlev"]):
            rows = S["perm"][S["lev_ptr"][l]:S["lev_ptr"][l + 1]]
            kernel = "folded" if len(rows) < FOLD_BELOW else "unfolded"
            out[(triangle, kernel)].update(int(c) for c in counts[rows])
    return out
