"""The hand-built pattern of tests/test_gpu_bilu4_wide_limits.py: block rows in layers, ALREADY in colour order — the greedy rule
(tests/bilu4_order_cases.py) gives layer l colour l and the identity permutation — with prescribed level widths in both sweeps
and prescribed numbers of off-diagonal blocks per row in both triangles.

Links (all stored both ways, so the pattern is structurally symmetric):
  down     row r of layer l is linked to row r mod w_m of EVERY layer m < l: it cannot take a colour below l, and its forward
           level is l; from these alone it has exactly l blocks left of the diagonal
  cover    row r of layer l is linked to row r mod w_{l+1} of layer l + 1: every row is needed by the layer above, so the
           backward levels are the layers reversed
No link joins two rows of one layer."""
import functools

import numpy as np

import bilu4_cases as C

P = 4  # kBiluSweepDepth: the depth of the wide kernel's pipeline
WIDE_MIN = 64  # MI355_BILU_WIDE_MIN of the limit tests
# both sides of one workgroup (64 block rows) and of two; 63 is a folded launch between wide ones; 129 and 65 leave a last
# workgroup with one quad.  Thirteen layers: rows with 0 .. 12 blocks left of the diagonal.
WIDTHS = (64, 65, 63, 127, 128, 129, 64, 63, 65, 128, 129, 127, 64)
WANTED_COUNTS = (0, 1, P - 1, P, P + 1, 2 * P + 1)


@functools.lru_cache(maxsize=None)
def matrix():
    first = np.concatenate([[0], np.cumsum(WIDTHS)]).astype(np.int64)
    rows = [{i} for i in range(int(first[-1]))]

    def link(i, j):
        rows[int(i)].add(int(j))
        rows[int(j)].add(int(i))

    for l, w in enumerate(WIDTHS):
        for r in range(w):
            for m in range(l):
                link(first[l] + r, first[m] + r % WIDTHS[m])
            if l + 1 < len(WIDTHS):
                link(first[l] + r, first[l + 1] + r % WIDTHS[l + 1])
    return C._from_rows(rows, 61)


def layer_of():
    return np.repeat(np.arange(len(WIDTHS)), WIDTHS)


def offdiag_counts():
    """(blocks left of the diagonal, blocks right of it) per block row."""
    nb, bp, bc, _ = matrix()
    row = np.repeat(np.arange(nb), np.diff(bp))
    return np.bincount(row[bc < row], minlength=nb), np.bincount(row[bc > row], minlength=nb)
