"""Block patterns at the limits of the multi-vector product's tile plan (navierstokes_amd/csrc/spmm_tile_plan.hpp, spmm_tile.hpp), shared by
tests/test_spmm_tile_plan.py (CPU: the plan's invariants through mi_bcsr4_spmm_plan_probe) and tests/test_gpu_spmm_tile_limits.py (GPU:
forms 1-3 bit for bit against the oracle).

A case is (nbrows, nbcols, bp, bc) with seeded block values from uniform(-1, 1).  Every pattern holds at least MIN_BLOCKS blocks — below
that the handle builds no plan — except `below:4095`, and at most MAX_BLOCKS, so that a case costs milliseconds; case() asserts both.

  grid            3-D 7-point block grid, 11 x 10 x 9 = 990 block rows (990 % 128 = 94, 990 % 64 = 30)
  rows:N          N in 127, 128, 129, 63, 64, 65: ONE connected band (row r holds columns r .. r + w - 1): the block-row count against `per`
  rowsdiag:N      the same counts, diagonal-only rows (every row a component of its own) and four dense rows to reach MIN_BLOCKS
  components:fwd  disconnected pieces of 1, 2, 63, 64, 65, 127, 128, 129, 300 block rows; components:rev the same in reverse
  empty           row 0 empty; rows 1-255 a band (so that the clusters before it are full: 2 x 128, 4 x 64); rows 256-383 empty and named by
                  no block (a tile whose list is empty); empty rows interleaved with rows of one block; a band; the last three rows empty
  lengths         rows of 1, 2, 3, 4, 5, 7, 8, 9, 13 blocks interleaved (P - 1, P, P + 1, 2 P, 2 P + 1 for the pipeline depths 3 and 4)
  repeated        a band with one row that repeats block columns out of order and one with descending columns
  rect_wide       nbcols = nbrows + 500, every row with a block in the extra columns; rect_tall: nbcols = nbrows - 500
  long:L          a band and one block row of L distinct block columns; L at both sides of umax (4 s + 2) 8 <= 163 840 for s = 8 ... 1
  below:N         N = 4095, 4096 diagonal-only block rows

SMALL_CAPS are MI355_SPMM_TILE_UCAP settings ("<128-row cap>,<64-row cap>") that make the planner halve once, several times, and down to
single rows."""
import numpy as np

MIN_BLOCKS = 4096
MAX_BLOCKS = 20000
LDS_BYTES = 160 * 1024
DEFAULT_CAPS = (368, 256)
SMALL_CAPS = ("40,24", "12,12", "1,1")
ROW_COUNTS = (127, 128, 129, 63, 64, 65)
COMPONENT_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 300)
ROW_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 13)
LONG = (602, 603, 787, 788, 1137, 1138, 1462, 1463, 2048, 2049, 3413, 3414)


def lds_bytes(umax, s):
    """Dynamic LDS of a tile launch at s columns: node records of 4 s + 2 doubles (spmm_tile.hpp)."""
    return umax * (4 * s + 2) * 8


class Case:
    def __init__(self, name, nbrows, nbcols, rows, seed):
        """rows: one sequence of block columns per block row, in stored order."""
        self.name, self.nbrows, self.nbcols, self.seed = name, int(nbrows), int(nbcols), seed
        assert len(rows) == nbrows
        lens = np.array([len(r) for r in rows], np.int64)
        self.bp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        self.bc = (np.concatenate([np.asarray(r, np.int64) for r in rows]) if lens.sum() else np.zeros(0, np.int64)).astype(np.int32)
        self.nblocks = int(self.bp[-1])
        assert self.nblocks == 0 or (0 <= self.bc.min() and self.bc.max() < self.nbcols), name
        self._bv = None

    @property
    def bv(self):
        if self._bv is None:
            self._bv = np.random.default_rng(self.seed).uniform(-1, 1, 16 * self.nblocks)
        return self._bv

    def values(self, seed):
        return np.random.default_rng(seed).uniform(-1, 1, 16 * self.nblocks)

    def x(self, s, seed=0):
        """(s, 4 nbcols) columns from uniform(-1, 1)."""
        return np.random.default_rng(1_000_003 * (seed + 1) + self.seed).uniform(-1, 1, (s, 4 * self.nbcols))

    def row_cols(self, r):
        return self.bc[self.bp[r]:self.bp[r + 1]]

    def __repr__(self):
        return self.name


def _band(n, half, lo=0, hi=None):
    """Rows lo .. hi - 1 of n: columns within `half` of the diagonal, clipped to [lo, hi)."""
    hi = n if hi is None else hi
    return [list(range(max(lo, r - half), min(hi, r + half + 1))) for r in range(lo, hi)]


def _grid(nx, ny, nz):
    rows = []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                me = (k * ny + j) * nx + i
                nb = [me]
                if i > 0: nb.append(me - 1)
                if i < nx - 1: nb.append(me + 1)
                if j > 0: nb.append(me - nx)
                if j < ny - 1: nb.append(me + nx)
                if k > 0: nb.append(me - nx * ny)
                if k < nz - 1: nb.append(me + nx * ny)
                rows.append(sorted(nb))
    return rows


def _build(name):
    kind, _, arg = name.partition(":")
    if kind == "grid":
        rows = _grid(11, 10, 9)
        return Case(name, len(rows), len(rows), rows, 11)
    if kind == "rows":
        n = int(arg)
        w = -(-MIN_BLOCKS // n) + 1
        return Case(name, n, n + w - 1, [list(range(r, r + w)) for r in range(n)], 20 + n)
    if kind == "rowsdiag":
        n = int(arg)
        dense = (1, n // 2, n - 2, n - 3)
        w = -(-(MIN_BLOCKS - (n - len(dense))) // len(dense))
        rows = [[r] for r in range(n)]
        for i, r in enumerate(dense):  # the row's own node and w - 1 columns beyond the rows, which join no two rows
            rows[r] = [r] + list(range(n + 37 * i, n + 37 * i + w - 1))
        return Case(name, n, n + 37 * len(dense) + w, rows, 40 + n)
    if kind == "components":
        sizes = COMPONENT_SIZES if arg == "fwd" else COMPONENT_SIZES[::-1]
        n, rows, lo = sum(sizes), [], 0
        for m in sizes:
            rows += _band(n, 2, lo, lo + m)
            lo += m
        return Case(name, n, n, rows, 60 + len(arg))
    if kind == "empty":
        rows = [[]] + _band(256, 2, 1, 256) + [[] for _ in range(128)]
        lo = len(rows)                                              # 384
        rows += [[r] if r % 2 else [] for r in range(lo, lo + 200)]  # empty rows interleaved with rows of one block
        lo = len(rows)
        n = lo + 520 + 3
        rows += _band(n, 3, lo, lo + 520)
        rows += [[], [], []]
        return Case(name, n, n, rows, 71)
    if kind == "lengths":
        n = 801
        rows = [list(range(r, r + ROW_LENGTHS[r % len(ROW_LENGTHS)])) for r in range(n)]
        return Case(name, n, n + max(ROW_LENGTHS), rows, 72)
    if kind == "repeated":
        n = 700
        rows = _band(n, 3)
        rows[10] = [12, 10, 10, 11, 12, 300, 10]   # repeated, not ascending: blocks share slots, the chain runs in stored order
        rows[20] = [24, 23, 22, 21, 20, 5]         # descending
        rows[n - 1] = [n - 1, n - 1]
        return Case(name, n, n, rows, 73)
    if kind == "rect_wide":
        n = 900
        rows = [r + [n + (7 * i) % 500] for i, r in enumerate(_band(n, 2))]
        rows[5] += [n + 499]
        return Case(name, n, n + 500, rows, 74)
    if kind == "rect_tall":
        n, nc = 1300, 800
        rows = [sorted({(r + j) % nc for j in range(4)}) for r in range(n)]
        return Case(name, n, nc, rows, 75)
    if kind == "long":
        L, n = int(arg), 900
        rows = _band(n, 2)
        rows[450] = list(range(50, 50 + L))
        return Case(name, n, max(n, L + 100), rows, 100 + L)
    if kind == "below":
        n = int(arg)
        return Case(name, n, n, [[r] for r in range(n)], 90)
    raise KeyError(name)


NAMES = (["grid"] + [f"rows:{n}" for n in ROW_COUNTS] + [f"rowsdiag:{n}" for n in ROW_COUNTS] + ["components:fwd", "components:rev", "empty", "lengths",
         "repeated", "rect_wide", "rect_tall"] + [f"long:{L}" for L in LONG] + ["below:4095", "below:4096"])
CAPPED = [(name, caps) for name in ("grid", "components:fwd", "components:rev") for caps in SMALL_CAPS]

_CASES = {}


def case(name):
    if name not in _CASES:
        C = _build(name)
        if name != "below:4095":
            assert MIN_BLOCKS <= C.nblocks <= MAX_BLOCKS, (name, C.nblocks)
        else:
            assert C.nblocks == MIN_BLOCKS - 1
        _CASES[name] = C
    return _CASES[name]


def caps_of(ucap_env):
    """(128-row cap, 64-row cap) of an MI355_SPMM_TILE_UCAP setting, None for the defaults."""
    if ucap_env is None:
        return DEFAULT_CAPS
    a, b = ucap_env.split(",")
    return int(a), int(b)


def expected_form(C, plan128, plan64, form, s):
    """The form a product of s <= 8 columns runs when `form` is forced (include/mi355_spmv.h: mi_bcsr4_spmm_info, mi_bcsr4_spmm_plan_probe):
    the lists are built from 4 096 blocks on and only if the 128-row plan exists; form 1 takes up to four columns on the 128-row plan,
    forms 2 and 3 even column counts on the 64-row plan; the longest list's records must fit 160 KiB of LDS.  Else the gather kernels."""
    if C.nblocks < MIN_BLOCKS or plan128["refused"]:
        return 0
    if form == 1:
        return 1 if s <= 4 and lds_bytes(plan128["umax"], s) <= LDS_BYTES else 0
    if form in (2, 3):
        return form if s % 2 == 0 and s <= 8 and not plan64["refused"] and lds_bytes(plan64["umax"], s) <= LDS_BYTES else 0
    raise ValueError(form)


def expected_longest_list(C, plan128, plan64, s):
    """mi_bcsr4_spmm_info's longest_list after the first product: the 128-row plan's where form 1 could run at s, else the 64-row plan's."""
    if C.nblocks < MIN_BLOCKS or plan128["refused"]:
        return 0
    if s <= 4 and lds_bytes(plan128["umax"], s) <= LDS_BYTES:
        return plan128["umax"]
    return 0 if plan64["refused"] else plan64["umax"]


def to_csr(C, bv=None):
    """The block matrix written out as CSR with node blocks of 4 (square patterns with ascending columns per row)."""
    bv = C.bv if bv is None else bv
    lens = np.repeat(np.diff(C.bp), 4) * 4
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    c = np.empty(p[-1], np.int32)
    v = np.empty(p[-1], np.float64)
    B = np.asarray(bv).reshape(-1, 4, 4)
    for r in range(C.nbrows):
        k0, k1 = C.bp[r], C.bp[r + 1]
        cols = (4 * C.bc[k0:k1, None] + np.arange(4)[None, :]).ravel()
        for q in range(4):
            o = p[4 * r + q]
            c[o:o + len(cols)] = cols
            v[o:o + len(cols)] = B[k0:k1, q, :].ravel()
    return p, c, v
