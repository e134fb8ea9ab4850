"""Seeded patterns at the limits of the one-launch powers step's plan (spmk_ring.hpp, ring_plan.hpp: configuration 4 — 256 threads,
blocks of <= 2048 nonzeros and <= 256 rows, a 5120-entry window, always 512 workgroups), shared by tests/test_spmk_model.py (no GPU)
and tests/test_gpu_spmk_limits.py.  build(name) -> (n, ptrow, indcol, coef); EXPECT[name] = what mi_spmk_plan_probe and
mi_spmk_plan_dump report for it — pinned, so that a planner change that moves a case off its limit is noticed.

  band:n:hb         rows {i - hb .. i + hb} cut at the matrix' edges.
                      1:0 one row, one run that waits for itself, 511 idle runs; 2:1 the same with a second row;
                      256:1 / 257:1 one block / two (a block takes at most T = 256 rows);
                      2000:7 16 blocks in 16 runs of one, and the window's first fill makes every run list all 16;
                      12000:11 / 12000:12 the longest list is 61 (eligible) / 65 (beyond the cap of 64: k launches);
                      131072:1 / 131073:1 512 blocks, one per workgroup / 513: two per run, and 255 of the 512 runs idle
  band64            the cap of 64 itself: band:12000:12 in which every other row reaches only 11 to the left — rows of 25 and 24
                    nonzeros alternately.  Found by varying the share of shorter rows between band:12000:11 (61) and band:12000:12
                    (65): shares of 3/8 .. 5/8 all give 64.
  s15:66000:300     516 blocks, runs of two;  svar:30000:300 variable row lengths (synth.rows)
  jump, swap        n = 12000, hb = 7.  jump: the second half of the rows names the first half's columns (row i >= n / 2 holds the band
                    of row i - n / 2), so the window jumps back in the middle; swap: the halves are exchanged as well (row i < n / 2
                    holds the band of row i + n / 2).  The planner cuts a run where the window jumps: a non-uniform deal (the kernel
                    reads run_rng instead of deriving the runs from bpw) — but ONLY where the jump brings more than T new columns
                    into a block that is not its run's first, and at 12000 rows every run is one block: both keep the uniform deal.
  cut               the pattern that does force a cut: n = 66000 (runs of two), hb = 7, rows from 32896 = 257 * 128 on — the SECOND block
                    of run 128 — hold the band of row i - 32896 + 8000: the window restarts there with 5120 new columns, the planner
                    ends the run before it, and every later run is shifted by a block.  259 live runs, two of them of one block.
  empty:head|mid|tail   band:12000:7 with 700 consecutive empty rows at 0, at 3000, at the end: whole runs of empty blocks (they store
                    zeros, load where the plan says an empty block loads, and are waited for like any other run)
  len16, len8       every row exactly 16 / 8 nonzeros: ring_wants_skew is true for such a matrix by itself (SKEW instantiations)
  long:2048|2049    one row of that many nonzeros inside band:12000:7: a block of its own / longer than a block (a PLAIN block behind the
                    loop: not eligible)
Values: uniform in [-1, 1] over the row's length, so that eight powers stay finite and far from the denormals."""
import numpy as np

from navierstokes_amd import synth

N0 = 12000


def _from_cols(cols, ok):
    p = np.concatenate([[0], np.cumsum(ok.sum(axis=1))]).astype(np.int32)
    return p, cols[ok].astype(np.int32)


def _band(n, lo, hi, centre=None):
    """row i holds centre[i] - lo .. centre[i] + hi (lo, hi scalars or per row), cut at the edges"""
    i = np.arange(n, dtype=np.int64) if centre is None else np.asarray(centre, np.int64)
    lo = np.broadcast_to(np.asarray(lo, np.int64), (n,))
    hi = np.broadcast_to(np.asarray(hi, np.int64), (n,))
    d = np.arange(-int(lo.max()), int(hi.max()) + 1, dtype=np.int64)
    cols = i[:, None] + d[None, :]
    ok = (cols >= 0) & (cols < n) & (d[None, :] >= -lo[:, None]) & (d[None, :] <= hi[:, None])
    return _from_cols(cols, ok)


def _without_rows(p, c, r0, r1):
    lens = np.diff(p).astype(np.int64)
    keep = np.ones(len(c), bool)
    keep[p[r0]:p[r1]] = False
    lens[r0:r1] = 0
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), c[keep]


def _exact(n, length):
    start = np.clip(np.arange(n, dtype=np.int64) - length // 2, 0, n - length)
    c = (start[:, None] + np.arange(length)[None, :]).astype(np.int32).ravel()
    return (np.arange(n + 1, dtype=np.int64) * length).astype(np.int32), c


def _long(n, length, row=5000):
    p, c = _band(n, 7, 7)
    lens = np.diff(p).astype(np.int64)
    first = row - length // 2
    c = np.concatenate([c[:p[row]], np.arange(first, first + length, dtype=np.int32), c[p[row + 1]:]])
    lens[row] = length
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), c


def pattern(name):
    f = name.split(":")
    if f[0] == "band":
        n, hb = int(f[1]), int(f[2])
        return (n,) + _band(n, hb, hb)
    if f[0] == "band64":
        return (N0,) + _band(N0, np.where(np.arange(N0) % 2 == 0, 12, 11), 12)
    if f[0] in ("s15", "svar"):
        n = int(f[1])
        p, c, _ = synth.rows(f[0], n, w=int(f[2]))
        return n, p, c
    if f[0] == "jump":
        i = np.arange(N0)
        return (N0,) + _band(N0, 7, 7, centre=np.where(i < N0 // 2, i, i - N0 // 2))
    if f[0] == "swap":
        i = np.arange(N0)
        return (N0,) + _band(N0, 7, 7, centre=np.where(i < N0 // 2, i + N0 // 2, i - N0 // 2))
    if f[0] == "cut":
        n, h = 66000, 257 * 128
        i = np.arange(n)
        return (n,) + _band(n, 7, 7, centre=np.where(i < h, i, i - h + 8000))
    if f[0] == "empty":
        r0 = dict(head=0, mid=3000, tail=N0 - 700)[f[1]]
        return (N0,) + _without_rows(*_band(N0, 7, 7), r0, r0 + 700)
    if f[0] in ("len16", "len8"):
        return (N0,) + _exact(N0, int(f[0][3:]))
    if f[0] == "long":
        return (N0,) + _long(N0, int(f[1]))
    raise KeyError(name)


_CACHE = {}


def build(name):
    """(n, ptrow, indcol, coef) of a case — built once, shared, never written to"""
    if name not in _CACHE:
        n, p, c = pattern(name)
        p = np.ascontiguousarray(p, np.int32)
        c = np.ascontiguousarray(c, np.int32)
        rng = np.random.default_rng(sum(name.encode()) + 977 * len(name))
        lens = np.maximum(np.diff(p), 1)
        v = rng.uniform(-1.0, 1.0, len(c)) / np.repeat(lens, np.diff(p))
        for a in (p, c, v):
            a.setflags(write=False)
        _CACHE[name] = (n, p, c, v)
    return _CACHE[name]


# name: (eligible, row blocks, blocks per run of the uniform deal, longest dependency list [0: no lists], uniform deal)
EXPECT = {
    "band:1:0": (True, 1, 1, 1, True),
    "band:2:1": (True, 1, 1, 1, True),
    "band:256:1": (True, 1, 1, 1, True),
    "band:257:1": (True, 2, 1, 2, True),
    "band:2000:7": (True, 16, 1, 16, True),
    "band:12000:11": (True, 141, 1, 61, True),
    "band64": (True, 146, 1, 64, True),
    "band:12000:12": (False, 150, 1, 65, True),
    "band:131072:1": (True, 512, 1, 21, True),
    "band:131073:1": (True, 513, 2, 12, True),
    "s15:66000:300": (True, 516, 2, 22, True),
    "svar:30000:300": (True, 234, 1, 41, True),
    "jump": (True, 94, 1, 42, True),
    "swap": (True, 94, 1, 42, True),
    "cut": (True, 516, 2, 23, False),
    "empty:head": (True, 91, 1, 41, True),
    "empty:mid": (True, 91, 1, 41, True),
    "empty:tail": (True, 91, 1, 41, True),
    "len16": (True, 94, 1, 41, True),
    "len8": (True, 47, 1, 21, True),
    "long:2048": (True, 96, 1, 43, True),
    "long:2049": (False, 96, 1, 0, True),
}
CASES = list(EXPECT)
INELIGIBLE = [nm for nm, e in EXPECT.items() if not e[0]]
