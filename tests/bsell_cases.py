"""Cases at the limits of the blocked sliced-stream plan (tests/test_bsell_limits.py; TEST INFRASTRUCTURE, not a conftest).

Three parts:
  restate        a plain restatement of build_sell_plan and build_sell_wave_ranges (spmv_bcsr_sell.hpp), written from the layout the
                 header describes and independent of the library: the slice lengths, sptr with its three terminators, the column
                 stream (block column, pad bit and first-step flag of every place, the 48 tail steps), the wave count and the wave
                 ranges for both caps (1024: variants 0, 1, 3 and the multi-vector product; 2048: variant 2) — and what the kernels'
                 branches depend on: slices and steps per wave, empty waves, empty slices, the longest slice's values, the padding.
  TABLE          deterministic cases, each on one side of one limit, tagged with what it claims; every claim is checked against
                 the restatement (CLAIMS), never against the library.
  seeded_cases   about 100 seeded ragged patterns around the same limits.

A tag is "<limit>:<side>" (LIMITS lists the sides every limit must have a case on) or a bare feature name (FEATURES)."""
import functools
import math

import numpy as np

# ---- constants of spmv_bcsr_sell.hpp / capi_bcsr.hip ---------------------------------------------------------------------------
ROWS, PADSTEPS = 16, 48
PAD, FIRST, MASK = 0x80000000, 0x40000000, 0x3FFFFFFF
CAPS = (1024, 2048)
PARK = {"w1": 32, "w2": 32, "mm4": 16, "mm8": 8}       # slices a wave parks before it stores: single vector (both caps), 4 and 8 columns
PARK_CAP = {"w1": 1024, "w2": 2048, "mm4": 1024, "mm8": 1024}
DEPTH = {0: 8, 1: 8, 2: 4, 3: 12}                      # steps per trip of the single-vector variants
DEPTH_MM = 6                                           # ... of the multi-vector kernel
FORM_CAP = {0: 1024, 1: 1024, 2: 2048, 3: 1024}
TIER_SMALL, TIER_LARGE = 4096, 16384                   # LDS doubles of the refresh kernels' staging buffers
GRID, GRID_LARGE = 2048, 256                           # their grids (the 16384 tier's is capped lower)
MAX_BLOCKS = 400_000

# Limits that could not be built, and why (test_bsell_limits.py checks that none of them is claimed by a case).
NOT_REACHED = {}


def wave_count(nslices, cap):
    """min(cap, max(32, nslices / 2 rounded up to a multiple of 32))"""
    return min(cap, max(32, 32 * math.ceil((nslices // 2) / 32)))


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def restate(nbrows, ptrow, indcol):
    """The plan of a block pattern.  Returns a dict: nslices, nsteps, slice_len, slice_blocks, sptr (nslices + 3), col
    ((nsteps + 48, 16) uint32), max_slice_vals, padding (as mi_bcsr4_sell_info reports it), and per cap c in CAPS under key c:
    dict(nwaves, wrng, spw = slices per wave, wsteps = steps per wave range)."""
    ptrow = np.asarray(ptrow, np.int64)
    indcol = np.asarray(indcol, np.int64)
    ns = -(-nbrows // ROWS)
    lens = np.diff(ptrow[: nbrows + 1])
    nb = int(lens.sum())
    per = np.zeros(ns * ROWS, np.int64)
    per[:nbrows] = lens
    per = per.reshape(ns, ROWS)
    slice_len = np.maximum(per.max(axis=1), 1) if ns else np.zeros(0, np.int64)  # a slice of empty rows is one padding step
    first = np.concatenate([[0], np.cumsum(slice_len)]).astype(np.int64)        # first[s]: first step of slice s; first[ns] = all steps
    nsteps = int(first[-1])
    col = np.full((nsteps + PADSTEPS, ROWS), PAD, np.uint32)
    rows = np.repeat(np.arange(nbrows), lens)
    place = np.arange(nb) - ptrow[rows]                                          # a block is the place-th of its row
    col[first[rows // ROWS] + place, rows % ROWS] = indcol[:nb].astype(np.uint32)
    col[first] |= np.uint32(FIRST)                                               # every slice's first step, and the step behind the last slice
    slice_blocks = per.sum(axis=1)
    R = dict(nslices=ns, nsteps=nsteps, slice_len=slice_len, slice_blocks=slice_blocks, first=first,
             sptr=np.concatenate([first, [nsteps, nsteps]]).astype(np.int32), col=col,
             max_slice_vals=16 * int(slice_blocks.max()) if ns else 0,
             padding=float(nsteps) * ROWS / float(nb) - 1.0 if nb else 0.0, nblocks=nb)
    for cap in CAPS:
        W = wave_count(ns, cap)
        # wave w begins at the first slice that starts at or behind w / W of all steps
        inner = np.searchsorted(first[:ns], nsteps * np.arange(1, W, dtype=np.int64) // W, side="left")
        wrng = np.concatenate([[0], inner, [ns]]).astype(np.int32)
        R[cap] = dict(nwaves=W, wrng=wrng, spw=np.diff(wrng), wsteps=first[wrng[1:]] - first[wrng[:-1]])
    return R


def refresh_tier(max_slice_vals):
    """(LDS doubles of the refresh kernels' instantiation; 0: unstaged, its grid cap)"""
    if max_slice_vals <= TIER_SMALL:
        return TIER_SMALL, GRID
    if max_slice_vals <= TIER_LARGE:
        return TIER_LARGE, GRID_LARGE
    return 0, GRID


# ---- what a tag claims, measured on the restatement ---------------------------------------------------------------------------------
def _max_spw(which):
    return lambda c, R: str(int(R[PARK_CAP[which]]["spw"].max()))


def _range_side(D, cap):
    def f(c, R):  # the sides some non-empty wave range of this case lies on
        st = R[cap]["wsteps"][R[cap]["spw"] > 0]
        return {s for s, hit in (("lt", (st < D).any()), ("eq", (st == D).any()), ("gt", (st == D + 1).any())) if hit}
    return f


def _empty_waves(R, cap):
    e = np.nonzero(R[cap]["spw"] == 0)[0]
    full = np.nonzero(R[cap]["spw"] > 0)[0]
    return e, full


def _feature(name):
    def f(c, R):
        empty = R["slice_blocks"] == 0
        ns = R["nslices"]
        if name == "no_blocks":
            return R["nblocks"] == 0 and c.nbrows > 0
        if name == "onestep":
            return ns > 0 and (R["slice_len"] == 1).all() and R["nblocks"] > 0
        if name == "empty_slice_first":
            return ns > 1 and empty[0] and not empty.all()
        if name == "empty_slice_last":
            return ns > 1 and empty[-1] and not empty.all()
        if name in ("empty_slice_mid_range", "empty_slice_whole_range"):
            for cap in CAPS:
                w = R[cap]["wrng"]
                for a, b in zip(w[:-1], w[1:]):
                    if name == "empty_slice_mid_range" and b - a >= 3 and empty[a + 1: b - 1].any() and not empty[a: b].all():
                        return True
                    if name == "empty_slice_whole_range" and b > a and empty[a:b].all() and not empty.all():
                        return True
            return False
        if name.startswith("empty_waves_"):
            for cap in CAPS:
                e, full = _empty_waves(R, cap)
                if not len(e) or not len(full):
                    continue
                if name == "empty_waves_front" and e[0] < full[0]:
                    return True
                if name == "empty_waves_back" and e[-1] > full[-1]:
                    return True
                if name == "empty_waves_middle" and ((e > full[0]) & (e < full[-1])).any():
                    return True
            return False
        if name.startswith("stride_"):  # more slices than the grid of the refresh tier the case lies in
            cap, grid = refresh_tier(R["max_slice_vals"])
            return cap == {"stride_4096": TIER_SMALL, "stride_16384": TIER_LARGE, "stride_unstaged": 0}[name] and ns > grid
        if name == "tail_full":  # the last step of the stream holds a block in the last quad of the last slice
            return c.nbrows > 0 and c.nbrows % ROWS == 0 and (R["col"][R["nsteps"] - 1, ROWS - 1] & PAD) == 0
        if name == "neg_zero":
            return c.special == "neg_zero" and R["padding"] > 0
        if name == "square":
            return c.nbrows == c.nbcols
        if name.startswith("rows_"):
            return c.nbrows == int(name[5:])
        raise KeyError(name)
    return f


# limit -> (sides every limit needs a case on, function (case, restatement) -> the side or set of sides the case lies on)
LIMITS = {
    "slice_rows": (("lt", "eq", "gt"), lambda c, R: {"lt": c.nbrows % ROWS == ROWS - 1, "eq": c.nbrows % ROWS == 0, "gt": c.nbrows % ROWS == 1}),
    "waves_floor": (("in", "out"), lambda c, R: "in" if R[1024]["nwaves"] == 32 else "out"),          # 32 waves up to 65 slices
    "waves_cap1024": (("in", "out"), lambda c, R: "in" if 32 * math.ceil((R["nslices"] // 2) / 32) < 1024 else "out"),
    "waves_past1024": (("in", "out"), lambda c, R: "in" if R[2048]["nwaves"] <= 1024 else "out"),     # where the two caps part
    "waves_cap2048": (("in", "out"), lambda c, R: "in" if 32 * math.ceil((R["nslices"] // 2) / 32) < 2048 else "out"),
    "tier4096": (("in", "out"), lambda c, R: "in" if R["max_slice_vals"] <= TIER_SMALL else "out"),
    "tier16384": (("in", "out"), lambda c, R: "in" if R["max_slice_vals"] <= TIER_LARGE else "out"),
}
for _w, _p in PARK.items():  # the most slices one wave owns, against the park: park - 1, park, park + 1, 2 park, 2 park + 1
    LIMITS[f"park_{_w}"] = (tuple(str(k) for k in (_p - 1, _p, _p + 1, 2 * _p, 2 * _p + 1)), _max_spw(_w))
for _D, _cap in ((4, 2048), (6, 1024), (8, 1024), (12, 1024)):  # a wave range of fewer than D, of D and of D + 1 steps
    LIMITS[f"range_D{_D}"] = (("lt", "eq", "gt"), _range_side(_D, _cap))

FEATURES = ("no_blocks", "onestep", "empty_slice_first", "empty_slice_last", "empty_slice_mid_range", "empty_slice_whole_range",
            "empty_waves_front", "empty_waves_middle", "empty_waves_back", "stride_4096", "stride_16384", "stride_unstaged", "tail_full",
            "neg_zero", "square", "rows_0", "rows_1", "rows_15", "rows_16", "rows_17", "rows_1023", "rows_1025")
FEATURE_CHECK = {f: _feature(f) for f in FEATURES}


def claim_holds(tag, case, R):
    if ":" not in tag:
        return bool(FEATURE_CHECK[tag](case, R))
    lim, side = tag.split(":")
    got = LIMITS[lim][1](case, R)
    if isinstance(got, dict):
        return bool(got.get(side))
    return side in got if isinstance(got, set) else got == side


# ---- cases -----------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, lens, nbcols=None, tags=(), waves=None, special=None, seed=0):
        lens = np.asarray(lens, np.int64)
        self.name, self.tags, self.waves, self.special = name, tuple(tags), waves, special
        self.nbrows = len(lens)
        need = int(lens.max()) + 1 if len(lens) and lens.max() > 0 else 1
        self.nbcols = max(need, 2) if nbcols is None else nbcols
        assert self.nbcols >= need, (name, self.nbcols, need)
        self.ptrow = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        nb = int(self.ptrow[-1])
        assert nb <= MAX_BLOCKS, (name, nb)
        # block columns: distinct within a row, never block column 0 (x is infinite there: a padding place reads it)
        rng = np.random.default_rng(1000 + seed)
        m = self.nbcols - 1
        a = 1
        if m > 2 and seed % 2:  # a stride coprime to m keeps a row's columns distinct
            a = int(rng.integers(2, m))
            while math.gcd(a, m) != 1:
                a += 1
        rows = np.repeat(np.arange(self.nbrows), lens)
        start = rng.integers(0, max(m, 1), self.nbrows)
        place = np.arange(nb) - self.ptrow[rows]
        self.indcol = (1 + (a * (start[rows] + place)) % max(m, 1)).astype(np.int32)
        self.seed = seed

    @property
    def nblocks(self):
        return int(self.ptrow[-1])

    def __repr__(self):
        return self.name

    def values(self, k=0):
        """16 values per block, row-major; k picks a set (refreshes)."""
        rng = np.random.default_rng(77 + 13 * self.seed + k)
        v = rng.uniform(-1, 1, 16 * self.nblocks)
        if self.special == "neg_zero":  # every third block row: products that underflow to -0.0 (x is 1e-200 everywhere)
            rows = np.repeat(np.arange(self.nbrows), np.diff(self.ptrow))
            v = v.reshape(-1, 16)
            v[rows % 3 == 0] = -1e-200 * (1 + np.arange(16))
            v = v.reshape(-1)
        return v

    def x(self, inf=True):
        """x with every entry finite, or infinite at node 0 and at every block column no block names."""
        rng = np.random.default_rng(5 + self.seed)
        x = rng.uniform(-1, 1, 4 * self.nbcols)
        if self.special == "neg_zero":
            x[:] = 1e-200
            x[:4] = 1.0
        if inf:
            named = np.zeros(self.nbcols, bool)
            named[self.indcol] = True
            x = np.where(np.repeat(named, 4), x, np.inf)
        return x

    def csr(self, v=None):
        """the pattern as a CSR matrix with full 4x4 blocks: (n, ncols, ptrow, indcol[, coef])"""
        lens = np.diff(self.ptrow).astype(np.int64)
        p = np.concatenate([[0], np.cumsum(np.repeat(4 * lens, 4))]).astype(np.int32)
        blk = np.arange(self.nblocks, dtype=np.int64)
        rows = np.repeat(np.arange(self.nbrows), lens)
        # CSR row 4 i + q holds, block after block, the block's row q
        c = np.empty(16 * self.nblocks, np.int32)
        src = np.empty(16 * self.nblocks, np.int64)
        base = p[4 * rows].astype(np.int64) + 4 * (blk - self.ptrow[rows])
        for q in range(4):
            for cc in range(4):
                pos = base + q * 4 * lens[rows] + cc
                c[pos] = 4 * self.indcol + cc
                src[pos] = 16 * blk + 4 * q + cc
        out = (4 * self.nbrows, 4 * self.nbcols, p, c)
        return out if v is None else out + (np.asarray(v)[src],)


def _rows_of_slices(slice_lens, rng, nbrows=None, fill=2):
    """Row lengths: slice s has one row (a varying one) of slice_lens[s] blocks, the others at most `fill` (and never more than it);
    slice_lens[s] == 0: an all-empty slice."""
    ns = len(slice_lens)
    lens = np.zeros(ns * ROWS, np.int64)
    sl = np.asarray(slice_lens, np.int64)
    other = rng.integers(0, fill + 1, ns * ROWS)
    lens[:] = np.minimum(other, np.repeat(sl, ROWS))
    lens[np.arange(ns) * ROWS + (7 * np.arange(ns)) % ROWS] = sl
    if nbrows is not None:
        cut = ns * ROWS - nbrows
        assert 0 <= cut < ROWS
        if cut:
            keep = lens[:nbrows].copy()
            s_last = (ns - 1) * ROWS
            keep[s_last] = max(keep[s_last], sl[-1])  # the long row of the last slice stays inside
            lens = keep
    return lens


def _ragged(nbrows, maxlen, seed, empty=0.2):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, maxlen + 1, nbrows)
    lens[rng.random(nbrows) < empty] = 0
    return lens


def one_heavy(ns, K, cap, light_empty_every=0, seed=0):
    """One slice of L steps in front of ns - 1 slices of one step, L such that the steps are K per wave: the last wave then owns
    exactly K slices, the waves under the heavy slice's steps none."""
    W = wave_count(ns, cap)
    M = ns - 1
    L = W * K - M
    assert L >= 1 and M >= K, (ns, K, W, L)
    sl = np.ones(ns, np.int64)
    sl[0] = L
    if light_empty_every:
        sl[2::light_empty_every] = 0
        sl[1] = sl[-1] = 1
    return _rows_of_slices(sl, np.random.default_rng(seed), fill=1)


def _tier_case(name, ns, blocks_in_big, where, tags, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 3, ns * ROWS)
    # the big slice: blocks_in_big blocks spread unevenly over its 16 rows
    cuts = np.sort(rng.integers(0, blocks_in_big + 1, ROWS - 1))
    lens[where * ROWS: (where + 1) * ROWS] = np.diff(np.concatenate([[0], cuts, [blocks_in_big]]))
    return Case(name, lens, tags=tags, seed=seed)


@functools.lru_cache(maxsize=None)
def table():
    T = []
    rng = np.random.default_rng(2)
    # --- the row count against the slice of 16
    for nbr, tags in ((0, ("rows_0", "slice_rows:eq")), (1, ("rows_1", "slice_rows:gt", "empty_waves_front")), (15, ("rows_15", "slice_rows:lt")),
                      (16, ("rows_16", "slice_rows:eq")), (17, ("rows_17", "slice_rows:gt")), (1023, ("rows_1023", "slice_rows:lt")),
                      (1025, ("rows_1025", "slice_rows:gt"))):
        lens = _ragged(nbr, 6, 10 + nbr)
        if nbr:
            lens[0] = 3
        T.append(Case(f"rows_{nbr}", lens, nbcols=max(nbr, 8), tags=tags + (("square",) if nbr >= 8 else ()), seed=nbr))
    # --- the wave-count rule, both caps: (waves at cap 1024, waves at cap 2048) written out by hand
    for ns, w, tags in ((65, (32, 32), ("waves_floor:in",)), (66, (64, 64), ("waves_floor:out",)),
                        (1985, (992, 992), ("waves_cap1024:in",)), (1986, (1024, 1024), ("waves_cap1024:out",)),
                        (2049, (1024, 1024), ("waves_past1024:in",)), (2050, (1024, 1056), ("waves_past1024:out",)),
                        (4033, (1024, 2016), ("waves_cap2048:in",)), (4034, (1024, 2048), ("waves_cap2048:out",)),
                        (4097, (1024, 2048), ()), (4098, (1024, 2048), ())):
        lens = _rows_of_slices(np.ones(ns, np.int64), rng, nbrows=ns * ROWS - 5, fill=1)
        T.append(Case(f"slices_{ns}", lens, nbcols=64, tags=tags + ("onestep",), waves=w, seed=ns))
    # --- parks: the most slices of one wave; the single-vector parks at both caps (the same ranges below 2050 slices) and the multi-vector parks
    for K, ns, tags in ((7, 9, ("park_mm8:7",)), (8, 10, ("park_mm8:8",)), (9, 11, ("park_mm8:9", "empty_slice_mid_range")),
                        (15, 17, ("park_mm4:15",)), (16, 18, ("park_mm4:16", "park_mm8:16")), (17, 19, ("park_mm4:17", "park_mm8:17")),
                        (31, 33, ("park_w1:31", "park_w2:31")), (32, 34, ("park_w1:32", "park_w2:32", "park_mm4:32")),
                        (33, 35, ("park_w1:33", "park_w2:33", "park_mm4:33", "empty_slice_mid_range")),
                        (64, 65, ("park_w1:64", "park_w2:64")), (65, 100, ("park_w1:65", "park_w2:65"))):
        lens = one_heavy(ns, K, 1024, light_empty_every=4 if "empty_slice_mid_range" in tags else 0, seed=K)
        T.append(Case(f"park_{K}", lens, tags=tags + ("empty_waves_middle",), seed=K))
    for K in (31, 32, 33, 64, 65):  # 2051 slices: 1056 waves at cap 2048, 1024 at cap 1024 — variant 2 walks ranges of its own
        T.append(Case(f"park2_{K}", one_heavy(2051, K, 2048, seed=K), tags=(f"park_w2:{K}", "empty_waves_middle", "waves_past1024:out"), seed=100 + K))
    # a square park-filling case (powers, relabelling): 192 slices in 96 waves, the heavy row nearly as long as the matrix is wide
    T.append(Case("park_square", one_heavy(192, 33, 1024, seed=41), nbcols=192 * ROWS, tags=("square", "park_w1:33", "empty_waves_middle"), seed=41))
    # 40 long slices in front of 12 000 of one step: 129 slices per wave at cap 1024, 65 at cap 2048; the long slices are unstaged
    lens = np.ones(12040 * ROWS, np.int64)
    lens[np.arange(40) * ROWS + 3] = 3000
    T.append(Case("park_big", lens, tags=("tier16384:out", "stride_unstaged", "waves_cap2048:out"), seed=9))
    # --- wave ranges against the steps of one trip: 32 slices of L steps, one per wave
    side = {3: ("range_D4:lt",), 4: ("range_D4:eq",), 5: ("range_D4:gt", "range_D6:lt"), 6: ("range_D6:eq",), 7: ("range_D6:gt", "range_D8:lt"),
            8: ("range_D8:eq",), 9: ("range_D8:gt",), 11: ("range_D12:lt",), 12: ("range_D12:eq",), 13: ("range_D12:gt",)}
    for L, tags in side.items():
        T.append(Case(f"range_32x{L}", _rows_of_slices(np.full(32, L), rng, fill=L), tags=tags, seed=L))
    # ... and slices of ONE step, as many per wave as a trip has steps: every step of the trip is a slice boundary
    ones = {5120: ("range_D6:lt", "range_D4:lt"), 6144: ("range_D6:eq",), 7168: ("range_D6:gt", "range_D8:lt"), 8192: ("range_D8:eq", "range_D4:eq"),
            9216: ("range_D8:gt", "range_D4:gt"), 12288: ("range_D12:eq",), 13312: ("range_D12:gt",)}
    for ns, tags in ones.items():
        T.append(Case(f"ones_{ns}", _rows_of_slices(np.ones(ns, np.int64), rng, fill=1), nbcols=512, tags=tags + ("onestep",), seed=ns))
    # --- empty slices and empty waves
    sl = np.ones(64, np.int64)
    sl[[0, 1, 10, 11, 62, 63]] = 0  # 32 waves of two slices: waves 0, 5 and 31 own empty slices only
    T.append(Case("empty_slices", _rows_of_slices(sl, rng, fill=1), nbcols=32,
                  tags=("empty_slice_first", "empty_slice_last", "empty_slice_whole_range"), seed=3))
    T.append(Case("no_blocks", np.zeros(100, np.int64), nbcols=8, tags=("no_blocks", "empty_waves_front"), seed=4))
    sl = np.concatenate([np.ones(39, np.int64), [2000]])  # the heavy slice LAST: wave 0 owns all 40 slices, the other 31 none
    T.append(Case("heavy_last", _rows_of_slices(sl, rng, fill=1), tags=("empty_waves_back",), seed=5))
    # --- refresh tiers: the longest slice's values on both sides of 4096 and of 16384, more slices than the tier's grid,
    #     the longest slice behind the grid's first turn
    T.append(_tier_case("tier_4096", 2100, 256, 2090, ("tier4096:in", "stride_4096"), 6))
    T.append(_tier_case("tier_4112", 300, 257, 290, ("tier4096:out", "tier16384:in", "stride_16384"), 7))
    T.append(_tier_case("tier_16384", 300, 1024, 270, ("tier16384:in", "stride_16384"), 8))
    T.append(_tier_case("tier_16400", 2100, 1025, 2070, ("tier16384:out", "stride_unstaged"), 9))
    # --- the stream's last step holds a block of the last quad
    lens = _ragged(80, 5, 12)
    lens[79] = 9
    T.append(Case("tail_full", lens, tags=("tail_full", "slice_rows:eq"), seed=12))
    # --- rows that sum to -0.0 with padding steps behind them
    lens = _ragged(90, 3, 13, empty=0.0)
    lens[5::16] = 7
    T.append(Case("neg_zero", lens, tags=("neg_zero",), special="neg_zero", seed=13))
    names = [c.name for c in T]
    assert len(set(names)) == len(names)
    return tuple(T)


@functools.lru_cache(maxsize=None)
def seeded_cases(count=100):
    """Ragged patterns: slices of one step, empty slices, short slices and a few long ones in any order; any row count."""
    out = []
    for q in range(count):
        rng = np.random.default_rng(9000 + q)
        kind = q % 5
        ns = int(rng.integers(1, 40)) if kind == 0 else int(rng.integers(40, 140)) if kind in (1, 2) else int(rng.integers(140, 700))
        sl = rng.choice([0, 1, 1, 1, 2, 3, 5, 9, 14], size=ns)
        if kind in (2, 4):  # a few long slices: waves of many short slices and empty waves beside them
            for s in rng.integers(0, ns, int(rng.integers(1, 4))):
                sl[s] = int(rng.integers(100, 2500))
        if kind == 3:
            sl[rng.integers(0, ns)] = int(rng.choice([256, 257, 300, 1024, 1100]))
        nbrows = ns * ROWS - int(rng.integers(0, ROWS))
        lens = _rows_of_slices(sl, rng, nbrows=nbrows, fill=int(rng.integers(0, 4)))
        square = kind == 1 and lens.max() < nbrows
        out.append(Case(f"seed_{q}", lens, nbcols=nbrows if square else None, seed=q))
    return tuple(out)
