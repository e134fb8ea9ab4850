"""Cases at the limits of the sliced-stream plans (tests/test_sstream_limits.py; TEST INFRASTRUCTURE, not a conftest).

Three parts:
  restate_plan   a plain restatement of build_sstream_plan (spmv_sstream.hpp) for shift 0 and 1 without ghost columns, written from
                 its rules and independent of the library: eligibility and the first refusal reason, the dealing of the rounds
                 (ss_deal_plain), every round's window (a workgroup's first fill, then the new columns per round), the per-slice step
                 counts, the padding and the longest slice.
  TABLE          deterministic cases, each on one side of one limit of the plain form or of the cut-ring form
                 (spmv_sstream_mw.hpp), with the outcome it must have: "plain", "cut-ring" or "refused" (+ the reason).  The cut-ring
                 planner is not restated: its outcomes are pinned here from reading build_sstream_mw_plan.
  seeded_cases   about 200 seeded cases near the same limits; their outcome comes from restate_plan (and, for the cut-ring form,
                 from the library's probe).

A case's tags name the limits it sits on: "<limit>:in" or "<limit>:out" for a limit with two sides (LIMITS lists them), a bare
name for a feature that only has to occur (FEATURES)."""
import functools

import numpy as np

from navierstokes_amd import synth

# ---- constants of spmv_sstream.hpp / spmv_sstream_mw.hpp ---------------------------------------------------------------------
RING, SLICE, ROUND, NEWMAX, PARK, TAIL, PADSTEPS, MAXWGS, FILL = 8192, 128, 512, 1024, 20, 2, 64, 256, 24
MW_CAP, MW_GAP, MW_NEW, MW_FILL, MW_TABMAX = 2048, 512, 512, 16, 480
DEFAULT_MAX_PADDING = 0.12  # kSsMaxPadding (capi_csr.hip)

R_EMPTY = "empty matrix"
R_NEW = "a round brings more new columns than the window takes in at once"
R_REACH = "a round's rows reach further apart than the LDS ring holds"
R_STEPS = "too many steps for 32-bit offsets"
R_PAD = "row lengths vary too much inside the 128-row slices (padding)"
R_BADSHIFT = "bad shift"
PLAIN_REASONS = (R_EMPTY, R_BADSHIFT, R_NEW, R_REACH, R_STEPS, R_PAD)

M_TWO = "fewer than two columns"
M_FOUR = "a round's rows name more than four column neighbourhoods"
M_WIDE = "a column neighbourhood is wider than a sub-ring"
M_TAB = "too many rounds per workgroup for the staged intake table"
M_BACK = "a column neighbourhood moves backwards"
M_NOFREE = "no free sub-ring for a new column neighbourhood"
M_BUSY = "a wide new column neighbourhood finds its sub-ring busy in the rounds before"
M_WIDE_AHEAD = "a column neighbourhood is wider than a sub-ring (with what it takes in ahead)"
M_FAST = "a column neighbourhood moves on faster than its sub-ring has room for"
M_INTAKE = "a round brings a sub-ring more new columns than the window wave takes in at once"
M_NEW_WIDE = "a new column neighbourhood is wider than the window wave takes in at once"
MW_REASONS = (R_EMPTY, M_TWO, R_BADSHIFT, M_FOUR, M_WIDE, M_TAB, M_BACK, M_NOFREE, M_BUSY, M_WIDE_AHEAD, M_FAST, M_INTAKE, M_NEW_WIDE,
              R_STEPS, R_PAD)

# Refusal reasons no case reaches, and why.
NOT_REACHED = {
    R_STEPS: "needs more than 33.5 M steps of 64 lanes: well over 60 M rows",
    M_TAB: "needs more than 480 rounds in one of 256 workgroups: more than 62.9 M rows",
    R_BADSHIFT: "both probes and mi_csr_create pass only shift 0 or 1 (the probes refuse any other as a bad argument)",
    M_INTAKE: "unreachable: the backward pass gives every continued sub-ring need[r - 1] >= need[r] - 512, so an intake is never wider",
}


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def _deal(nwg, rounds):
    """ss_deal_plain: rounds // nwg each; inside each XCD's chunk of nwg / 8 workgroups the first ones take the remainder."""
    cnt = np.full(nwg, rounds // nwg, np.int64)
    extra = rounds % nwg
    per = nwg // 8 if nwg % 8 == 0 else nwg
    chunks = nwg // per
    for xcd in range(chunks):
        e = extra * (xcd + 1) // chunks - extra * xcd // chunks
        cnt[xcd * per: xcd * per + e] += 1
    return np.concatenate([[0], np.cumsum(cnt)])


def _view(n, ptrow, shift, rows):
    """first nonzero of view rows `rows` (view row v is the matrix's row v - shift, clamped to [0, n])."""
    return ptrow[np.clip(np.asarray(rows, np.int64) - shift, 0, n)]


def restate_plan(n, ncols, ptrow, indcol, shift=0, max_padding=DEFAULT_MAX_PADDING):
    """build_sstream_plan without ghost columns.  Returns a dict: eligible, why, rounds, nwg, rptr (rounds of workgroup g:
    rptr[g] .. rptr[g + 1] - 1), share, win (per round (first column, count)), w0 (per workgroup its first window's width),
    newcols (per round; -1 for a workgroup's first round), whi (per round the window's upper end), cmin (per round its lowest column;
    0x7fffffff: no nonzero), slice_len (per slice 4 r + wave), steps, pad_places, max_slice_nnz,
    padding (pad_places / nnz, as the probe reports it)."""
    ptrow = np.asarray(ptrow, np.int64)
    indcol = np.asarray(indcol, np.int64)
    nnz = int(ptrow[n]) if n > 0 else 0
    P = dict(eligible=False, why="", rounds=0, nwg=0, rptr=None, share=None, win=None, w0=None, newcols=None, slice_len=None, steps=0,
             pad_places=0, max_slice_nnz=0, padding=0.0)
    if n <= 0 or nnz <= 0:
        P["why"] = R_EMPTY
        return P
    if shift not in (0, 1):
        P["why"] = R_BADSHIFT
        return P
    nv = n + shift
    rounds = (nv + ROUND - 1) // ROUND
    nwg = min(MAXWGS, rounds)
    if nwg >= 8:
        nwg = nwg // 8 * 8
    P.update(rounds=rounds, nwg=nwg)
    # column extent of every round
    rb = _view(n, ptrow, shift, np.arange(rounds) * ROUND)
    re = _view(n, ptrow, shift, np.minimum(nv, (np.arange(rounds) + 1) * ROUND))
    BIG = 0x7FFFFFFF
    cmin = np.full(rounds, BIG, np.int64)
    cmax = np.full(rounds, -1, np.int64)
    full = re > rb
    if full.any():
        cmin[full] = np.minimum.reduceat(indcol[:nnz], rb[full])
        cmax[full] = np.maximum.reduceat(indcol[:nnz], rb[full])
    rptr = _deal(nwg, rounds)
    P["rptr"], P["share"] = rptr, np.diff(rptr)
    # windows: per workgroup a monotone upper end; everything a round names lies within RING below it
    win = np.zeros((rounds, 2), np.int64)
    whis = np.zeros(rounds, np.int64)
    newcols = np.full(rounds, -1, np.int64)
    w0 = np.zeros(nwg, np.int64)
    cmin_l, cmax_l = cmin.tolist(), cmax.tolist()
    for g in range(nwg):
        r0, r1 = int(rptr[g]), int(rptr[g + 1])
        allmin = min(cmin_l[r0:r1])
        whi = 0
        for r in range(r0, r1):
            nhi = max(whi, cmax_l[r] + 1)
            if r == r0:
                lo = max(max(0, nhi - RING), min(allmin, nhi))
                win[r] = (lo, nhi - lo)
                w0[g] = nhi - lo
            else:
                win[r] = (whi, nhi - whi)
                newcols[r] = nhi - whi
                if nhi - whi > NEWMAX:
                    P["why"] = R_NEW
                    return P
            whi = whis[r] = nhi
            if cmin_l[r] != BIG and cmin_l[r] < whi - RING:
                P["why"] = R_REACH
                return P
    P.update(win=win, newcols=newcols, w0=w0, whi=whis, cmin=cmin)
    # slices: 128 view rows each, padded to the longest (at least one step)
    nsl = 4 * rounds
    pt = _view(n, ptrow, shift, np.arange(nsl * SLICE + 1))
    lens = np.diff(pt).reshape(nsl, SLICE)
    L = np.maximum(1, lens.max(axis=1))
    row0 = np.arange(nsl) * SLICE
    live = row0 < nv
    seg = _view(n, ptrow, shift, np.minimum(nv, row0 + SLICE)) - _view(n, ptrow, shift, row0)
    steps = int(L.sum())
    pad_places = steps * SLICE - nnz
    P.update(slice_len=L, steps=steps, pad_places=pad_places, max_slice_nnz=int(seg[live].max()), padding=pad_places / nnz)
    if steps + PADSTEPS >= 0x7FFFFFFF // 64:
        P["why"] = R_STEPS
        return P
    if float(pad_places) > max_padding * float(nnz):
        P["why"] = R_PAD
        return P
    P["eligible"] = True
    return P


def fill_instantiation(max_slice_nnz):
    """(LDS capacity of sstream_fill_kernel, its grid) the fill takes for a plan's longest slice (sstream_fill_values)."""
    if max_slice_nnz <= 2048:
        return 2048, 2048
    if max_slice_nnz <= 8192:
        return 8192, 1024
    return 0, 2048


def max_slice_nnz(n, ptrow, shift=0):
    """the longest slice's CSR segment, as sstream_fill_values sees it (view rows of 128)."""
    ptrow = np.asarray(ptrow, np.int64)
    nv = n + shift
    row0 = np.arange(0, nv, SLICE)
    return int((_view(n, ptrow, shift, np.minimum(nv, row0 + SLICE)) - _view(n, ptrow, shift, row0)).max())


# ---- pattern builders ----------------------------------------------------------------------------------------------------------
def band(n, ncols=None, k=3, slope=1.0, lens=None, base=0):
    """row i: lens[i] (default k) columns centred on base + floor(slope * i), one apart, clipped to [0, ncols)."""
    ncols = n if ncols is None else ncols
    lens = np.full(n, k, np.int64) if lens is None else np.asarray(lens, np.int64)
    p = np.concatenate([[0], np.cumsum(lens)])
    row = np.repeat(np.arange(n, dtype=np.int64), lens)
    j = np.arange(p[-1], dtype=np.int64) - p[row]
    centre = base + np.floor(slope * np.arange(n)).astype(np.int64)
    c = np.clip(centre[row] + j - lens[row] // 2, 0, ncols - 1)
    return p.astype(np.int32), c.astype(np.int32)


def multiband(n, ncols, offsets, k=3, slope=1.0):
    """rows naming len(offsets) neighbourhoods: k columns around floor(slope * i) + off for each offset (ascending), clipped."""
    m = len(offsets) * k
    row = np.repeat(np.arange(n, dtype=np.int64), m)
    j = np.tile(np.arange(m, dtype=np.int64), n)
    off = np.asarray(offsets, np.int64)[j // k] + j % k - k // 2
    c = np.clip(np.floor(slope * row).astype(np.int64) + off, 0, ncols - 1)
    return (np.arange(n + 1, dtype=np.int64) * m).astype(np.int32), c.astype(np.int32)


def from_rows(rows):
    lens = np.array([len(r) for r in rows], np.int64)
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    c = np.concatenate([np.asarray(r, np.int64) for r in rows]).astype(np.int32) if p[-1] else np.zeros(0, np.int32)
    return p, c


def empty_rows(p, c, rows):
    """the same pattern with the given rows emptied."""
    n = len(p) - 1
    lens = np.diff(p.astype(np.int64))
    keep = np.ones(len(c), bool)
    for i in np.asarray(rows).reshape(-1):
        keep[p[i]:p[i + 1]] = False
    lens[np.asarray(rows).reshape(-1)] = 0
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), c[keep].copy(), n


def poke(p, c, row, j, col):
    """set the j-th nonzero of `row` (negative j: from the row's end) to column `col`."""
    c = c.copy()
    k = p[row] + j if j >= 0 else p[row + 1] + j
    assert p[row] <= k < p[row + 1]
    c[k] = col
    return c


def values(seed, nnz):
    return np.random.default_rng(seed).uniform(-1, 1, nnz) * np.where(np.arange(nnz) % 5 == 0, 3.0, 1.0)


# ---- the limit table -------------------------------------------------------------------------------------------------------------
class Case:
    """One pattern.  build() -> (n, ncols, ptrow, indcol) (deterministic, cached); expect: "plain" | "cut-ring" | "refused";
    why: the plain planner's reason when it refuses; mw: the cut-ring planner's pinned outcome when the plain one refuses —
    "cut-ring" or the reason it refuses with; max_padding: the padding budget the case runs with (None: the default 0.12)."""

    def __init__(self, name, tags, build, expect, why=None, mw=None, max_padding=None, note=""):
        self.name, self.tags, self._build, self.expect, self.why, self.mw = name, tuple(tags), build, expect, why, mw
        self.max_padding, self.note = max_padding, note

    @functools.cached_property
    def data(self):
        n, ncols, p, c = self._build()
        return int(n), int(ncols), np.ascontiguousarray(p, np.int32), np.ascontiguousarray(c, np.int32)

    @property
    def padding_budget(self):
        return DEFAULT_MAX_PADDING if self.max_padding is None else self.max_padding

    def __repr__(self):
        return f"Case({self.name})"


def _sq(p, c):
    n = len(p) - 1
    return n, n, p, c


def _rect(p, c, ncols):
    return len(p) - 1, ncols, p, c


def _n_for_rounds(R, rem=300):
    return 512 * (R - 1) + (rem if R > 1 else 512)


def _first_window(W):
    """one round (512 rows, slope-1 band of 3) whose last row also names column W - 1: the first window is W columns wide."""
    p, c = band(512, W + 1)
    return _rect(p, poke(p, c, 511, -1, W - 1), W + 1)


def _two_round_band(k=3, slope=1.0, ncols=None):
    """512 rounds of a slope band: 256 workgroups of two rounds each (round 2 g, 2 g + 1)."""
    n = 512 * 512
    return band(n, ncols if ncols is not None else int(np.ceil(slope * n)) + 8, k=k, slope=slope)


G = 100  # the workgroup whose second round (2 G + 1) the two-round cases edit
RG = 2 * G + 1


def _span_case(extra):
    """workgroup G's second round names a column `8192 + extra` below its window's upper end (extra = 0: exactly the ring)."""
    p, c = _two_round_band()
    whi = 512 * RG + 511 + 1 + 1  # the round's last row names column i + 1
    return _rect(p, poke(p, c, 512 * RG, 0, whi - RING - extra), len(p) - 1 + 8)


def _newcols_case(extra):
    p, c = _two_round_band(slope=2.0)
    last = 512 * RG + 511
    return _rect(p, poke(p, c, last, -1, 2 * last + 1 + extra), 2 * (len(p) - 1) + 8)


def _padding_case(m):
    """64 slices of rows of 8 nonzeros; m of them have one row of 9: padding 127 m / (8192 * 8 + m)."""
    n = 8192
    lens = np.full(n, 8)
    lens[np.arange(m) * SLICE] = 9
    return _sq(*band(n, lens=lens))


def _long_slice(n, k_long, slice_idx=4, k=3):
    lens = np.full(n, k)
    lens[slice_idx * SLICE:(slice_idx + 1) * SLICE] = k_long
    return _sq(*band(n, lens=lens))


def _share(R, rows_per=2):
    """a largest share of R rounds per workgroup: 256 R - 3 rounds (253 workgroups take R, three take R - 1)."""
    return _sq(*band(512 * (256 * R - 3), k=rows_per))


def _unsorted_repeated():
    n = 20_000
    p, c = band(n, k=5)
    c = c.reshape(n, 5)[:, [4, 1, 3, 1, 0]].reshape(-1)  # descending-ish, column i - 1 twice
    return _sq(p, c.astype(np.int32))


def _empty_round(r, n=512 * 512):
    p, c = band(n)
    p, c, _ = empty_rows(p, c, np.arange(512 * r, 512 * r + 512))
    return _sq(p, c)


def _empty_slices():
    n = 40_000
    p, c = band(n, k=6)
    rows = np.concatenate([np.arange(128, 256), np.arange(5000, 5512), np.arange(9001, 9002)])
    return _sq(*empty_rows(p, c, rows)[:2])


def _wg_empty():
    n = 16 * 512  # 16 rounds, 16 workgroups of one round: workgroup 5 has only empty rows
    p, c = band(n)
    return _sq(*empty_rows(p, c, np.arange(5 * 512, 6 * 512))[:2])


def _reach_back_first_fill():
    """workgroup G's SECOND round names a column 7000 below its first round's: the first fill starts there (7000+ columns)."""
    p, c = _two_round_band()
    return _rect(p, poke(p, c, 512 * RG + 3, 1, 512 * (RG - 1) - 7000), len(p) - 1 + 8)


def _reach_back_inside():
    """rows of every round reach 6000 columns back (inside the ring) and forward: unsorted, the band keeps moving."""
    n = 200_000
    p, c = band(n, k=4)
    c = c.copy()
    i = np.arange(n)
    back = np.maximum(0, i - 6000)
    c[p[:-1] + 1] = back  # the row's second nonzero reaches back
    return _sq(p, c)


# the cut-ring builders (rows naming several column neighbourhoods, as a 3-D mesh operator in natural order does)
def _mw_bands(nb, gap, n=60_000, k=3, slope=1.0):
    offs = [j * gap for j in range(nb)]
    ncols = int(slope * n) + offs[-1] + k + 2
    return _rect(*multiband(n, ncols, offs, k=k, slope=slope), ncols)


def _with_extras(p, c, extra):
    """the pattern with the columns extra[i] appended to row i."""
    n = len(p) - 1
    lens = np.diff(p.astype(np.int64))
    lens2 = lens.copy()
    for i, e in extra.items():
        lens2[i] += len(e)
    p2 = np.concatenate([[0], np.cumsum(lens2)])
    row = np.repeat(np.arange(n), lens)
    c2 = np.empty(p2[-1], np.int64)
    c2[p2[row] + (np.arange(len(c)) - p.astype(np.int64)[row])] = c
    for i, e in extra.items():
        c2[p2[i] + lens[i]: p2[i + 1]] = e
    return p2.astype(np.int32), c2.astype(np.int32)


def _bridge(lo, hi, rows):
    """columns lo .. hi - 1 reached with gaps of at most 400 (one neighbourhood), spread over `rows`, one each."""
    cols = list(range(lo, hi - 1, 400)) + [hi - 1]
    assert len(cols) <= len(rows)
    return {int(r): [cc] for r, cc in zip(rows, cols)}


def _mw_gap(g):
    """rows name four bands 10 000 apart; round 10's first row also names a column g above the round's highest (the fourth band's
    last row's): g = 512 keeps four neighbourhoods, 513 makes five."""
    n = 60_000
    p, c = multiband(n, n + 40_000, [0, 10_000, 20_000, 30_000], k=2)
    r0 = 512 * 10
    top = int(c[p[r0 + 511]: p[r0 + 512]].max())
    p, c = _with_extras(p, c, {r0: [top + g]})
    return _rect(p, c, n + 40_000)


def _mw_width(w):
    """two bands 30 000 apart (2 columns per row); round 10's first neighbourhood is widened to exactly w columns (its low end is row
    5120's i - 1; extra columns every 400 up to the low end + w - 1)."""
    n = 60_000
    p, c = multiband(n, n + 40_000, [0, 30_000], k=2)
    r0 = 512 * 10
    lo = r0 - 1
    p, c = _with_extras(p, c, _bridge(lo + 400, lo + w, range(r0, r0 + 512, 2)))
    return _rect(p, c, n + 40_000)


def _mw_backwards(below=100):
    """two rounds per workgroup; workgroup G's second round also names columns `below` under its first round's low end, bridged to
    its band (the neighbourhood continues in its sub-ring, and moves backwards)."""
    n = 512 * 512
    p, c = multiband(n, n + 30_000, [0, 20_000], k=2)
    lo_prev = 512 * (RG - 1) - 1
    rows = range(512 * RG, 512 * RG + 512, 3)
    p, c = _with_extras(p, c, _bridge(lo_prev - below, 512 * RG, rows))
    return _rect(p, c, n + 30_000)


def _late_layout():
    """four rounds per workgroup (1024 rounds); rows name a band (2 columns) and a second band 20 000 away."""
    n = 1024 * 512
    ncols = n + 60_000
    p, c = multiband(n, ncols, [0, 20_000], k=2)
    return n, ncols, p, c


def _mw_late(width, busy=False, nofree=False):
    """in workgroup G's round 4 G + 2 a NEW neighbourhood `width` columns wide appears 40 000 columns above the band.  busy: round
    4 G also names a neighbourhood up there (the sub-ring the new one finds free in rounds 4 G + 1 and 4 G + 2 was busy in 4 G).
    nofree: round 4 G + 1 names two further neighbourhoods (four in all), round 4 G + 2 keeps one of them, drops the other and adds
    the new one."""
    n, ncols, p, c = _late_layout()
    r2 = 4 * G + 2
    a = 40_000 + 512 * r2
    extra = _bridge(a, a + width, range(512 * r2, 512 * r2 + 512, 2))
    if busy:
        for i in range(512 * (4 * G), 512 * (4 * G) + 512, 64):
            extra[i] = [a - 20_000 + 15_000]
    if nofree:
        e1, e2 = a + 5_000, a + 9_000
        for i in range(512 * (r2 - 1) + 1, 512 * r2, 64):
            extra[i] = [e1, e2]
        for i in range(512 * r2 + 1, 512 * r2 + 512, 64):
            extra[i] = extra.get(i, []) + [e1]
    return _rect(*_with_extras(p, c, extra), ncols)


def _mw_grow(x_off, w0, lo1, hi1):
    """four rounds per workgroup; rows name a band and a second one 20 000 away, and, in workgroup G's round x = 4 G + x_off, a
    third neighbourhood [a, a + w0) that continues as [a + lo1, a + hi1) in round x + 1 (a = 40 000 + 512 x)."""
    n, ncols, p, c = _late_layout()
    x = 4 * G + x_off
    a = 40_000 + 512 * x
    extra = _bridge(a, a + w0, range(512 * x, 512 * x + 512, 2))
    extra.update(_bridge(a + lo1, a + hi1, range(512 * (x + 1), 512 * (x + 1) + 512, 2)))
    return _rect(*_with_extras(p, c, extra), ncols)


def _mw_speed(step, width=10, rounds_per=2):
    """a narrow cluster (columns ctr, ctr + width - 1) moving `step` columns per round (ctr = step * i // 512), plus a band 20 000
    above the cluster's end that moves 512 per round."""
    n = 512 * 256 * rounds_per
    top = step * n // 512 + width
    ncols = top + n + 20_000 + 2
    i = np.arange(n, dtype=np.int64)
    ctr = (step * i) // 512
    cols = np.stack([ctr, ctr + width - 1, i + top + 20_000], axis=1)
    return _rect((np.arange(n + 1) * 3).astype(np.int32), cols.reshape(-1).astype(np.int32), ncols)


def _mw_wide_fill(each):
    """three neighbourhoods of `each` columns, 30 000 apart, in every round (rows j of a round name j * each // 512 + band): a first
    fill of 3 * each columns; four rounds, four workgroups of one round."""
    n = 512 * 4
    j = np.arange(n) % 512
    base = (j * (each - 1)) // 511
    cols = np.stack([base, base + 30_000, base + 60_000], axis=1)
    return _rect((np.arange(n + 1) * 3).astype(np.int32), cols.reshape(-1).astype(np.int32), 60_000 + each + 1)


def _pressure(cells):
    p, c, _ = synth.pressure_matrix(cells)
    return _sq(p, c)


def _table():
    T = []
    add = T.append
    lift = 1e9  # padding budget lifted: a few hundred rows pad more than 12 % whatever their lengths
    # row counts (slice of 128 rows, round of 512, 8 rounds = one workgroup per XCD)
    for n in (1, 2, 127, 128, 129, 511, 512, 513, 4095, 4097):
        side128 = "in" if n <= 128 else "out"
        side512 = "in" if n <= 512 else "out"
        tags = [f"n_vs_slice:{side128}", f"n_vs_round:{side512}"]
        if n > 512:
            tags.append(f"n_vs_8_rounds:{'in' if n <= 4096 else 'out'}")
        add(Case(f"rows_{n}", tags, functools.partial(lambda n: _sq(*band(n)), n), "plain", max_padding=lift))
    add(Case("rows_1_default_budget", ["padding:out"], lambda: _sq(*band(1)), "refused", R_PAD, mw=M_TWO))
    add(Case("rows_1_ncols_1", ["ncols_1"], lambda: _rect(*band(1, 1, k=1), 1), "plain", max_padding=lift))
    add(Case("empty_matrix", ["empty_matrix"], lambda: _sq(np.zeros(1001, np.int32), np.zeros(0, np.int32)), "refused", R_EMPTY, mw=R_EMPTY))
    # rounds: nwg = rounds below 8, then a multiple of 8 (<= 256); rounds past 256 give some workgroups two
    for R in (1, 7, 8, 9, 100, 255, 256, 257, 300, 1000):
        tags = [f"rounds_vs_8:{'in' if R < 8 else 'out'}"]
        if R >= 8:
            tags.append(f"rounds_vs_256:{'in' if R <= 256 else 'out'}")
        add(Case(f"rounds_{R}", tags, functools.partial(lambda R: _sq(*band(_n_for_rounds(R))), R), "plain"))
    # rectangular
    add(Case("ncols_half", ["rectangular"], lambda: _rect(*band(50_001, 25_001, slope=0.5), 25_001), "plain"))
    add(Case("ncols_1", ["ncols_1"], lambda: _rect(*band(3000, 1, k=1), 1), "plain"))
    add(Case("ncols_3n_one_round_each", ["rectangular", "slope_3"], lambda: _rect(*band(3000, 9000, slope=3.0), 9000), "plain"))
    add(Case("ncols_odd", ["rectangular", "ncols_odd"], lambda: _rect(*band(5001, 7777, slope=1.5), 7777), "plain"))
    # the round's span: exactly the ring, one more
    add(Case("span_8192_first_round", ["round_span:in", "first_window_8192:in"], lambda: _first_window(8192), "plain", max_padding=lift))
    add(Case("span_8193_first_round", ["round_span:out", "first_window_8192:out"], lambda: _first_window(8193), "cut-ring", R_REACH, mw="cut-ring", max_padding=lift))
    add(Case("span_8192_second_round", ["round_span:in", "reach_back"], lambda: _span_case(0), "plain"))
    add(Case("span_8193_second_round", ["round_span:out"], lambda: _span_case(1), "cut-ring", R_REACH, mw="cut-ring"))
    # new columns per round
    add(Case("newcols_1024", ["new_columns:in"], lambda: _newcols_case(0), "plain"))
    add(Case("newcols_1025", ["new_columns:out"], lambda: _newcols_case(1), "refused", R_NEW, mw=M_FAST))
    # first-window width: one batch of 24 loads per thread (6144), further batches of 8
    add(Case("first_window_6144", ["first_window_6144:in"], lambda: _first_window(6144), "plain", max_padding=lift))
    add(Case("first_window_6145", ["first_window_6144:out"], lambda: _first_window(6145), "plain", max_padding=lift))
    add(Case("first_window_8192", ["first_window_6144:out", "first_window_8192:in"], lambda: _first_window(8192), "plain", max_padding=lift))
    add(Case("first_window_7000_two_rounds", ["first_window_6144:out", "reach_back"], _reach_back_first_fill, "plain"))
    add(Case("reach_back_inside_ring", ["reach_back", "unsorted"], _reach_back_inside, "plain"))
    # unsorted and repeated columns
    add(Case("unsorted_repeated", ["unsorted", "repeated"], _unsorted_repeated, "plain"))
    # empty rows, slices, rounds, a workgroup
    add(Case("empty_every_10th", ["empty_rows", "padding:in"], lambda: _sq(*empty_rows(*band(30_000), np.arange(0, 30_000, 10))[:2]), "plain"))
    add(Case("empty_every_7th", ["empty_rows", "padding:out"], lambda: _sq(*empty_rows(*band(30_000), np.arange(0, 30_000, 7))[:2]), "refused", R_PAD,
             mw=R_PAD))
    add(Case("empty_slices", ["empty_slice", "empty_round", "empty_rows"], _empty_slices, "plain"))
    add(Case("empty_workgroup", ["empty_workgroup"], _wg_empty, "plain"))
    add(Case("empty_second_round", ["empty_round"], lambda: _empty_round(RG), "plain"))
    # (a workgroup whose FIRST round is empty takes in its second round's whole extent as new columns: the planner refuses it)
    add(Case("empty_first_round", ["empty_round", "new_columns:out", "mw_one_neighbourhood"], lambda: _empty_round(RG - 1), "cut-ring", R_NEW, mw="cut-ring"))
    # padding just under and just over 12 %
    add(Case("padding_under", ["padding:in"], lambda: _padding_case(61), "plain"))
    add(Case("padding_over", ["padding:out"], lambda: _padding_case(62), "refused", R_PAD, mw=R_PAD))
    # the longest slice: three fill instantiations, and each past its grid (grid-stride loop)
    add(Case("slice_2048", ["slice_2048:in"], lambda: _sq(*band(1024, k=16)), "plain"))
    add(Case("slice_2049", ["slice_2048:out"], lambda: _long_slice(1024, 17, 2, k=16), "plain"))
    add(Case("slice_8192", ["slice_8192:in", "slice_2048:out"], lambda: _sq(*band(1024, k=64)), "plain"))
    add(Case("slice_8193", ["slice_8192:out"], lambda: _long_slice(1024, 65, 2, k=64), "plain"))
    add(Case("slice_12800", ["slice_8192:out"], lambda: _sq(*band(1024, k=100)), "plain"))
    add(Case("slices_2112_cap2048", ["slice_2048:in", "fill_grid:out"], lambda: _long_slice(270_000, 16), "plain"))
    add(Case("slices_1096_cap8192", ["slice_8192:in", "fill_grid:out"], lambda: _long_slice(140_000, 64), "plain"))
    add(Case("slices_2112_unstaged", ["slice_8192:out", "fill_grid:out"], lambda: _long_slice(270_000, 100), "plain"))
    add(Case("slices_2048_cap2048", ["fill_grid:in"], lambda: _sq(*band(512 * 512, k=3)), "plain"))
    # rounds per workgroup around the park (20 slices) and the tail (2 rounds)
    for R in (19, 20, 21, 22, 23):
        add(Case(f"share_{R}", [f"park:{'in' if R <= 22 else 'out'}"], functools.partial(_share, R), "plain"))
    # ---- the cut-ring form (the plain plan refuses these: rows name columns further apart than the ring holds)
    mw = functools.partial(Case, expect="cut-ring", why=R_REACH, mw="cut-ring")
    for nb in (2, 3, 4):
        add(mw(f"mw_{nb}_neighbourhoods", ["mw_neighbourhoods:in"], functools.partial(_mw_bands, nb, 10_000)))
    add(Case("mw_5_neighbourhoods", ["mw_neighbourhoods:out"], lambda: _mw_bands(5, 10_000), "refused", R_REACH, mw=M_FOUR))
    add(mw("mw_gap_512", ["mw_gap:in", "mw_neighbourhoods:in"], lambda: _mw_gap(512)))
    add(Case("mw_gap_513", ["mw_gap:out", "mw_neighbourhoods:out"], lambda: _mw_gap(513), "refused", R_REACH, mw=M_FOUR))
    add(mw("mw_width_2048", ["mw_width:in"], lambda: _mw_width(2048)))
    add(Case("mw_width_2049", ["mw_width:out"], lambda: _mw_width(2049), "refused", R_REACH, mw=M_WIDE))
    add(mw("mw_backwards_0", ["mw_backwards:in"], lambda: _mw_backwards(0)))
    add(Case("mw_backwards_1", ["mw_backwards:out"], lambda: _mw_backwards(1), "refused", R_REACH, mw=M_BACK))
    add(Case("mw_backwards_100", ["mw_backwards:out"], lambda: _mw_backwards(100), "refused", R_REACH, mw=M_BACK))
    add(mw("mw_late_narrow", ["mw_late:in", "mw_late_narrow"], lambda: _mw_late(300)))
    add(mw("mw_late_512", ["mw_late:in", "mw_late_narrow"], lambda: _mw_late(512)))
    add(mw("mw_late_wide", ["mw_late:in", "mw_late_wide"], lambda: _mw_late(1500)))
    add(Case("mw_late_wide_busy", ["mw_late:out", "mw_late_wide"], lambda: _mw_late(1500, busy=True), "refused", R_REACH, mw=M_BUSY))
    add(mw("mw_late_narrow_after_busy", ["mw_late:in", "mw_late_narrow"], lambda: _mw_late(512, busy=True)))
    add(Case("mw_late_no_free", ["mw_late:out"], lambda: _mw_late(300, nofree=True), "refused", R_REACH, mw=M_NOFREE))
    # a new narrow neighbourhood that widens in the next round: what exceeds 512 comes in a round early, as part of its first intake
    add(mw("mw_grow_1024", ["mw_new_intake:in"], lambda: _mw_grow(2, 10, 5, 1024)))
    add(Case("mw_grow_1025", ["mw_new_intake:out"], lambda: _mw_grow(2, 10, 5, 1025), "refused", R_REACH, mw=M_NEW_WIDE))
    # ... and one that exists from the workgroup's first round and widens past a sub-ring with what it takes in ahead
    # (taking in more than 2048 ahead always means moving on faster than the sub-ring has room for one round later: the first
    # reason is the one reported)
    add(mw("mw_grow_ahead_1536", ["mw_width_ahead:in"], lambda: _mw_grow(0, 1000, 900, 2048)))
    add(Case("mw_grow_ahead_2049", ["mw_width_ahead:out"], lambda: _mw_grow(0, 1000, 900, 2561), "refused", R_REACH, mw=M_WIDE_AHEAD))
    add(Case("ncols_3n_two_rounds_mw", ["mw_width_ahead:out"], lambda: _rect(*band(512 * 512, 3 * 512 * 512, slope=3.0), 3 * 512 * 512),
             "refused", R_NEW, mw=M_WIDE_AHEAD))
    add(mw("mw_speed_512", ["mw_speed:in"], lambda: _mw_speed(512, width=40)))
    add(mw("mw_speed_1020", ["mw_speed:in"], lambda: _mw_speed(1020)))  # 2 s + 8 = 2048: the sub-ring just holds both rounds
    add(Case("mw_speed_1021", ["mw_speed:out"], lambda: _mw_speed(1021), "refused", R_REACH, mw=M_FAST))
    add(mw("mw_first_fill_4095", ["mw_first_fill:in"], lambda: _mw_wide_fill(1365), max_padding=lift))
    add(mw("mw_first_fill_6000", ["mw_first_fill:out"], lambda: _mw_wide_fill(2000), max_padding=lift))
    add(Case("mw_ncols_1", ["ncols_1"], lambda: _rect(*band(100, 1, k=1), 1), "refused", R_PAD, mw=M_TWO))
    for cells in (20, 33, 70):
        add(Case(f"mw_pressure_{cells}", ["mw_mesh"], functools.partial(_pressure, cells), "plain" if cells < 70 else "cut-ring",
                 None if cells < 70 else R_REACH, mw=None if cells < 70 else "cut-ring"))
    return T


TABLE = _table()
BY_NAME = {c.name: c for c in TABLE}
assert len(BY_NAME) == len(TABLE), "case names must be unique"

LIMITS = sorted({t.split(":")[0] for c in TABLE for t in c.tags if ":" in t})
FEATURES = sorted({t for c in TABLE for t in c.tags if ":" not in t})


# ---- the seeded cases ------------------------------------------------------------------------------------------------------------
def seeded_cases(count=200, seed=20261016):
    """`count` Cases near the limits: random band slopes, widths, row-length profiles, empty runs, sizes around 128 / 512 multiples,
    far reaches.  Their expectation is left to restate_plan / the probe (expect = None)."""
    rng = np.random.default_rng(seed)
    out = []
    for q in range(count):
        r = np.random.default_rng(rng.integers(1 << 62))
        big = q % 8 == 7
        if big:
            n = int(r.integers(131_073, 300_000))
        else:
            base = int(r.choice([128, 512, 4096, 8192, 20_000]))
            n = max(1, base * int(r.integers(1, 4)) + int(r.integers(-3, 4)))
        slope = float(r.choice([0.25, 0.5, 1.0, 1.5, 1.99, 2.0, 2.01, 2.5, 3.0]))
        ncols = max(1, int(np.ceil(slope * n)) + int(r.integers(0, 50)))
        prof = str(r.choice(["const", "slice", "random", "spiky"]))
        k = int(r.integers(1, 12 if not big else 4))
        if prof == "const":
            lens = np.full(n, k)
        elif prof == "slice":  # constant inside each slice of 128, varying between slices
            lens = np.repeat(r.integers(1, k + 2, (n + 127) // 128), 128)[:n]
        elif prof == "random":
            lens = r.integers(max(1, k - 1), k + 2, n)
        else:
            lens = np.full(n, k)
            lens[r.integers(0, n, max(1, n // 2000))] = int(r.integers(k, 200))
        if r.random() < 0.3:  # empty runs
            for _ in range(int(r.integers(1, 4))):
                a = int(r.integers(0, n))
                lens[a:a + int(r.choice([1, 64, 128, 512, 1000]))] = 0
        p, c = band(n, ncols, slope=slope, lens=lens)
        if r.random() < 0.4 and p[-1] > 0:  # a few far reaches (back or forward), near the ring's reach
            c = c.copy()
            for _ in range(int(r.integers(1, 6))):
                kk = int(r.integers(0, p[-1]))
                c[kk] = int(np.clip(c[kk] + int(r.choice([-1, 1])) * int(r.integers(5000, 8400)), 0, ncols - 1))
        if r.random() < 0.2 and p[-1] > 0:  # unsorted rows
            c = _reverse_rows(p, c)
        mp = None if r.random() < 0.7 else 1e9
        out.append(Case(f"seeded_{q:03d}", [], functools.partial(lambda n, ncols, p, c: (n, ncols, p, c), n, ncols, p, c), None, max_padding=mp))
    return out


def _reverse_rows(p, c):
    """every row's columns in reverse order (unsorted rows)."""
    n = len(p) - 1
    lens = np.diff(p.astype(np.int64))
    row = np.repeat(np.arange(n), lens)
    k = np.arange(len(c)) - p.astype(np.int64)[row]
    return c[p.astype(np.int64)[row] + lens[row] - 1 - k]
