"""Matrices at the limits of the ring kernel's plan (spmv_ring.hpp, ring_plan.hpp) — TEST INFRASTRUCTURE, not a conftest.
Deterministic numpy, no GPU; shared by tests/test_ring_limits.py (census of every case) and tests/test_gpu_ring_limits.py (bits).

A case is built for ONE configuration of ring_plan.hpp (its sizes come from that configuration's constants) and named after the
limit it sits on.  case(name, cfg) -> Case(n, ncols, ptrow, indcol, coef, want): `want` maps a census counter
(navierstokes_amd.mpk.RING_CENSUS) to the smallest value the case must reach, or to ("==", v) for an exact one.

Why the cases are as large as they are: a ring launch has at least wg_unit workgroups, so a run has ceil(blocks / wg_unit) blocks or
fewer, and a block holds at most ROWS rows.  A run of three blocks therefore needs more than 2 * wg_unit * ROWS rows whatever the rows
hold; one nonzero per row is the cheapest way to get there.  Blocks the window cannot serve weigh kRingPlainWeight when the rows
are dealt out, so a run takes four of them only once the mean weight per run passes sixteen (R1).

Values are seeded uniform(-1, 1); rows of more than one nonzero name their columns in an order that is not ascending."""
import collections
import functools

import numpy as np

# ---- constants of ring_plan.hpp ------------------------------------------------------------------------------------------------
Config = collections.namedtuple("Config", "id T NNZB RING D WG_UNIT ROWS")
CONFIGS = {1: Config(1, 512, 2048, 5120, 2, 512, 1024), 2: Config(2, 512, 4096, 5120, 2, 256, 1024),
           3: Config(3, 512, 4096, 11264, 2, 256, 1024), 4: Config(4, 256, 2048, 5120, 2, 512, 256)}   # ROWS: T for 4, else 2 T
K_RING_MAX_B, K_RING_MAX_PLAIN, K_RING_PLAIN_WEIGHT = 160, 3, 4
K_MEASURE_NNZ = 200_000   # capi_csr.hip: from here on mi_csr_create would time its kernels (the tests switch that off)

Case = collections.namedtuple("Case", "n ncols ptrow indcol coef want")


def assemble(n, ncols, base, special, seed):
    """CSR arrays of a matrix whose row r names the columns base[r] (an [n, k] array) unless special[r] (a 1-D array, maybe empty)
    replaces them.  Values: seeded uniform(-1, 1)."""
    base = np.asarray(base, np.int64).reshape(n, -1)
    k = base.shape[1]
    lens = np.full(n, k, np.int64)
    rows = sorted(special)
    for r in rows:
        lens[r] = len(special[r])
    ptrow = np.concatenate([[0], np.cumsum(lens)])
    indcol = np.empty(int(ptrow[-1]), np.int64)
    keep = np.ones(n, bool)
    keep[rows] = False
    indcol[(ptrow[:-1][keep][:, None] + np.arange(k)[None, :]).ravel()] = base[keep].ravel()
    for r in rows:
        indcol[ptrow[r]:ptrow[r + 1]] = special[r]
    assert n == 0 or (indcol.min() >= 0 and indcol.max() < ncols), (indcol.min(), indcol.max(), ncols)
    assert ptrow[-1] < 2 ** 31
    coef = np.random.default_rng(seed).uniform(-1.0, 1.0, len(indcol))
    out = ptrow.astype(np.int32), indcol.astype(np.int32), coef
    for a in out:
        a.setflags(write=False)
    return out


def scramble(cols, r):
    """the columns of row r in an order that is not ascending (rotated by a third, every other row reversed as well)"""
    cols = np.asarray(cols, np.int64)
    if len(cols) < 2:
        return cols
    cols = np.roll(cols, len(cols) // 3 + 1)
    return cols[::-1] if r & 1 else cols


def long_row(r, nn, ncols):
    """nn columns around r, three apart, scrambled"""
    start = max(0, min(r - nn, ncols - 3 * nn - 1))
    assert start >= 0 and start + 3 * nn < ncols + 3
    return scramble(np.minimum(start + 3 * np.arange(nn), ncols - 1), r)


def diagonal(n):
    return np.arange(n, dtype=np.int64)[:, None]


# ---- R1: run kinds -----------------------------------------------------------------------------------------------------------------
# One nonzero per row; every PERIOD rows three clusters of 3, 4 and 40 adjacent rows of two nonzeros more than RING columns apart
# (each such row is a block of its own that the window cannot serve).  N_R1: the smallest n (in steps of 100 000 rows) at which the
# plan holds runs of all three kinds with a run of exactly kRingMaxPlain and a kind-0 run — found with the census, pinned by
# tests/test_ring_limits.py, which also shows that 600 000 rows are not enough.
R1_PERIOD = 400_000
R1_CLUSTERS = (K_RING_MAX_PLAIN, K_RING_MAX_PLAIN + 1, 40)
N_R1 = {4: 1_800_000, 2: 2_200_000}


def r1_matrix(cfg, n, period=R1_PERIOD, clusters=R1_CLUSTERS, seed=101):
    C = CONFIGS[cfg]
    special = {}
    for g0 in range(period // 2, n - 3 * 20 * C.ROWS, period):
        r = g0
        for m in clusters:
            for q in range(m):
                c = min(r + q, n - C.RING - 2)
                special[r + q] = np.array([c + C.RING + 1, c])            # descending, RING + 2 columns apart
            r += 20 * C.ROWS                                              # the clusters of a group lie twenty blocks apart
    return assemble(n, n, diagonal(n), special, seed)


def r1(cfg):
    n = N_R1[cfg]
    p, c, v = r1_matrix(cfg, n)
    want = dict(runs_kind0=1, runs_kind1=1, runs_kind3=1, runs_wide3=1, runs_wide4=1, kind0_wide=K_RING_MAX_PLAIN + 1, plain=3,
                slot_wrap=1, base_advance=1)
    return Case(n, n, p, c, v, want)


def r1_small(cfg):
    """the finding: the same matrix at 600 000 rows deals every block the window cannot serve into a run of its own"""
    n = 600_000
    p, c, v = r1_matrix(cfg, n)
    return Case(n, n, p, c, v, dict(runs_kind0=("==", 0), wide_max_per_run=("==", 1), runs_kind3=1, plain=sum(R1_CLUSTERS)))


# ---- R2: PLAIN block flavours ------------------------------------------------------------------------------------------------------
def r2(cfg, ncols_cut=0, dense=False):
    """Rows of NNZB + 1, 2 NNZB, 2 NNZB + 1 and 3 NNZB + 7 nonzeros (the chunked chain of thread 0) and one-row blocks spanning
    RING + 1 columns, 6.4 blocks apart so that they fall on every position of a run; two of them in a row; one as the last row.
    Configuration 4: the window restarts behind a PLAIN block, which brings RING new columns, so a LEAN plan ends the run there and
    a PLAIN block is the last of its run (and the first, behind another).  dense: twice as many such rows — more forced cuts than
    workgroups, the plan is not LEAN, the runs are dealt by weight and the PLAIN blocks fall on every position, as for 1 to 3."""
    C = CONFIGS[cfg]
    n = C.ROWS * (4 * C.WG_UNIT + 16)
    ncols = n - ncols_cut
    flav = [C.NNZB + 1, 2 * C.NNZB, 2 * C.NNZB + 1, 3 * C.NNZB + 7, -1]
    special = {}

    def put(r, f):
        if f < 0:
            c = max(0, min(r, ncols - 1) - C.RING)
            special[r] = np.array([c + C.RING, c])                        # spans exactly RING + 1 columns
        else:
            special[r] = long_row(r, f, ncols)
    stride = ((16 if dense else 32) * C.ROWS) // 5
    for j, r in enumerate(range(stride, n - 2 * C.ROWS, stride)):
        put(r + (j % 7), flav[j % len(flav)])
        if j % 11 == 5:                                                   # two in a row
            put(r + (j % 7) + 1, flav[(j + 2) % len(flav)])
    put(n - 1, flav[3])                                                   # the last row: the kernel's unclamped loads read the padding
    p, c, v = assemble(n, ncols, np.minimum(diagonal(n), ncols - 1), special, 200 + cfg)
    want = dict(plain_first=1, plain_last=1, plain_middle=1, plain_after_plain=1, plain_ends_matrix=("==", 1), plain_long_row=4, plain_span=1,
                runs_kind3=1, runs_kind1=1)
    if cfg == 4:
        want["lean"] = ("==", 0 if dense else 1)
        if dense:
            del want["runs_kind1"]
        else:
            del want["plain_middle"], want["plain_after_plain"], want["runs_kind1"]
    return Case(n, ncols, p, c, v, want)


# ---- R3: full and empty blocks -----------------------------------------------------------------------------------------------------
def r3(cfg, ncols_cut=0):
    """One nonzero per row gives blocks of exactly the row limit; a stretch of rows of NNZB / ROWS nonzeros gives blocks that are full
    in rows AND nonzeros, one row a nonzero short gives NNZB - 1; a stretch of empty rows gives empty blocks at every position of a
    run; the last 300 rows are empty."""
    C = CONFIGS[cfg]
    n = C.ROWS * (2 * C.WG_UNIT + 40) + 300
    ncols = n - ncols_cut
    per = C.NNZB // C.ROWS
    special = {}
    d0 = 10 * C.ROWS
    for r in range(d0, d0 + 6 * C.ROWS):                                  # dense stretch: full blocks
        special[r] = scramble(np.minimum(r + 2 * np.arange(per), ncols - 1), r)
    special[d0 + 2 * C.ROWS + 5] = special[d0 + 2 * C.ROWS + 5][:-1]      # NNZB - 1 in that block
    e0 = 30 * C.ROWS + 17
    for r in range(e0, e0 + 9 * C.ROWS):                                  # empty stretch: more blocks than a run holds
        special[r] = np.zeros(0, np.int64)
    for r in range(n - 300, n):
        special[r] = np.zeros(0, np.int64)
    p, c, v = assemble(n, ncols, np.minimum(diagonal(n), ncols - 1), special, 300 + cfg)
    want = dict(served_full=1, served_full_less1=1, served_row_limit=100, empty_first=1, empty_last=1, empty_middle=1,
                runs_kind1=C.WG_UNIT // 2, run_max=3)
    if cfg != 4:
        want["served_rows_over_t"] = 100
    return Case(n, ncols, p, c, v, want)


# ---- R4: window width --------------------------------------------------------------------------------------------------------------
def r4(cfg):
    """A block whose columns span exactly RING (served); a row one column further, which the planner cuts off into the next block;
    a single row spanning RING + 1 (PLAIN)."""
    C = CONFIGS[cfg]
    n = C.ROWS * 40 + 3 * C.RING
    special = {}
    for k, b in enumerate((5, 11, 17)):
        r = b * C.ROWS
        special[r + C.ROWS // 2] = np.array([r + C.RING - 1 + (k > 0)])     # block b: columns r .. r + RING - 1 (then one more)
    r = 23 * C.ROWS + 9
    special[r] = np.array([r + C.RING - 1, r])                             # one row spanning RING: served
    special[r + 3 * C.ROWS] = np.array([r + 3 * C.ROWS + C.RING, r + 3 * C.ROWS])   # RING + 1: PLAIN
    p, c, v = assemble(n, n, diagonal(n), special, 400 + cfg)
    return Case(n, n, p, c, v, dict(served_span_ring=2, served_span_max=("==", C.RING), plain_span=("==", 1), plain=("==", 1)))


# ---- R5: restarts and refills inside a run -------------------------------------------------------------------------------------------
def r5(cfg, ncols_cut=0):
    """Blocks of ROWS rows, one nonzero each, whose column ranges are chosen block by block against the window [.., whi) the block
    before left: bring exactly T, T + 1, 4 T, 4 T + 1 and RING new columns without a restart, jump ahead of the window, reach back
    behind it.  Eight such blocks a cycle against runs of three, so every step falls on every position of a run.  Under
    configuration 4 five blocks of a cycle would each have to start a LEAN run: that takes more runs than workgroups, so the
    planner keeps the uniform deal and the plan is NOT LEAN — the general kernel's refill loop and its tail run inside runs."""
    C = CONFIGS[cfg]
    nblk = 2 * C.WG_UNIT + 24
    n = nblk * C.ROWS
    tail = 64 * C.ROWS if ncols_cut else 0                                # rectangular form: diagonal rows behind, clamped to the last column
    steps = (None, C.T, C.T + 1, 4 * C.T, 4 * C.T + 1, C.RING, "ahead", 3 * C.T // 2)
    col = np.empty(n, np.int64)
    whi = 0
    for b in range(nblk):
        r0 = b * C.ROWS
        s = steps[b % len(steps)]
        if s is None:                                                     # back to the diagonal: behind the window from the second cycle on
            lo, hi = r0, r0 + C.ROWS - 1
        elif s == "ahead":
            lo, hi = whi + 1000, whi + 1000 + 2 * C.ROWS
        else:                                                             # exactly s new columns, the window's upper end kept
            hi = whi + s - 1
            lo = max(whi - 7, hi - C.RING + 1)
        i = np.arange(C.ROWS)
        col[r0:r0 + C.ROWS] = np.minimum(lo + i, hi)
        col[r0 + C.ROWS - 1 - (b % 5)] = hi
        col[r0 + (b % 3)] = lo
        whi = max(hi + 1, whi) if s is not None and s != "ahead" else hi + 1
    ncols = int(col.max()) + 1
    if tail:
        assert ncols <= n + tail - ncols_cut
        n, ncols = n + tail, n + tail - ncols_cut
        col = np.concatenate([col, np.minimum(np.arange(n - tail, n), ncols - 1)])
    p, c, v = assemble(n, ncols, col[:, None], {}, 500 + cfg)
    want = dict(restart_ahead=10, restart_back=10, new_t=10, new_t1=10, new_4t=10, new_4t1=10, new_ring=10, new_mid=10, lean=("==", 0),
                runs_kind1=C.WG_UNIT // 2, run_max=("==", 3), slot_wrap=1, base_advance=1, uniform=("==", 1))
    return Case(n, ncols, p, c, v, want)


# ---- R7: non-uniform runs (LEAN, forced cuts) ----------------------------------------------------------------------------------------
def r7(cfg=4):
    """three nonzeros per row around a centre that jumps every 3000 rows, 600 000 rows: the LEAN planner cuts its runs at the jumps"""
    C = CONFIGS[cfg]
    n = 600_000
    r = np.arange(n, dtype=np.int64)
    centre = np.clip(r + 4 * C.RING * ((r // 3000) % 2), 1, n - 2)
    base = np.stack([centre + 1, centre - 1, centre], axis=1)
    p, c, v = assemble(n, n, base, {}, 700 + cfg)
    return Case(n, n, p, c, v, dict(lean=("==", 1), uniform=("==", 0), runs_idle=1, runs_kind1=200, runs_kind0=("==", 0), runs_kind3=("==", 0)))


# ---- R8: run length against depth ----------------------------------------------------------------------------------------------------
def r8(cfg=4):
    """More than 8 * wg_unit blocks, so that a run may hold nine; the column jumps ahead at the blocks that make the first runs 1, 2,
    3, 4 and 5 blocks long (a LEAN run ends where the window would restart)."""
    C = CONFIGS[cfg]
    nblk = 8 * C.WG_UNIT + 40
    n = nblk * C.ROWS
    col = np.arange(n, dtype=np.int64)
    shift, b = 0, 0
    for length in (1, 2, 3, 4, 5):
        b += length
        shift += 2 * C.RING
        col[b * C.ROWS:] += 2 * C.RING
    ncols = n + shift
    p, c, v = assemble(n, ncols, col[:, None], {}, 800 + cfg)
    want = dict(runs_len1=1, runs_len2=1, runs_len3=1, runs_len4=1, runs_len5=1, runs_len9=100, lean=("==", 1), depth=("==", 2))
    return Case(n, ncols, p, c, v, want)


BUILDERS = dict(r1=r1, r1_small=r1_small, r2=r2, r2_dense=functools.partial(r2, dense=True), r3=r3, r4=r4, r5=r5, r7=r7, r8=r8,
                r2_rect=functools.partial(r2, ncols_cut=700), r3_rect=functools.partial(r3, ncols_cut=700), r5_rect=functools.partial(r5, ncols_cut=700))
# the configurations every case is built for: wherever a configuration's constants change the case, all of them
CONFIGS_OF = dict(r1=(4, 2), r1_small=(4, 2), r2=(4, 2, 1, 3), r2_dense=(4,), r3=(4, 2, 1, 3), r4=(4, 2, 1, 3), r5=(4, 2, 1, 3), r7=(4,), r8=(4,),
                  r2_rect=(4, 2), r3_rect=(4, 2), r5_rect=(4, 2))
ALL = [(name, cfg) for name in BUILDERS for cfg in CONFIGS_OF[name]]


@functools.lru_cache(maxsize=4)
def case(name, cfg):
    return BUILDERS[name](cfg)


def row_maps(n):
    """(name, rowmap, length of y) for R9: rows scattered over a longer y (a fixed odd stride keeps them distinct), rows moved up by an
    odd offset"""
    m = n + n // 2 + 11
    while np.gcd(7919, m) != 1:
        m += 1
    scattered = (np.arange(n, dtype=np.int64) * 7919) % m
    return [("scattered", scattered.astype(np.int32), m), ("offset", (np.arange(n, dtype=np.int64) + 37).astype(np.int32), n + 37 + 11)]
