"""Seeded cases for the multi-rank fuzz (tests/test_multirank_fuzz.py and its worker; TEST INFRASTRUCTURE, not a conftest).

Every case is (P, C, V, row_starts, label): one global CSR matrix and a cut of its rows into N = len(row_starts) - 1 ranks.  The
patterns are the ones where a ghost range or a unit's row count can be off by one without a band noticing:
  ragged   test_planner_fuzz.random_pattern / test_gpu_parity._random_banded: rows of length 0 and rows longer than a block,
           unsorted and repeated columns, clusters that wander or jump, a few far couplings (sparse ghost sets towards ranks
           that are not neighbours: the pack kernel runs)
  upwind   rows that reach only down the numbering: some ranks send or receive nothing
  fe       synth.fe_matrix with some node rows emptied and a few far 4x4 blocks, cut at node boundaries (the blocked one-launch
           step is eligible); one cut that is not a multiple of 4 (the documented fallback, same bits)
  mesh     synth.pressure_matrix: several column bands per row (cut-ring pieces, the staged scalar one-launch step)
  degenerate  n < N, every row on one rank, a rank whose rows are all empty, a rank that names only ghost columns, a
           block-diagonal matrix (no ghosts at all), n = 1
Cuts: nnz-balanced, equal rows, random, and repeated cut points (empty ranks)."""
import numpy as np

from navierstokes_amd import dist as D
from navierstokes_amd import synth
from test_gpu_parity import _random_banded
from test_planner_fuzz import random_pattern

NRANKS = (2, 3, 5, 8)
CUTS = ("balanced", "equal", "random", "repeated")


def _csr(rows, vals):
    lens = np.array([len(r) for r in rows], np.int64)
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    c = np.concatenate(rows).astype(np.int32) if len(rows) and p[-1] else np.zeros(0, np.int32)
    v = np.concatenate(vals).astype(np.float64) if len(rows) and p[-1] else np.zeros(0)
    return p, c, v


def _split(p, c, v):
    n = len(p) - 1
    return [c[p[i]:p[i + 1]].astype(np.int64) for i in range(n)], [v[p[i]:p[i + 1]] for i in range(n)]


def cut_rows(rng, n, nranks, how, lens=None, align=1):
    """row_starts for one of the four cuts (align: cut points at multiples of `align` where the cut can choose)."""
    if how == "balanced":
        return D.balanced_row_starts(n, nranks, lens, align=align)
    if how == "equal":
        return D.balanced_row_starts(n, nranks, None, align=align)
    if how == "random":
        cuts = np.sort(rng.integers(0, n // align + 1, nranks - 1)) * align
    else:  # "repeated": at most two distinct cut points, so that several ranks own nothing
        pts = rng.integers(0, n // align + 1, 2) * align
        cuts = np.sort(rng.choice(pts, nranks - 1))
    return np.concatenate([[0], np.minimum(cuts, n), [n]]).astype(np.int64)


def ragged(rng, n):
    if rng.random() < 0.5:
        p, c = random_pattern(rng, n)
        v = rng.uniform(-1, 1, len(c))
    else:
        mode = str(rng.choice(["uniform", "mult8", "const", "spiky"]))
        p, c, v = _random_banded(rng, n, n, int(rng.integers(2, 20)), int(rng.choice([5, 60, 400])), mode)
        rows, vals = _split(p, c, v)
        for i in rng.choice(n, max(1, n // 100), replace=False):  # far couplings, appended (the row is no longer sorted)
            far = rng.integers(0, n, int(rng.integers(1, 4)))
            rows[i] = np.concatenate([rows[i], far])
            vals[i] = np.concatenate([vals[i], rng.uniform(-1, 1, len(far))])
        p, c, v = _csr(rows, vals)
    return p, c, v


def upwind(rng, n):
    p, c, v = ragged(rng, n)
    keep = c <= np.repeat(np.arange(n), np.diff(p))
    rows = np.repeat(np.arange(n), np.diff(p))[keep]
    p2 = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return p2, c[keep].copy(), v[keep].copy()


def fe(rng, nx):
    """FE matrix (4x4 node blocks) with a few node rows emptied and a few far node blocks appended: still exact block structure."""
    p, c, v = synth.fe_matrix(nx)
    n = len(p) - 1
    rows, vals = _split(p, c, v)
    nn = n // 4
    for b in rng.choice(nn, max(1, nn // 40), replace=False):
        for r in range(4):
            rows[4 * b + r], vals[4 * b + r] = np.zeros(0, np.int64), np.zeros(0)
    for b in rng.choice(nn, max(1, nn // 60), replace=False):
        far = int(rng.integers(0, nn))
        for r in range(4):
            rows[4 * b + r] = np.concatenate([rows[4 * b + r], 4 * far + np.arange(4)])
            vals[4 * b + r] = np.concatenate([vals[4 * b + r], rng.uniform(-1, 1, 4)])
    return _csr(rows, vals)


def mesh(rng, nx):
    return synth.pressure_matrix(nx)


FAMILIES = ("ragged", "upwind", "fe", "mesh", "ragged", "fe")


def case(seed):
    """The seed-th fuzz case: family, size, N and cut drawn from the seed."""
    rng = np.random.default_rng(7000 + seed)
    fam = FAMILIES[seed % len(FAMILIES)]
    nranks = NRANKS[(seed // len(FAMILIES)) % len(NRANKS)] if seed >= len(FAMILIES) else NRANKS[seed % len(NRANKS)]
    how = CUTS[(seed // 2) % len(CUTS)]
    align = 1
    if fam == "ragged":
        P, C, V = ragged(rng, int(rng.choice([37, 300, 1500, 4000])))
    elif fam == "upwind":
        P, C, V = upwind(rng, int(rng.choice([300, 2000, 5000])))
    elif fam == "fe":
        P, C, V = fe(rng, int(rng.integers(3, 7)))
        align = 4
    else:
        P, C, V = mesh(rng, int(rng.integers(5, 12)))
    n = len(P) - 1
    rs = cut_rows(rng, n, nranks, how, np.diff(P), align)
    if fam == "fe" and seed % 12 == 5:  # one cut off the node boundaries: the blocked step's documented fallback, same bits
        rs[1] = min(rs[1] + 2, rs[2])
        align = 0
    return P, C, V, rs, f"{fam}-s{seed}-N{nranks}-{how}-a{align}-n{n}"


def degenerate():
    """The named corner cases (P, C, V, row_starts, label)."""
    out = []
    rng = np.random.default_rng(99)
    # n < N: three rows over five and eight ranks
    P, C, V = _csr([np.array([0, 2]), np.array([1, 0, 1]), np.array([2])], [rng.uniform(-1, 1, 2), rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 1)])
    for N in (5, 8):
        out.append((P, C, V, D.balanced_row_starts(3, N), f"n<N-{N}"))
    # every row on one rank (the others own nothing)
    P, C, V = ragged(np.random.default_rng(5), 300)
    out.append((P, C, V, np.array([0, 0, 300, 300], np.int64), "all-on-rank1-of-3"))
    out.append((P, C, V, np.array([0, 0, 0, 0, 0, 300], np.int64), "all-on-last-of-5"))
    # a rank whose rows are all empty (its columns are still other ranks' ghosts)
    P, C, V = ragged(np.random.default_rng(6), 600)
    rows, vals = _split(P, C, V)
    for i in range(200, 400):
        rows[i], vals[i] = np.zeros(0, np.int64), np.zeros(0)
    P, C, V = _csr(rows, vals)
    out.append((P, C, V, np.array([0, 200, 400, 600], np.int64), "empty-rows-rank1-of-3"))
    # a rank that names only ghost columns (its own rows look at the other ranks' x only)
    rows, vals = _split(*ragged(np.random.default_rng(8), 800))
    for i in range(300, 500):
        rows[i] = rows[i][(rows[i] < 300) | (rows[i] >= 500)]
        if not len(rows[i]):
            rows[i] = np.array([(7 * i) % 300, 500 + (11 * i) % 300])
        vals[i] = rng.uniform(-1, 1, len(rows[i]))
    P, C, V = _csr(rows, vals)
    out.append((P, C, V, np.array([0, 300, 500, 800], np.int64), "only-ghosts-rank1-of-3"))
    # block diagonal: no ghosts anywhere
    rs = np.array([0, 250, 400, 900, 1000], np.int64)
    rows, vals = _split(*ragged(np.random.default_rng(9), 1000))
    for r in range(4):
        lo, hi = int(rs[r]), int(rs[r + 1])
        for i in range(lo, hi):
            rows[i] = lo + rows[i] % (hi - lo)
    P, C, V = _csr(rows, vals)
    out.append((P, C, V, rs, "block-diagonal-4"))
    # n = 1
    P, C, V = np.array([0, 2], np.int32), np.array([0, 0], np.int32), np.array([0.75, -1.5])
    out.append((P, C, V, np.array([0, 1], np.int64), "n1-N1"))
    out.append((P, C, V, np.array([0, 0, 1], np.int64), "n1-N2"))
    out.append((P, C, V, np.array([0, 1, 1, 1], np.int64), "n1-N3"))
    return out


def all_cases(nseeds):
    return [case(s) for s in range(nseeds)] + degenerate()


def slices(P, C, V, rs, r):
    """rank r's rows as mi_part_create wants them"""
    lo, hi = int(rs[r]), int(rs[r + 1])
    p = (P[lo:hi + 1] - P[lo]).astype(np.int32)
    return p, np.ascontiguousarray(C[P[lo]:P[hi]]), np.ascontiguousarray(V[P[lo]:P[hi]])


def make_plans(P, C, V, rs):
    """N mi_part handles (test_partition._Plan) with every peer's send list handed over by hand, as torch.distributed would."""
    from test_partition import _Plan
    N = len(rs) - 1
    plans = [_Plan(rs, r, N, *slices(P, C, V, rs, r)) for r in range(N)]
    for r in range(N):
        for q in range(N):
            if q != r:
                plans[r].set_send(q, plans[q].recv_ids[r])
    return plans


def halo_of(plans, rs, r, x):
    """rank r's halo as the peers pack it: peer q's send index, its send counts and offsets, applied to q's slice of x"""
    pl = plans[r]
    parts = []
    for q in range(len(plans)):
        cnt = pl.recv_counts[q]
        if not cnt:
            continue
        sidx, sc = plans[q].send_index(), plans[q].send_counts_()
        assert sc[r] == cnt, f"rank {q} sends {sc[r]} entries to rank {r}, which expects {cnt}"
        s_off = int(sc[:r].sum())
        parts.append(x[int(rs[q]):int(rs[q + 1])][sidx[s_off:s_off + cnt]])
    halo = np.concatenate(parts) if parts else np.zeros(0)
    assert len(halo) == pl.n_halo
    return halo


IEEE = np.array([-0.0, np.inf, -np.inf, np.nan, 5e-324, -1.1e-308, 0.0, 1e308])


def ieee_at_ghosts(x, P, C, rs):
    """x with -0.0, +-Inf, NaN and subnormals at ghost positions only (columns some OTHER rank reads)"""
    x = x.copy()
    g = ghost_columns(P, C, rs)
    x[g] = IEEE[np.arange(len(g)) % len(IEEE)]
    return x


def ghost_columns(P, C, rs):
    """global columns that some rank reads as a ghost"""
    rows = np.repeat(np.arange(len(P) - 1), np.diff(P))
    owner_row = np.searchsorted(rs, rows, side="right") - 1
    owner_col = np.searchsorted(rs, C, side="right") - 1
    return np.unique(C[owner_row != owner_col])
