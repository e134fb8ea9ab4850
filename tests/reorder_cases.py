"""Pattern families for the create-time relabelling (reorder.hpp, maybe_reorder in capi_csr.hip): small matrices, each built to reach one
limit of the relabelled twin or of the kernels that serve it.  CPU only, seeded, cached.  tests/test_reorder_cases.py asserts through
mi_reorder_probe that every family reaches what it is for; tests/test_gpu_reorder_limits.py runs them through a relabelled handle.

case(name) -> (n, ptrow, indcol, values) with values(0 | 1 | 2) three seeded draws from (-1, 1), one per nonzero.

  tridiag:N        tridiagonal.  RCM of a path graph is the identity: the twin gets a contiguous row map, so it is created in the OFFSET form
                   (y_offset = 0, no device row map) that was written for partition pieces.  N = 7 is below the size at which a matrix is
                   relabelled at all, 8 is the first that is; 63 / 64 / 65 / 127 / 128 / 129 lie around the 64-row groups of the refresh kernel.
  blocktridiag:NB  4x4 blocks, block-tridiagonal, NB nodes: block = 4 with the identity, the blocked copy built without a block-row map.
  band:N           narrow S15-like band (about 15 of 25 columns) under a random numbering: a scattered permutation at small n.
  fe:K             synth.fe_matrix(K) under a random NODE numbering: block = 4, nodes kept together.
  fe_broken        fe:3 with one stored entry removed: almost blocked, relabelled row by row (block = 1).
  odd:N            band with n % 4 != 0: never block 4.
  components       three components of unequal size, rows holding only their diagonal, empty rows (some named by other rows, some not) and one
                   column no row names: disconnected RCM; x = Inf at the unnamed column must not reach y.
  upper            strictly upper band, the last rows empty: an unsymmetric pattern (the graph is symmetrised).
  unsorted         rows with shuffled and repeated columns: the order of a row's terms is the caller's.
  hub              row 0 and column 0 dense (n = 600) plus a band: one RCM level of n - 1 nodes, one row of 600 nonzeros (> 256).
  long:2500        n = 3000, one row of 2500 nonzeros, one of 257, the rest short: the segment loop of the refresh kernel takes several
                   passes, and the long row is a PLAIN block of the twin's ring plan written through a row map.
  stride           tridiagonal, n = 262 209 = 4096 * 64 + 65: the refresh kernel's grid (capped at 4096 groups) takes a second turn.
  powers           S15 band (w = 300) under a random numbering, the smallest n of POWERS_SIZES whose RELABELLED pattern mi_spmk_plan_probe
                   reports eligible for the one-launch powers step (None if none is: see powers_size()).
  sliced           S15 band under a random numbering, the smallest n of SLICED_SIZES whose relabelled pattern mi_sstream_plan_probe reports
                   eligible with MI355_SSTREAM_MAX_PADDING=1e9.

All but tridiag / blocktridiag (which must stay in natural order) end with a seeded random numbering; `scramble` keeps every row's terms in the
order they were written (unlike synth.permute_nodes, which sorts them)."""
import ctypes
import functools
import os
import zlib

import numpy as np

from navierstokes_amd import mpk, synth

TRIDIAG = (7, 8, 9, 63, 64, 65, 127, 128, 129)
BLOCKTRIDIAG = (2, 16, 17)
BAND = (8, 65, 129, 1000)
ODD = (1001, 1002)
POWERS_SIZES = (20_000, 40_000, 60_000)
SLICED_SIZES = (1_000, 2_000, 4_000, 8_000, 20_000, 60_000)
SLICED_ENV = ("MI355_SSTREAM_MAX_PADDING", "1e9")
STRIDE_N = 4096 * 64 + 65

NAMES = ([f"tridiag:{n}" for n in TRIDIAG] + [f"blocktridiag:{n}" for n in BLOCKTRIDIAG] + [f"band:{n}" for n in BAND]
         + ["fe:3", "fe:4", "fe_broken"] + [f"odd:{n}" for n in ODD]
         + ["components", "upper", "unsorted", "hub", "long:2500", "stride", "powers", "sliced"])

# what maybe_reorder must report for each family: None = not relabelled
BLOCK = {name: 1 for name in NAMES}
BLOCK.update({f"blocktridiag:{n}": 4 for n in BLOCKTRIDIAG})
BLOCK.update({"fe:3": 4, "fe:4": 4, "tridiag:7": None})
IDENTITY = tuple(f"tridiag:{n}" for n in TRIDIAG) + tuple(f"blocktridiag:{n}" for n in BLOCKTRIDIAG)


def seed(name):
    return zlib.crc32(name.encode())


def from_rows(rows):
    """CSR pattern of a list of per-row column arrays, terms in the order given"""
    lens = np.array([len(r) for r in rows], np.int64)
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    c = np.concatenate([np.asarray(r, np.int64) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    return p, c


def scramble(p, c, seed):
    """P A P^T for a seeded random numbering: old row r becomes row perm[r], its columns are renamed, its terms keep their order"""
    n = len(p) - 1
    perm = synth.node_permutation(n, seed).astype(np.int64)
    iperm = np.empty(n, np.int64)
    iperm[perm] = np.arange(n)
    lens = np.diff(p).astype(np.int64)[iperm]
    p2 = np.concatenate([[0], np.cumsum(lens)])
    idx = np.repeat(p[:-1].astype(np.int64)[iperm] - p2[:-1], lens) + np.arange(p2[-1])
    return p2.astype(np.int32), perm[c[idx]].astype(np.int32)


def tridiag(n):
    i = np.arange(n, dtype=np.int64)
    cols = np.stack([i - 1, i, i + 1], 1)
    ok = (cols >= 0) & (cols < n)
    return np.concatenate([[0], np.cumsum(ok.sum(1))]).astype(np.int32), cols[ok].astype(np.int32)


def blocktridiag(nb):
    rows = []
    for b in range(nb):
        nodes = [q for q in (b - 1, b, b + 1) if 0 <= q < nb]
        cols = np.concatenate([4 * q + np.arange(4) for q in nodes])
        rows += [cols] * 4
    return from_rows(rows)


def _band(n, seed):
    """the diagonal and a seeded 60 % of the columns within w = min(12, n / 4) of it (about 15 of 25 where n allows: synth's S15 fills
    a row of n < 15 columns completely, which at n = 8 is a dense and therefore 4x4-blocked matrix), columns ascending, scrambled"""
    w, rng = min(12, n // 4), np.random.default_rng(seed)
    i = np.arange(n)[:, None]
    cols = i + np.arange(-w, w + 1)[None, :]
    keep = (cols >= 0) & (cols < n) & ((rng.random(cols.shape) < 0.6) | (cols == i))
    p = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int32)
    c = cols[keep].astype(np.int32)
    return synth.permute_nodes(p, c, np.zeros(len(c)), block=1, seed=seed)[:2]


def _fe(k, seed):
    p, c, v = synth.fe_matrix(k)
    return synth.permute_nodes(p, c, v, block=4, seed=seed)[:2]


def _components():
    n = 200
    rows = [np.zeros(0, np.int64)] * n
    for i in range(0, 90):       # component A: a pentadiagonal band; each row also names one of the empty rows 170..189
        rows[i] = np.array([q for q in range(i - 2, i + 3) if 0 <= q < 90] + [170 + i % 20])
    for i in range(90, 130):     # component B: a path; nine of its rows name the empty rows 190..198
        rows[i] = np.array([q for q in (i - 1, i, i + 1) if 90 <= q < 130] + ([190 + (i - 90)] if i - 90 < 9 else []))
    for i in range(130, 150):    # component C: a star around 130
        rows[i] = np.array([130, i]) if i > 130 else np.arange(130, 150)
    for i in range(150, 170):    # rows holding only their diagonal: components of one node
        rows[i] = np.array([i])
    # rows 170..199 are empty; column 199 is named by no row
    return from_rows(rows)


def _upper():
    n = 300
    return from_rows([np.arange(i + 1, min(i + 6, n)) if i < n - 5 else np.zeros(0, np.int64) for i in range(n)])


def _unsorted():
    n, rng = 400, np.random.default_rng(seed("unsorted"))
    rows = []
    for i in range(n):
        r = np.clip(i + rng.integers(-8, 9, 10), 0, n - 1)   # drawn with repetition, in no order
        rows.append(np.concatenate([r, r[:1], [i]]))          # ... and the first column once more, then the diagonal
    return from_rows(rows)


def _hub():
    n = 600
    return from_rows([np.arange(n)] + [np.array([0] + [q for q in (i - 1, i, i + 1) if 1 <= q < n]) for i in range(1, n)])


def _long(m):
    n = 3000
    rows = [np.array([q for q in (i - 1, i, i + 1) if 0 <= q < n]) for i in range(n)]
    rows[17] = 250 + np.arange(m)
    rows[1000] = 872 + np.arange(257)
    return from_rows(rows)


def probe_spmk(p, c):
    n = len(p) - 1
    e, r, m = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    mpk.check(mpk.lib().mi_spmk_plan_probe(n, p.ctypes.data, c.ctypes.data, ctypes.byref(e), ctypes.byref(r), ctypes.byref(m)))
    return bool(e.value)


def probe_sstream(p, c):
    n = len(p) - 1
    e, r, st, pad = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong(), ctypes.c_double()
    old = os.environ.get(SLICED_ENV[0])
    os.environ[SLICED_ENV[0]] = SLICED_ENV[1]
    try:
        mpk.check(mpk.lib().mi_sstream_plan_probe(n, n, p.ctypes.data, c.ctypes.data, ctypes.byref(e), ctypes.byref(r), ctypes.byref(st), ctypes.byref(pad)))
    finally:
        if old is None:
            del os.environ[SLICED_ENV[0]]
        else:
            os.environ[SLICED_ENV[0]] = old
    return bool(e.value)


def relabelled_pattern(p, c):
    """pattern of the twin the library would build: test_ring_plan.relabelled"""
    from test_ring_plan import relabelled
    return relabelled(np.ascontiguousarray(p, np.int32), np.ascontiguousarray(c, np.int32))


def _smallest_eligible(sizes, w, probe, seed):
    for n in sizes:
        p, c, v = synth.rows("s15", n, w=w)
        p, c = synth.permute_nodes(p, c, v, block=1, seed=seed)[:2]
        if probe(*relabelled_pattern(p, c)):
            return n, p, c
    return None, p, c


@functools.lru_cache(maxsize=None)
def powers_size():
    """the n of `powers`: the smallest of POWERS_SIZES whose relabelled pattern is eligible for the one-launch powers step, or None"""
    return _smallest_eligible(POWERS_SIZES, 300, probe_spmk, 21)[0]


@functools.lru_cache(maxsize=None)
def _pattern(name):
    kind, _, arg = name.partition(":")
    if kind == "tridiag":
        return tridiag(int(arg))
    if kind == "blocktridiag":
        return blocktridiag(int(arg))
    if kind in ("band", "odd"):
        return _band(int(arg), seed(name) % 1000)
    if kind == "fe":
        return _fe(int(arg), 11)
    if name == "fe_broken":
        p, c = _fe(3, 11)
        r = len(p) // 2                                   # one stored entry of one row of a node goes: no exact 4x4 structure any more
        k = int(p[r]) + 1
        p = p.copy()
        p[r + 1:] -= 1
        return p, np.delete(c, k)
    if name == "powers":
        return _smallest_eligible(POWERS_SIZES, 300, probe_spmk, 21)[1:]
    if name == "sliced":
        return _smallest_eligible(SLICED_SIZES, 20, probe_sstream, 22)[1:]
    if name == "stride":
        return scramble(*tridiag(STRIDE_N), seed(name))
    build = {"components": _components, "upper": _upper, "unsorted": _unsorted, "hub": _hub, "long": lambda: _long(int(arg))}[kind]
    return scramble(*build(), seed(name))


@functools.lru_cache(maxsize=None)
def _values(name, k):
    nnz = int(_pattern(name)[0][-1])
    v = np.random.default_rng([seed(name), k]).uniform(np.nextafter(-1.0, 0.0), 1.0, nnz)
    v.setflags(write=False)
    return v


def case(name):
    p, c = _pattern(name)
    p = np.ascontiguousarray(p, np.int32)
    c = np.ascontiguousarray(c, np.int32)
    p.setflags(write=False)
    c.setflags(write=False)

    def values(k):
        assert k in (0, 1, 2)
        return _values(name, k)

    return len(p) - 1, p, c, values
