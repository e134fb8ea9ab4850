"""Every pattern family of tests/reorder_cases.py reaches what it is for — checked without a GPU through mi_reorder_probe (the relabelling
mi_csr_create would compute) and the planners' host probes, so that tests/test_gpu_reorder_limits.py meets its limits by construction."""
import ctypes

import numpy as np
import pytest

import reorder_cases as RC
from navierstokes_amd import mpk


def reorder_probe(p, c):
    n = len(p) - 1
    perm = np.full(n, -1, np.int32)
    blk = ctypes.c_int()
    sb, sa = ctypes.c_double(), ctypes.c_double()
    mpk.check(mpk.lib().mi_reorder_probe(n, p.ctypes.data, c.ctypes.data, ctypes.byref(blk), perm.ctypes.data, ctypes.byref(sb), ctypes.byref(sa)))
    return blk.value, perm


def n_components(n, p, c):
    """connected components of the symmetrised pattern (union-find; every row is a node, named or not)"""
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    rows = np.repeat(np.arange(n), np.diff(p))
    for r, q in zip(rows.tolist(), c.tolist()):
        a, b = find(r), find(q)
        if a != b:
            parent[a] = b
    return len({find(a) for a in range(n)})


@pytest.mark.parametrize("name", RC.NAMES)
def test_family_reaches_what_it_is_for(name):
    n, p, c, values = RC.case(name)
    nnz = int(p[-1])
    assert len(p) == n + 1 and len(c) == nnz and p[0] == 0 and (np.diff(p) >= 0).all()
    assert nnz == 0 or (c.min() >= 0 and c.max() < n)
    vs = [values(k) for k in range(3)]
    for k, v in enumerate(vs):
        assert v.shape == (nnz,) and v.dtype == np.float64 and (np.abs(v) < 1).all()
        assert values(k) is v                                   # cached: the draws are shared, nobody changes them
        assert not v.flags.writeable
    assert not np.array_equal(vs[0], vs[1]) and not np.array_equal(vs[1], vs[2]) and not np.array_equal(vs[0], vs[2])
    block, perm = reorder_probe(p, c)
    assert sorted(perm.tolist()) == list(range(n)), "perm is not a permutation"
    lens = np.diff(p)
    if RC.BLOCK[name] is None:
        assert n < 8                                            # maybe_reorder leaves it alone even when forced
    else:
        assert n >= 8 and block == RC.BLOCK[name]
    if block == 4:
        assert n % 4 == 0 and (perm[0::4] % 4 == 0).all(), "a node does not start on a multiple of four"
        for j in (1, 2, 3):
            assert (perm[j::4] == perm[0::4] + j).all(), "the four rows of a node do not stay together"
    if name in RC.IDENTITY:
        assert np.array_equal(perm, np.arange(n)), "RCM of a path (of nodes) must be the identity"
    else:
        assert not np.array_equal(perm, np.arange(n)), "meant to end with a scattered permutation"
    kind = name.partition(":")[0]
    if kind == "odd":
        assert n % 4 != 0
    if name == "fe_broken":
        p3 = RC.case("fe:3")[1]
        assert n == len(p3) - 1 and n % 4 == 0 and nnz == int(p3[-1]) - 1
    if name == "components":
        assert n_components(n, p, c) >= 3
        assert (lens == 0).sum() >= 1
        assert ((lens == 1) & (c[np.minimum(p[:-1], nnz - 1)] == np.arange(n))).sum() >= 1, "no row holds only its diagonal"
        assert len(np.setdiff1d(np.arange(n), c)) == 1, "exactly one column is named by no row"
    if name == "upper":
        rows = np.repeat(np.arange(n), lens)
        # scrambled, so 'upper' is not visible in the indices: the pattern has no diagonal and no pair (i, j), (j, i)
        keys = set(zip(rows.tolist(), c.tolist()))
        assert all(r != q and (q, r) not in keys for r, q in keys)
        assert (lens == 0).sum() >= 5
    if name == "unsorted":
        unsorted = repeated = 0
        for r in range(n):
            row = c[p[r]:p[r + 1]]
            unsorted += bool((np.diff(row) < 0).any())
            repeated += len(np.unique(row)) < len(row)
        assert unsorted > n // 2 and repeated == n
    if name == "hub":
        assert n == 600 and lens.max() == 600 and (lens == 600).sum() == 1
        hub_col = int(np.bincount(c, minlength=n).argmax())
        assert np.bincount(c, minlength=n)[hub_col] == n     # column 0 of the unscrambled matrix: every row names it
    if name == "long:2500":
        assert n == 3000 and sorted(lens.tolist())[-2:] == [257, 2500] and sorted(lens.tolist())[-3] <= 3
    if name == "stride":
        assert (n + 63) // 64 > 4096 and n % 64 == 1          # the refresh kernel's grid is capped at 4096 groups of 64 rows
    if name == "powers":
        # None of the three sizes eligible would mean the one-launch form cannot be pinned on a twin: say so here and in profiles/NOTES.md
        assert RC.powers_size() in RC.POWERS_SIZES, "no size of POWERS_SIZES gives a relabelled pattern eligible for the one-launch powers step"
        assert n == RC.powers_size() and RC.probe_spmk(*RC.relabelled_pattern(p, c))
    if name == "sliced":
        assert RC.probe_sstream(*RC.relabelled_pattern(p, c)), "the relabelled pattern is not eligible for the sliced stream"


def test_every_family_of_the_table_is_listed():
    assert len(RC.NAMES) == len(set(RC.NAMES)) == 9 + 3 + 4 + 3 + 2 + 8
    assert set(RC.BLOCK) == set(RC.NAMES)
