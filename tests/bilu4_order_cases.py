"""What the tests of the ordered block ILU (mi_bilu4_create_ordered, mpk.bilu4(order="colour")) share: the colouring rule restated
in plain Python, the explicit permutation of a block matrix in numpy, the patterns, and the model's factor of every permuted
system (tests/bilu4_model.py, computed once per process).

THE RULE (include/mi355_spmv.h): greedy colouring of the symmetrised block graph (A + A^T, diagonal excluded), block rows in
ascending natural order, each taking the smallest colour no already-coloured neighbour holds; new numbering colour ascending, old
row number ascending inside a colour; perm[old] = new."""
import functools

import numpy as np

import bilu4_cases as C
import bilu4_model as M


def colour_model(nb, ptr, col, symmetrise=True):
    """(perm, colour): the rule, literally.  symmetrise=False colours the graph of the stored upper triangle alone (what the rule
    is NOT; the unsymmetric case exists to tell the two apart)."""
    nbrs = [set() for _ in range(nb)]
    for i in range(nb):
        for j in col[ptr[i]:ptr[i + 1]]:
            j = int(j)
            if j != i and (symmetrise or j > i):
                nbrs[i].add(j)
                nbrs[j].add(i)
    colour = [-1] * nb
    for i in range(nb):
        used = {colour[j] for j in nbrs[i] if colour[j] >= 0}
        c = 0
        while c in used:
            c += 1
        colour[i] = c
    order = sorted(range(nb), key=lambda i: (colour[i], i))
    perm = np.empty(nb, np.int32)
    perm[order] = np.arange(nb, dtype=np.int32)
    return perm, np.array(colour, np.int64)


def max_degree(nb, ptr, col):
    nbrs = [set() for _ in range(nb)]
    for i in range(nb):
        for j in col[ptr[i]:ptr[i + 1]]:
            if int(j) != i:
                nbrs[i].add(int(j))
                nbrs[int(j)].add(i)
    return max((len(s) for s in nbrs), default=0)


def permute(nb, ptr, col, val, perm):
    """B = Q A Q^T in numpy: (bptr, bcol, bval (nblocks, 4, 4), src) — row perm[i] of B is row i of A, its block columns renamed
    and sorted ascending; src[k] = the index in A of B's k-th block."""
    ptr, col = np.asarray(ptr), np.asarray(col)
    inv = np.empty(nb, np.int64)
    inv[np.asarray(perm)] = np.arange(nb)
    bptr, bcol, src = [0], [], []
    for n in range(nb):
        i = int(inv[n])
        ks = np.arange(ptr[i], ptr[i + 1])
        newc = np.asarray(perm)[col[ks]]
        o = np.argsort(newc, kind="stable")
        bcol.extend(newc[o].tolist())
        src.extend(ks[o].tolist())
        bptr.append(len(bcol))
    src = np.array(src, np.int64)
    bval = np.asarray(val, np.float64).reshape(-1, 4, 4)[src] if len(src) else np.zeros((0, 4, 4))
    return np.array(bptr, np.int32), np.array(bcol, np.int32), bval, src


def vec_in(b, perm):
    """b in the new numbering: b_int[perm[i]] = b[i], per block of four."""
    out = np.empty_like(np.asarray(b, np.float64)).reshape(-1, 4)
    out[np.asarray(perm)] = np.asarray(b, np.float64).reshape(-1, 4)
    return out.reshape(-1)


def vec_out(x_int, perm):
    """x in the caller's numbering: x[i] = x_int[perm[i]]."""
    return np.asarray(x_int, np.float64).reshape(-1, 4)[np.asarray(perm)].reshape(-1)


def unsymmetric():
    """Seven block rows whose stored pattern is NOT symmetric: blocks (2, 0), (4, 1), (6, 0) and (6, 2) have no mirror.  The upper
    triangle alone would leave rows 0, 2, 4, 6 without a link between them; the symmetrised graph links 0-2, 0-6, 2-6 and 1-4."""
    rows = [{0, 1}, {1, 3}, {0, 2, 3}, {3, 5}, {1, 4, 5}, {5}, {0, 2, 6}]
    return C._from_rows(rows, 51)


PATTERNS = ["fe:3", "fe:4", "chain", "arrow", "unsym"] + [f"random:{s}" for s in range(20)]


@functools.lru_cache(maxsize=None)
def matrix(name):
    return unsymmetric() if name == "unsym" else C.matrix(name)


def values(name, variant=0):
    if not variant:
        return np.asarray(matrix(name)[3], np.float64)
    if name == "unsym":  # C.new_values looks its matrix up by name: the same recipe on this file's own pattern
        nb, bp, bc, bv = matrix(name)
        rng = np.random.default_rng(77 + variant)
        v = np.array(bv, np.float64).reshape(-1, 4, 4) * rng.uniform(0.5, 1.5, (len(bc), 1, 1))
        for i in range(nb):
            k = bp[i] + list(bc[bp[i]:bp[i + 1]]).index(i)
            v[k] = np.asarray(bv).reshape(-1, 4, 4)[k] * 1.25
        return v.reshape(-1)
    return np.asarray(C.new_values(name, variant), np.float64)


@functools.lru_cache(maxsize=None)
def ordered(name):
    """(nb, perm, colour, bptr, bcol, src) of the pattern under the rule."""
    nb, bp, bc, _ = matrix(name)
    perm, colour = colour_model(nb, bp, bc)
    bptr, bcol, _, src = permute(nb, bp, bc, np.zeros(16 * len(bc)), perm)
    return nb, perm, colour, bptr, bcol, src


@functools.lru_cache(maxsize=None)
def permuted_values(name, variant=0):
    return values(name, variant).reshape(-1, 4, 4)[ordered(name)[5]]


@functools.lru_cache(maxsize=None)
def model_factor(name, fill, variant=0):
    """The model's factor (ptr, col, diag, val) of the explicitly permuted matrix."""
    nb, _, _, bptr, bcol, _ = ordered(name)
    return M.factor(nb, bptr, bcol, permuted_values(name, variant).reshape(-1), fill)


def model_solve(name, fill, b, variant=0):
    """The exact solve in the caller's numbering: permute b, the model's solve of the permuted system, un-permute."""
    nb, perm = ordered(name)[:2]
    return vec_out(M.solve(nb, *model_factor(name, fill, variant), vec_in(b, perm)), perm)
