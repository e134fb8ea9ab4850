"""The matrices the mi_bilu4_* tests share, and the model's factor of each (computed once per process: tests/bilu4_model.py
takes seconds per case).  A case is (name, nb, ptrow, indcol, coef, fill), blocks row-major."""
import functools

import numpy as np

import bilu4_model as M


def _fe(nx, permuted):
    from navierstokes_amd import synth
    p, c, v = synth.fe_matrix(nx)
    if permuted:
        p, c, v, _ = synth.permute_nodes(p, c, v, block=4)
    return synth.csr_to_bcsr4(p, c, v)


def _values(nb, ptr, col, seed):
    """Diagonally dominated random blocks: entries in [-1, 1), the diagonal of every diagonal block raised above its row's sum."""
    rng = np.random.default_rng(seed)
    val = rng.uniform(-1.0, 1.0, (len(col), 4, 4))
    for i in range(nb):
        k = ptr[i] + list(col[ptr[i]:ptr[i + 1]]).index(i)
        val[k][np.arange(4), np.arange(4)] = 4.0 * (ptr[i + 1] - ptr[i]) + 1.0 + rng.uniform(0, 1, 4)
    return val.reshape(-1)


def _from_rows(rows, seed):
    nb = len(rows)
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    col = np.array([c for r in rows for c in sorted(r)], np.int32)
    return nb, ptr, col, _values(nb, ptr, col, seed)


def chain(nb=150):
    return _from_rows([{j for j in (i - 1, i, i + 1) if 0 <= j < nb} for i in range(nb)], 11)


def block_diagonal(nb=150):
    return _from_rows([{i} for i in range(nb)], 12)


def arrow(nb=80):
    return _from_rows([({i, nb - 1} if i < nb - 1 else set(range(nb))) for i in range(nb)], 13)


def random_pattern(seed):
    rng = np.random.default_rng(1000 + seed)
    nb = int(rng.integers(1, 40))
    dens = rng.uniform(0.03, 0.3)
    rows = [set(np.nonzero(rng.uniform(size=nb) < dens)[0].tolist()) | {i} for i in range(nb)]
    return _from_rows(rows, 2000 + seed)


@functools.lru_cache(maxsize=None)
def matrix(name):
    kind, _, arg = name.partition(":")
    if kind in ("fe", "fe_perm"):
        bp, bc, bv = _fe(int(arg), kind == "fe_perm")
        return len(bp) - 1, bp, bc, bv
    if kind == "random":
        return random_pattern(int(arg))
    return {"chain": chain, "diag": block_diagonal, "arrow": arrow}[kind]()


FE_CASES = [(f"{kind}:{nx}", fill) for kind in ("fe", "fe_perm") for nx in (3, 6, 10) for fill in (0, 1, 2)]
SHAPE_CASES = [("chain", 0), ("chain", 2), ("diag", 0), ("arrow", 0), ("arrow", 1)]
RANDOM_CASES = [(f"random:{s}", s % 3) for s in range(100)]
ALL_CASES = FE_CASES + SHAPE_CASES + RANDOM_CASES


def case_id(c):
    return f"{c[0]}-fill{c[1]}"


@functools.lru_cache(maxsize=None)
def model_factor(name, fill, variant=0):
    """(ptr, col, diag, val) of the model, or the ZeroPivot it raised.  variant > 0: the values of new_values(name, variant)."""
    nb, bp, bc, bv = matrix(name)
    if variant:
        bv = new_values(name, variant)
    try:
        return M.factor(nb, bp, bc, bv, fill)
    except M.ZeroPivot as e:
        return e


def new_values(name, variant):
    """Other values on the same pattern (a Newton step): every block scaled by a seeded factor in [0.5, 1.5), its diagonal kept."""
    nb, bp, bc, bv = matrix(name)
    rng = np.random.default_rng(77 + variant)
    v = np.array(bv, np.float64).reshape(-1, 4, 4) * rng.uniform(0.5, 1.5, (len(bc), 1, 1))
    for i in range(nb):
        k = bp[i] + list(bc[bp[i]:bp[i + 1]]).index(i)
        v[k] = np.asarray(bv).reshape(-1, 4, 4)[k] * 1.25
    return v.reshape(-1)
