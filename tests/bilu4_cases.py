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


def layered(widths, extra, seed):
    """A structurally symmetric pattern whose dependency levels are prescribed: layer l holds widths[l] consecutive block rows;
    row r of layer l+1 is linked to row r mod widths[l] of layer l, and row r of layer l to row r mod widths[l+1] of layer l+1
    (so every row depends on the layer before it and is needed by the layer after it, and on nothing inside its own layer);
    every row of a layer l >= 2 gets `extra` seeded links to rows of layers < l-1 — far dependencies, which leave the levels
    alone.  At fill 0 the forward level sizes are `widths` and the backward ones `widths` reversed (asserted by the tests)."""
    first = np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)
    rows = [{i} for i in range(int(first[-1]))]

    def link(i, j):
        rows[i].add(int(j))
        rows[j].add(int(i))

    rng = np.random.default_rng(seed)
    for l in range(len(widths) - 1):
        for r in range(widths[l + 1]):
            link(first[l + 1] + r, first[l] + r % widths[l])
        for r in range(widths[l]):
            link(first[l] + r, first[l + 1] + r % widths[l + 1])
    for l in range(2, len(widths)):
        for r in range(widths[l]):
            for j in rng.integers(0, first[l - 1], extra):
                link(first[l] + r, j)
    return _from_rows(rows, seed)


LIMITS_WIDTHS = (1, 63, 64, 65, 1, 1, 128, 129, 2, 63, 64, 200, 1)
ALTERNATING_WIDTHS = (63, 64) * 24
FOLD_DEEP_LAYERS = 252


def fold_widths(layers):
    """1 + 5 i mod 63: every width from 1 to 63 once per 63 layers, neighbours far apart in width."""
    return tuple(1 + (5 * i) % 63 for i in range(layers))


LAYERED = {  # name -> (widths, extra, seed)
    "limits:0": (LIMITS_WIDTHS, 0, 31),
    "limits:3": (LIMITS_WIDTHS, 3, 32),
    "fold_deep": (fold_widths(FOLD_DEEP_LAYERS), 2, 33),
    "alternating": (ALTERNATING_WIDTHS, 1, 34),
}
FOLD_HUGE = (fold_widths(1500), 1, 35)  # 48 006 block rows: too large for the model's factorisation (tests/test_gpu_bilu4_limits.py)


@functools.lru_cache(maxsize=None)
def matrix(name):
    kind, _, arg = name.partition(":")
    if kind in ("fe", "fe_perm"):
        bp, bc, bv = _fe(int(arg), kind == "fe_perm")
        return len(bp) - 1, bp, bc, bv
    if kind == "random":
        return random_pattern(int(arg))
    if name in LAYERED:
        return layered(*LAYERED[name])
    if kind == "wide":
        return _from_rows([{i} for i in range(int(arg))], 40 + int(arg))
    return {"chain": chain, "diag": block_diagonal, "arrow": arrow}[kind]()


FE_CASES = [(f"{kind}:{nx}", fill) for kind in ("fe", "fe_perm") for nx in (3, 6, 10) for fill in (0, 1, 2)]
SHAPE_CASES = [("chain", 0), ("chain", 2), ("diag", 0), ("arrow", 0), ("arrow", 1)]
RANDOM_CASES = [(f"random:{s}", s % 3) for s in range(100)]
LAYERED_CASES = [(name, 0) for name in LAYERED]  # fill 0 only: fill above 0 can change the levels
WIDE_CASES = [("wide:63", 0), ("wide:64", 0), ("wide:65", 0)]  # one level: the widest that folds, exactly one workgroup, one row over
ALL_CASES = FE_CASES + SHAPE_CASES + RANDOM_CASES + LAYERED_CASES + WIDE_CASES


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


def layered_widths(name):
    return LAYERED[name][0] if name in LAYERED else (int(name.partition(":")[2]),)


def assert_layered_levels(name, fwd_sizes, bwd_sizes):
    """The property the layered and wide cases exist for: the forward levels are the layers, the backward levels the layers
    reversed.  Every test that relies on a prescribed width calls this on the sizes it was given."""
    w = list(layered_widths(name))
    assert list(fwd_sizes) == w, (name, list(fwd_sizes)[:20], w[:20])
    assert list(bwd_sizes) == w[::-1], (name, list(bwd_sizes)[:20], w[::-1][:20])
