"""What tests/test_ref_baij.py (CPU, against the reference's compiled PETSc kernels), tests/golden/make_golden.py (which records
those kernels' outputs in tests/golden/ref_baij.npz) and tests/test_gpu_petsc_seam.py (GPU, against the recording) share: the
cases, their right-hand sides, the extended-precision yardsticks and the error measure.  Plain numpy; nothing here needs the
reference or a GPU."""
import functools

import numpy as np

import bilu4_cases as C
import bilu4_model as M
from test_gpu_bilu4 import _rhs

# (matrix of tests/bilu4_cases.py, fill): fill 4 is the reference's PCFactorSetLevels
SOLVE_CASES = ([("fe:3", 0), ("fe:3", 4), ("fe:6", 0), ("fe:6", 1), ("fe_perm:6", 1), ("limits:0", 0), ("arrow", 0), ("chain", 0), ("diag", 0),
                ("wide:65", 0)] + [(f"random:{s}", s % 3) for s in range(10)])
EMPTY_ROWS = "empty_rows"  # products only
TILED = "fe:7"             # products only: 6238 blocks, the smallest FE matrix for which a handle builds its tiled copy (4096 blocks up)
PRODUCT_MATRICES = list(dict.fromkeys(name for name, _ in SOLVE_CASES)) + [EMPTY_ROWS, TILED]
RHS_KINDS = ("ones", "random", "edge")
SPMM_WIDTHS = (1, 3, 4, 5, 8)  # 3 and 5: the s_remaining tail of MatMatMult_SeqBAIJ_4_AVX2 alone and behind a full group of four
GOLDEN_SKIP = ("limits:0",)    # 782 block rows: left out of the recording, kept in the CPU test


def case_id(c):
    return f"{c[0]}-fill{c[1]}"


def rhs(nb):
    """{kind: b}: ones, seeded random, and the IEEE edge vector of tests/test_gpu_bilu4.py."""
    r = _rhs(nb)
    return {k: r[k] for k in RHS_KINDS}


def empty_rows_matrix():
    """A square pattern with empty block rows at the start (0, 1), in the middle (9, 10, 11, 20) and at the end (37, 38, 39):
    what PETSc's compressed-row view exists for.  (nb, ptrow, indcol, coef), blocks row-major."""
    nb = 40
    empty = {0, 1, 9, 10, 11, 20, 37, 38, 39}
    rng = np.random.default_rng(4040)
    rows = [set() if i in empty else set(rng.choice(nb, size=int(rng.integers(1, 9)), replace=False).tolist()) for i in range(nb)]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    col = np.array([c for r in rows for c in sorted(r)], np.int32)
    return nb, ptr, col, rng.uniform(-1.0, 1.0, 16 * len(col))


@functools.lru_cache(maxsize=None)
def matrix(name):
    """(nb, ptrow, indcol, coef) of a product case, blocks row-major."""
    return empty_rows_matrix() if name == EMPTY_ROWS else C.matrix(name)


def product_x(name, s=None):
    """The seeded x of a product case; s: the (s, n) vectors of the multi-vector product."""
    nb = matrix(name)[0]
    rng = np.random.default_rng(900 + 17 * PRODUCT_MATRICES.index(name) + (0 if s is None else s))
    return rng.uniform(-1.0, 1.0, 4 * nb if s is None else (s, 4 * nb))


def to_csr(nb, bp, bc, bv):
    """The same matrix as scalar CSR (every entry of every block kept, zeros too): what the AIJ products take."""
    bp, bc = np.asarray(bp, np.int64), np.asarray(bc, np.int64)
    blk = np.asarray(bv, np.float64).reshape(-1, 4, 4)
    ptr, col, val = [0], [], []
    for i in range(nb):
        for r in range(4):
            for k in range(bp[i], bp[i + 1]):
                col.extend(range(4 * bc[k], 4 * bc[k] + 4))
                val.extend(blk[k][r])
            ptr.append(len(col))
    return np.array(ptr, np.int32), np.array(col, np.int32), np.array(val, np.float64)


# ------------------------------------------------------------------ yardsticks in extended precision

def err(x, x_ld):
    """max|x - x_ld| / max|x_ld|, in extended precision."""
    x_ld = np.asarray(x_ld, np.longdouble)
    with np.errstate(all="ignore"):
        return float(np.abs(np.asarray(x, np.longdouble) - x_ld).max() / np.abs(x_ld).max())


def solve_ld(nb, ptr, col, diag, val, b):
    """x = U^-1 L^-1 b in np.longdouble over the same (double) factor values: forward substitution with the unit lower triangle of
    multipliers, backward substitution with U, the stored inverse of the diagonal block applied last."""
    v = np.asarray(val, np.float64).reshape(-1, 4, 4).astype(np.longdouble)
    t = np.asarray(b, np.float64).astype(np.longdouble).reshape(nb, 4).copy()
    with np.errstate(all="ignore"):
        for i in range(nb):
            s = t[i].copy()
            for k in range(ptr[i], diag[i]):
                s -= v[k] @ t[col[k]]
            t[i] = s
        for i in range(nb - 1, -1, -1):
            s = t[i].copy()
            for k in range(diag[i] + 1, ptr[i + 1]):
                s -= v[k] @ t[col[k]]
            t[i] = v[diag[i]] @ s
    return t.reshape(-1)


def mult_ld(nb, bp, bc, bv, x):
    """y = A x in np.longdouble."""
    blk = np.asarray(bv, np.float64).reshape(-1, 4, 4).astype(np.longdouble)
    xl = np.asarray(x, np.float64).astype(np.longdouble).reshape(-1, 4)
    y = np.zeros((nb, 4), np.longdouble)
    prod = np.einsum("krc,kc->kr", blk, xl[np.asarray(bc, np.int64)]) if len(bc) else np.zeros((0, 4), np.longdouble)
    np.add.at(y, np.repeat(np.arange(nb), np.diff(bp)), prod)
    return y.reshape(-1)


# ------------------------------------------------------------------ the association of MatMult_SeqBAIJ_4_AVX2

def avx2_mult_model(nb, bp, bc, bv, x):
    """src/kernels/baij4_avx2.c:39-65 in numpy: per block row four accumulators of four lanes, one per block COLUMN —
    sum_c = fma(column c of the block, x[4 j + c], sum_c) over the row's blocks in storage order — then (sum0 + sum1) + (sum2 + sum3).
    bv: row-major blocks (blk[k][:, c] is the column the kernel loads from the column-major bytes)."""
    bp, bc = np.asarray(bp, np.int64), np.asarray(bc, np.int64)
    blk = np.asarray(bv, np.float64).reshape(-1, 4, 4)
    xb = np.asarray(x, np.float64).reshape(-1, 4)
    acc = np.zeros((nb, 4, 4))  # [row, c, lane]
    lens = np.diff(bp)
    for step in range(int(lens.max()) if nb else 0):
        live = np.nonzero(lens > step)[0]
        k = bp[live] + step
        acc[live] = M.fma_vec(blk[k].transpose(0, 2, 1), xb[bc[k]][:, :, None], acc[live])
    with np.errstate(all="ignore"):
        return ((acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])).reshape(-1)


# ------------------------------------------------------------------ the recording, tests/golden/ref_baij.npz
# Vectors that agree with another one to a few units in the last place are kept as the int64 difference of their bit patterns from
# it (exact, and it deflates to almost nothing); an extended-precision vector as a float64 pair hi + lo (exact: 64 bits of mantissa).

def pack_ulps(a, base):
    return np.ascontiguousarray(a, np.float64).view(np.int64) - np.ascontiguousarray(base, np.float64).view(np.int64)


def unpack_ulps(d, base):
    return (np.ascontiguousarray(base, np.float64).view(np.int64) + d).view(np.float64)


def split_ld(x_ld):
    hi = np.asarray(x_ld, np.longdouble).astype(np.float64)
    with np.errstate(all="ignore"):
        lo = (np.asarray(x_ld, np.longdouble) - hi.astype(np.longdouble)).astype(np.float64)
    return hi, np.where(np.isfinite(hi), lo, 0.0)


def solve_key(case, kind, what):
    return f"solve__{case_id(case)}__{kind}__{what}"


def pack_solve(case, kind, d):
    """The npz entries of one right-hand side of solve_record (tests/test_ref_baij.py)."""
    hi, lo = split_ld(d["x_ld"])
    out = {"x_model": d["x_model"], "d_scalar": pack_ulps(d["x_scalar"], d["x_model"]), "d_avx2": pack_ulps(d["x_avx2"], d["x_model"]),
           "d_ld_hi": pack_ulps(hi, d["x_model"]), "ld_lo": lo, "e": np.array([d["e_scalar"], d["e_avx2"], d["e_model"]])}
    return {solve_key(case, kind, k): v for k, v in out.items()}


def load_solve(g, case, kind):
    """dict(x_model, x_scalar, x_avx2, x_ld, e_scalar, e_avx2, e_model) of a recorded right-hand side; g: the opened npz."""
    get = lambda what: g[solve_key(case, kind, what)]
    xm = get("x_model")
    e = get("e")
    x_ld = unpack_ulps(get("d_ld_hi"), xm).astype(np.longdouble) + get("ld_lo").astype(np.longdouble)
    return dict(x_model=xm, x_scalar=unpack_ulps(get("d_scalar"), xm), x_avx2=unpack_ulps(get("d_avx2"), xm), x_ld=x_ld,
                e_scalar=float(e[0]), e_avx2=float(e[1]), e_model=float(e[2]))


SPMM_GOLDEN = ("fe:3", EMPTY_ROWS) + tuple(f"random:{s}" for s in range(10))  # the multi-vector recordings (21 vectors a matrix)


def pack_product(name, d):
    out = {f"product__{name}__y_fma": d["y_fma"], f"product__{name}__d_avx2": pack_ulps(d["y_avx2"], d["y_fma"]),
           f"product__{name}__d_mad": pack_ulps(d["y_mad"], d["y_fma"])}
    if name in SPMM_GOLDEN:
        for s, (_, Y) in d["spmm"].items():
            out[f"product__{name}__spmm{s}"] = Y
    return out


def load_product(g, name):
    """dict(y_fma, y_avx2, y_mad, spmm={s: Y}) of a recorded matrix (spmm only for SPMM_GOLDEN)."""
    y = g[f"product__{name}__y_fma"]
    d = dict(y_fma=y, y_avx2=unpack_ulps(g[f"product__{name}__d_avx2"], y), y_mad=unpack_ulps(g[f"product__{name}__d_mad"], y), spmm={})
    if name in SPMM_GOLDEN:
        d["spmm"] = {s: g[f"product__{name}__spmm{s}"] for s in SPMM_WIDTHS}
    return d
