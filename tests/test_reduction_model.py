"""The oracle's bitwise models of the library's device reduction trees (oracle/cpu_ref.c, "BITWISE MODELS"), checked on the CPU:

- against an independent pure-Python restatement of each tree that rounds every fma exactly once (through Fraction);
- for teeth: on adversarial data the model differs from the trees a subtly wrong kernel would build (the sequential fma chain,
  the stride-256 lane order the 8-byte-aligned branch of reduce_stage1 used to take, a reassociated block_sum), so a bitwise
  check against it catches them;
- against the exact dot: |model - exact| <= gamma_h * sum |a_i b_i| with h the tree's depth.

tests/test_gpu_reductions.py holds the device to these models bit for bit.  The data generators below serve both modules."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as O

WG = 256
MAXP = 1024
# every regime of red_geometry and of the switch to non-temporal loads (2 000 000); the GPU module adds one n above 2^28
GPU_SIZES = (0, 1, 2, 511, 512, 513, 524_287, 524_288, 524_289, 1_048_577, 1_999_999, 2_000_000, 5_000_000)
MODEL_SIZES = (0, 1, 2, 255, 256, 511, 512, 513, 1023, 1025, 3001)


# ------------------------------------------------------------------------------------------------------------------- data

def data_uniform(n, rng):
    return rng.uniform(0.5, 1.0, n), rng.uniform(0.5, 1.0, n)


def data_mixed(n, rng):
    """Mixed signs, magnitudes 2^k with k spread over [-20, 20]."""
    def one():
        return rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-20, 21, n))
    return one(), one()


def data_cancel(n, rng):
    """Heavy cancellation: products come in pairs that cancel to ~1e-12 of their size, the pairs scattered, so the sum is about
    1e-12 of the sum of absolute values."""
    a, b = data_mixed(n, rng)
    h = n // 2
    if h:
        a[h:2 * h] = a[:h]
        b[h:2 * h] = -b[:h] * (1.0 + 1e-12 * rng.standard_normal(h))
        perm = rng.permutation(n)
        a, b = a[perm], b[perm]
    return a, b


def data_negzero(n, rng):
    """Every product is -0.0 (the tree's +0.0 start decides the sign of the result)."""
    a = rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 2.0, n)
    b = np.copysign(np.zeros(n), -a)
    return a, b


DATA = {"uniform": data_uniform, "mixed": data_mixed, "cancel": data_cancel, "negzero": data_negzero}


# ------------------------------------------------------------------------------- independent restatement (exact fma)

def fma(a, b, c):
    """a*b + c rounded once (IEEE round to nearest even, signed zeros included), for finite operands."""
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        prod_neg = (math.copysign(1.0, a) * math.copysign(1.0, b)) < 0
        if (a == 0 or b == 0) and c == 0 and prod_neg and math.copysign(1.0, c) < 0:
            return -0.0
        return 0.0
    return float(r)  # int / int true division: correctly rounded


def geometry(n):
    q = 2 * WG
    s = -(-n // MAXP)
    s = max(q, -(-s // q) * q)
    return max(1, -(-n // s)), s


def wave(v):
    w = list(v)
    off = 32
    while off:
        for lane in range(off):
            w[lane] = w[lane] + w[lane + off]
        off >>= 1
    return w[0]


def block(v, reassoc=False):
    w = [wave(v[64 * k:64 * k + 64]) for k in range(4)]
    return w[0] + (w[1] + (w[2] + w[3])) if reassoc else ((w[0] + w[1]) + w[2]) + w[3]


def lane_orders(lo, hi, order):
    """Element indices of each thread's chain in one segment: 'pair' (reduce_stage1) or 'stride' (the old 8-byte branch)."""
    lanes = [[] for _ in range(WG)]
    if order == "pair":
        for t in range(WG):
            i = lo + 2 * t
            while i + 1 < hi:
                lanes[t] += [i, i + 1]
                i += 2 * WG
        if (hi - lo) & 1:
            lanes[0].append(hi - 1)
    else:
        for t in range(WG):
            lanes[t] = list(range(lo + t, hi, WG))
    return lanes


def stage1(a, b, mode=0, order="pair", reassoc=False):
    n = len(a)
    np_, seg = geometry(n)
    p, p2 = [], []
    for g in range(np_):
        lo, hi = g * seg, min(g * seg + seg, n)
        s, s2 = [], []
        for idx in lane_orders(lo, hi, order):
            acc = acc2 = 0.0
            for i in idx:
                if mode == 0:
                    acc = fma(a[i], b[i], acc)
                else:
                    d = a[i] - b[i]
                    acc = fma(d, d, acc)
                    acc2 = fma(a[i], a[i], acc2)
            s.append(acc)
            s2.append(acc2)
        p.append(block(s, reassoc))
        p2.append(block(s2, reassoc))
    return p, p2


def finish(p, reassoc=False):
    s = []
    for t in range(WG):
        acc = 0.0
        for i in range(t, len(p), WG):
            acc = acc + p[i]
        s.append(acc)
    return block(s, reassoc)


def py_dot(a, b, order="pair", reassoc=False):
    return finish(stage1(a, b, 0, order, reassoc)[0], reassoc)


def py_rel_error(a, b):
    p, p2 = stage1(a, b, 1)
    return math.sqrt(finish(p)) / math.sqrt(finish(p2))


def py_mgs(basis, y):
    n, m = len(y), len(basis)
    y = list(y)
    if n == 0:
        return y, [0.0] * m
    np_, seg = geometry(n)
    part = stage1(y, basis[0])[0]
    dots = []
    for j in range(m):
        d = finish(part)
        dots.append(d)
        v, vn = basis[j], (basis[j + 1] if j + 1 < m else None)
        nxt = []
        for g in range(np_):
            lo, hi = g * seg, min(g * seg + seg, n)
            s = []
            for t in range(WG):
                acc = 0.0
                for i in range(lo + t, hi, WG):
                    y[i] = fma(-d, v[i], y[i])
                    if vn is not None:
                        acc = fma(y[i], vn[i], acc)
                s.append(acc)
            nxt.append(block(s))
        part = nxt
    return y, dots


def py_ring_partials(layout, b, y):
    T = layout["threads"]
    first, row0, rows = layout["run_first_block"], layout["block_row0"], layout["block_rows"]
    out = []
    for g in range(len(first) - 1):
        dacc = [0.0] * T
        for blk in range(first[g], first[g + 1]):
            for t in range(min(rows[blk], T)):
                r = row0[blk] + t
                dacc[t] = fma(b[r], y[r], dacc[t])
        acc = wave(dacc[:64])
        for w in range(1, T // 64):
            acc = acc + wave(dacc[64 * w:64 * w + 64])
        out.append(acc)
    return out


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def same(got, want):
    return np.array_equal(bits(got), bits(want))


# ------------------------------------------------------------------------------------------------------------------ tests

@pytest.mark.parametrize("n", MODEL_SIZES)
@pytest.mark.parametrize("kind", ["mixed", "cancel", "negzero"])
def test_stage_trees_equal_an_exact_fma_restatement(n, kind):
    rng = np.random.default_rng(n * 7 + len(kind))
    a, b = DATA[kind](n, rng)
    assert O.tree_geometry(n) == geometry(n)
    al, bl = a.tolist(), b.tolist()
    pm, _ = O.tree_partials(a, b, 0)
    pp, _ = stage1(al, bl)
    assert same(pm, pp), (n, kind, "stage-1 partials")
    assert same(O.tree_dot(a, b), py_dot(al, bl)), (n, kind, "dot")
    if n:
        assert same(O.tree_norm2(a), math.sqrt(py_dot(al, al))), (n, kind, "norm2")
        t = (a * (1 + 1e-9 * rng.standard_normal(n))).tolist()
        p1, p2 = O.tree_partials(a, t, 1)
        q1, q2 = stage1(al, t, 1)
        assert same(p1, q1) and same(p2, q2), (n, kind, "MODE 1 partials")
        assert same(O.tree_rel_error(a, t), py_rel_error(al, t)), (n, kind, "rel_error")
    beta, x3 = O.tree_orthogonalize(a, b, 1e-8)
    assert same(beta, py_dot(al, bl))
    nab = -(1e-8 * beta)
    assert same(x3, [fma(nab, ai, bi) for ai, bi in zip(al, bl)]), (n, kind, "ortho update")


def test_finish_keeps_the_sign_of_zero_as_the_device_does():
    """0.0 + (-0.0) is +0.0: every lane of the finishing tree starts from +0.0."""
    assert same(O.tree_finish(np.array([-0.0])), 0.0)
    assert same(O.tree_finish(np.full(1024, -0.0)), 0.0)
    assert same(O.tree_dot(np.array([-1.0]), np.array([0.0])), 0.0)
    assert same(O.tree_finish(np.array([-1.5, 2.0])), 0.5)


@pytest.mark.parametrize("n", [1, 2, 511, 513, 1025, 3001])
@pytest.mark.parametrize("m", [1, 2, 3])
def test_gram_schmidt_sweep_equals_an_exact_fma_restatement(n, m):
    rng = np.random.default_rng(100 + n + m)
    basis = np.stack([data_mixed(n, rng)[0] for _ in range(m)])
    y = data_mixed(n, rng)[1]
    ym, dm = O.tree_mgs(basis, y)
    yp, dp = py_mgs([r.tolist() for r in basis], y.tolist())
    assert same(dm, dp), (n, m, dm, dp)
    assert same(ym, yp), (n, m)


def test_ring_epilogue_equals_an_exact_fma_restatement():
    """A hand-built layout: uneven blocks, a block shorter than the wave, an empty run, runs of one and of several blocks."""
    rng = np.random.default_rng(5)
    rows = np.array([256, 256, 17, 256, 100, 64, 65, 1, 256, 200], np.int32)
    row0 = np.concatenate([[0], np.cumsum(rows)[:-1]]).astype(np.int32)
    first = np.array([0, 3, 3, 4, 7, 10], np.int32)
    layout = dict(threads=256, run_first_block=first, block_row0=row0, block_rows=rows)
    n = int(rows.sum())
    b, y = data_mixed(n, rng)
    pm = O.tree_ring_partials(layout, b, y)
    pp = py_ring_partials(layout, b.tolist(), y.tolist())
    assert same(pm, pp)
    assert same(pm[1], 0.0)
    assert same(O.tree_ring_dot(layout, b, y), finish(pp))
    assert O.tree_rank_sum(np.array([1.0, 1e-17, -1.0])) == (0.0 + 1.0 + 1e-17) - 1.0


def test_the_comparison_has_teeth():
    """On adversarial data the model differs from each tree a subtly wrong kernel would build, on most cases."""
    cases = [(kind, n, seed) for kind in ("mixed", "cancel") for n in (513, 1025, 3001) for seed in range(3)]
    differ = {"sequential": 0, "stride-256 lanes": 0, "reassociated block_sum": 0}
    for kind, n, seed in cases:
        a, b = DATA[kind](n, np.random.default_rng(1000 * seed + n))
        al, bl = a.tolist(), b.tolist()
        model = O.tree_dot(a, b)
        seq = 0.0
        for x, y in zip(al, bl):
            seq = fma(x, y, seq)
        assert same(seq, O.dot(a, b))
        differ["sequential"] += not same(model, seq)
        differ["stride-256 lanes"] += not same(model, py_dot(al, bl, order="stride"))
        differ["reassociated block_sum"] += not same(model, py_dot(al, bl, reassoc=True))
    for what, k in differ.items():
        assert 2 * k > len(cases), (what, k, len(cases))  # most cases


def depth(n):
    """Roundings on the longest path from a product to the result: the longest lane chain, the wave (6), the block (3), the
    finishing lane chain, its wave and block (9)."""
    np_, seg = geometry(n)
    return 2 * (-(-seg // (2 * WG))) + 1 + 6 + 3 + (-(-np_ // WG)) + 9


@pytest.mark.parametrize("n", GPU_SIZES)
@pytest.mark.parametrize("kind", ["uniform", "mixed", "cancel"])
def test_model_is_within_gamma_h_of_the_exact_dot(n, kind):
    a, b = DATA[kind](n, np.random.default_rng(n + 3))
    model = O.tree_dot(a, b)
    p, e = O.two_products(a, b)
    exact = math.fsum(np.concatenate([p, e]).tolist())
    total = math.fsum(np.abs(p).tolist()) * (1 + 2.0 ** -52)
    u = 2.0 ** -53
    h = depth(n)
    gamma = h * u / (1 - h * u)
    assert abs(model - exact) <= gamma * total, (n, kind, h, model, exact, total)
