"""The CPU oracle against the REAL reference object code (oracle/_ref), on
larger seeded matrices than the committed goldens.  What the reference's
object code returned on every case below is recorded in
tests/golden/ref_digests.json (conftest.digest of each output; regenerate with
tests/golden/make_golden.py where oracle/_ref is built), so the comparison is
bitwise and needs nothing outside the repository."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, digest
from navierstokes_amd import synth
from oracle import oracle as O

SPMV_CASES = [("s15", 30000, 2000), ("svar", 20000, 500), ("sfe", 12000, 400)]
POWERS_CASES = [("s15", 5000, 300), ("svar", 4000, 100), ("sfe", 2000, 100)]
LAYER_CASES = [("s15", 3000, 200), ("svar", 2500, 80), ("sfe", 1200, 60)]
COO_NROWS = (16, 33, 64)
BLAS1_LENGTHS = list(range(1, 13)) + [255, 1000, 4099]


def coo_inputs():
    rng = np.random.default_rng(7)
    for nrow in COO_NROWS:
        m = nrow * 9
        ir = rng.integers(0, nrow, m).astype(np.int32)
        jc = rng.integers(0, nrow, m).astype(np.int32)
        va = rng.uniform(-1, 1, m)
        yield nrow, ir, jc, va


def blas1_inputs():
    rng = np.random.default_rng(11)
    for n in BLAS1_LENGTHS:
        b, x1 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
        B = rng.uniform(-1, 1, (5, n))
        yield n, b, x1, B


def case_id(*parts):
    return "/".join(str(p) for p in parts)


@pytest.fixture(scope="module")
def ref():
    with open(os.path.join(GOLDEN, "ref_digests.json")) as f:
        return json.load(f)


def assert_ref(ref, a, key):
    assert key in ref, f"{key}: no recorded reference output"
    assert digest(a) == ref[key], f"{key}: differs bitwise from the reference's recorded output (shape {np.shape(a)})"


@pytest.mark.parametrize("kind,n,w", SPMV_CASES)
def test_spmv_all_variants(ref, kind, n, w):
    p, c, v = synth.rows(kind, n, w=w)
    x = synth.x_sin(0, n)
    y = O.spmv(p, c, v, x, "fma")
    assert_ref(ref, y, case_id("spmv", kind, n, w, "opt"))
    assert_ref(ref, y, case_id("spmv", kind, n, w, "fma"))
    y87 = O.spmv(p, c, v, x, "x87")
    assert_ref(ref, y87, case_id("spmv", kind, n, w, "scalar"))
    assert O.rel_error(y87, y) <= 1e-15  # (y87 is bit for bit the reference's scalar output, checked just above)


@pytest.mark.parametrize("kind,n,w", POWERS_CASES)
def test_powers(ref, kind, n, w):
    p, c, v = synth.rows(kind, n, w=w)
    x = synth.x_ones(n)
    key = lambda name: case_id("powers", kind, n, w, name)
    assert_ref(ref, O.gen_layer1(p, c), key("layer1"))
    y, z = O.spm2v_fused(p, c, v, x)
    assert_ref(ref, y, key("spm2v_opt_y"))
    assert_ref(ref, z, key("spm2v_opt_z"))
    assert_ref(ref, O.spmkv_fused(3, p, c, v, x, "fma"), key("powers3"))
    assert_ref(ref, O.spmkv_fused(4, p, c, v, x, "x87"), key("powers4"))
    assert_ref(ref, O.spmkv_fused(2, p, c, v, x, "x87"), key("powers2"))


def test_coo_rules_random(ref):
    for nrow, ir, jc, va in coo_inputs():
        for name, arrs in (("csr", O.coo2csr(nrow, ir, jc, va)), ("bcsr4", O.coo2bcsr4(nrow, ir, jc, va))):
            for i, a in enumerate(arrs):
                assert_ref(ref, a, case_id("coo", nrow, name, i))


def test_blas1_random_lengths(ref):
    """orthogonalize (3-vector and in-place) and orthonormalize_against_basis, every tail length."""
    for n, b, x1, B in blas1_inputs():
        assert_ref(ref, O.orthogonalize(b, x1, 0.37)[1], case_id("blas1", n, "orthogonalize3"))
        assert_ref(ref, O.orthogonalize_inplace(b, x1, 0.37)[1], case_id("blas1", n, "orthogonalize_inplace"))
        assert_ref(ref, O.mgs(B, x1)[0], case_id("blas1", n, "mgs"))


@pytest.mark.parametrize("kind,n,w", LAYER_CASES)
def test_layer_tables_and_avx2_powers(ref, kind, n, w):
    p, c, v = synth.rows(kind, n, w=w)
    a = O.gen_layers(p, c)
    for name in sorted(a):
        assert_ref(ref, a[name], case_id("layers", kind, n, w, name))
    assert case_id("layers", kind, n, w, "keys") in ref and sorted(a) == ref[case_id("layers", kind, n, w, "keys")]
    x = synth.x_sin(0, n)
    assert_ref(ref, O.spmkv_fused(4, p, c, v, x, "avx2row"), case_id("layers", kind, n, w, "spm4v_avx2"))
