"""Why the library has a classical Gram-Schmidt Arnoldi basis with two passes (mi_krylov_basis_cgs_dev, passes = 2), on the CPU:
the oracle's bitwise models replay both orthogonalisations on the project's own matrix families, whose spectrum is clustered at 1,
so that Krylov vectors become dependent quickly.

- _replay_krylov_cgs is what the device computes, composed only of models the oracle already has: O.spmv, O.tree_dot (every dot
  of a pass against the same vector), successive O.axpy(-d_j, v_j, .), one numpy add per Hessenberg entry, O.tree_norm2 and IEEE
  division.  tests/test_gpu_multi_blas1.py holds the device to it bit for bit.
- With two passes max |V^T V - I| stays at a few ulps (bound 1e-14, about 45 eps: one order over the 2.2e-16 .. 8.9e-16 the
  model gives, fourteen under what the sweep leaves).
- The sequential sweep of mi_krylov_basis_dev(orth = 1) (tests/test_gpu_reductions._replay_krylov) ends more than 0.1 away from
  orthonormal on the two large cases."""
import numpy as np
import pytest

from navierstokes_amd import synth
from oracle import oracle as O
from test_gpu_reductions import _replay_krylov

# (matrix family, n, s): the cases of DESIGN.md 4.4
CASES = [("s15", 20_001, 30), ("svar", 20_001, 30), ("s15", 3_001, 12)]


def cgs_model(basis, y, passes):
    """(y_new, h, norm) of mi_cgs_dev: per pass every dot against the same y, then the axpy chain in basis order."""
    y = np.array(y, dtype=np.float64)
    h = np.zeros(len(basis))
    for p in range(passes):
        d = np.array([O.tree_dot(y, v) for v in basis], dtype=np.float64).reshape(len(basis))
        for j, v in enumerate(basis):
            y = O.axpy(-d[j], v, y)
        h = d if p == 0 else h + d
    return y, h, O.tree_norm2(y)


def _replay_krylov_cgs(p, c, v, v0, s, passes):
    n = len(v0)
    V = np.zeros((s + 1, n))
    H = np.zeros((s, s + 2))
    nrm0 = O.tree_norm2(v0)
    V[0] = v0 / nrm0
    for k in range(s):
        w, h, nr = cgs_model(V[:k + 1], O.spmv(p, c, v, V[k]), passes)
        V[k + 1] = w / nr
        H[k, :k + 1] = h
        H[k, k + 1] = nr
    return V, H, nrm0


def loss(V):
    return float(np.max(np.abs(V @ V.T - np.eye(len(V)))))


@pytest.mark.parametrize("kind,n,s", CASES)
def test_two_passes_keep_the_basis_orthonormal(kind, n, s):
    p, c, v = synth.rows(kind, n)
    V, H, nrm0 = _replay_krylov_cgs(p, c, v, synth.x_sin(0, n), s, 2)
    e = loss(V)
    print(f"{kind} n={n} s={s}: max |V^T V - I| = {e:.3e} (CGS2)")
    assert e <= 1e-14, (kind, n, s, e)
    assert np.all(H[np.arange(s), np.arange(s) + 1] > 0) and nrm0 > 0


@pytest.mark.parametrize("kind,n,s", CASES[:2])
def test_the_sweep_loses_orthogonality_there(kind, n, s):
    p, c, v = synth.rows(kind, n)
    V, _, _ = _replay_krylov(p, c, v, synth.x_sin(0, n), s)
    e = loss(V)
    print(f"{kind} n={n} s={s}: max |V^T V - I| = {e:.3e} (sweep)")
    assert e > 0.1, (kind, n, s, e)


def test_one_pass_is_the_first_pass_of_two():
    """passes = 1 and passes = 2 share their first pass: h of one pass is the first term of the two-pass sum, and with an
    orthonormal basis the second pass changes h by a rounding-sized correction only."""
    rng = np.random.default_rng(3)
    n, m = 3001, 5
    Q = np.linalg.qr(rng.standard_normal((n, m)))[0].T.copy()
    y0 = rng.standard_normal(n)
    y1, h1, n1 = cgs_model(Q, y0, 1)
    y2, h2, n2 = cgs_model(Q, y0, 2)
    d2 = np.array([O.tree_dot(y1, q) for q in Q])
    assert np.array_equal(h2, h1 + d2)
    # Q is orthonormal to ~1e-15, so what the first pass leaves along it is ~1e-15 ||y0||: three orders under this bound
    assert np.max(np.abs(h2 - h1)) <= 1e-12 * np.linalg.norm(y0)
    assert abs(n2 - n1) <= 1e-12 * n1
