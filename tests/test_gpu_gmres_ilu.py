"""The preconditioner at work: GMRES(30) on fe_matrix(10) with and without M = bilu4(fill = 0).  Bounds from a CPU run of the same
problem (scipy GMRES(30), 60 iterations: true relative residual 8e-15 with a block ILU(0), 8e-4 without; scipy preconditions from
the left, mpk.GMRES from the right, hence six and two orders of magnitude of room)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _true_residual(bp, bc, bv, x, b):
    blocks = bv.reshape(-1, 4, 4)
    xb = x.reshape(-1, 4)
    y = np.zeros_like(xb)
    rows = np.repeat(np.arange(len(bp) - 1), np.diff(bp))
    np.add.at(y, rows, np.einsum("kij,kj->ki", blocks, xb[bc]))
    return np.linalg.norm(b - y.reshape(-1)) / np.linalg.norm(b)


def test_gmres_with_and_without_ilu0():
    import torch
    from navierstokes_amd import mpk, synth
    bp, bc, bv = synth.csr_to_bcsr4(*synth.fe_matrix(10))
    nb = len(bp) - 1
    n = 4 * nb
    A = mpk.bcsr4x4_matrix(nb, bp, bc, bv)
    M = mpk.bilu4(A, fill=0)
    b = synth.x_sin(0, n) + 1.0
    db = torch.from_numpy(b).cuda()
    out = {}
    for label, pre in (("ilu0", M), ("none", None)):
        dx = torch.zeros(n, dtype=torch.float64, device="cuda")
        its, hist = mpk.GMRES(A, db, dx, M=pre, restart=30, rtol=1e-8, maxiter=60)
        res = _true_residual(bp, bc, bv, dx.cpu().numpy(), b)
        print(f"GMRES(30) {label}: {its} iterations, true relative residual {res:.3e}, last of the history {hist[-1]:.3e}")
        assert 1 <= its <= 60 and len(hist) == its + 1
        h = np.array(hist)
        for c0 in range(0, its, 30):  # non-increasing within a cycle (entry c0 is the cycle's starting residual)
            cyc = h[c0:c0 + 31]
            assert (np.diff(cyc) <= 1e-14 * cyc[:-1]).all(), (label, c0, cyc)
        assert res / 10 <= h[-1] <= res * 10, (label, res, h[-1])
        out[label] = (its, res)
    assert out["ilu0"][1] <= 1e-8, out          # within 60 iterations (the CPU rehearsal of this driver: 21)
    assert out["none"][0] == 60 and out["none"][1] > 1e-5, out
    M.close()
    A.close()
