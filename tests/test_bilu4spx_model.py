"""The two statements of the single-precision exact solve (mi_bilu4spx_*, include/mi355_spmv.h) agree in the model, bit for bit:
  (a) tests/bilu4_model.solve on tests/bilu4_sp_model.rounded(factor) — the exact solve with v32 in place of every value;
  (b) tests/bilu4_sp_model.solve_sweeps_sp with both counts at the clamp — what mi_bilu4sp_solve_dev returns there.
Pure numpy.  This is the licence for tests/test_gpu_bilu4spx.py to take either as the GPU's oracle."""
import numpy as np
import pytest

import bilu4_model as M
import bilu4_sp_cases as SC
import bilu4_sp_model as SP
import bilu4_sweeps_model as S

PATTERNS = ["fe:6", "chain", "arrow", "sp_edges", "sp_overflow", "random:3", "random:7", "random:12"]
CASES = [(name, fill) for name in PATTERNS for fill in (0, 1)]


@pytest.mark.parametrize("name,fill", CASES, ids=[f"{n}-fill{f}" for n, f in CASES])
def test_the_exact_solve_of_the_rounded_factor_is_the_f32_sweeps_at_the_clamp(name, fill):
    nb = SC.matrix(name)[0]
    fac = SC.model_factor(name, fill)
    assert not isinstance(fac, M.ZeroPivot), f"{name} fill {fill} does not factor: not a case here"
    b = np.random.default_rng(5 * nb + fill).standard_normal(4 * nb)
    with np.errstate(all="ignore"):  # (sp_overflow: Inf in the rounded factor, Inf - Inf in its rows)
        exact = M.solve(nb, *SP.rounded(fac), b)
        mf, mb = S.max_sweeps(nb, *fac[:3])
        at_clamp = SP.solve_sweeps_sp(nb, *fac, b, mf, mb)
        far_above = SP.solve_sweeps_sp(nb, *fac, b, 10 ** 6, 10 ** 6)
        double = M.solve(nb, *fac, b)
    assert np.array_equal(exact.view(np.int64), at_clamp.view(np.int64)), f"{name} fill {fill}: the two statements differ"
    assert np.array_equal(exact.view(np.int64), far_above.view(np.int64)), f"{name} fill {fill}: counts above the clamp"
    if name == "sp_overflow":
        assert not np.isfinite(exact[:4]).all() and np.isfinite(exact[4:]).all(), "the overflow stays in block row 0, the sink"
    else:
        assert np.isfinite(exact).all()
    if nb > 1 and name != "sp_edges":
        assert not np.array_equal(exact, double), "the rounded factor is another operator than the factor"
