"""The ownership paths of an mi_bilu4 handle, which the other suites pass through once each: everything a handle can come to own —
the two level-major sweeps, the scratch vectors, the device refactor's tables, the one-launch solve's tables — built, used, built
again where it is idempotent, refused where the pattern is not eligible, and released; then the same life 25 times over with the
free device memory watched.  One test, one process.  Nothing is provoked: no give-up, no fault, no shortened spin bound."""
import numpy as np
import pytest

import bilu4_cases as C
import bilu4one_cases as C1
from conftest import assert_bit_equal
from test_gpu_bilu4 import _model_solve, _same
from test_gpu_bilu4dev import _assert_factor, _dev, _solve

pytestmark = pytest.mark.gpu

NAME = "limits:0"  # the smallest layered case with a wide and a folded launch in each sweep (782 block rows)
# the leak check's pattern: the same layers with three of 5 500 rows in front of the last two (no row then has more than 64 blocks).
# 17 482 block rows with more than one L and one U block each: the L values, the U values and the inverted diagonal blocks (128 bytes
# a block) are each above the allocator's 2 MiB granule
LEAK_WIDTHS = C.LIMITS_WIDTHS[:-1] + (5500, 5500, 5500, 200, 1)
GRANULE = 2 << 20


def _scaled(nb, bp, bc, bv, seed):
    """Other values on the same pattern, as bilu4_cases.new_values: every block scaled by a seeded factor, its diagonal kept."""
    v = np.array(bv, np.float64).reshape(-1, 4, 4)
    new = v * np.random.default_rng(seed).uniform(0.5, 1.5, (len(bc), 1, 1))
    on_diag = np.asarray(bc) == np.repeat(np.arange(nb), np.diff(bp))
    new[on_diag] = v[on_diag] * 1.25
    return new.reshape(-1)


def _life(nb, bp, bc, vals, b, want, what):
    """One handle from create to close.  vals: the values at create, of the device refactor, of the host refactor; want: the model's
    solve with the first and the third, and the host's factor of the second."""
    from navierstokes_amd import mpk
    F = mpk.bilu4(nb, bp, bc, vals[0], fill=0)
    _same(_solve(F, nb, b), want["x0"], f"{what}: the solve after create")
    F.prepare_dev()
    F.refactor_dev(_dev(vals[1])).factor_status().fetch_factor()
    _assert_factor(F.factor_host(), want["fac1"], f"{what}: the fetched device factor against the host's")
    assert F.info_dev()["prepared"] is True
    xs = []
    for form in (1, 0, 1):
        assert F.set_form(form) == form and F.info_one()["prepared"] is True
        xs.append(_solve(F, nb, b))
    assert not np.isnan(xs[0]).any()
    assert_bit_equal(xs[1], xs[0], f"{what}: form 0 against form 1")
    assert_bit_equal(xs[2], xs[0], f"{what}: form 1 again")
    F.refactor(vals[2])
    _same(_solve(F, nb, b), want["x2"], f"{what}: the solve after the host refactor")
    F.close()


def _host_factor(nb, bp, bc, v):
    from navierstokes_amd import mpk
    H = mpk.bilu4(nb, bp, bc, v, fill=0, host_only=True)
    fac = H.factor_host()
    H.close()
    return fac


def test_a_handle_owns_what_it_builds_and_frees_all_of_it():
    """Steady state, not the first cycles (the runtime and torch's allocator keep what they first took): free device memory after
    cycle 24 must not be below free memory after cycle 4.  A leaked value array is then certain to show, being larger than the
    2 MiB granule device memory is handed out in (asserted below).  A leaked SMALL table — a permutation, a chunk list, a flag array —
    can hide under that granule for many cycles: that the small tables go rests on the owning members' destructors being the only
    release path of capi_ilu.hip, not on this test."""
    import torch
    from navierstokes_amd import mpk
    nb, bp, bc, bv = C.matrix(NAME)
    pr = mpk.bilu4_plan_probe(nb, bp, bc, 0)
    C.assert_layered_levels(NAME, pr["fwd_sizes"], pr["bwd_sizes"])
    assert 1 < pr["fwd_launches"] < pr["fwd_levels"] and 1 < pr["bwd_launches"] < pr["bwd_levels"] and max(pr["fwd_sizes"]) >= 64
    b = np.random.default_rng(nb).standard_normal(4 * nb)
    vals = (bv, C.new_values(NAME, 1), C.new_values(NAME, 2))
    want = dict(x0=_model_solve(C.model_factor(NAME, 0), nb, b), fac1=_host_factor(nb, bp, bc, vals[1]),
                x2=_model_solve(C.model_factor(NAME, 0, 2), nb, b))
    _life(nb, bp, bc, vals, b, want, NAME)

    # the pattern that is not eligible for the one-launch form: refused twice, and the handle goes on in form 0
    nb1, bp1, bc1, bv1 = C1.matrix(C1.PROBE_ONLY[0])
    F = mpk.bilu4(nb1, bp1, bc1, bv1, fill=0)
    for _ in range(2):
        with pytest.raises(mpk.MiError) as e:
            F.prepare_one()
        assert e.value.status == 5
    one = F.info_one()
    assert one["prepared"] is False and one["eligible"] is False and one["workgroups"] == 0 and one["plan_bytes"] == 0
    b1 = np.random.default_rng(9).standard_normal(4 * nb1)
    assert F.info()["form"] == 0
    _same(_solve(F, nb1, b1), _model_solve(F.factor_host(), nb1, b1), "over_cap on form 0 after two refusals")
    F.close()

    # the same life over and over
    nb, bp, bc, bv = C.layered(LEAK_WIDTHS, 0, 36)
    vals = (bv, _scaled(nb, bp, bc, bv, 37), _scaled(nb, bp, bc, bv, 38))
    facs = [_host_factor(nb, bp, bc, v) for v in vals]
    ptr, col, diag = (np.asarray(a) for a in facs[0][:3])
    n_l, n_u = int((diag - ptr[:-1]).sum()), int((ptr[1:] - diag - 1).sum())
    assert min(n_l, n_u, nb) * 128 > GRANULE, "a value array of the leak check's pattern would fit the granule"
    b = np.random.default_rng(nb).standard_normal(4 * nb)
    want = dict(x0=_model_solve(facs[0], nb, b), fac1=facs[1], x2=_model_solve(facs[2], nb, b))
    free = {}
    for cycle in range(25):
        _life(nb, bp, bc, vals, b, want, f"cycle {cycle}")
        torch.cuda.synchronize()
        free[cycle] = torch.cuda.mem_get_info()[0]
    print(f"free device memory after cycle 4: {free[4]}, after cycle 24: {free[24]}")
    assert free[24] >= free[4], f"{free[4] - free[24]} bytes of device memory went in 20 lives of a handle"
