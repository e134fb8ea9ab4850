"""mi_bilu4_plan_probe and the pattern of mi_bilu4_factor_host against the model (tests/bilu4_model.py), exactly: symbolic ILU(k),
the dependency levels of the two sweeps, their sizes, the launches after folding.  No GPU.  Also: the model's vectorised fma is
the C library's fma, and every refusal of the argument rules is reached.

The layered cases of tests/bilu4_cases.py prescribe their level widths; here it is asserted that they have them, in the model and
in the library's plan, and that together they reach the limits of the schedule: levels of 1, 63, 64, 65, 128 and 129 rows in each
sweep, a folded run of more than 100 levels that fills every slot a folded level can fill (63 of the workgroup's 64: a level of 64
is no longer folded), and a sweep in which every launch boundary is a switch between the two kernels."""
import ctypes

import numpy as np
import pytest

import bilu4_cases as C
import bilu4_model as M

MI_ERR_ARG = 1


def test_model_fma_emulation_is_libm_fma():
    rng = np.random.default_rng(5)
    n = 60000
    a = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
    b = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
    c = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
    near = -a * b  # cancelling addends: the rounded product, and neighbours of it
    c[0::4] = near[0::4]
    c[1::4] = np.nextafter(near[1::4], np.inf)
    c[2::4] = near[2::4] * (1 + 2.0 ** -30)
    edge = np.array([0.0, -0.0, 1e300, -1e300, 5e-324, 2.2e-308, np.inf, np.nan, 1.0, 1 + 2.0 ** -52, 3.0, 1e-200])
    ea, eb, ec = (t.reshape(-1) for t in np.meshgrid(edge, edge, edge))
    a, b, c = np.concatenate([a, ea]), np.concatenate([b, eb]), np.concatenate([c, ec])
    want = np.array([M.fma(x, y, z) for x, y, z in zip(a, b, c)])
    got = M.fma_vec(a, b, c)
    same = (want.view(np.uint64) == got.view(np.uint64)) | (np.isnan(want) & np.isnan(got))
    assert same.all(), (a[~same][:3], b[~same][:3], c[~same][:3], want[~same][:3], got[~same][:3])


@pytest.mark.parametrize("case", C.ALL_CASES, ids=C.case_id)
def test_plan_and_pattern_equal_the_model(case):
    from navierstokes_amd import mpk
    name, fill = case
    nb, bp, bc, bv = C.matrix(name)
    ptr, col, diag = M.symbolic(nb, bp, bc, fill)
    fw, bw = M.schedule(nb, ptr, col, diag, False), M.schedule(nb, ptr, col, diag, True)
    pr = mpk.bilu4_plan_probe(nb, bp, bc, fill)
    assert pr["nblocks"] == len(col)
    assert (pr["fwd_levels"], pr["bwd_levels"]) == (fw["nlev"], bw["nlev"])
    assert np.array_equal(pr["fwd_sizes"], fw["sizes"]) and np.array_equal(pr["bwd_sizes"], bw["sizes"])
    assert (pr["fwd_launches"], pr["bwd_launches"]) == (fw["launches"], bw["launches"])
    # the pattern of a handle's factor: no values needed, so the identity matrix on A's pattern (it always factors)
    eye = ((np.repeat(np.arange(nb), np.diff(bp)) == bc)[:, None] * np.eye(4).reshape(-1)).reshape(-1)
    F = mpk.bilu4(nb, bp, bc, eye, fill=fill, host_only=True)
    fp, fc, fd, _ = F.factor_host()
    info = F.info()
    F.close()
    assert np.array_equal(fp, ptr) and np.array_equal(fc, col) and np.array_equal(fd, diag)
    assert info["nblocks"] == len(col) and info["launches"] == fw["launches"] + bw["launches"]
    assert (info["fwd_levels"], info["bwd_levels"], info["form"]) == (fw["nlev"], bw["nlev"], 0)


def test_shapes_schedule_as_they_must():
    from navierstokes_amd import mpk
    nb, bp, bc, _ = C.matrix("chain")
    pr = mpk.bilu4_plan_probe(nb, bp, bc, 0)  # nbrows levels of width 1: everything folds into one launch per sweep
    assert (pr["fwd_levels"], pr["bwd_levels"], pr["fwd_launches"], pr["bwd_launches"]) == (nb, nb, 1, 1)
    assert (pr["fwd_sizes"] == 1).all() and pr["nblocks"] == 3 * nb - 2
    nb, bp, bc, _ = C.matrix("diag")
    pr = mpk.bilu4_plan_probe(nb, bp, bc, 3)
    assert (pr["fwd_levels"], pr["bwd_levels"], pr["fwd_launches"], pr["bwd_launches"]) == (1, 1, 1, 1) and pr["fwd_sizes"][0] == nb
    nb, bp, bc, _ = C.matrix("arrow")
    pr = mpk.bilu4_plan_probe(nb, bp, bc, 0)  # the dense last row waits for everybody, everybody waits for the last column
    assert list(pr["fwd_sizes"]) == [nb - 1, 1] and list(pr["bwd_sizes"]) == [1, nb - 1]
    assert (pr["fwd_launches"], pr["bwd_launches"]) == (2, 2)  # a wide level and a narrow one each
    assert pr["nblocks"] == 3 * nb - 2  # no fill: every pair of rows meets in the last column only, which is there already


@pytest.mark.parametrize("nx,levels", [(6, 19), (10, 31), (16, 49)])
def test_fe_levels_are_the_mesh_planes(nx, levels):
    """Natural node order: the levels of the block lower triangle are the planes i + j + k = const, 3 nx + 1 of them."""
    from navierstokes_amd import mpk, synth
    bp, bc, _ = synth.csr_to_bcsr4(*synth.fe_matrix(nx))
    pr = mpk.bilu4_plan_probe(len(bp) - 1, bp, bc, 0)
    assert pr["fwd_levels"] == levels == 3 * nx + 1 and pr["bwd_levels"] == levels
    assert pr["fwd_sizes"].sum() == (nx + 1) ** 3 and pr["nblocks"] == len(bc)


@pytest.mark.parametrize("case", C.LAYERED_CASES + C.WIDE_CASES, ids=C.case_id)
def test_layered_cases_have_their_prescribed_levels_and_factor(case):
    from navierstokes_amd import mpk
    name, fill = case
    assert fill == 0  # fill above 0 can change the levels
    nb, bp, bc, _ = C.matrix(name)
    ptr, col, diag = M.symbolic(nb, bp, bc, 0)
    C.assert_layered_levels(name, M.schedule(nb, ptr, col, diag, False)["sizes"], M.schedule(nb, ptr, col, diag, True)["sizes"])
    pr = mpk.bilu4_plan_probe(nb, bp, bc, 0)
    C.assert_layered_levels(name, pr["fwd_sizes"], pr["bwd_sizes"])
    # structurally symmetric, as the generator promises
    pairs = set(zip(np.repeat(np.arange(nb), np.diff(bp)).tolist(), bc.tolist()))
    assert all((j, i) in pairs for i, j in pairs)
    # a zero pivot among the new cases is a failure, never a way round a GPU test
    assert not isinstance(C.model_factor(name, 0), M.ZeroPivot) and not isinstance(C.model_factor(name, 0, 1), M.ZeroPivot)


def test_layered_cases_reach_the_limits_of_the_schedule():
    from navierstokes_amd import mpk
    W = M.ROWS_PER_WG
    seen = {False: set(), True: set()}
    longest_full_fold, most_switches, longest_row = 0, 0, 0
    for name, _ in C.LAYERED_CASES + C.WIDE_CASES:
        nb, bp, bc, _ = C.matrix(name)
        ptr, col, diag = M.symbolic(nb, bp, bc, 0)
        pr = mpk.bilu4_plan_probe(nb, bp, bc, 0)
        longest_row = max(longest_row, int(np.diff(bp).max()))
        for backward in (False, True):
            S = M.schedule(nb, ptr, col, diag, backward)
            assert S["launches"] == pr["bwd_launches" if backward else "fwd_launches"]
            seen[backward] |= set(int(s) for s in S["sizes"])
            folded = []  # per launch: is it the folded kernel
            for a in range(S["launches"]):
                l0, l1 = S["launch_ptr"][a], S["launch_ptr"][a + 1]
                sz = S["sizes"][l0:l1]
                folded.append(bool(sz[0] < W))
                assert (sz < W).all() if folded[-1] else (l1 - l0 == 1 and sz[0] >= W)
                if folded[-1] and sz.max() == W - 1 and sz.min() == 1:
                    longest_full_fold = max(longest_full_fold, l1 - l0)
            most_switches = max(most_switches, sum(a != b for a, b in zip(folded, folded[1:])))
    for backward in (False, True):
        assert {1, W - 1, W, W + 1, 2 * W, 2 * W + 1} <= seen[backward], sorted(seen[backward])
        assert set(range(1, W)) <= seen[backward]  # every slot count of a folded level
    assert longest_full_fold > 100 and most_switches > 20 and longest_row > 200, (longest_full_fold, most_switches, longest_row)


def _refused(status, word):
    from navierstokes_amd import mpk
    assert status == MI_ERR_ARG, status
    msg = mpk.lib().mi_last_error().decode()
    assert word in msg, msg


def test_every_refusal_is_reached():
    from navierstokes_amd import mpk
    L = mpk.lib()
    i32 = lambda *a: np.array(a, np.int32)
    ok_p, ok_c = i32(0, 2, 4), i32(0, 1, 0, 1)
    val = np.concatenate([np.eye(4).reshape(-1), np.zeros(16), np.zeros(16), np.eye(4).reshape(-1)])
    nblk, n4 = ctypes.c_longlong(), [ctypes.c_int() for _ in range(4)]
    h = ctypes.c_void_p()

    def probe(nb, p, c, fill):
        return L.mi_bilu4_plan_probe(nb, None if p is None else p.ctypes.data, None if c is None else c.ctypes.data, fill,
                                     ctypes.byref(nblk), *[ctypes.byref(t) for t in n4], None, None, 0)

    def create(nb, p, c, v, layout, fill, host=True, out=h):
        f = L.mi_bilu4_create_host if host else L.mi_bilu4_create
        return f(nb, None if p is None else p.ctypes.data, None if c is None else c.ctypes.data, None if v is None else v.ctypes.data,
                 layout, fill, None if out is None else ctypes.byref(out))

    for call in (probe, lambda nb, p, c, fill: create(nb, p, c, val, 0, fill), lambda nb, p, c, fill: create(nb, p, c, val, 0, fill, host=False)):
        _refused(call(-1, ok_p, ok_c, 0), "negative")
        _refused(call(2, ok_p, ok_c, -1), "fill")
        _refused(call(2, None, ok_c, 0), "null")
        _refused(call(2, ok_p, None, 0), "null")
        _refused(call(2, ok_p, i32(0, 2, 0, 1), 0), "square")      # a block column past the last block row: not square
        _refused(call(2, ok_p, i32(0, -1, 0, 1), 0), "out of range")
        _refused(call(2, ok_p, i32(1, 0, 0, 1), 0), "unsorted")
        _refused(call(2, ok_p, i32(0, 0, 0, 1), 0), "duplicate")
        _refused(call(2, i32(0, 2, 3), i32(0, 1, 0), 0), "missing diagonal")
        _refused(call(2, i32(0, 2, 1), i32(0, 1), 0), "ptrow")
    _refused(create(2, ok_p, ok_c, None, 0, 0), "null")
    _refused(create(2, ok_p, ok_c, val, 2, 0), "layout")
    _refused(create(2, ok_p, ok_c, val, 0, 0, out=None), "null")
    assert h.value is None
    # nbrows == 0 is a no-op everywhere
    assert probe(0, None, None, 0) == 0 and nblk.value == 0 and n4[0].value == 0
    assert create(0, None, None, None, 0, 0) == 0 and h.value
    assert L.mi_bilu4_refactor(h, None, 0) == 0 and L.mi_bilu4_solve(h, None, None) == 0 and L.mi_bilu4_solve_dev(h, None, None, None) == 0
    assert L.mi_bilu4_destroy(h) == 0
