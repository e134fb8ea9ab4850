"""The plan of the one-launch block ILU solve (mi_bilu4one_plan_probe) on a box without a GPU: for every pattern of
tests/bilu4_cases.py and tests/bilu4one_cases.py, replayed for 1, 2, 3, 8 and 256 workgroups, every integer of the four tables
(chunk positions, chunk levels, dependency pointers, dependencies) equals the numpy restatement of tests/bilu4one_model.py, whose
own replay of the dealing finishes every chunk; the pattern with 257 dependencies is not eligible; bad patterns are refused with
mi_bilu4_plan_probe's messages."""
import ctypes

import numpy as np
import pytest

import bilu4_cases as C
import bilu4one_cases as C1
import bilu4one_model as M1

WORKGROUPS = (1, 2, 3, 8, 256)
MI_ERR_ARG = 1
CASES = [(C, c) for c in C.ALL_CASES] + [(C1, c) for c in C1.SOLVE_CASES]


def _assert_tables_equal(got, want, what):
    for key in ("chunk_pos", "chunk_lev", "dep_ptr", "dep"):
        for b, sweep in enumerate(("forward", "backward")):
            g, w = np.asarray(got[key][b]), np.asarray(want[key][b])
            assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {key} of the {sweep} sweep differs"
    assert tuple(got["nchunks"]) == tuple(want["nchunks"]) and tuple(got["max_deps"]) == tuple(want["max_deps"]), what


@pytest.mark.parametrize("mod,case", CASES, ids=[C.case_id(c) for _, c in CASES])
def test_probe_tables_equal_the_restatement(mod, case):
    from navierstokes_amd import mpk
    name, fill = case
    nb, bp, bc, _ = mod.matrix(name)
    want = M1.plan(nb, bp, bc, fill)
    assert want["eligible"]
    for G in WORKGROUPS:
        got = mpk.bilu4one_plan_probe(nb, bp, bc, fill, workgroups=G)  # MI_OK: the library's own replay found no violation
        assert got["eligible"] and got["why"] == "" and got["plan_bytes"] > 0
        _assert_tables_equal(got, want, f"{name} fill {fill} G {G}")
    for b in range(2):
        cp, dp, d = want["chunk_pos"][b], want["dep_ptr"][b], want["dep"][b]
        assert (np.diff(cp) > 0).all() and cp[0] == 0 and cp[-1] == nb
        assert all((d[dp[c]:dp[c + 1]] < c).all() for c in range(len(cp) - 1)), "a dependency that is not an earlier chunk"
        for G in WORKGROUPS:
            assert sorted(M1.replay(dp, d, G)) == list(range(len(cp) - 1))


def test_the_extra_patterns_have_the_chunks_they_were_built_for():
    from navierstokes_amd import mpk
    got = mpk.bilu4one_plan_probe(*C1.matrix("wide3")[:3], 0)
    assert np.diff(got["chunk_pos"][0]).tolist() == [64, 64, 2, 64, 64, 1] and got["chunk_lev"][0].tolist() == [0, 0, 0, 1, 2, 2, 3]
    nb, bp, bc, _ = C1.matrix("wide3")
    pairs = {(i, int(j)) for i in range(nb) for j in bc[bp[i]:bp[i + 1]]}
    assert any(j < i and (j, i) not in pairs for i, j in pairs), "wide3 lost its L(k, i) without U(i, k)"
    got = mpk.bilu4one_plan_probe(*C1.matrix("fold_wide_fold")[:3], 0)
    for b in range(2):
        assert np.diff(got["chunk_pos"][b]).tolist() == [20, 64, 64, 64, 8, 20]
        assert got["dep"][b][got["dep_ptr"][b][5]:].tolist() == [1, 2, 3, 4]
    got = mpk.bilu4one_plan_probe(*C1.matrix("arrow200")[:3], 0)
    assert np.diff(got["chunk_pos"][0]).tolist() == [64, 64, 64, 7, 1] and got["max_deps"] == (4, 0)
    assert np.diff(got["chunk_pos"][1]).tolist() == [64, 64, 64, 8]
    # every small pattern of bilu4_cases folds or has prescribed layers; fe:6 has no plane of 64 rows
    got = mpk.bilu4one_plan_probe(*C.matrix("fe:6")[:3], 0)
    assert got["nchunks"] == (1, 1) and got["max_deps"] == (0, 0)


def test_a_chunk_with_more_than_256_dependencies_is_not_eligible():
    from navierstokes_amd import mpk
    name, fill = C1.PROBE_ONLY
    nb, bp, bc, _ = C1.matrix(name)
    want = M1.plan(nb, bp, bc, fill)
    assert not want["eligible"] and want["max_deps"] == [257, 0]
    for G in WORKGROUPS:
        got = mpk.bilu4one_plan_probe(nb, bp, bc, fill, workgroups=G)
        assert not got["eligible"] and "256" in got["why"] and "257" in got["why"], got["why"]
        _assert_tables_equal(got, want, f"{name} G {G}")


def test_bad_patterns_are_refused_with_the_plan_probe_s_messages():
    from navierstokes_amd import mpk
    L = mpk.lib()
    i32 = lambda a: np.array(a, np.int32)
    cases = [(2, i32([0, 1, 2]), i32([0, 1]), -1), (-1, i32([0]), i32([0]), 0), (2, i32([1, 2, 3]), i32([0, 0, 1]), 0), (2, i32([0, 2, 1]), i32([0, 1]), 0),
             (2, i32([0, 1, 2]), i32([0, 2]), 0), (2, i32([0, 2, 3]), i32([1, 0, 1]), 0), (2, i32([0, 2, 3]), i32([0, 0, 1]), 0),
             (2, i32([0, 1, 2]), i32([0, 0]), 0)]
    el = ctypes.c_int(7)
    for nb, p, c, fill in cases:
        assert L.mi_bilu4_plan_probe(nb, p.ctypes.data, c.ctypes.data, fill, *([None] * 7), 0) == MI_ERR_ARG
        want = L.mi_last_error().decode()
        assert L.mi_bilu4one_plan_probe(nb, p.ctypes.data, c.ctypes.data, fill, 0, ctypes.byref(el), *([None] * 7)) == MI_ERR_ARG
        assert L.mi_last_error().decode() == want and want
    assert L.mi_bilu4one_plan_probe(2, None, None, 0, 0, *([None] * 8)) == MI_ERR_ARG and "null ptrow" in L.mi_last_error().decode()
    p, c = i32([0, 1, 2]), i32([0, 1])
    assert L.mi_bilu4one_plan_probe(2, p.ctypes.data, c.ctypes.data, 0, -1, *([None] * 8)) == MI_ERR_ARG and "workgroups" in L.mi_last_error().decode()
    with pytest.raises(mpk.MiError):
        mpk.bilu4one_plan_probe(2, [0, 1, 2], [0, 0], 0)
    empty = mpk.bilu4one_plan_probe(0, [0], [], 0)
    assert empty["eligible"] and empty["nchunks"] == (0, 0) and empty["chunk_pos"][0].tolist() == [0]
