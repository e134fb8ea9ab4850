"""The plan of the one-launch block ILU solve (mi_bilu4one_plan_probe) on a box without a GPU: for every pattern of
tests/bilu4_cases.py and tests/bilu4one_cases.py, replayed for 1, 2, 3, 8 and 256 workgroups, every integer of the four tables
(chunk positions, chunk levels, dependency pointers, dependencies) equals the numpy restatement of tests/bilu4one_model.py, whose
own replay of the dealing finishes every chunk; the pattern with 257 dependencies is not eligible; bad patterns are refused with
mi_bilu4_plan_probe's messages.  The same for the patterns at the limits of the hand-off (bilu4one_cases.LIMIT_CASES: a chunk that
waits for 63, 64, 65, 128, 129, 255 and 256 others), whose shapes — chunk sizes, dependency counts, the widest consumer's list —
are asserted one by one, so that neither the generators nor the planner can dissolve a limit unnoticed; the cap from both sides
(fan:256 eligible, fan:257 not, on both sweeps)."""
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


def _sizes(got, b):
    return np.diff(got["chunk_pos"][b]).tolist()


def _deps(got, b, c):
    return got["dep"][b][got["dep_ptr"][b][c]:got["dep_ptr"][b][c + 1]].tolist()


@pytest.mark.parametrize("case", C1.LIMIT_CASES, ids=C.case_id)
def test_limit_patterns_tables_equal_the_restatement(case):
    from navierstokes_amd import mpk
    name, fill = case
    nb, bp, bc, _ = C1.matrix(name)
    want = M1.plan(nb, bp, bc, fill)
    assert want["eligible"]
    for G in WORKGROUPS:
        got = mpk.bilu4one_plan_probe(nb, bp, bc, fill, workgroups=G)
        assert got["eligible"] and got["why"] == ""
        _assert_tables_equal(got, want, f"{name} G {G}")
        for b in range(2):
            assert sorted(M1.replay(want["dep_ptr"][b], want["dep"][b], G)) == list(range(want["nchunks"][b]))


@pytest.mark.parametrize("k", C1.FAN_KS)
def test_fan_has_one_consumer_of_k_chunks_per_sweep(k):
    from navierstokes_amd import mpk
    got = mpk.bilu4one_plan_probe(*C1.matrix(f"fan:{k}")[:3], 0)
    assert got["nchunks"] == (k + 2, k + 2) and got["max_deps"] == (k, k)
    for b in range(2):
        assert _sizes(got, b) == [64] * k + [1, 1]
        assert np.diff(got["dep_ptr"][b]).tolist() == [0] * (k + 1) + [k]
        assert _deps(got, b, k + 1) == list(range(k)), "lane d of the poll no longer waits for chunk d"


@pytest.mark.parametrize("k", [64, 65, 256])
def test_fan_late_lists_the_dependency_that_finishes_last_in_last_place(k):
    from navierstokes_amd import mpk
    assert (f"fan_late:{k}", 0) in C1.LIMIT_CASES
    got = mpk.bilu4one_plan_probe(*C1.matrix(f"fan_late:{k}")[:3], 0)
    assert got["nchunks"][0] == k + 2 and got["max_deps"] == (k, 0)
    assert _sizes(got, 0) == [64] * (k - 1) + [C1.FAN_LATE_CHAIN, 64, 1]
    assert got["chunk_lev"][0].tolist()[k - 1:] == [1, C1.FAN_LATE_CHAIN + 1, C1.FAN_LATE_CHAIN + 2, C1.FAN_LATE_CHAIN + 3]
    assert np.diff(got["dep_ptr"][0]).tolist() == [0] * (k - 1) + [1, 1, k]
    assert _deps(got, 0, k - 1) == [0] and _deps(got, 0, k) == [k - 1], "the 64-row chunk no longer waits for the folded chain"
    last = _deps(got, 0, k + 1)
    assert last == list(range(k - 1)) + [k] and last[-3:] == [k - 3, k - 2, k], "lane k - 1 no longer polls the chunk behind the chain"
    assert set(_sizes(got, 1)) <= set(range(1, 65)) and not len(got["dep"][1])  # L links only: the backward sweep is one level


@pytest.mark.parametrize("k", [65, 256])
def test_spread_has_a_chunk_of_k_dependencies_made_of_rows_of_four(k):
    from navierstokes_amd import mpk
    assert (f"spread:{k}", 0) in C1.LIMIT_CASES
    nb, bp, bc, _ = C1.matrix(f"spread:{k}")
    got = mpk.bilu4one_plan_probe(nb, bp, bc, 0)
    assert got["nchunks"][0] == k + 2 and got["max_deps"][0] == k
    assert _sizes(got, 0) == [64] * k + [64, 1]
    assert _deps(got, 0, k) == list(range(k)), "the first consumer chunk no longer names every diagonal chunk"
    assert _deps(got, 0, k + 1) == list(range(64, k, 64)) and len(_deps(got, 0, k + 1)) <= 4
    lower = [int((bc[bp[i]:bp[i + 1]] < i).sum()) for i in range(64 * k, nb)]
    assert max(lower) <= 4 and sum(lower) == len(C1.spread_links(k)), "a consumer row with more than 4 blocks: its own lanes could poll"
    # the 65 consumer rows are consecutive positions of the backward sweep's level 0: no backward chunk names more than 3 chunks
    assert 1 <= got["max_deps"][1] <= 3
    pairs = set(C1.spread_links(k))
    mirrored = {(i, j) for i, j in pairs if i in bc[bp[j]:bp[j + 1]]}
    assert mirrored and mirrored != pairs, "spread lost its L(i, j) without U(j, i)"


def test_the_cap_of_256_dependencies_from_both_sides_on_both_sweeps():
    from navierstokes_amd import mpk
    name, fill = C1.FAN_OVER_CAP
    nb, bp, bc, _ = C1.matrix(name)
    want = M1.plan(nb, bp, bc, fill)
    assert not want["eligible"] and want["max_deps"] == [257, 257]
    for G in WORKGROUPS:
        got = mpk.bilu4one_plan_probe(nb, bp, bc, fill, workgroups=G)
        assert not got["eligible"] and got["max_deps"] == (257, 257) and "256" in got["why"] and "257" in got["why"], got["why"]
        _assert_tables_equal(got, want, f"{name} G {G}")
    got = mpk.bilu4one_plan_probe(*C1.matrix("fan:256")[:3], 0)
    assert got["eligible"] and got["why"] == "" and got["max_deps"] == (256, 256)


def test_the_limit_patterns_cover_every_count_of_polling_waves():
    """What the suite reached before these patterns was 44 dependencies (alternating, backward sweep)."""
    from navierstokes_amd import mpk
    seen = [set(), set()]
    for name, fill in C1.LIMIT_CASES:
        got = mpk.bilu4one_plan_probe(*C1.matrix(name)[:3], fill)
        assert max(got["max_deps"]) == C1.limit_k(name)
        for b in range(2):
            seen[b].add(got["max_deps"][b])
    for b in range(2):
        assert {63, 64, 65, 128, 129, 255, 256} <= seen[b]
