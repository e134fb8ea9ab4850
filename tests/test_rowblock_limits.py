"""Every case of tests/rowblock_cases.py reaches the branches of spmv_csr_stream<1024> / spmv_csr_tile<2048> it is named for — shown on
the CPU with mi_rowblock_census (rowblock_census.hpp), whose table is the one the handle runs (the same build_row_blocks /
build_tile_plan call under the same row_block_align rule).  A planner change that moves a case off its limit fails here (and in
tests/test_gpu_rowblock_limits.py, which asserts the same census first) instead of quietly emptying the GPU test.  The planner itself
is held to a numpy model of its three rules, block start by block start."""
import os
import re

import numpy as np
import pytest

import rowblock_cases as RB
from conftest import ROOT
from navierstokes_amd import mpk
from test_ring_limits import check_want
from test_tile_plan import probe as tile_probe

CSRC = os.path.join(ROOT, "navierstokes_amd", "csrc")


def model_row_starts(ptrow, nnzb, max_rows=RB.ROW_CAP, align=RB.ROW_ALIGN, keep=RB.KEEP_EIGHTHS):
    """build_row_blocks restated: fill greedily up to nnzb nonzeros and max_rows rows (at least one row); if the block does not end
    the matrix, pull its end back to a multiple of `align` rows where that leaves it a row and keep/8 of its nonzeros."""
    p = np.asarray(ptrow, np.int64)
    n, starts, r = len(p) - 1, [], 0
    while r < n:
        e = min(n, r + max_rows, max(r + 1, int(np.searchsorted(p, p[r] + nnzb, side="right")) - 1))
        ea = e // align * align
        if e < n and ea > r and 8 * (p[ea] - p[r]) >= keep * (p[e] - p[r]):
            e = ea
        starts.append(r)
        r = e
    return np.array(starts + [n], np.int64)


def test_constants_are_those_of_the_library():
    part = open(os.path.join(CSRC, "partition.hpp")).read()
    assert int(re.search(r"constexpr int kRowBlockKeepEighths = (\d+);", part).group(1)) == RB.KEEP_EIGHTHS
    assert re.search(r"inline int row_block_align\(long long nnz\) \{ return nnz < kRowBlockAlignMaxNnz \? (\d+) : 1; \}", part).group(1) == str(RB.ROW_ALIGN)
    tile = open(os.path.join(CSRC, "tile_plan.hpp")).read()
    assert int(re.search(r"constexpr int kTileNnzb = (\d+);", tile).group(1)) == RB.NNZBS["tile"]
    assert int(re.search(r"constexpr int kTileThreads = (\d+);", tile).group(1)) == RB.T
    assert int(re.search(r"constexpr int kWG = (\d+);", open(os.path.join(CSRC, "spmv_kernels.hpp")).read()).group(1)) == RB.T
    hdr = open(os.path.join(ROOT, "include", "mi355_spmv.h")).read()
    assert int(re.search(r"#define MI_ROWBLOCK_CENSUS_LEN (\d+)", hdr).group(1)) == len(mpk.ROWBLOCK_CENSUS)


def test_the_rules_exist_once():
    """the row-alignment rule, the tile kernel's SKEW rule and the blocked kernel's x-tile lists: one definition each, called by the
    library and by the probes"""
    src = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hpp", ".hip"))}
    everything = "\n".join(src.values())
    assert len(re.findall(r"nnz < \w+ \? 64 : 1", everything)) == 1 and "20000000 ?" not in everything
    assert src["capi_csr.hip"].count("row_block_align(") == 3                   # get_table, build_tile, mi_rowblock_census
    assert len(re.findall(r"mult8 > n", everything)) == 1 and src["capi_csr.hip"].count("tile_wants_skew(") == 2
    assert len(re.findall(r"<= cap;", src["bcsr4_tile_plan.hpp"])) == 1 and "u.size() <= kBtileNodes" not in everything
    assert src["capi_bcsr.hip"].count("build_bcsr4_tile_lists(") == 2           # build_bcsr4_tile, mi_bcsr4_tile_probe


def test_census_refuses_bad_arguments():
    p = np.array([0, 1], np.int32)
    c = np.zeros(1, np.int32)
    out = np.zeros(len(mpk.ROWBLOCK_CENSUS), np.int64)
    L = mpk.lib()
    assert L.mi_rowblock_census(1, p.ctypes.data, c.ctypes.data, mpk.KERNELS["stream"], out.ctypes.data, 4) == 1        # MI_ERR_ARG
    assert L.mi_rowblock_census(1, p.ctypes.data, c.ctypes.data, mpk.KERNELS["ring"], out.ctypes.data, out.size) == 1
    assert L.mi_rowblock_census(1, p.ctypes.data, c.ctypes.data, mpk.KERNELS["tile"], out.ctypes.data, out.size) == 0
    assert mpk.rowblock_census(0, np.zeros(1, np.int32), np.zeros(0, np.int32), "tile")["blocks"] == 0


@pytest.mark.parametrize("name,kern", RB.ALL)
def test_case_sits_on_its_limit_and_the_planner_follows_the_model(name, kern):
    K = RB.case(name, kern)
    nnzb = RB.NNZBS[kern]
    S, starts = mpk.rowblock_census(K.n, K.ptrow, K.indcol, kern, starts=True)
    print(name, kern, {k: v for k, v in S.items() if v})
    model = model_row_starts(K.ptrow, nnzb)
    assert S["blocks"] == len(model) - 1 and np.array_equal(starts, model), (name, kern, S["blocks"], len(model) - 1)
    assert S["row_align"] == RB.ROW_ALIGN and S["idle_wgs"] == -S["blocks"] % 8
    nn = np.diff(K.ptrow.astype(np.int64)[model])
    assert S["empty"] == int((nn == 0).sum()) and S["long"] == int((nn > nnzb).sum()) and S["full"] == int((nn == nnzb).sum())
    assert S["empty_first"] + S["empty_last"] + S["empty_middle"] >= S["empty"] >= S["empty_middle"]
    check_want(S, K.want, f"{name}, {kern}")
    if kern == "tile":
        check_want(S, K.want_tile, f"{name}, {kern}")
        assert sum(S[f"r{k}"] for k in range(1, 9)) == S["blocks"] - S["empty"] - S["long"]
    else:
        assert not any(S[k] for k in mpk.ROWBLOCK_CENSUS[mpk.ROWBLOCK_CENSUS.index("r1"):])
    # the tile plan's own invariants (mi_tile_plan_probe replays every slot), whichever block size the case was cut for
    nblk, total, umax, listed = tile_probe(K.ptrow, K.indcol)
    T = S if kern == "tile" else mpk.rowblock_census(K.n, K.ptrow, K.indcol, "tile")
    assert (nblk, umax) == (T["blocks"], T["u_max"]), (name, kern, nblk, umax, T["blocks"], T["u_max"])
    if name in RB.TILE_ONLY:
        assert total == sum(RB.LIST_LENGTHS) and listed == K.ptrow[-1]
    if K.ptrow[-1] > K.n:                                                  # rows of several nonzeros: not all ascending
        order = np.diff(K.indcol.astype(np.int64))
        inside = np.ones(len(order), bool)
        ends = K.ptrow[1:-1]
        inside[ends[(ends > 0) & (ends <= len(order))] - 1] = False
        assert name == "rect_one_column" or (order[inside] < 0).any(), "columns inside the rows are all ascending"


def test_every_counter_a_case_names_is_reached_by_some_case():
    """taken over the whole list: a case dropped, or a counter nobody fills any more, leaves a visible hole"""
    named, reached = set(), set()
    for name, kern in RB.ALL:
        K = RB.case(name, kern)
        S = mpk.rowblock_census(K.n, K.ptrow, K.indcol, kern)
        named |= set(K.want) | (set(K.want_tile) if kern == "tile" else set())
        reached |= {k for k, v in S.items() if v}
    assert named <= reached, sorted(named - reached)
    # ... and the counters the issue of this suite lists are all named by some case
    assert set(mpk.ROWBLOCK_CENSUS) - {"row_align"} <= named, sorted(set(mpk.ROWBLOCK_CENSUS) - named)


def test_the_model_knows_the_three_rules():
    """the model on hand-made row pointers: the nonzero limit, the row cap, the pull-back and its 7/8 refusal"""
    one = np.arange(0, 3001)                                               # 3000 rows of one nonzero
    assert model_row_starts(one, 2048).tolist() == [0, 1024, 2048, 3000]
    # 100 rows fit: 64 of [0, 100) are not 7/8 of it; [100, 200) back to 192 keeps 92; 256 would leave [192, 292) 64 of 100
    assert model_row_starts(one, 100).tolist()[:4] == [0, 100, 192, 292]
    assert model_row_starts(np.array([0, 0, 0, 5000, 5000, 5001]), 1024).tolist() == [0, 2, 3, 5]      # a long row stands alone
