"""Every case of tests/bcsr4_row_cases.py is what it is named for — shown on the CPU: mi_bcsr4_tile_probe (the list builder
mi_bcsr4_create runs, bcsr4_tile_plan.hpp) gives the stated answer at 1024 and 1025 block columns per group and at 4095 and 4096
blocks, the pipeline cases hold every pair of neighbouring block-row lengths, and each pattern expanded to CSR is recognised as
blocked again.  tests/test_gpu_bcsr4_row_limits.py asserts the same probe first."""
import ctypes
import os
import re

import numpy as np
import pytest

import bcsr4_row_cases as BC
from conftest import ROOT
from navierstokes_amd import mpk

CSRC = os.path.join(ROOT, "navierstokes_amd", "csrc")


def test_constants_are_those_of_the_library():
    assert int(re.search(r"constexpr int kBtileNodes = (\d+);", open(os.path.join(CSRC, "spmv_kernels.hpp")).read()).group(1)) == BC.TILE_NODES
    assert int(re.search(r"constexpr long long kBtileMinBlocks = (\d+);", open(os.path.join(CSRC, "bcsr4_tile_plan.hpp")).read()).group(1)) == BC.TILE_MIN_BLOCKS
    assert int(re.search(r"constexpr int kBcsrDepth = (\d+);", open(os.path.join(CSRC, "spmv_kernels.hpp")).read()).group(1)) == 2


@pytest.mark.parametrize("name", BC.ALL)
def test_probe_gives_the_stated_answer(name):
    K = BC.case(name)
    got = mpk.bcsr4_tile_probe(K.nbrows, K.ptrow, K.indcol)
    assert got == K.probe, (name, got, K.probe)
    # the lists restated: distinct block columns of every group of 64 block rows
    per_group = [len(np.unique(K.indcol[K.ptrow[g]:K.ptrow[min(g + BC.TILE_ROWS, K.nbrows)]])) for g in range(0, K.nbrows, BC.TILE_ROWS)]
    nb = int(K.ptrow[-1])
    assert got["would_build"] == (nb >= BC.TILE_MIN_BLOCKS and max(per_group) <= BC.TILE_NODES)
    if got["would_build"]:
        assert (got["max_nodes"], got["groups_at_cap"]) == (max(per_group), per_group.count(BC.TILE_NODES))


def test_the_x_tile_cases_sit_on_both_limits():
    cap, over, small, exact = (BC.case(nm) for nm in ("xtile_cap", "xtile_over", "xtile_small", "xtile_exact"))
    assert cap.ptrow[-1] >= BC.TILE_MIN_BLOCKS and small.ptrow[-1] == BC.TILE_MIN_BLOCKS - 1 and exact.ptrow[-1] == BC.TILE_MIN_BLOCKS
    for K in (cap, over, small, exact):
        groups = [np.unique(K.indcol[K.ptrow[g]:K.ptrow[min(g + 64, K.nbrows)]]) for g in range(0, K.nbrows, 64)]
        assert len(groups[0]) == (1025 if K is over else 1024) and len(groups[1]) == 1
        assert K.nbrows % 64 != 0 and K.ptrow[-1] == K.ptrow[-2], "a partial last group whose last block row is empty"


@pytest.mark.parametrize("nbrows", BC.PIPE_ROWS)
def test_pipeline_cases_hold_every_neighbourhood(nbrows):
    K = BC.case(f"pipe_{nbrows}")
    lens = np.diff(K.ptrow).tolist()
    assert K.nbrows == nbrows and K.nbcols > nbrows
    if nbrows == 1:
        assert lens == [5]
        return
    assert int(K.indcol.max()) == K.nbcols - 1, "the last block column is named"
    assert lens[0] == 0 and lens[-1] == 0 and set(lens) == set(BC.PIPE_LENGTHS)
    pairs = set(zip(lens[:-1], lens[1:]))
    assert len(pairs) == len(BC.PIPE_LENGTHS) ** 2, sorted(set((a, b) for a in BC.PIPE_LENGTHS for b in BC.PIPE_LENGTHS) - pairs)
    order = [np.diff(K.indcol[K.ptrow[i]:K.ptrow[i + 1]].astype(np.int64)) for i in range(nbrows)]
    assert any((d < 0).any() for d in order) and any((d == 0).any() or len(np.unique(K.indcol[K.ptrow[i]:K.ptrow[i + 1]])) < lens[i]
                                                      for i, d in enumerate(order))


@pytest.mark.parametrize("name", BC.ALL)
def test_expanded_to_csr_the_pattern_is_blocked_again(name):
    K = BC.case(name)
    n, ncols, p, c, v = BC.to_csr(K)
    blocked, nblocks = ctypes.c_int(), ctypes.c_longlong()
    mpk.check(mpk.lib().mi_csr_block4_structure(n, p.ctypes.data, c.ctypes.data, ctypes.byref(blocked), ctypes.byref(nblocks)))
    assert blocked.value == 1 and nblocks.value == K.ptrow[-1]
    assert p[-1] == 16 * K.ptrow[-1] and np.array_equal(np.sort(v), np.sort(K.coef))
