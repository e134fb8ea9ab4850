"""Every case of tests/ring_cases.py reaches the state of the ring kernel's plan it is named for — shown on the CPU with
mi_ring_plan_census (ring_plan.hpp: ring_plan_census), after the C++ replay of mi_ring_plan_probe has accepted the plan.  A planner
change that moves a case off its limit fails here (and in tests/test_gpu_ring_limits.py, which asserts the same census first)
instead of quietly emptying the GPU test."""
import os
import re

import numpy as np
import pytest

import ring_cases as RC
from conftest import ROOT
from navierstokes_amd import mpk
from test_ring_plan import probe

HPP = os.path.join(ROOT, "navierstokes_amd", "csrc", "ring_plan.hpp")


def check_want(S, want, what):
    for k, w in want.items():
        if isinstance(w, tuple):
            assert S[k] == w[1], f"{what}: census {k} = {S[k]}, the case needs exactly {w[1]}"
        else:
            assert S[k] >= w, f"{what}: census {k} = {S[k]}, the case needs at least {w}"


def test_constants_are_those_of_the_planner():
    txt = open(HPP).read()
    rows = re.findall(r"^\s*\{(\d), (\d+), (\d+), (\d+), (\d), (\d+)\},", txt, re.M)
    assert len(rows) == len(RC.CONFIGS) == 4
    for row in rows:
        cid, T, nnzb, ring, D, unit = map(int, row)
        C = RC.CONFIGS[cid]
        assert (C.T, C.NNZB, C.RING, C.D, C.WG_UNIT) == (T, nnzb, ring, D, unit)
        assert C.ROWS == (T if cid == 4 else 2 * T)
    for name, v in (("kRingMaxB", RC.K_RING_MAX_B), ("kRingMaxPlain", RC.K_RING_MAX_PLAIN), ("kRingPlainWeight", RC.K_RING_PLAIN_WEIGHT)):
        assert int(re.search(rf"constexpr int {name} = (\d+);", txt).group(1)) == v
    hdr = open(os.path.join(ROOT, "include", "mi355_spmv.h")).read()
    assert int(re.search(r"#define MI_RING_CENSUS_LEN (\d+)", hdr).group(1)) == len(mpk.RING_CENSUS)
    assert int(re.search(r"#define MI_MRING_CENSUS_LEN (\d+)", hdr).group(1)) == len(mpk.MRING_CENSUS)


def test_census_refuses_a_short_array():
    p = np.array([0, 1], np.int32)
    c = np.zeros(1, np.int32)
    out = np.zeros(4, np.int64)
    assert mpk.lib().mi_ring_plan_census(1, p.ctypes.data, c.ctypes.data, 4, out.ctypes.data, 4) == 1       # MI_ERR_ARG
    assert mpk.lib().mi_mring_plan_census(1, p.ctypes.data, c.ctypes.data, out.ctypes.data, 4) == 1
    assert mpk.ring_plan_census(0, np.zeros(1, np.int32), np.zeros(0, np.int32), 4)["blocks"] == 0


@pytest.mark.parametrize("name,cfg", RC.ALL)
def test_case_is_planned_soundly_and_sits_on_its_limit(name, cfg):
    K = RC.case(name, cfg)
    nblk, runs, bad, frac, mslot = probe(K.ptrow, K.indcol, cfg)          # the C++ replay: MiError names the first violation
    S = mpk.ring_plan_census(K.n, K.ptrow, K.indcol, cfg)
    assert (S["blocks"], S["table_len"], S["runs_kind0"]) == (nblk, runs, bad), (name, cfg)
    assert S["runs_nonempty"] + S["runs_idle"] == S["table_len"] and S["runs_kind0"] + S["runs_kind1"] + S["runs_kind3"] == S["runs_nonempty"]
    assert S["served"] + S["plain"] <= S["blocks"] - S["empty"] <= S["served"] + S["plain"] + S["kind0_blocks"]
    assert S["run_max"] <= RC.K_RING_MAX_B and mslot < RC.CONFIGS[cfg].RING
    check_want(S, K.want, f"{name}, configuration {cfg}")
    order = np.diff(K.indcol.astype(np.int64))
    if K.ptrow[-1] > K.n:                                                  # rows of several nonzeros: not all ascending
        inside = np.ones(len(order), bool)
        ends = K.ptrow[1:-1]
        inside[ends[(ends > 0) & (ends <= len(order))] - 1] = False       # (differences across a row boundary do not count)
        assert (order[inside] < 0).any(), "columns inside the rows are all ascending"


@pytest.mark.parametrize("cfg", RC.CONFIGS_OF["r1"])
def test_why_the_run_kind_case_is_as_large_as_it_is(cfg):
    """The R1 matrix at 600 000 rows: every block the window cannot serve is dealt into a run of its own (they weigh kRingPlainWeight,
    the mean weight of a run is far below 4 * kRingPlainWeight), so no run holds two PLAIN blocks and none goes down the plain path
    as a whole.  One step of 100 000 rows below the pinned size one of the three kinds is still missing."""
    K = RC.case("r1_small", cfg)
    S = mpk.ring_plan_census(K.n, K.ptrow, K.indcol, cfg)
    assert S["wide_max_per_run"] == 1 and S["runs_kind0"] == 0 and S["runs_wide1"] == S["runs_kind3"] > 0, S
    n = RC.N_R1[cfg] - 100_000
    p, c, _ = RC.r1_matrix(cfg, n)
    S = mpk.ring_plan_census(n, p, c, cfg)
    assert not (S["runs_kind0"] and S["runs_kind1"] and S["runs_kind3"] and S["runs_wide3"] and S["runs_wide4"]), (n, S)


def test_depth_and_lean_follow_the_rule_of_the_handle():
    """blocks of prefetch: 4 from 40 blocks a run on (configuration 4), else the configuration's; LEAN only for configuration 4"""
    K = RC.case("r8", 4)
    assert mpk.ring_plan_census(K.n, K.ptrow, K.indcol, 4)["depth"] == 2
    K = RC.case("r3", 2)
    S = mpk.ring_plan_census(K.n, K.ptrow, K.indcol, 2)
    assert S["lean"] == 0 and S["depth"] == RC.CONFIGS[2].D
