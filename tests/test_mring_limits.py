"""Every case of tests/mring_cases.py reaches the state of the multi-window ring kernel's plan it is named for — shown on the CPU
with mi_mring_plan_census (mring_plan.hpp: mring_plan_census), after the C++ replay of mi_mring_plan_probe has accepted the plan."""
import os
import re

import pytest

import mring_cases as MC
from conftest import ROOT
from navierstokes_amd import mpk
from test_mring_plan import probe
from test_ring_limits import check_want

HPP = os.path.join(ROOT, "navierstokes_amd", "csrc", "mring_plan.hpp")
# mi_mring_plan_probe takes no column count and bounds every group's first column by the number of ROWS: it cannot describe a
# matrix with more columns than rows.  That case has its census here and its bits on the GPU.
NO_PROBE = ("m6_wide",)


def test_constants_are_those_of_the_planner():
    txt = open(HPP).read()
    for name, v in (("kMringK", MC.K), ("kMringW", MC.W), ("kMringGap", MC.GAP), ("kMringLead", MC.LEAD), ("kMringGroups", MC.GROUPS),
                    ("kMringXcds", MC.XCDS), ("kMringMaxB", MC.MAX_B)):
        assert int(re.search(rf"constexpr int {name} = (\d+);", txt).group(1)) == v, name
    m = re.search(r"constexpr int kMringNnzb = (\d+), kMringThreads = (\d+), kMringWgUnit = (\d+);", txt)
    assert tuple(map(int, m.groups())) == (MC.NNZB, MC.T, MC.WG_UNIT)


@pytest.mark.parametrize("name", MC.NAMES)
def test_case_is_planned_soundly_and_sits_on_its_limit(name):
    K = MC.case(name)
    S = mpk.mring_plan_census(K.n, K.ptrow, K.indcol)
    if name not in NO_PROBE:
        nblk, runs, bad, frac, restarts = probe(K.ptrow, K.indcol)      # the C++ replay: MiError names the first violation
        assert (S["blocks"], S["runs"], S["runs_kind0"], S["forced_cuts"]) == (nblk, runs, bad, restarts), name
    assert S["runs_kind0"] + S["runs_kind1"] + S["runs_kind3"] == S["runs"] == S["table_len"] - S["table_padded"]
    assert S["table_len"] % MC.XCDS == 0 and S["run_max"] <= MC.MAX_B and S["groups_max"] <= MC.GROUPS
    check_want(S, K.want, name)


def test_one_group_more_than_the_loop_refills_starts_exactly_one_run():
    """M2: the same matrix but for ONE column of one block: GROUPS groups stay inside the run, GROUPS + 1 cut it"""
    a, b = MC.case("m2"), MC.case("m2_cut")
    Sa, Sb = mpk.mring_plan_census(a.n, a.ptrow, a.indcol), mpk.mring_plan_census(b.n, b.ptrow, b.indcol)
    assert (Sa["forced_cuts"], Sb["forced_cuts"]) == (0, 1) and Sb["runs"] == Sa["runs"] + 1
    assert Sa["groups_full"] == 1 and Sb["groups_full"] == 0


def test_why_the_run_kind_case_is_as_large_as_it_is():
    """M4 at 800 blocks: PLAIN blocks weigh kRingPlainWeight, so each is dealt into a run of its own; one step of 200 blocks below
    the pinned size there is still no run of four"""
    K = MC.case("m4_small")
    S = mpk.mring_plan_census(K.n, K.ptrow, K.indcol)
    assert S["wide_max_per_run"] == 1 and S["runs_kind0"] == 0, S
    nblk = MC.N_M4 // MC.ROWS - 200
    p, c, _ = MC.m4_matrix(nblk)
    S = mpk.mring_plan_census(nblk * MC.ROWS, p, c)
    assert S["runs_kind0"] == 0 and S["runs_wide4"] == 0 and S["runs_wide3"] > 0, S
