"""The one-launch powers step's hand-off, held to a host model of the kernel (no GPU).  spmk_csr_ring reads what other workgroups
wrote in the same launch without an acquire; that is right only while every x index a run loads lies in the rows of a run on its
dependency list (ring_plan.hpp: build_run_deps).  mi_spmk_plan_probe checks the lists against the expression build_run_deps itself
uses; tests/spmk_model.py restates the loads from the KERNEL (every issue() of T lanes, sentinel blocks behind the run included,
and the clamped first fill) and the stores, and check() holds the dumped plan (mi_spmk_plan_dump) to them: every row stored by
exactly one run, every loaded and every named column owned by a listed run, lists without duplicates and of live runs only, idle
runs unlisted, and `eligible` = all rows in the loop, LEAN, longest list <= 64.  For both depths, on the cases of
tests/spmk_cases.py (whose plan outcomes are pinned here), the patterns of test_ring_plan's dependency test, and two eligible
patterns of the planner fuzz.

Teeth.  build_run_deps broken in a scratch build, one mutation at a time, and the 68 test_model cases (34 patterns, two depths) run
against it — every failure is the model's "run g loads x[lo..hi], rows of runs .. which are not on its list":
  * cmax without the T-lane over-read (Q[4] + Q[5] - 1 for Q[4] + max(Q[5], T) - 1): 20 fail, ten patterns at both depths —
    band:12000:11, band64, band:12000:12 (a first fill of fewer than T columns at the matrix' start), cut, empty:head, empty:mid,
    empty:tail (an empty block brings nothing and loads T lanes), svar:200000:2000, s15:200000:empty-rows, band:120000:40.  The
    narrow bands survive it: with one or two blocks per run every block's new columns are T or more.
  * cmin from the columns the run's rows name instead of Q[4] (the window's first fill starts as low as the ring allows, below
    them): 52 fail, 26 patterns at both depths.  What survives has one or two runs (band:1:0, 2:1, 256:1, 257:1), lists that hold
    every live run anyway (fuzz:19), or no lists at all (long:2049, s15:400000:4000, s15:200000:60000).
No mutation survives the file.  mi_spmk_plan_probe's own replay fails on the same patterns (its side of the comparison was not
touched): the model adds no case there, it adds a second, independent statement of the loads — a change to the kernel's side, or to
both sides of the probe at once, is what only the model sees."""
import numpy as np
import pytest

import spmk_cases as C
import spmk_model as M
from navierstokes_amd import mpk, synth
from test_planner_fuzz import random_pattern


def narrow(n, hb):
    i = np.arange(n, dtype=np.int64)
    cols = np.stack([i + d for d in range(-hb, hb + 1)], axis=1)
    ok = (cols >= 0) & (cols < n)
    return n, np.concatenate([[0], np.cumsum(ok.sum(axis=1))]).astype(np.int32), cols[ok].astype(np.int32)


def with_empty_rows(n):
    """test_ring_plan's: every seventh row empty, and a stretch of 3000 empty rows"""
    p, c, _ = synth.rows("s15", n)
    rows = np.repeat(np.arange(n), np.diff(p).astype(np.int64))
    keep = ~((rows % 7 == 3) | ((rows >= 50_000) & (rows < 53_000)))
    cnt = np.bincount(rows[keep], minlength=n)
    return n, np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32), c[keep]


def synth_rows(kind, n, w):
    p, c, _ = synth.rows(kind, n, w=w)
    return n, p, c


def fuzz(seed):
    """pattern `seed` of test_planner_fuzz.test_powers_step_dependencies_on_random_patterns"""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.choice([7, 300, 5000, 20000, 60000, 200000]))
    p, c = random_pattern(rng, n)
    return n, p, c


# the patterns of test_ring_plan.test_one_launch_powers_step_dependencies_cover_every_load (of its two 1 M-row ones the narrow band,
# whose over-read ADVICE r3 found), and two of the planner fuzz that are eligible.  name: (builder, eligible)
OTHERS = {
    "s15:300000:2000": (lambda: synth_rows("s15", 300_000, 2000), True),
    "svar:200000:2000": (lambda: synth_rows("svar", 200_000, 2000), True),
    "s15:60000:300": (lambda: synth_rows("s15", 60_000, 300), True),
    "s15:400000:2400": (lambda: synth_rows("s15", 400_000, 2400), True),
    "s15:400000:4000": (lambda: synth_rows("s15", 400_000, 4000), False),
    "s15:200000:empty-rows": (lambda: with_empty_rows(200_000), True),
    "s15:200000:60000": (lambda: synth_rows("s15", 200_000, 60_000), False),
    "band:1000000:1": (lambda: narrow(1_000_000, 1), True),
    "band:300000:3": (lambda: narrow(300_000, 3), True),
    "band:120000:40": (lambda: narrow(120_000, 40), True),
    "fuzz:5": (lambda: fuzz(5), True),     # 5000 rows of 0..2 entries, a quarter of them empty: 20 blocks of 256 rows
    "fuzz:19": (lambda: fuzz(19), True),   # 5000 rows of 0..18 entries: 25 blocks
}

_plans = {}


def plan_of(name):
    """(n, p, c, probe's (eligible, runs, max_deps), dump) — built once per pattern, shared by both depths"""
    if name not in _plans:
        n, p, c = C.build(name)[:3] if name in C.EXPECT else OTHERS[name][0]()
        p = np.ascontiguousarray(p, np.int32)
        c = np.ascontiguousarray(c, np.int32)
        _plans[name] = (n, p, c, mpk.spmk_plan_probe(n, p, c), mpk.spmk_plan_dump(n, p, c))
    return _plans[name]


@pytest.mark.parametrize("name", C.CASES)
def test_case_plans(name):
    """every case sits where spmk_cases says it does"""
    n, p, c, (e, runs, md), d = plan_of(name)
    assert (e, d["nblk"], d["bpw"], md, d["uniform"]) == C.EXPECT[name], name
    assert d["wgs"] == 512 and (runs == 512 or not d["in_loop"])


def test_case_plans_reach_their_limits():
    """... and the limit each case is there for shows in its plan"""
    def st(nm, D=2):
        n, p, c, (e, runs, md), d = plan_of(nm)
        return M.check(d, n, p, c, D, e, md), d
    assert st("band:1:0")[0]["live"] == 1 and st("band:1:0")[0]["idle"] == 511         # one run that waits for itself
    assert st("band:2000:7")[0]["live"] == 16 and st("band:2000:7")[0]["max_list"] == 16  # every run lists every run
    assert st("band:131072:1")[0]["idle"] == 0 and st("band:131073:1")[0]["idle"] == 255   # bpw 1 -> 2: half the grid idle
    assert not st("cut")[1]["uniform"] and st("jump")[1]["uniform"] and st("swap")[1]["uniform"]
    sizes = np.diff(st("cut")[1]["run_rng"], axis=1).ravel()
    assert (np.bincount(sizes) == [253, 2, 257]).all()                                     # the forced cut: two runs of one block
    for nm in ("empty:head", "empty:mid", "empty:tail"):
        assert st(nm)[0]["empty_runs"] >= 1, nm                                            # a run of empty blocks only
    assert not st("long:2049")[0]["all_in_loop"] and not st("long:2049")[1]["in_loop"]     # the long row is a PLAIN block


@pytest.mark.parametrize("D", [2, 4])
@pytest.mark.parametrize("name", C.CASES + list(OTHERS))
def test_model(name, D):
    n, p, c, (e, runs, md), d = plan_of(name)
    if name in OTHERS:
        assert e == OTHERS[name][1], (name, e, md)
    got = M.check(d, n, p, c, D, e, md if d["in_loop"] else None)
    assert got["all_in_loop"] or not d["in_loop"], (name, got)
