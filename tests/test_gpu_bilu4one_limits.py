"""The one-launch form of the block ILU solve (bilu4_solve_one.hpp) at every limit of its hand-off between workgroups, bit for bit
(uint64 views) against the model's solve (tests/bilu4_model.py); every x is filled with NaN before the solve, so a row read before
its producer stored it shows.  A consumer chunk polls the flags of its dependencies with one lane per dependency, at most 256; with
more than 64 the polls span several waves and a workgroup barrier has to stand between them and wave 0's acquire.  The patterns of
bilu4one_cases.LIMIT_CASES (their shapes are pinned without a GPU by tests/test_bilu4one_plan.py):

  fan:k       k = 63, 64, 65, 128, 129, 255, 256: one chunk per sweep that waits for exactly k others — one lane short of a wave of
              polls, exactly one, one lane of a second wave; two waves and a third; one lane short of the workgroup; every lane (the cap)
  fan_late:k  k = 64, 65, 256: the same count, but the dependency listed LAST (polled by lane k - 1: the last lane of wave 0, the
              first of wave 1, the last of the workgroup) finishes long after all others, behind a folded chain of single-row
              levels: a poll that leaves that lane out reads a row of NaN.  The tests never rely on timing to pass, only to fail.
  spread:k    k = 65, 256: the k dependencies come from 64 rows of at most 4 blocks each — the polling lanes are not the rows' lanes

each with 2, 7 and the default number of persistent workgroups (2 and 7: every workgroup owns many chunks of a sweep, dealt round
robin, 7 being coprime to the chunk size and to every k; default: one chunk each up to the CU count, so the k = 255 and 256 cases
deal two chunks to some workgroups and one to the others).  Then: NaN and Inf in a row that only a lane >= 64 polls; two handles on
form 1 on two streams at once (each has its own flags, counter and epoch); the cap of 256 from both sides on the device.
No test makes a wait give up: that path stays read, not provoked (tests/test_gpu_bilu4one.py).
Wall time of the file on an MI355X: 10 s (44 tests), most of it the model; k = 128 and 129 are kept (profiles/NOTES.md R7.2)."""
import functools

import numpy as np
import pytest

import bilu4_model as M
import bilu4one_cases as C1
import bilu4one_model as M1
from bilu4_cases import case_id
from conftest import assert_bit_equal
from test_gpu_bilu4one import _form0, _handle, _model_solve, _rhs, _same

pytestmark = pytest.mark.gpu
WGS = ("2", "7", None)  # MI355_BILU_ONE_WGS


def _nan(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _wants(name):
    """The model's results for one pattern, computed once and shared by the workgroup settings: dict(rhs, random, edge, second,
    third, refactored, max_deps)."""
    nb, bp, bc, _ = C1.matrix(name)
    fac = C1.model_factor(name, 0)
    ptr, col, diag, _ = fac
    sched = M.schedule(nb, ptr, col, diag, False), M.schedule(nb, ptr, col, diag, True)  # the pattern's: shared by all the solves
    rhs = _rhs(nb)
    out = dict(rhs=rhs, random=M.solve(nb, *fac, rhs["random"], sched), edge=M.solve(nb, *fac, rhs["edge"], sched))
    out["second"] = M.solve(nb, *fac, out["random"], sched)
    out["third"] = M.solve(nb, *fac, out["second"], sched)
    out["refactored"] = M.solve(nb, *C1.model_factor(name, 0, 1), rhs["edge"], sched)
    out["max_deps"] = tuple(M1.plan(nb, bp, bc, 0)["max_deps"])
    return out


@pytest.mark.parametrize("wgs", WGS, ids=lambda w: f"wgs{w}")
@pytest.mark.parametrize("case", C1.LIMIT_CASES, ids=case_id)
def test_limit_patterns_equal_the_model_and_form_0(case, wgs):
    import torch
    name, fill = case
    nb, bp, bc, bv = C1.matrix(name)
    n = 4 * nb
    W = _wants(name)
    rhs = W["rhs"]
    F = _handle(wgs, nb, bp, bc, bv, fill)
    what = f"{name} workgroups {wgs}"
    one = F.info_one()
    assert one["max_deps"] == W["max_deps"] and one["max_deps"][0] == max(one["max_deps"]) == C1.limit_k(name), one
    for k in ("random", "edge"):
        db, dx = _dev(rhs[k]), _nan(n)
        F.solve(dx, db)
        _same(dx.cpu().numpy(), W[k], f"{what} b={k} out of place")
        assert_bit_equal(db.cpu().numpy(), rhs[k], "b was written")
        F.solve(db, db)
        _same(db.cpu().numpy(), W[k], f"{what} b={k} in place")
    _same(_form0(F, _dev(rhs["random"])), W["random"], f"{what} form 0 on the same handle")
    # three solves back to back on a side stream, each consuming the one before: flags of the earlier epoch must not satisfy the later
    st = torch.cuda.Stream()
    d1, (x1, x2, x3) = _dev(rhs["random"]), (_nan(n) for _ in range(3))
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        F.solve(x1, d1)
        F.solve(x2, x1)
        F.solve(x3, x2)
    st.synchronize()
    _same(x1.cpu().numpy(), W["random"], f"{what} back to back, first")
    _same(x2.cpu().numpy(), W["second"], f"{what} back to back, second")
    _same(x3.cpu().numpy(), W["third"], f"{what} back to back, third")
    F.refactor(C1.new_values(name, 1))
    dx = _nan(n)
    F.solve(dx, _dev(rhs["edge"]))
    _same(dx.cpu().numpy(), W["refactored"], f"{what} after refactor")
    assert F.info()["form"] == 1
    F.one_status()
    F.close()


@pytest.mark.parametrize("name", [c[0] for c in C1.LIMIT_CASES if C1.limit_k(c[0]) >= 255])
def test_the_default_grid_deals_more_than_one_chunk_to_a_workgroup(name):
    """More chunks per sweep than the default grid has workgroups (one per CU at the most): on any device of at most 256 CUs some
    workgroups own two chunks of a sweep and the others one."""
    nb, bp, bc, bv = C1.matrix(name)
    F = _handle(None, nb, bp, bc, bv, 0)
    one = F.info_one()
    if not one["workgroups"] < max(one["nchunks"]):
        F.close()
        pytest.skip(f"{one['workgroups']} workgroups for {one['nchunks']} chunks: this device has more CUs than {name} has chunks")
    W = _wants(name)
    dx = _nan(4 * nb)
    F.solve(dx, _dev(W["rhs"]["edge"]))
    _same(dx.cpu().numpy(), W["edge"], f"{name} on {one['workgroups']} workgroups")
    F.one_status()
    F.close()


def _far_rows(name):
    """Block rows of producer chunks that only a lane >= 64 polls (the consumer's dependency list is 0 .. k - 1 in both patterns, and
    diagonal row r lies in chunk r // 64 of the forward sweep: tests/test_bilu4one_plan.py)."""
    k = C1.limit_k(name)
    if name.startswith("fan:"):
        rows = [64 * (k - 1) + 6] * 3  # the one row of chunk k - 1 = 64 that both consumers name
    else:
        links = dict((j // 64, j) for i, j in C1.spread_links(k) if i < 64 * k + 64)
        rows = [links[69], links[133], links[255]]
    assert all(r // 64 >= 64 for r in rows)
    return rows


@pytest.mark.parametrize("name", ["fan:65", "spread:256"])
def test_nan_and_inf_behind_a_lane_of_a_later_wave_reach_the_rows_the_model_says(name):
    nb, bp, bc, bv = C1.matrix(name)
    fac = C1.model_factor(name, 0)
    n = 4 * nb
    for wgs in ("2", None):
        F = _handle(wgs, nb, bp, bc, bv, 0)
        for q, (row, bad) in enumerate(zip(_far_rows(name), (np.nan, np.inf, -np.inf))):
            b = np.random.default_rng(row + q).standard_normal(n)
            b[4 * row + q] = bad
            dx = _nan(n)
            F.solve(dx, _dev(b))
            got, want = dx.cpu().numpy(), _model_solve(fac, nb, b)
            _same(got, want, f"{name} {bad} in block row {row}, workgroups {wgs}")
            # the consumer rows behind the poisoned one: more rows than the poisoned one itself are not finite
            assert (~np.isfinite(want.reshape(nb, 4)).all(axis=1)).sum() >= 2, "the special value does not cross a hand-off in the model"
        F.one_status()
        F.close()


def test_two_handles_on_form_1_on_two_streams():
    """fan_late:65 and spread:65, three solves each (each consuming the one before), enqueued alternately with no synchronise in
    between.  Each handle has its own flags, counter and epoch; both grids together stay below the CU count, so residency is not in
    question."""
    import torch
    names = ("fan_late:65", "spread:65")
    Fs = [_handle(None, *C1.matrix(name), 0) for name in names]
    assert sum(F.info_one()["workgroups"] for F in Fs) < torch.cuda.get_device_properties(0).multi_processor_count
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    xs = [[_dev(_wants(name)["rhs"]["random"])] + [_nan(4 * F.nbrows) for _ in range(3)] for name, F in zip(names, Fs)]
    torch.cuda.synchronize()
    for s in range(3):
        for F, st, x in zip(Fs, streams, xs):
            with torch.cuda.stream(st):
                F.solve(x[s + 1], x[s])
    torch.cuda.synchronize()
    for name, F, x in zip(names, Fs, xs):
        for s, key in enumerate(("random", "second", "third")):
            _same(x[s + 1].cpu().numpy(), _wants(name)[key], f"{name} beside the other handle, solve {s}")
        F.one_status()
        F.close()


def test_the_cap_of_256_dependencies_from_both_sides():
    """fan:256 solves in one launch; fan:257 refuses form 1 (status 5), stays on form 0 and still solves — checked against the
    pattern done by hand: t = b but for the last row, which subtracts its L blocks in ascending column order; x_i = Dinv_i t_i but
    for row 0, which first subtracts its U blocks times x, in ascending column order."""
    from navierstokes_amd import mpk
    nb, bp, bc, bv = C1.matrix("fan:256")
    F = _handle(None, nb, bp, bc, bv, 0)
    assert F.info_one()["max_deps"] == (256, 256)
    W = _wants("fan:256")
    dx = _nan(4 * nb)
    F.solve(dx, _dev(W["rhs"]["random"]))
    _same(dx.cpu().numpy(), W["random"], "fan:256 on form 1")
    F.one_status()
    F.close()

    nb, bp, bc, bv = C1.matrix(C1.FAN_OVER_CAP[0])
    F = mpk.bilu4(nb, bp, bc, bv, fill=0)
    with pytest.raises(mpk.MiError) as e:
        F.set_form(1)
    assert e.value.status == 5 and "256" in str(e.value) and "257" in str(e.value)
    assert F.info()["form"] == 0 and F.info_one()["eligible"] is False and F.info_one()["max_deps"] == (257, 257)
    ptr, col, diag, val = F.factor_host()
    b = np.random.default_rng(10).standard_normal(4 * nb)
    t = b.reshape(nb, 4).copy()
    for k in range(ptr[nb - 1], diag[nb - 1]):
        t[nb - 1] = t[nb - 1] - M.matvec4(val[k], t[col[k]])
    x = M.matvec4(val[diag], t)
    s = t[0].copy()
    for k in range(diag[0] + 1, ptr[1]):
        s = s - M.matvec4(val[k], x[col[k]])
    x[0] = M.matvec4(val[diag[0]], s)
    dx = _nan(4 * nb)
    F.solve(dx, _dev(b))
    assert_bit_equal(dx.cpu().numpy(), x.reshape(-1), "fan:257 on form 0")
    F.close()
