"""The block DILU sweeps (mi_dilu4_*, dilu4_kernels.hpp) at every limit of their pipeline and of their launches, on the patterns of
tests/dilu4_limit_cases.py, BIT for bit against tests/dilu4_model.py.  tests/test_dilu4_limit_cases.py shows, without a GPU, that the
patterns have these limits and that a dropped block changes the expected bits.

  sweeps     to_hat, from_hat and apply_hat on every case in natural and in colour order, outputs pre-filled with NaN, the input
             left unwritten, and in place.  What each case adds over the sweep cases of tests/test_gpu_dilu4.py:
               wide          dilu4_level (unfolded) rows with 4, 5, 8, 9, 10..13 blocks LEFT of the diagonal and 5..15, 17, 18, 22
                             RIGHT of it (there: 1, 3, 7 left; 1, 2, 3, 4, 7 right); levels of 127, 128 and 129 rows.  In natural
                             order the level kernels run on the caller's own vectors
               limits:3      dilu4_folded rows with 2, 4..16 blocks RIGHT of the diagonal; unfolded rows with up to 12
               limits:3~     dilu4_folded rows with 2, 4..16 blocks LEFT of the diagonal (there: 0, 1, 3, 7 and 64, 65, 200)
               fold_deep     natural: ONE dilu4_folded launch of 252 levels per sweep, a barrier per level
               alternating   natural: 48 launches per sweep, dilu4_folded and dilu4_level in turn
               wide:63/64/65 ONE level: the widest that folds, exactly one workgroup, one quad in a second workgroup
               tiny:1/16/17  matrices of one quad, one wave of quads and one quad over (levels of 16 and 17 rows are fold_deep's)
  alignment  on `wide` and the tiny chains, in both orders, input and output each 16-byte aligned or offset by 8 bytes, all four
             combinations, on a non-default stream, and in place at both offsets; the doubles around every vector stay untouched
  refactor   a graph of the three operations, captured once, replays the values of the LAST refactor: the device arrays keep
             their addresses
  gmres      the solver on the DILU operator against the composed loop of tests/test_gpu_gmres_dev.py with apply_hat as the product,
             on the chain in colour order (two levels of 75 rows: every launch is dilu4_level) and on `wide` in natural order:
             eager with check_every 1 and 4, and one captured cycle replayed twice
  empty      a device handle on an empty matrix: every operation is a no-op that returns 0"""
import functools

import numpy as np
import pytest

import bilu4_cases as C
import dilu4_limit_cases as LC
import dilu4_model as DM
import test_gpu_gmres_dev as T
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

OPS = ("to_hat", "from_hat", "apply_hat")
ORDERS = ("natural", "colour")
SWEEP_CASES = [(name, order) for name in LC.NAMES for order in ORDERS]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()  # (a copy: the shared expectations are read-only)


def _poisoned(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


@functools.lru_cache(maxsize=None)
def expected(name, order, variant=0):
    """(u, {op: the model's result}) — computed once, read-only."""
    m = LC.model(name, order, variant)
    u = np.random.default_rng(300).uniform(-1.0, 1.0, 4 * m.nb)
    out = {op: getattr(m, op)(u) for op in OPS}
    for v in (u, *out.values()):
        v.setflags(write=False)
    return u, out


def _handle(name, order, variant=0):
    from navierstokes_amd import mpk
    nb, bp, bc, _ = LC.matrix(name)
    return mpk.dilu4(nb, bp, bc, LC.values(name, variant), order=order)


# ---------------------------------------------------------------- the three sweeps on every case

@pytest.mark.parametrize("name,order", SWEEP_CASES, ids=[f"{n}-{o}" for n, o in SWEEP_CASES])
def test_the_three_operations_are_the_models(name, order):
    u, want = expected(name, order)
    n = u.size
    E = _handle(name, order)
    try:
        assert E.info()["device_bytes"] > 0
        du = _dev(u)
        for op in OPS:
            out = _poisoned(n)
            getattr(E, op)(out, du)
            assert_bit_equal(out.cpu().numpy(), want[op], f"{name} {order} {op}")
            assert_bit_equal(du.cpu().numpy(), u, f"{name} {order} {op}: the input was written")
            inplace = du.clone()
            getattr(E, op)(inplace, inplace)
            assert_bit_equal(inplace.cpu().numpy(), want[op], f"{name} {order} {op}: in place")
    finally:
        E.close()


# ---------------------------------------------------------------- alignment

@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ["wide", "tiny:1", "tiny:16", "tiny:17"])
def test_every_pairing_of_alignments(name, order):
    """Which kernel form (AL: 16-byte loads and stores; or 8-byte ones) a pairing reaches.  Natural order: to_hat and from_hat run
    their level kernels on the caller's OUTPUT, so its alignment alone picks the form, and the input is only ever read entry by
    entry; apply_hat sweeps over the handle's own aligned vectors whatever the caller passes.  Ordered: every level kernel runs on the
    handle's aligned vector; the gather picks its form by the input and the scatter by the output, so the mixed pairings are the only
    ones that run one form of each.  The 8-byte forms of those two have four lanes per block row: the 16 rows of tiny:16 are exactly
    one wave of them, tiny:17 one quad over."""
    import torch
    u, want = expected(name, order)
    n = u.size
    E = _handle(name, order)
    st = torch.cuda.Stream()
    FRONT, BACK = -3.0, -5.0  # what stands around each vector

    def carve(offset, fill):
        """(buffer, the n doubles from 2 + offset on): 16-byte aligned for offset 0, 8 bytes off for offset 1."""
        buf = torch.full((n + 4,), fill, dtype=torch.float64, device="cuda")
        buf[1 + offset], buf[2 + offset + n] = FRONT, BACK
        v = buf[2 + offset: 2 + offset + n]
        assert v.data_ptr() % 16 == 8 * offset
        return buf, v

    def untouched(buf, offset, what):
        assert (float(buf[1 + offset].item()), float(buf[2 + offset + n].item())) == (FRONT, BACK), f"{what}: written outside the vector"

    try:
        for op in OPS:
            for off_in in (0, 1):
                for off_out in (0, 1):
                    what = f"{name} {order} {op}: input offset {off_in}, output offset {off_out}"
                    buf_in, vin = carve(off_in, 0.0)
                    buf_out, vout = carve(off_out, float("nan"))
                    vin.copy_(_dev(u))
                    torch.cuda.synchronize()
                    with torch.cuda.stream(st):
                        getattr(E, op)(vout, vin)
                    st.synchronize()
                    assert_bit_equal(vout.cpu().numpy(), want[op], what)
                    assert_bit_equal(vin.cpu().numpy(), u, what + ": the input was written")
                    untouched(buf_in, off_in, what)
                    untouched(buf_out, off_out, what)
                what = f"{name} {order} {op}: in place at offset {off_in}"
                with torch.cuda.stream(st):
                    getattr(E, op)(vin, vin)
                st.synchronize()
                assert_bit_equal(vin.cpu().numpy(), want[op], what)
                untouched(buf_in, off_in, what)
    finally:
        E.close()


# ---------------------------------------------------------------- a captured graph across a refactor

@pytest.mark.parametrize("name", ["wide", "limits:3~"])
def test_a_captured_graph_replays_the_last_refactor(name):
    import torch
    order = "natural"
    u, want0 = expected(name, order)
    _, want1 = expected(name, order, variant=1)
    assert not any(np.array_equal(want0[op], want1[op]) for op in OPS)
    n = u.size
    E = _handle(name, order)
    du = _dev(u)
    outs = {op: _poisoned(n) for op in OPS}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for op in OPS:
            getattr(E, op)(outs[op], du)
    try:
        for step, (variant, want) in enumerate(((0, want0), (1, want1), (0, want0))):
            if step:
                E.refactor(LC.values(name, variant))  # no new capture
            for op in OPS:
                outs[op].fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            for op in OPS:
                assert_bit_equal(outs[op].cpu().numpy(), want[op], f"{name} {op}: replayed, step {step}, the values of variant {variant}")
            assert_bit_equal(du.cpu().numpy(), u, "the input was written")
    finally:
        E.close()


# ---------------------------------------------------------------- GMRES through an unfolded level

RESTART = 5
GMRES_CASES = [("chain", "colour"), ("wide", "natural")]


@pytest.fixture
def apply_hat_is_the_product(monkeypatch):
    """As in tests/test_gpu_dilu4.py: the composed loop's product on a dilu4 is its public apply_hat."""
    from navierstokes_amd import mpk
    plain = mpk.SpMV_CSR
    monkeypatch.setattr(mpk, "SpMV_CSR", lambda y, x, A: A.apply_hat(y, x) if isinstance(A, mpk.dilu4) else plain(y, x, A))


def _gmres_matrix(name):
    return C.matrix("chain") if name == "chain" else LC.matrix(name)


def _hat_system(name, order):
    """(E, b^, u0) after asserting what the case is here for: launches of dilu4_level inside the solver."""
    from navierstokes_amd import mpk
    nb, bp, bc, bv = _gmres_matrix(name)
    B = DM.Ordered(nb, bp, bc, bv, order).B if name == "chain" else LC.model(name, order).B
    plan = mpk.bilu4_plan_probe(nb, B.ptr, B.col, 0)
    sizes = list(plan["fwd_sizes"]) + list(plan["bwd_sizes"])
    if name == "chain":  # two colours of 75 rows: no folded launch at all
        assert sizes == [75] * 4 and plan["fwd_launches"] == plan["bwd_launches"] == 2, plan
    else:  # unfolded levels with every count of WANTED, and the folded ones between them
        assert sum(s >= LC.FOLD_BELOW for s in sizes) == 22 and plan["fwd_launches"] == 13, plan
    E = mpk.dilu4(nb, bp, bc, bv, order=order)
    bhat = _dev(T._rhs(4 * nb))
    E.to_hat(bhat, bhat)
    return E, bhat, _dev(np.zeros(4 * nb))


def _assert_what_the_matrix_gives(name, want, maxiter):
    """What is true of the composed loop on these two matrices.  Both are strongly diagonally dominant (tests/bilu4_cases.py,
    _values), so the preconditioned operator is close to the identity: in the first cycle every step takes at least a factor of ten
    off the recurrence's residual (the chain about 100, `wide` about 300).  rtol 1e-30 lies below what double precision reaches
    (the true residual a later cycle starts from is near 1e-18), so no cycle ends early and the solve ends at maxiter with reason 2,
    its last cycle maxiter mod restart steps long (a whole cycle where that is 0)."""
    print(f"dilu4 gmres {name}: composed loop {want[0]} iterations, reason {want[2]}, last cycle of {want[4][0]}, history {want[1]}")
    hist = want[1]
    assert (want[0], want[2], want[4][0]) == (maxiter, 2, maxiter % RESTART or RESTART), want[:3]
    assert len(hist) == maxiter + 1 and np.isfinite(hist).all() and np.isfinite(want[3]).all()
    assert all(hist[k + 1] < hist[k] / 10 for k in range(RESTART)), hist


@pytest.mark.parametrize("check_every", [1, 4])
@pytest.mark.parametrize("name,order", GMRES_CASES, ids=[f"{n}-{o}" for n, o in GMRES_CASES])
def test_gmres_through_unfolded_levels_is_the_composed_loop(name, order, check_every, apply_hat_is_the_product):
    E, bhat, u0 = _hat_system(name, order)
    try:
        want = T.composed(E, None, bhat, u0, RESTART, 1e-30, 12)
        got = T.solver_run(E, None, bhat, u0, RESTART, 1e-30, 12, check_every=check_every)
        _assert_what_the_matrix_gives(name, want, 12)
        T.assert_same_solve(got, want, f"{name} {order} check_every {check_every}")
    finally:
        E.close()


@pytest.mark.parametrize("name,order", GMRES_CASES, ids=[f"{n}-{o}" for n, o in GMRES_CASES])
def test_one_captured_cycle_through_unfolded_levels(name, order, apply_hat_is_the_product):
    import torch
    from navierstokes_amd import mpk
    E, bhat, u0 = _hat_system(name, order)
    S = None
    try:
        # maxiter = restart: exactly one cycle, which ends at the restart or where the recurrence freezes it
        want = T.composed(E, None, bhat, u0, RESTART, 1e-30, RESTART)
        _assert_what_the_matrix_gives(name, want, RESTART)
        assert want[0] == want[4][0]
        S = mpk.gmres_solver(E, None, RESTART)
        u = u0.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            S.prepare_stream()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            S.cycle(bhat, u, True, 1e-30, RESTART)
        for _ in range(2):
            u.copy_(u0)
            g.replay()
            torch.cuda.synchronize()
            st = S.state()
            assert (st["its"], st["k"]) == (want[0], want[0]), st
            assert_bit_equal(st["history"], want[1][1:], f"{name} {order}: the captured cycle's history")
            assert_bit_equal(u.cpu().numpy(), want[3], f"{name} {order}: the captured cycle's x")
    finally:
        if S is not None:
            S.close()
        E.close()


# ---------------------------------------------------------------- an empty matrix

@pytest.mark.parametrize("order", ORDERS)
def test_a_device_handle_on_an_empty_matrix(order):
    from navierstokes_amd import mpk
    L = mpk.lib()
    E = mpk.dilu4(0, [0], [], [], order=order)
    info = E.info()
    assert info["nbrows"] == 0 and info["nblocks"] == 0 and info["order"] == order and info["device_bytes"] == 0, info
    for fn in (L.mi_dilu4_to_hat_dev, L.mi_dilu4_from_hat_dev, L.mi_dilu4_apply_hat_dev):
        assert fn(E.handle, None, None, None) == 0
    assert L.mi_dilu4_refactor(E.handle, None, 0) == 0
    assert E.refactor([]) is E
    einv, k = E.fetch()
    assert einv.shape == (0, 4, 4) and k.shape == (0, 4, 4)
    E.close()
