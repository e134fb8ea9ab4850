"""mi_maxpy_upto_dev / mi_maxpy_upto_f32_dev (mpk.maxpy_upto) on the GPU: the multi-AXPY whose vector count the KERNELS read from
device memory, so that the update of a GMRES cycle can sit in a graph.  Every result is compared, bit for bit, with mpk.maxpy
(mi_maxpy_dev / mi_maxpy_f32_dev) on the first c vectors, c the count clamped to [0, m].

  sizes      n in {1, 2, 511, 513, 1025} (one lane, one pair, one segment short of / past a workgroup's 512 elements, three
             segments with an odd tail), m in {1, 8, 9, 17, 64} (one chunk, a full tile, one over, three chunks, the most),
             count in {-2, 0, 1, 7, 8, 9, m - 1, m, m + 3}, negate 0 and 1, y 16-byte aligned and offset by one double, the double
             and the float basis
  not read   every basis vector and every coefficient with index >= c is NaN: none may reach y
  count 0    y, with entries of -0.0, keeps every bit
  large      n = 2 000 001 once: the non-temporal path
  captured   ONE graph, replayed with the count changed in device memory between replays — what the kernel exists for"""
import numpy as np
import pytest

from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

NS = (1, 2, 511, 513, 1025)
MS = (1, 8, 9, 17, 64)


def _counts(m):
    return sorted({-2, 0, 1, 7, 8, 9, m - 1, m, m + 3})


def _setup(n, m, seed):
    """(V32 [m, ld], V64 = widen(V32), coef [m], y0 [n]) with entries of mixed magnitude; ld even: every float row is 8-byte aligned."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    ld = n + (n & 1)
    V32 = torch.randn((m, ld), dtype=torch.float32, device="cuda", generator=g)
    coef = torch.randn(m, dtype=torch.float64, device="cuda", generator=g)
    y0 = torch.randn(n, dtype=torch.float64, device="cuda", generator=g) * torch.exp(3.0 * torch.randn(n, dtype=torch.float64, device="cuda", generator=g))
    return V32, V32.double(), coef, y0


def _placed(y, offset):
    import torch
    buf = torch.zeros(y.numel() + 2, dtype=torch.float64, device="cuda")
    out = buf[offset: offset + y.numel()]
    assert out.data_ptr() % 16 == 8 * offset
    out.copy_(y)
    return out


def _same(got, want, what):
    import torch
    if not torch.equal(got.view(torch.int64), want.view(torch.int64)):
        assert_bit_equal(got.cpu().numpy(), want.cpu().numpy(), what)


def _poisoned(V, coef, c):
    """Copies in which everything the call must not read is NaN."""
    Vp, cp = V.clone(), coef.clone()
    Vp[c:] = float("nan")
    cp[c:] = float("nan")
    return Vp, cp


def _case(n, m, V, coef, y0, count_t, counts, offsets=(0, 1), negates=(False, True)):
    from navierstokes_amd import mpk
    for count in counts:
        c = min(max(count, 0), m)
        count_t.fill_(count)
        Vp, cp = _poisoned(V, coef, c)
        rows, rows_p = [V[j, :n] for j in range(m)], [Vp[j, :n] for j in range(m)]
        for offset in offsets:
            for negate in negates:
                what = f"{str(V.dtype)[6:]} basis, n {n} m {m} count {count} y offset {offset} negate {negate}"
                want, got = _placed(y0, offset), _placed(y0, offset)
                mpk.maxpy(coef[:c], rows[:c], want, negate=negate)
                assert mpk.maxpy_upto(count_t, cp, rows_p, got, negate=negate) is got
                _same(got, want, what)
                if c == 0:
                    _same(got, y0, what + ": y untouched")


@pytest.mark.parametrize("n", NS)
def test_equal_to_maxpy_at_the_clamped_count(n):
    import torch
    count_t = torch.zeros(1, dtype=torch.int32, device="cuda")
    for m in MS:
        V32, V64, coef, y0 = _setup(n, m, 300 + 7 * n + m)
        y0[::3] = -0.0  # (count 0 must keep the sign of a zero)
        for V in (V64, V32):
            _case(n, m, V, coef, y0, count_t, _counts(m))


def test_non_temporal_path():
    import torch
    n, m = 2_000_001, 3
    count_t = torch.zeros(1, dtype=torch.int32, device="cuda")
    V32, V64, coef, y0 = _setup(n, m, 17)
    for V in (V64, V32):
        _case(n, m, V, coef, y0, count_t, (2,), offsets=(0,), negates=(True,))


def test_m_zero_and_an_empty_vector_do_nothing():
    import torch
    from navierstokes_amd import mpk
    count_t = torch.ones(1, dtype=torch.int32, device="cuda")
    y = torch.full((5,), -0.0, dtype=torch.float64, device="cuda")
    mpk.maxpy_upto(count_t, torch.zeros(1, dtype=torch.float64, device="cuda"), [], y)
    torch.cuda.synchronize()
    assert_bit_equal(y.cpu().numpy(), np.full(5, -0.0), "m = 0")


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_one_graph_replayed_with_the_count_changed_on_the_device(f32):
    """The call is captured ONCE, on a stream that never reduced (it needs no workspace); between replays only the word in device
    memory changes."""
    import torch
    from navierstokes_amd import mpk
    n, m = 1025, 17
    V32, V64, coef, y0 = _setup(n, m, 5)
    V = V32 if f32 else V64
    rows = [V[j, :n] for j in range(m)]
    count_t = torch.full((1,), 4, dtype=torch.int32, device="cuda")
    y, want = y0.clone(), y0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        mpk.maxpy_upto(count_t, coef, rows, y, negate=True)
    for count in (0, 3, 9, 17, 20, -1, 8, 16):
        c = min(max(count, 0), m)
        count_t.fill_(count)
        y.copy_(y0)
        g.replay()
        want.copy_(y0)
        mpk.maxpy(coef[:c], rows[:c], want, negate=True)
        torch.cuda.synchronize()
        _same(y, want, f"replay with count {count}")
