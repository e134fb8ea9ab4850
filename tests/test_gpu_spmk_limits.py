"""The one-launch powers step (spmk_ring.hpp, launch_spmk.hip) at every limit of its plan and of its hand-off, on the device.
tests/test_spmk_model.py holds the plan's dependency lists to a host model of the kernel's loads; this file runs the kernel on the
same cases (tests/spmk_cases.py: one run that waits for itself, runs of one block — all sentinel pipeline under D = 4 —, 512 / 513
blocks, a forced cut (the run_rng form of the launch), runs of empty blocks only, lists of 61 / 64 entries and the 65 that are
refused, a row of 2048 nonzeros and the 2049 that are refused), in all eight instantiations launch_fused can pick, at k on both sides
of 2 and kSpmkFusedMaxK, off 16-byte alignment, on side streams, and with the flag epoch crossing 2^31 and 2^32.

Common to all: the handle is set_kernel("ring") with MI355_SPMK_FUSED=1 (but for the measured choice); every output is NaN before
every launch; every launch gets an x the handle has not seen; every power is compared bit for bit with the oracle's k chained
products; before comparing, the handle must say that it ran in one launch (or, for the two refused cases and the refused k, that
it did not), in agreement with mi_spmk_plan_probe as pinned in spmk_cases.EXPECT.

Nothing here makes a wait give up: no spin budget is lowered, nothing blocks the card, and where two one-launch kernels are in
flight at once their live runs together (16 + 94) are far fewer than the 512 workgroups the card holds, the idle ones leaving at
once.  The give-up path stays read, not provoked; tools/spmk_stress.py is the tool for long runs under load.

Largest matrix: 131 073 rows.  Measured on one MI355X: 66 tests, 5.3 s for the file alone (2.3 s of it the child process of
test_epoch_wrap, 0.2 s the slowest of the others)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import spmk_cases as C
from conftest import ROOT, assert_bit_equal
from navierstokes_amd import mpk
from oracle import oracle as O

pytestmark = pytest.mark.gpu

MI_MAX_POWERS = 16   # include/mi355_spmv.h
FUSED_MAX_K = 8      # spmk_ring.hpp: kSpmkFusedMaxK
KSEQ = (2, 8, 3, 4, 8, 2)
DEVLIB = os.path.join(ROOT, "navierstokes_amd", "csrc", "libmi355spmv_dev.so")


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()  # (a copy: the shared inputs are read-only)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    mpk.lib()
    yield


_X, _Y = {}, {}


def x_of(name, i):
    """the i-th input of a case: seeded, shared by every test, never written to"""
    if (name, i) not in _X:
        n = C.build(name)[0]
        x = np.random.default_rng(1 + 7919 * i + sum(name.encode())).uniform(-1.0, 1.0, n)
        x.setflags(write=False)
        _X[name, i] = x
    return _X[name, i]


def chain_of(name, i, k=FUSED_MAX_K):
    """the oracle's A x, .., A^k x for that input — computed once (k = 8 serves every smaller k: power q does not depend on k)"""
    kk = FUSED_MAX_K if k <= FUSED_MAX_K else MI_MAX_POWERS
    if (name, i, kk) not in _Y:
        n, p, c, v = C.build(name)
        Y = O.spmk_chain(kk, p, c, v, x_of(name, i))
        assert np.isfinite(Y).all()
        Y.setflags(write=False)
        _Y[name, i, kk] = Y
    return _Y[name, i, kk]


class Handle:
    """a ring handle of one case that counts the inputs it has had"""

    def __init__(self, name, offset=0):
        self.name = name
        self.n, p, c, v = C.build(name)
        self.A = mpk.csrmatrix(self.n, p, c, v).set_kernel("ring")
        self.A.handle  # created here, under whatever the caller put into the environment
        self.eligible = C.EXPECT[name][0]
        self.i = 0
        self.off = offset  # doubles between a vector and its 16-byte-aligned allocation
        self.bufs = [torch.empty(self.n + offset, dtype=torch.float64, device="cuda") for _ in range(MI_MAX_POWERS)]
        self.xbuf = torch.empty(self.n + offset, dtype=torch.float64, device="cuda")

    def launch(self, k):
        """enqueue one k-step on torch's current stream with the next input; returns what check() needs"""
        i = self.i
        self.i += 1
        x = self.xbuf[self.off:]
        x.copy_(dev(x_of(self.name, i)))
        outs = [b[self.off:] for b in self.bufs[:k]]
        for t in outs:
            t.fill_(float("nan"))
        if self.off:
            assert x.data_ptr() % 16 == 8 and all(t.data_ptr() % 16 == 8 for t in outs)
        mpk.SpMkV(outs, x, self.A)
        return i, k, [t.clone() for t in outs]

    def check(self, launched, what="", one_launch=None, eligible=None):
        i, k, outs = launched
        info = self.A.spmk_info(k)
        can = self.eligible and 2 <= k <= FUSED_MAX_K
        want = (can if one_launch is None else one_launch, can if eligible is None else eligible)
        assert (info["one_launch"], info["eligible"]) == want, (self.name, k, info, self.A.kernel_name(), self.A.ring_shape_info())
        Y = chain_of(self.name, i, k)
        for q in range(k):
            assert_bit_equal(outs[q].cpu().numpy(), Y[q], f"{self.name} {what} input {i}, k = {k}, power {q + 1}")

    def step(self, k, what="", one_launch=None, eligible=None):
        self.check(self.launch(k), what, one_launch, eligible)

    def product(self):
        i = self.i
        self.i += 1
        y = torch.full((self.n,), float("nan"), dtype=torch.float64, device="cuda")
        mpk.SpMV_CSR(y, dev(x_of(self.name, i)), self.A)
        assert_bit_equal(y.cpu().numpy(), chain_of(self.name, i)[0], f"{self.name}: a plain product after the k-steps")

    def close(self):
        self.A.close()


def ring_name(depth, nt, skew):
    """mi_csr_kernel_name of a LEAN configuration-4 handle: the fields launch_fused reads (ring.cfg.depth, ring.nt, ring.skew)"""
    b = {False: "false", True: "true"}
    return f"spmv_csr_ring<256, 2048, 5120, {depth}, 160, false, {b[nt]}, {b[skew]}, false, true, false>"


@pytest.mark.parametrize("depth", [0, 4])
@pytest.mark.parametrize("name", C.CASES)
def test_every_case(name, depth, monkeypatch):
    """k = 2, 8, 3, 4, 8, 2 on one handle (the flags count on from step to step, whatever k was), then a plain product — at the
    depth the planner picks (2: no case has runs of 40 blocks) and at depth 4, where a run of one block is D sentinel blocks for
    every real one.  band:12000:12 and long:2049 are refused and must give the same bits through k launches."""
    monkeypatch.setenv("MI355_SPMK_FUSED", "1")
    if depth:
        monkeypatch.setenv("MI355_RING_DEPTH", str(depth))
    H = Handle(name)
    assert H.A.ring_shape_info()["depth"] == (depth or 2) and "spmv_csr_ring<256," in H.A.kernel_name(), (H.A.kernel_name(), H.A.ring_shape_info())
    for k in KSEQ:
        H.step(k, f"depth {depth or 2}")
    H.product()
    H.close()


@pytest.mark.parametrize("skew", [False, True])
@pytest.mark.parametrize("nt", [False, True])
@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("name", ["band:2000:7", "s15:66000:300"])
def test_every_instantiation(name, depth, nt, skew, monkeypatch):
    """launch_fused picks spmk_csr_ring<256, 2048, 5120, D, kRingMaxB, NT, SKEW> from ring.cfg.depth, ring.nt and ring.skew; left to
    themselves these matrices only ever run <2, false, false>.  All eight, on runs of one block and runs of two; the handle's
    kernel name and depth show the three settings (the same fields feed launch_fused)."""
    monkeypatch.setenv("MI355_SPMK_FUSED", "1")
    monkeypatch.setenv("MI355_RING_DEPTH", str(depth))
    monkeypatch.setenv("MI355_RING_SKEW", "1" if skew else "0")
    H = Handle(name)
    mpk.check(mpk.lib().mi_csr_set_nontemporal(H.A.handle, int(nt), -1))
    assert H.A.kernel_name() == ring_name(depth, nt, skew) and H.A.ring_shape_info()["depth"] == depth, (H.A.kernel_name(), H.A.ring_shape_info())
    for k in KSEQ:
        H.step(k, f"<{depth}, {nt}, {skew}>")
    assert H.A.kernel_name() == ring_name(depth, nt, skew)
    H.close()


@pytest.mark.parametrize("name", ["band:2000:7", "s15:66000:300"])
def test_depth_3_is_refused(name, monkeypatch):
    """there is no one-launch instantiation at D = 3: k launches of the depth-3 ring kernel, same bits"""
    monkeypatch.setenv("MI355_SPMK_FUSED", "1")
    monkeypatch.setenv("MI355_RING_DEPTH", "3")
    H = Handle(name)
    assert H.A.ring_shape_info()["depth"] == 3
    for k in (2, 8, 3):
        H.step(k, "depth 3", one_launch=False, eligible=False)
    H.close()


def test_k_limits(monkeypatch):
    """k = 1 and k > kSpmkFusedMaxK take k launches and leave the epoch alone; 8 is followed by 9 and then 2, so a step that did not
    publish must not have moved what the next one waits for"""
    monkeypatch.setenv("MI355_SPMK_FUSED", "1")
    H = Handle("s15:66000:300")
    for k in (1, 8, 9, 2, MI_MAX_POWERS, FUSED_MAX_K, FUSED_MAX_K + 1, 2, 1, 3):
        H.step(k)
    for k in range(1, MI_MAX_POWERS + 1):
        assert H.A.spmk_info(k)["one_launch"] == (2 <= k <= FUSED_MAX_K), k
    H.close()


def test_off_alignment_and_side_stream(monkeypatch):
    monkeypatch.setenv("MI355_SPMK_FUSED", "1")
    # x and every y one double off 16-byte alignment
    H = Handle("s15:66000:300", offset=1)
    for k in (4, 8, 2):
        H.step(k, "8 bytes off alignment")
    H.close()
    # a fresh handle whose FIRST step is on a side stream: its flags were zeroed on the null stream
    H = Handle("cut")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        done = [H.launch(k) for k in (4, 8, 2)]
    side.synchronize()
    for d in done:
        H.check(d, "side stream")
    H.close()
    # two handles stepping on two streams at once, each with its own flags and epoch (16 + 94 live runs: all resident together)
    Hs = [Handle("band:2000:7"), Handle("jump")]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    done = [[], []]
    for k0, k1 in ((4, 3), (2, 8), (8, 2), (3, 4)):
        for j, k in ((0, k0), (1, k1)):
            with torch.cuda.stream(streams[j]):
                done[j].append(Hs[j].launch(k))
    torch.cuda.synchronize()
    for j in range(2):
        for d in done[j]:
            Hs[j].check(d, f"two streams at once, handle {j}")
        Hs[j].close()


def test_measured_choice_small(monkeypatch):
    """no override: the first k-step times both forms on the caller's vectors and keeps the faster; whichever wins, the bits are the
    oracle's and the handle says what it does"""
    monkeypatch.delenv("MI355_SPMK_FUSED", raising=False)
    H = Handle("band:2000:7")
    first = H.launch(4)
    info = H.A.spmk_info(4)
    print(f"band:2000:7, k = 4: {info['us_k_launches']:.2f} us in 4 launches, {info['us_one_launch']:.2f} us in one -> one_launch = {info['one_launch']}")
    assert info["us_k_launches"] > 0 and info["us_one_launch"] > 0, info
    H.check(first, "measured choice", one_launch=info["one_launch"], eligible=True)
    H.step(4, "measured choice, again", one_launch=info["one_launch"], eligible=True)
    H.close()


def test_epoch_wrap():
    """(int)(flag - want) < 0 across 2^31 and 2^32: a solver that runs the step for a day or so gets there.  In a child process on the
    devtools build, whose mi_debug_spmk_set_epoch puts a handle into the state a step ending at e - 1 leaves (tests/spmk_epoch_worker.py)."""
    assert os.path.exists(DEVLIB), "the devtools build (make devtools; __graft_entry__.build) is missing"
    env = dict(os.environ, MI355_SPMV_LIBRARY=DEVLIB, MI355_SPMK_FUSED="1")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "tests", "spmk_epoch_worker.py")],
                       capture_output=True, text=True, env=env, timeout=150)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "SPMK_EPOCH_OK" in r.stdout, f"exit {r.returncode}\n" + r.stdout[-4000:] + r.stderr[-3000:]
    assert r.stdout.count("epoch ") == 4, r.stdout
