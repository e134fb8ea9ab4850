"""Seeded fuzz of the multi-rank paths (mi_part_*, the one-launch push steps, mi_dist_*) against the oracle, bit for bit.

The cases come from tests/multirank_cases.py: ragged bands with far couplings, upwind couplings, FE node blocks with emptied rows
and far blocks, a multi-band mesh operator, and the degenerate partitions (n < N, everything on one rank, a rank of empty rows, a
rank that reads only ghosts, no ghosts at all, n = 1), cut nnz-balanced, by equal rows, at random and with repeated cut points.

- CPU: the hand exchange of test_partition.py with the oracle on every piece (interior, boundary, the one-launch step's combined
  piece), and the sliced-stream planner's replay on every combined piece.
- GPU, one process: all N handles on cuda:0, pack -> halo copied by the test through the recv offsets -> interior -> boundary,
  three powers, then a value refresh, for every piece kernel a partition takes; the kernel that served every piece is asserted.
- GPU, child processes (tests/multirank_worker.py): the one-launch push steps of N handles in ONE process with their pushes looped
  back (every wait satisfied in advance), and mi_dist end to end over the event and fake-RCCL exchanges.

Comparison is bitwise; with IEEE specials in x (ghost positions only) a NaN matches any NaN (test_gpu_edges.assert_same)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import multirank_cases as MC
from conftest import ROOT, assert_bit_equal
from navierstokes_amd import mpk
from oracle import oracle as O

NSEEDS = 48
WORKER = os.path.join(ROOT, "tests", "multirank_worker.py")
DEVLIB = os.path.join(ROOT, "navierstokes_amd", "csrc", "libmi355spmv_dev.so")
FAKE = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")
CASES = {c[4]: c for c in MC.all_cases(NSEEDS)}
LABELS = list(CASES)


def _env(monkeypatch, label):
    """the planner's two switches, varied with the case"""
    h = sum(map(ord, label))
    monkeypatch.setenv("MI355_PART_DENSE_HALO", str(h % 2))
    monkeypatch.setenv("MI355_PART_CONTIGUOUS_INTERIOR", str((h // 2) % 2))
    # (ragged pieces of a few hundred rows pad their 128-row slices beyond the default limit: let the sliced stream take them anyway,
    # as test_ring_plan does, so that its kernels meet these patterns instead of handing every one to a fallback)
    monkeypatch.setenv("MI355_SSTREAM_MAX_PADDING", "1e9")


def _combined(pl):
    L = mpk.lib()
    nr, pp, pc, pv, pm = ctypes.c_int(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    mpk.check(L.mi_part_local_csr(pl._h, 2, ctypes.byref(nr), ctypes.byref(pp), ctypes.byref(pc), ctypes.byref(pv), ctypes.byref(pm)))
    nleft = ctypes.c_int()
    mpk.check(L.mi_part_combined_info(pl._h, ctypes.byref(nleft)))
    ptrow = np.ctypeslib.as_array(ctypes.cast(pp, ctypes.POINTER(ctypes.c_int)), shape=(nr.value + 1,)).copy()
    nnz = int(ptrow[-1])
    col = np.ctypeslib.as_array(ctypes.cast(pc, ctypes.POINTER(ctypes.c_int)), shape=(max(nnz, 1),))[:nnz].copy() if nnz else np.zeros(0, np.int32)
    val = np.ctypeslib.as_array(ctypes.cast(pv, ctypes.POINTER(ctypes.c_double)), shape=(max(nnz, 1),))[:nnz].copy() if nnz else np.zeros(0)
    return nr.value, nleft.value, ptrow, col, val, pm.value


# ----------------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("label", LABELS)
def test_hand_exchange_pieces_equal_global_product(label, monkeypatch):
    """Every rank's interior and boundary pieces, fed the halo its peers would pack, and its combined piece fed x in its own
    numbering, reproduce the rank's slice of the global product bit for bit; where the combined piece is eligible for the sliced
    stream, its ghost-aware plan replays (mi_sstream_plan_probe_ex raises on the first broken invariant)."""
    P, C, V, rs, _ = CASES[label]
    _env(monkeypatch, label)
    N, n = len(rs) - 1, len(P) - 1
    x = np.random.default_rng(len(label)).uniform(-1, 1, n)
    yg = O.spmv(P, C, V, x)
    plans = MC.make_plans(P, C, V, rs)
    L = mpk.lib()
    try:
        for r, pl in enumerate(plans):
            lo, hi = int(rs[r]), int(rs[r + 1])
            assert pl.n_local == hi - lo and pl.n_interior + pl.n_boundary == pl.n_local
            assert sum(pl.recv_counts) == pl.n_halo and pl.recv_counts[r] == 0
            halo_ids = np.concatenate([pl.recv_ids[q] for q in range(N)] + [np.zeros(0, np.int64)])
            assert (np.diff(halo_ids) > 0).all() and ((halo_ids < lo) | (halo_ids >= hi)).all()
            halo = MC.halo_of(plans, rs, r, x)
            assert_bit_equal(halo, x[halo_ids], f"{label} rank {r}: packed halo")
            x_ext = np.concatenate([x[lo:hi], halo])
            y = np.full(pl.n_local, np.nan)
            seen = np.zeros(pl.n_local, np.int64)
            for which in (0, 1):
                p, c, v, rmap = pl.local_piece(which)
                assert len(p) == len(rmap) + 1
                if len(c):
                    assert c.min() >= 0 and c.max() < pl.n_local + pl.n_halo
                if which == 0 and len(c):
                    assert c.max() < pl.n_local, "an interior row names a ghost"
                seen[rmap] += 1
                y[rmap] = O.spmv(p, c, v, x_ext)
            assert (seen == 1).all(), f"{label} rank {r}: a row in no piece or in both"
            assert_bit_equal(y, yg[lo:hi], f"{label} rank {r}: interior + boundary")
            nr, nleft, cp, cc, cv, pm = _combined(pl)
            assert nr == pl.n_local and not pm and nleft == int((halo_ids < lo).sum())
            gid = np.concatenate([halo_ids[:nleft], np.arange(lo, hi), halo_ids[nleft:]]).astype(np.int64)
            assert np.array_equal(gid[cc], C[P[lo]:P[hi]]), "combined piece: other terms or another order"
            assert_bit_equal(O.spmv(cp, cc, cv, x[gid]) if nr else np.zeros(0), yg[lo:hi], f"{label} rank {r}: combined piece")
            if nr:
                e, rd, gw, st, pad = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong(), ctypes.c_double()
                mm = (ctypes.c_int * 2)()
                mpk.check(L.mi_sstream_plan_probe_ex(nr, pl.n_local + pl.n_halo, cp.ctypes.data, cc.ctypes.data if len(cc) else None, 0,
                                                     nleft, nleft + pl.n_local, ctypes.byref(e), ctypes.byref(rd), ctypes.byref(st),
                                                     ctypes.byref(pad), ctypes.byref(gw), mm))
                if e.value and pl.n_halo == 0:
                    assert gw.value == 0, "a ghost-free piece with a ghost-marked workgroup"
    finally:
        for pl in plans:
            pl.close()


# ------------------------------------------------------------------------------------------- GPU, four-launch step by hand
PIECE_KERNELS = ("auto", "stream", "ring", "rowpar", "sstream")
ALLOWED = {"stream": ("spmv_csr_stream<",), "ring": ("spmv_csr_ring<", "spmv_csr_stream<"), "rowpar": ("spmv_csr_rowpar",),
           "sstream": ("spmv_sstream<", "spmv_sstream_mw<", "spmv_csr_ring<", "spmv_csr_stream<"),
           "auto": ("spmv_sstream", "spmv_csr_ring<", "spmv_csr_stream<", "spmv_csr_rowpar", "spmv_csr_tile<", "spmv_csr_mring<", "spmv_bcsr4")}
SERVED = {}   # (forced kernel, served kernel family) -> pieces; filled by the GPU cases, checked and printed at the end
GPU_LABELS = [lab for lab in LABELS if not lab.startswith("n1-N1")]
IEEE_LABELS = {GPU_LABELS[0], "only-ghosts-rank1-of-3", "fe-s8-N3-balanced-a4-n1372"}


def _family(name):
    for k in ("spmv_sstream_mw", "spmv_sstream", "spmv_csr_ring", "spmv_csr_stream", "spmv_csr_rowpar"):
        if name.startswith(k):
            return k
    return name.split("<")[0]


class _DevRanks:
    """N finalized handles on cuda:0 and the step of DistCSR done by hand: pack, halo copies through the recv offsets, interior, boundary"""

    def __init__(self, P, C, V, rs):
        import torch
        self.torch = torch
        self.rs, self.N = rs, len(rs) - 1
        self.plans = MC.make_plans(P, C, V, rs)
        L = mpk.lib()
        for pl in self.plans:
            mpk.check(L.mi_part_finalize(pl._h))
        self.sidx = [pl.send_index() for pl in self.plans]
        self.sc = [pl.send_counts_() for pl in self.plans]
        self.sendbuf = [torch.full((max(1, int(s.sum())),), float("nan"), dtype=torch.float64, device="cuda") for s in self.sc]

    def buf(self, r, owned=None):
        pl = self.plans[r]
        t = self.torch.full((max(1, pl.n_local + pl.n_halo),), float("nan"), dtype=self.torch.float64, device="cuda")
        if owned is not None and pl.n_local:
            t[:pl.n_local] = self.torch.from_numpy(np.ascontiguousarray(owned)).cuda()
        return t

    def step(self, xs, ys):
        """ys[r][:n_local] = (A x)_r for x_ext = xs[r]; fills the halo part of every xs[r] first"""
        L, vp, sp = mpk.lib(), ctypes.c_void_p, mpk._stream_ptr()
        for r, pl in enumerate(self.plans):
            mpk.check(L.mi_part_pack_dev(pl._h, vp(xs[r].data_ptr()), vp(self.sendbuf[r].data_ptr()), sp))
        for r, pl in enumerate(self.plans):
            off = pl.n_local
            for q in range(self.N):
                cnt = pl.recv_counts[q]
                if cnt:
                    s_off = int(self.sc[q][:r].sum())
                    xs[r][off:off + cnt] = self.sendbuf[q][s_off:s_off + cnt]
                    off += cnt
        for r, pl in enumerate(self.plans):
            mpk.check(L.mi_part_spmv_interior_dev(pl._h, vp(xs[r].data_ptr()), vp(ys[r].data_ptr()), sp))
            mpk.check(L.mi_part_spmv_boundary_dev(pl._h, vp(xs[r].data_ptr()), vp(ys[r].data_ptr()), sp))

    def close(self):
        for pl in self.plans:
            pl.close()


@pytest.mark.gpu
@pytest.mark.parametrize("label", GPU_LABELS)
def test_four_launch_step_by_hand(label, monkeypatch):
    """Three powers with one exchange each, for every piece kernel, then mi_part_update_values and one more product: every rank's
    slice bitwise against O.spmk_chain / O.spmv of the global matrix; the kernel that served each piece is the forced one or its
    documented fallback (resolve_kernel), never another."""
    import torch
    from test_gpu_edges import assert_same
    P, C, V, rs, _ = CASES[label]
    _env(monkeypatch, label)
    N, n = len(rs) - 1, len(P) - 1
    rng = np.random.default_rng(3 + len(label))
    x = rng.uniform(-1, 1, n)
    if label in IEEE_LABELS:
        x = MC.ieee_at_ghosts(x, P, C, rs)
    Y = O.spmk_chain(3, P, C, V, x)
    R = _DevRanks(P, C, V, rs)
    L = mpk.lib()
    try:
        for kern in PIECE_KERNELS:
            for pl in R.plans:
                mpk.check(L.mi_part_set_kernel(pl._h, mpk.KERNELS[kern]))
                for w in (0, 1):
                    name = L.mi_part_kernel_name(pl._h, w).decode()
                    assert name.startswith(ALLOWED[kern]), f"{label}: forced {kern}, piece {w} of rank {pl.rank} ran {name!r}"
                    SERVED[(kern, _family(name))] = SERVED.get((kern, _family(name)), 0) + 1
            bufs = [[R.buf(r, x[int(rs[r]):int(rs[r + 1])]) for r in range(N)]] + [[R.buf(r) for r in range(N)] for _ in range(3)]
            for k in range(3):
                R.step(bufs[k], bufs[k + 1])
            torch.cuda.synchronize()
            for k in range(3):
                for r, pl in enumerate(R.plans):
                    lo, hi = int(rs[r]), int(rs[r + 1])
                    assert_same(bufs[k + 1][r][:pl.n_local], Y[k][lo:hi], f"{label} {kern}: power {k + 1}, rank {r}")
        V2 = V * np.cos(np.arange(len(V)))
        for r, pl in enumerate(R.plans):
            lo, hi = int(rs[r]), int(rs[r + 1])
            mpk.check(L.mi_part_update_values(pl._h, np.ascontiguousarray(V2[P[lo]:P[hi]]).ctypes.data))
        xs = [R.buf(r, x[int(rs[r]):int(rs[r + 1])]) for r in range(N)]
        ys = [R.buf(r) for r in range(N)]
        R.step(xs, ys)
        torch.cuda.synchronize()
        y2 = O.spmv(P, C, V2, x)
        for r, pl in enumerate(R.plans):
            assert_same(ys[r][:pl.n_local], y2[int(rs[r]):int(rs[r + 1])], f"{label}: after mi_part_update_values, rank {r}")
    finally:
        R.close()


@pytest.mark.gpu
def test_four_launch_fuzz_reached_every_piece_kernel(monkeypatch):
    """The fuzz above must not only exercise fallbacks: every forced piece kernel served pieces itself (counts printed for the record)."""
    if not SERVED:  # (run on its own: the sweep first)
        for lab in GPU_LABELS:
            test_four_launch_step_by_hand(lab, monkeypatch)
    print("\npieces served, by forced kernel:")
    for (kern, fam), cnt in sorted(SERVED.items()):
        print(f"  {kern:8s} -> {fam:18s} {cnt}")
    for kern, fam in (("stream", "spmv_csr_stream"), ("ring", "spmv_csr_ring"), ("rowpar", "spmv_csr_rowpar"), ("sstream", "spmv_sstream")):
        assert SERVED.get((kern, fam), 0) >= 10, (kern, fam, SERVED)


# ------------------------------------------------------------------------------------------------ GPU, child processes
def _worker(args, env, timeout):
    r = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, WORKER] + args, capture_output=True, text=True,
                       env=dict(os.environ, **env), timeout=timeout + 30)
    assert r.returncode == 0 and "MULTIRANK_OK" in r.stdout, f"exit {r.returncode}\n" + r.stdout[-4000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.gpu
def test_push_steps_looped_back():
    """The one-launch push steps of N handles in one process, pushes looped back (MI355_PUSH_LOOPBACK, every flag preset before every
    launch): every forced form asserted by mi_part_push_info / mi_part_kernel_name(P, 2), bitwise against the oracle from the third
    sweep on (the window's two parities are then full), a second x, and a value refresh through the fused handles.  Each form must
    have served at least three cases, one of them with an empty or ghost-free rank."""
    assert os.path.exists(DEVLIB), "the devtools build (make devtools; __graft_entry__.build) is missing"
    out = _worker(["push"], {"MI355_SPMV_LIBRARY": DEVLIB, "MI355_PUSH_LOOPBACK": "1", "MI355_SSTREAM_MAX_PADDING": "1e9"}, 420)
    print(out[-3000:])
    table = {}
    for ln in out.splitlines():
        if ln.startswith("FORM "):
            _, form, cases, degenerate = ln.split()
            table[form] = (int(cases), int(degenerate))
    want = ["four-launch", "ring", "sstream", "csr_ext"] +[f"bcsr4_ext-l{l16}-s{split}" for l16 in (0, 1, 2) for split in (0, 1)] + ["bcsr4_ext-wgs1"]
    for form in want:
        cases, degenerate = table.get(form, (0, 0))
        assert cases >= 3 and degenerate >= 1, (form, table)


@pytest.mark.gpu
@pytest.mark.parametrize("exchange", ["event", "sendrecv", "allgather"])
def test_dist_handles_end_to_end(exchange):
    """mi_dist over ndev in {2, 3, 5, 8} (ndev > n included): spmv, spmk k = 3, five spmv_dev back to back, update_values, and dot
    bitwise against the rank-order sum of every rank's fixed-tree dot over the slice mi_dist_rank_info reports."""
    env = {"MI355_DIST_EXCHANGE": "event"} if exchange == "event" else {
        "MI355_DIST_EXCHANGE": "rccl", "MI355_RCCL_LIBRARY": FAKE, "MI355_PART_EXCHANGE": exchange}
    if exchange != "event":
        assert os.path.exists(FAKE), "tests/fake_rccl not built"
    out = _worker(["dist", exchange], env, 420)
    assert out.count(" ok") >= 20, out[-3000:]
