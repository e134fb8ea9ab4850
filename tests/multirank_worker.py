"""Worker for tests/test_multirank_fuzz.py (TEST INFRASTRUCTURE): runs in a child process because the library reads its
environment (MI355_SPMV_LIBRARY, MI355_PUSH_LOOPBACK, MI355_RCCL_LIBRARY) once per process.
  push            the one-launch push steps: N mi_part handles in THIS process, pushes looped back into their windows
  dist <exchange> mi_dist end to end (event | sendrecv | allgather; the two RCCL forms over tests/fake_rccl)
  lifecycle <cycles>  tests/test_gpu_part_lifecycle.py: every way a partition and an mi_dist handle come to own device memory, over and over
Prints one line per case, FORM lines (push), and MULTIRANK_OK on success."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import multirank_cases as MC  # noqa: E402
from conftest import assert_bit_equal  # noqa: E402
from navierstokes_amd import mpk  # noqa: E402
from oracle import oracle as O  # noqa: E402

vp = ctypes.c_void_p

# forced form -> environment; the name mi_part_kernel_name(P, 2) then reports for a rank that form serves ("": the four launches)
# (MI355_SSTREAM=1: the combined pieces here are small, and the sliced copy is built at create only for large ones or on request)
PUSH_FORMS = {"four-launch": ({"MI355_PUSH_FUSED": "0"}, ""),
              "ring": ({"MI355_PUSH_FUSED_KERNEL": "ring"}, "[FUSED]"),
              "sstream": ({"MI355_PUSH_FUSED_KERNEL": "sstream", "MI355_SSTREAM": "1"}, "spmv_sstream_fused<"),
              "csr_ext": ({"MI355_PUSH_FUSED_KERNEL": "csr_ext", "MI355_PUSH_EXT_SPLIT": "0"}, "spmv_csr_fused_ext")}
for l16 in (0, 1, 2):
    for split in (0, 1):
        PUSH_FORMS[f"bcsr4_ext-l{l16}-s{split}"] = ({"MI355_PUSH_EXT_LANES16": str(l16), "MI355_PUSH_EXT_SPLIT": str(split)}, "spmv_bcsr4_fused_ext")
PUSH_FORMS["bcsr4_ext-wgs1"] = ({"MI355_PUSH_EXT_WGS": "1", "MI355_PUSH_EXT_SPLIT": "0"}, "spmv_bcsr4_fused_ext")
FORM_VARS = ("MI355_PUSH_FUSED", "MI355_PUSH_FUSED_KERNEL", "MI355_SSTREAM", "MI355_PUSH_EXT_LANES16", "MI355_PUSH_EXT_SPLIT", "MI355_PUSH_EXT_WGS")


def _cases_for(form, cases):
    fe = [c for c in cases if c[4].startswith("fe-") and "-a4-" in c[4]]
    if form.startswith("bcsr4_ext"):
        return fe[:6]
    rest = [c for c in cases if not c[4].startswith("fe-") or "-a0-" in c[4]]
    return rest


class PushRanks:
    def __init__(self, P, C, V, rs):
        L = mpk.lib()
        self.rs, self.N = rs, len(rs) - 1
        self.plans = MC.make_plans(P, C, V, rs)
        for pl in self.plans:
            mpk.check(L.mi_part_finalize(pl._h))
        self.connect()

    def connect(self):
        """export every window, connect every rank, read the forms the ranks took"""
        L = mpk.lib()
        hb = [ctypes.create_string_buffer(64) for _ in range(self.N)]
        lays = np.zeros((self.N, 2 * self.N + 1), np.int64)
        for r, pl in enumerate(self.plans):
            lay = np.zeros(2 * self.N + 1, np.int64)
            mpk.check(L.mi_part_push_export(pl._h, hb[r], lay.ctypes.data))
            lays[r] = lay
        handles = b"".join(h.raw for h in hb)
        lays = np.ascontiguousarray(lays)
        for pl in self.plans:
            mpk.check(L.mi_part_push_connect(pl._h, ctypes.create_string_buffer(handles, len(handles)), lays.ctypes.data))
        self.names, self.fused = [], []
        for pl in self.plans:
            fz = ctypes.c_int()
            mpk.check(L.mi_part_push_info(pl._h, None, ctypes.byref(fz), None))
            name = L.mi_part_kernel_name(pl._h, 2).decode()
            assert bool(fz.value) == bool(name), (fz.value, name)
            self.fused.append(bool(fz.value))
            self.names.append(name)

    def sweep(self, xs, ys):
        """every rank's step once, one after another on one stream; all N windows' flags preset before every launch"""
        L, sp = mpk.lib(), mpk._stream_ptr()
        for r, pl in enumerate(self.plans):
            for q in self.plans:
                mpk.check(L.mi_part_push_debug_preset(q._h, 0x3fffffff))
            mpk.check(L.mi_part_spmv_push_dev(pl._h, vp(xs[r].data_ptr()), vp(ys[r].data_ptr()), sp))
            torch.cuda.synchronize()
            mpk.check(L.mi_part_status(pl._h))

    def product(self, x, label, what):
        """three sweeps with the same x (the window's two parities then hold entries pushed from x); the third is checked"""
        xs, ys = [], []
        for r, pl in enumerate(self.plans):
            t = torch.full((max(1, pl.n_local + pl.n_halo),), float("nan"), dtype=torch.float64, device="cuda")
            if pl.n_local:
                t[:pl.n_local] = torch.from_numpy(np.ascontiguousarray(x[int(self.rs[r]):int(self.rs[r + 1])])).cuda()
            xs.append(t)
            ys.append(torch.full((max(1, pl.n_local),), float("nan"), dtype=torch.float64, device="cuda"))
        for _ in range(3):
            for y in ys:
                y.fill_(float("nan"))
            self.sweep(xs, ys)
        return [ys[r][:pl.n_local].cpu().numpy() for r, pl in enumerate(self.plans)]

    def close(self):
        for pl in self.plans:
            pl.close()


def push():
    cases = MC.all_cases(48)
    served = {}
    for form, (env, marker) in PUSH_FORMS.items():
        for k in FORM_VARS:
            os.environ.pop(k, None)
        os.environ.update(env)
        count = degenerate = 0
        for P, C, V, rs, label in _cases_for(form, cases):
            if len(rs) == 2:
                continue
            R = PushRanks(P, C, V, rs)
            try:
                if marker:
                    hit = any(marker in nm for nm in R.names)
                else:  # the four launches, with something to exchange
                    hit = not any(R.fused) and any(pl.n_halo for pl in R.plans)
                    assert not any(R.fused), R.names
                for nm in R.names:
                    served[(form, nm.split("<")[0] or "four-launch")] = served.get((form, nm.split("<")[0] or "four-launch"), 0) + 1
                n = len(P) - 1
                rng = np.random.default_rng(11 + len(label))
                for t, x in enumerate((rng.uniform(-1, 1, n), np.sin(0.37 * np.arange(n)) + 0.5)):
                    got = R.product(x, label, form)
                    yg = O.spmv(P, C, V, x)
                    for r in range(R.N):
                        assert_bit_equal(got[r], yg[int(rs[r]):int(rs[r + 1])], f"{form} {label}: x{t + 1}, rank {r} ({R.names[r] or 'four launches'})")
                if hit and count == 0:  # a value refresh through the fused handles, once per form
                    V2 = V * np.cos(np.arange(len(V)))
                    L = mpk.lib()
                    for r, pl in enumerate(R.plans):
                        lo, hi = int(rs[r]), int(rs[r + 1])
                        mpk.check(L.mi_part_update_values(pl._h, np.ascontiguousarray(V2[P[lo]:P[hi]]).ctypes.data))
                    got = R.product(x, label, form)
                    yg = O.spmv(P, C, V2, x)
                    for r in range(R.N):
                        assert_bit_equal(got[r], yg[int(rs[r]):int(rs[r + 1])], f"{form} {label}: after mi_part_update_values, rank {r}")
                if hit:
                    count += 1
                    degenerate += any(pl.n_local == 0 or pl.n_halo == 0 for pl in R.plans)
                print(f"  push {form} {label}: {' | '.join(nm or '-' for nm in R.names)} ok", flush=True)
            finally:
                R.close()
        print(f"FORM {form} {count} {degenerate}", flush=True)
    print("kernels of the one-launch step, by forced form:")
    for (form, nm), cnt in sorted(served.items()):
        print(f"  {form:16s} {nm:28s} {cnt}")


def dist(exchange):
    cases = [c for c in MC.all_cases(48)]
    picked = cases[:12] + MC.degenerate()
    ndevs = (2, 3, 5, 8)
    for i, (P, C, V, _, label) in enumerate(picked):
        n = len(P) - 1
        for ndev in (ndevs[i % 4], 8) if n < 8 else (ndevs[i % 4],):
            try:
                Dm = mpk.DistMatrix(ndev, n, P, C, V)
            except mpk.MiError as e:
                print(f"  dist {exchange} {label} ndev={ndev}: refused: {e}", flush=True)
                raise
            try:
                info = Dm.info()
                assert info["nranks"] == ndev and sum(r["n_local"] for r in info["ranks"]) == n, info
                want = "event" if exchange == "event" else ("rccl-allgather" if exchange == "allgather" else "rccl")
                assert info["exchange"] == want, (info["exchange"], info["note"])
                rng = np.random.default_rng(21 + i)
                x = rng.uniform(-1, 1, n)
                y = np.full(n, np.nan)
                Dm.spmv(y, x)
                assert_bit_equal(y, O.spmv(P, C, V, x), f"{label} ndev={ndev}: spmv")
                Y = O.spmk_chain(3, P, C, V, x)
                outs = [np.full(n, np.nan) for _ in range(3)]
                Dm.spmk(outs, x)
                for q in range(3):
                    assert_bit_equal(outs[q], Y[q], f"{label} ndev={ndev}: power {q + 1}")
                vx, vy = Dm.vector(x), Dm.vector()
                for _ in range(5):
                    Dm.spmv_dev(vy, vx)
                Dm.synchronize()
                assert_bit_equal(vy.get(), Y[0], f"{label} ndev={ndev}: five spmv_dev back to back")
                b = np.cos(0.003 * np.arange(n)) - 0.25
                sl = [(r["row_start"], r["row_start"] + r["n_local"]) for r in info["ranks"]]
                want_dot = O.tree_rank_sum([O.tree_dot(b[s:e], Y[0][s:e]) for s, e in sl])
                assert_bit_equal(np.float64(Dm.dot(b, Y[0])), np.float64(want_dot), f"{label} ndev={ndev}: dot")
                V2 = V * np.cos(np.arange(len(V)))
                Dm.update_values(V2)
                Dm.spmv(y, x)
                assert_bit_equal(y, O.spmv(P, C, V2, x), f"{label} ndev={ndev}: after mi_dist_update_values")
                for t in (vx, vy):
                    t.close()
                print(f"  dist {exchange} {label} ndev={ndev}: exchange={info['exchange']} ok", flush=True)
            finally:
                Dm.close()


# ---------------------------------------------------------------------------------------------------- lifecycle
GRANULE = 2 << 20
FE_CELLS = 13     # the smallest synth.fe_matrix whose two ranks each hold a value array above the granule (tests/test_gpu_part_lifecycle.py asserts it)
S15_ROWS = 34954  # ... and the smallest even synth.rows("s15", n): 15 nonzeros per row, 17 477 rows per rank
S15_WIDTH = 300
SCALAR_FORMS = ("ring", "sstream", "csr_ext")
DIST_LIVES = (("event", 0, 2), ("sendrecv", 2, 3), ("allgather", 3, 5))  # exchange, seed of the multirank_cases case, ranks (all on device 0)


def lifecycle_matrices():
    """(P, C, V, row_starts) of the two push lives: a blocked FE matrix and a scalar band, two ranks each"""
    from navierstokes_amd import dist, synth
    out = []
    for (P, C, V), align in ((synth.fe_matrix(FE_CELLS), 4), (synth.rows("s15", S15_ROWS, w=S15_WIDTH), 1)):
        out.append((P, C, V, dist.balanced_row_starts(len(P) - 1, 2, np.diff(P), align=align)))
    return out


def lifecycle_reference():
    """Everything the lives compare against, computed once: x, the second set of values, the oracle's products."""
    ref = {"push": [], "dist": []}
    for i, (P, C, V, rs) in enumerate(lifecycle_matrices()):
        x = np.random.default_rng(31 + i).uniform(-1, 1, len(P) - 1)
        V2 = V * np.cos(np.arange(len(V)))
        ref["push"].append(dict(P=P, C=C, V=V, rs=rs, x=x, V2=V2, y=O.spmv(P, C, V, x), y2=O.spmv(P, C, V2, x)))
    for exchange, seed, ndev in DIST_LIVES:
        P, C, V, _, label = MC.case(seed)
        x = np.random.default_rng(41 + seed).uniform(-1, 1, len(P) - 1)
        V2 = V * np.cos(np.arange(len(V)))
        ref["dist"].append(dict(P=P, C=C, V=V, x=x, V2=V2, Y=O.spmk_chain(3, P, C, V, x), y2=O.spmv(P, C, V2, x), exchange=exchange, ndev=ndev, label=label))
    return ref


def push_life(R_, form, what, say=None):
    """create -> send ids -> finalize -> export -> connect, a one-launch product, new values, the four launches, the exchange given
    up, brought up again, destroy; every product bitwise.  say: told which kernels the pieces' create-time measurements chose"""
    env, marker = PUSH_FORMS[form]
    for k in FORM_VARS:
        os.environ.pop(k, None)
    os.environ.update(env)
    L = mpk.lib()
    P, rs = R_["P"], R_["rs"]
    R = PushRanks(P, R_["C"], R_["V"], rs)
    if say:
        say(f"{what}: " + " | ".join(L.mi_part_kernel_name(pl._h, w).decode() for pl in R.plans for w in (0, 1, 2)))

    def check(want, step, one_launch):
        assert all((marker in nm) if one_launch else nm == "" for nm in R.names), (what, step, R.names)
        got = R.product(R_["x"], what, form)
        for r in range(R.N):
            assert_bit_equal(got[r], want[int(rs[r]):int(rs[r + 1])], f"{what}: {step}, rank {r} ({R.names[r] or 'four launches'})")

    try:
        check(R_["y"], "one launch", True)
        for r, pl in enumerate(R.plans):
            mpk.check(L.mi_part_update_values(pl._h, np.ascontiguousarray(R_["V2"][P[int(rs[r])]:P[int(rs[r + 1])]]).ctypes.data))
        check(R_["y2"], "after mi_part_update_values", True)
        for pl in R.plans:
            mpk.check(L.mi_part_push_unfuse(pl._h))
        R.names = [L.mi_part_kernel_name(pl._h, 2).decode() for pl in R.plans]
        check(R_["y2"], "after mi_part_push_unfuse", False)
        torch.cuda.synchronize()
        for pl in R.plans:
            mpk.check(L.mi_part_push_disable(pl._h))
        R.connect()
        check(R_["y2"], "connected again", True)
        torch.cuda.synchronize()
    finally:
        R.close()
        for k in FORM_VARS:  # (the lives that follow run under no forced form)
            os.environ.pop(k, None)


def dist_life(R_, what):
    """an mi_dist handle: product, three powers, a device vector left to the handle's destroy, one closed, new values, destroy"""
    ex = R_["exchange"]
    os.environ["MI355_DIST_EXCHANGE"] = "event" if ex == "event" else "rccl"
    os.environ["MI355_PART_EXCHANGE"] = ex
    P, C, n = R_["P"], R_["C"], len(R_["P"]) - 1
    Dm = mpk.DistMatrix(R_["ndev"], n, P, C, R_["V"])
    try:
        info = Dm.info()
        assert info["exchange"] == {"event": "event", "sendrecv": "rccl", "allgather": "rccl-allgather"}[ex], (what, info["exchange"], info["note"])
        assert_bit_equal(Dm.spmv(np.full(n, np.nan), R_["x"]), R_["Y"][0], f"{what}: product")
        outs = Dm.spmk([np.full(n, np.nan) for _ in range(3)], R_["x"])
        for q in range(3):
            assert_bit_equal(outs[q], R_["Y"][q], f"{what}: power {q + 1}")
        left, closed = Dm.vector(R_["x"]), Dm.vector()
        Dm.spmv_dev(closed, left)
        Dm.synchronize()
        assert_bit_equal(closed.get(), R_["Y"][0], f"{what}: device-resident vectors")
        closed.close()
        Dm.update_values(R_["V2"])
        assert_bit_equal(Dm.spmv(np.full(n, np.nan), R_["x"]), R_["y2"], f"{what}: after mi_dist_update_values")
    finally:
        Dm.close()
    left.close()  # (its device memory went with the handle: this frees the host object)


def lifecycle_cycle(ref, cycle, say=None):
    """one cycle: a push life on the FE matrix (the blocked staged step), one on the scalar band (its form rotates), three mi_dist lives"""
    push_life(ref["push"][0], "bcsr4_ext-l1-s0", f"cycle {cycle}, FE", say)
    form = SCALAR_FORMS[cycle % 3]
    push_life(ref["push"][1], form, f"cycle {cycle}, scalar {form}", say)
    for R_ in ref["dist"]:
        dist_life(R_, f"cycle {cycle}, mi_dist {R_['exchange']} {R_['label']} ndev={R_['ndev']}")


def lifecycle(cycles):
    import time
    ref = lifecycle_reference()
    free = {}
    t0 = time.perf_counter()
    for cycle in range(cycles):
        lifecycle_cycle(ref, cycle)
        torch.cuda.synchronize()
        free[cycle] = torch.cuda.mem_get_info()[0]
    print(f"LIFECYCLE cycles {cycles} free4 {free[4]} last {free[cycles - 1]} seconds {time.perf_counter() - t0:.1f}", flush=True)
    assert free[cycles - 1] >= free[4], f"{free[4] - free[cycles - 1]} bytes of device memory went in {cycles - 5} cycles"


if __name__ == "__main__":
    mode = sys.argv[1]
    torch.cuda.set_device(0)
    if mode == "push":
        push()
    elif mode == "lifecycle":
        lifecycle(int(sys.argv[2]))
    else:
        dist(sys.argv[2])
    print("MULTIRANK_OK", flush=True)
    sys.stdout.flush()
    os._exit(0)
