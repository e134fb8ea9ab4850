"""What one workgroup of spmk_csr_ring<256, 2048, 5120, D, kRingMaxB, NT, SKEW> touches of x and y in one power, restated in plain
Python FROM THE KERNEL (navierstokes_amd/csrc/spmk_ring.hpp), not from build_run_deps (ring_plan.hpp), whose lists it judges.  The
hand-off between powers has no acquire: it is safe only if no load of a run reaches a row of a run that is not on its list.

Inputs: the plan as mi_csr_create builds it (mpk.spmk_plan_dump), the CSR pattern, D in {2, 4}.  The kernel, line by line:

  run         `rng = bpw > 0 ? {min(nblk, gw * bpw), min(nblk, (gw + 1) * bpw)} : run_rng[gw]` — the launch passes bpw only for the
              uniform deal; nb = rng.y - rng.x blocks; nb <= 0 returns at once (an idle run)
  records     s_plan[2 lb], s_plan[2 lb + 1] = {r0, p0, rows, nnz}, {new_lo, new_cnt, base, flags} for lb < nb; behind them 2 D + 2
              sentinels {r0 + rows, p0 + nnz, 0, 0}, {new_lo of the LAST block, 0, 0, 0}
  issue(lb)   every lane loads x[min(m1.x + tid, n - 1)], tid < 256.  Issued: lb = 0 .. D - 1 before the loop, then lb + D for every
              lb the loop `for (g = 0; g < nb; g += D) for (s < D) lb = g + s` visits — it runs past nb to the next multiple of D, so
              lb = 0 .. ceil(nb / D) D + D - 1 in all, of which the last D .. 2 D - 1 are sentinels
  first fill  q = s_plan[1]; chi = min(max(q.x + q.y, q.x + 256) - 1, n - 1); lanes load x[min(q.x + tid + u 256, chi)], u < 20
  window      block lb + 1's new columns are what issue(lb + 1) loaded: lane tid < new_cnt holds column new_lo + tid — right only if
              new_cnt <= 256 for every block but the first and the clamp to n - 1 does not bite below new_lo + new_cnt; the first
              block's are the fill's: new_cnt <= 20 * 256
  stores      y[r0 + tid], tid < rows, for every lb the loop visits (sentinels: no rows); rows <= 256 or rows are lost

check() holds a dump to that.  Everything is kept as closed index ranges; a run's loads are a few dozen of them."""
import numpy as np

T = 256
FILL = 20          # (RING + T - 1) / T with RING = 5120
MAXB = 160         # kRingMaxB: blocks per run the LDS plan holds (plus 2 D + 2 sentinels)
MAX_LIST = 64      # launch_spmk.hip: longer lists mean k launches


def run_range(d, g):
    """blocks [b0, b1) of run g as the kernel finds them"""
    if d["uniform"]:
        return min(d["nblk"], g * d["bpw"]), min(d["nblk"], (g + 1) * d["bpw"])
    return int(d["run_rng"][g][0]), int(d["run_rng"][g][1])


def run_touches(d, n, D, g):
    """(loads, stores, named) of run g in one power: closed x index ranges loaded, half-open y row ranges stored, and the
    half-open ranges of nonzeros its rows hold.  Raises AssertionError where the kernel itself would go wrong."""
    b0, b1 = run_range(d, g)
    nb = b1 - b0
    if nb <= 0:
        return [], [], []
    assert nb <= MAXB, f"run {g}: {nb} blocks, the LDS plan holds {MAXB}"
    rec = [tuple(int(t) for t in d["plan"][b]) for b in range(b0, b1)]
    last = rec[-1]
    rec += [(last[0] + last[2], last[1] + last[3], 0, 0, last[4], 0, 0, 0)] * (2 * D + 2)
    visited = -(-nb // D) * D                      # lb = 0 .. visited - 1 go through the loop body
    issued = visited + D                           # lb = 0 .. issued - 1 are issued
    assert issued <= len(rec) and visited <= len(rec) - 1, f"run {g}: the loop reads behind the sentinels"  # (s_plan[2 (lb + 1) + 1])
    clast = n - 1
    loads = []
    for lb in range(issued):
        x0 = rec[lb][4]
        loads.append((min(x0, clast), min(x0 + T - 1, clast)))
    qx, qy = rec[0][4], rec[0][5]
    chi = min(max(qx + qy, qx + T) - 1, clast)
    loads.append((min(qx, chi), min(qx + FILL * T - 1, chi)))
    assert qy <= FILL * T, f"run {g}: the first block brings {qy} new columns, the fill loads {FILL * T}"
    stores, named = [], []
    for lb in range(visited):
        r0, p0, rows, nnz, new_lo, new_cnt = rec[lb][:6]
        assert rows <= T, f"run {g}, block {b0 + lb}: {rows} rows for {T} lanes"
        if lb > 0:
            assert new_cnt <= T, f"run {g}, block {b0 + lb}: {new_cnt} new columns for {T} lanes"
        assert new_cnt == 0 or new_lo + new_cnt - 1 <= clast, f"run {g}, block {b0 + lb}: new columns behind the last column"
        if rows > 0:
            stores.append((r0, r0 + rows))
        if lb < nb and nnz > 0:
            named.append((p0, p0 + nnz))
    return loads, stores, named


def check(d, n, p, c, D, eligible, max_deps=None):
    """Hold the dumped plan and lists to the kernel's loads and stores; `eligible`, `max_deps`: what mi_spmk_plan_probe said.
    Returns dict(live, idle, max_list, empty_runs) for the caller's own pins."""
    assert D in (2, 4)
    assert d["T"] == T and d["wgs"] >= 8 and d["wgs"] % 8 == 0, (d["T"], d["wgs"])
    W = d["wgs"]
    touches = [run_touches(d, n, D, g) for g in range(W)] if d["lean"] else None
    # every row is stored by exactly one run ("all rows in the loop")
    count = np.zeros(n, np.int64)
    owner = np.full(n, -1, np.int64)
    if touches:
        for g, (_, stores, _) in enumerate(touches):
            for r0, r1 in stores:
                count[r0:r1] += 1
                owner[r0:r1] = g
    all_in_loop = bool(touches) and bool((count == 1).all())
    if not d["in_loop"]:
        # a PLAIN block hides its rows from the loop (all_in_loop false), a plain run keeps them in records the ring loop never sees
        assert not eligible, "the probe calls a plan eligible whose rows are not all computed in the ring loop"
        return dict(live=0, idle=W, max_list=0, empty_runs=0, all_in_loop=all_in_loop)
    assert d["lean"] and all_in_loop, f"rows stored {count.min()} .. {count.max()} times"
    dp, dr = d["dep_ptr"], d["dep_run"]
    assert dp[0] == 0 and dp[W] == len(dr) and (np.diff(dp) >= 0).all()
    live = np.array([len(t[1]) > 0 for t in touches])
    listed_anywhere = np.zeros(W, bool)
    max_list = empty_runs = 0
    for g in range(W):
        lst = dr[dp[g]:dp[g + 1]]
        loads, stores, named = touches[g]
        if not live[g]:
            assert len(lst) == 0, f"idle run {g} has a list"
            assert not loads, f"run {g} has blocks and no rows"  # (every block takes at least one row)
            continue
        assert len(np.unique(lst)) == len(lst), f"run {g}: a run is listed twice"
        assert ((lst >= 0) & (lst < W)).all() and live[lst].all(), f"run {g} lists a run without rows"
        listed_anywhere[lst] = True
        max_list = max(max_list, len(lst))
        on = np.zeros(W, bool)
        on[lst] = True
        for lo, hi in loads:
            assert 0 <= lo <= hi < n, (g, lo, hi)
            own = np.unique(owner[lo:hi + 1])
            assert on[own].all(), f"D={D}: run {g} loads x[{lo}..{hi}], rows of runs {own[~on[own]]} which are not on its list {lst}"
        nnz_named = 0
        for p0, p1 in named:
            own = np.unique(owner[c[p0:p1]])
            assert on[own].all(), f"run {g} names columns of runs {own[~on[own]]} which are not on its list {lst}"
            nnz_named += p1 - p0
        empty_runs += nnz_named == 0
    assert not listed_anywhere[~live].any(), "an idle run is on somebody's list"
    assert eligible == (max_list <= MAX_LIST), (eligible, max_list)
    if max_deps is not None:
        assert max_deps == max_list, (max_deps, max_list)
    return dict(live=int(live.sum()), idle=int(W - live.sum()), max_list=max_list, empty_runs=int(empty_runs), all_in_loop=True)
