"""The ownership paths of the partition and mi_dist handles, which the other suites pass through once each: everything such a
handle can come to own — the two pieces and the send index, the receive window with its registry entry, the link and work tables,
the combined piece of every one-launch form with its run links, staged ghosts and unit lists, the RCCL exchange with its stream,
events and buffers, the all-gather tables, the give-up word, and per mi_dist rank the stream, events, scalars and vectors — built,
used, given up (mi_part_push_unfuse, mi_part_push_disable), built again and released; then the same lives over and over with the
free device memory watched.  One test, one child process (tests/multirank_worker.py lifecycle: the library reads
MI355_SPMV_LIBRARY and MI355_RCCL_LIBRARY once per process).  Nothing is provoked.

One cycle: a push life of two ranks on a blocked FE matrix (spmv_bcsr4_fused_ext) and one on a scalar band (ring / sliced stream /
staged scalar step by cycle % 3, asserted through mi_part_kernel_name(P, 2)), both driven as PushRanks.sweep does — pushes looped
back, flags preset, one rank at a time, three sweeps — and one mi_dist life under each of the event, RCCL send/recv and RCCL
all-gather exchanges (tests/fake_rccl, every rank on device 0), one of whose device vectors is still open when the handle is
destroyed.  Every product is compared bit for bit with the oracle.  At most 2 + 8 rank handles exist at a time."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import multirank_worker as W
from conftest import ROOT

pytestmark = pytest.mark.gpu

CYCLES = 25
DEVLIB = os.path.join(ROOT, "navierstokes_amd", "csrc", "libmi355spmv_dev.so")
FAKE = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")


def _smallest_rank_values(P, align):
    """bytes of the smaller of the two ranks' value arrays (the combined piece holds all of a rank's nonzeros)"""
    from navierstokes_amd import dist
    rs = dist.balanced_row_starts(len(P) - 1, 2, np.diff(P), align=align)
    return 8 * min(int(P[rs[r + 1]] - P[rs[r]]) for r in range(2))


def test_partition_and_dist_handles_own_what_they_build_and_free_all_of_it():
    """Steady state, not the first cycles (the runtime and torch's allocator keep what they first took): free device memory after
    the last cycle must not be below free memory after cycle 4.  What this can see: the pieces (interior, boundary, combined) and
    anything else above the 2 MiB granule device memory is handed out in — every rank's combined piece has a value array larger
    than that (asserted below), so one leaked piece per cycle is certain to show.  That the small tables, the streams and the events
    go rests on the owning members (dev_array.hpp) being the handles' only release path, not on this test."""
    from navierstokes_amd import synth
    if not os.path.exists(FAKE):
        pytest.skip("tests/fake_rccl not built")
    assert os.path.exists(DEVLIB), "the devtools build (make devtools; __graft_entry__.build) is missing"
    assert _smallest_rank_values(synth.fe_matrix(W.FE_CELLS)[0], 4) > W.GRANULE, "a rank's value array of the FE matrix fits the granule"
    assert _smallest_rank_values(synth.fe_matrix(W.FE_CELLS - 1)[0], 4) <= W.GRANULE, "a smaller FE matrix would do"
    assert _smallest_rank_values(synth.rows("s15", W.S15_ROWS, w=W.S15_WIDTH)[0], 1) > W.GRANULE, "a rank's value array of the band fits the granule"
    assert _smallest_rank_values(synth.rows("s15", W.S15_ROWS - 2, w=W.S15_WIDTH)[0], 1) <= W.GRANULE, "a shorter band would do"
    env = dict(os.environ, MI355_SPMV_LIBRARY=DEVLIB, MI355_PUSH_LOOPBACK="1", MI355_RCCL_LIBRARY=FAKE)
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "multirank_worker.py"), "lifecycle", str(CYCLES)],
                       capture_output=True, text=True, env=env, timeout=270)
    print(f"{time.perf_counter() - t0:.1f} s in the child\n" + r.stdout[-1500:])
    assert r.returncode == 0 and "MULTIRANK_OK" in r.stdout, f"exit {r.returncode}\n" + r.stdout[-4000:] + r.stderr[-3000:]
    line = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("LIFECYCLE ")][0]
    assert int(line[2]) == CYCLES and int(line[6]) >= int(line[4]), line
