"""Host-side planners under the address and undefined-behaviour sanitizers and, where they start host threads, a second time under the
thread sanitizer (CPU only: GPU sanitizers are not available on this pool, and nothing here launches a kernel).  Every harness is a
stand-alone program that is built and run directly.  The harnesses live under tools/ (plan_asan.hip, part_asan.cpp, bilu_asan.cpp,
spmm_plan_asan.cpp, reorder_asan.cpp, gmres_drive_check.cpp, dispatch_check.cpp, ring_plan_asan.cpp, sell_plan_asan.hip; under the thread
sanitizer bilu_asan.cpp, bilu4_order_asan.cpp, ring_plan_asan.cpp and plan_asan.hip) and say what they check."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "navierstokes_amd", "csrc")


def _run(cmd, exe, tmp_path):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "ThreadSanitizer" not in r.stderr, r.stdout[-1500:] + r.stderr[-3000:]
    return r.stdout


ASAN = ["-fsanitize=address,undefined"]
TSAN = ["-fsanitize=thread"]


def _gxx(tmp_path, source, exe, sanitizer):
    """build tools/<source> with g++ under one sanitizer set and run it; its output"""
    if not shutil.which("g++"):
        pytest.skip("g++ not found")
    exe = str(tmp_path / exe)
    return _run(["g++", "-O1", "-g", "-std=c++17", "-pthread"] + sanitizer + ["-I" + CSRC, "-o", exe, os.path.join(ROOT, "tools", source)], exe, tmp_path)


def _hipcc(tmp_path, source, exe, sanitizer):
    """the same with hipcc, for a header that holds kernels: host sanitizers only"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    exe = str(tmp_path / exe)
    return _run([hipcc, "-O1", "-g", "-std=c++17", "-pthread", "--offload-arch=gfx950"] + sanitizer + ["-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", exe,
                 os.path.join(ROOT, "tools", source)], exe, tmp_path)


def _count(out, label):
    """the number printed behind `label`"""
    assert label in out, out
    return int(out.split(label)[1].split()[0])


def test_partition_planner_under_host_sanitizers(tmp_path):
    """partition.hpp: PartPlan::build, build_combined, build_all_ext (the [owned | halo] piece of the staged one-launch step, round 5) on random
    banded / multi-band / node-blocked patterns cut into 1-6 ranks; every nonzero found again under the caller's order, the 4x4 structure kept."""
    if not shutil.which("g++"):
        pytest.skip("g++ not found")
    exe = str(tmp_path / "part_asan")
    out = _run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tools", "part_asan.cpp")], exe, tmp_path)
    assert "bad 0" in out, out


def test_block_ilu_planner_under_host_sanitizers(tmp_path):
    """bilu4_plan.hpp: the schedule (off-diagonal ranges, launches and the folding rule), the host factorisation with 1 and 4 threads, the
    device refactor's plan and the one-launch solve's plan replayed for 1, 2, 7 and 256 workgroups, every table checked by brute force on
    the empty matrix, a diagonal one, a chain, random patterns at fill 0-3 and layered patterns with levels of 1, 63, 64, 65 and 129 rows."""
    if not shutil.which("g++"):
        pytest.skip("g++ not found")
    exe = str(tmp_path / "bilu_asan")
    out = _run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tools", "bilu_asan.cpp")], exe, tmp_path)
    assert "bad 0" in out, out
    _check_bilu_counts(out)


def _check_bilu_counts(out):
    """tools/bilu_asan.cpp's own enumeration: at each fill 0-3 the empty, the diagonal and the chain matrix and 12 random patterns; at fill
    0 eight layered shapes with 0 and 3 extra links, a strictly lower pattern and 12 that lost some (j, i) blocks.  Every fill-0 pattern
    gets the DILU device plan without and with a src table; every planted corruption of it is reported."""
    fill0 = (3 + 12) + 8 * 2 + 1 + 12
    assert _count(out, "block ILU plans: patterns") >= 3 * (3 + 12) + fill0, out
    assert _count(out, "DILU device plans") >= 2 * fill0, out
    # three corruptions per plan (a mate moved, a gather entry duplicated, two fpos entries swapped) wherever the plan has two blocks to
    # tell apart: all 12 dropped-mate patterns and the 12 random ones of fill 0 have, without and with src
    assert _count(out, "teeth planted") >= 3 * 2 * (12 + 12) - 2 * 12, out  # (a random pattern may have no mated pair: that one corruption is then not planted)
    assert _count(out, "teeth planted") == _count(out, "caught"), out


def test_sliced_stream_planners_under_host_sanitizers(tmp_path):
    """spmv_sstream.hpp / spmv_sstream_mw.hpp: both planners and their host replays on random multi-band patterns, both row shifts."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    exe = str(tmp_path / "plan_asan")
    out = _run([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-I" + CSRC,
                "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tools", "plan_asan.hip")], exe, tmp_path)
    assert "bad 0" in out and "eligible" in out, out


def test_spmm_tile_planner_under_host_sanitizers(tmp_path):
    """spmm_tile_plan.hpp: the tile plan of the multi-vector product's forms 1-3 on the pattern families of tests/spmm_tile_cases.py and on
    random unsymmetric patterns, 128 and 64 rows per tile, default and small caps, rows sorted and in growth order, every array checked by
    brute force; the 16-bit refusal and the matrices with nothing to list."""
    if not shutil.which("g++"):
        pytest.skip("g++ not found")
    exe = str(tmp_path / "spmm_plan_asan")
    out = _run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tools", "spmm_plan_asan.cpp")], exe, tmp_path)
    assert "bad 0" in out, out


def test_relabelling_under_host_sanitizers(tmp_path):
    """reorder.hpp: the node graph, Cuthill-McKee, the permutation and the permuted CSR with its value offsets, checked by brute force on the
    pattern families of tests/reorder_cases.py (generated in C++) and on 220 random patterns with empty rows, repeated columns and a 300-entry
    row, each as a scalar matrix (block 1) and expanded to 4x4 node blocks (block 4); the spread figures against a direct sum."""
    if not shutil.which("g++"):
        pytest.skip("g++ not found")
    exe = str(tmp_path / "reorder_asan")
    out = _run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tools", "reorder_asan.cpp")], exe, tmp_path)
    assert "bad 0" in out and "reorder patterns" in out, out
    assert int(out.split("reorder patterns")[1].split()[0]) >= 2 * 200, out


def test_gmres_host_loop_under_host_sanitizers(tmp_path):
    """gmres_drive.hpp: the host loop of mi_gmres_solve_dev and mi_gmres_plan_solve over a scripted device, eager and planned, restart
    in {1, 2, 5} x six maxiter x four check_every / segment x both bases x (6 restart + 6) scripts: results against a loop with no
    pipeline, slot safety, no idle device inside a cycle, what may be enqueued, the header's waste and read-back bounds."""
    if not shutil.which("g++"):
        pytest.skip("g++ not found")
    exe = str(tmp_path / "gmres_drive_check")
    out = _run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tools", "gmres_drive_check.cpp")], exe, tmp_path)
    assert "bad 0" in out and "gmres_drive cases" in out, out
    assert int(out.split("gmres_drive cases")[1].split()[0]) >= sum(6 * 4 * 2 * (6 * m + 6) for m in (1, 2, 5)), out


def test_launch_dispatch_helpers_under_host_sanitizers(tmp_path):
    """dispatch.hpp: pick hands fn the compile-time twins of one to four runtime flags (all 2 + 4 + 8 + 16 combinations), calls it once and
    returns its value; pick_int hands over every listed value as itself and an unlisted one (negative, zero, one past the largest, INT_MAX)
    as the last listed; launch_grid gives the grids the launch sites used to write out."""
    if not shutil.which("g++"):
        pytest.skip("g++ not found")
    exe = str(tmp_path / "dispatch_check")
    out = _run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tools", "dispatch_check.cpp")], exe, tmp_path)
    assert "bad 0" in out and "dispatch cases" in out, out
    assert int(out.split("dispatch cases")[1].split()[0]) >= 2 + 4 + 8 + 16, out


def _check_ring_counts(out):
    """tools/ring_plan_asan.cpp's own enumeration: ten families at eleven sizes and 30 random patterns, each with the four ring
    configurations x three workgroup units x three row alignments x ghost range off / on, the multi-ring plan at three row alignments
    x two skews, the tile plan at two row alignments x four thread counts; one large pattern the same, but for the ring only with the
    configurations' own unit at the default alignment."""
    small, large = 10 * 11 + 30, 1
    assert "bad 0" in out, out
    assert _count(out, "tile plans: patterns") >= small + large, out
    assert _count(out, "ring plans") >= small * 4 * 3 * 3 * 2 + large * 4 * 1 * 1 * 2, out
    assert _count(out, "multi-ring plans") >= (small + large) * 3 * 2, out
    assert _count(out, "tile plans") >= (small + large) * 2 * 4, out
    # configuration 4 on the narrow band (square, every run inside the ring loop) at every size but 0: three units x three alignments x two
    assert _count(out, "run-dependency lists") >= 10 * 3 * 3 * 2, out
    # corruptions: the ring checker on three patterns x four configurations, at least four each; check_mring_plan on the large pattern at
    # two skews, at least four each; check_tile_plan on three patterns, five each
    assert _count(out, "teeth planted") >= 3 * 4 * 4 + 2 * 4 + 3 * 5, out
    assert _count(out, "teeth planted") == _count(out, "caught"), out


def test_ring_mring_tile_planners_under_host_sanitizers(tmp_path):
    """ring_plan.hpp, mring_plan.hpp, tile_plan.hpp: every plan checked by brute force (blocks and runs cover the matrix once, every
    nonzero's column is in its window and in its 16-bit slot when its block runs, flags, LEAN, run dependencies, the censuses against
    direct counts, the kernels' unclamped indices inside the padding), the tile plan the same at 0, 1, 3 and 16 threads, and corruptions
    planted in built plans that each checker must report."""
    _check_ring_counts(_gxx(tmp_path, "ring_plan_asan.cpp", "ring_plan_asan", ASAN))


def test_sell_planner_under_host_sanitizers(tmp_path):
    """spmv_bcsr_sell.hpp: build_sell_plan and build_sell_wave_ranges on 70 patterns (11 row counts, 9 slice counts, 3 heavy slices, 2 equal
    shapes, 5 single limits, 40 random) x four wave caps, the wave ranges again through their own door over all and over three slices:
    every block in exactly one step in its row's order, padding places marked, the ranges a partition balanced by steps, direct counts."""
    out = _hipcc(tmp_path, "sell_plan_asan.hip", "sell_plan_asan", ASAN + ["-fno-gpu-sanitize"])
    assert "bad 0" in out, out
    assert _count(out, "sliced block plans: cases") >= (11 + 9 + 3 + 2 + 5 + 40) * 4 * (1 + 2), out


def test_block_ilu_planner_under_thread_sanitizer(tmp_path):
    """tools/bilu_asan.cpp again, under the thread sanitizer: the level loop the factorisation and the DILU pivots share, at 3, 4 and 16 threads."""
    out = _gxx(tmp_path, "bilu_asan.cpp", "bilu_tsan", TSAN)
    assert "bad 0" in out, out
    _check_bilu_counts(out)


def test_block_ilu_ordering_under_thread_sanitizer(tmp_path):
    """tools/bilu4_order_asan.cpp again, under the thread sanitizer: the factorisation through the src table at 4 threads."""
    assert "bad 0" in _gxx(tmp_path, "bilu4_order_asan.cpp", "bilu4_order_tsan", TSAN)


def test_ring_mring_tile_planners_under_thread_sanitizer(tmp_path):
    """tools/ring_plan_asan.cpp again, under the thread sanitizer: the tile planner's pool at 3 and 16 threads on every pattern, and sized by
    itself on the pattern of three million nonzeros."""
    _check_ring_counts(_gxx(tmp_path, "ring_plan_asan.cpp", "ring_plan_tsan", TSAN))


def test_sliced_stream_planners_under_thread_sanitizer(tmp_path):
    """tools/plan_asan.hip again, its host code under the thread sanitizer: both sliced-stream planners sort and fill over the host's threads."""
    out = _hipcc(tmp_path, "plan_asan.hip", "plan_tsan", ["-Xarch_host"] + TSAN)
    assert "bad 0" in out and "eligible" in out, out
