"""Host-side planners under the address and undefined-behaviour sanitizers (CPU only: GPU sanitizers are not available on this pool, and
nothing here launches a kernel).  The harnesses live under tools/ (plan_asan.hip, part_asan.cpp, bilu_asan.cpp, spmm_plan_asan.cpp, reorder_asan.cpp, gmres_drive_check.cpp, dispatch_check.cpp) and say what they check."""
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
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout[-1500:] + r.stderr[-3000:]
    return r.stdout


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
