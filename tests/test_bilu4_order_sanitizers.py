"""bilu4_order.hpp under the host address and undefined-behaviour sanitizers (CPU only; nothing here launches a kernel): the harness
tools/bilu4_order_asan.cpp says what it checks."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "navierstokes_amd", "csrc")


def test_block_ilu_ordering_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "bilu4_order_asan")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tools", "bilu4_order_asan.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout[-1500:] + r.stderr[-3000:]
    assert "bad 0" in r.stdout, r.stdout
