"""The scratch layout of csrc/host.h without a device: tests/host_layout_check.cpp is compiled
host-only, the way the Makefile compiles the .cpp sources, and run.  It checks offsets against
the prefix sums of the 256-padded sizes for a list with zeros, non-multiples of 256, exactly 256
and a size above 4 GiB, the total, the ranges and the packed variant."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tsbb15-3d-reconstruction-project_amd", "csrc")


def test_layout_arithmetic(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "host_layout_check")
    cmd = [hipcc, "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-Wall", "-Werror", "-x", "c++",
           os.path.join(ROOT, "tests", "host_layout_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "layout ok"
