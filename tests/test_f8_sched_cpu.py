"""The F plan's host decisions (csrc/f8_sched.h) without a device: tests/f8_sched_check.cpp is
compiled host-only, the way the Makefile compiles the .cpp sources, and run.  It checks the arena
layout (every buffer inside its arena, disjoint, 256-aligned, the element counts, a regrow that
moves nothing per hypothesis), the lane placement and the set guard over the call sequences of
tests/test_gpu_lanes.py and over every run / result sequence of up to 12 calls, the count path
(staged, carried, when the carry words are dropped) and the numbers of the pruned count."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tsbb15-3d-reconstruction-project_amd", "csrc")


def test_f8_sched(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "f8_sched_check")
    cmd = [hipcc, "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-Wall", "-Werror", "-x", "c++",
           os.path.join(ROOT, "tests", "f8_sched_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "f8 sched ok"
