"""The F plan's point order (csrc/f8_order.h) without a device: tests/f8_order_check.cpp is compiled
host-only, the way the Makefile compiles the .cpp sources, and run.  It checks the permutation
builder (a permutation for every subset pattern of n <= 12, the identity cases, the winner's
outliers before its inliers and each ascending, lists that are no index sets), when a read flush
installs, the layout of the ordered copies, and the drop rule of the pruned count under the
permuted order on random certificate planes.  The same program is built once more with the host's
address and undefined-behaviour sanitizers and run directly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tsbb15-3d-reconstruction-project_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_f8_order(tmp_path, sanitize):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "f8_order_check")
    opt = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O3"]
    cmd = [hipcc, *opt, "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-Wall", "-Werror", "-x", "c++",
           os.path.join(ROOT, "tests", "f8_order_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "f8 order ok"
