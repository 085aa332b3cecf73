"""DevBuf / PinBuf, the buffers that own the handles' device and pinned memory (compv_amd/csrc/device_memory.hpp): tests/host/device_memory_check.cpp is a
program of its own that includes that header alone, built with hipcc for the host under AddressSanitizer + UBSan and run as a child process.  Without a
GPU every hipMalloc / hipHostMalloc fails, so this is where the failure paths, reserve(0), the empty release / destructor and the moves are executed; no
GPU test reaches them.  Where a GPU is present the allocations would succeed (and a sanitized program must not open a GPU): skipped."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "device_memory_check.cpp")


def _hipcc():
    for cxx in (os.environ.get("HIPCC"), "hipcc", "/opt/rocm/bin/hipcc"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


@pytest.mark.skipif(_hipcc() is None, reason="no hipcc")
@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: the allocations would succeed")
def test_buffers_stay_empty_when_allocation_fails_and_move_without_double_counting(tmp_path):
    exe = tmp_path / "device_memory_check"
    build = subprocess.run([_hipcc(), "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Xarch_host",
                            "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", SRC, "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "device_memory_check OK"
