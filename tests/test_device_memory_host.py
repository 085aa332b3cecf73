"""DevBuf / PinBuf, the buffers that own the handles' device and pinned memory (compv_amd/csrc/device_memory.hpp): tests/host/device_memory_check.cpp is a
program of its own that includes that header alone, built with hipcc for the host under AddressSanitizer + UBSan and run as a child process.  Without a
GPU every hipMalloc / hipHostMalloc fails, so this is where the failure paths (with the fill of fresh allocations off and on), reserve(0), the empty
release / destructor and the moves are executed; no GPU test reaches them.  Where a GPU is present the allocations would succeed (and a sanitized program must not open a GPU): skipped."""
import os
import subprocess

import pytest

from host_programs import HIPCC_ASAN_UBSAN, HIPCC_HOST_ONLY, WARN, build, hipcc


@pytest.mark.skipif(hipcc() is None, reason="no hipcc")
@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: the allocations would succeed")
def test_buffers_stay_empty_when_allocation_fails_and_move_without_double_counting(tmp_path):
    exe = build("device_memory_check.cpp", tmp_path, hipcc(), [*HIPCC_HOST_ONLY, "-O1", "-g", *WARN, *HIPCC_ASAN_UBSAN])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "device_memory_check OK"
