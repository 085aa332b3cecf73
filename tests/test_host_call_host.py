"""HostCall, the frame of the calls that stage the caller's host memory (compv_amd/csrc/host_call.hpp): tests/host/host_call_check.cpp is a program of its
own that includes that header alone and DEFINES the five runtime functions the header calls (the asynchronous and blocking copies, hipStreamSynchronize), so
that they record the call sequence and fail where a script says.  Built with hipcc for the host under AddressSanitizer + UBSan, linked into the program, and
run as a child process.  This is where the drain on every way out of a call, the sticky first failure and the synchronisation counts are executed: a healthy
GPU never reaches the failure paths, and no GPU test may provoke one.  Where a GPU is present a sanitized program must not run beside it: skipped."""
import os
import subprocess

import pytest

from host_programs import HIPCC_ASAN_UBSAN, HIPCC_HOST_ONLY, WARN, build, hipcc


@pytest.mark.skipif(hipcc() is None, reason="no hipcc")
@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: sanitized host programs run where there is none")
def test_frame_skips_behind_a_failure_and_drains_once_on_every_way_out(tmp_path):
    exe = build("host_call_check.cpp", tmp_path, hipcc(), [*HIPCC_HOST_ONLY, "-O1", "-g", *WARN, *HIPCC_ASAN_UBSAN])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "host_call_check OK"
