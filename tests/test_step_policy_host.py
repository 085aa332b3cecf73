"""The decisions around an asynchronous pipeline step (compv_amd/csrc/step_policy.hpp): the sort range compvhip_plan_pipeline_async predicts, what
compvhip_plan_wait concludes from a step's round flags and line total (rounds needed, replay or not) and the speculative rounds of the next step.  On a GPU
they only show when a frame happens to need a fourth round; tests/host/step_policy_check.cpp is a program of its own that includes that header alone, built
with hipcc for the host under AddressSanitizer + UBSan and run as a child process.  It opens no GPU, so it runs wherever hipcc does."""
import subprocess

import pytest

from host_programs import HIPCC_ASAN_UBSAN, HIPCC_HOST_ONLY, WARN, build, hipcc


@pytest.mark.skipif(hipcc() is None, reason="no hipcc")
def test_sort_range_wait_verdict_and_next_rounds(tmp_path):
    exe = build("step_policy_check.cpp", tmp_path, hipcc(), [*HIPCC_HOST_ONLY, "-O1", "-g", *WARN, *HIPCC_ASAN_UBSAN])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "step_policy_check OK"
