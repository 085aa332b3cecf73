"""The decisions around an asynchronous pipeline step (compv_amd/csrc/step_policy.hpp): the sort range compvhip_plan_pipeline_async predicts, what
compvhip_plan_wait concludes from a step's round flags and line total (rounds needed, replay or not) and the speculative rounds of the next step.  On a GPU
they only show when a frame happens to need a fourth round; tests/host/step_policy_check.cpp is a program of its own that includes that header alone, built
with hipcc for the host under AddressSanitizer + UBSan and run as a child process.  It opens no GPU, so it runs wherever hipcc does."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "step_policy_check.cpp")


def _hipcc():
    for cxx in (os.environ.get("HIPCC"), "hipcc", "/opt/rocm/bin/hipcc"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


@pytest.mark.skipif(_hipcc() is None, reason="no hipcc")
def test_sort_range_wait_verdict_and_next_rounds(tmp_path):
    exe = tmp_path / "step_policy_check"
    build = subprocess.run([_hipcc(), "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Xarch_host",
                            "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", SRC, "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "step_policy_check OK"
