"""The table arithmetic of a group of KHT frames (compv_amd/csrc/kht_group.hpp: string descriptors, cluster slots, the by-value tables of the batched
launches), which the host entry points use with a group of one frame and the plan call with up to kKhtBatch: tests/host/kht_group_check.cpp is a program
of its own that includes that header, built with hipcc for the host under AddressSanitizer + UBSan and run as a child process.  It opens no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "kht_group_check.cpp")


def _hipcc():
    for cxx in (os.environ.get("HIPCC"), "hipcc", "/opt/rocm/bin/hipcc"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


@pytest.mark.skipif(_hipcc() is None, reason="no hipcc")
def test_group_tables_for_one_frame_an_empty_frame_and_a_full_group(tmp_path):
    exe = tmp_path / "kht_group_check"
    build = subprocess.run([_hipcc(), "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Xarch_host",
                            "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", SRC, "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "kht_group_check OK"
