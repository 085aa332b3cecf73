"""The table arithmetic of a group of KHT frames (compv_amd/csrc/kht_group.hpp: string descriptors, cluster slots, the by-value tables of the batched
launches), which the host entry points use with a group of one frame and the plan call with up to kKhtBatch: tests/host/kht_group_check.cpp is a program
of its own that includes that header, built with hipcc for the host under AddressSanitizer + UBSan and run as a child process.  It opens no GPU."""
import subprocess

import pytest

from host_programs import HIPCC_ASAN_UBSAN, HIPCC_HOST_ONLY, WARN, build, hipcc


@pytest.mark.skipif(hipcc() is None, reason="no hipcc")
def test_group_tables_for_one_frame_an_empty_frame_and_a_full_group(tmp_path):
    exe = build("kht_group_check.cpp", tmp_path, hipcc(), [*HIPCC_HOST_ONLY, "-O1", "-g", *WARN, *HIPCC_ASAN_UBSAN])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "kht_group_check OK"
