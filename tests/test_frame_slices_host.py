"""for_frame_slices, the loop that launches a batch in slices of at most 65 535 frames (compv_amd/csrc/frame_slices.hpp): tests/host/frame_slices_check.cpp
is a program of its own (standard library only, no GPU), built with the host C++ compiler and run as a child process.  This is where the slicing
arithmetic is executed on its own, at frame counts up to 2^31 - 1; what the kernels do with a later slice's frame offset is executed on the GPU by
tests/test_gpu_large_batches.py (65 541, 131 073 and 524 285 frames)."""
import subprocess

from host_programs import WARN, build, host_cxx


def test_frame_slices_tile_the_batch_and_stop_at_the_first_error(tmp_path):
    exe = build("frame_slices_check.cpp", tmp_path, host_cxx(), ["-O1", *WARN])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "frame_slices_check OK"
