"""for_frame_slices, the loop that launches a batch in slices of at most 65 535 frames (compv_amd/csrc/frame_slices.hpp): tests/host/frame_slices_check.cpp
is a program of its own (standard library only, no GPU), built with the host C++ compiler and run as a child process.  This is where the slicing
arithmetic is executed on its own, at frame counts up to 2^31 - 1; what the kernels do with a later slice's frame offset is executed on the GPU by
tests/test_gpu_large_batches.py (65 541, 131 073 and 524 285 frames)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "frame_slices_check.cpp")


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cxx and shutil.which(cxx):
            return cxx
    return None


def test_frame_slices_tile_the_batch_and_stop_at_the_first_error(tmp_path):
    cxx = _compiler()
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "frame_slices_check"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "frame_slices_check OK"
