"""One recipe for the stand-alone host checks under tests/host: each is a program of its own, built by the test that runs it as a child process.  The
sanitizers' runtimes are linked into the program (statically with the host compiler), so nothing is preloaded anywhere.  A test names its own opt level,
-g, -ffp-contract=off and sanitizer set; how the program is run and what is asserted about it stays with the test."""
import os
import pathlib
import shutil
import subprocess

HOST_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host")

WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror"]
ASAN_UBSAN_STATIC = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]
HIPCC_HOST_ONLY = ["-x", "hip", "--offload-host-only"]          # a header that includes the HIP runtime's, compiled for the host alone: no GPU is opened
HIPCC_ASAN_UBSAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]


def host_cxx():
    """the host C++ compiler's name, or None"""
    return next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)


def hipcc():
    """the path of hipcc, or None"""
    return next((shutil.which(c) for c in (os.environ.get("HIPCC"), "hipcc", "/opt/rocm/bin/hipcc") if c and shutil.which(c)), None)


def build(src_name, out_dir, compiler, flags):
    """tests/host/<src_name> -> the program <out_dir>/<src_name without its suffix>"""
    assert compiler, "no compiler to build %s with" % src_name
    exe = pathlib.Path(out_dir) / os.path.splitext(src_name)[0]
    done = subprocess.run([compiler, *flags, os.path.join(HOST_DIR, src_name), "-o", str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, "%s %s: exit %d\n%s" % (compiler, src_name, done.returncode, done.stderr)
    return exe
