"""KhtPool, the host work pool of compvhip_plan_houghkht (compv_amd/csrc/kht_pool.hpp), under the thread sanitizer and under the address +
undefined-behaviour sanitizers: tests/host/kht_pool_stress.cpp is a program of its own (standard library only, no GPU), built with the host C++
compiler and run as a child process."""
import os
import shutil
import subprocess

import pytest

from host_programs import build, host_cxx

FLAGS = ["-std=c++17", "-O1", "-g", "-pthread"]
# the sanitizer's runtime is linked statically: the program then starts whatever other libraries its process loads, and in whatever order
SANITIZERS = {"thread": ["-fsanitize=thread", "-static-libtsan"], "address,undefined": ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"]}


@pytest.mark.parametrize("sanitize", sorted(SANITIZERS))
def test_kht_pool_stress_is_clean_under_sanitizer(tmp_path, sanitize):
    cxx = host_cxx()
    assert cxx, "no host C++ compiler"
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main(){}\n")
    flags = SANITIZERS[sanitize]
    if subprocess.run([cxx, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("%s cannot link an empty program with %s: no such runtime here" % (cxx, " ".join(flags)))
    # The runtime must also start: the thread sanitizer of some compilers aborts in front of main() ("unexpected memory mapping") on kernels with
    # high-entropy address randomisation.  The empty program decides, with randomisation switched off for the child where the system allows that.
    launch = None
    for prefix in ([shutil.which("setarch") or "setarch", os.uname().machine, "-R"], []):
        try:
            if subprocess.run([*prefix, str(tmp_path / "probe")], capture_output=True, timeout=60).returncode == 0:
                launch = prefix
                break
        except OSError:
            pass
    if launch is None:
        pytest.skip("an empty program built with %s does not start here: no usable runtime" % " ".join(flags))
    exe = build("kht_pool_stress.cpp", tmp_path, cxx, [*FLAGS, *flags])
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([*launch, str(exe)], capture_output=True, text=True, timeout=120, env=env)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert run.stderr.strip() == "", run.stderr
    assert run.stdout.strip() == "kht_pool_stress OK"
