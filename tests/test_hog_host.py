"""compv_amd/csrc/hog_math.hpp -- the arithmetic the HOG kernels are made of -- run on the host by tests/host/hog_math_check.cpp (a stand-alone program,
standard library only, no GPU, built with AddressSanitizer and UBSan) over the frames of the golden cases, and held against tests/hog_model.py and the
golden descriptors byte for byte.  The GPU tests (tests/test_gpu_hog.py) hold the kernels against the same model."""
import struct
import subprocess

import numpy as np
import pytest

import hog_cases as hc
import hog_model as hm
from fixtures import load_golden
from host_programs import ASAN_UBSAN_STATIC, WARN, build, host_cxx

GEOMETRY = ["cellsX", "cellsY", "validX", "validY", "blocksX", "blocksY", "cpbX", "cpbY", "stepX", "stepY"]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = build("hog_math_check.cpp", tmp_path_factory.mktemp("hog"), host_cxx(), ["-O1", "-g", "-ffp-contract=off", *WARN, *ASAN_UBSAN_STATIC])

    def run(img, opts):
        o = hm.resolve(opts)
        H, W = img.shape
        g = hm.geometry(W, H, o)
        d = exe.parent
        with open(d / "in.bin", "wb") as f:
            f.write(struct.pack("<22i", W, H, *[o[k] for k in hm.FIELDS], *[g[k] for k in GEOMETRY]))
            f.write(np.ascontiguousarray(img, np.uint8).tobytes())
        r = subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr          # a sanitizer report goes to stderr
        raw = np.fromfile(d / "out.bin", np.float32)
        n = g["cellsY"] * g["cellsX"] * o["nbins"]
        assert raw.size == n + g["descLen"]
        return raw[n:], raw[:n].reshape(g["cellsY"], g["cellsX"], o["nbins"])
    return run


@pytest.fixture(scope="module")
def golden():
    meta, arrays = load_golden("golden_hog")
    return {c["id"]: c for c in meta["cases"]}, arrays


@pytest.mark.parametrize("cid", [c["id"] for c in hc.CASES])
def test_header_equals_model_and_golden(checker, golden, cid):
    by_id, arrays = golden
    c = hc.BY_ID[cid]
    img = hc.case_frame(c)
    desc, cells = checker(img, c["opts"])
    exp_desc, exp_cells = hm.hog(img, c["opts"])
    assert cells.tobytes() == exp_cells.tobytes()
    assert desc.tobytes() == exp_desc.tobytes()
    if by_id[cid]["stored"]:
        assert desc.tobytes() == arrays["desc_" + cid].tobytes()


def test_header_equals_model_on_other_frames(checker):
    """the frames the GPU tests add behind the golden one (other seeds), and a frame whose every pixel is a border pixel of some kind"""
    for kind, seed in (("noise", 2), ("blocks", 3), ("checkerboard", 1)):
        for o in (hc.LAYOUTS["b8s4c8"], hc.layout(16, 8, 8, signed=False, interp=hm.INTERP_NEAREST), hc.layout(8, 8, 8, 15, norm=hm.NORM_L1SQRT, signed=False)):
            img = hc.frame(kind, 37, 29, seed)
            desc, cells = checker(img, o)
            exp_desc, exp_cells = hm.hog(img, o)
            assert cells.tobytes() == exp_cells.tobytes() and desc.tobytes() == exp_desc.tobytes(), (kind, seed, o)
    img = hc.noise(2, 2, 5)
    o = hc.layout(2, 1, 2, 4, norm=hm.NORM_L2)          # stride = cell / 2 with block == cell, down to a 2 x 2 frame: all gradients are 0
    desc, cells = checker(img, o)
    assert not desc.view(np.uint32).any() and desc.tobytes() == hm.hog(img, o)[0].tobytes()
