"""compv_amd/csrc/bicubic_math.hpp -- the arithmetic the bicubic kernel is made of, and the rule by which it reads a tap row as one 4-byte word -- run on
the host by tests/host/bicubic_math_check.cpp (a stand-alone program, standard library only, no GPU, built with AddressSanitizer and UBSan, nothing
preloaded) over every case's frame and coordinates, and held against tests/bicubic_model.py and the fixture byte for byte.  The GPU tests
(tests/test_gpu_bicubic.py) hold the kernel against the same model and the same fixture."""
import struct
import subprocess

import numpy as np
import pytest

import bicubic_cases as bc
import bicubic_model as bm
import remap_cases as rc
import remap_model as rm
from fixtures import load_golden
from host_programs import ASAN_UBSAN_STATIC, WARN, build, host_cxx

A = load_golden("golden_bicubic")[1]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = build("bicubic_math_check.cpp", tmp_path_factory.mktemp("bicubic"), host_cxx(), ["-O2", "-g", "-ffp-contract=off", *WARN, *ASAN_UBSAN_STATIC])

    def run(img, S, x, y, roi, default):
        """-> (uint8 plane, float32 plane) of the frame img staged at stride S"""
        h, w = img.shape
        ho, wo = x.shape
        frame = np.full((h, S), 0xA5, np.uint8)
        frame[:, :w] = img
        d = exe.parent
        with open(d / "in.bin", "wb") as f:
            f.write(struct.pack("<6i", w, h, S, wo, ho, default))
            f.write(np.array(rm.clip_roi(roi, w, h), np.float32).tobytes())
            f.write(frame.tobytes() + np.ascontiguousarray(x, np.float32).tobytes() + np.ascontiguousarray(y, np.float32).tobytes())
        r = subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr          # a sanitizer report goes to stderr
        raw = np.fromfile(d / "out.bin", np.uint8)
        assert raw.size == 5 * wo * ho
        return raw[:wo * ho].reshape(ho, wo), raw[wo * ho:].view(np.float32).reshape(ho, wo)
    return run


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def check(checker, c, x, y, strides):
    w, h, _, _ = c["size"]
    img = rc.frame(w, h, c["seed"])
    exp = {i: bm.remap(img, x, y, i, c.get("roi"), c["default"]) for i in bc.INTERPS}
    for S in strides:
        u8, f32 = checker(img, S, x, y, c.get("roi"), c["default"])
        for interp, got in ((bm.BICUBIC, u8), (bm.BICUBIC_FLOAT32, f32)):
            assert same(got, exp[interp]), "%s S %d %s: the header against the model" % (c["id"], S, bc.INTERP_NAMES[interp])
            assert same(got, A[bc.key(c["id"], interp)]), "%s S %d %s: the header against the fixture" % (c["id"], S, bc.INTERP_NAMES[interp])


@pytest.mark.parametrize("c", bc.all_map_cases(), ids=lambda c: c["id"])
def test_header_equals_model_and_fixture_on_the_maps(checker, c):
    w = c["size"][0]
    # a narrow source at the stride of its case (below 4: byte loads; from 4 on: the 4-byte word) and at the next one; the others tight and padded
    check(checker, c, *bc.map_of(c), (c["S"], c["S"] + 1) if "S" in c else (w, w + 3))


@pytest.mark.parametrize("c", bc.warp_cases(), ids=lambda c: c["id"])
def test_header_equals_model_and_fixture_on_the_matrices(checker, c):
    w, _, wo, ho = c["size"]
    check(checker, c, *rm.warp_coords(c["M"], wo, ho), (w,))


def test_the_narrow_cases_cover_both_ways_of_reading_a_row():
    strides = [c["S"] for c in bc.narrow_cases()]
    assert min(strides) < 4 <= max(strides) and 4 in strides
    assert {c["size"][0] for c in bc.narrow_cases()} >= {1, 3, 4, 5}
