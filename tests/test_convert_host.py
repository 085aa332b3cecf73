"""compv_amd/csrc/convert_math.hpp -- the arithmetic the colour conversion kernel is made of -- run on the host by tests/host/convert_math_check.cpp (a
stand-alone program, standard library only, no GPU, built with AddressSanitizer and UBSan, nothing preloaded) over the small cases and both exhaustive
frames, and held against tests/convert_model.py and the golden MD5s byte for byte.  The GPU tests (tests/test_gpu_convert.py) hold the kernel against the
same model and the same fixture."""
import struct
import subprocess

import numpy as np
import pytest

import convert_cases as cc
import convert_model as cm
from fixtures import load_golden, md5
from host_programs import ASAN_UBSAN_STATIC, WARN, build, host_cxx


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = build("convert_math_check.cpp", tmp_path_factory.mktemp("convert"), host_cxx(), ["-O2", "-g", "-ffp-contract=off", *WARN, *ASAN_UBSAN_STATIC])

    def run(src, dst, W, H, planes=None):
        """planes None: the program generates the exhaustive frame itself.  Returns the destination's dense planes."""
        d = exe.parent
        with open(d / "in.bin", "wb") as f:
            f.write(struct.pack("<5i", src, dst, W, H, 1 if planes is None else 0))
            for p in planes or ():
                f.write(np.ascontiguousarray(p, np.uint8).tobytes())
        r = subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr          # a sanitizer report goes to stderr
        raw = np.fromfile(d / "out.bin", np.uint8)
        out, off = [], 0
        for rows, cols in cm.plane_shapes(dst, W, H):
            out.append(raw[off:off + rows * cols].reshape(rows, cols))
            off += rows * cols
        assert off == raw.size
        return out
    return run


@pytest.fixture(scope="module")
def golden():
    meta, arrays = load_golden("golden_convert")
    return {c["id"]: c for c in meta["cases"]}, arrays


@pytest.mark.parametrize("src", cc.SOURCES, ids=[cm.NAMES[s] for s in cc.SOURCES])
def test_header_equals_model_and_golden_on_the_small_cases(checker, golden, src):
    by_id, arrays = golden
    for c in cc.SMALL:
        if c["src"] != src:
            continue
        planes = cc.case_planes(c)
        for dst in cc.destinations(src):
            got = checker(src, dst, c["W"], c["H"], planes)
            exp = cm.convert(src, dst, planes, c["W"], c["H"])
            for i, (g, e) in enumerate(zip(got, exp)):
                assert g.tobytes() == e.tobytes(), (c["id"], cm.NAMES[dst], i)
                assert md5(g) == by_id[c["id"]]["md5"][cm.NAMES[dst]][i]
                assert g.tobytes() == arrays[cc.key(c, dst, i)].tobytes()


@pytest.mark.parametrize("src,dst", [(cm.YUV444P, cm.RGBA32), (cm.YUV444P, cm.RGB24), (cm.YUV444P, cm.HSV), (cm.RGB24, cm.HSV), (cm.RGB24, cm.YUV444P), (cm.RGB24, cm.BGR24)],
                         ids=lambda v: cm.NAMES[v])
def test_header_equals_golden_on_the_exhaustive_frames(checker, golden, src, dst):
    """every (Y, U, V) and every (R, G, B) once: every clamp, every entry of both HSV tables -- what the compiled reference gave, by MD5"""
    by_id, _ = golden
    c = by_id["%s_exhaustive4096x4096" % cm.NAMES[src]]
    assert c["checked"][cm.NAMES[dst]] == "reference"
    got = checker(src, dst, 4096, 4096)
    assert [md5(p) for p in got] == c["md5"][cm.NAMES[dst]]
