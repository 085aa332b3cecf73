"""CPU tests of the image-moments boundary of the C ABI (include/compv_hip.h, "image moments"): the exports exist and are bound, follow the header's
rules (no stream parameter: the stream travels in the descriptor; no handle type; no plan_ name), compvhip_moments_fits holds on both sides of the 2^64
rule, and compvhip_moments_shape_host -- plain arithmetic through compv_amd/csrc/moments_math.hpp -- equals tests/moments_model.py on every field and
the fixture of the compiled reference: skew bit for bit, theta within the angle bound.  Every refusal that needs no device is asserted."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import moments_model as mm
from fixtures import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("compvhip_moments_frames", "compvhip_moments_components", "compvhip_moments_shapes", "compvhip_moments_shape_host", "compvhip_moments_fits",
         "compvhip_moments_host")


def header():
    return open(os.path.join(ROOT, "include", "compv_hip.h")).read()


@pytest.fixture(scope="module")
def golden():
    return load_golden("golden_moments")


def test_exports_are_declared_bound_and_present():
    from compv_amd import capi
    lib = capi.load()
    txt = header()
    for s in NAMES:
        assert re.search(r"COMPVHIP_API\s+\w+\s+%s\s*\(" % s, txt), s
        assert s in capi.EXPORTS and hasattr(lib, s), s
    assert C.sizeof(capi.MomentsDesc) == 24 and capi.MOMENTS_DTYPE.itemsize == 48 and capi.MOMENTS_SHAPE_DTYPE.itemsize == 72
    assert capi.MOMENTS_DTYPE.names == mm.NAMES and capi.MOMENTS_SHAPE_DTYPE.names[:8] == mm.SHAPE_NAMES
    assert (capi.MOMENTS_VALUE, capi.MOMENTS_UNIT, capi.MOMENTS_ORIGIN_FRAME, capi.MOMENTS_ORIGIN_BOX) == (mm.VALUE, mm.UNIT, mm.ORIGIN_FRAME, mm.ORIGIN_BOX)
    for word, value in (("VALUE", 0), ("UNIT", 1), ("ORIGIN_FRAME", 0), ("ORIGIN_BOX", 1)):
        assert re.search(r"COMPVHIP_MOMENTS_%s = %d\b" % (word, value), txt), word


def test_the_stream_travels_in_the_descriptor():
    txt = re.sub(r"/\*.*?\*/", " ", header(), flags=re.S)
    decls = re.findall(r"COMPVHIP_API\s+[\w\s\*]+?\b(compvhip_moments_\w+)\s*\(([^)]*)\)\s*;", txt)
    assert sorted(n for n, _ in decls) == sorted(NAMES)
    for name, params in decls:
        assert not re.search(r"void\s*\*\s*stream", params), name
    body = header()[header().index("typedef struct compvhip_moments_desc"):][:600]
    assert re.search(r"void\*\s+hipStream;", body)
    assert not re.search(r"typedef\s+struct\s+compvhip_moments\w*\s+compvhip_moments\w*\s*;", header())          # records, no opaque handle


def test_fits_on_both_sides_of_the_rule():
    from compv_amd import capi
    sizes = [(3840, 2160), (16384, 16384), (32767, 32767), (16406, 16384), (16407, 16384), (2056, 32767), (2057, 32767), (32767, 2056), (32767, 2057), (1, 1), (0, 1), (1, 0),
             (32768, 1), (1, 32768), (65535, 32767), (2 ** 32 + 5, 5), (5, 2 ** 32 + 5), (2 ** 63, 2), (46341, 46341)]
    for w, h in sizes:
        for weights in (mm.VALUE, mm.UNIT, 2, -1):
            assert capi.moments_fits(w, h, weights) == mm.fits(w, h, weights), (w, h, weights)
    assert capi.moments_fits(16384, 16384) and capi.moments_fits(3840, 2160) and not capi.moments_fits(32767, 32767) and capi.moments_fits(32767, 32767, capi.MOMENTS_UNIT)
    assert capi.moments_fits(16406, 16384) and not capi.moments_fits(16407, 16384)          # 0.99999 and 1.00017 times 2^64


def test_shape_host_equals_the_model_and_the_reference(golden):
    from compv_amd import capi
    meta, arrays = golden
    frames = {r["id"]: r for r in meta["frames"]}
    checked = angles = 0
    for key in (k for k in arrays.files if k.startswith("raw_")):
        raw = arrays[key].reshape(-1, 6)
        got = capi.moments_shape_host(raw)
        assert got.tobytes() == mm.shape_array([tuple(int(v) for v in r) for r in raw], capi.MOMENTS_SHAPE_DTYPE).tobytes(), key
        rec = frames.get(key[4:])
        if rec is not None and rec.get("model_only"):
            continue
        skews, thetas = ([float.fromhex(rec["skew"])], [float.fromhex(rec["theta"])]) if rec is not None else (arrays["skew_" + key[4:]], arrays["theta_" + key[4:]])
        for g, skew, theta in zip(got, skews, thetas):
            assert np.float64(g["skew"]).tobytes() == np.float64(skew).tobytes(), key
            if mm.angle_case({n: g[n] for n in got.dtype.names}):
                assert abs(np.arctan2(g["sn"], g["cs"]) - theta) <= 4 * meta["max_angle_distance"], key
                angles += 1
            checked += 1
    assert checked >= 150 and angles >= 100


def test_shape_host_beyond_2_53_and_refusals():
    from compv_amd import capi
    lib = capi.load()
    raw = [(2 ** 53 + 1, 2 ** 53 + 3, 2 ** 54 + 2, 2 ** 64 - 1, 2 ** 63 + 1025, 2 ** 64 - 1025), (0, 1, 2, 3, 4, 5), (7, 0, 0, 0, 0, 0)]
    assert capi.moments_shape_host(raw).tobytes() == mm.shape_array(raw, capi.MOMENTS_SHAPE_DTYPE).tobytes()
    r, s = np.zeros(1, capi.MOMENTS_DTYPE), np.full(1, 7, np.uint8).repeat(72).view(capi.MOMENTS_SHAPE_DTYPE)
    p = capi._ptr
    assert lib.compvhip_moments_shape_host(None, 1, p(s)) == capi.E_INVALID_PARAMETER and lib.compvhip_moments_shape_host(p(r), 1, None) == capi.E_INVALID_PARAMETER
    assert (s.view(np.uint8) == 7).all()
    assert lib.compvhip_moments_shape_host(None, 0, None) == capi.OK


def test_device_calls_refuse_a_null_context():
    from compv_amd import capi
    lib = capi.load()
    desc = capi.MomentsDesc()
    d = C.byref(desc)
    assert lib.compvhip_moments_frames(None, d, None, 4, 4, 4, 1, None, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_moments_components(None, d, None, 4, 4, 4, None, 4, None, 1, None, 1, None, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_moments_shapes(None, d, None, 1, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_moments_host(None, d, None, 4, 4, 4, None, None) == capi.E_INVALID_PARAMETER
