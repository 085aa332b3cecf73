"""CPU tests of the lens-undistortion boundary of the C ABI (include/compv_hip.h, "lens undistortion"): the exports exist, follow the two rules of the
header (a handle family of its own, no stream parameter), and the host entry points -- compvhip_undistort_coeffs_* and compvhip_undistort_map_*,
plain arithmetic through compv_amd/csrc/undistort_math.hpp -- equal tests/undistort_model.py and the fixture of the compiled reference bit for bit.
Every refusal that needs no device is asserted with the destination untouched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import undistort_cases as uc
import undistort_model as um

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("compvhip_undistort_coeffs_f32", "compvhip_undistort_coeffs_f64", "compvhip_undistort_map_f32", "compvhip_undistort_map_f64", "compvhip_undistort_create",
         "compvhip_undistort_destroy", "compvhip_undistort_frames", "compvhip_undistort_maps", "compvhip_undistort_points", "compvhip_undistort_project",
         "compvhip_undistort_u8", "compvhip_undistort_set_timing", "compvhip_undistort_get_timing")


def header():
    return open(os.path.join(ROOT, "include", "compv_hip.h")).read()


@pytest.fixture(scope="module")
def arrays():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_undistort.npz"))


def test_exports_are_declared_bound_and_present():
    from compv_amd import capi
    lib = capi.load()
    txt = header()
    for s in NAMES:
        assert re.search(r"COMPVHIP_API\s+\w+\s+%s\s*\(" % s, txt), s
        assert s in capi.EXPORTS and hasattr(lib, s), s
    assert C.sizeof(capi.UndistortDesc) == 56 and capi.UNDISTORT_COEFFS == len(um.NAMES) == 14


def test_the_family_takes_its_stream_at_creation():
    """no export of the family has a `void* stream` parameter (the stream is a field of the descriptor), and the section does not use the class words
    of the stream-order table, which belong to the exports that take one"""
    txt = re.sub(r"/\*.*?\*/", " ", header(), flags=re.S)
    decls = re.findall(r"COMPVHIP_API\s+[\w\s\*]+?\b(compvhip_undistort_\w+)\s*\(([^)]*)\)\s*;", txt)
    assert sorted(n for n, _ in decls) == sorted(NAMES)
    for name, params in decls:
        assert not re.search(r"void\s*\*\s*stream", params), name
    assert re.search(r"void\*\s+stream;", header()[header().index("typedef struct compvhip_undistort_desc"):][:2000])


@pytest.mark.parametrize("c", uc.image_cases(), ids=lambda c: c["id"])
def test_host_coefficients_and_maps(arrays, c):
    from compv_amd import capi
    wo, ho = c["size"][2:]
    x0, y0 = c["origin"]
    for T in (np.float32, np.float64):
        assert capi.undistort_coeffs(c["K"], c["d"], T).tobytes() == um.coeffs(c["K"], c["d"], T).tobytes()
        mx, my = capi.undistort_map(c["K"], c["d"], wo, ho, x0, y0, T)
        ex, ey = um.map_planes(c["K"], c["d"], wo, ho, x0, y0, T)
        assert mx.dtype == T and mx.tobytes() == ex.tobytes() and my.tobytes() == ey.tobytes()
        if T is np.float32:
            assert mx.tobytes() == arrays["mapx_" + c["id"]].tobytes() and my.tobytes() == arrays["mapy_" + c["id"]].tobytes()


def test_host_refusals_write_nothing():
    from compv_amd import capi
    lib = capi.load()
    c = uc.case("pin61")
    for T, coeffs, mapf in ((np.float32, lib.compvhip_undistort_coeffs_f32, lib.compvhip_undistort_map_f32), (np.float64, lib.compvhip_undistort_coeffs_f64, lib.compvhip_undistort_map_f64)):
        K, d = np.ascontiguousarray(c["K"], T), np.ascontiguousarray(c["d"], T)
        singular = K.copy()
        singular[1, 1] = 0
        rec = np.full(14, 7, T)
        mx, my = np.full(6, 7, T), np.full(6, 7, T)
        p = capi._ptr
        assert coeffs(p(K), p(d), 4, p(rec)) == capi.OK and rec[0] == K[0, 0]
        rec[:] = 7
        for args in ((None, p(d), 4, p(rec)), (p(K), None, 4, p(rec)), (p(K), p(d), 4, None), (p(K), p(d), 1, p(rec)), (p(K), p(d), 5, p(rec)), (p(singular), p(d), 4, p(rec))):
            assert coeffs(*args) == capi.E_INVALID_PARAMETER
        assert (rec == 7).all()
        bad = ((None, p(d), 4, 0, 0, 3, 2, p(mx), p(my)), (p(K), None, 4, 0, 0, 3, 2, p(mx), p(my)), (p(K), p(d), 4, 0, 0, 3, 2, None, p(my)), (p(K), p(d), 4, 0, 0, 3, 2, p(mx), None),
               (p(K), p(d), 1, 0, 0, 3, 2, p(mx), p(my)), (p(K), p(d), 5, 0, 0, 3, 2, p(mx), p(my)), (p(singular), p(d), 4, 0, 0, 3, 2, p(mx), p(my)),
               (p(K), p(d), 4, 0, 0, 0, 2, p(mx), p(my)), (p(K), p(d), 4, 0, 0, 3, 0, p(mx), p(my)), (p(K), p(d), 4, 0, 0, 32768, 1, p(mx), p(my)),
               (p(K), p(d), 4, 32765, 0, 3, 2, p(mx), p(my)), (p(K), p(d), 4, 0, 32766, 3, 2, p(mx), p(my)))
        for args in bad:
            assert mapf(*args) == capi.E_INVALID_PARAMETER, args[2:7]
        assert (mx == 7).all() and (my == 7).all()
        assert mapf(p(K), p(d), 4, 32764, 32765, 3, 2, p(mx), p(my)) == capi.OK and not (mx == 7).any()          # x0 + Wout == y0 + Hout == 32767: served
    with pytest.raises(capi.CompvHipError):
        capi.undistort_coeffs(singular, c["d"])


def test_handle_calls_refuse_null_handles_and_contexts():
    from compv_amd import capi
    lib = capi.load()
    h = C.c_void_p()
    desc = capi.UndistortDesc(64, 48, 64, 1, 64, 48)
    assert lib.compvhip_undistort_create(None, C.byref(desc), C.byref(h)) == capi.E_INVALID_PARAMETER and not h.value
    assert lib.compvhip_undistort_frames(None, None, None, None, 4, 1, 1, None, 0, None, 64) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_undistort_maps(None, None, None, 4, 1, 0, None, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_undistort_points(None, None, None, 4, 1, 0, None, 1, 1, None, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_undistort_project(None, None, None, 4, 1, None, None, 1, 1, None, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_undistort_u8(None, None, 1, 1, 1, None, None, 4, 0, 0, 1, None, 0, None, 1, 1, 1) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_undistort_set_timing(None, 1) == capi.E_INVALID_PARAMETER and lib.compvhip_undistort_get_timing(None, None, None, 0) == capi.E_INVALID_PARAMETER
    lib.compvhip_undistort_destroy(None)          # a no-op


def test_the_wider_type_is_another_number():
    """The pitfall the definition names: x = ((kinv11 * X) + (kinv21 * Y)) + kinv31 rounds after every operation.  With skew == 0 the middle term is a
    signed zero, so the float32 entry is fl(fl(kinv11 * X) + kinv31) -- and evaluating kinv11 * X + kinv31 in float64 and rounding once lands on the
    neighbouring float32 for some X.  One such entry is shown, and the host call gives the definition's value."""
    from compv_amd import capi
    c = uc.case("pin61")
    assert c["K"][0][1] == 0.0
    rec = um.coeffs(c["K"], c["d"], np.float32)
    k11, k31 = rec[um.NAMES.index("kinv11")], rec[um.NAMES.index("kinv31")]
    X = np.arange(61, dtype=np.float32)
    stepwise = (k11 * X) + k31
    once = (np.float64(k11) * X.astype(np.float64) + np.float64(k31)).astype(np.float32)
    differ = np.flatnonzero(stepwise != once)
    assert differ.size, "no column of this camera shows the pitfall"
    i = int(differ[0])
    assert abs(int(stepwise[i:i + 1].view(np.int32)[0]) - int(once[i:i + 1].view(np.int32)[0])) == 1          # neighbours
    # the normalised x of the host map is the stepwise one: re-derive the entry of (i, 0) from it and compare with the call
    y = (rec[um.NAMES.index("kinv22")] * np.float32(0)) + rec[um.NAMES.index("kinv32")]
    u, v = um.distort(rec, stepwise[i:i + 1], np.array([y], np.float32))
    mx, my = capi.undistort_map(c["K"], c["d"], 61, 1)
    assert mx[0, i] == u[0] and my[0, i] == v[0]
    u1, _ = um.distort(rec, once[i:i + 1], np.array([y], np.float32))
    assert u1.dtype == np.float32
