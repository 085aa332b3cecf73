"""CPU tests of the scale / ORB pyramid boundary: the library exports the new entries, the Python binding lists and binds them with the right argument
counts, the header declares the signatures, the options struct is the ctypes one, and the null-handle checks that precede any HIP call answer without a
GPU with the outputs untouched.  compvhip_orbpyr_geometry needs an object, which needs a context, so its arithmetic is pinned here through the model
(tests/orb_pyramid_model.py) and held against the device object by tests/test_gpu_orb_pyramid.py."""
import ctypes as C
import os
import re

import numpy as np

import orb_pyramid_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"compvhip_orbpyr_create": 8, "compvhip_orbpyr_destroy": 1, "compvhip_orbpyr_geometry": 7, "compvhip_orbpyr_plane": 4, "compvhip_orbpyr_detect": 8,
           "compvhip_orbpyr_describe": 9, "compvhip_plan_scale": 7, "compvhip_scale_u8": 9, "compvhip_orb_pyramid_u8": 11, "compvhip_orbpyr_set_timing": 2,
           "compvhip_orbpyr_get_timing": 4}


def test_symbols_are_exported_and_bound():
    from compv_amd import capi
    lib = capi.load()
    for s, nargs in SYMBOLS.items():
        assert s in capi.EXPORTS and hasattr(lib, s), s
        assert len(getattr(lib, s).argtypes) == nargs, s
    assert hasattr(capi, "OrbPyramid") and hasattr(capi.Context, "scale") and hasattr(capi.Context, "orb_pyramid") and hasattr(capi.Plan, "scale")
    for m in ("geometry", "plane", "detect", "describe", "set_timing", "get_timing", "close"):
        assert hasattr(capi.OrbPyramid, m), m


def test_header_declares_the_issue_signatures():
    txt = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "compv_hip.h")).read())
    for sig in (
            "int compvhip_orbpyr_create(compvhip_ctx* ctx, size_t W, size_t H, size_t S, size_t frames, const compvhip_orbpyr_opts* opts, size_t cornerCap, compvhip_orbpyr** pyramid);",
            "void compvhip_orbpyr_destroy(compvhip_orbpyr* pyramid);",
            "int compvhip_orbpyr_geometry(const compvhip_orbpyr* pyramid, int level, size_t* W, size_t* H, size_t* S, float* scale, int* quota);",
            "int compvhip_orbpyr_plane(compvhip_orbpyr* pyramid, int level, int blurred, const uint8_t** d_plane);",
            "int compvhip_orbpyr_detect(compvhip_orbpyr* pyramid, const uint8_t* d_gray, compvhip_keypoint* d_keypoints, size_t keyCap, int32_t* d_keyCounts, "
            "int32_t* d_levelCounts, int32_t* d_levelCorners, void* stream);",
            "int compvhip_orbpyr_describe(compvhip_orbpyr* pyramid, const uint8_t* d_gray, int reusePlanes, const compvhip_keypoint* d_keypoints, size_t keyCap, "
            "const int32_t* d_keyCounts, uint8_t* d_desc, size_t descStride, void* stream);",
            "int compvhip_plan_scale(compvhip_plan* src, const uint8_t* d_in, uint8_t* d_out, size_t Wout, size_t Hout, size_t Sout, void* stream);",
            "int compvhip_scale_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, uint8_t* out, size_t Wout, size_t Hout, size_t Sout);",
            "int compvhip_orb_pyramid_u8(compvhip_ctx* ctx, const uint8_t* gray, size_t W, size_t H, size_t S, const compvhip_orbpyr_opts* opts, "
            "compvhip_keypoint* keypoints, uint8_t* desc, size_t descStride, size_t cap, size_t* n);",
            "int compvhip_orbpyr_set_timing(compvhip_orbpyr* pyramid, int enabled);",
            "int compvhip_orbpyr_get_timing(compvhip_orbpyr* pyramid, const char** names, float* ms, int cap);"):
        assert sig in txt, sig


def test_options_struct_is_the_c_struct():
    from compv_amd import capi
    txt = open(os.path.join(ROOT, "include", "compv_hip.h")).read()
    body = re.search(r"typedef struct compvhip_orbpyr_opts \{(.*?)\} compvhip_orbpyr_opts;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+)\s*[,;]", body) == ["levels", "scaleFactor", "threshold", "fastType", "nonmax", "maxFeatures"] == [f[0] for f in capi.OrbPyramidOpts._fields_]
    assert [f[1] for f in capi.OrbPyramidOpts._fields_] == [C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int]
    assert C.sizeof(capi.OrbPyramidOpts) == 24 and [getattr(capi.OrbPyramidOpts, f[0]).offset for f in capi.OrbPyramidOpts._fields_] == [0, 4, 8, 12, 16, 20]
    o = capi.OrbPyramidOpts()          # CompVCornerDeteORB's defaults (compv_core_feature_orb_dete.cxx:35-40)
    assert (o.levels, o.threshold, o.fastType, o.nonmax, o.maxFeatures) == (8, 20, 9, 1, 2000) and np.float32(o.scaleFactor) == np.float32(0.83)


def test_null_handles_are_refused_before_any_hip_call():
    from compv_amd import capi
    lib = capi.load()
    gray = np.zeros((40, 40), np.uint8)
    small = np.full((20, 24), 0xA5, np.uint8)
    keys = np.zeros(4, capi.KEYPOINT_DTYPE)
    desc = np.full((4, 32), 0xA5, np.uint8)
    counts = np.array([4], np.int32)
    levels = np.full(8, 77, np.int32)
    n = C.c_size_t(77)
    W, H, S, sf, q = C.c_size_t(71), C.c_size_t(72), C.c_size_t(73), C.c_float(7.5), C.c_int(74)
    plane, handle = C.c_void_p(75), C.c_void_p(76)
    opts = capi.OrbPyramidOpts()
    p = lambda a: a.ctypes.data          # noqa: E731
    assert lib.compvhip_orbpyr_create(None, 40, 40, 40, 1, C.byref(opts), 16, C.byref(handle)) == capi.E_INVALID_PARAMETER and handle.value == 76
    lib.compvhip_orbpyr_destroy(None)
    assert lib.compvhip_orbpyr_geometry(None, 0, C.byref(W), C.byref(H), C.byref(S), C.byref(sf), C.byref(q)) == capi.E_INVALID_PARAMETER
    assert (W.value, H.value, S.value, sf.value, q.value) == (71, 72, 73, 7.5, 74)
    assert lib.compvhip_orbpyr_plane(None, 0, 0, C.byref(plane)) == capi.E_INVALID_PARAMETER and plane.value == 75
    assert lib.compvhip_orbpyr_detect(None, p(gray), p(keys), 4, p(counts), p(levels), p(levels), None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_orbpyr_describe(None, p(gray), 0, p(keys), 4, p(counts), p(desc), 32, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_plan_scale(None, p(gray), p(small), 24, 20, 24, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_scale_u8(None, p(gray), 40, 40, 40, p(small), 24, 20, 24) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_orb_pyramid_u8(None, p(gray), 40, 40, 40, C.byref(opts), p(keys), p(desc), 32, 4, C.byref(n)) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_orbpyr_set_timing(None, 1) == capi.E_INVALID_PARAMETER and lib.compvhip_orbpyr_get_timing(None, None, None, 0) == capi.E_INVALID_PARAMETER
    assert n.value == 77 and (desc == 0xA5).all() and (small == 0xA5).all() and not keys["size"].any() and counts[0] == 4 and (levels == 77).all()


# ---- the arithmetic compvhip_orbpyr_geometry returns, through the model (float32, operation by operation) -----------------------------------
def sizes(W, H, levels=8, sf=0.83):
    return [(g["W"], g["H"]) for g in pm.geometry(W, H, levels, sf)], [g["empty"] for g in pm.geometry(W, H, levels, sf)]


def test_level_sizes_and_empty_levels():
    assert sizes(200, 258) == ([(200, 258), (166, 214), (137, 177), (114, 147), (94, 122), (78, 101), (65, 84), (54, 70)], [False] * 8)
    assert sizes(100, 90) == ([(100, 90), (83, 74), (68, 62), (57, 51), (47, 42), (39, 35), (32, 29), (27, 24)], [False] * 5 + [True] * 3)
    assert sizes(64, 41)[1] == [False] + [True] * 7
    assert sizes(96, 80, 3, 0.5) == ([(96, 80), (48, 40), (24, 20)], [False, False, True])
    for g in pm.geometry(100, 90):
        assert g["S"] == (0 if g["empty"] else (g["W"] + 7) // 8 * 8)


def test_scale_factor_sum_and_quotas():
    sf, sfs = pm.scale_factors(8, 0.83)
    assert sfs == np.float32(4.5574746) and sf[0] == 1 and sf[1] == np.float32(0.83) and sf[2] == np.float32(0.83) * np.float32(0.83)
    assert [g["quota"] for g in pm.geometry(200, 258, max_features=500)] == [110, 91, 76, 63, 52, 43, 36, 30]
    assert [g["quota"] for g in pm.geometry(200, 258, max_features=60)] == [13, 11, 10, 10, 10, 10, 10, 10]
    assert [g["quota"] for g in pm.geometry(200, 258, max_features=2000)] == [439, 364, 302, 251, 208, 173, 143, 119]
    assert [g["quota"] for g in pm.geometry(200, 258, max_features=0)] == [0] * 8


def test_a_strict_downscale_reads_inside_the_plane():
    """rule A.5: the last nx + 1 the reference reaches, with the float32 steps"""
    for w_in, w_out, last in ((200, 166, 199), (9, 7, 8), (1100, 1021, 1096), (300, 2, 151), (3840, 3187, 3834)):
        sx, _ = pm.scale_steps(w_in, 10, w_out, 9)
        assert (((w_out - 1) * sx) >> 8) + 1 == last <= w_in - 1
    sx, _ = pm.scale_steps(16, 16, 40, 23)
    assert ((39 * sx) >> 8) + 1 == 16          # an upscale reaches the stride padding in the reference: the clamp is this library's rule
    assert pm.scale_steps(300, 8, 1, 8) is None and pm.scale_steps(8, 8, 0, 8) is None and pm.scale_steps(255, 8, 1, 8) is not None
