"""CPU tests of the ORB boundary: the library exports compvhip_plan_orb_keypoints, compvhip_plan_orb_describe and compvhip_orb_u8, the Python binding
lists and binds them, the keypoint dtype is the C struct's (and CompVInterestPoint's), and the null-handle checks that precede any HIP call answer
without a GPU.  (Without a device no context can be made, so the parameter refusals that need one are exercised by tests/test_gpu_orb.py.)"""
import ctypes as C
import os
import re

import numpy as np

import orb_model as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"compvhip_plan_orb_keypoints": 12, "compvhip_plan_orb_describe": 10, "compvhip_orb_u8": 13}


def test_symbols_are_exported_and_bound():
    from compv_amd import capi
    lib = capi.load()
    for s, nargs in SYMBOLS.items():
        assert s in capi.EXPORTS and hasattr(lib, s), s
        assert len(getattr(lib, s).argtypes) == nargs, s
    assert hasattr(capi, "Keypoint") and hasattr(capi.Context, "orb") and hasattr(capi.Plan, "orb_keypoints") and hasattr(capi.Plan, "orb_describe")


def test_record_dtype_is_the_c_struct():
    from compv_amd import capi
    assert capi.KEYPOINT_DTYPE == om.KEYPOINT_DTYPE and capi.KEYPOINT_DTYPE.itemsize == 24 == C.sizeof(capi.Keypoint)          # sizeof(CompVInterestPoint)
    assert capi.KEYPOINT_DTYPE.names == ("x", "y", "strength", "orient", "level", "size") == tuple(f[0] for f in capi.Keypoint._fields_)
    assert [capi.KEYPOINT_DTYPE.fields[n][1] for n in capi.KEYPOINT_DTYPE.names] == [getattr(capi.Keypoint, n).offset for n in capi.KEYPOINT_DTYPE.names]
    txt = open(os.path.join(ROOT, "include", "compv_hip.h")).read()
    body = re.search(r"typedef struct compvhip_keypoint \{(.*?)\} compvhip_keypoint;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+)\s*[,;]", body) == ["x", "y", "strength", "orient", "level", "size"]
    assert re.findall(r"\b(float|int32_t)\b", body) == ["float", "float", "float", "int32_t", "float"]


def test_header_declares_the_issue_signatures():
    txt = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "compv_hip.h")).read())
    assert ("compvhip_plan_orb_keypoints(compvhip_plan* plan, const uint8_t* d_gray, const compvhip_corner* d_corners, size_t cornerCap, const int32_t* d_cornerCounts, "
            "int level, float scale, compvhip_keypoint* d_keypoints, size_t keyCap, int32_t* d_keyCounts, int32_t* d_moments, void* stream);") in txt
    assert ("compvhip_plan_orb_describe(compvhip_plan* plan, const uint8_t* d_gray, const compvhip_keypoint* d_keypoints, size_t keyCap, const int32_t* d_keyCounts, "
            "float scale, int blur, uint8_t* d_desc, size_t descStride, void* stream);") in txt


def test_null_handles_are_refused_before_any_hip_call():
    from compv_amd import capi
    lib = capi.load()
    gray = np.zeros((40, 40), np.uint8)
    corners = np.zeros(4, capi.CORNER_DTYPE)
    keys = np.zeros(4, capi.KEYPOINT_DTYPE)
    desc = np.full((4, 32), 0xA5, np.uint8)
    counts = np.array([4], np.int32)
    kept = C.c_size_t(77)
    p = lambda a: a.ctypes.data          # noqa: E731
    assert lib.compvhip_plan_orb_keypoints(None, p(gray), p(corners), 4, p(counts), 0, 1.0, p(keys), 4, p(counts), None, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_plan_orb_describe(None, p(gray), p(keys), 4, p(counts), 1.0, 1, p(desc), 32, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_orb_u8(None, p(gray), 40, 40, 40, p(corners), 4, 0, 1.0, p(keys), p(desc), 32, C.byref(kept)) == capi.E_INVALID_PARAMETER
    assert kept.value == 77 and (desc == 0xA5).all() and not keys["size"].any() and counts[0] == 4
