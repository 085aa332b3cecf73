"""CPU tests of the matcher boundary: the library exports the compvhip_matcher_* calls and compvhip_match_hamming_u8, the Python binding lists and
binds them, the record dtype is the C struct's (and CompVDMatch's), and the null-handle checks that precede any HIP call answer without a GPU.
(Without a device no context can be made, so the parameter refusals that need one are exercised by tests/test_gpu_match.py.)"""
import ctypes as C
import os
import re

import numpy as np

import match_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"compvhip_matcher_create": 7, "compvhip_matcher_destroy": 1, "compvhip_matcher_knn": 10, "compvhip_matcher_good": 14,
           "compvhip_match_hamming_u8": 12, "compvhip_matcher_set_timing": 2, "compvhip_matcher_get_timing": 4}


def test_symbols_are_exported_and_bound():
    from compv_amd import capi
    lib = capi.load()
    for s, nargs in SYMBOLS.items():
        assert s in capi.EXPORTS and hasattr(lib, s), s
        assert len(getattr(lib, s).argtypes) == nargs, s
    assert hasattr(capi, "Matcher") and hasattr(capi.Context, "match_hamming")


def test_record_dtype_is_the_c_struct():
    from compv_amd import capi
    assert capi.MATCH_DTYPE == mm.MATCH_DTYPE and capi.MATCH_DTYPE.itemsize == 16          # sizeof(compvhip_match) == sizeof(CompVDMatch)
    assert capi.MATCH_DTYPE.names == ("queryIdx", "trainIdx", "imageIdx", "distance")
    txt = open(os.path.join(ROOT, "include", "compv_hip.h")).read()
    body = re.search(r"typedef struct compvhip_match \{(.*?)\} compvhip_match;", txt, re.S).group(1)
    assert re.findall(r"\b(\w+)\s*[,;]", body) == ["queryIdx", "trainIdx", "imageIdx", "distance"] and body.count("int32_t") == 1
    assert C.sizeof(capi.MatchOpts) == 16 and capi.MatchOpts.ratio.offset == 0 and capi.MatchOpts.maxDistance.offset == 8


def test_null_handles_are_refused_before_any_hip_call():
    from compv_amd import capi
    lib = capi.load()
    desc = np.zeros((4, 32), np.uint8)
    rec = np.zeros(8, capi.MATCH_DTYPE)
    rows = C.c_size_t(77)
    h = C.c_void_p(1234)
    assert lib.compvhip_matcher_create(None, 32, 4, 4, 1, 2, C.byref(h)) == capi.E_INVALID_PARAMETER
    assert h.value == 1234
    assert lib.compvhip_match_hamming_u8(None, desc.ctypes.data, 4, 32, desc.ctypes.data, 4, 32, 32, 2, rec.ctypes.data, 4, C.byref(rows)) == capi.E_INVALID_PARAMETER
    assert rows.value == 77 and not rec["distance"].any()
    assert lib.compvhip_matcher_knn(None, desc.ctypes.data, 32, None, desc.ctypes.data, 32, None, 0, rec.ctypes.data, None) == capi.E_INVALID_PARAMETER
    o = capi.MatchOpts(0.8, -1, 0)
    assert lib.compvhip_matcher_good(None, rec.ctypes.data, desc.ctypes.data, 32, None, desc.ctypes.data, 32, None, 0, C.byref(o), rec.ctypes.data, 8,
                                     rec.ctypes.data, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_matcher_set_timing(None, 1) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_matcher_get_timing(None, None, None, 0) == capi.E_INVALID_PARAMETER
    lib.compvhip_matcher_destroy(None)          # a no-op
