"""CPU tests of the FAST boundary: the library exports compvhip_plan_fast / compvhip_fast_u8, the Python binding lists and binds them, the record
dtype is the C struct's, and the argument checks that precede any HIP call answer without a GPU.  (Without a device no context or plan can be
made, so the refusals that need one -- W or H < 7, a fast type other than 9 or 12 -- are exercised by tests/test_gpu_fast.py.)"""
import ctypes as C
import os
import re

import numpy as np

import fast_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["compvhip_plan_fast", "compvhip_fast_u8"]


def test_symbols_are_exported_and_bound():
    from compv_amd import capi
    lib = capi.load()
    for s in SYMBOLS:
        assert s in capi.EXPORTS and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s
    assert len(lib.compvhip_plan_fast.argtypes) == 11 and len(lib.compvhip_fast_u8.argtypes) == 14


def test_record_dtype_is_the_c_struct():
    from compv_amd import capi
    assert capi.CORNER_DTYPE == fm.CORNER_DTYPE and capi.CORNER_DTYPE.itemsize == 12
    assert capi.CORNER_DTYPE.names == ("x", "y", "strength")
    txt = open(os.path.join(ROOT, "include", "compv_hip.h")).read()
    body = re.search(r"typedef struct compvhip_corner \{(.*?)\} compvhip_corner;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+)\s*[,;]", body) == ["x", "y", "strength"] and body.count("int32_t") == 2


def test_null_handles_are_refused_before_any_hip_call():
    from compv_amd import capi
    lib = capi.load()
    img = np.zeros((16, 16), np.uint8)
    rec = np.zeros(4, capi.CORNER_DTYPE)
    n = C.c_size_t(77)
    assert lib.compvhip_fast_u8(None, img.ctypes.data, 16, 16, 16, 20, 9, 1, -1, None, 0, rec.ctypes.data, 4, C.byref(n)) == capi.E_INVALID_PARAMETER
    assert n.value == 77 and not rec["x"].any()
    assert lib.compvhip_plan_fast(None, img.ctypes.data, 20, 9, 1, -1, None, rec.ctypes.data, 4, rec.ctypes.data, None) == capi.E_INVALID_PARAMETER
