"""CPU tests of the image statistics boundary: the library exports the nine calls, the Python binding lists and binds them with the header's argument
counts, compvhip_integral_dims (host arithmetic) equals the model's shapes and refuses what the definition refuses, and the refusals that precede any HIP
call answer without a GPU and leave the outputs untouched.  (Without a device no context can be made, so the refusals that need a handle are exercised by
tests/test_gpu_stats.py.)"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import stats_cases as sc
import stats_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"compvhip_integral_dims": 4, "compvhip_plan_integral": 6, "compvhip_integral_u8": 8, "compvhip_plan_histogram": 4, "compvhip_histogram_u8": 6,
           "compvhip_plan_equalize": 7, "compvhip_equalize_u8": 10, "compvhip_plan_projections": 5, "compvhip_projections_u8": 7}


def test_symbols_are_exported_and_bound():
    from compv_amd import capi
    lib = capi.load()
    txt = open(os.path.join(ROOT, "include", "compv_hip.h")).read()
    assert len(SYMBOLS) == 9
    for s, nargs in SYMBOLS.items():
        assert s in capi.EXPORTS and hasattr(lib, s), s
        assert len(getattr(lib, s).argtypes) == nargs, s
        decl = re.search(r"COMPVHIP_API \w+ %s\((.*?)\);" % s, txt, re.S).group(1)
        assert decl.count(",") + 1 == nargs, s          # the binding's argument count is the header's


def test_python_signatures():
    from compv_amd import capi
    sig = lambda f: list(inspect.signature(f).parameters)          # noqa: E731
    assert sig(capi.integral_dims) == ["W", "H"]
    assert sig(capi.Context.integral) == ["self", "img", "want_sum", "want_sumsq", "sum_stride"]
    assert sig(capi.Context.histogram) == ["self", "img"]
    assert sig(capi.Context.equalize) == ["self", "img", "hist", "scale", "out_stride"]
    assert sig(capi.Context.projections) == ["self", "img", "want_x", "want_y"]
    assert sig(capi.Plan.integral) == ["self", "d_gray", "d_sum", "d_sumsq", "sum_stride", "stream"]
    assert sig(capi.Plan.histogram) == ["self", "d_gray", "d_hist", "stream"]
    assert sig(capi.Plan.equalize) == ["self", "d_gray", "d_out", "d_hist", "scale", "d_lut", "stream"]
    assert sig(capi.Plan.projections) == ["self", "d_gray", "d_proj_x", "d_proj_y", "stream"]


def test_integral_dims_equal_the_models_shapes():
    from compv_amd import capi
    shapes = [(c["W"], c["H"]) for c in sc.CASES] + [(3840, 2160), (64, 128), (5000, 3400), (32767, 1), (1, 32767), (32767, 32767)]
    for W, H in shapes:
        assert capi.integral_dims(W, H) == sm.integral_dims(W, H) == (H + 1, W + 1), (W, H)
    lib = capi.load()
    rows, cols = C.c_size_t(777), C.c_size_t(777)          # either output is optional
    assert lib.compvhip_integral_dims(37, 29, C.byref(rows), None) == capi.OK and rows.value == 30
    assert lib.compvhip_integral_dims(37, 29, None, C.byref(cols)) == capi.OK and cols.value == 38
    assert lib.compvhip_integral_dims(37, 29, None, None) == capi.OK


@pytest.mark.parametrize("W,H", [(0, 5), (5, 0), (0, 0), (32768, 5), (5, 32768), (46341, 46341), (32768, 65536), (65536, 32768)])
def test_integral_dims_refuse(W, H):
    from compv_amd import capi
    lib = capi.load()
    rows, cols = C.c_size_t(777), C.c_size_t(777)
    assert lib.compvhip_integral_dims(W, H, C.byref(rows), C.byref(cols)) == capi.E_INVALID_PARAMETER
    assert rows.value == 777 and cols.value == 777          # nothing is written
    with pytest.raises(capi.CompvHipError):
        capi.integral_dims(W, H)
    with pytest.raises(ValueError):
        sm.integral_dims(W, H)


def test_refusals_before_any_hip_call():
    from compv_amd import capi
    lib = capi.load()
    img = np.full((8, 8), 9, np.uint8)
    f64 = np.full(81, 5.0)
    u32 = np.full(256, 5, np.uint32)
    i32 = np.full(8, 5, np.int32)
    out = np.full((8, 8), 5, np.uint8)
    g = (img.ctypes.data, 8, 8, 8)
    bad = capi.E_INVALID_PARAMETER
    assert lib.compvhip_integral_u8(None, *g, f64.ctypes.data, None, 9) == bad          # null contexts and plans
    assert lib.compvhip_histogram_u8(None, *g, u32.ctypes.data) == bad
    assert lib.compvhip_equalize_u8(None, *g, None, -1.0, out.ctypes.data, 8, None) == bad
    assert lib.compvhip_projections_u8(None, *g, i32.ctypes.data, None) == bad
    assert lib.compvhip_plan_integral(None, img.ctypes.data, f64.ctypes.data, None, 9, None) == bad
    assert lib.compvhip_plan_histogram(None, img.ctypes.data, u32.ctypes.data, None) == bad
    assert lib.compvhip_plan_equalize(None, img.ctypes.data, None, -1.0, out.ctypes.data, None, None) == bad
    assert lib.compvhip_plan_projections(None, img.ctypes.data, i32.ctypes.data, None, None) == bad
    assert (f64 == 5.0).all() and (u32 == 5).all() and (i32 == 5).all() and (out == 5).all() and (img == 9).all()
