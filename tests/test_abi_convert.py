"""CPU tests of the colour conversion boundary: the header section and the binding agree, compvhip_convert_layout (host arithmetic) equals the model's
layout() and refuses what the definition refuses, and the refusals that precede any HIP call answer without a GPU.  (Without a device no context can be
made, so the refusals that need one are exercised by tests/test_gpu_convert.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import convert_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"compvhip_convert_layout": 6, "compvhip_convert_frames": 7, "compvhip_convert_u8": 5}
SIZES = (1, 2, 7, 640)


def test_header_section_and_binding_agree():
    from compv_amd import capi
    lib = capi.load()
    txt = open(os.path.join(ROOT, "include", "compv_hip.h")).read()
    section = txt[txt.index("/* ---- colour conversion"):]
    for s, nargs in SYMBOLS.items():
        assert s in capi.EXPORTS and hasattr(lib, s), s
        assert len(getattr(lib, s).argtypes) == nargs, s
        decl = re.search(r"COMPVHIP_API int %s\((.*?)\);" % s, section, re.S).group(1)
        assert decl.count(",") + 1 == nargs, s          # the binding's argument count is the header's
    # the struct: field for field
    body = re.search(r"typedef struct compvhip_image \{(.*?)\} compvhip_image;", section, re.S).group(1)
    fields = re.findall(r"(int|void\*|size_t) (\w+)(\[3\])?;", body)
    assert [(f[1], bool(f[2])) for f in fields] == [("pixfmt", False), ("plane", True), ("rowBytes", True), ("frameBytes", True)]
    assert [n for n, _ in capi.Image._fields_] == [f[1] for f in fields]
    assert C.sizeof(capi.Image) == 8 + 3 * 8 * 3
    # the format ids: the header's enum, the binding's constants and the model's
    for name in ("NV12", "NV21", "YUV420P", "YUV422P", "YUV444P", "HSV"):
        v = int(re.search(r"COMPVHIP_FMT_%s = (\d+)" % name, txt).group(1))
        assert v == getattr(capi, "FMT_" + name) == getattr(cm, name)
    for name in ("RGBA32", "ARGB32", "BGRA32", "RGB24", "BGR24", "RGB565LE", "RGB565BE", "BGR565LE", "BGR565BE", "YUYV422", "UYVY422", "Y"):
        assert getattr(capi, "FMT_" + name) == getattr(cm, name)          # 0..11 as they were


@pytest.mark.parametrize("fmt", cm.FORMATS, ids=cm.NAMES)
def test_layout_equals_the_model(fmt):
    from compv_amd import capi
    for W in SIZES:
        for H in SIZES:
            assert capi.convert_layout(fmt, W, H) == cm.layout(fmt, W, H), (W, H)
    lib = capi.load()
    n = C.c_int(77)          # every output is optional
    assert lib.compvhip_convert_layout(fmt, 7, 5, C.byref(n), None, None) == capi.OK and n.value == cm.layout(fmt, 7, 5)[0]
    assert lib.compvhip_convert_layout(fmt, 7, 5, None, None, None) == capi.OK


@pytest.mark.parametrize("fmt,W,H", [(18, 4, 4), (-1, 4, 4), (99, 4, 4), (0, 0, 4), (0, 4, 0), (12, 0, 0), (17, 0, 1)])
def test_layout_refuses(fmt, W, H):
    from compv_amd import capi
    lib = capi.load()
    n, rb, rows = C.c_int(77), (C.c_size_t * 3)(7, 7, 7), (C.c_size_t * 3)(7, 7, 7)
    assert lib.compvhip_convert_layout(fmt, W, H, C.byref(n), rb, rows) == capi.E_INVALID_PARAMETER
    assert n.value == 77 and list(rb) == [7, 7, 7] and list(rows) == [7, 7, 7]          # nothing is written
    with pytest.raises(capi.CompvHipError):
        capi.convert_layout(fmt, W, H)
    with pytest.raises(ValueError):
        cm.layout(fmt, W, H)


def test_null_context_is_refused_before_any_hip_call():
    from compv_amd import capi
    lib = capi.load()
    src, dst = np.full((2, 2), 9, np.uint8), np.full((2, 8), 5, np.uint8)
    a = capi.Image(capi.FMT_Y, [src.ctypes.data], [2], [4])
    b = capi.Image(capi.FMT_RGBA32, [dst.ctypes.data], [8], [16])
    assert lib.compvhip_convert_frames(None, 2, 2, 1, C.byref(a), C.byref(b), None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_convert_u8(None, 2, 2, C.byref(a), C.byref(b)) == capi.E_INVALID_PARAMETER
    assert (src == 9).all() and (dst == 5).all()
