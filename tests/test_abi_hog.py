"""CPU tests of the HOG boundary: the library exports the three calls, the Python binding lists and binds them with the header's argument counts, the option
struct is the C struct, compvhip_hog_geometry (host arithmetic) equals the model on every case and refuses everything item 8 of the definition refuses, and
the refusals that precede any HIP call answer without a GPU and leave the outputs untouched.  (Without a device no context can be made, so the refusals that
need a handle are exercised by tests/test_gpu_hog.py.)"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import hog_cases as hc
import hog_model as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"compvhip_hog_geometry": 8, "compvhip_plan_hog": 7, "compvhip_hog_u8": 9}


def opts_of(capi, o):
    """a model option dict -> capi.HogOpts, field by field"""
    return capi.HogOpts(**o)


def test_symbols_are_exported_and_bound():
    from compv_amd import capi
    lib = capi.load()
    txt = open(os.path.join(ROOT, "include", "compv_hip.h")).read()
    for s, nargs in SYMBOLS.items():
        assert s in capi.EXPORTS and hasattr(lib, s), s
        assert len(getattr(lib, s).argtypes) == nargs, s
        decl = re.search(r"COMPVHIP_API \w+ %s\((.*?)\);" % s, txt, re.S).group(1)
        assert decl.count(",") + 1 == nargs, s          # the binding's argument count is the header's


def test_python_signatures():
    from compv_amd import capi
    assert list(inspect.signature(capi.Context.hog).parameters) == ["self", "img", "opts", "kw"]
    assert list(inspect.signature(capi.Plan.hog).parameters) == ["self", "d_gray", "d_desc", "desc_stride", "d_cells", "opts", "stream", "kw"]
    assert list(inspect.signature(capi.hog_geometry).parameters) == ["W", "H", "opts", "kw"]


def test_option_struct_is_the_c_struct_and_the_constants_are_the_headers():
    from compv_amd import capi
    txt = open(os.path.join(ROOT, "include", "compv_hip.h")).read()
    body = re.search(r"typedef struct compvhip_hog_opts \{(.*?)\} compvhip_hog_opts;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+)\s*[,;]", body) == [f for f, _ in capi.HogOpts._fields_] == ["size"] + hm.FIELDS
    assert C.sizeof(capi.HogOpts) == 44 and all(t in (C.c_uint32, C.c_int32) for _, t in capi.HogOpts._fields_)
    o = capi.HogOpts()
    assert o.size == 44 and not any(getattr(o, f) for f in hm.FIELDS)          # zero-initialised with `size` set: the reference's defaults
    for name, value in re.findall(r"COMPVHIP_HOG_(\w+) = (\d+)", txt):
        if name.endswith("DEFAULT"):
            assert int(value) == 0
        else:
            assert getattr(capi, "HOG_" + name) == int(value), name
    assert (capi.HOG_NORM_NONE, capi.HOG_NORM_L1, capi.HOG_NORM_L1SQRT, capi.HOG_NORM_L2, capi.HOG_NORM_L2HYS) == tuple(hc.ALL_NORMS)
    assert (capi.HOG_GRADIENT_SIGNED, capi.HOG_GRADIENT_UNSIGNED) == (hm.GRADIENT_SIGNED, hm.GRADIENT_UNSIGNED)
    assert (capi.HOG_INTERP_NEAREST, capi.HOG_INTERP_BILINEAR, capi.HOG_INTERP_BILINEAR_LUT) == (hm.INTERP_NEAREST, hm.INTERP_BILINEAR, hm.INTERP_BILINEAR_LUT)
    o = capi.HogOpts(block=(8, 16), stride=(4, 8), cell=(4, 8), nbins=6, norm="l1sqrt", signed=False, interp="nearest")
    assert [getattr(o, f) for f in hm.FIELDS] == [8, 16, 4, 8, 4, 8, 6, 3, 2, 1]


def test_geometry_on_the_host_equals_the_model():
    from compv_amd import capi
    shapes = [(c["W"], c["H"], c["opts"]) for c in hc.CASES]
    shapes += [(3840, 2160, {}), (64, 128, {}), (35, 27, hc.layout(8, 4, 8)), (32767, 16, {}), (16, 32767, {}), (2, 2, hc.layout(2, 1, 2, 4)), (5500, 8, hc.layout((2740, 4), (2740, 4), (2740, 4))),
               (200, 100, hc.layout(96, 96, 96))]
    for W, H, o in shapes:
        g = hm.geometry(W, H, o)
        got = capi.hog_geometry(W, H, opts_of(capi, o))
        assert got == {k: g[k] for k in ("cellsX", "cellsY", "blocksX", "blocksY", "descLen")}, (W, H, o)
    assert capi.hog_geometry(64, 128) == capi.hog_geometry(64, 128, capi.HogOpts(block=16, stride=8, cell=8, nbins=9, norm="l2hys", signed=True, interp="bilinear"))
    assert capi.hog_geometry(64, 128)["descLen"] == 3780
    lib = capi.load()
    n = C.c_size_t(0)
    o = capi.HogOpts()          # every output pointer is optional
    assert lib.compvhip_hog_geometry(64, 128, C.byref(o), None, None, None, None, C.byref(n)) == capi.OK and n.value == 3780
    assert lib.compvhip_hog_geometry(64, 128, C.byref(o), None, None, None, None, None) == capi.OK


REFUSED = [
    (64, 64, hc.layout(16, 8, 6)),                                   # block % cell != 0
    (64, 64, hc.layout(16, 4, 8)),                                   # stride = cell / 2 needs block == cell
    (64, 64, hc.layout(16, 16, 8)),                                  # stride > cell
    (64, 64, hc.layout(16, 3, 8)),                                   # any other stride
    (64, 64, hc.layout((16, 16), (8, 4), (8, 8))),                   # ... in y alone
    (64, 64, hc.layout((8, 16), (4, 4), (8, 8))),                    # ... stride = cell / 2 in both, block == cell in x only
    (64, 64, hc.layout(16, 8, 8, 1)), (64, 64, hc.layout(16, 8, 8, 361)),
    (64, 64, hc.layout(16, 8, 8, 7)), (64, 64, hc.layout(16, 8, 8, 8, signed=False)), (64, 64, hc.layout(16, 8, 8, 360, signed=False)),
    (15, 64, hc.layout(16, 8, 8)), (64, 15, hc.layout(16, 8, 8)), (0, 0, hc.layout(16, 8, 8)),
    (32768, 64, hc.layout(16, 8, 8)), (64, 32768, hc.layout(16, 8, 8)),
    (64, 64, hc.layout(16, 8, 8, interp=hm.INTERP_BILINEAR_LUT)), (64, 64, hc.layout(16, 8, 8, interp=4)),
    (64, 64, hc.layout(16, 8, 8, norm=6)), (64, 64, dict(gradientSigned=3)), (64, 64, dict(cellW=-8)), (64, 64, dict(nbins=-9)),
    (30000, 8, hc.layout((30000, 8), (30000, 8), (30000, 8), 360)),  # the resource limit: three rows of one cell and 360 bins exceed the LDS
]


@pytest.mark.parametrize("W,H,o", REFUSED)
def test_every_refusal_of_the_definition(W, H, o):
    from compv_amd import capi
    lib = capi.load()
    out = [C.c_size_t(777) for _ in range(5)]
    op = capi.HogOpts(**{k: v for k, v in o.items() if v >= 0})
    for k, v in o.items():
        if v < 0:
            setattr(op, k, v)
    assert lib.compvhip_hog_geometry(W, H, C.byref(op), *[C.byref(x) for x in out]) == capi.E_INVALID_PARAMETER
    assert all(x.value == 777 for x in out)          # nothing is written
    if W <= 32767 and H <= 32767 and min(o.values()) >= 0 and o.get("cellW", 8) < 30000:
        assert hm.geometry(W, H, o) is None          # the model refuses the same


def test_refusals_before_any_hip_call():
    from compv_amd import capi
    lib = capi.load()
    out = C.c_size_t(777)
    assert lib.compvhip_hog_geometry(64, 64, None, None, None, None, None, C.byref(out)) == capi.E_INVALID_PARAMETER and out.value == 777          # null options
    o = capi.HogOpts()
    o.size = 40          # another struct
    assert lib.compvhip_hog_geometry(64, 64, C.byref(o), None, None, None, None, C.byref(out)) == capi.E_INVALID_PARAMETER and out.value == 777
    o = capi.HogOpts()
    img = np.full((64, 64), 9, np.uint8)
    desc = np.full(16, 5.0, np.float32)
    n = C.c_size_t(777)
    assert lib.compvhip_hog_u8(None, img.ctypes.data, 64, 64, 64, C.byref(o), desc.ctypes.data, 16, C.byref(n)) == capi.E_INVALID_PARAMETER          # null context
    assert lib.compvhip_plan_hog(None, img.ctypes.data, C.byref(o), None, desc.ctypes.data, 16, None) == capi.E_INVALID_PARAMETER                    # null plan
    assert n.value == 777 and (desc == 5.0).all() and (img == 9).all()
    with pytest.raises(capi.CompvHipError):
        capi.hog_geometry(15, 64)
    with pytest.raises(TypeError):
        capi.hog_geometry(64, 64, capi.HogOpts(), nbins=9)
    with pytest.raises(TypeError):
        capi.HogOpts(bins=9)
