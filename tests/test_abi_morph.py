"""CPU tests of the thresholding / morphology boundary: the library exports the new symbols, the Python binding lists them, and the
structuring-element builder (host arithmetic, no GPU) equals the model and refuses what include/compv_hip.h says it refuses."""
import numpy as np
import pytest

import morph_model as mm

SYMBOLS = ["compvhip_threshold_u8", "compvhip_plan_threshold", "compvhip_threshold_adaptive_u8", "compvhip_plan_threshold_adaptive",
           "compvhip_morph_strel", "compvhip_morph_u8", "compvhip_plan_morph", "compvhip_plan_morph_ex"]


def test_symbols_are_exported_and_bound():
    from compv_amd import capi
    lib = capi.load()
    for s in SYMBOLS:
        assert s in capi.EXPORTS and hasattr(lib, s), s


def test_enum_values_are_the_reference_values():
    from compv_amd import capi
    assert (capi.MORPH_ERODE, capi.MORPH_DILATE, capi.MORPH_OPEN, capi.MORPH_CLOSE) == (mm.ERODE, mm.DILATE, mm.OPEN, mm.CLOSE)
    assert (capi.STREL_RECT, capi.STREL_DIAMOND, capi.STREL_CROSS) == (mm.RECT, mm.DIAMOND, mm.CROSS)
    assert (capi.BORDER_ZERO, capi.BORDER_REPLICATE) == (mm.BORDER_ZERO, mm.BORDER_REPLICATE)


@pytest.mark.parametrize("kind", [mm.RECT, mm.CROSS, mm.DIAMOND])
@pytest.mark.parametrize("w,h", [(1, 1), (3, 3), (7, 7), (31, 5), (5, 31), (31, 31), (2, 4)])
def test_strel_builder_equals_model(kind, w, h):
    from compv_amd import capi
    if kind == mm.DIAMOND and w != h:
        with pytest.raises(capi.CompvHipError) as e:
            capi.morph_strel(kind, w, h)
        assert e.value.code == capi.E_INVALID_PARAMETER
        return
    assert capi.morph_strel(kind, w, h).tobytes() == mm.strel(kind, w, h).tobytes()


def test_strel_builder_refusals():
    from compv_amd import capi
    lib = capi.load()
    buf = np.zeros(16, np.uint8)
    assert lib.compvhip_morph_strel(mm.RECT, 0, 3, buf.ctypes.data) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_morph_strel(mm.RECT, 3, 0, buf.ctypes.data) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_morph_strel(mm.RECT, 3, 3, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_morph_strel(3, 3, 3, buf.ctypes.data) == capi.E_NOT_IMPLEMENTED
    assert lib.compvhip_morph_strel(mm.DIAMOND, 3, 5, buf.ctypes.data) == capi.E_INVALID_PARAMETER
    assert (buf == 0).all()
