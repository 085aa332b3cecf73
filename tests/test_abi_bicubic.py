"""CPU tests of the bicubic boundary: the header holds the two new values of `interp` and paragraph F of the remap section, the Python binding the same
constants; no export was added for them; the null checks that precede any HIP call answer with the new values without a GPU."""
import os
import re

import bicubic_cases as bc
import bicubic_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "compv_hip.h")).read()


def test_header_holds_the_defines_and_paragraph_f():
    txt = header()
    flat = re.sub(r"\s+", " ", txt)
    assert re.search(r"^#define COMPVHIP_INTERP_BICUBIC 4\b", txt, re.M) and re.search(r"^#define COMPVHIP_INTERP_BICUBIC_FLOAT32 5\b", txt, re.M)
    assert not re.search(r"^#define COMPVHIP_INTERP_\w+ 3\b", txt, re.M), "3 stays unassigned"
    assert "* F. Bicubic interpolation: COMPVHIP_INTERP_BICUBIC and _BICUBIC_FLOAT32" in flat
    section = flat[flat.index("---- remap and inverse warp"):flat.index("---- RANSAC homography")]
    assert section.index("* E. Where this library differs") < section.index("* F. Bicubic interpolation") < section.index("#define COMPVHIP_INTERP_NEAREST")
    assert "the bicubic interpolation and the forward" not in section, "E.4 no longer lists bicubic as missing"
    for piece in ("a = ((D - A) * 0.5f) + ((B - C) * 1.5f)", "b = ((A + (B * -2.5f)) + (C * 2.0f)) + (D * -0.5f)", "c = (C - A) * 0.5f",
                  "a = ((A * -0.5f) + (B * 1.5f)) + ((C * -1.5f) + (D * 0.5f))", "b = (A + (B * -2.5f)) + ((C * 2.0f) + (D * -0.5f))", "c = (A * -0.5f) + (C * 0.5f)",
                  "xf = x - floorf(x)", "a NaN is outside"):
        assert piece in section, piece


def test_binding_has_the_constants_and_no_new_export():
    from compv_amd import capi
    assert (capi.INTERP_BICUBIC, capi.INTERP_BICUBIC_FLOAT32) == (bm.BICUBIC, bm.BICUBIC_FLOAT32) == bc.INTERPS == (4, 5)
    assert not [s for s in capi.EXPORTS if "bicubic" in s.lower()]
    assert "BICUBIC" in capi.Context.remap.__doc__ and "BICUBIC" in capi.Context.warp_inverse.__doc__


def test_null_handles_are_refused_with_the_new_values_before_any_hip_call():
    from compv_amd import capi
    lib = capi.load()
    for interp in bc.INTERPS:
        assert lib.compvhip_plan_remap(None, None, None, None, 1, interp, None, 0, None, 4, 4, 4, None) == capi.E_INVALID_PARAMETER
        assert lib.compvhip_plan_warp_inverse(None, None, None, 2, 1, interp, 0, None, 4, 4, 4, None) == capi.E_INVALID_PARAMETER
        assert lib.compvhip_remap_u8(None, None, 4, 4, 4, None, None, interp, None, 0, None, 4, 4, 4) == capi.E_INVALID_PARAMETER
        assert lib.compvhip_warp_inverse_u8(None, None, 4, 4, 4, None, 2, interp, 0, None, 4, 4, 4) == capi.E_INVALID_PARAMETER
