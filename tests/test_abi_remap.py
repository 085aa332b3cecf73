"""CPU tests of the remap / inverse-warp boundary: the library exports the entries and the Python binding lists and binds them; the header declares the
signatures; compvhip_warp_tables -- host arithmetic, no context -- equals the model's running sums bit for bit for every golden matrix and for
Wout = 1, 2 and 4097; the model (tests/remap_model.py) equals every plane the compiled reference wrote (tests/golden/golden_remap.npz); the model's fused
multiply-add is exact where float64 emulation would round twice; the null checks that precede any HIP call answer without a GPU."""
import ctypes as C
import hashlib
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import remap_cases as rc
import remap_model as rm
from fixtures import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"compvhip_warp_tables": 10, "compvhip_plan_remap": 13, "compvhip_plan_warp_inverse": 12, "compvhip_remap_u8": 14, "compvhip_warp_inverse_u8": 13}


@pytest.fixture(scope="module")
def golden():
    return load_golden("golden_remap")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_symbols_are_exported_and_bound():
    from compv_amd import capi
    lib = capi.load()
    for s, nargs in SYMBOLS.items():
        assert s in capi.EXPORTS and hasattr(lib, s), s
        assert len(getattr(lib, s).argtypes) == nargs, s
    assert hasattr(capi, "warp_tables") and hasattr(capi, "Roi")
    for cls in (capi.Plan, capi.Context):
        assert hasattr(cls, "remap") and hasattr(cls, "warp_inverse"), cls
    assert (capi.INTERP_NEAREST, capi.INTERP_BILINEAR, capi.INTERP_BILINEAR_FLOAT32) == (rm.NEAREST, rm.BILINEAR, rm.BILINEAR_FLOAT32) == (0, 1, 2)
    assert [f[0] for f in capi.Roi._fields_] == ["left", "right", "top", "bottom"] and C.sizeof(capi.Roi) == 16


def test_header_declares_the_signatures():
    txt = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "compv_hip.h")).read())
    for sig in (
            "int compvhip_warp_tables(const float* M, int rows, size_t Wout, size_t Hout, float* ac, float* df, float* gi, float* by, float* ey, float* hy);",
            "int compvhip_plan_remap(compvhip_plan* plan, const uint8_t* d_in, const float* d_mapX, const float* d_mapY, size_t mapCount, int interp, "
            "const compvhip_roi* roi, uint8_t defaultValue, void* d_out, size_t Wout, size_t Hout, size_t Sout, void* stream);",
            "int compvhip_plan_warp_inverse(compvhip_plan* plan, const uint8_t* d_in, const float* M, int rows, size_t matrixCount, int interp, "
            "uint8_t defaultValue, void* d_out, size_t Wout, size_t Hout, size_t Sout, void* stream);",
            "int compvhip_remap_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, const float* mapX, const float* mapY, int interp, "
            "const compvhip_roi* roi, uint8_t defaultValue, void* out, size_t Wout, size_t Hout, size_t Sout);",
            "int compvhip_warp_inverse_u8(compvhip_ctx* ctx, const uint8_t* in, size_t W, size_t H, size_t S, const float* M, int rows, int interp, "
            "uint8_t defaultValue, void* out, size_t Wout, size_t Hout, size_t Sout);",
            "typedef struct compvhip_roi { float left, right, top, bottom; } compvhip_roi;"):
        assert sig in txt, sig
    for name, value in (("NEAREST", 0), ("BILINEAR", 1), ("BILINEAR_FLOAT32", 2)):
        assert "#define COMPVHIP_INTERP_%s %d" % (name, value) in txt


def test_the_fixtures_hold_what_the_cases_say(golden):
    G, A = golden
    assert [r["id"] for r in G["remap"]] == [c["id"] for c in rc.remap_cases()] and [r["id"] for r in G["warp"]] == [c["id"] for c in rc.warp_cases()]
    for r, c in zip(G["warp"], rc.warp_cases()):
        assert r["M_bits"] == [int(v) for v in bits(c["M"]).ravel()] and tuple(r["size"]) == c["size"] and r["seed"] == c["seed"]
    for r in G["remap"] + G["warp"]:
        for name, md5 in r["md5"].items():
            assert hashlib.md5(np.ascontiguousarray(A["%s_%s" % (r["id"], name)]).tobytes()).hexdigest() == md5
    assert {s[2] % 4 for s in rc.SIZES} == {0, 1, 2, 3} and max(s[2] for s in rc.SIZES) > 256
    assert any(r["inside_share"] < 0.1 for r in G["warp"]) and any(r["outside_share"] > 0.3 for r in G["remap"])
    for c in rc.remap_cases():          # every map holds coordinates just below an integer, whose neighbour is x1 + 2
        w, h, wo, ho = c["size"]
        x, y = rc.random_map(w, h, wo, ho, c["map_seed"])
        assert rc.skips_a_neighbour(x[1], w).sum() >= 3 and rc.skips_a_neighbour(y[1], h).sum() >= 3, c["id"]


def test_warp_tables_equal_the_model_bit_for_bit():
    from compv_amd import capi
    todo = [(c["M"], c["size"][2], c["size"][3]) for c in rc.warp_cases()]
    hom = rc.matrices(*rc.SIZES[1])["homography"]
    # 0.1f is inexact: 4096 running additions drift from 0.1f * i, which the definition forbids to substitute
    drift = np.array([[0.1, 0.3, -7.7], [1e-3, 0.7, 2.2], [1e-5, -3e-5, 1.0]], np.float32)
    todo += [(M, w, h) for M in (hom, hom[:2], drift) for (w, h) in ((1, 1), (2, 3), (4097, 2), (3, 4097))]
    for M, w, h in todo:
        got, exp = capi.warp_tables(M, w, h), rm.warp_tables(M, w, h)
        for name, g, e in zip(("ac", "df", "gi", "by", "ey", "hy"), got, exp):
            assert (g is None) == (e is None), name
            if e is not None:
                assert g.shape == e.shape and (bits(g) == bits(e)).all(), (name, w, h)
    ac = capi.warp_tables(drift, 4097, 1)[0]
    assert ac[4096] != np.float32(0.1) * np.float32(4096) + np.float32(-7.7), "the running sum is not a * i + c"


def test_warp_tables_refuses_without_writing():
    from compv_amd import capi
    lib = capi.load()
    M = np.eye(3, dtype=np.float32)
    t = [np.full(4, 7, np.float32) for _ in range(6)]
    p = [capi._ptr(a) for a in t]
    for args in ((None, 3, 4, 4, *p), (capi._ptr(M), 1, 4, 4, *p), (capi._ptr(M), 4, 4, 4, *p), (capi._ptr(M), 3, 0, 4, *p), (capi._ptr(M), 3, 4, 0, *p),
                 (capi._ptr(M), 3, 4, 4, None, *p[1:]), (capi._ptr(M), 3, 4, 4, p[0], p[1], None, *p[3:]), (capi._ptr(M), 3, 4, 4, *p[:5], None)):
        assert lib.compvhip_warp_tables(*args) == capi.E_INVALID_PARAMETER
    assert all((a == 7).all() for a in t)
    assert lib.compvhip_warp_tables(capi._ptr(M), 2, 4, 4, p[0], p[1], None, p[3], p[4], None) == capi.OK          # two rows need no gi, hy
    assert (t[2] == 7).all() and (t[5] == 7).all() and (t[0] == [0, 1, 2, 3]).all()


def test_null_handles_are_refused_before_any_hip_call():
    from compv_amd import capi
    lib = capi.load()
    assert lib.compvhip_plan_remap(None, None, None, None, 1, 1, None, 0, None, 4, 4, 4, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_plan_warp_inverse(None, None, None, 2, 1, 1, 0, None, 4, 4, 4, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_remap_u8(None, None, 4, 4, 4, None, None, 1, None, 0, None, 4, 4, 4) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_warp_inverse_u8(None, None, 4, 4, 4, None, 2, 1, 0, None, 4, 4, 4) == capi.E_INVALID_PARAMETER


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def test_the_model_equals_the_reference_planes(golden):
    G, A = golden
    planes = 0
    for r, c in zip(G["remap"], rc.remap_cases()):
        w, h, wo, ho = c["size"]
        img = rc.frame(w, h, c["seed"])
        x, y = rc.random_map(w, h, wo, ho, c["map_seed"])
        assert set(r["md5"]) == {rc.INTERP_NAMES[i] for i in rc.interps_of(wo)}
        for interp in rc.interps_of(wo):
            assert same(rm.remap(img, x, y, interp, c["roi"], c["default"]), A["%s_%s" % (c["id"], rc.INTERP_NAMES[interp])]), (c["id"], interp)
            planes += 1
    for r, c in zip(G["warp"], rc.warp_cases()):
        w, h, wo, ho = c["size"]
        img = rc.frame(w, h, c["seed"])
        for interp in rc.interps_of(wo):
            name = "%s_%s" % (c["id"], rc.INTERP_NAMES[interp])
            if c["nan"] and interp == rm.NEAREST:
                assert name not in A.files          # the reference's nearest leaf takes a NaN for inside: never run there
                continue
            assert same(rm.warp_inverse(img, c["M"], wo, ho, interp, c["default"]), A[name]), name
            planes += 1
    assert planes == len(A.files) == 55


def test_the_z_case_holds_infinities_and_a_nan_and_they_are_outside():
    c = rc.warp_cases()[-1]
    w, h, wo, ho = c["size"]
    x, y = rm.warp_coords(c["M"], wo, ho)
    assert np.isinf(x[:, 8]).all() and np.isnan(y[0, 8]) and np.isinf(y[1:, 8]).all()
    for interp in (rm.NEAREST, rm.BILINEAR, rm.BILINEAR_FLOAT32):
        out = rm.warp_inverse(rc.frame(w, h, c["seed"]), c["M"], wo, ho, interp, c["default"])
        assert (out[:, 8] == c["default"]).all() and (out[:, 9:14] != c["default"]).any()


def test_fma32_rounds_once():
    # (2^-12 + 2^-30)(2^-12 - 2^-30) = 2^-24 - 2^-60, exact in float64; added to 1 + 2^-23, float64 rounds the sum up to 1 + 2^-23 + 2^-24, the midpoint of two
    # float32, which then ties to even: 1 + 2^-22.  The sum lies BELOW that midpoint: one rounding gives 1 + 2^-23.
    twice = (np.float32(2.0 ** -12 + 2.0 ** -30), np.float32(2.0 ** -12 - 2.0 ** -30), np.float32(1.0 + 2.0 ** -23))
    cases = [twice, (np.float32(2.0 ** -30), np.float32(2.0 ** -30), np.float32(1.0)), (np.float32(3.0), np.float32(5.0), np.float32(-15.0)),
             (np.float32(2.0 ** -70), np.float32(2.0 ** -70), np.float32(0.0))]
    rng = np.random.default_rng(5)
    cases += [(np.float32(v[0]), np.float32(v[1]), np.float32(v[2])) for v in rng.uniform(-256, 256, (200, 3))]
    A, B, Cc = (np.array(v, np.float32) for v in zip(*cases))
    before = rm.fma32.redone
    got = rm.fma32(A, B, Cc)
    for k, (p, q, r) in enumerate(cases):
        exact = Fraction(float(p)) * Fraction(float(q)) + Fraction(float(r))
        lo = np.float32(float(exact))
        best = min((np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))),
                   key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert got[k].view(np.uint32) == np.float32(best).view(np.uint32), (k, p, q, r)
    assert rm.fma32.redone > before, "the midpoint case takes the exact path"
    assert got[0] == np.float32(1.0 + 2.0 ** -23)
    assert np.float32(np.float64(twice[0]) * np.float64(twice[1]) + np.float64(twice[2])) == np.float32(1.0 + 2.0 ** -22), "float64 emulation rounds this one twice"
