"""tests/bicubic_model.py -- paragraph F of the remap definition in numpy -- against the fixtures tests/golden/make_golden_bicubic.py wrote after holding
the model against the compiled reference (SIMD flags off) on every element: golden_bicubic.npz holds the planes, golden_bicubic.json their MD5s and what
each was checked against.  No GPU."""
import functools

import numpy as np
import pytest

import bicubic_cases as bc
import bicubic_model as bm
import remap_cases as rc
import remap_model as rm
from fixtures import load_golden, md5

G, A = load_golden("golden_bicubic")
MAPS = {c["id"]: c for c in bc.all_map_cases()}
WARPS = {c["id"]: c for c in bc.warp_cases()}


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@functools.lru_cache(maxsize=None)
def frame_of(cid):
    c = MAPS.get(cid) or WARPS[cid]
    return rc.frame(c["size"][0], c["size"][1], c["seed"])


def test_the_fixture_lists_every_case_and_only_nan_cases_are_model_only():
    assert [r["id"] for r in G["remap"]] == list(MAPS) and [r["id"] for r in G["warp"]] == list(WARPS)
    assert sorted(A.files) == sorted(bc.key(cid, i) for cid in list(MAPS) + list(WARPS) for i in bc.INTERPS)
    for r in G["remap"] + G["warp"]:
        for name in bc.INTERP_NAMES.values():
            assert r["checked"][name] == "reference" or (r["nan"] and r["checked"][name].startswith("model only: ")), r["id"]
    assert sum(r["nan"] for r in G["remap"] + G["warp"]) == 2


@pytest.mark.parametrize("cid", list(MAPS))
def test_model_equals_the_fixture_on_the_maps(cid):
    c = MAPS[cid]
    x, y = bc.map_of(c)
    rec = next(r for r in G["remap"] if r["id"] == cid)
    for interp in bc.INTERPS:
        got = bm.remap(frame_of(cid), x, y, interp, c["roi"], c["default"])
        assert same(got, A[bc.key(cid, interp)]), (cid, interp)
        assert md5(got) == rec["md5"][bc.INTERP_NAMES[interp]]


@pytest.mark.parametrize("cid", list(WARPS))
def test_model_equals_the_fixture_on_the_matrices(cid):
    c = WARPS[cid]
    rec = next(r for r in G["warp"] if r["id"] == cid)
    for interp in bc.INTERPS:
        got = bm.warp_inverse(frame_of(cid), c["M"], c["size"][2], c["size"][3], interp, c["default"])
        assert same(got, A[bc.key(cid, interp)]), (cid, interp)
        assert md5(got) == rec["md5"][bc.INTERP_NAMES[interp]]


def test_nan_and_infinite_coordinates_are_outside():
    c = MAPS["map_nan"]
    for interp in bc.INTERPS:
        plane = A[bc.key("map_nan", interp)]
        for (j, i, _, _) in bc.NAN_ENTRIES:
            assert plane[j, i] == c["default"]
        assert (plane != c["default"]).mean() > 0.9
    z = WARPS["warp_z_sign"]
    for interp in bc.INTERPS:
        assert (A[bc.key("warp_z_sign", interp)][:, 8] == z["default"]).all(), "Z == 0: infinities and a NaN"


@pytest.mark.parametrize("cid", ["map0", "map1", "map4", "map_roi"])
def test_the_fixture_exercises_the_clip_and_the_cast(cid):
    """noise frames overshoot: the unclipped value leaves [0, 255] on both sides, and truncation is not rounding"""
    c = MAPS[cid]
    x, y = bc.map_of(c)
    img = frame_of(cid)
    inside = bm.inside_of(img, x, y, c["roi"])
    v = bm.unclipped(img, x[inside], y[inside])
    below, above = int((v < 0).sum()), int((v > 255).sum())
    w = bm.clip255(v)
    rounding = int((w.astype(np.int32) != np.rint(w).astype(np.int32)).sum())
    print(cid, "below 0:", below, "above 255:", above, "truncation differs from rounding:", rounding)
    assert below >= 1 and above >= 1
    assert rounding > 100
    u8, f32 = A[bc.key(cid, bm.BICUBIC)], A[bc.key(cid, bm.BICUBIC_FLOAT32)]
    assert (f32[inside] == w).all() and (u8[inside] == w.astype(np.int32)).all()
    assert f32.min() >= 0 and f32.max() <= 255


def test_the_two_hermite_expressions_differ_in_bits():
    """HERMITE4_32F_C along the rows, HERMITE1_32F_C down the column: swapping them, or using the row expression for both, changes float32 planes of the
    fixtures.  (The column expression along the rows changes nothing: the taps are integers up to 255, so the coefficients a, b, c of a row are exact in
    either association.  The two differ on the row values, which are not integers.)"""
    changed = {"swapped": 0, "row twice": 0}
    for cid in ("map0", "map1"):
        c = MAPS[cid]
        x, y = bc.map_of(c)
        ref = A[bc.key(cid, bm.BICUBIC_FLOAT32)]
        for name, (row, col) in (("swapped", (bm.hermite_col, bm.hermite_row)), ("row twice", (bm.hermite_row, bm.hermite_row))):
            got = bm.remap(frame_of(cid), x, y, bm.BICUBIC_FLOAT32, c["roi"], c["default"], row=row, col=col)
            changed[name] += int((got.view(np.uint32) != ref.view(np.uint32)).sum())
    assert all(v > 0 for v in changed.values()), changed


def test_the_model_computes_in_float32_only():
    x, y = bc.map_of(MAPS["map3"])
    img = frame_of("map3")
    inside = bm.inside_of(img, x, y, None)
    assert bm.unclipped(img, x[inside], y[inside]).dtype == np.float32
    assert all(a.dtype == np.float32 for a in bm.split(x[inside])[1:])
    assert rm.warp_coords(WARPS["warp0_homography"]["M"], 8, 8)[0].dtype == np.float32
