"""tests/undistort_model.py -- the numpy statement of the lens-undistortion definition (include/compv_hip.h, "lens undistortion") -- against the fixture
that tests/golden/make_golden_undistort.py made from the compiled reference: every map plane (float32 bytes, float64 by MD5), every point and
projection case, and the image of every case for all five interpolations.  The GPU tests (tests/test_gpu_undistort.py) hold the kernels against the
same fixture."""
import numpy as np
import pytest

import undistort_cases as uc
import undistort_model as um
from fixtures import load_golden, md5


@pytest.fixture(scope="module")
def golden():
    return load_golden("golden_undistort")


def test_the_fixture_covers_the_case_list(golden):
    meta, arrays = golden
    assert [r["id"] for r in meta["images"]] == [c["id"] for c in uc.image_cases()]
    assert [r["id"] for r in meta["points"]] == [c["id"] for c in uc.point_cases()]
    assert [r["id"] for r in meta["proj"]] == [c["id"] for c in uc.proj_cases()]
    assert len({m["id"] for m in meta["model_only"]}) <= 2
    shares = [r["outside_share"] for r in meta["images"]]
    assert any(0.05 <= s <= 0.60 for s in shares) and any(s == 0.0 for s in shares)
    assert {r["nd"] for r in meta["images"]} == {2, 3, 4}
    z0 = next(r for r in meta["proj"] if r["id"] == "proj_z0")
    assert 0 < z0["z_zero"] < z0["n"]


@pytest.mark.parametrize("c", uc.image_cases(), ids=lambda c: c["id"])
def test_maps_and_images(golden, c):
    meta, arrays = golden
    rec = next(r for r in meta["images"] if r["id"] == c["id"])
    w, h, wo, ho = c["size"]
    mx, my = um.map_planes(c["K"], c["d"], wo, ho, *c["origin"], dtype=np.float32)
    assert mx.tobytes() == arrays["mapx_" + c["id"]].tobytes() and my.tobytes() == arrays["mapy_" + c["id"]].tobytes()
    dx, dy = um.map_planes(c["K"], c["d"], wo, ho, *c["origin"], dtype=np.float64)
    assert dx.dtype == np.float64 and (md5(dx), md5(dy)) == (rec["md5"]["mapx_f64"], rec["md5"]["mapy_f64"])
    assert round(um.outside_share(w, h, mx, my, c["roi"]), 4) == rec["outside_share"]
    img = uc.frame(c)
    for interp in um.INTERPS:
        out = um.undistort(img, c["K"], c["d"], wo, ho, *c["origin"], interp=interp, roi=c["roi"], default=c["default"])
        assert md5(out) == rec["md5"][um.INTERP_NAMES[interp]], um.INTERP_NAMES[interp]


@pytest.mark.parametrize("c", uc.point_cases(), ids=lambda c: c["id"])
def test_points(golden, c):
    cam = uc.case(c["camera"])
    got = um.dist_points(cam["K"], cam["d"], uc.points(c), c["dtype"])
    assert got.dtype == c["dtype"] and got.tobytes() == golden[1][c["id"]].tobytes()


@pytest.mark.parametrize("c", uc.proj_cases(), ids=lambda c: c["id"])
def test_projection(golden, c):
    cam = uc.case(c["camera"])
    got = um.proj2d(cam["K"], cam["d"], c["R"], c["t"], uc.proj_points(c))
    assert got.tobytes() == golden[1][c["id"]].tobytes()


def test_a_singular_camera_has_no_coefficients():
    assert um.coeffs([[0.0, 0, 1], [0, 2.0, 1], [0, 0, 1]], (0.1, 0.2)) is None
    assert um.coeffs([[3.0, 0, 1], [0, 0.0, 1], [0, 0, 1]], (0.1, 0.2), np.float64) is None
