"""tests/hog_model.py -- the numpy float32 statement of the HOG definition (include/compv_hip.h, "HOG descriptors") -- against the goldens that
tests/golden/make_golden_hog.py wrote after it had found model == compiled reference (AVX2 + FMA3 off) byte for byte on every case.  CPU only."""
import os

import numpy as np
import pytest

import hog_cases as hc
import hog_model as hm
from fixtures import GOLDEN_DIR, load_golden, md5


@pytest.fixture(scope="module")
def golden():
    meta, arrays = load_golden("golden_hog")
    return {c["id"]: c for c in meta["cases"]}, arrays, meta


def test_the_goldens_cover_the_case_list(golden):
    by_id, arrays, meta = golden
    assert sorted(by_id) == sorted(hc.BY_ID)
    assert sorted(arrays.files) == sorted("desc_" + c["id"] for c in by_id.values() if c["stored"])
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "golden_hog.npz")) <= 292745          # no larger than golden_homography.npz
    # the reference's fused AVX2 leaf is recorded, never compared: it differs from the definition in the last bits only
    assert meta["avx2_fma3"]["differs"] and 0 < meta["avx2_fma3"]["max_abs_difference"] < 1e-6


@pytest.mark.parametrize("cid", [c["id"] for c in hc.CASES])
def test_model_equals_the_golden_bit_for_bit(golden, cid):
    by_id, arrays, _ = golden
    c, g = hc.BY_ID[cid], by_id[cid]
    img = hc.case_frame(c)
    assert md5(img) == g["frame_md5"], "the frame generator drifted"
    assert hm.geometry(c["W"], c["H"], c["opts"]) == g["geometry"]
    desc, cells = hm.hog(img, c["opts"])
    assert desc.dtype == np.float32 and cells.dtype == np.float32 and desc.size == g["geometry"]["descLen"]
    assert md5(desc) == g["desc_md5"] and md5(cells) == g["cells_md5"]
    if g["stored"]:
        assert desc.tobytes() == arrays["desc_" + cid].tobytes()
    if c["kind"] == "constant":
        assert not desc.view(np.uint32).any() and not cells.view(np.uint32).any()          # +0.0 everywhere, under every norm


def test_geometry_rules():
    g = hm.geometry(64, 48, hc.layout(8, 4, 8))          # stride = cell / 2: twice the cells, the last column and row left out
    assert (g["cellsX"], g["validX"], g["cellsY"], g["validY"], g["blocksX"], g["blocksY"], g["stepX"], g["count"]) == (16, 15, 12, 11, 15, 11, 1, 9)
    g = hm.geometry(37, 29, hc.layout(8, 4, 8))          # 37 = 4 * 8 + 5: the last origin 28 + 8 <= 37 stays; 29 = 3 * 8 + 5: 20 + 8 <= 29 stays too
    assert (g["cellsX"], g["validX"], g["cellsY"], g["validY"]) == (8, 8, 6, 6)
    g = hm.geometry(35, 27, hc.layout(8, 4, 8))          # 28 + 8 > 35 and 20 + 8 > 27: both left out
    assert (g["cellsX"], g["validX"], g["cellsY"], g["validY"]) == (8, 7, 6, 5)
    g = hm.geometry(3840, 2160, None)
    assert (g["cellsX"], g["cellsY"], g["blocksX"], g["blocksY"], g["count"], g["descLen"]) == (480, 270, 479, 269, 36, 479 * 269 * 36)
    assert hm.geometry(64, 128, {})["descLen"] == 3780          # the pedestrian window


@pytest.mark.parametrize("W,H,o", [
    (64, 64, hc.layout(16, 8, 6)),                                   # block % cell != 0
    (64, 64, hc.layout(16, 4, 8)),                                   # stride = cell / 2 needs block == cell
    (64, 64, hc.layout(16, 16, 8)),                                  # stride > cell
    (64, 64, hc.layout(16, 3, 8)),                                   # any other stride
    (64, 64, hc.layout((16, 16), (8, 4), (8, 8))),                   # ... in y alone
    (64, 64, hc.layout(16, 8, 8, 1)), (64, 64, hc.layout(16, 8, 8, 361)),            # 2 <= nbins <= 360
    (64, 64, hc.layout(16, 8, 8, 7)), (64, 64, hc.layout(16, 8, 8, 8, signed=False)), (64, 64, hc.layout(16, 8, 8, 360, signed=False)),   # nbins divides thetaMax
    (15, 64, hc.layout(16, 8, 8)), (64, 15, hc.layout(16, 8, 8)),    # the frame holds one block
    (64, 64, hc.layout(16, 8, 8, interp=hm.INTERP_BILINEAR_LUT)), (64, 64, hc.layout(16, 8, 8, interp=4)),
    (64, 64, hc.layout(16, 8, 8, norm=6)), (64, 64, dict(gradientSigned=3)), (64, 64, dict(cellW=-8)),
])
def test_refused_parameters(W, H, o):
    assert hm.geometry(W, H, o) is None


def test_the_dropped_vote_and_the_order_of_the_two_additions():
    """NEAREST, unsigned: a pixel with gy == 0 and gx < 0 has theta == 180 == thetaMax, bin index nbins: its magnitude appears in no bin"""
    img = np.zeros((16, 16), np.uint8)
    img[:, :8] = 200          # a vertical edge: gx = -200 at x = 7 and 8, gy = 0
    o = hc.layout(16, 8, 8, signed=False, interp=hm.INTERP_NEAREST, norm=hm.NORM_NONE)
    _, cells = hm.hog(img, o)
    assert not cells.any()
    _, cells = hm.hog(img[:, ::-1], o)          # gx = +200: bin 0 takes them all
    assert cells[:, :, 0].sum() == 200.0 * 2 * 16 and not cells[:, :, 1:].any()
    # BILINEAR: the two additions of a pixel go to different bins, and every histogram value is a sum of non-negative terms
    d, cells = hm.hog(hc.noise(37, 29), hc.layout(16, 8, 8, norm=hm.NORM_NONE))
    assert (cells >= 0).all() and (d >= 0).all()
