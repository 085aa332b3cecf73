"""The ORB pyramid on the GPU (compvhip_orbpyr_*, compvhip_orb_pyramid_u8) against tests/orb_pyramid_model.py byte for byte: level geometry, level planes,
counts per frame and per level, keypoint records in level order, descriptor rows -- and the level planes of the 100 x 90 golden case against what the
compiled reference wrote (tests/golden/golden_orb_pyramid.npz).  Three frames per geometry (noise, blocks, flat: no corner at all), S > W, guarded buffers
from the Arena of tests/gpu_support.py with outputs pre-filled with a sentinel, the input registered as kept."""
import functools

import numpy as np
import pytest

import fast_model as fm
import match_model as mm
import orb_model as om
import orb_pyramid_model as pm
from gpu_support import SENTINEL, Arena, ptr
from orb_pyramid_rig import GOLD_100x90, KREC, THRESHOLD, A, F, Rig, batch, opts_of

pytestmark = pytest.mark.gpu

# W, H, S, levels, scale factor, maxFeatures: the four geometries of rule B.5
GEOMETRIES = ((200, 258, 208, 8, 0.83, 500), (100, 90, 112, 8, 0.83, 60), (64, 41, 72, 8, 0.83, 2000), (96, 80, 104, 3, 0.5, 2000))
GID = lambda g: "%dx%d_L%d_mf%d" % (g[0], g[1], g[3], g[5])          # noqa: E731


@functools.lru_cache(maxsize=None)
def model(W, H, levels, sf, mf, corner_cap=None, threshold=THRESHOLD):
    """per frame: (keys, level counts, level corners, planes), and the geometry"""
    geo = pm.geometry(W, H, levels, sf, mf)
    return [pm.detect(img, levels, sf, threshold, 9, True, mf, corner_cap) for img in batch(W, H)], geo


@pytest.mark.parametrize("geom", GEOMETRIES, ids=GID)
def test_detect_and_describe_match_the_model(hip_ctx, geom):
    W, H, S, levels, sf, mf = geom
    exp, geo = model(W, H, levels, sf, mf)
    total = max(len(e[0]) for e in exp)
    assert total > 0 and len(exp[2][0]) == 0, "the flat frame has no corner"
    rig = Rig(hip_ctx, geom, key_cap=total + 7, desc_stride=36)
    try:
        for l, g in enumerate(geo):          # host arithmetic of the object against the model
            gw, gh, gs, gsf, gq = rig.pyr.geometry(l)
            assert (gw, gh, gq) == (g["W"], g["H"], g["quota"]) and gsf.view(np.uint32) == np.float32(g["scale"]).view(np.uint32)
            assert gs == (0 if g["empty"] else (S if l == 0 else g["S"]))
        rig.detect()
        rig.check_detect("detect", exp)
        first = (rig.d_keys.cpu().numpy().copy(), rig.d_kcounts.cpu().numpy().copy(), rig.d_lcounts.cpu().numpy().copy())
        for l, g in enumerate(geo):          # the level planes the call built
            if g["empty"]:
                continue
            got = rig.level_planes(l, geo)
            for f in range(F):
                assert (got[f] == exp[f][3][l]).all(), "level %d frame %d plane" % (l, f)
            key = "c%d_l%d_plane" % (GOLD_100x90, l)
            if (W, H) == (100, 90) and l:
                assert (got[0] == A[key]).all(), "level %d against the reference's plane" % l
        counts = [len(e[0]) for e in exp]
        exp_rows = [pm.describe(e[3], geo, e[0]) for e in exp]
        assert any(r.any() for r in exp_rows)
        rig.pyr.describe(ptr(rig.d_in), ptr(rig.d_keys), rig.key_cap, ptr(rig.d_kcounts), ptr(rig.d_desc), rig.desc_stride, reuse_planes=True)
        rig.ar.check("describe, reused planes")
        reused = rig.rows().copy()
        rig.check_rows("reused planes", reused, exp_rows, counts)
        for l, g in enumerate(geo):
            if not g["empty"]:
                got = rig.level_planes(l, geo, blurred=True)
                assert all((got[f] == om.blur(exp[f][3][l])).all() for f in range(F)), "level %d blurred plane" % l
        rig.ar.refill(rig.d_desc)
        rig.pyr.describe(ptr(rig.d_in), ptr(rig.d_keys), rig.key_cap, ptr(rig.d_kcounts), ptr(rig.d_desc), rig.desc_stride, reuse_planes=False)
        rig.ar.check("describe, rebuilt planes")
        assert (rig.rows() == reused).all(), "reusePlanes 0 and 1 give equal rows"
        # a second run writes the same bytes
        rig.ar.refill(rig.d_keys)
        rig.detect()
        rig.check_detect("detect again", exp)
        assert (rig.d_keys.cpu().numpy() == first[0]).all() and (rig.d_kcounts.cpu().numpy() == first[1]).all() and (rig.d_lcounts.cpu().numpy() == first[2]).all()
    finally:
        rig.close()


def test_one_level_is_the_single_level_chain(hip_ctx):
    """levels = 1 reproduces compvhip_plan_fast -> compvhip_plan_orb_keypoints -> compvhip_plan_orb_describe byte for byte"""
    from compv_amd import capi
    W, H, S = 200, 258, 208
    cap, ccap, mf = 700, 8192, 300
    rig = Rig(hip_ctx, (W, H, S, 1, 0.83, mf), key_cap=cap)
    plan = capi.Plan(hip_ctx, W, H, S, F)
    try:
        ar = rig.ar
        d_corners, d_ccounts = ar.new(F * ccap * om.CORNER_DTYPE.itemsize), ar.new(4 * F)
        d_keys, d_kcounts, d_desc = ar.new(F * cap * KREC), ar.new(4 * F), ar.new(F * cap * 32)
        quota = pm.geometry(W, H, 1, 0.83, mf)[0]["quota"]
        assert quota == mf          # one level: sfs = 1
        plan.fast(ptr(rig.d_in), THRESHOLD, 9, True, quota, 0, ptr(d_corners), ccap, ptr(d_ccounts))
        plan.orb_keypoints(ptr(rig.d_in), ptr(d_corners), ccap, ptr(d_ccounts), 0, 1.0, ptr(d_keys), cap, ptr(d_kcounts))
        plan.orb_describe(ptr(rig.d_in), ptr(d_keys), cap, ptr(d_kcounts), 1.0, ptr(d_desc))
        rig.detect()
        rig.pyr.describe(ptr(rig.d_in), ptr(rig.d_keys), cap, ptr(rig.d_kcounts), ptr(rig.d_desc), 32, reuse_planes=True)
        ar.check("one level")
        counts = rig.ints(d_kcounts, F)
        assert counts[0] > mf // 2 and counts[2] == 0
        assert (rig.d_kcounts.cpu().numpy() == d_kcounts.cpu().numpy()).all() and (rig.ints(rig.d_lcounts, F) == counts).all()
        assert (rig.ints(rig.d_lcorners, F) == rig.ints(d_ccounts, F)).all()
        assert (rig.d_keys.cpu().numpy() == d_keys.cpu().numpy()).all() and (rig.d_desc.cpu().numpy() == d_desc.cpu().numpy()).all()
    finally:
        plan.close()
        rig.close()


def test_key_cap_clips_inside_a_level(hip_ctx):
    geom = GEOMETRIES[0]
    W, H, S, levels, sf, mf = geom
    exp, _ = model(W, H, levels, sf, mf)
    lc = exp[0][1]
    assert lc[2] >= 2
    cap = int(lc[0] + lc[1] + lc[2] // 2)          # frame 0 is cut in the middle of level 2
    assert len(exp[1][0]) != len(exp[0][0])
    rig = Rig(hip_ctx, geom, key_cap=cap)
    try:
        rig.detect()
        rig.check_detect("clipped", exp)
        keys = np.frombuffer(rig.d_keys.cpu().numpy().tobytes(), om.KEYPOINT_DTYPE).reshape(F, cap)
        assert keys[0, -1]["level"] == 2 and rig.ints(rig.d_kcounts, F)[0] > cap
        rig.detect(key_cap=0)          # counts only
        rig.check_detect("counts only", exp)
    finally:
        rig.close()


def test_corner_cap_below_the_corner_count(hip_ctx):
    W, H, S, levels, sf = 100, 90, 112, 8, 0.83
    ccap = 50
    exp, _ = model(W, H, levels, sf, 0, ccap)
    full, _ = model(W, H, levels, sf, 0)
    assert exp[0][2][0] > ccap and exp[0][2].tolist() == full[0][2].tolist(), "d_levelCorners reports the overflow"
    assert exp[0][1][0] < full[0][1][0], "level 0's list was truncated to its raster prefix"
    rig = Rig(hip_ctx, (W, H, S, levels, sf, 0), key_cap=1024, corner_cap=ccap)
    try:
        rig.detect()
        rig.check_detect("corner cap", exp)
    finally:
        rig.close()


def test_quota_floor_and_ties_at_the_cut(hip_ctx):
    geom = (200, 258, 208, 8, 0.83, 60)
    W, H, S, levels, sf, mf = geom
    exp, geo = model(W, H, levels, sf, mf)
    assert [g["quota"] for g in geo] == [13, 11, 10, 10, 10, 10, 10, 10], "the floor of 10"
    assert any(exp[0][2][l] > geo[l]["quota"] for l in range(levels)), "a tie at the cut keeps more than the quota"
    rig = Rig(hip_ctx, geom, key_cap=256)
    try:
        rig.detect()
        rig.check_detect("small quota", exp)
    finally:
        rig.close()


def test_callers_keypoints_with_mixed_and_invalid_levels(hip_ctx):
    geom = GEOMETRIES[1]          # 100 x 90: levels 5 .. 7 are empty
    W, H, S, levels, sf, _ = geom
    exp, geo = model(W, H, levels, sf, 0)
    cap = 256
    rig = Rig(hip_ctx, (W, H, S, levels, sf, 0), key_cap=cap)
    try:
        rng = np.random.default_rng(5)
        host = np.zeros((F, cap), om.KEYPOINT_DTYPE)
        host.view(np.uint8)[:] = 0x5A          # behind the count: records that must not be read
        counts, lists = np.zeros(F, np.int32), []
        for f in range(F):
            k = exp[0][0].copy() if f == 2 else exp[f][0].copy()          # the flat frame takes frame 0's records: its own list is empty
            k = k[rng.permutation(len(k))][:cap - 9]
            assert len(np.unique(k["level"])) >= 3
            k["level"][0::11] = -1
            k["level"][1::11] = levels
            k["level"][2::11] = 6          # an empty level
            k["level"][3::11] = 1 << 30
            lists.append(k)
            host[f, :len(k)] = k
            counts[f] = len(k)
        rig.d_keys.copy_(rig.ar.torch.from_numpy(np.frombuffer(host.tobytes(), np.uint8).copy()))
        rig.d_kcounts.copy_(rig.ar.torch.from_numpy(np.frombuffer(counts.tobytes(), np.uint8).copy()))
        rig.pyr.describe(ptr(rig.d_in), ptr(rig.d_keys), cap, ptr(rig.d_kcounts), ptr(rig.d_desc), 32, reuse_planes=False)
        rig.ar.check("mixed levels")
        assert rig.d_keys.cpu().numpy().tobytes() == host.tobytes(), "the caller's keypoints are read only"
        exp_rows = [pm.describe(exp[f][3], geo, lists[f]) for f in range(F)]
        for f in range(F):
            bad = ~np.isin(lists[f]["level"], np.arange(5))
            assert bad.sum() >= 4 and not exp_rows[f][bad].any() and exp_rows[f][~bad].any()
        rig.check_rows("mixed levels", rig.rows(), exp_rows, counts)
        from compv_amd import capi
        with pytest.raises(capi.CompvHipError) as e:          # the planes were built from d_in: another frame pointer has nothing to reuse
            rig.pyr.describe(ptr(rig.d_keys), ptr(rig.d_keys), cap, ptr(rig.d_kcounts), ptr(rig.d_desc), 32, reuse_planes=True)
        assert e.value.code == capi.E_INVALID_STATE
    finally:
        rig.close()


def test_detect_describe_match_on_one_stream(hip_ctx):
    """detect -> describe -> matcher_knn enqueued on one stream, every count read from device memory, one synchronisation at the end; the pair is an image
    and its np.rot90"""
    import torch
    from compv_amd import capi
    W = H = S = 96
    Fp, cap, levels, sf, mf = 2, 512, 3, 0.75, 0
    img = fm.blocks(W, H, 11)
    frames = np.stack([img, np.ascontiguousarray(np.rot90(img))])
    ar = Arena()
    d_in = ar.new(frames.size, frames.reshape(-1))
    ar.keep(d_in, frames)
    d_keys, d_kcounts, d_desc = ar.new(Fp * cap * KREC), ar.new(4 * Fp), ar.new(Fp * cap * 32)
    d_matches = ar.new(2 * cap * 16)
    pyr = capi.OrbPyramid(hip_ctx, W, H, S, Fp, opts_of(levels, sf, mf, 30), 2048)
    matcher = capi.Matcher(hip_ctx, 32, cap, cap, 1, 2)
    try:
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        s = st.cuda_stream
        pyr.detect(ptr(d_in), ptr(d_keys), cap, ptr(d_kcounts), 0, 0, s)
        pyr.describe(ptr(d_in), ptr(d_keys), cap, ptr(d_kcounts), ptr(d_desc), 32, True, s)
        matcher.knn(ptr(d_desc), 32, ptr(d_kcounts), ptr(d_desc) + cap * 32, 32, ptr(d_kcounts) + 4, False, ptr(d_matches), s)
        st.synchronize()
        ar.check("chain")
        geo = pm.geometry(W, H, levels, sf, mf)
        runs = [pm.detect(frames[f], levels, sf, 30, 9, True, mf) for f in range(Fp)]
        exp_k = [r[0] for r in runs]
        exp_d = [pm.describe(r[3], geo, r[0]) for r in runs]
        n0, n1 = len(exp_k[0]), len(exp_k[1])
        assert 8 <= n0 <= cap and 8 <= n1 <= cap and len(np.unique(exp_k[0]["level"])) >= 2
        assert np.frombuffer(d_kcounts.cpu().numpy().tobytes(), np.int32).tolist() == [n0, n1]
        keys = d_keys.cpu().numpy().tobytes()
        desc = d_desc.cpu().numpy().reshape(Fp, cap, 32)
        for f in range(Fp):
            assert keys[f * cap * KREC:f * cap * KREC + len(exp_k[f]) * KREC] == exp_k[f].tobytes()
            assert desc[f, :len(exp_d[f])].tobytes() == exp_d[f].tobytes() and (desc[f, len(exp_d[f]):] == SENTINEL).all()
        got = np.frombuffer(d_matches.cpu().numpy().tobytes(), mm.MATCH_DTYPE).reshape(2, cap)
        assert got[:, :n0].tobytes() == mm.knn_device(exp_d[0], exp_d[1], 2).tobytes()
    finally:
        matcher.close()
        pyr.close()


def test_host_entry_and_its_out_of_bound_prefix(hip_ctx):
    import ctypes as C
    from compv_amd import capi
    W, H, levels, sf, mf = 100, 90, 8, 0.83, 60
    img = batch(W, H)[0]
    (keys, _, _, planes), geo = model(W, H, levels, sf, mf)[0][0], pm.geometry(W, H, levels, sf, mf)
    rows = pm.describe(planes, geo, keys)
    wide = np.full((H, W + 3), 9, np.uint8)
    wide[:, :W] = img
    o = opts_of(levels, sf, mf)
    gk, gd = hip_ctx.orb_pyramid(wide[:, :W], o, cap=len(keys) + 5)
    assert gk.tobytes() == keys.tobytes() and (gd == rows).all() and len(keys) >= 8
    gk, gd = hip_ctx.orb_pyramid(wide[:, :W], o, cap=3)          # the binding repeats the call with the reported size
    assert gk.tobytes() == keys.tobytes() and (gd == rows).all()
    cap = len(keys) - 3
    k = np.zeros(len(keys), om.KEYPOINT_DTYPE)
    d = np.full((len(keys), 32), SENTINEL, np.uint8)
    n = C.c_size_t(0)
    rc = hip_ctx.lib.compvhip_orb_pyramid_u8(hip_ctx.h, img.ctypes.data, W, H, W, C.byref(o), k.ctypes.data, d.ctypes.data, 32, cap, C.byref(n))
    assert rc == capi.E_OUT_OF_BOUND and n.value == len(keys)
    assert k[:cap].tobytes() == keys[:cap].tobytes() and not k[cap:]["size"].any() and (d[:cap] == rows[:cap]).all() and (d[cap:] == SENTINEL).all()
    dk, dd = hip_ctx.orb_pyramid(fm.blocks(200, 258, 3))          # the defaults: opts == NULL
    mk = pm.detect(fm.blocks(200, 258, 3))
    assert dk.tobytes() == mk[0].tobytes() and (dd == pm.describe(mk[3], pm.geometry(200, 258), mk[0])).all()


def test_refusals_and_live_allocations(hip_ctx):
    from compv_amd import capi
    before = hip_ctx.live_allocations()
    for (W, H, S, levels, sf, fast_type, ccap) in ((36, 90, 40, 8, 0.83, 9, 64), (100, 36, 104, 8, 0.83, 9, 64), (100, 90, 100, 8, 0.83, 9, 64), (100, 90, 104, 0, 0.83, 9, 64),
                                                   (100, 90, 104, 17, 0.83, 9, 64), (100, 90, 104, 8, 1.0, 9, 64), (100, 90, 104, 8, 0.0, 9, 64), (100, 90, 104, 8, 0.83, 10, 64),
                                                   (100, 90, 104, 8, 0.83, 9, 0)):
        with pytest.raises(capi.CompvHipError) as e:
            capi.OrbPyramid(hip_ctx, W, H, S, F, capi.OrbPyramidOpts(levels, sf, 20, fast_type, True, 2000), ccap)
        assert e.value.code == capi.E_INVALID_PARAMETER, (W, H, S, levels, sf, fast_type, ccap)
    assert hip_ctx.live_allocations() == before
    rig = Rig(hip_ctx, GEOMETRIES[3], key_cap=128)
    try:
        assert hip_ctx.live_allocations() > before
        with pytest.raises(capi.CompvHipError) as e:
            rig.pyr.plane(0)          # nothing built yet
        assert e.value.code == capi.E_INVALID_STATE
        with pytest.raises(capi.CompvHipError) as e:
            rig.pyr.plane(2)          # an empty level
        assert e.value.code == capi.E_INVALID_PARAMETER
        rig.pyr.set_timing(1)
        rig.detect()
        rig.pyr.describe(ptr(rig.d_in), ptr(rig.d_keys), rig.key_cap, ptr(rig.d_kcounts), ptr(rig.d_desc), 32, reuse_planes=True)
        names = [n for n, ms in rig.pyr.get_timing() if ms >= 0]
        assert names == ["convlt_fxp_kernels", "convlt_fxp_kernels", "orb_brief_pyramid_kernel"]
        rig.detect()
        names = [n for n, _ in rig.pyr.get_timing()]
        assert names == ["scale_bilinear_kernel"] + ["fast_score_kernel", "fast_list_kernels", "orb_select_kernel", "orb_orient_kernel"] * 2 + ["orb_pyramid_counts_kernel"]
        rig.ar.check("timing")
    finally:
        rig.close()
    assert hip_ctx.live_allocations() == before


def test_global_byte_variant_writes_the_same_rows(hip_ctx, monkeypatch):
    """COMPVHIP_ORB_BRIEF=global, read when the pyramid is created, runs orb_brief_pyramid_kernel<false>: the rows of the model, under its own timing name"""
    geom = GEOMETRIES[1]
    W, H, S, levels, sf, mf = geom
    exp, geo = model(W, H, levels, sf, mf)
    monkeypatch.setenv("COMPVHIP_ORB_BRIEF", "global")
    rig = Rig(hip_ctx, geom, key_cap=64)
    try:
        rig.detect()
        rig.check_detect("detect", exp)
        rig.pyr.set_timing(1)
        rig.pyr.describe(ptr(rig.d_in), ptr(rig.d_keys), rig.key_cap, ptr(rig.d_kcounts), ptr(rig.d_desc), 32, reuse_planes=True)
        rig.ar.check("global bytes")
        assert [n for n, _ in rig.pyr.get_timing()][-1] == "orb_brief_pyramid_kernel_global"
        rig.check_rows("global bytes", rig.rows(), [pm.describe(e[3], geo, e[0]) for e in exp], [len(e[0]) for e in exp])
    finally:
        rig.close()
