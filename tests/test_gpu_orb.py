"""ORB on the GPU (compvhip_plan_orb_keypoints, compvhip_plan_orb_describe, compvhip_orb_u8) against tests/orb_model.py, byte for byte: counts,
keypoint records, moments and descriptor rows of every frame.  Buffers come from the Arena of tests/gpu_support.py: guards either side,
outputs pre-filled with a sentinel (so whatever must be written is seen to be, and nothing behind a list or a row is), the input registered as kept
(it must come back unchanged: the blur goes to a plane of the plan's own).

The corner lists are made by the test, not by a detector: positions 17 / 18 and W - 19 / W - 18 from every border, the centre column (where a
mirrored frame has m10 == 0), seeded positions anywhere in the frame, repeated where a frame has fewer admissible positions than corners (37 x 37 has
one).  The number of SURVIVORS per frame cycles through 257, 1, 0, 63, 64, 65 (a round of the select kernel is 256 corners, a wave 64).  Frames
cycle through noise, blocks, constant, a horizontal ramp (m01 == 0) and a mirrored frame."""
import numpy as np
import pytest

import fast_model as fm
import match_model as mm
import orb_model as om
from gpu_support import SENTINEL, Arena, pad_frames, ptr
from orb_rig import CREC, KINDS, KREC, Rig, blurred_batch, corner_list, u8

pytestmark = pytest.mark.gpu

GEOMETRIES = ((37, 37, 40, 2), (38, 39, 40, 3), (131, 70, 136, 5), (513, 65, 576, 9), (1001, 333, 1008, 33))          # W, H, S, F
SCALE1 = np.float32(0.83)
GID = lambda g: "%dx%d_S%d_F%d" % g          # noqa: E731


@pytest.mark.parametrize("geom", GEOMETRIES, ids=GID)
def test_orb_geometry_sweep(hip_ctx, geom):
    """level 0 and level 1 (scale 0.83): counts, records, moments and descriptor rows of every frame; then without moments, with a capacity below
    the count (a prefix, the true count, nothing behind) and with capacity 0 (counts only)"""
    W, H, S, F = geom
    seed = W + H
    rig = Rig(hip_ctx, geom, seed, 260, desc_stride=48 if W == 131 else 32)
    try:
        exp0 = rig.expected(0, 1.0)
        for f in range(F):          # what the frame content promises
            k, m = exp0[f]
            if KINDS[f % 5] == "constant":
                assert not m.any() and not k["orient"].any()
            if KINDS[f % 5] == "ramp":
                assert not m[:, 0].any()
            if KINDS[f % 5] == "mirrored" and W % 2 and len(k) > 4:
                assert (m[k["x"] == W // 2, 1] == 0).all() and (k["x"] == W // 2).any()
        rig.keypoints(0, 1.0)
        rig.check_keypoints("level 0", exp0)
        rig.describe(1.0)
        first = rig.check_desc("level 0", [k for k, _ in exp0], 1.0, seed)
        rig.ar.refill(rig.d_desc)
        rig.describe(1.0)
        assert (rig.check_desc("level 0, again", [k for k, _ in exp0], 1.0, seed) == first).all()
        rig.refill()
        exp1 = rig.expected(1, SCALE1)
        rig.keypoints(1, SCALE1, moments=False)
        rig.check_keypoints("level 1, no moments", exp1, moments=False)
        rig.describe(SCALE1)
        rig.check_desc("level 1", [k for k, _ in exp1], SCALE1, seed)
        rig.refill()
        small = 40
        rig.keypoints(0, 1.0, key_cap=small)
        rig.check_keypoints("cap %d" % small, exp0, key_cap=small)
        rig.refill()
        rig.keypoints(0, 1.0, key_cap=0)
        rig.check_keypoints("counts only", exp0, key_cap=0)
    finally:
        rig.close()


def brief_timing(rig, brief_name):
    """brief_name: None, or the timing entry the plan's next describe call has to stamp for its orb_brief_kernel variant (checked by brief_stamped)"""
    if brief_name is not None:
        rig.plan.set_timing(1)


def brief_stamped(rig, brief_name, blur=True):
    if brief_name is not None:
        assert [n for n, _ in rig.plan.get_timing()] == (["convlt_fxp_kernels"] if blur else []) + [brief_name]


def single_admissible_position_case(hip_ctx, brief_name=None):
    AX, AY, BX, BY = om.pattern()
    c, s, _ = om.canonical_cos_sin(np.array([45.0], np.float32))
    reach = [np.rint(P * c - Q * s) for P, Q in ((AX, AY), (BX, BY))] + [np.rint(P * s + Q * c) for P, Q in ((AX, AY), (BX, BY))]
    assert min(r.min() for r in reach) == -18
    geom = GEOMETRIES[0]
    W, H, S, F = geom
    rig = Rig(hip_ctx, geom, W + H, 8)
    try:
        keys = np.zeros(len(om.FIXED_ORIENTS) + 1, om.KEYPOINT_DTYPE)
        keys["x"], keys["y"], keys["orient"], keys["size"] = 18, 18, om.FIXED_ORIENTS + (360.0,), 31
        host = np.zeros((F, 8), om.KEYPOINT_DTYPE)
        host[:] = keys
        rig.d_keys.copy_(rig.ar.torch.from_numpy(u8(host)))
        rig.d_kcounts.copy_(rig.ar.torch.from_numpy(u8(np.array([8, 5], np.int32))))
        brief_timing(rig, brief_name)
        rig.describe(1.0)
        brief_stamped(rig, brief_name)
        rows = rig.check_desc("fixed orientations", [keys, keys[:5]], 1.0, W + H)
        assert (rows[0, 0, :32] == rows[0, 7, :32]).all() and rows[0, 0, :32].any()          # 0 and 360 degrees
        assert (rows[0, 1, :32] != rows[0, 0, :32]).any()
    finally:
        rig.close()


def test_single_admissible_position_reads_the_zero_blur_border(hip_ctx):
    """37 x 37: the only keypoint is (18, 18); turned by 45 degrees its pattern reaches row and column 0 of the blurred plane, which the blur leaves zero"""
    single_admissible_position_case(hip_ctx)


def callers_keypoints_case(hip_ctx, brief_name=None):
    import torch
    geom = GEOMETRIES[2]
    W, H, S, F = geom
    seed = W + H
    cap = 24
    rig = Rig(hip_ctx, geom, seed, cap)
    try:
        rng = np.random.default_rng(99)
        host = np.zeros((F, cap), om.KEYPOINT_DTYPE)
        counts = np.array([cap, cap + 9, 0, -3, 11], np.int32)
        sfi = np.float32(1) / SCALE1
        for f in range(F):
            k = host[f]
            k["x"] = (rng.integers(18, int(W * 0.83) - 18, cap) + rng.random(cap)).astype(np.float32) * sfi          # non-integer, in level-0 units
            k["y"] = (rng.integers(18, int(H * 0.83) - 18, cap) + rng.random(cap)).astype(np.float32) * sfi
            k["orient"] = (rng.random(cap) * 360).astype(np.float32)
            k["orient"][:8] = om.FIXED_ORIENTS + (360.0,)
            k["level"], k["size"] = 1, np.float32(31) / SCALE1
            k["x"][9] = np.float32(17.4) * sfi          # rounds to 17: inside the margin
            k["y"][10] = np.float32(H) * sfi
            k["x"][12], k["y"][13], k["x"][14] = np.nan, np.inf, -3e9
        rig.d_keys.copy_(torch.from_numpy(u8(host)))
        rig.d_kcounts.copy_(torch.from_numpy(u8(counts)))
        used = [host[f, :min(max(int(counts[f]), 0), cap)] for f in range(F)]
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        brief_timing(rig, brief_name)
        rig.describe(SCALE1, stream=st.cuda_stream)
        st.synchronize()
        brief_stamped(rig, brief_name)
        rows = rig.check_desc("caller's keypoints", used, SCALE1, seed)
        zero = (9, 10, 12, 13, 14)
        assert not rows[0, zero, :32].any() and rows[0, [q for q in range(cap) if q not in zero], :32].any(axis=1).all()
        pre = pad_frames(blurred_batch(W, H, F, seed), S, np.random.default_rng(5))
        d_pre = rig.ar.new(pre.size, pre)
        rig.ar.keep(d_pre, pre)
        rig.ar.refill(rig.d_desc)
        rig.describe(SCALE1, blur=False, d_gray=d_pre)
        brief_stamped(rig, brief_name, blur=False)
        assert (rig.check_desc("pre-blurred", used, SCALE1, seed) == rows).all()
    finally:
        rig.close()


def test_describe_callers_keypoints(hip_ctx):
    """fixed orientations and 360.0, non-integer coordinates at scale 0.83, points inside the 18-pixel margin or holding no number (a zero row each, in
    place), a count above keyCap; blur = 0 on a pre-blurred plane equals blur = 1 on the raw one; a non-default stream"""
    callers_keypoints_case(hip_ctx)


# ---- orb_brief_kernel<false>: COMPVHIP_ORB_BRIEF=global (read when a plan first describes) makes the tests' bytes come straight from the blurred plane
GLOBAL_NAME = "orb_brief_kernel_global"


@pytest.mark.parametrize("geom", (GEOMETRIES[0], GEOMETRIES[2], GEOMETRIES[3]), ids=GID)
def test_global_byte_variant_geometries(hip_ctx, monkeypatch, geom):
    """keypoints and descriptor rows of level 0 and level 1 as in test_orb_geometry_sweep, the rows made by the global-byte variant"""
    monkeypatch.setenv("COMPVHIP_ORB_BRIEF", "global")
    W, H, S, F = geom
    seed = W + H
    rig = Rig(hip_ctx, geom, seed, 260, desc_stride=48 if W == 131 else 32)
    try:
        for level, scale in ((0, 1.0), (1, SCALE1)):
            exp = rig.expected(level, scale)
            rig.plan.set_timing(0)
            rig.keypoints(level, scale)
            rig.check_keypoints("level %d" % level, exp)
            brief_timing(rig, GLOBAL_NAME)
            rig.describe(scale)
            brief_stamped(rig, GLOBAL_NAME)
            rig.check_desc("level %d, global bytes" % level, [k for k, _ in exp], scale, seed)
            rig.refill()
    finally:
        rig.close()


def test_global_byte_variant_reads_the_zero_blur_border(hip_ctx, monkeypatch):
    """the single position of 37 x 37 at fixed orientations: this variant reads row and column 0 of the blurred plane straight from memory"""
    monkeypatch.setenv("COMPVHIP_ORB_BRIEF", "global")
    single_admissible_position_case(hip_ctx, GLOBAL_NAME)


def test_global_byte_variant_on_callers_keypoints(hip_ctx, monkeypatch):
    """NaN, inf and in-margin points: in this variant the `inside` flag alone keeps the loads in the plane"""
    monkeypatch.setenv("COMPVHIP_ORB_BRIEF", "global")
    callers_keypoints_case(hip_ctx, GLOBAL_NAME)


@pytest.mark.parametrize("value", [None, "lds"], ids=["unset", "lds"])
def test_the_default_variant_keeps_its_timing_name(hip_ctx, monkeypatch, value):
    if value is None:
        monkeypatch.delenv("COMPVHIP_ORB_BRIEF", raising=False)
    else:
        monkeypatch.setenv("COMPVHIP_ORB_BRIEF", value)
    single_admissible_position_case(hip_ctx, "orb_brief_kernel")


def test_streams_scratch_and_timing(hip_ctx):
    """both calls on a non-default stream; the plan's scratch -- the index list, then the blurred batch -- is allocated on first use, grows with keyCap only, is
    counted by compvhip_live_allocations and released with the plan; the timing entries carry the kernels' names"""
    import torch
    torch.cuda.synchronize()
    start = hip_ctx.live_allocations()
    geom = GEOMETRIES[1]
    W, H, S, F = geom
    seed = W + H
    rig = Rig(hip_ctx, geom, seed, 260)
    try:
        exp = rig.expected(0, 1.0)
        base = hip_ctx.live_allocations()
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        rig.plan.set_timing(1)
        rig.keypoints(0, 1.0, stream=st.cuda_stream)
        assert [n for n, _ in rig.plan.get_timing()] == ["orb_select_kernel", "orb_orient_kernel"]
        assert hip_ctx.live_allocations() == base + 1
        rig.describe(1.0, stream=st.cuda_stream)
        assert [n for n, _ in rig.plan.get_timing()] == ["convlt_fxp_kernels", "orb_brief_kernel"]
        assert hip_ctx.live_allocations() == base + 2
        st.synchronize()
        rig.check_keypoints("on a stream", exp)
        rig.check_desc("on a stream", [k for k, _ in exp], 1.0, seed)
        rig.refill()
        rig.keypoints(0, 1.0, moments=False)
        rig.describe(1.0, blur=False)
        assert [n for n, _ in rig.plan.get_timing()] == ["orb_brief_kernel"]
        assert hip_ctx.live_allocations() == base + 2
        torch.cuda.synchronize()
    finally:
        rig.close()
    assert hip_ctx.live_allocations() == start


def test_refusals(hip_ctx):
    from compv_amd import capi

    def code(fn, *a, **k):
        with pytest.raises(capi.CompvHipError) as e:
            fn(*a, **k)
        return e.value.code
    ar = Arena()
    d = ar.new(2 * 40 * 40)
    d_rec = ar.new(4096)
    d_counts = ar.new(16)
    small = capi.Plan(hip_ctx, 36, 40, 40, 1)
    low = capi.Plan(hip_ctx, 40, 36, 40, 1)
    plan = capi.Plan(hip_ctx, 40, 40, 40, 2)
    g, r, c = ptr(d), ptr(d_rec), ptr(d_counts)
    bad = capi.E_INVALID_PARAMETER
    try:
        for p in (small, low):
            assert code(p.orb_keypoints, g, r, 4, c, 0, 1.0, r + 1024, 4, c + 8) == bad          # W or H < 37
            assert code(p.orb_describe, g, r, 4, c, 1.0, r + 1024) == bad
        for scale in (0.0, -1.0, float("nan")):
            assert code(plan.orb_keypoints, g, r, 4, c, 0, scale, r + 1024, 4, c + 8) == bad
            assert code(plan.orb_describe, g, r, 4, c, scale, r + 1024) == bad
        assert code(plan.orb_keypoints, 0, r, 4, c, 0, 1.0, r + 1024, 4, c + 8) == bad
        assert code(plan.orb_keypoints, g, 0, 4, c, 0, 1.0, r + 1024, 4, c + 8) == bad
        assert code(plan.orb_keypoints, g, r, 4, 0, 0, 1.0, r + 1024, 4, c + 8) == bad
        assert code(plan.orb_keypoints, g, r, 4, c, 0, 1.0, 0, 4, c + 8) == bad          # a capacity without a buffer
        assert code(plan.orb_keypoints, g, r, 4, c, 0, 1.0, r + 1024, 4, 0) == bad
        assert code(plan.orb_keypoints, g, r + 2, 4, c, 0, 1.0, r + 1024, 4, c + 8) == bad          # misaligned records, counts, moments, frames
        assert code(plan.orb_keypoints, g, r, 4, c + 1, 0, 1.0, r + 1024, 4, c + 8) == bad
        assert code(plan.orb_keypoints, g, r, 4, c, 0, 1.0, r + 1026, 4, c + 8) == bad
        assert code(plan.orb_keypoints, g, r, 4, c, 0, 1.0, r + 1024, 4, c + 8, r + 2049) == bad
        assert code(plan.orb_keypoints, g + 2, r, 4, c, 0, 1.0, r + 1024, 4, c + 8) == bad
        assert code(plan.orb_describe, g, r, 4, c, 1.0, 0) == bad          # no descriptor buffer
        assert code(plan.orb_describe, g, 0, 4, c, 1.0, r + 1024) == bad
        assert code(plan.orb_describe, g, r, 4, 0, 1.0, r + 1024) == bad
        assert code(plan.orb_describe, g, r, 0, c, 1.0, r + 1024) == bad
        for stride in (0, 28, 31, 34, 33):
            assert code(plan.orb_describe, g, r, 4, c, 1.0, r + 1024, stride) == bad
        assert code(plan.orb_describe, g, r, 4, c, 1.0, r + 1026) == bad
        assert code(plan.orb_describe, g + 1, r, 4, c, 1.0, r + 1024) == bad
        img = np.zeros((40, 40), np.uint8)
        corners = np.zeros(3, capi.CORNER_DTYPE)
        assert code(hip_ctx.orb, img[:36], corners) == bad
        assert code(hip_ctx.orb, img[:, :36], corners) == bad
        assert code(hip_ctx.orb, img, corners, 0, 0.0) == bad
        ar.check("refusals")
        for b in (d, d_rec, d_counts):
            assert (b.cpu().numpy() == SENTINEL).all()
    finally:
        for p in (small, low, plan):
            p.close()


def test_host_form_agrees_with_the_model(hip_ctx):
    W, H = 131, 70
    store = np.zeros((H, 160), np.uint8)
    store[:] = 0xEE
    view = store[:, :W]
    view[:] = fm.blocks(W, H, 4)
    for level, scale in ((0, 1.0), (2, 0.6889)):
        for survivors in (0, 1, 65):
            corners = corner_list(W, H, survivors, 50 + survivors)
            keys, desc = hip_ctx.orb(view, corners, level, scale)
            exp_k, _ = om.keypoints(view, corners, level, np.float32(scale))
            assert keys.tobytes() == exp_k.tobytes() and len(keys) == survivors
            assert desc.tobytes() == om.describe(om.blur(view), exp_k, np.float32(scale)).tobytes()
    keys, desc = hip_ctx.orb(view, np.zeros(0, om.CORNER_DTYPE))
    assert len(keys) == 0 and desc.shape == (0, 32)
    assert (store[:, W:] == 0xEE).all()


def test_chain_fast_orb_match_on_one_stream(hip_ctx):
    """fast -> orb_keypoints -> orb_describe -> matcher_knn enqueued on one stream, every count read from device memory, no host synchronisation in between; the
    pair is an image and its np.rot90.  Records equal the model chain's."""
    import torch
    from compv_amd import capi
    W = H = S = 96
    F, cap, t = 2, 512, 30
    img = fm.blocks(W, H, 11)
    frames = np.stack([img, np.ascontiguousarray(np.rot90(img))])
    ar = Arena()
    d_in = ar.new(frames.size, frames)
    ar.keep(d_in, frames)
    d_corners, d_ccounts = ar.new(F * cap * CREC), ar.new(4 * F)
    d_keys, d_kcounts, d_desc = ar.new(F * cap * KREC), ar.new(4 * F), ar.new(F * cap * 32)
    d_matches = ar.new(2 * cap * 16)
    plan = capi.Plan(hip_ctx, W, H, S, F)
    matcher = capi.Matcher(hip_ctx, 32, cap, cap, 1, 2)
    try:
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        s = st.cuda_stream
        plan.fast(ptr(d_in), t, 9, True, -1, 0, ptr(d_corners), cap, ptr(d_ccounts), s)
        plan.orb_keypoints(ptr(d_in), ptr(d_corners), cap, ptr(d_ccounts), 0, 1.0, ptr(d_keys), cap, ptr(d_kcounts), 0, s)
        plan.orb_describe(ptr(d_in), ptr(d_keys), cap, ptr(d_kcounts), 1.0, ptr(d_desc), 32, True, s)
        matcher.knn(ptr(d_desc), 32, ptr(d_kcounts), ptr(d_desc) + cap * 32, 32, ptr(d_kcounts) + 4, False, ptr(d_matches), s)
        st.synchronize()
        ar.check("chain")
        exp_k = [om.keypoints(frames[f], fm.fast(frames[f], t, 9, True)[0], 0, 1.0)[0] for f in range(F)]
        exp_d = [om.describe(om.blur(frames[f]), exp_k[f], 1.0) for f in range(F)]
        n0, n1 = len(exp_k[0]), len(exp_k[1])
        assert 8 <= n0 <= cap and 8 <= n1 <= cap
        assert np.frombuffer(d_kcounts.cpu().numpy().tobytes(), np.int32).tolist() == [n0, n1]
        keys = d_keys.cpu().numpy().tobytes()
        desc = d_desc.cpu().numpy().reshape(F, cap, 32)
        for f in range(F):
            assert keys[f * cap * KREC:f * cap * KREC + len(exp_k[f]) * KREC] == exp_k[f].tobytes()
            assert desc[f, :len(exp_d[f])].tobytes() == exp_d[f].tobytes() and (desc[f, len(exp_d[f]):] == SENTINEL).all()
        got = np.frombuffer(d_matches.cpu().numpy().tobytes(), mm.MATCH_DTYPE).reshape(2, cap)
        exp_m = mm.knn_device(exp_d[0], exp_d[1], 2)
        assert got[:, :n0].tobytes() == exp_m.tobytes()
        # the rotation is found: most keypoints' nearest neighbour is their own rotated position
        x0, y0 = exp_k[0]["x"], exp_k[0]["y"]
        t1 = exp_k[1][got[0, :n0]["trainIdx"]]
        assert np.mean((t1["x"] == y0) & (t1["y"] == W - 1 - x0)) > 0.5
    finally:
        matcher.close()
        plan.close()
