"""GPU lens undistortion (compvhip_undistort_*) against the fixture the compiled reference made (tests/golden/golden_undistort.*) and
tests/undistort_model.py, bit for bit: nothing here is compared with a tolerance.

Harness of tests/gpu_support.py: every device buffer sits between two guards; a destination starts filled with a sentinel and is compared as a
WHOLE with the expected bytes, so stride padding, bytes behind Wout, points behind a count and every refused call must leave the sentinel.

The fused form is the remap tile (256 x 4, a lane 4 pixels, vector stores where pointer, stride and frame size allow it, 8 frames per workgroup for a
shared camera); shapes come from those numbers (tests/undistort_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import undistort_cases as uc
import undistort_model as um
from fixtures import load_golden, md5
from gpu_support import SENTINEL, Arena, ptr, u8
from undistort_rig import F32_OUT, Rig, layouts, maps_of, model_image, padded_frames, point_rig

pytestmark = pytest.mark.gpu

LIMIT = 65535             # kMaxFramesPerLaunch


@pytest.fixture(scope="module")
def golden():
    return load_golden("golden_undistort")


@pytest.mark.parametrize("c", uc.image_cases(), ids=lambda c: c["id"])
def test_fused_cases_against_the_model_and_the_fixture(hip_ctx, golden, c):
    rec = next(r for r in golden[0]["images"] if r["id"] == c["id"])
    rig = Rig(hip_ctx, c)
    try:
        for interp in um.INTERPS:
            exp = model_image(c, interp)
            assert md5(exp) == rec["md5"][um.INTERP_NAMES[interp]]
            for name, Sout, off in layouts(c["size"][2], interp):
                rig.run(interp, c["K"], c["d"], Sout, off)
                rig.check("%s %s %s" % (c["id"], um.INTERP_NAMES[interp], name), [exp], Sout, off)
    finally:
        rig.close()


def test_nine_frames_share_a_camera(hip_ctx):
    """one full group of 8 frames and a tail of one: the coordinates are worked out once per group"""
    c = uc.case("pin61")
    rig = Rig(hip_ctx, c, 9)
    try:
        for interp in um.INTERPS:
            planes = [model_image(c, interp, k) for k in range(9)]
            assert len({p.tobytes() for p in planes}) == 9
            for name, Sout, off in layouts(61, interp):
                rig.run(interp, c["K"], c["d"], Sout, off)
                rig.check("9 frames %s %s" % (um.INTERP_NAMES[interp], name), planes, Sout, off)
    finally:
        rig.close()


@pytest.mark.parametrize("cid", ["pin40", "pin61"])
def test_three_frames_with_three_cameras(hip_ctx, cid):
    c = uc.case(cid)
    K, d = uc.cameras_for_frames(c, 3)
    K, d = K.astype(np.float32), d.astype(np.float32)
    rig = Rig(hip_ctx, c, 3)
    try:
        for interp in um.INTERPS:
            planes = [model_image(c, interp, k, K[k], d[k]) for k in range(3)]
            assert planes[0].tobytes() != model_image(c, interp, 0, K[1], d[1]).tobytes()          # the cameras differ in what they give
            for name, Sout, off in layouts(c["size"][2], interp):
                rig.run(interp, K, d, Sout, off)
                rig.check("3 cameras %s %s %s" % (cid, um.INTERP_NAMES[interp], name), planes, Sout, off)
    finally:
        rig.close()


@pytest.mark.parametrize("c", uc.image_cases(), ids=lambda c: c["id"])
def test_device_maps_are_the_fixtures_bytes(hip_ctx, golden, c):
    meta, arrays = golden
    rec = next(r for r in meta["images"] if r["id"] == c["id"])
    rig = Rig(hip_ctx, c)
    try:
        for T, offsets in ((np.float32, (0, 4)), (np.float64, (0, 8))):          # 16-byte aligned planes take vector stores where Wout % 4 == 0; the others never
            for off in offsets:
                x, y, _, _ = maps_of(rig, c["K"], c["d"], 1, T, rig.ar, off)
                if T is np.float32:
                    assert x.tobytes() == arrays["mapx_" + c["id"]].tobytes() and y.tobytes() == arrays["mapy_" + c["id"]].tobytes(), off
                else:
                    assert (md5(x), md5(y)) == (rec["md5"]["mapx_f64"], rec["md5"]["mapy_f64"]), off
    finally:
        rig.close()


def test_device_maps_of_three_cameras(hip_ctx):
    c = uc.case("pin40")
    K, d = uc.cameras_for_frames(c, 3)
    rig = Rig(hip_ctx, c, 3)
    try:
        for T in (np.float32, np.float64):
            x, y, _, _ = maps_of(rig, K, d, 3, T, rig.ar)
            ex, ey = zip(*[um.map_planes(K[k].astype(T), d[k].astype(T), 40, 40, dtype=T) for k in range(3)])
            assert x.tobytes() == np.stack(ex).tobytes() and y.tobytes() == np.stack(ey).tobytes()
    finally:
        rig.close()


@pytest.mark.parametrize("cid,count", [("pin61", 9), ("pin40", 3), ("window", 1), ("roi203", 1)])
def test_device_maps_fed_to_the_remap_equal_the_fused_form(hip_ctx, cid, count):
    """compvhip_undistort_maps (float32) -> compvhip_plan_remap, against compvhip_undistort_frames: byte for byte, for all five interpolations"""
    from compv_amd import capi
    c = uc.case(cid)
    w, h, wo, ho = c["size"]
    shared = cid != "pin40"
    K, d = (np.asarray(c["K"]), np.asarray(c["d"])) if shared else uc.cameras_for_frames(c, count)
    rig = Rig(hip_ctx, c, count, pad=(-w) % 8 + 8)          # a plan's stride is a multiple of 8
    plan = capi.Plan(hip_ctx, w, h, rig.S, count)
    try:
        _, _, dx, dy = maps_of(rig, K, d, 1 if shared else count, np.float32, rig.ar)
        for interp in um.INTERPS:
            Sout = wo + 4
            item = 4 if interp in F32_OUT else 1
            d_remap = rig.ar.new(count * ho * Sout * item)
            plan.remap(ptr(rig.d_in), ptr(dx), ptr(dy), 1 if shared else count, interp, ptr(d_remap), wo, ho, Sout, c["roi"], c["default"])
            rig.run(interp, K, d, Sout)
            rig.ar.check("remap and fused %s" % um.INTERP_NAMES[interp])
            got = rig.d_out.cpu().numpy()[:d_remap.numel()]
            assert got.tobytes() == d_remap.cpu().numpy().tobytes(), um.INTERP_NAMES[interp]
            assert (got != SENTINEL).any()
    finally:
        plan.close()
        rig.close()


@pytest.mark.parametrize("c", uc.point_cases(), ids=lambda c: c["id"])
def test_points_against_the_fixture(hip_ctx, golden, c):
    from compv_amd import capi
    T, n = c["dtype"], c["n"]
    cam = uc.case(c["camera"])
    pts, exp = uc.points(c), golden[1][c["id"]]
    ptype = capi.UNDISTORT_F32 if T is np.float32 else capi.UNDISTORT_F64
    rig = point_rig(hip_ctx, 3, 200)
    try:
        ar = rig.ar
        d_in = ar.new(pts.nbytes, u8(pts))
        ar.keep(d_in, u8(pts))
        d_out = ar.new(pts.nbytes)
        rig.h.points(cam["K"], cam["d"], ptr(d_in), 1, n, ptr(d_out), ptype)
        ar.check(c["id"])
        assert d_out.cpu().numpy().tobytes() == exp.tobytes()
        # a count shorter than n: the points behind it are neither read nor written
        short = max(n - 3, 0)
        d_cnt = ar.new(4, u8(np.array([short], np.int32)))
        ar.refill(d_out)
        rig.h.points(cam["K"], cam["d"], ptr(d_in), 1, n, ptr(d_out), ptype, ptr(d_cnt))
        ar.check(c["id"] + " short")
        got = np.frombuffer(d_out.cpu().numpy().tobytes(), T).reshape(n, 2)
        assert got[:short].tobytes() == exp[:short].tobytes() and (u8(got[short:]) == SENTINEL).all()
    finally:
        rig.close()


def test_point_sets_with_a_camera_each_counts_and_in_place(hip_ctx):
    from compv_amd import capi
    c = uc.case("pin61")
    K, d = uc.cameras_for_frames(c, 3)
    rig = point_rig(hip_ctx, 3, 65)
    try:
        ar = rig.ar
        for T, ptype in ((np.float32, capi.UNDISTORT_F32), (np.float64, capi.UNDISTORT_F64)):
            pts = np.random.default_rng(9).uniform(-3, 64, (3, 65, 2)).astype(T)
            counts = np.array([65, 0, 17], np.int32)
            exp = pts.copy()
            for s in range(3):
                exp[s, :counts[s]] = um.dist_points(K[s].astype(T), d[s].astype(T), pts[s, :counts[s]], T)
            d_pts = ar.new(pts.nbytes, u8(pts))          # in place: d_in == d_out
            d_cnt = ar.new(12, u8(counts))
            ar.keep(d_cnt, u8(counts))
            rig.h.points(K, d, ptr(d_pts), 3, 65, ptr(d_pts), ptype, ptr(d_cnt))
            ar.check("sets in place")
            assert d_pts.cpu().numpy().tobytes() == exp.tobytes()
            assert exp[0].tobytes() != pts[0].tobytes()
    finally:
        rig.close()


@pytest.mark.parametrize("c", uc.proj_cases(), ids=lambda c: c["id"])
def test_projection_against_the_fixture(hip_ctx, golden, c):
    cam = uc.case(c["camera"])
    pts, exp, n = uc.proj_points(c), golden[1][c["id"]], c["n"]
    pose = np.concatenate([np.asarray(c["R"], np.float64).ravel(), np.asarray(c["t"], np.float64)])
    other = uc.proj_cases()[1 if c["id"] == "proj_z0" else 0]
    rig = point_rig(hip_ctx, 2, 80)
    try:
        ar = rig.ar
        d_in = ar.new(pts.nbytes, u8(pts))
        ar.keep(d_in, u8(pts))
        d_out = ar.new(n * 16)
        rig.h.project(cam["K"], cam["d"], pose[None], ptr(d_in), 1, n, ptr(d_out))
        ar.check(c["id"])
        assert d_out.cpu().numpy().tobytes() == exp.tobytes()
        # two sets, a camera and a pose each, the second cut short by its count
        cam2 = uc.case(other["camera"])
        pose2 = np.concatenate([np.asarray(other["R"], np.float64).ravel(), np.asarray(other["t"], np.float64)])
        pts2 = uc.proj_points(other)[:n] if other["n"] >= n else np.concatenate([uc.proj_points(other)] * 2)[:n]
        both = np.stack([pts, pts2])
        K2 = np.stack([np.asarray(cam["K"], np.float64), np.asarray(cam2["K"], np.float64)])
        nd = min(len(cam["d"]), len(cam2["d"]))
        d2 = np.stack([np.asarray(cam["d"][:nd], np.float64), np.asarray(cam2["d"][:nd], np.float64)])
        counts = np.array([n, 5], np.int32)
        d_both, d_cnt, d_out2 = ar.new(both.nbytes, u8(both)), ar.new(8, u8(counts)), ar.new(2 * n * 16)
        rig.h.project(K2, d2, np.stack([pose, pose2]), ptr(d_both), 2, n, ptr(d_out2), ptr(d_cnt))
        ar.check(c["id"] + " two sets")
        got = np.frombuffer(d_out2.cpu().numpy().tobytes(), np.float64).reshape(2, n, 2)
        assert got[0].tobytes() == um.proj2d(K2[0], d2[0], pose[:9], pose[9:], pts).tobytes()
        assert got[1, :5].tobytes() == um.proj2d(K2[1], d2[1], pose2[:9], pose2[9:], pts2[:5]).tobytes() and (u8(got[1, 5:]) == SENTINEL).all()
    finally:
        rig.close()


def test_one_handle_across_changing_cameras_and_content(hip_ctx):
    """nothing is carried from call to call: the expectation of every call is the model on that call's own frames and cameras.  More calls than the
    staging ring has slots, shared and per-frame cameras in turn."""
    c = uc.case("pin61")
    Ks, ds = uc.cameras_for_frames(c, 7)
    Ks, ds = Ks.astype(np.float32), ds.astype(np.float32)
    rig = Rig(hip_ctx, c, 3)
    try:
        for turn in range(7):
            interp = um.INTERPS[turn % 5]
            src = padded_frames(c, 3, rig.S, seed=40 + turn)
            for k in range(3):
                src[k, :, :61] = uc.frame(c, 3 * turn + k)
            rig.ar.reload(rig.d_in, src)
            if turn % 2:
                sel = [(turn + k) % 7 for k in range(3)]
                K, d = Ks[sel], ds[sel]
                planes = [um.undistort(src[k, :, :61], K[k], d[k], interp=interp, default=turn) for k in range(3)]
            else:
                K, d = Ks[turn].copy(), ds[turn].copy()
                planes = [um.undistort(src[k, :, :61], K, d, interp=interp, default=turn) for k in range(3)]
            rig.run(interp, K, d, 64, roi=None, default=turn)
            K[...] = 0          # the caller's arrays are free when the call returns
            rig.check("turn %d" % turn, planes, 64)
    finally:
        rig.close()


def test_behind_pending_work_on_the_handles_stream(hip_ctx):
    """a handle created on a side stream: the frames reach the device on that stream behind a delay, the call follows on it and returns at once"""
    import torch
    c = uc.case("pin61")
    side = torch.cuda.Stream()
    rig = Rig(hip_ctx, c, 9, stream=side.cuda_stream)
    try:
        host = torch.from_numpy(u8(rig.src).copy()).pin_memory()
        for turn, interp in enumerate((1, 4)):
            rig.d_in.fill_(SENTINEL)
            rig.ar.refill(rig.d_out)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                torch.cuda._sleep(20_000_000)          # a few milliseconds of pending work in front of the copy
                rig.d_in.copy_(host, non_blocking=True)
            rig.h.undistort(ptr(rig.d_in), c["K"], c["d"], interp, ptr(rig.d_out), 64, None, c["default"])
            side.synchronize()
            rig.check("behind pending work %d" % turn, [model_image(c, interp, k) for k in range(9)], 64)
    finally:
        rig.close()


def test_host_form_and_timing_entries(hip_ctx):
    from compv_amd import capi
    for cid in ("pin61", "window", "one"):
        c = uc.case(cid)
        wo, ho = c["size"][2:]
        for interp in um.INTERPS:
            got = hip_ctx.undistort(uc.frame(c), c["K"], c["d"], wo, ho, *c["origin"], interp=interp, roi=c["roi"], default=c["default"])
            exp = model_image(c, interp)
            assert got.dtype == exp.dtype and got.tobytes() == exp.tobytes(), (cid, interp)
    c = uc.case("pin40")
    rig = Rig(hip_ctx, c, max_sets=1, max_points=8)
    try:
        rig.h.set_timing(1)
        rig.run(1, c["K"], c["d"], 44)
        assert [n for n, _ in rig.h.get_timing()] == ["undistort_kernel"]
        maps_of(rig, c["K"], c["d"], 1, np.float32, rig.ar)
        assert [n for n, _ in rig.h.get_timing()] == ["undist_map_kernel"]
        pts = np.zeros((8, 2), np.float64)
        d_p, d_q = rig.ar.new(pts.nbytes, u8(pts)), rig.ar.new(8 * 24, u8(np.ones((8, 3))))
        rig.h.points(c["K"], c["d"], ptr(d_p), 1, 8, ptr(d_p), capi.UNDISTORT_F64)
        t = rig.h.get_timing()
        assert [n for n, _ in t] == ["undist_points_kernel"] and all(ms >= 0 for _, ms in t)
        rig.h.project(c["K"], c["d"], np.concatenate([np.eye(3).ravel(), [0, 0, 1.0]])[None], ptr(d_q), 1, 8, ptr(d_p))
        assert [n for n, _ in rig.h.get_timing()] == ["undist_project_kernel"]
    finally:
        rig.close()


def test_allocations_are_made_at_creation_and_returned(hip_ctx):
    c = uc.case("pin40")
    start = hip_ctx.live_allocations()
    rig = Rig(hip_ctx, c, 3, max_sets=2, max_points=16)
    try:
        made = hip_ctx.live_allocations()
        assert made > start
        K, d = uc.cameras_for_frames(c, 3)
        for interp in (0, 5):
            rig.run(interp, K.astype(np.float32), d.astype(np.float32), 44)
            maps_of(rig, K, d, 3, np.float64, Arena())
            assert hip_ctx.live_allocations() == made          # no later call allocates
    finally:
        rig.close()
    assert hip_ctx.live_allocations() == start


# ---------------------------------------------------------------------------------------------------------------
# batches beyond the slicing bound: 4 x 2-pixel frames
# ---------------------------------------------------------------------------------------------------------------
SMALL = {"id": "small", "size": (4, 2, 4, 2), "origin": (0, 0), "K": [[3.5, 0.05, 1.5], [0.0, 3.25, 0.5], [0.0, 0.0, 1.0]], "d": (-0.2, 0.05, 0.01, 0.02), "roi": None, "default": 3}
CONTENT, PARAM = 7, 11


def small_frames():
    return np.stack([np.random.default_rng(990 + k).integers(0, 256, (2, 4), dtype=np.uint8) for k in range(CONTENT)])


def small_cameras(n):
    """n float32 cameras around SMALL's, close enough that most of the 8 pixels stay inside"""
    K, d = np.repeat(np.asarray(SMALL["K"])[None], n, axis=0), np.repeat(np.asarray(SMALL["d"])[None], n, axis=0)
    for k in range(n):
        K[k, 0, 0] *= 1 + 0.02 * k
        K[k, 0, 2] += 0.04 * k
        K[k, 1, 2] -= 0.02 * k
        d[k, 0] *= 1 - 0.05 * k
    return K.astype(np.float32), d.astype(np.float32)


def check_cycle(body, table, lin, what):
    """body: device bytes [F][n]; frame f must hold table[lin[f]].  Compared on the device; the first wrong frame is named."""
    import torch
    F, n = lin.numel(), table.shape[1]
    exp = torch.from_numpy(np.ascontiguousarray(table)).to(body.device)[lin]
    got = body.view(F, n)
    if torch.equal(got, exp):
        return
    f = int((got != exp).any(dim=1).nonzero()[0])
    raise AssertionError("%s: frame %d (slice %d) differs: got %s, expected %s" % (what, f, f // LIMIT, got[f].tolist(), exp[f].tolist()))


def test_a_shared_camera_beyond_65535_groups_of_8(hip_ctx):
    """8 * 65 535 + 5 frames: the second slice is one ragged group of 5.  Frame f holds content f % 7; 8 * 65 535 is no multiple of 7, so a slice that
    started at frame 0 again would show."""
    import torch
    from compv_amd import capi
    F = 8 * LIMIT + 5
    assert (8 * LIMIT) % CONTENT != 0
    frames = small_frames()
    ar = Arena()
    host = frames[np.arange(F) % CONTENT]
    d_in = ar.new(host.size, u8(host))
    lin = torch.arange(F, device=d_in.device) % CONTENT
    h = capi.Undistort(hip_ctx, 4, 2, 4, F)
    try:
        for interp in um.INTERPS:
            item = 4 if interp in F32_OUT else 1
            table = np.stack([u8(um.undistort(f, SMALL["K"], SMALL["d"], interp=interp, default=3)) for f in frames])
            assert table[(8 * LIMIT) % CONTENT].tobytes() != table[0].tobytes()          # the first frame of the second slice differs from frame 0
            d_out = ar.new(F * 8 * item)
            h.undistort(ptr(d_in), SMALL["K"], SMALL["d"], interp, ptr(d_out), 4, None, 3)
            ar.check("shared camera, %s" % um.INTERP_NAMES[interp])
            check_cycle(d_out, table, lin, "shared camera, %s" % um.INTERP_NAMES[interp])
    finally:
        h.close()


def test_a_camera_per_frame_beyond_65535_frames(hip_ctx):
    """65 541 frames, frame f (content f % 7) through camera f % 11: the record offset of the later slice"""
    import torch
    from compv_amd import capi
    F = LIMIT + 6
    assert LIMIT % CONTENT and LIMIT % PARAM
    frames = small_frames()
    Ks, ds = small_cameras(PARAM)
    ar = Arena()
    host = frames[np.arange(F) % CONTENT]
    d_in = ar.new(host.size, u8(host))
    f = torch.arange(F, device=d_in.device)
    lin = (f % CONTENT) * PARAM + f % PARAM
    K, d = np.ascontiguousarray(Ks[np.arange(F) % PARAM]), np.ascontiguousarray(ds[np.arange(F) % PARAM])
    h = capi.Undistort(hip_ctx, 4, 2, 4, F)
    try:
        for interp in um.INTERPS:
            item = 4 if interp in F32_OUT else 1
            table = np.stack([u8(um.undistort(frames[a], Ks[b], ds[b], interp=interp, default=3)) for a in range(CONTENT) for b in range(PARAM)])
            assert table[1 * PARAM + 8].tobytes() != table[0].tobytes()          # frame 65 535 (content 1, camera 8) differs from frame 0
            d_out = ar.new(F * 8 * item)
            h.undistort(ptr(d_in), K, d, interp, ptr(d_out), 4, None, 3)
            ar.check("camera per frame, %s" % um.INTERP_NAMES[interp])
            check_cycle(d_out, table, lin, "camera per frame, %s" % um.INTERP_NAMES[interp])
        # the maps of 65 541 cameras: the camera index of the later slice
        d_x, d_y = ar.new(F * 8 * 4), ar.new(F * 8 * 4)
        h.maps(K, d, ptr(d_x), ptr(d_y))
        ar.check("maps per frame")
        ex, ey = zip(*[um.map_planes(Ks[b], ds[b], 4, 2) for b in range(PARAM)])
        check_cycle(d_x, np.stack([u8(m) for m in ex]), f % PARAM, "mapX per frame")
        check_cycle(d_y, np.stack([u8(m) for m in ey]), f % PARAM, "mapY per frame")
    finally:
        h.close()


def test_point_sets_beyond_65535(hip_ctx):
    """65 541 sets of 2 points, set s through camera (and pose) s % 11: the set index of the later slice, for points and for the projection"""
    from compv_amd import capi
    F, n = LIMIT + 6, 2
    Ks, ds = small_cameras(PARAM)
    sel = np.arange(F) % PARAM
    rng = np.random.default_rng(77)
    pts = rng.uniform(-1, 5, (F, n, 2)).astype(np.float32)
    pts3 = np.concatenate([rng.uniform(-1, 1, (F, n, 2)), np.ones((F, n, 1))], axis=2)
    poses = np.stack([np.concatenate([np.eye(3).ravel(), [0.01 * b, -0.02 * b, 2.0 + 0.1 * b]]) for b in range(PARAM)])
    exp, exp3 = np.empty_like(pts), np.empty((F, n, 2))
    for b in range(PARAM):
        at = sel == b
        exp[at] = um.dist_points(Ks[b], ds[b], pts[at].reshape(-1, 2), np.float32).reshape(-1, n, 2)
        exp3[at] = um.proj2d(Ks[b], ds[b], poses[b, :9], poses[b, 9:], pts3[at].reshape(-1, 3)).reshape(-1, n, 2)
    assert exp[LIMIT].tobytes() != um.dist_points(Ks[0], ds[0], pts[LIMIT], np.float32).tobytes()          # set 65 535 through camera 0 would show
    ar = Arena()
    d_pts, d_pts3 = ar.new(pts.nbytes, u8(pts)), ar.new(pts3.nbytes, u8(pts3))
    d_out, d_out3 = ar.new(exp.nbytes), ar.new(exp3.nbytes)
    h = capi.Undistort(hip_ctx, 4, 2, 4, 1, max_sets=F, max_points=n)
    try:
        h.points(Ks[sel], ds[sel], ptr(d_pts), F, n, ptr(d_out), capi.UNDISTORT_F32)
        h.project(Ks[sel], ds[sel], poses[sel], ptr(d_pts3), F, n, ptr(d_out3))
        ar.check("sets beyond the limit")
        assert d_out.cpu().numpy().tobytes() == exp.tobytes()
        assert d_out3.cpu().numpy().tobytes() == exp3.tobytes()
    finally:
        h.close()


def test_refusals_leave_everything_untouched(hip_ctx):
    from compv_amd import capi
    lib, E = hip_ctx.lib, capi.E_INVALID_PARAMETER
    start = hip_ctx.live_allocations()
    hnd = C.c_void_p(99)

    def create(**kw):
        args = dict(W=64, H=48, S=64, frames=2, Wout=64, Hout=48, x0=0, y0=0, max_sets=2, max_points=8)
        args.update(kw)
        desc = capi.UndistortDesc(**args)
        hnd.value = 99
        rc = lib.compvhip_undistort_create(hip_ctx.h, C.byref(desc), C.byref(hnd))
        assert hnd.value is None
        return rc
    for kw in (dict(W=0), dict(H=0), dict(W=32768, S=32768), dict(H=32768), dict(S=63), dict(W=2, S=3, Wout=2), dict(frames=0), dict(Wout=0), dict(Hout=0), dict(Wout=32768),
               dict(x0=32767 - 63), dict(y0=32767 - 47), dict(max_sets=1 << 31)):
        assert create(**kw) == E, kw
    desc = capi.UndistortDesc(64, 48, 64, 2, 64, 48)
    desc.size = 48
    assert lib.compvhip_undistort_create(hip_ctx.h, C.byref(desc), C.byref(hnd)) == E and lib.compvhip_undistort_create(hip_ctx.h, None, C.byref(hnd)) == E
    assert lib.compvhip_undistort_create(hip_ctx.h, C.byref(capi.UndistortDesc(64, 48, 64, 2, 64, 48)), None) == E
    assert hip_ctx.live_allocations() == start          # a refused create leaves nothing behind

    c = uc.case("pin61")
    rig = Rig(hip_ctx, c, 2, pad=3, max_sets=2, max_points=8)
    try:
        ar = rig.ar
        K, d = np.ascontiguousarray(c["K"], np.float32), np.ascontiguousarray(c["d"], np.float32)
        K64, d64 = K.astype(np.float64), d.astype(np.float64)
        singular = K.copy()
        singular[0, 0] = 0
        two = np.stack([K, singular])
        p = capi._ptr
        h, src, out = rig.h.h, ptr(rig.d_in), ptr(rig.d_out)
        ar.refill(rig.d_out)
        roi = None
        frames = [(None, p(K), p(d), 4, 1, 1, roi, 0, out, 64), (src, None, p(d), 4, 1, 1, roi, 0, out, 64), (src, p(K), None, 4, 1, 1, roi, 0, out, 64), (src, p(K), p(d), 4, 1, 1, roi, 0, None, 64),
                  (src, p(K), p(d), 1, 1, 1, roi, 0, out, 64), (src, p(K), p(d), 5, 1, 1, roi, 0, out, 64), (src, p(singular), p(d), 4, 1, 1, roi, 0, out, 64),
                  (src, p(two), p(np.stack([d, d])), 4, 2, 1, roi, 0, out, 64), (src, p(K), p(d), 4, 3, 1, roi, 0, out, 64), (src, p(K), p(d), 4, 0, 1, roi, 0, out, 64),
                  (src, p(K), p(d), 4, 1, 3, roi, 0, out, 64), (src, p(K), p(d), 4, 1, 6, roi, 0, out, 64), (src, p(K), p(d), 4, 1, -1, roi, 0, out, 64),
                  (src, p(K), p(d), 4, 1, 1, roi, 0, out, 60), (src, p(K), p(d), 4, 1, 2, roi, 0, out + 2, 64), (src, p(K), p(d), 4, 1, 5, roi, 0, out + 1, 64),
                  (src, p(K), p(d), 4, 1, 1, roi, 0, src + 8, 64)]
        for args in frames:
            assert lib.compvhip_undistort_frames(h, *args) == E, args[3:]
            assert hip_ctx.last_error()
        F32, F64 = capi.UNDISTORT_F32, capi.UNDISTORT_F64
        mx, my = ar.new(2 * 61 * 37 * 8), ar.new(2 * 61 * 37 * 8)
        maps = [(None, p(d), 4, 1, F32, ptr(mx), ptr(my)), (p(K), p(d), 4, 1, F32, None, ptr(my)), (p(K), p(d), 4, 1, F32, ptr(mx), None), (p(K), p(d), 4, 1, 2, ptr(mx), ptr(my)),
                (p(K), p(d), 4, 1, -1, ptr(mx), ptr(my)), (p(K), p(d), 0, 1, F32, ptr(mx), ptr(my)), (p(singular), p(d), 4, 1, F32, ptr(mx), ptr(my)), (p(K), p(d), 4, 3, F32, ptr(mx), ptr(my)),
                (p(K), p(d), 4, 1, F32, ptr(mx) + 2, ptr(my)), (p(K64), p(d64), 4, 1, F64, ptr(mx), ptr(my) + 4), (p(K), p(d), 4, 1, F32, ptr(mx), ptr(mx) + 64)]
        for args in maps:
            assert lib.compvhip_undistort_maps(h, *args) == E, args[2:5]
        pts, cnt, pout = ar.new(2 * 8 * 24), ar.new(8), ar.new(2 * 8 * 16)
        points = [(None, p(d64), 4, 1, F64, ptr(pts), 2, 8, ptr(cnt), ptr(pout)), (p(K64), p(d64), 4, 1, F64, None, 2, 8, ptr(cnt), ptr(pout)), (p(K64), p(d64), 4, 1, F64, ptr(pts), 2, 8, ptr(cnt), None),
                  (p(K64), p(d64), 4, 1, F64, ptr(pts), 3, 8, None, ptr(pout)), (p(K64), p(d64), 4, 1, F64, ptr(pts), 2, 9, None, ptr(pout)), (p(K64), p(d64), 4, 1, F64, ptr(pts), 0, 8, None, ptr(pout)),
                  (p(K64), p(d64), 4, 1, F64, ptr(pts), 2, 0, None, ptr(pout)), (p(K64), p(d64), 4, 3, F64, ptr(pts), 2, 8, None, ptr(pout)), (p(K64), p(d64), 4, 1, 7, ptr(pts), 2, 8, None, ptr(pout)),
                  (p(K64), p(d64), 5, 1, F64, ptr(pts), 2, 8, None, ptr(pout)), (p(singular.astype(np.float64)), p(d64), 4, 1, F64, ptr(pts), 2, 8, None, ptr(pout)),
                  (p(K64), p(d64), 4, 1, F64, ptr(pts) + 4, 2, 8, None, ptr(pout)), (p(K), p(d), 4, 1, F32, ptr(pts), 2, 8, None, ptr(pout) + 2), (p(K64), p(d64), 4, 1, F64, ptr(pts), 2, 8, ptr(cnt) + 2, ptr(pout)),
                  (p(K64), p(d64), 4, 1, F64, ptr(pts), 2, 8, None, ptr(pts) + 16)]
        for args in points:
            assert lib.compvhip_undistort_points(h, *args) == E, args[2:9]
        pose = np.concatenate([np.eye(3).ravel(), [0, 0, 1.0]] * 2)
        proj = [(None, p(d64), 4, 1, p(pose), ptr(pts), 2, 8, None, ptr(pout)), (p(K64), p(d64), 4, 1, None, ptr(pts), 2, 8, None, ptr(pout)), (p(K64), p(d64), 4, 1, p(pose), None, 2, 8, None, ptr(pout)),
                (p(K64), p(d64), 4, 1, p(pose), ptr(pts), 2, 8, None, None), (p(K64), p(d64), 4, 1, p(pose), ptr(pts), 3, 8, None, ptr(pout)), (p(K64), p(d64), 4, 1, p(pose), ptr(pts), 2, 9, None, ptr(pout)),
                (p(K64), p(d64), 1, 1, p(pose), ptr(pts), 2, 8, None, ptr(pout)), (p(K64), p(d64), 4, 3, p(pose), ptr(pts), 2, 8, None, ptr(pout)),
                (p(singular.astype(np.float64)), p(d64), 4, 1, p(pose), ptr(pts), 2, 8, None, ptr(pout)), (p(K64), p(d64), 4, 1, p(pose), ptr(pts) + 4, 2, 8, None, ptr(pout)),
                (p(K64), p(d64), 4, 1, p(pose), ptr(pts), 2, 8, None, ptr(pout) + 4), (p(K64), p(d64), 4, 1, p(pose), ptr(pts), 2, 8, None, ptr(pts) + 8)]
        for args in proj:
            assert lib.compvhip_undistort_project(h, *args) == E, args[2:9]
        ar.check("refused calls")
        for t in (rig.d_out, mx, my, pts, pout):
            assert (t.cpu().numpy() == SENTINEL).all()          # every destination still holds the sentinel
        # the host form
        img, host_out = uc.frame(c), np.full((37, 61), 7, np.uint8)
        ho = host_out.ctypes.data
        for args in ((None, 61, 37, 61, p(K), p(d), 4, 0, 0, 1, None, 0, ho, 61, 37, 61), (p(img), 61, 37, 61, None, p(d), 4, 0, 0, 1, None, 0, ho, 61, 37, 61), (p(img), 61, 37, 61, p(K), p(d), 5, 0, 0, 1, None, 0, ho, 61, 37, 61),
                     (p(img), 61, 37, 61, p(singular), p(d), 4, 0, 0, 1, None, 0, ho, 61, 37, 61), (p(img), 61, 37, 61, p(K), p(d), 4, 0, 0, 3, None, 0, ho, 61, 37, 61), (p(img), 61, 37, 61, p(K), p(d), 4, 32767, 0, 1, None, 0, ho, 61, 37, 61),
                     (p(img), 61, 37, 61, p(K), p(d), 4, 0, 0, 1, None, 0, ho, 61, 37, 60), (p(img), 61, 37, 61, p(K), p(d), 4, 0, 0, 1, None, 0, None, 61, 37, 61), (p(img), 0, 37, 61, p(K), p(d), 4, 0, 0, 1, None, 0, ho, 61, 37, 61)):
            assert lib.compvhip_undistort_u8(hip_ctx.h, *args) == E, args[6:11]
        assert (host_out == 7).all()
        # the handle still serves
        rig.run(1, K, d, 64)
        rig.check("after the refusals", [model_image(c, 1, k) for k in range(2)], 64)
    finally:
        rig.close()
    assert hip_ctx.live_allocations() == start
