"""The bicubic remap and inverse warp on the GPU (COMPVHIP_INTERP_BICUBIC / _BICUBIC_FLOAT32 through compvhip_plan_remap, compvhip_plan_warp_inverse and
the host entries) against tests/bicubic_model.py on every frame and against the fixture (tests/golden/golden_bicubic.npz, the model held against the compiled
reference's plain leaves) on frame 0, byte for byte -- float32 output by bit pattern.  Three frames, source S > W, guarded buffers from the Arena of
tests/gpu_support.py: the destination is pre-filled with a sentinel, so the padding columns and whatever lies behind the last frame must still
hold it afterwards.  Every destination runs once aligned (vector stores) and once with a stride that is no multiple of 4 elements (element stores); the widths
cover Wout % 4 = 0 .. 3 and 261 exceeds one tile.  Every call is made twice.  The model's results are computed once per case and shared.

Dispatch arms (docs/dispatch_coverage.md): remap_bicubic_kernel over map / 2 x 3 / 3 x 3, times uint8 / float32, times vector / element stores --
test_remap_cases and test_warp_cases launch all 12; the base clamp of the 4-byte tap row in test_narrow_sources; the 8-frame loop with a ragged last group in
test_eleven_frames_cross_the_frame_groups; the sliced launch in test_sliced_launch_beyond_65535_frames."""
import functools

import numpy as np
import pytest

import bicubic_cases as bc
import bicubic_model as bm
import remap_cases as rc
import remap_model as rm
from fixtures import load_golden
from gpu_support import Arena, SENTINEL, pad_frames, ptr

pytestmark = pytest.mark.gpu

A = load_golden("golden_bicubic")[1]
F = 3
INTERPS = bc.INTERPS
REMAP = {c["id"]: c for c in bc.remap_cases()}
WARP = {c["id"]: c for c in bc.warp_cases()}
NARROW = {c["id"]: c for c in bc.narrow_cases()}


def elem(interp):
    return 4 if interp == bm.BICUBIC_FLOAT32 else 1


def dtype_of(interp):
    return np.float32 if interp == bm.BICUBIC_FLOAT32 else np.uint8


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@functools.lru_cache(maxsize=None)
def frames_of(w, h, seed, n=F):
    """frame 0 is the fixture's"""
    out = np.stack([rc.frame(w, h, seed)] + [rc.frame(w, h, seed + 9000 + f, "noise" if f % 2 else "blocks") for f in range(1, n)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def maps_of(cid):
    """[F] maps of a remap case: frame 0 has the fixture's map"""
    c = REMAP[cid]
    w, h, wo, ho = c["size"]
    xs, ys = zip(*[rc.random_map(w, h, wo, ho, c["map_seed"] + 500 * f) for f in range(F)])
    return np.stack(xs), np.stack(ys)


@functools.lru_cache(maxsize=None)
def matrices_of(cid):
    """[F] matrices of a warp case: frame 0 has the fixture's matrix, the others a shifted and slightly sheared one"""
    M = WARP[cid]["M"]
    out = [M]
    for f in range(1, F):
        Mf = M.copy()
        Mf[0, 2] += np.float32(1.25 * f)
        Mf[1, 0] += np.float32(0.015 * f)
        out.append(Mf)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def expected_remap(cid, interp, per_frame):
    c = REMAP[cid]
    w, h, _, _ = c["size"]
    x, y = maps_of(cid)
    out = np.stack([bm.remap(v, x[f if per_frame else 0], y[f if per_frame else 0], interp, c["roi"], c["default"]) for f, v in enumerate(frames_of(w, h, c["seed"]))])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_warp(cid, interp, per_frame):
    c = WARP[cid]
    w, h, wo, ho = c["size"]
    Ms = matrices_of(cid)
    out = np.stack([bm.warp_inverse(v, Ms[f if per_frame else 0], wo, ho, interp, c["default"]) for f, v in enumerate(frames_of(w, h, c["seed"]))])
    out.setflags(write=False)
    return out


def strides(w_out):
    """in elements: one a multiple of 4 (vector stores), one not (element stores)"""
    aligned = (w_out + 3) // 4 * 4 + 4
    odd = w_out + 1 + ((w_out + 1) % 4 == 0)
    assert aligned % 4 == 0 and odd % 4 != 0
    return aligned, odd


def upload_frames(ar, valid, S):
    host = pad_frames(valid, S, np.random.default_rng(valid.shape[2] * 31 + valid.shape[1]))
    d = ar.new(host.size, host.reshape(-1))
    ar.keep(d, host)
    return d


def upload_floats(ar, a):
    raw = np.ascontiguousarray(a, np.float32).view(np.uint8).reshape(-1)
    d = ar.new(raw.size, raw)
    ar.keep(d, raw)
    return d


def check_body(got, frames, wo, ho, So, interp, exp, what, ref=None):
    """got: the destination's bytes [frames][ho][So] (+ a tail); the valid elements equal exp, everything else the sentinel"""
    n = frames * ho * So * elem(interp)
    body = got[:n].view(dtype_of(interp)).reshape(frames, ho, So)
    assert same(np.ascontiguousarray(body[:, :, :wo]), np.ascontiguousarray(exp)), "%s: %d bytes differ from the model" % (
        what, int((np.ascontiguousarray(body[:, :, :wo]).view(np.uint8) != np.ascontiguousarray(exp).view(np.uint8)).sum()))
    assert (np.ascontiguousarray(body[:, :, wo:]).view(np.uint8) == SENTINEL).all() and (got[n:] == SENTINEL).all(), "%s: padding or tail written" % what
    if ref is not None:
        assert same(np.ascontiguousarray(body[0, :, :wo]), ref), "%s: the device against the fixture's plane" % what


def run_and_check(ar, call, frames, wo, ho, So, interp, exp, what, ref=None, tail=5):
    """call(d_out) twice on a sentinel-filled destination [frames][ho][So] (+ tail bytes)"""
    n = frames * ho * So * elem(interp)
    d_out = ar.new(n + tail)
    call(ptr(d_out))
    ar.check(what)
    got = d_out.cpu().numpy()
    check_body(got, frames, wo, ho, So, interp, exp, what, ref)
    call(ptr(d_out))          # twice: the same bytes
    ar.check(what + " again")
    assert (d_out.cpu().numpy() == got).all(), "%s: the second call differs" % what


def test_the_cases_cover_every_tail_and_two_tiles():
    assert {c["size"][2] % 4 for c in REMAP.values()} == {0, 1, 2, 3} == {c["size"][2] % 4 for c in WARP.values()}
    assert max(c["size"][2] for c in REMAP.values()) > 256 and max(c["size"][2] for c in WARP.values()) > 256
    assert {WARP[k]["M"].shape[0] for k in WARP} == {2, 3}


@pytest.mark.parametrize("cid", list(REMAP))
def test_remap_cases(hip_ctx, cid):
    from compv_amd import capi
    c = REMAP[cid]
    w, h, wo, ho = c["size"]
    S = (w + 7) // 8 * 8 + 8
    x, y = maps_of(cid)
    ar = Arena()
    d_in = upload_frames(ar, frames_of(w, h, c["seed"]), S)
    d_x, d_y = upload_floats(ar, x), upload_floats(ar, y)          # [F] maps; the first alone is the shared one
    plan = capi.Plan(hip_ctx, w, h, S, F)
    try:
        for interp in INTERPS:
            shared, ref = expected_remap(cid, interp, False), A[bc.key(cid, interp)]
            assert same(np.ascontiguousarray(shared[0]), ref), "the model against the fixture's plane"
            for So in strides(wo):
                what = "%s %s So %d" % (cid, bc.INTERP_NAMES[interp], So)
                run_and_check(ar, lambda o: plan.remap(ptr(d_in), ptr(d_x), ptr(d_y), 1, interp, o, wo, ho, So, c["roi"], c["default"]), F, wo, ho, So, interp, shared,
                              what + " shared", ref)
                run_and_check(ar, lambda o: plan.remap(ptr(d_in), ptr(d_x), ptr(d_y), F, interp, o, wo, ho, So, c["roi"], c["default"]), F, wo, ho, So, interp,
                              expected_remap(cid, interp, True), what + " per frame", ref)
    finally:
        plan.close()


@pytest.mark.parametrize("cid", list(WARP))
def test_warp_cases(hip_ctx, cid):
    from compv_amd import capi
    c = WARP[cid]
    w, h, wo, ho = c["size"]
    S = (w + 7) // 8 * 8 + 8
    Ms = matrices_of(cid)
    ar = Arena()
    d_in = upload_frames(ar, frames_of(w, h, c["seed"]), S)
    plan = capi.Plan(hip_ctx, w, h, S, F)
    try:
        for interp in INTERPS:
            shared, ref = expected_warp(cid, interp, False), A[bc.key(cid, interp)]
            if c["nan"]:
                assert (shared[:, :, 8].astype(np.float32) == c["default"]).all(), "Z == 0: infinities and a NaN, the default value"
                assert (shared[:, :, 9:14] != c["default"]).any(), "X, Z < 0: inside again"
            for So in strides(wo):
                what = "%s %s So %d" % (cid, bc.INTERP_NAMES[interp], So)
                run_and_check(ar, lambda o: plan.warp_inverse(ptr(d_in), Ms[0], interp, o, wo, ho, So, c["default"]), F, wo, ho, So, interp, shared, what + " shared", ref)
                run_and_check(ar, lambda o: plan.warp_inverse(ptr(d_in), Ms, interp, o, wo, ho, So, c["default"]), F, wo, ho, So, interp, expected_warp(cid, interp, True),
                              what + " per frame", ref)
    finally:
        plan.close()


@pytest.mark.parametrize("cid", list(NARROW))
def test_narrow_sources(hip_ctx, cid):
    """sources narrower than, as wide as and one wider than the four taps: every tap clamps, the 4-byte tap row sits at base 0 (or 1).  The host calls take
    any size; a plan takes W, H >= 3 at a stride that is a multiple of 8."""
    from compv_amd import capi
    c = NARROW[cid]
    w, h, wo, ho = c["size"]
    img = rc.frame(w, h, c["seed"])
    x, y = bc.map_of(c)
    M = np.array([[w / wo, 0.0, -0.25], [0.0, h / ho, -0.25]], np.float32)
    for interp in INTERPS:
        ref = A[bc.key(cid, interp)]
        got = hip_ctx.remap(img, x, y, interp, None, c["default"])
        assert same(got, bm.remap(img, x, y, interp, None, c["default"])) and same(got, ref), (cid, interp)
        assert same(hip_ctx.warp_inverse(img, M, wo, ho, interp, c["default"]), bm.warp_inverse(img, M, wo, ho, interp, c["default"])), (cid, interp)
    if w < 3 or h < 3:
        return
    valid = frames_of(w, h, c["seed"])
    ar = Arena()
    d_in = upload_frames(ar, valid, 8)
    d_x, d_y = upload_floats(ar, x), upload_floats(ar, y)
    plan = capi.Plan(hip_ctx, w, h, 8, F)
    try:
        for interp in INTERPS:
            exp = np.stack([bm.remap(v, x, y, interp, None, c["default"]) for v in valid])
            for So in strides(wo):
                run_and_check(ar, lambda o: plan.remap(ptr(d_in), ptr(d_x), ptr(d_y), 1, interp, o, wo, ho, So, None, c["default"]), F, wo, ho, So, interp, exp,
                              "%s %s So %d" % (cid, bc.INTERP_NAMES[interp], So), A[bc.key(cid, interp)])
    finally:
        plan.close()


def test_nan_and_infinities_in_a_map_give_the_default_value(hip_ctx):
    from compv_amd import capi
    c = bc.nan_case()
    w, h, wo, ho = c["size"]
    S = (w + 7) // 8 * 8 + 8
    valid = frames_of(w, h, c["seed"])
    x, y = bc.nan_map()
    ar = Arena()
    d_in = upload_frames(ar, valid, S)
    d_x, d_y = upload_floats(ar, x), upload_floats(ar, y)
    plan = capi.Plan(hip_ctx, w, h, S, F)
    try:
        for interp in INTERPS:
            exp = np.stack([bm.remap(v, x, y, interp, None, c["default"]) for v in valid])
            for (j, i, _, _) in bc.NAN_ENTRIES:
                assert (exp[:, j, i] == c["default"]).all()
            assert (exp != c["default"]).mean() > 0.9
            So = strides(wo)[0]
            run_and_check(ar, lambda o: plan.remap(ptr(d_in), ptr(d_x), ptr(d_y), 1, interp, o, wo, ho, So, None, c["default"]), F, wo, ho, So, interp, exp,
                          "NaN map %s" % bc.INTERP_NAMES[interp], A[bc.key(c["id"], interp)])
    finally:
        plan.close()


def test_eleven_frames_cross_the_frame_groups(hip_ctx):
    """a shared map or matrix serves 8 frames per workgroup: 11 frames make a full group and a ragged one"""
    from compv_amd import capi
    w, h, wo, ho = rc.SIZES[2]
    n = 11
    assert n > 8 and n % 8
    S = (w + 7) // 8 * 8 + 8
    valid = frames_of(w, h, 65001, n)
    x, y = rc.random_map(w, h, wo, ho, 65002)
    M = rc.matrices(w, h, wo, ho)["homography"]
    ar = Arena()
    d_in = upload_frames(ar, valid, S)
    d_x, d_y = upload_floats(ar, x), upload_floats(ar, y)
    plan = capi.Plan(hip_ctx, w, h, S, n)
    try:
        So = strides(wo)[0]
        exp = np.stack([bm.remap(v, x, y, bm.BICUBIC, None, 3) for v in valid])
        run_and_check(ar, lambda o: plan.remap(ptr(d_in), ptr(d_x), ptr(d_y), 1, bm.BICUBIC, o, wo, ho, So, None, 3), n, wo, ho, So, bm.BICUBIC, exp, "11 frames, map")
        exp = np.stack([bm.warp_inverse(v, M, wo, ho, bm.BICUBIC_FLOAT32, 3) for v in valid])
        run_and_check(ar, lambda o: plan.warp_inverse(ptr(d_in), M, bm.BICUBIC_FLOAT32, o, wo, ho, So, 3), n, wo, ho, So, bm.BICUBIC_FLOAT32, exp, "11 frames, matrix")
    finally:
        plan.close()


@pytest.mark.parametrize("cid", ["map0", "map2", "map_roi"])
def test_host_remap(hip_ctx, cid):
    c = REMAP[cid]
    w, h, wo, ho = c["size"]
    img = rc.frame(w, h, c["seed"])
    wide = np.full((h, w + 5), 201, np.uint8)          # a host plane with a stride of its own
    wide[:, :w] = img
    x, y = rc.random_map(w, h, wo, ho, c["map_seed"])
    for interp in INTERPS:
        got = hip_ctx.remap(wide[:, :w], x, y, interp, c["roi"], c["default"])
        assert got.dtype == dtype_of(interp)
        assert same(got, bm.remap(img, x, y, interp, c["roi"], c["default"])) and same(got, A[bc.key(cid, interp)]), (cid, interp)


@pytest.mark.parametrize("cid", ["warp0_affine", "warp1_homography", "warp3_mostly_outside", "warp_z_sign"])
def test_host_warp_inverse(hip_ctx, cid):
    c = WARP[cid]
    w, h, wo, ho = c["size"]
    img = rc.frame(w, h, c["seed"])
    wide = np.full((h, w + 3), 201, np.uint8)
    wide[:, :w] = img
    for interp in INTERPS:
        got = hip_ctx.warp_inverse(wide[:, :w], c["M"], wo, ho, interp, c["default"])
        assert got.dtype == dtype_of(interp)
        assert same(got, bm.warp_inverse(img, c["M"], wo, ho, interp, c["default"])) and same(got, A[bc.key(cid, interp)]), (cid, interp)


def test_odd_byte_offsets_of_source_and_destination(hip_ctx):
    """the 4-byte tap rows are read at any address; a uint8 destination is served at any byte, a float32 destination at +1 and +2 is refused untouched"""
    from compv_amd import capi
    c = REMAP["map5"]
    w, h, wo, ho = c["size"]
    S, So = (w + 7) // 8 * 8 + 8, 32
    valid = frames_of(w, h, c["seed"])
    x, y = rc.random_map(w, h, wo, ho, c["map_seed"])
    M = rc.matrices(w, h, wo, ho)["affine"]
    host = pad_frames(valid, S, np.random.default_rng(5)).reshape(-1)
    ar = Arena()
    d_x, d_y = upload_floats(ar, x), upload_floats(ar, y)
    plan = capi.Plan(hip_ctx, w, h, S, F)
    try:
        for interp in INTERPS:
            exp_r = np.stack([bm.remap(v, x, y, interp, None, 9) for v in valid])
            exp_w = np.stack([bm.warp_inverse(v, M, wo, ho, interp, 9) for v in valid])
            for oi, oo in ((1, 0), (3, 1), (2, 2), (1, 3), (0, 4)):
                d_in = ar.new(host.size + oi)[oi:]
                d_in.copy_(ar.torch.from_numpy(host))
                n = F * ho * So * elem(interp)
                d_out = ar.new(n + oo)
                for name, exp, call in (("remap", exp_r, lambda: plan.remap(ptr(d_in), ptr(d_x), ptr(d_y), 1, interp, ptr(d_out) + oo, wo, ho, So, None, 9)),
                                        ("warp", exp_w, lambda: plan.warp_inverse(ptr(d_in), M, interp, ptr(d_out) + oo, wo, ho, So, 9))):
                    what = "%s %s at +%d -> +%d" % (name, bc.INTERP_NAMES[interp], oi, oo)
                    ar.refill(d_out)
                    if elem(interp) == 4 and oo % 4:
                        with pytest.raises(capi.CompvHipError) as err:
                            call()
                        assert err.value.code == capi.E_INVALID_PARAMETER and "align" in hip_ctx.last_error(), what
                        ar.check(what)
                        assert (d_out.cpu().numpy() == SENTINEL).all(), what + ": a refused call wrote"
                        continue
                    call()
                    ar.check(what)
                    got = d_out.cpu().numpy()
                    assert (got[:oo] == SENTINEL).all(), what + ": bytes in front of the destination written"
                    check_body(got[oo:], F, wo, ho, So, interp, exp, what)
                    assert (d_in.cpu().numpy() == host).all(), what + ": input modified"
    finally:
        plan.close()


def test_behind_pending_work_on_a_callers_stream(hip_ctx):
    """the frames reach the device on the caller's stream behind a delay, the call follows on that stream and returns at once; the matrix array is
    overwritten as soon as it has returned"""
    import torch
    from compv_amd import capi
    c = WARP["warp0_homography"]
    w, h, wo, ho = c["size"]
    S, So = (w + 7) // 8 * 8 + 8, strides(wo)[0]
    valid = frames_of(w, h, c["seed"])
    Ms = matrices_of(c["id"]).copy()
    host = torch.from_numpy(pad_frames(valid, S, np.random.default_rng(6)).reshape(-1)).pin_memory()
    ar = Arena()
    d_in = ar.new(host.numel())          # holds the sentinel until the copy on the side stream lands
    plan = capi.Plan(hip_ctx, w, h, S, F)
    side = torch.cuda.Stream()
    try:
        for interp in INTERPS:
            exp = expected_warp(c["id"], interp, True)
            d_out = ar.new(F * ho * So * elem(interp) + 5)
            ar.refill(d_in)
            torch.cuda.synchronize()
            M = Ms.copy()
            with torch.cuda.stream(side):
                torch.cuda._sleep(20_000_000)          # a few milliseconds of pending work in front of the copy
                d_in.copy_(host, non_blocking=True)
            plan.warp_inverse(ptr(d_in), M, interp, ptr(d_out), wo, ho, So, c["default"], stream=side.cuda_stream)
            M[:] = np.float32(777.0)          # the call has staged it
            side.synchronize()
            ar.check("stream %s" % bc.INTERP_NAMES[interp])
            check_body(d_out.cpu().numpy(), F, wo, ho, So, interp, exp, "behind pending work, %s" % bc.INTERP_NAMES[interp])
    finally:
        plan.close()


def test_sliced_launch_beyond_65535_frames(hip_ctx):
    """65 537 frames of 4 x 4 (S = 8, the smallest stride a plan takes) to 5 x 3 with a matrix per frame: two launches, the second starts at frame 65 535.
    Frame f holds content f % 7 and goes through matrix f % 11: neither period divides 65 535, so a slice that started at frame 0 again would fail."""
    from compv_amd import capi
    w, h, S, wo, ho, n = 4, 4, 8, 5, 3, 65537
    content, param = 7, 11
    assert 65535 % content and 65535 % param
    frames = np.stack([rc.frame(w, h, 69000 + d) for d in range(content)])
    base = np.array([[0.7, 0.05, 0.1], [0.02, 1.1, -0.2], [1e-3, 5e-4, 1.0]], np.float32)
    Ms = np.stack([base] * param)
    for k in range(param):
        Ms[k, 0, 2] += np.float32(0.125 * k)
        Ms[k, 1, 0] += np.float32(0.03 * k)
    f = np.arange(n)
    host = np.full((n, h, S), 0x5A, np.uint8)
    host[:, :, :w] = frames[f % content]
    all_M = np.ascontiguousarray(Ms[f % param])
    ar = Arena()
    d_in = ar.new(host.size, host.reshape(-1))
    ar.keep(d_in, host)
    plan = capi.Plan(hip_ctx, w, h, S, n)
    try:
        for interp in INTERPS:
            table = np.stack([np.stack([bm.warp_inverse(frames[d], Ms[k], wo, ho, interp, 17) for k in range(param)]) for d in range(content)])
            assert table[65535 % content, 65535 % param].tobytes() != table[0, 0].tobytes()
            exp = table[f % content, f % param]
            d_out = ar.new(n * ho * wo * elem(interp) + 5)
            plan.warp_inverse(ptr(d_in), all_M, interp, ptr(d_out), wo, ho, wo, 17)
            ar.check("sliced %s" % bc.INTERP_NAMES[interp])
            check_body(d_out.cpu().numpy(), n, wo, ho, wo, interp, exp, "65 537 frames, %s" % bc.INTERP_NAMES[interp])
    finally:
        plan.close()


def test_refusals_leave_the_destination_alone(hip_ctx):
    from compv_amd import capi
    w, h, S = 64, 48, 72
    wo, ho = 16, 8
    ar = Arena()
    d_in = ar.new(F * h * S, 17)
    d_map = upload_floats(ar, np.zeros((F, ho, wo), np.float32))
    d_out = ar.new(8192)
    M3 = np.eye(3, dtype=np.float32)
    plan = capi.Plan(hip_ctx, w, h, S, F)
    lib = plan.lib

    def remap(interp, out=None, so=wo):
        return lib.compvhip_plan_remap(plan.h, ptr(d_in), ptr(d_map), ptr(d_map), 1, interp, None, 0, ptr(d_out) if out is None else out, wo, ho, so, None)

    def warp(interp, out=None, so=wo):
        return lib.compvhip_plan_warp_inverse(plan.h, ptr(d_in), capi._ptr(M3), 3, 1, interp, 0, ptr(d_out) if out is None else out, wo, ho, so, None)
    try:
        for interp in INTERPS:
            assert remap(interp) == capi.OK and warp(interp) == capi.OK          # the calls are sound before they are spoilt
        ar.refill(d_out)
        for call in (remap, warp):
            for interp in (3, 6):          # 3 stays unassigned between the bilinear and the bicubic values
                assert call(interp) == capi.E_INVALID_PARAMETER
            for interp in INTERPS:
                assert call(interp, so=wo - 1) == capi.E_INVALID_PARAMETER          # Sout < Wout: in bytes, and in elements for float32
                assert call(interp, out=ptr(d_in)) == capi.E_INVALID_PARAMETER          # in place
                assert call(interp, out=ptr(d_in) + F * h * S - 1) == capi.E_INVALID_PARAMETER          # the last source byte is the first of the destination
        img = np.zeros((h, w), np.uint8)
        for interp in (3, 6):
            with pytest.raises(capi.CompvHipError) as e:
                hip_ctx.remap(img, np.zeros((4, 4), np.float32), np.zeros((4, 4), np.float32), interp=interp)
            assert e.value.code == capi.E_INVALID_PARAMETER
            with pytest.raises(capi.CompvHipError) as e:
                hip_ctx.warp_inverse(img, np.eye(3, dtype=np.float32), 4, 4, interp=interp)
            assert e.value.code == capi.E_INVALID_PARAMETER
        ar.check("refusals")
        assert (d_out.cpu().numpy() == SENTINEL).all()
        assert (d_in.cpu().numpy() == 17).all()
    finally:
        plan.close()
