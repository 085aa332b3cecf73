"""The remap and the inverse warp on the GPU (compvhip_plan_remap, compvhip_plan_warp_inverse and the host entries) against tests/remap_model.py on every
frame and against the planes the compiled reference wrote (tests/golden/golden_remap.npz) on frame 0, byte for byte -- float32 output by bit pattern.
Three frames, source S > W, guarded buffers from the Arena of tests/gpu_support.py: the destination is pre-filled with a sentinel, so the padding
columns and whatever lies behind the last frame must still hold it afterwards.  Every destination runs once aligned (the vector-store path) and once with a
stride that is no multiple of 4 elements (the element-store path); the widths cover Wout % 4 = 0, 1, 2, 3 and 261 exceeds one tile.  Every call is made twice.
The model's results are computed once per case and shared.

Dispatch arms (docs/dispatch_coverage.md): coordinate source map / 2 x 3 / 3 x 3, times nearest / bilinear / bilinear-float32, times vector / element
stores -- test_remap_cases and test_warp_cases launch all 18; the float4 map read (Wout % 4 == 0) runs in the 40-wide cases; the 8-frame loop with a
ragged last group in test_eleven_frames_cross_the_frame_groups."""
import functools

import numpy as np
import pytest

import remap_cases as rc
import remap_model as rm
from fixtures import load_golden
from gpu_support import Arena, SENTINEL, pad_frames, ptr

pytestmark = pytest.mark.gpu

G, A = load_golden("golden_remap")
F = 3
INTERPS = (rm.NEAREST, rm.BILINEAR, rm.BILINEAR_FLOAT32)
REMAP = {c["id"]: c for c in rc.remap_cases()}
WARP = {c["id"]: c for c in rc.warp_cases()}


def elem(interp):
    return 4 if interp == rm.BILINEAR_FLOAT32 else 1


def dtype_of(interp):
    return np.float32 if interp == rm.BILINEAR_FLOAT32 else np.uint8


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@functools.lru_cache(maxsize=None)
def frames_of(w, h, seed, n=F):
    out = np.stack([rc.frame(w, h, seed)] + [rc.frame(w, h, seed + 9000 + f, "noise" if f % 2 else "blocks") for f in range(1, n)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def maps_of(cid):
    """[F] maps of a remap case: frame 0 has the golden map"""
    c = REMAP[cid]
    w, h, wo, ho = c["size"]
    xs, ys = zip(*[rc.random_map(w, h, wo, ho, c["map_seed"] + 500 * f) for f in range(F)])
    return np.stack(xs), np.stack(ys)


@functools.lru_cache(maxsize=None)
def matrices_of(cid):
    """[F] matrices of a warp case: frame 0 has the golden matrix, the others a shifted and slightly sheared one"""
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
    out = np.stack([rm.remap(v, x[f if per_frame else 0], y[f if per_frame else 0], interp, c["roi"], c["default"]) for f, v in enumerate(frames_of(w, h, c["seed"]))])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_warp(cid, interp, per_frame):
    c = WARP[cid]
    w, h, wo, ho = c["size"]
    Ms = matrices_of(cid)
    out = np.stack([rm.warp_inverse(v, Ms[f if per_frame else 0], wo, ho, interp, c["default"]) for f, v in enumerate(frames_of(w, h, c["seed"]))])
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


def run_and_check(ar, call, frames, wo, ho, So, interp, exp, what, ref=None, tail=5):
    """call(d_out) twice on a sentinel-filled destination [frames][ho][So] (+ tail bytes); the valid elements equal exp, everything else the sentinel"""
    e = elem(interp)
    n = frames * ho * So * e
    d_out = ar.new(n + tail)
    call(ptr(d_out))
    ar.check(what)
    got = d_out.cpu().numpy()
    body = got[:n].view(dtype_of(interp)).reshape(frames, ho, So)
    assert same(np.ascontiguousarray(body[:, :, :wo]), np.ascontiguousarray(exp)), "%s: %d elements differ from the model" % (
        what, int((body[:, :, :wo].view(np.uint8) != exp.view(np.uint8)).sum()))
    assert (body[:, :, wo:].view(np.uint8) == SENTINEL).all() and (got[n:] == SENTINEL).all(), "%s: padding or tail written" % what
    if ref is not None:
        assert same(np.ascontiguousarray(body[0, :, :wo]), ref), "%s: the device against the reference's plane" % what
    call(ptr(d_out))          # twice: the same bytes
    ar.check(what + " again")
    assert (d_out.cpu().numpy() == got).all(), "%s: the second call differs" % what


def golden_plane(cid, interp):
    name = "%s_%s" % (cid, rc.INTERP_NAMES[interp])
    return A[name] if name in A.files else None


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
    d_x0, d_y0 = upload_floats(ar, np.stack([x[0]] * F)), upload_floats(ar, np.stack([y[0]] * F))          # the shared map, once per frame
    plan = capi.Plan(hip_ctx, w, h, S, F)
    try:
        for interp in INTERPS:
            shared = expected_remap(cid, interp, False)
            ref = golden_plane(cid, interp)
            assert ref is not None or (interp == rm.BILINEAR_FLOAT32 and wo % 8), "every plane the reference can vouch for is in the fixtures"
            if ref is not None:
                assert same(np.ascontiguousarray(shared[0]), ref), "the model against the reference's plane"
            for So in strides(wo):
                what = "%s %s So %d" % (cid, rc.INTERP_NAMES[interp], So)
                run_and_check(ar, lambda o: plan.remap(ptr(d_in), ptr(d_x), ptr(d_y), 1, interp, o, wo, ho, So, c["roi"], c["default"]), F, wo, ho, So, interp, shared,
                              what + " shared", ref)
                run_and_check(ar, lambda o: plan.remap(ptr(d_in), ptr(d_x), ptr(d_y), F, interp, o, wo, ho, So, c["roi"], c["default"]), F, wo, ho, So, interp,
                              expected_remap(cid, interp, True), what + " per frame", ref)
            # one map per frame, all the same map: what the shared map gives
            run_and_check(ar, lambda o: plan.remap(ptr(d_in), ptr(d_x0), ptr(d_y0), F, interp, o, wo, ho, strides(wo)[0], c["roi"], c["default"]), F, wo, ho,
                          strides(wo)[0], interp, shared, "%s %s same map per frame" % (cid, rc.INTERP_NAMES[interp]), ref)
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
            shared = expected_warp(cid, interp, False)
            ref = golden_plane(cid, interp)
            assert ref is not None or (interp == rm.BILINEAR_FLOAT32 and wo % 8) or (c["nan"] and interp == rm.NEAREST)
            if c["nan"]:
                assert (shared[:, :, 8].astype(np.float32) == c["default"]).all(), "Z == 0: infinities and a NaN, the default value"
            for So in strides(wo):
                what = "%s %s So %d" % (cid, rc.INTERP_NAMES[interp], So)
                run_and_check(ar, lambda o: plan.warp_inverse(ptr(d_in), Ms[0], interp, o, wo, ho, So, c["default"]), F, wo, ho, So, interp, shared, what + " shared", ref)
                run_and_check(ar, lambda o: plan.warp_inverse(ptr(d_in), Ms, interp, o, wo, ho, So, c["default"]), F, wo, ho, So, interp, expected_warp(cid, interp, True),
                              what + " per frame", ref)
            run_and_check(ar, lambda o: plan.warp_inverse(ptr(d_in), np.stack([Ms[0]] * F), interp, o, wo, ho, strides(wo)[0], c["default"]), F, wo, ho, strides(wo)[0],
                          interp, shared, "%s %s same matrix per frame" % (cid, rc.INTERP_NAMES[interp]), ref)
    finally:
        plan.close()


def test_nan_and_infinities_in_a_map_give_the_default_value(hip_ctx):
    from compv_amd import capi
    w, h, wo, ho = rc.SIZES[0]
    S = (w + 7) // 8 * 8 + 8
    valid = frames_of(w, h, 64001)
    x, y = rc.random_map(w, h, wo, ho, 64002)
    x, y = np.clip(x, 0, w - 1), np.clip(y, 0, h - 1)          # everything inside ...
    bad = ((0, 0, np.nan, 1.0), (1, 5, 1.0, np.nan), (2, 9, np.inf, 1.0), (3, 60, 1.0, -np.inf), (ho - 1, wo - 1, -np.inf, np.nan), (7, 13, np.nan, np.nan))
    for (j, i, vx, vy) in bad:          # ... but these
        x[j, i], y[j, i] = vx, vy
    ar = Arena()
    d_in = upload_frames(ar, valid, S)
    d_x, d_y = upload_floats(ar, x), upload_floats(ar, y)
    plan = capi.Plan(hip_ctx, w, h, S, F)
    try:
        for interp in INTERPS:
            exp = np.stack([rm.remap(v, x, y, interp, None, 201) for v in valid])
            for (j, i, _, _) in bad:
                assert (exp[:, j, i] == 201).all()
            assert (exp != 201).mean() > 0.9
            So = strides(wo)[0]
            run_and_check(ar, lambda o: plan.remap(ptr(d_in), ptr(d_x), ptr(d_y), 1, interp, o, wo, ho, So, None, 201), F, wo, ho, So, interp, exp,
                          "NaN map %s" % rc.INTERP_NAMES[interp])
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
        exp = np.stack([rm.remap(v, x, y, rm.BILINEAR, None, 3) for v in valid])
        run_and_check(ar, lambda o: plan.remap(ptr(d_in), ptr(d_x), ptr(d_y), 1, rm.BILINEAR, o, wo, ho, So, None, 3), n, wo, ho, So, rm.BILINEAR, exp, "11 frames, map")
        exp = np.stack([rm.warp_inverse(v, M, wo, ho, rm.NEAREST, 3) for v in valid])
        run_and_check(ar, lambda o: plan.warp_inverse(ptr(d_in), M, rm.NEAREST, o, wo, ho, So, 3), n, wo, ho, So, rm.NEAREST, exp, "11 frames, matrix")
    finally:
        plan.close()


def test_timing_entries(hip_ctx):
    from compv_amd import capi
    w, h, wo, ho = rc.SIZES[3]
    S = (w + 7) // 8 * 8 + 8
    ar = Arena()
    d_in = upload_frames(ar, frames_of(w, h, 66001), S)
    x, y = rc.random_map(w, h, wo, ho, 66002)
    d_x, d_y = upload_floats(ar, x), upload_floats(ar, y)
    d_out = ar.new(F * ho * 8)
    plan = capi.Plan(hip_ctx, w, h, S, F)
    try:
        plan.set_timing(1)
        plan.remap(ptr(d_in), ptr(d_x), ptr(d_y), 1, rm.BILINEAR, ptr(d_out), wo, ho, 8)
        t = plan.get_timing()
        assert [n for n, _ in t] == ["remap_kernel"] and t[0][1] >= 0
        plan.warp_inverse(ptr(d_in), np.eye(3, dtype=np.float32), rm.NEAREST, ptr(d_out), wo, ho, 8)
        t = plan.get_timing()
        assert [n for n, _ in t] == ["warp_inverse_kernel"] and t[0][1] >= 0
        ar.check("timing")
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
    M2, M3 = np.eye(3, dtype=np.float32)[:2], np.eye(3, dtype=np.float32)
    plan = capi.Plan(hip_ctx, w, h, S, F)
    lib = plan.lib

    def refused(rc_):
        assert rc_ == capi.E_INVALID_PARAMETER

    def remap(d_in_=None, mx=None, my=None, count=1, interp=rm.BILINEAR, out=None, wo_=wo, ho_=ho, so=wo):
        return lib.compvhip_plan_remap(plan.h, ptr(d_in) if d_in_ is None else d_in_ or None, ptr(d_map) if mx is None else mx or None,
                                       ptr(d_map) if my is None else my or None, count, interp, None, 0, ptr(d_out) if out is None else out or None, wo_, ho_, so, None)

    def warp(M=M3, rows=3, count=1, interp=rm.BILINEAR, out=None, wo_=wo, ho_=ho, so=wo, d_in_=None):
        return lib.compvhip_plan_warp_inverse(plan.h, ptr(d_in) if d_in_ is None else d_in_ or None, capi._ptr(M) if M is not None else None, rows, count, interp, 0,
                                              ptr(d_out) if out is None else out or None, wo_, ho_, so, None)
    try:
        assert remap() == capi.OK and warp() == capi.OK and warp(M2, 2) == capi.OK          # the calls are sound before they are spoilt
        ar.refill(d_out)
        for bad in (dict(d_in_=0), dict(mx=0), dict(my=0), dict(out=0),          # null pointers
                    dict(wo_=0), dict(ho_=0),          # a zero size
                    dict(so=wo - 1), dict(interp=rm.BILINEAR_FLOAT32, so=wo - 1),          # Sout < Wout, in bytes and in elements
                    dict(count=0), dict(count=2), dict(count=F + 1),          # a count that is neither 1 nor frames
                    dict(interp=3), dict(interp=-1)):          # an unknown interpolation
            refused(remap(**bad))
        for bad in (dict(d_in_=0), dict(M=None), dict(out=0), dict(wo_=0), dict(ho_=0), dict(so=wo - 1), dict(interp=rm.BILINEAR_FLOAT32, so=wo - 1),
                    dict(rows=1), dict(rows=4), dict(rows=0), dict(count=0), dict(count=2), dict(interp=3), dict(interp=-1)):
            refused(warp(**bad))
        refused(remap(out=ptr(d_in)))          # in place
        img = np.zeros((h, w), np.uint8)
        with pytest.raises(capi.CompvHipError) as e:
            hip_ctx.remap(img, np.zeros((4, 4), np.float32), np.zeros((4, 4), np.float32), interp=7)
        assert e.value.code == capi.E_INVALID_PARAMETER
        with pytest.raises(capi.CompvHipError) as e:
            hip_ctx.warp_inverse(img, np.zeros((4, 3), np.float32), 4, 4)
        assert e.value.code == capi.E_INVALID_PARAMETER
        ar.check("refusals")
        assert (d_out.cpu().numpy() == SENTINEL).all()
    finally:
        plan.close()


@pytest.mark.parametrize("cid", ["map0", "map2", "map4", "map_roi"])
def test_host_remap(hip_ctx, cid):
    c = REMAP[cid]
    w, h, wo, ho = c["size"]
    img = rc.frame(w, h, c["seed"])
    wide = np.full((h, w + 5), 201, np.uint8)          # a host plane with a stride of its own
    wide[:, :w] = img
    x, y = rc.random_map(w, h, wo, ho, c["map_seed"])
    for interp in INTERPS:
        got = hip_ctx.remap(wide[:, :w], x, y, interp, c["roi"], c["default"])
        assert same(got, rm.remap(img, x, y, interp, c["roi"], c["default"])), (cid, interp)
        ref = golden_plane(cid, interp)
        if ref is not None:
            assert same(got, ref)


@pytest.mark.parametrize("cid", ["warp0_affine", "warp1_homography", "warp2_homography", "warp3_mostly_outside", "warp4_affine", "warp_z_sign"])
def test_host_warp_inverse(hip_ctx, cid):
    c = WARP[cid]
    w, h, wo, ho = c["size"]
    img = rc.frame(w, h, c["seed"])
    wide = np.full((h, w + 3), 201, np.uint8)
    wide[:, :w] = img
    for interp in INTERPS:
        got = hip_ctx.warp_inverse(wide[:, :w], c["M"], wo, ho, interp, c["default"])
        assert same(got, rm.warp_inverse(img, c["M"], wo, ho, interp, c["default"])), (cid, interp)
        ref = golden_plane(cid, interp)
        if ref is not None:
            assert same(got, ref)
