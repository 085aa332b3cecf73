"""The bilinear scale on the GPU (compvhip_plan_scale, compvhip_scale_u8) against tests/orb_pyramid_model.py byte for byte, and -- for the downscales the
golden generator ran through CompVImage::scale -- against the planes the compiled reference wrote (tests/golden/golden_orb_pyramid.npz).  Three frames,
S > W on both sides, guarded buffers from the Arena of tests/gpu_support.py: the destination is pre-filled with a sentinel, so the padding
columns and whatever lies behind the last frame must still hold it afterwards.  Every destination runs with a dword-aligned stride (the dword-store path)
and with one that is no multiple of 4 (the byte path); the widths cover Wout % 4 = 0, 1, 2, 3.  Upscales and the identity are held against the model alone:
the reference reads past its plane there (include/compv_hip.h, rule A.5)."""
import numpy as np
import pytest

import fast_model as fm
import orb_pyramid_model as pm
from fixtures import load_golden
from gpu_support import Arena, SENTINEL, pad_frames, ptr

pytestmark = pytest.mark.gpu

G, A = load_golden("golden_orb_pyramid")
F = 3
DOWN = tuple((s["W"], s["H"], s["Wout"], s["Hout"]) for s in G["scales"])          # (9, 7, 7, 5), (64, 41, 53, 34), (1100, 5, 1021, 4), (300, 8, 2, 1)
UP = ((16, 16, 40, 23), (37, 37, 38, 37))
SAME = ((64, 41, 64, 41),)
CASES = DOWN + UP + SAME
CID = lambda c: "%dx%d_to_%dx%d" % c          # noqa: E731


def test_the_widths_cover_every_tail():
    assert {c[2] % 4 for c in CASES} == {0, 1, 2, 3}


def frames_of(case):
    W, H = case[:2]
    k = DOWN.index(case) if case in DOWN else None
    seed0 = G["scales"][k]["seed"] if k is not None else 900 + W
    return np.stack([fm.noise(W, H, seed0)] + [fm.noise(W, H, seed0 + 7000 + f) if f == 1 else fm.blocks(W, H, seed0 + 7000 + f) for f in range(1, F)]), k


def strides(w_out):
    aligned = (w_out + 3) // 4 * 4 + 4
    odd = w_out + 1 + ((w_out + 1) % 4 == 0)
    assert aligned % 4 == 0 and odd % 4 != 0
    return aligned, odd


@pytest.mark.parametrize("case", CASES, ids=CID)
def test_plan_scale_matches_the_model_and_the_reference(hip_ctx, case):
    from compv_amd import capi
    W, H, Wo, Ho = case
    S = (W + 7) // 8 * 8 + 8
    valid, k = frames_of(case)
    exp = np.stack([pm.scale(v, Wo, Ho) for v in valid])
    if k is not None:
        assert (exp[0] == A["scale_%d" % k]).all(), "the model against the reference's plane"
    ar = Arena()
    host_in = pad_frames(valid, S, np.random.default_rng(W * 31 + H))
    d_in = ar.new(host_in.size, host_in.reshape(-1))
    ar.keep(d_in, host_in)
    plan = capi.Plan(hip_ctx, W, H, S, F)
    try:
        for So in strides(Wo):
            d_out = ar.new(F * Ho * So + 5)          # 5 bytes behind the last frame
            plan.scale(ptr(d_in), ptr(d_out), Wo, Ho, So)
            ar.check("scale %s So %d" % (CID(case), So))
            got = d_out.cpu().numpy()
            body = got[:F * Ho * So].reshape(F, Ho, So)
            assert (body[:, :, :Wo] == exp).all(), "So %d" % So
            assert (body[:, :, Wo:] == SENTINEL).all() and (got[F * Ho * So:] == SENTINEL).all(), "So %d: padding or tail written" % So
            if k is not None:
                assert (body[0, :, :Wo] == A["scale_%d" % k]).all(), "the device against the reference's plane"
            plan.scale(ptr(d_in), ptr(d_out), Wo, Ho, So)          # twice: the same bytes
            ar.check("scale again")
            assert (d_out.cpu().numpy() == got).all()
    finally:
        plan.close()


def test_refusals_leave_the_destination_alone(hip_ctx):
    from compv_amd import capi
    W, H, S = 300, 8, 304
    ar = Arena()
    d_in = ar.new(F * H * S, 17)
    d_out = ar.new(4096)
    plan = capi.Plan(hip_ctx, W, H, S, F)
    try:
        for (Wo, Ho, So) in ((1, 8, 4), (0, 8, 4), (8, 0, 8), (300, 8, 296)):          # a ratio of 300, a zero width, a zero height, Sout < Wout
            with pytest.raises(capi.CompvHipError) as e:
                plan.scale(ptr(d_in), ptr(d_out), Wo, Ho, So)
            assert e.value.code == capi.E_INVALID_PARAMETER, (Wo, Ho, So)
        with pytest.raises(capi.CompvHipError) as e:
            plan.scale(ptr(d_in), 0, 8, 8, 8)
        assert e.value.code == capi.E_INVALID_PARAMETER
        with pytest.raises(capi.CompvHipError) as e:          # 255.99 passes, 256 does not: 2 x 512 rows to 2 x 2
            hip_ctx.scale(np.zeros((512, 8), np.uint8), 8, 2)
        assert e.value.code == capi.E_INVALID_PARAMETER
        ar.check("refusals")
        assert (d_out.cpu().numpy() == SENTINEL).all()
    finally:
        plan.close()


@pytest.mark.parametrize("case", DOWN + UP[:1] + SAME, ids=CID)
def test_host_entry(hip_ctx, case):
    W, H, Wo, Ho = case
    valid, k = frames_of(case)
    wide = np.full((H, W + 5), 201, np.uint8)          # a host plane with a stride of its own
    wide[:, :W] = valid[0]
    got = hip_ctx.scale(wide[:, :W], Wo, Ho)
    assert got.shape == (Ho, Wo) and (got == pm.scale(valid[0], Wo, Ho)).all()
    if k is not None:
        assert (got == A["scale_%d" % k]).all()
