"""GPU parity of the optional Gaussian pre-blur through the C ABI: compvhip_convlt1_fixedpoint_u8 and the plan
variant against the oracle (pinned to the compiled reference and to the reference's own golden by tests/test_gauss_oracle.py)."""
import numpy as np
import pytest

from gauss_cases import CASE0_KERNEL_LITERAL, case0_input, convlt_inputs
from gpu_support import SENTINEL, Arena, frames_view, pad_frames, ptr
from oracle_bindings import md5_rows, synth_frame

pytestmark = pytest.mark.gpu


def test_reference_known_answer_case0_on_gpu(hip_ctx):
    """unittests/math_convlt.cxx:21 (case 0): the reference's own MD5 for the fixed-point convolution, computed by the HIP path."""
    kern = np.array(CASE0_KERNEL_LITERAL[:7], np.uint16)
    out = hip_ctx.convlt_fixedpoint(case0_input(), kern, kern)
    assert md5_rows(out) == "2678b73a89681f12fb474dd8102fc37c"


@pytest.mark.parametrize("W,H,S", [(16, 16, 64), (64, 16, 64), (333, 77, 384), (641, 130, 704), (1920, 70, 1920), (2049, 65, 2112)])
@pytest.mark.parametrize("size", [3, 5, 7, 9, 11, 13, 15])
def test_convlt_fixedpoint_matches_oracle(hip_ctx, oracle, W, H, S, size):
    rng = np.random.default_rng(W * 31 + size)
    buf = np.zeros((H, S), np.uint8)
    buf[:, :W] = rng.integers(0, 256, (H, W), dtype=np.uint8)
    img = buf[:, :W]
    for kern in (oracle.gauss_kernel_fxp(size, 0.3 * size), rng.integers(0, 65536 // size, size).astype(np.uint16), np.full(size, 65535, np.uint16)):
        vt, hz = kern, kern[::-1].copy()
        rc, exp = oracle.convlt_fxp(img, vt, hz)
        assert rc == 0
        got = hip_ctx.convlt_fixedpoint(img, vt, hz)
        assert (got == exp).all(), int((got != exp).sum())


def test_convlt_fixedpoint_errors(hip_ctx):
    from compv_amd import capi
    img = np.zeros((32, 32), np.uint8)
    with pytest.raises(capi.CompvHipError) as e:
        hip_ctx.convlt_fixedpoint(img, [1, 2, 3, 4], [1, 2, 3, 4])           # even size (compv_math_convlt.h:100)
    assert e.value.code == capi.E_INVALID_PARAMETER
    with pytest.raises(capi.CompvHipError) as e:
        hip_ctx.convlt_fixedpoint(np.zeros((4, 32), np.uint8), [1] * 5, [1] * 5)   # H < kernel
    assert e.value.code == capi.E_INVALID_PARAMETER
    with pytest.raises(capi.CompvHipError) as e:
        hip_ctx.convlt_fixedpoint(img, [1] * 17, [1] * 17)                   # > 15 taps
    assert e.value.code == capi.E_NOT_IMPLEMENTED


def test_plan_blur_then_canny_batch(hip_ctx, oracle):
    """Gaussian(5, sigma 1) -> Canny on a 4-frame batch on the device, in place, against the oracle chain."""
    import torch
    from compv_amd import capi
    W, H, S, F = 1282, 720, 1344, 4
    dev = torch.device("cuda", 0)
    frames = np.zeros((F, H, S), np.uint8)
    kern = capi.gauss_kernel_fixedpoint(5, 1.0)
    assert kern.tolist() == oracle.gauss_kernel_fxp(5, 1.0).tolist()
    exp = []
    for f in range(F):
        frames[f, :, :W] = synth_frame(W, H, 4321 + f)
        rc, b = oracle.convlt_fxp(frames[f][:, :W], kern, kern)
        rc2, e = oracle.canny(np.ascontiguousarray(b), 30.0, 70.0)
        assert rc == 0 and rc2 == 0
        exp.append((b, e))
    d = torch.from_numpy(frames).to(dev)
    d_edges = torch.empty_like(d)
    plan = capi.Plan(hip_ctx, W, H, S, F, 1.0)
    try:
        d_blur = torch.zeros_like(d)                                           # the kernels write the W valid columns only: keep the stride padding defined
        plan.convlt_fixedpoint(d.data_ptr(), kern, kern, d_blur.data_ptr())   # out of place: fused single-kernel path
        plan.convlt_fixedpoint(d.data_ptr(), kern, kern, d.data_ptr())        # in place: two passes through the plan's scratch
        torch.cuda.synchronize()
        assert torch.equal(d_blur, d)
        plan.canny(d.data_ptr(), 30.0, 70.0, d_edges.data_ptr())
        torch.cuda.synchronize()
        b = d.cpu().numpy(); e = d_edges.cpu().numpy()
        for f in range(F):
            assert (b[f][:, :W] == exp[f][0]).all(), f
            assert (e[f][:, :W] == exp[f][1]).all(), f
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------
# the plan form at every kernel size: the fused kernel on batches and the two-pass path (convlt_fxp_hz_kernel<K> then convlt_fxp_vt_kernel<K>),
# which launch_convlt_fxp takes only when the input and output spans overlap.  Buffers come from the Arena of tests/gpu_support.py.
#
# Geometries (W, H, S, F) from the kernels' seams: 8 pixels per thread, 256 threads = 2048 columns per workgroup, kFxpRows = 64 output rows per
# workgroup, the right-hand load clamped to S - 8, the row clamp at 0 and H - 1.
# ---------------------------------------------------------------------------------------------------------------
FXP_SIZES = (3, 5, 7, 9, 11, 13, 15)
FXP_GEOMETRIES = ((15, 15, 16, 2),          # W = H = the largest K: one non-zero pixel per frame at K = 15; a single group
                  (16, 17, 24, 3),          # two groups, the stride holds a third that is all padding
                  (23, 64, 32, 2),          # exactly one row block; W % 8 == 7
                  (41, 65, 48, 3),          # one row past a row block; S - W == 7: the last group's right load is clamped
                  (2049, 23, 2056, 2),      # one column past a workgroup's 2048; clamped last group
                  (2041, 129, 2112, 2))     # S - W >= 64; two row blocks and one row
FXP_OVERLAP_GEOMETRIES = (FXP_GEOMETRIES[3], FXP_GEOMETRIES[4])
FXP_ID = lambda v: "%dx%d_S%d_F%d" % v if isinstance(v, tuple) else "K%d" % v          # noqa: E731
_fxp_cases = {}


def one_hot(K, tap):
    k = np.zeros(K, np.uint16)
    k[tap] = 65535
    return k


def shifted_minus_two(valid, r, dx, dy):
    """What a one-hot pair of weights 65535 makes of a batch: (b * 65535) >> 16 = b - 1 for b >= 1, once per pass, so the interior holds
    max(in[y + dy][x + dx] - 2, 0) and the border of r pixels is zero"""
    F, H, W = valid.shape
    out = np.zeros_like(valid)
    src = valid[:, r + dy:H - r + dy, r + dx:W - r + dx].astype(np.int32)
    out[:, r:H - r, r:W - r] = np.maximum(src - 2, 0).astype(np.uint8)
    return out


def fxp_case(oracle, geom, K):
    """(valid [F][H][W], padded input [F][H][S], [(name, vt, hz, oracle's blur of every frame)]) of one geometry and kernel size, computed once"""
    if (geom, K) not in _fxp_cases:
        W, H, S, F = geom
        rng = np.random.default_rng(W * 131 + H * 17 + K)
        valid = rng.integers(0, 256, (F, H, W), dtype=np.uint8)
        host_in = pad_frames(valid, S, rng)
        gauss = oracle.gauss_kernel_fxp(K, 0.3 * K)
        vt, hz = (rng.integers(0, 65536 // K, K).astype(np.uint16) for _ in range(2))
        assert (vt != hz).any() and (vt != hz[::-1]).any() and int(vt.sum()) <= 65535 and int(hz.sum()) <= 65535
        full = np.full(K, 65535, np.uint16)
        pairs = [("gauss", gauss, gauss), ("random", vt, hz), ("saturating", full, full),
                 ("one-hot", one_hot(K, K - 1), one_hot(K, 0)), ("one-hot mirrored", one_hot(K, 0), one_hot(K, K - 1))]
        out = []
        for name, v, h in pairs:
            exp = []
            for f in range(F):
                rc, e = oracle.convlt_fxp(valid[f], v, h)
                assert rc == 0
                exp.append(e.copy())
            out.append((name, v, h, np.stack(exp)))
        valid.setflags(write=False)
        _fxp_cases[(geom, K)] = (valid, host_in, out)
    return _fxp_cases[(geom, K)]


def fxp_expect(got, exp, what):
    if not (got == exp).all():
        f, y, x = (int(v[0]) for v in np.nonzero(got != exp))
        raise AssertionError("%s: %d pixels differ, first (frame %d, y %d, x %d): got %d, expected %d" % (what, int((got != exp).sum()), f, y, x, got[f, y, x], exp[f, y, x]))


@pytest.mark.parametrize("K", FXP_SIZES, ids=FXP_ID)
@pytest.mark.parametrize("geom", FXP_GEOMETRIES, ids=FXP_ID)
def test_plan_convlt_every_size_out_of_place_and_in_place(hip_ctx, oracle, geom, K):
    """Every kernel size through Plan.convlt_fixedpoint on a batch, out of place (convlt_fxp_fused_kernel<K>, frames > 1) and in place (the
    two-pass path), with five kernel pairs: the Gaussian, random weights with vt != hz, all taps 65535 (saturates in both passes), and two
    one-hot pairs whose result is the input shifted by r columns one way and r rows the other -- which alone tells an axis swap or a reversed
    tap order."""
    import torch
    from compv_amd import capi
    W, H, S, F = geom
    assert W >= K and H >= K
    r = K // 2
    valid, host_in, pairs = fxp_case(oracle, geom, K)
    A = Arena()
    n = F * H * S
    d_in = A.new(n, host_in)
    A.keep(d_in, host_in)
    d_out = A.new(n)
    d_alias = A.new(n)
    flat_in = torch.from_numpy(host_in.reshape(-1).copy())
    plan = capi.Plan(hip_ctx, W, H, S, F)
    directions = {}
    try:
        for name, vt, hz, exp in pairs:
            what = "%s K %d" % (name, K)
            A.refill(d_out)
            plan.convlt_fixedpoint(ptr(d_in), vt, hz, ptr(d_out))
            A.check(what + " out of place")
            got = frames_view(d_out, F, H, S, W)
            fxp_expect(got, exp, what + " out of place")
            d_alias.copy_(flat_in)
            plan.convlt_fixedpoint(ptr(d_alias), vt, hz, ptr(d_alias))
            A.check(what + " in place")
            got_in_place = frames_view(d_alias, F, H, S, W)
            fxp_expect(got_in_place, got, what + " in place against out of place")
            fxp_expect(got_in_place, exp, what + " in place")
            if name.startswith("one-hot"):
                found = [(dx, dy) for dx in (-r, r) for dy in (-r, r) if (shifted_minus_two(valid, r, dx, dy) == exp).all()]          # the oracle's directions
                assert len(found) == 1, (what, found)
                dx, dy = found[0]
                fxp_expect(got, shifted_minus_two(valid, r, dx, dy), what + " shift identity, out of place")
                fxp_expect(got_in_place, shifted_minus_two(valid, r, dx, dy), what + " shift identity, in place")
                directions[name] = (dx, dy)
            if name == "saturating":
                assert (exp[:, r:H - r, r:W - r] == 255).mean() > 0.9
        assert directions["one-hot mirrored"] == (-directions["one-hot"][0], -directions["one-hot"][1]) and directions["one-hot"][0] == -directions["one-hot"][1]
    finally:
        plan.close()


@pytest.mark.parametrize("K", FXP_SIZES, ids=FXP_ID)
@pytest.mark.parametrize("geom", FXP_OVERLAP_GEOMETRIES, ids=FXP_ID)
def test_plan_convlt_partly_overlapping_and_touching_spans(hip_ctx, oracle, geom, K):
    """The alias tests of compvhip_plan_convlt1_fixedpoint and launch_convlt_fxp: the output span one frame behind the input span and one frame
    in front of it (both overlap: two passes, the output is the blur of the ORIGINAL frames), and the two spans touching (no overlap: the
    fused kernel, no scratch)."""
    import torch
    from compv_amd import capi
    W, H, S, F = geom
    valid, host_in, pairs = fxp_case(oracle, geom, K)
    name, vt, hz, exp = pairs[1]
    assert name == "random"
    one = H * S
    flat_in = torch.from_numpy(host_in.reshape(-1).copy())
    torch.cuda.synchronize()
    start = hip_ctx.live_allocations()
    A = Arena()
    d = A.new((F + 1) * one)
    d2 = A.new(2 * F * one)
    plan = capi.Plan(hip_ctx, W, H, S, F)
    try:
        base = hip_ctx.live_allocations()
        # touching: [0, F) -> [F, 2F)
        d2[:F * one].copy_(flat_in)
        plan.convlt_fixedpoint(ptr(d2), vt, hz, ptr(d2) + F * one)
        A.check("touching")
        assert hip_ctx.live_allocations() == base          # no overlap: no two-pass scratch
        assert (d2[:F * one].cpu().numpy() == host_in.reshape(-1)).all(), "touching: input modified"
        fxp_expect(frames_view(d2[F * one:], F, H, S, W), exp, "touching")
        # output one frame behind the input: frames [0, F) -> [1, F + 1)
        d[:F * one].copy_(flat_in)
        plan.convlt_fixedpoint(ptr(d), vt, hz, ptr(d) + one)
        A.check("d_out = d_in + H * S")
        assert hip_ctx.live_allocations() == base + 1
        fxp_expect(frames_view(d[one:], F, H, S, W), exp, "d_out = d_in + H * S")
        assert (d[:one].cpu().numpy() == host_in[0].reshape(-1)).all(), "the input frame outside the output span was written"
        # output one frame in front of the input: frames [1, F + 1) -> [0, F)
        A.refill(d)
        d[one:].copy_(flat_in)
        plan.convlt_fixedpoint(ptr(d) + one, vt, hz, ptr(d))
        A.check("d_out = d_in - H * S")
        assert hip_ctx.live_allocations() == base + 1
        fxp_expect(frames_view(d[:F * one], F, H, S, W), exp, "d_out = d_in - H * S")
        assert (d[F * one:].cpu().numpy() == host_in[F - 1].reshape(-1)).all(), "the input frame outside the output span was written"
    finally:
        plan.close()
    assert hip_ctx.live_allocations() == start


def test_plan_convlt_scratch_is_allocated_by_the_first_in_place_call_only(hip_ctx, oracle):
    import torch
    from compv_amd import capi
    geom, K = FXP_GEOMETRIES[3], 9
    W, H, S, F = geom
    valid, host_in, pairs = fxp_case(oracle, geom, K)
    _, vt, hz, exp = pairs[1]
    torch.cuda.synchronize()
    start = hip_ctx.live_allocations()
    A = Arena()
    n = F * H * S
    d_in = A.new(n, host_in)
    A.keep(d_in, host_in)
    d_out = A.new(n)
    d_alias = A.new(n, host_in)
    plan = capi.Plan(hip_ctx, W, H, S, F)
    try:
        base = hip_ctx.live_allocations()
        plan.convlt_fixedpoint(ptr(d_in), vt, hz, ptr(d_out))
        assert hip_ctx.live_allocations() == base          # a plan that has never gone in place holds no scratch
        plan.convlt_fixedpoint(ptr(d_alias), vt, hz, ptr(d_alias))
        assert hip_ctx.live_allocations() == base + 1          # the two-pass scratch
        A.check("first in-place call")
        fxp_expect(frames_view(d_alias, F, H, S, W), exp, "first in-place call")
        for i in range(2):
            d_alias.copy_(torch.from_numpy(host_in.reshape(-1).copy()))
            plan.convlt_fixedpoint(ptr(d_alias), vt, hz, ptr(d_alias))
            A.refill(d_out)
            plan.convlt_fixedpoint(ptr(d_in), vt, hz, ptr(d_out))
            assert hip_ctx.live_allocations() == base + 1
            A.check("later calls")
            fxp_expect(frames_view(d_alias, F, H, S, W), exp, "later in-place call")
            fxp_expect(frames_view(d_out, F, H, S, W), exp, "later out-of-place call")
    finally:
        plan.close()
    assert hip_ctx.live_allocations() == start


def test_plan_convlt_refusals_write_nothing(hip_ctx):
    from compv_amd import capi

    def code(fn, *a):
        with pytest.raises(capi.CompvHipError) as e:
            fn(*a)
        return e.value.code
    A = Arena()
    W, H, S, F = 20, 20, 24, 2
    d_in, d_out = A.new(F * H * S), A.new(F * H * S)
    plan = capi.Plan(hip_ctx, W, H, S, F)
    narrow = capi.Plan(hip_ctx, 9, 20, 16, 2)
    low = capi.Plan(hip_ctx, 20, 9, 24, 2)
    try:
        i, o = ptr(d_in), ptr(d_out)
        k5 = np.full(5, 1000, np.uint16)

        def raw(vt, hz):          # Plan.convlt_fixedpoint with a kernel pointer of the caller's
            hip_ctx._chk(plan.lib.compvhip_plan_convlt1_fixedpoint(plan.h, i, vt, hz, 5, o, 0))
        for dst in (o, i):          # out of place and in place
            assert code(plan.convlt_fixedpoint, i, [1] * 4, [1] * 4, dst) == capi.E_INVALID_PARAMETER          # even size
            assert code(plan.convlt_fixedpoint, i, [1] * 17, [1] * 17, dst) == capi.E_NOT_IMPLEMENTED          # more than 15 taps
            assert code(narrow.convlt_fixedpoint, i, [1] * 11, [1] * 11, dst) == capi.E_INVALID_PARAMETER          # K > W
            assert code(low.convlt_fixedpoint, i, [1] * 11, [1] * 11, dst) == capi.E_INVALID_PARAMETER          # K > H
        assert code(raw, None, k5.ctypes.data) == capi.E_INVALID_PARAMETER          # null kernel pointers
        assert code(raw, k5.ctypes.data, None) == capi.E_INVALID_PARAMETER
        assert code(plan.convlt_fixedpoint, 0, k5, k5, o) == capi.E_INVALID_PARAMETER          # null frame pointers
        assert code(plan.convlt_fixedpoint, i, k5, k5, 0) == capi.E_INVALID_PARAMETER
        A.check("refusals")
        assert (d_in.cpu().numpy() == SENTINEL).all() and (d_out.cpu().numpy() == SENTINEL).all()
    finally:
        for p in (plan, narrow, low):
            p.close()


def test_plan_convlt_on_a_stream(hip_ctx, oracle):
    """both paths enqueued on a non-default stream"""
    import torch
    from compv_amd import capi
    geom, K = FXP_GEOMETRIES[3], 7
    W, H, S, F = geom
    valid, host_in, pairs = fxp_case(oracle, geom, K)
    _, vt, hz, exp = pairs[1]
    A = Arena()
    n = F * H * S
    d_in = A.new(n, host_in)
    A.keep(d_in, host_in)
    d_out = A.new(n)
    d_alias = A.new(n, host_in)
    plan = capi.Plan(hip_ctx, W, H, S, F)
    try:
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        plan.convlt_fixedpoint(ptr(d_in), vt, hz, ptr(d_out), stream=st.cuda_stream)
        plan.convlt_fixedpoint(ptr(d_alias), vt, hz, ptr(d_alias), stream=st.cuda_stream)
        st.synchronize()
        A.check("on a stream")
        fxp_expect(frames_view(d_out, F, H, S, W), exp, "out of place on a stream")
        fxp_expect(frames_view(d_alias, F, H, S, W), exp, "in place on a stream")
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------
# integer separable correlation: the reference's own known-answer vectors on the GPU
# ---------------------------------------------------------------------------------------------------------------
def test_convlt1_int16_reference_known_answers_on_the_gpu(hip_ctx):
    """unittests/math_convlt.cxx:24-25, cases 5 and 6 (1285x720, stride 1344, k = 7, data (i*j)+53 with alternating signs for the int16
    case): MD5 of the int16 result -- the only reference-held golden vectors on the hot path's operators -- from the HIP kernels."""
    d8, d16, k = convlt_inputs()
    assert md5_rows(hip_ctx.convlt1_i16(d8, k, k)) == "7f1116ade2a1cdb37842084c781ee05e"
    assert md5_rows(hip_ctx.convlt1_i16(d16, k, k)) == "cad2f4d2fd66e171997f39804e667699"


@pytest.mark.parametrize("W,H,K", [(9, 9, 3), (64, 33, 5), (257, 65, 1), (301, 200, 15), (1282, 70, 9)])
def test_convlt1_int16_matches_oracle(hip_ctx, oracle, W, H, K):
    """Generic odd kernel sizes, both input types, saturation included (weights up to +-32767 overflow int16 on purpose), and the gradient
    of the path as two calls: gx = (vt smoothing, hz derivative), gy swapped (canny_dete.cxx:237-241)."""
    from compv_amd import capi
    rng = np.random.default_rng(W * 7 + K)
    img8 = rng.integers(0, 256, (H, W), dtype=np.uint8)
    img16 = rng.integers(-32768, 32768, (H, W), dtype=np.int16)
    for scale in (3, 32767):
        vt = rng.integers(-scale, scale + 1, K).astype(np.int16)
        hz = rng.integers(-scale, scale + 1, K).astype(np.int16)
        rc, exp = oracle.convlt_8u(img8, vt, hz)
        assert rc == 0 and (hip_ctx.convlt1_i16(img8, vt, hz) == exp).all()
        rc, exp = oracle.convlt_16s(img16, vt, hz)
        assert rc == 0 and (hip_ctx.convlt1_i16(img16, vt, hz) == exp).all()
    if K == 3:
        gx_exp, gy_exp, _ = oracle.gradient(img8, 0)
        assert (hip_ctx.convlt1_i16(img8, [1, 2, 1], [-1, 0, 1]) == gx_exp).all()
        assert (hip_ctx.convlt1_i16(img8, [-1, 0, 1], [1, 2, 1]) == gy_exp).all()
    with pytest.raises(capi.CompvHipError) as e:
        hip_ctx.convlt1_i16(img8[:2], [1, 2, 1], [1, 2, 1])          # H < k (compv_math_convlt.h:100)
    assert e.value.code == capi.E_INVALID_PARAMETER
    with pytest.raises(capi.CompvHipError) as e:
        hip_ctx.convlt1_i16(img8, [1, 2], [1, 2])                    # even kernel size
    assert e.value.code == capi.E_INVALID_PARAMETER
