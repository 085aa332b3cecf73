"""GPU image statistics (compvhip_plan_integral / _histogram / _equalize / _projections and their host forms) against tests/stats_model.py on every frame
and against the fixtures of tests/golden/golden_stats.* on frame 0, by bit pattern: nothing here is compared with a tolerance.

Harness of tests/gpu_support.py: every device buffer sits between two guards; the outputs start filled with a sentinel, so every element the
definition defines must be written and every other one must keep it (columns > W of the integral images, columns >= W of the equalised frames); the frames'
padding columns [W, S) hold seeded random bytes and the frames must come back unchanged.  Every call is made twice and must repeat itself byte for byte.
Three frames per case, S > W.

The numbers the shapes are chosen from (compv_amd/csrc/kernels.hpp): the integral kernel walks tiles of kStatsTile = 64 columns, one wave per band of
kStatsBandRows = 16 rows; the band-sums kernel gives a thread four columns, one wave up to 256 columns, kStatsThreads = 256 threads = 1024 columns at a
time beyond; the histogram and the equalisation kernel cut a frame into chunks of at least 16 rows, which the 4 waves of a workgroup walk row by row, four
pixels per lane = 256 columns at a time.  So: 65 x 3 and 64 x 33 (one past / exactly a 64-column tile, one row past two bands), 33 x 17 (one past a band
and a 16-row chunk), 257 x 66 (one past 256 columns), 7 x 5 (one past the 4 waves), 521 x 19 / 19 x 521 / 1030 x 70 (several tiles, 33 bands and chunks,
past 1024 columns); W % 4 = 1, 2, 3 (37, 1030, 19) for the last, partial group of four pixels.  Frames on a dword boundary take the dword loads (and
stores), frames 3 bytes into their buffer the byte ones.

A plan has at least 3 x 3 pixels (compvhip_plan_create), so 1 x 1, 1 x 300 and 300 x 1 -- which these calls accept -- go through the host forms, which
need no plan: host arrays pre-filled with the sentinel, host strides beyond W, twice, against model and fixture."""
import ctypes as C

import numpy as np
import pytest

import stats_cases as sc
import stats_model as sm
from fixtures import load_golden, md5
from gpu_support import Arena, SENTINEL, pad_frames, ptr

pytestmark = pytest.mark.gpu

PLAN_CASES = [c["id"] for c in sc.CASES if c["W"] >= 3 and c["H"] >= 3]
HOST_ONLY = [c["id"] for c in sc.CASES if c["W"] < 3 or c["H"] < 3]
OTHER = {"const0": ("const255", 0), "const255": ("ramp", 3), "ramp": ("text", 2), "noise": ("text", 2), "text": ("noise", 3)}          # frame 1 of a case, by its kind
F64_SENTINEL = np.frombuffer(bytes([SENTINEL]) * 8, np.uint64)[0]


@pytest.fixture(scope="module")
def golden_stats():
    meta, arrays = load_golden("golden_stats")
    return {c["id"]: c for c in meta["cases"]}, arrays


def frames_of(c):
    """the golden frame, a frame of another kind, one more noise frame"""
    kind, seed = OTHER[c["kind"]]
    return [sc.case_frame(c), sc.frame(kind, c["W"], c["H"], seed), sc.noise(c["W"], c["H"], 7)]


def against_fixture(golden, cid, key, got):
    """frame 0 against what the generator held against the compiled reference: the bytes where they are stored, their MD5 for every case"""
    by_id, arrays = golden
    assert md5(got) == by_id[cid]["md5"][key], "%s: %s differs from the fixture" % (cid, key)
    if by_id[cid]["stored"]:
        a = arrays["%s_%s" % (key, cid)]
        assert a.dtype == got.dtype and a.tobytes() == np.ascontiguousarray(got).tobytes()


class Rig:
    """A plan of len(frames) frames of one size and its guarded buffers"""
    PAD = 6          # the widest sumStride in use: W + PAD

    def __init__(self, hip_ctx, frames, misalign=0):
        from compv_amd import capi
        self.ctx = hip_ctx
        self.frames = frames
        self.F, (self.H, self.W) = len(frames), frames[0].shape
        F, W, H = self.F, self.W, self.H
        self.S = (W + 7) // 8 * 8 + 8          # S > W, and S % 8 == 0 as a plan asks
        self.host = pad_frames(np.stack(frames), self.S, np.random.default_rng(W * 31 + H))
        self.ar = Arena()
        # misalign: the frames start that many bytes into their buffer (the bytes in front and behind are junk), so no row is dword aligned
        self.misalign = misalign
        raw = np.concatenate([np.full(misalign, 0xEE, np.uint8), self.host.reshape(-1), np.full((8 - misalign) % 8, 0xEE, np.uint8)])
        self.d_raw = self.ar.new(raw.size, raw)
        self.ar.keep(self.d_raw, raw)
        self.gray_ptr = ptr(self.d_raw) + misalign
        self.d_sum = self.ar.new(F * (H + 1) * (W + self.PAD) * 8)
        self.d_sumsq = self.ar.new(F * (H + 1) * (W + self.PAD) * 8)
        self.d_hist = self.ar.new(F * 256 * 4)
        self.d_lut = self.ar.new(F * 256)
        self.d_px = self.ar.new(F * W * 4)
        self.d_py = self.ar.new(F * H * 4)
        # the equalised frames: out of place, with the same offset as the frames; in place, a second copy of the frames that the calls may rewrite
        self.d_out = self.ar.new(raw.size)
        self.d_inplace = self.ar.new(raw.size, raw)
        self.raw = raw
        self.plan = capi.Plan(hip_ctx, W, H, self.S, F)
        self.model = None

    def close(self):
        self.plan.close()

    def expect(self):
        """the model's arrays per frame, computed once"""
        if self.model is None:
            self.model = [dict(zip(("sum", "sumsq"), sm.integral(f)), hist=sm.histogram(f), **dict(zip(("projX", "projY"), sm.projections(f)))) for f in self.frames]
        return self.model

    # ---- integral ----
    def integral(self, what, want_sum=True, want_sumsq=True, pad=1, expect=None):
        """pad: sumStride = W + pad.  Returns the bytes of both buffers."""
        F, W, H = self.F, self.W, self.H
        stride = W + pad
        exp = self.expect() if expect is None else expect
        self.ar.refill(self.d_sum)
        self.ar.refill(self.d_sumsq)
        self.plan.integral(self.gray_ptr, ptr(self.d_sum) if want_sum else 0, ptr(self.d_sumsq) if want_sumsq else 0, stride)
        self.ar.check(what)
        n = F * (H + 1) * stride
        for key, body, wanted in (("sum", self.d_sum, want_sum), ("sumsq", self.d_sumsq, want_sumsq)):
            got = body.cpu().numpy().view(np.uint64)
            if not wanted:
                assert (got == F64_SENTINEL).all(), "%s: %s was written without being passed" % (what, key)
                continue
            assert (got[n:] == F64_SENTINEL).all(), "%s: %s written behind the last frame" % (what, key)
            got = got[:n].reshape(F, H + 1, stride)
            assert (got[:, :, W + 1:] == F64_SENTINEL).all(), "%s: %s written at columns > W" % (what, key)
            for f in range(F):
                e = exp[f][key] if isinstance(exp[f], dict) else exp[f]
                bad = np.argwhere(got[f, :, :W + 1] != np.ascontiguousarray(e, np.float64).view(np.uint64))
                assert bad.size == 0, "%s: frame %d, %d elements of %s differ, first at (y, x) = %s" % (what, f, len(bad), key, tuple(bad[0]))
        return self.d_sum.cpu().numpy().tobytes() + self.d_sumsq.cpu().numpy().tobytes()

    def frame0_integral(self, key, pad=1):
        body = self.d_sum if key == "sum" else self.d_sumsq
        return body.cpu().numpy().view(np.float64)[:(self.H + 1) * (self.W + pad)].reshape(self.H + 1, self.W + pad)[:, :self.W + 1]

    # ---- histogram ----
    def histogram(self, what):
        self.ar.refill(self.d_hist)
        self.plan.histogram(self.gray_ptr, ptr(self.d_hist))
        self.ar.check(what)
        got = self.d_hist.cpu().numpy().view(np.uint32).reshape(self.F, 256)
        for f, e in enumerate(self.expect()):
            assert got[f].tobytes() == e["hist"].tobytes(), "%s: frame %d" % (what, f)
        return got

    # ---- projections ----
    def projections(self, what, want_x=True, want_y=True):
        self.ar.refill(self.d_px)
        self.ar.refill(self.d_py)
        self.plan.projections(self.gray_ptr, ptr(self.d_px) if want_x else 0, ptr(self.d_py) if want_y else 0)
        self.ar.check(what)
        px = self.d_px.cpu().numpy().view(np.int32).reshape(self.F, self.W)
        py = self.d_py.cpu().numpy().view(np.int32).reshape(self.F, self.H)
        pad = np.frombuffer(bytes([SENTINEL]) * 4, np.int32)[0]
        for f, e in enumerate(self.expect()):
            assert px[f].tobytes() == e["projX"].tobytes() if want_x else (px == pad).all(), "%s: projX, frame %d" % (what, f)
            assert py[f].tobytes() == e["projY"].tobytes() if want_y else (py == pad).all(), "%s: projY, frame %d" % (what, f)
        return px.tobytes() + py.tobytes()

    # ---- equalisation ----
    def equalize(self, what, hists=None, scale=0.0, in_place=False, lut=True):
        """hists: None (each frame's own) or uint32 (F, 256) of the caller.  Returns (equalised frames (F, H, W), tables (F, 256))."""
        F, W, H, S = self.F, self.W, self.H, self.S
        d_h = 0
        if hists is not None:
            hbuf = self.ar.new(F * 256 * 4, np.ascontiguousarray(hists, np.uint32).view(np.uint8).reshape(-1))
            self.ar.keep(hbuf, np.ascontiguousarray(hists, np.uint32).view(np.uint8))
            d_h = ptr(hbuf)
        self.ar.refill(self.d_lut)
        self.ar.refill(self.d_out)
        if in_place:
            self.d_inplace.copy_(self.d_raw)
        target = self.d_inplace if in_place else self.d_out
        src = (ptr(self.d_inplace) if in_place else ptr(self.d_raw)) + self.misalign
        self.plan.equalize(src, ptr(target) + self.misalign, d_h, scale, ptr(self.d_lut) if lut else 0)
        self.ar.check(what)
        whole = target.cpu().numpy()
        got = whole[self.misalign:self.misalign + F * H * S].reshape(F, H, S)
        # everything but the pixels keeps what it held: the sentinel out of place, the frames' padding (and the junk around them) in place
        before = self.raw if in_place else np.full(self.raw.size, SENTINEL, np.uint8)
        mask = np.ones(self.raw.size, bool)
        m = mask[self.misalign:self.misalign + F * H * S].reshape(F, H, S)
        m[:, :, :W] = False
        assert (whole[mask] == before[mask]).all(), "%s: written at columns >= W or outside the frames" % what
        luts = self.d_lut.cpu().numpy().reshape(F, 256)
        for f, img in enumerate(self.frames):
            e_out, e_lut = sm.equalize(img, None if hists is None else hists[f], scale)
            assert (got[f, :, :W] == e_out).all(), "%s: frame %d" % (what, f)
            assert (luts[f] == e_lut).all() if lut else (luts == SENTINEL).all(), "%s: table of frame %d" % (what, f)
        return got[:, :, :W].copy(), luts.copy()


@pytest.mark.parametrize("cid", PLAN_CASES)
def test_cases_against_model_and_golden(hip_ctx, golden_stats, cid):
    """every case of the fixture list that a plan can hold, all four calls with everything wanted, twice"""
    c = sc.BY_ID[cid]
    rig = Rig(hip_ctx, frames_of(c))
    try:
        first = rig.integral(cid)
        against_fixture(golden_stats, cid, "sum", rig.frame0_integral("sum"))
        against_fixture(golden_stats, cid, "sumsq", rig.frame0_integral("sumsq"))
        assert rig.integral(cid + " (again)") == first
        h = rig.histogram(cid)
        against_fixture(golden_stats, cid, "hist", h[0])
        assert rig.histogram(cid + " (again)").tobytes() == h.tobytes()
        p = rig.projections(cid)
        against_fixture(golden_stats, cid, "projX", rig.d_px.cpu().numpy().view(np.int32)[:rig.W])
        against_fixture(golden_stats, cid, "projY", rig.d_py.cpu().numpy().view(np.int32)[:rig.H])
        assert rig.projections(cid + " (again)") == p
        out, luts = rig.equalize(cid)
        against_fixture(golden_stats, cid, "eq_own", out[0])
        against_fixture(golden_stats, cid, "lut_own", luts[0])
        again = rig.equalize(cid + " (again)")
        assert again[0].tobytes() == out.tobytes() and again[1].tobytes() == luts.tobytes()
    finally:
        rig.close()


@pytest.mark.parametrize("cid", ["noise37x29", "noise65x3", "noise257x66"])
def test_integral_arms(hip_ctx, cid):
    """sum only, sumsq only, both; sumStride = W + 1 and W + 6"""
    c = sc.BY_ID[cid]
    rig = Rig(hip_ctx, frames_of(c))
    try:
        for pad in (1, 6):
            for s, q in ((True, False), (False, True), (True, True)):
                what = "%s sum=%d sumsq=%d stride=W+%d" % (cid, s, q, pad)
                first = rig.integral(what, s, q, pad)
                assert rig.integral(what + " (again)", s, q, pad) == first
    finally:
        rig.close()


@pytest.mark.parametrize("cid", ["noise37x29", "text257x66", "noise33x17"])
def test_equalize_arms(hip_ctx, golden_stats, cid):
    """its own histogram and a caller's, in place and out of place, with and without d_lut, the default scale and a clamped one"""
    c = sc.BY_ID[cid]
    rig = Rig(hip_ctx, frames_of(c))
    given = np.stack([sc.other_hist(c), sm.histogram(sc.noise(c["W"], c["H"], 12)), sm.histogram(rig.frames[0])])
    try:
        for hists in (None, given):
            for scale in (0.0, sc.CLAMP_SCALE):
                for in_place in (False, True):
                    for lut in (True, False):
                        what = "%s hist=%s scale=%g in_place=%d lut=%d" % (cid, "own" if hists is None else "given", scale, in_place, lut)
                        out, luts = rig.equalize(what, hists, scale, in_place, lut)
                        again = rig.equalize(what + " (again)", hists, scale, in_place, lut)
                        assert again[0].tobytes() == out.tobytes() and again[1].tobytes() == luts.tobytes()
                        key = ("eq_clamped" if hists is None else None) if scale else ("eq_own" if hists is None else "eq_given")
                        if key:
                            against_fixture(golden_stats, cid, key, out[0])
                            if lut:
                                against_fixture(golden_stats, cid, key.replace("eq_", "lut_"), luts[0])
        assert sm.lut_unclamped_max(sm.histogram(rig.frames[0]), sc.CLAMP_SCALE, c["W"], c["H"]) >= 256          # the clamp was reached
    finally:
        rig.close()


@pytest.mark.parametrize("cid", ["noise37x29", "noise257x66", "noise19x521"])
def test_projection_arms(hip_ctx, cid):
    """X only, Y only, both"""
    c = sc.BY_ID[cid]
    rig = Rig(hip_ctx, frames_of(c))
    try:
        for x, y in ((True, False), (False, True), (True, True)):
            what = "%s x=%d y=%d" % (cid, x, y)
            first = rig.projections(what, x, y)
            assert rig.projections(what + " (again)", x, y) == first
    finally:
        rig.close()


def test_frames_three_bytes_into_their_buffer(hip_ctx):
    """no row is dword aligned: the byte-load arms of the band-sums, histogram and equalisation kernels (and byte stores of the equalised frames)"""
    for cid in ("noise37x29", "noise257x66", "noise1030x70"):
        c = sc.BY_ID[cid]
        rig = Rig(hip_ctx, frames_of(c), misalign=3)
        try:
            what = cid + " at +3"
            first = rig.integral(what)
            assert rig.integral(what + " (again)") == first
            rig.histogram(what)
            rig.projections(what)
            rig.equalize(what)
            rig.equalize(what + " in place", in_place=True)
        finally:
            rig.close()


def test_sumsq_beyond_2_to_32(hip_ctx):
    """600 x 400 pixels of 255, sumsq only: its last element is 65 025 * 240 000 > 2^32"""
    W, H = 600, 400
    frames = [sc.const255(W, H)] * 3
    rig = Rig(hip_ctx, frames)
    try:
        q = 65025.0 * np.outer(np.arange(H + 1), np.arange(W + 1))
        assert q[-1, -1] > 2 ** 32
        first = rig.integral("600x400 of 255", False, True, 1, expect=[q] * 3)
        assert rig.integral("600x400 of 255 (again)", False, True, 1, expect=[q] * 3) == first
    finally:
        rig.close()


def test_sum_beyond_2_to_32(hip_ctx):
    """one 5000 x 3400 frame of 255, sum only: its last element is 4 335 000 000 > 2^32"""
    W, H = 5000, 3400
    rig = Rig(hip_ctx, [sc.const255(W, H)])
    try:
        s = 255.0 * np.outer(np.arange(H + 1), np.arange(W + 1))
        assert s[-1, -1] == 4335000000.0
        first = rig.integral("5000x3400 of 255", True, False, 1, expect=[s])
        assert rig.integral("5000x3400 of 255 (again)", True, False, 1, expect=[s]) == first
    finally:
        rig.close()


def test_a_batch_beyond_65535_frames_is_sliced(hip_ctx):
    """65 537 frames of 8 x 3 (S = 8) through all four plan calls.  The frames repeat four patterns and the last frame is a fifth, so EVERY frame is
    compared: the last of the first slice (65 534), the first of the second (65 535) and the one beyond (65 536) are all in the comparison"""
    from compv_amd import capi
    F, W, H, S = 65537, 8, 3, 8
    pats = [sc.noise(W, H, 21), sc.text(W, H, 22), sc.ramp(W, H, 5), sc.noise(W, H, 23), sc.noise(W, H, 24)]
    which = np.arange(F) % 4
    which[-1] = 4
    host = np.stack(pats)[which]          # (F, H, W), S == W
    ar = Arena()
    d_gray = ar.new(host.size, host.reshape(-1))
    ar.keep(d_gray, host)
    d_sum, d_sumsq = ar.new(F * (H + 1) * (W + 1) * 8), ar.new(F * (H + 1) * (W + 1) * 8)
    d_hist, d_out, d_lut = ar.new(F * 256 * 4), ar.new(F * H * S), ar.new(F * 256)
    d_px, d_py = ar.new(F * W * 4), ar.new(F * H * 4)
    exp_int = [sm.integral(p) for p in pats]
    exp_hist = np.stack([sm.histogram(p) for p in pats])
    exp_eq = [sm.equalize(p) for p in pats]
    exp_proj = [sm.projections(p) for p in pats]
    plan = capi.Plan(hip_ctx, W, H, S, F)
    try:
        for rep in range(2):
            for b in (d_sum, d_sumsq, d_hist, d_out, d_lut, d_px, d_py):
                ar.refill(b)
            plan.integral(ptr(d_gray), ptr(d_sum), ptr(d_sumsq), W + 1)
            plan.histogram(ptr(d_gray), ptr(d_hist))
            plan.equalize(ptr(d_gray), ptr(d_out), d_lut=ptr(d_lut))
            plan.projections(ptr(d_gray), ptr(d_px), ptr(d_py))
            ar.check("65537 frames")
            s = d_sum.cpu().numpy().view(np.uint64).reshape(F, -1)
            q = d_sumsq.cpu().numpy().view(np.uint64).reshape(F, -1)
            assert (s == np.stack([e[0].view(np.uint64).reshape(-1) for e in exp_int])[which]).all()
            assert (q == np.stack([e[1].view(np.uint64).reshape(-1) for e in exp_int])[which]).all()
            assert (d_hist.cpu().numpy().view(np.uint32).reshape(F, 256) == exp_hist[which]).all()
            assert (d_out.cpu().numpy().reshape(F, H, S) == np.stack([e[0] for e in exp_eq])[which]).all()
            assert (d_lut.cpu().numpy().reshape(F, 256) == np.stack([e[1] for e in exp_eq])[which]).all()
            assert (d_px.cpu().numpy().view(np.int32).reshape(F, W) == np.stack([e[0] for e in exp_proj])[which]).all()
            assert (d_py.cpu().numpy().view(np.int32).reshape(F, H) == np.stack([e[1] for e in exp_proj])[which]).all()
    finally:
        plan.close()


def test_histogram_then_otsu_on_the_same_plan(hip_ctx, oracle):
    """histogram -> compvhip_plan_otsu -> histogram: the Otsu levels equal the oracle's as before, the histogram equals the model before and after"""
    c = sc.BY_ID["text257x66"]
    rig = Rig(hip_ctx, frames_of(c))
    try:
        d_otsu = rig.ar.new(rig.F * 4)
        before = rig.histogram("before otsu")
        rig.plan.otsu(rig.gray_ptr, ptr(d_otsu))
        rig.ar.check("otsu")
        assert d_otsu.cpu().numpy().view(np.int32).tolist() == [int(oracle.otsu(f)) for f in rig.frames]
        assert rig.histogram("after otsu").tobytes() == before.tobytes()
        rig.plan.otsu(rig.gray_ptr, ptr(d_otsu))
        rig.ar.check("otsu (again)")
        assert d_otsu.cpu().numpy().view(np.int32).tolist() == [int(oracle.otsu(f)) for f in rig.frames]
    finally:
        rig.close()


def test_timing_names_every_kernel_on_a_stream(hip_ctx):
    import torch
    c = sc.BY_ID["noise37x29"]
    rig = Rig(hip_ctx, frames_of(c))
    try:
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        rig.plan.set_timing(1)
        names = lambda: [n for n, _ in rig.plan.get_timing()]          # noqa: E731
        rig.plan.integral(rig.gray_ptr, ptr(rig.d_sum), ptr(rig.d_sumsq), rig.W + 1, stream=st.cuda_stream)
        st.synchronize()
        assert names() == ["stats_band_sums_kernel", "stats_band_scan_kernel", "stats_integral_kernel"]
        rig.plan.histogram(rig.gray_ptr, ptr(rig.d_hist), stream=st.cuda_stream)
        st.synchronize()
        assert names() == ["stats_hist_kernel", "stats_hist_finish_kernel"]
        rig.plan.equalize(rig.gray_ptr, ptr(rig.d_out), stream=st.cuda_stream)
        st.synchronize()
        assert names() == ["stats_hist_kernel", "stats_hist_finish_kernel", "stats_equalize_kernel"]
        rig.plan.equalize(rig.gray_ptr, ptr(rig.d_out), d_hist=ptr(rig.d_hist), stream=st.cuda_stream)
        st.synchronize()
        assert names() == ["stats_hist_finish_kernel", "stats_equalize_kernel"]
        rig.plan.projections(rig.gray_ptr, ptr(rig.d_px), ptr(rig.d_py), stream=st.cuda_stream)
        st.synchronize()
        assert names() == ["stats_band_sums_kernel", "stats_band_scan_kernel"]
        rig.plan.projections(rig.gray_ptr, 0, ptr(rig.d_py), stream=st.cuda_stream)
        st.synchronize()
        assert names() == ["stats_band_sums_kernel"]
        rig.plan.set_timing(0)
        rig.ar.check("timing")
    finally:
        rig.close()


def test_refusals_write_nothing(hip_ctx):
    """each on a live plan with valid buffers: COMPVHIP_E_INVALID_PARAMETER, the reason in compvhip_last_error, the outputs keep the sentinel, nothing is
    allocated"""
    from compv_amd import capi
    c = sc.BY_ID["noise37x29"]
    rig = Rig(hip_ctx, frames_of(c))
    outs = (rig.d_sum, rig.d_sumsq, rig.d_hist, rig.d_lut, rig.d_px, rig.d_py, rig.d_out)
    W = rig.W

    def refused(reason, call, *args, **kw):
        with pytest.raises(capi.CompvHipError) as e:
            call(*args, **kw)
        assert e.value.code == capi.E_INVALID_PARAMETER and reason in hip_ctx.last_error(), (reason, hip_ctx.last_error())
        rig.ar.check(reason)
        for b in outs:
            assert (b.cpu().numpy() == SENTINEL).all(), reason

    try:
        start = hip_ctx.live_allocations()
        g, p = rig.gray_ptr, rig.plan
        refused("both outputs are NULL", p.integral, g, 0, 0, W + 1)
        refused("sumStride below W + 1", p.integral, g, ptr(rig.d_sum), ptr(rig.d_sumsq), W)
        refused("both outputs are NULL", p.projections, g, 0, 0)
        refused("null frame", p.integral, 0, ptr(rig.d_sum), ptr(rig.d_sumsq), W + 1)
        refused("null frame", p.histogram, 0, ptr(rig.d_hist))
        refused("null frame", p.equalize, 0, ptr(rig.d_out))
        refused("null frame", p.projections, 0, ptr(rig.d_px), ptr(rig.d_py))
        refused("null output", p.equalize, g, 0)
        refused("null output", p.histogram, g, 0)
        refused("8-byte aligned", p.integral, g, ptr(rig.d_sum) + 4, 0, W + 1)
        refused("4-byte aligned", p.projections, g, ptr(rig.d_px) + 2, 0)
        refused("not a finite float32", p.equalize, g, ptr(rig.d_out), scale=float("nan"))
        refused("not a finite float32", p.equalize, g, ptr(rig.d_out), scale=1e300)
        assert hip_ctx.live_allocations() == start          # a refusal allocates nothing
        first = rig.integral("after the refusals")
        assert rig.integral("after the refusals (again)") == first
        grown = hip_ctx.live_allocations()
        assert grown == start + 2          # the two column-sum planes, once
        rig.projections("after the refusals")
        assert hip_ctx.live_allocations() == grown          # projX reuses the first of them
    finally:
        rig.close()


def host_all(hip_ctx, img, hist):
    """every host form on one frame; host strides beyond W where the binding takes one"""
    H, W = img.shape
    wide = np.full((H, W + 11), 0x3C, np.uint8)          # a host stride beyond W
    wide[:, :W] = img
    src = wide[:, :W]
    s, q = hip_ctx.integral(src, sum_stride=W + 4)
    px, py = hip_ctx.projections(src)
    own, lut_own = hip_ctx.equalize(src, out_stride=W + 5)
    given, lut_given = hip_ctx.equalize(src, hist)
    clamped, lut_clamped = hip_ctx.equalize(src, None, sc.CLAMP_SCALE)
    return dict(sum=s, sumsq=q, hist=hip_ctx.histogram(src), eq_own=own, eq_given=given, projX=px, projY=py, lut_own=lut_own, lut_given=lut_given,
                eq_clamped=clamped, lut_clamped=lut_clamped)


@pytest.mark.parametrize("cid", HOST_ONLY)
def test_shapes_below_a_plans_minimum_through_the_host_forms(hip_ctx, golden_stats, cid):
    """1 x 1, 1 x 300, 300 x 1: twice, against the fixture (and so the model)"""
    c = sc.BY_ID[cid]
    img, hist = sc.case_frame(c), sc.other_hist(c)
    first = host_all(hip_ctx, img, hist)
    for k, v in first.items():
        against_fixture(golden_stats, cid, k, np.ascontiguousarray(v))
    again = host_all(hip_ctx, img, hist)
    assert all(np.ascontiguousarray(again[k]).tobytes() == np.ascontiguousarray(v).tobytes() for k, v in first.items())


def test_host_forms_equal_the_plan_forms(hip_ctx):
    """each _u8 call on 37 x 29 noise with So != S equals the plan form (frame 0 of the rig), and the host outputs are written only where defined"""
    from compv_amd import capi
    c = sc.BY_ID["noise37x29"]
    rig = Rig(hip_ctx, frames_of(c))
    W, H = rig.W, rig.H
    try:
        img, hist = rig.frames[0], sc.other_hist(c)
        host = host_all(hip_ctx, img, hist)
        rig.integral("plan")
        assert np.ascontiguousarray(host["sum"]).tobytes() == np.ascontiguousarray(rig.frame0_integral("sum")).tobytes()
        assert np.ascontiguousarray(host["sumsq"]).tobytes() == np.ascontiguousarray(rig.frame0_integral("sumsq")).tobytes()
        assert host["hist"].tobytes() == rig.histogram("plan")[0].tobytes()
        rig.projections("plan")
        assert host["projX"].tobytes() == rig.d_px.cpu().numpy()[:W * 4].tobytes() and host["projY"].tobytes() == rig.d_py.cpu().numpy()[:H * 4].tobytes()
        out, luts = rig.equalize("plan")
        assert (host["eq_own"] == out[0]).all() and (host["lut_own"] == luts[0]).all()
        out, luts = rig.equalize("plan, given", np.stack([hist] * 3))
        assert (host["eq_given"] == out[0]).all() and (host["lut_given"] == luts[0]).all()
        out, luts = rig.equalize("plan, clamped", None, sc.CLAMP_SCALE)
        assert (host["eq_clamped"] == out[0]).all() and (host["lut_clamped"] == luts[0]).all()
        # the raw calls: strides beyond the width, sentinels behind the defined elements, one output at a time
        lib, h = hip_ctx.lib, hip_ctx.h
        s = np.full((H + 1, W + 4), -7.0)
        assert lib.compvhip_integral_u8(h, img.ctypes.data, W, H, W, s.ctypes.data, None, W + 4) == capi.OK
        assert (s[:, :W + 1] == sm.integral(img)[0]).all() and (s[:, W + 1:] == -7.0).all()
        assert lib.compvhip_integral_u8(h, img.ctypes.data, W, H, W, None, s.ctypes.data, W + 4) == capi.OK
        assert (s[:, :W + 1] == sm.integral(img)[1]).all() and (s[:, W + 1:] == -7.0).all()
        o = np.full((H, W + 5), 0x77, np.uint8)
        assert lib.compvhip_equalize_u8(h, img.ctypes.data, W, H, W, None, C.c_double(-1.0), o.ctypes.data, W + 5, None) == capi.OK
        assert (o[:, :W] == sm.equalize(img)[0]).all() and (o[:, W:] == 0x77).all()
        py = np.full(H, 5, np.int32)
        assert lib.compvhip_projections_u8(h, img.ctypes.data, W, H, W, None, py.ctypes.data) == capi.OK and (py == sm.projections(img)[1]).all()
        # refusals
        bad = capi.E_INVALID_PARAMETER
        assert lib.compvhip_integral_u8(h, img.ctypes.data, W, H, W, None, None, W + 1) == bad
        assert lib.compvhip_integral_u8(h, img.ctypes.data, W, H, W, s.ctypes.data, None, W) == bad
        assert lib.compvhip_integral_u8(h, None, W, H, W, s.ctypes.data, None, W + 4) == bad
        assert lib.compvhip_integral_u8(h, img.ctypes.data, W, H, W - 1, s.ctypes.data, None, W + 4) == bad
        assert lib.compvhip_integral_u8(h, img.ctypes.data, 0, H, W, s.ctypes.data, None, W + 4) == bad
        assert lib.compvhip_projections_u8(h, img.ctypes.data, W, H, W, None, None) == bad
        assert lib.compvhip_histogram_u8(h, img.ctypes.data, W, H, W, None) == bad
        assert lib.compvhip_equalize_u8(h, img.ctypes.data, W, H, W, None, C.c_double(-1.0), None, W, None) == bad
        assert lib.compvhip_equalize_u8(h, img.ctypes.data, W, H, W, None, C.c_double(-1.0), o.ctypes.data, W - 1, None) == bad
        assert (s[:, W + 1:] == -7.0).all() and (o[:, W:] == 0x77).all()
    finally:
        rig.close()
