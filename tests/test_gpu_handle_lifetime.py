"""Who frees what: one small plan makes one call per buffer that a handle allocates on first use, then a matcher and an ORB pyramid do the same, and
everything is closed.  compvhip_live_allocations is read after every step.  The handles' members free themselves (compv_amd/csrc/device_memory.hpp), so
closing a handle must give back exactly what it took -- whichever of its first-use buffers exist -- and a second pass over the same calls must reuse every
buffer.  The counts themselves are pinned: the number of device allocations behind a public call is part of what the other tests assert deltas of."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, S, F = 64, 48, 64, 2          # the smallest size that admits ORB's 37 x 37 window, on the smallest legal stride
LINE_CAP, BIG_LINE_CAP, HUGE_LINE_CAP = 256, 1 << 17, 1 << 18
# A plan keeps max(lineCap, 65536) key slots a frame, clamped to R * T accumulator cells.  At theta 1 that is 225 * 180 = 40500 whatever the caller asks for:
# the first plan's "larger lineCap" step reuses its buffers.  The second plan (theta 0.25: 225 * 720 = 162000 cells) is there to GROW them: 65536 slots, then
# 131072 (32 sort chunks of 4096: still the device sort, its chunk histograms grow), then 162000 (40 chunks: past the device sort, whose tables go).
REGROW_THETA = 0.25
SEG_CAP, COMP_CAP, CORNER_CAP, KEY_CAP = 512, 256, 512, 256
Q = 64                               # descriptor rows a side of the matcher

# live_allocations() minus its value at the start, after each step of the sequence below.  Recorded from the commit BEFORE the handles' members became
# self-freeing buffers (every buffer a raw pointer, freed by hand in the destroy functions), with this same test: the refactored tree reproduces them
# exactly.  None = the batched KHT, whose buffers grow with the data and the CPU budget: the count must not fall there.
EXPECTED = {
    "plan": 6, "pipeline": 27, "async step + wait": 27, "packed step, no gray output": 28, "otsu": 30, "blur in place": 31, "canny in place": 32,
    "segments": 33, "fit": 33, "components, byte map, no labels": 36, "adaptive threshold in place": 37, "morph OPEN": 37, "FAST, no score map": 39,
    "ORB keypoints": 40, "ORB describe with blur": 41, "pipeline, larger lineCap": 41, "batched KHT": None,
}
EXPECTED_REGROW = {"plan": 6, "pipeline, 65536 slots": 27, "pipeline, 131072 slots": 27, "pipeline, 162000 slots": 25}
EXPECTED_MATCHER = {"matcher": 2, "knn": 2, "good, cross check": 2}
EXPECTED_PYRAMID = {"pyramid": 5, "detect": 6, "describe": 7}


def frames():
    rng = np.random.RandomState(20240607)
    img = rng.randint(0, 64, (F, H, S)).astype(np.uint8)
    img[:, 8:40, 10:50] += 120          # a bright box: long straight edges, corners
    img[:, 20, :] = 255
    for i in range(40):
        img[:, 4 + i, 12 + i] = 250     # a diagonal
    return img


class Rig:
    def __init__(self, hip_ctx):
        import torch
        from compv_amd import capi
        self.torch, self.capi, self.ctx = torch, capi, hip_ctx
        dev = torch.device("cuda:0")
        z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)   # noqa: E731
        img = frames()
        self.d_in = torch.from_numpy(img).to(dev)
        self.d_packed = torch.from_numpy(np.repeat(img[..., None], 3, axis=3).copy()).to(dev)     # RGB24, [F][H][S] pixels
        self.d_work = z(F * H * S)      # the in-place calls run on this copy
        self.d_tmp = z(F * H * S)
        self.d_edges, self.d_edges2 = z(F * H * S), z(F * H * S)
        self.d_lines, self.d_lines2 = z(F * LINE_CAP * capi.LINE_DTYPE.itemsize), z(F * LINE_CAP * capi.LINE_DTYPE.itemsize)
        self.d_lines_big = z(F * HUGE_LINE_CAP * capi.LINE_DTYPE.itemsize)
        self.d_counts, self.d_counts2 = z(F * 4), z(F * 4)
        self.d_otsu = z(F * 4)
        self.d_segs, self.d_seg_counts = z(F * SEG_CAP * capi.SEGMENT_DTYPE.itemsize), z(F * 4)
        self.d_fits, self.d_fit_counts = z(F * LINE_CAP * capi.LINE_FIT_DTYPE.itemsize), z(F * 4)
        self.d_comps, self.d_comp_counts = z(F * COMP_CAP * capi.COMP_DTYPE.itemsize), z(F * 4)
        self.d_corners, self.d_corner_counts = z(F * CORNER_CAP * capi.CORNER_DTYPE.itemsize), z(F * 4)
        self.d_keys, self.d_key_counts = z(F * KEY_CAP * capi.KEYPOINT_DTYPE.itemsize), z(F * 4)
        self.d_desc = z(F * KEY_CAP * 32)
        rng = np.random.RandomState(7)
        self.d_query = torch.from_numpy(rng.randint(0, 256, (Q, 32)).astype(np.uint8)).to(dev)
        self.d_train = torch.from_numpy(rng.randint(0, 256, (Q, 32)).astype(np.uint8)).to(dev)
        self.d_matches, self.d_good, self.d_good_counts = z(2 * Q * capi.MATCH_DTYPE.itemsize), z(Q * capi.MATCH_DTYPE.itemsize), z(4)
        torch.cuda.synchronize()
        self.gauss = capi.gauss_kernel_fixedpoint(5, 1.0)
        self.strel = capi.morph_strel(capi.STREL_RECT, 3, 3)

    def live(self):
        self.torch.cuda.synchronize()
        return self.ctx.live_allocations()

    def restore_work(self):
        self.d_work.copy_(self.d_in.reshape(-1))

    def plan_calls(self, plan):
        """(name, call): one per buffer the plan allocates on first use"""
        capi, p = self.capi, (lambda t: t.data_ptr())

        def asynchronous():
            plan.wait(plan.pipeline_async(p(self.d_in), 59.0, 119.0, 20, 0, p(self.d_edges), p(self.d_lines), LINE_CAP, p(self.d_counts)))

        def blur():
            self.restore_work()
            plan.convlt_fixedpoint(p(self.d_work), self.gauss, self.gauss, p(self.d_work))

        def canny():
            self.restore_work()
            plan.canny(p(self.d_work), 59.0, 119.0, p(self.d_work))

        def adaptive():
            self.restore_work()
            plan.threshold_adaptive(p(self.d_work), 5, 2.0, 255.0, False, p(self.d_work))

        return [
            ("pipeline", lambda: plan.pipeline(p(self.d_in), 59.0, 119.0, 20, 0, p(self.d_edges), p(self.d_lines), LINE_CAP, p(self.d_counts))),
            ("async step + wait", asynchronous),
            ("packed step, no gray output", lambda: plan.pipeline_ex(p(self.d_packed), 59.0, 119.0, 20, 0, p(self.d_edges2), p(self.d_lines2), LINE_CAP, p(self.d_counts2),
                                                                     pixfmt=capi.FMT_RGB24)),
            ("otsu", lambda: plan.otsu(p(self.d_in), p(self.d_otsu))),
            ("blur in place", blur),
            ("canny in place", canny),
            ("segments", lambda: plan.houghsht_segments(p(self.d_edges), p(self.d_lines), p(self.d_counts), LINE_CAP, 0, 4, 1, p(self.d_segs), SEG_CAP, p(self.d_seg_counts))),
            ("fit", lambda: plan.houghsht_fit(p(self.d_edges), p(self.d_lines), p(self.d_counts), LINE_CAP, 0, 3, 0, 0, 0, p(self.d_fits), LINE_CAP, p(self.d_fit_counts))),
            ("components, byte map, no labels", lambda: plan.components(p(self.d_edges), 8, 1, 0, 0, p(self.d_comps), COMP_CAP, p(self.d_comp_counts))),
            ("adaptive threshold in place", adaptive),
            ("morph OPEN", lambda: plan.morph(p(self.d_in), self.strel, capi.MORPH_OPEN, capi.BORDER_REPLICATE, p(self.d_tmp))),
            ("FAST, no score map", lambda: plan.fast(p(self.d_in), 20, 9, True, -1, 0, p(self.d_corners), CORNER_CAP, p(self.d_corner_counts))),
            ("ORB keypoints", lambda: plan.orb_keypoints(p(self.d_in), p(self.d_corners), CORNER_CAP, p(self.d_corner_counts), 0, 1.0, p(self.d_keys), KEY_CAP,
                                                         p(self.d_key_counts))),
            ("ORB describe with blur", lambda: plan.orb_describe(p(self.d_in), p(self.d_keys), KEY_CAP, p(self.d_key_counts), 1.0, p(self.d_desc), 32, blur=True)),
            ("pipeline, larger lineCap", lambda: plan.pipeline(p(self.d_in), 59.0, 119.0, 20, 0, p(self.d_edges), p(self.d_lines_big), BIG_LINE_CAP, p(self.d_counts))),
            ("batched KHT", lambda: plan.houghkht(p(self.d_edges), threads=2)),
        ]

    def regrow_calls(self, plan):
        """the line-key buffers of a plan whose accumulator has more cells than any of the three capacities (ensureLineCap)"""
        p = lambda t: t.data_ptr()   # noqa: E731
        step = lambda cap: (lambda: plan.pipeline(p(self.d_in), 59.0, 119.0, 20, 0, p(self.d_edges), p(self.d_lines_big), cap, p(self.d_counts)))   # noqa: E731
        return [("pipeline, 65536 slots", step(LINE_CAP)), ("pipeline, 131072 slots", step(BIG_LINE_CAP)), ("pipeline, 162000 slots", step(HUGE_LINE_CAP))]

    def matcher_calls(self, m):
        p = lambda t: t.data_ptr()   # noqa: E731
        return [
            ("knn", lambda: m.knn(p(self.d_query), 32, 0, p(self.d_train), 32, 0, False, p(self.d_matches))),
            ("good, cross check", lambda: m.good(p(self.d_matches), p(self.d_query), 32, 0, p(self.d_train), 32, 0, False, p(self.d_good), Q, p(self.d_good_counts),
                                                 cross_check=True)),
        ]

    def pyramid_calls(self, y):
        p = lambda t: t.data_ptr()   # noqa: E731
        return [
            ("detect", lambda: y.detect(p(self.d_in), p(self.d_keys), KEY_CAP, p(self.d_key_counts))),
            ("describe", lambda: y.describe(p(self.d_in), p(self.d_keys), KEY_CAP, p(self.d_key_counts), p(self.d_desc), 32)),
        ]


def run(rig, start, first, calls, seen):
    """every call once, the count after each into `seen`; then all of them again: nothing new is allocated"""
    seen[first] = rig.live() - start
    for name, call in calls:
        call()
        seen[name] = rig.live() - start
    after = rig.live()
    for name, call in calls:
        call()
        assert rig.live() == after, "the second '%s' allocated or freed" % name


def check(seen, expected):
    print("allocations above the start, step by step:", seen)
    assert list(seen) == list(expected)
    last = 0
    for name, want in expected.items():
        if want is None:
            assert seen[name] >= last, "%s: the count fell from %d to %d" % (name, last, seen[name])
        else:
            assert seen[name] == want, "%s: %d device allocations above the start, %d at the commit the counts were recorded from" % (name, seen[name], want)
        last = seen[name]


def test_handles_give_back_what_they_took_and_allocate_what_they_did(hip_ctx):
    from compv_amd import capi
    rig = Rig(hip_ctx)
    start = rig.live()

    plan = capi.Plan(hip_ctx, W, H, S, F, 1.0)
    seen = {}
    try:
        run(rig, start, "plan", rig.plan_calls(plan), seen)
    finally:
        rig.torch.cuda.synchronize()
        plan.close()
    assert rig.live() == start, "closing the plan left %d allocations" % (rig.live() - start)
    check(seen, EXPECTED)

    assert hip_ctx.houghsht_dims(W, H, REGROW_THETA)[:2] == (225, 720)
    plan = capi.Plan(hip_ctx, W, H, S, F, REGROW_THETA)
    seen = {}
    try:
        run(rig, start, "plan", rig.regrow_calls(plan), seen)
    finally:
        rig.torch.cuda.synchronize()
        plan.close()
    assert rig.live() == start, "closing the regrown plan left %d allocations" % (rig.live() - start)
    check(seen, EXPECTED_REGROW)

    matcher = capi.Matcher(hip_ctx, 32, Q, Q, pairs=1, knn=2)
    seen = {}
    try:
        run(rig, start, "matcher", rig.matcher_calls(matcher), seen)
    finally:
        rig.torch.cuda.synchronize()
        matcher.close()
    assert rig.live() == start, "closing the matcher left %d allocations" % (rig.live() - start)
    check(seen, EXPECTED_MATCHER)

    pyramid = capi.OrbPyramid(hip_ctx, W, H, S, F, capi.OrbPyramidOpts(2, 0.83, 20, 9, True, 100), corner_cap=CORNER_CAP)
    seen = {}
    try:
        assert pyramid.geometry(1)[2] != 0          # two levels that exist
        run(rig, start, "pyramid", rig.pyramid_calls(pyramid), seen)
    finally:
        rig.torch.cuda.synchronize()
        pyramid.close()
    assert rig.live() == start, "closing the pyramid left %d allocations" % (rig.live() - start)
    check(seen, EXPECTED_PYRAMID)
