"""GPU FAST corners (compvhip_plan_fast and its host form compvhip_fast_u8) against tests/fast_model.py, byte for byte, every frame of every case:
score map, counts, records.

Harness of tests/gpu_support.py: every device buffer sits between two guards; outputs start filled with a sentinel -- the score map's
padding columns [W, S) and the record slots behind a frame's count included -- and must still hold it there afterwards; the input's padding
columns hold seeded random bytes and the input must come back unchanged.

Geometries (W, H, S, F) and what they reach.  The score kernel works on 128 x 32 tiles (4-pixel dword groups, a 1-pixel score ring and a
4-pixel raw halo around the tile); the list kernels give one wave a row and walk it 512 pixels at a time:
  (7, 7, 8, 3)          one interior pixel
  (9, 9, 16, 3)         3 x 3 interior; one ragged dword (W % 4 == 1)
  (17, 9, 24, 2)        the interior ends inside a dword group (W - 3 = 14); S % 16 == 8
  (13, 70, 24, 2)       three row tiles, the last 6 rows tall
  (239, 24, 240, 5)     two column tiles, W % 4 == 3, S - W = 1: the last dword of a row is ragged
  (513, 65, 576, 9)     five column tiles, the last one column wide (all border); one column past a wave's 512-pixel step; three row tiles, the
                        last one row tall; 9 frames
  (1001, 333, 1008, 33) F = 33 frames (blockIdx.z), 11 row tiles, two steps per row
  (100, 1537, 104, 3)   tall: 49 row tiles, more rows than the scan's 256 threads take one each (7 rows per thread)
  (129, 33, 136, 2)     one column past the tile width and one row past the tile height: 1-wide / 1-tall tiles that are all border, whose
                        neighbours' NMS ring reads them
  (132, 36, 136, 2)     four columns and four rows past: the second tiles hold one interior column / row, suppressed from and suppressing
                        across the seam

Frames of a batch cycle through: noise, blurred blocks, noise confined to the 8 columns / rows around every tile seam, a constant frame (no
corner), isolated arcs of 9 at three strengths (ties)."""
import functools

import numpy as np
import pytest

import fast_model as fm
from fast_rig import Rig, batch
from gpu_support import SENTINEL, Arena, ptr
from plan_geometries import GEOMETRIES

pytestmark = pytest.mark.gpu

WANTED = [(9, 9, 16, 3), (17, 9, 24, 2), (13, 70, 24, 2), (239, 24, 240, 5), (513, 65, 576, 9), (1001, 333, 1008, 33), (100, 1537, 104, 3)]
SWEEP = [(7, 7, 8, 3)] + [g[:4] for g in GEOMETRIES if g[:4] in WANTED] + [(129, 33, 136, 2), (132, 36, 136, 2)]
assert len(SWEEP) == len(WANTED) + 3
COMBOS = [(9, True, 20), (12, True, 1), (9, False, 100), (12, False, 20)]          # N, NMS, t


@functools.lru_cache(maxsize=None)
def expected(geom, seed, N, nonmax, t):
    """model output of every frame of a batch, computed once: [(records, score map)]"""
    W, H, S, F = geom
    valid = batch(W, H, F, seed)
    return [fm.fast(valid[f], t, N, nonmax) for f in range(F)]


@pytest.mark.parametrize("geom", SWEEP, ids=lambda g: "%dx%d_S%d_F%d" % g)
def test_fast_geometry_sweep(hip_ctx, geom):
    """N 9 and 12, NMS on and off, three thresholds: score map, counts and records of every frame; then, on the first combination, the same list
    without a score map, a capacity below the count (a prefix and the true count), capacity 0 (counts only) and a second identical call"""
    W, H, S, F = geom
    seed = W + H
    big = W * H * F > 2_000_000          # the 33-frame batch: N 9 with NMS and N 12 without (the small ones cover all four)
    combos = COMBOS[:1] + COMBOS[3:] if big else COMBOS
    exps = {c: expected(geom, seed, c[0], c[1], c[2]) for c in combos}
    cap = max(max(len(e[0]) for e in exp) for exp in exps.values()) + 5
    rig = Rig(hip_ctx, geom, seed, cap)
    try:
        for (N, nonmax, t) in combos:
            rig.run(N, nonmax, t)
            rig.check("N %d nms %d t %d" % (N, nonmax, t), exps[(N, nonmax, t)])
        N, nonmax, t = combos[0]
        exp = exps[combos[0]]
        rig.run(N, nonmax, t, scores=False)
        first, _ = rig.check("no score map", exp, scores=False)
        rig.run(N, nonmax, t, scores=False)
        again, _ = rig.check("no score map, again", exp, scores=False)
        assert first == again
        most = max(len(e[0]) for e in exp)
        small = max(1, most // 2)
        rig.run(N, nonmax, t, cap=small)
        rig.check("cap %d of %d" % (small, most), exp, cap=small)
        rig.run(N, nonmax, t, cap=0)
        rig.check("counts only", exp, cap=0)
    finally:
        rig.close()


def test_content_reaches_what_the_docstring_says(hip_ctx):
    """the batches hold frames with corners on both sides of a tile seam that suppress each other across it, an empty frame and ties"""
    geom = (513, 65, 576, 9)
    exp = expected(geom, 513 + 65, 9, True, 20)
    valid = batch(513, 65, 9, 513 + 65)
    kinds = [(513 + 65 + f) % 5 for f in range(9)]
    assert any(len(exp[f][0]) == 0 for f in range(9) if kinds[f] == 3) and all(len(exp[f][0]) > 0 for f in range(9) if kinds[f] != 3)
    f = kinds.index(2)          # seam noise: before NMS there are scores in column 127 AND column 128, in row 31 AND row 32
    s = fm.score_map(valid[f], 20, 9)
    assert s[:, 127].any() and s[:, 128].any() and s[31].any() and s[32].any() and (fm.nms(s) != s).any()


@pytest.mark.parametrize("geom", [(239, 24, 240, 5), (513, 65, 576, 9)], ids=lambda g: "%dx%d_S%d_F%d" % g)
def test_max_features_cuts_at_a_tie(hip_ctx, geom):
    """maxFeatures below the count of most frames: the canonical cut, per frame.  The tied-arc frames hold three strengths only, so their cut
    falls inside a tie and the count exceeds maxFeatures; frames with fewer corners than maxFeatures keep all."""
    W, H, S, F = geom
    seed = W + H
    for (N, nonmax, t) in (COMBOS[0], COMBOS[3]):
        exp = expected(geom, seed, N, nonmax, t)
        cap = max(len(e[0]) for e in exp) + 5
        rig = Rig(hip_ctx, geom, seed, cap)
        try:
            for K in (2, 10, 37):
                cut = [fm.cut(e[0], K) for e in exp]
                if N == 9 and nonmax and K >= 10:
                    assert any(len(c) > K for c in cut), "no frame is cut at a tie"
                    assert any(len(c) < len(e[0]) for c, e in zip(cut, exp))
                rig.run(N, nonmax, t, max_features=K)
                rig.check("maxFeatures %d N %d nms %d" % (K, N, nonmax), exp, cut=K)          # the score map is NOT cut
            rig.run(N, nonmax, t, max_features=1)
            rig.check("maxFeatures 1 = no cut", exp)
            rig.run(N, nonmax, t, max_features=10, cap=4)
            rig.check("cut and clipped", exp, cap=4, cut=10)
        finally:
            rig.close()


def test_host_form_agrees_with_plan_and_model(hip_ctx):
    rng = np.random.default_rng(11)
    W, H = 77, 45
    padded = np.ascontiguousarray(rng.integers(0, 256, (H, 96), dtype=np.uint8))
    padded[:, :W] = fm.blocks(W, H, 5)
    view = padded[:, :W]                                   # a host image with a row stride
    for (N, nonmax, t) in COMBOS:
        exp_rec, exp_map = fm.fast(view, t, N, nonmax)
        rec, smap = hip_ctx.fast(view, t, N, nonmax, want_scores=True, cap=3)          # grows its buffer after COMPVHIP_E_OUT_OF_BOUND
        assert rec.tobytes() == exp_rec.tobytes() and smap.tobytes() == exp_map.tobytes(), (N, nonmax, t)
        assert hip_ctx.fast(view, t, N, nonmax, max_features=7).tobytes() == fm.cut(exp_rec, 7).tobytes()
    # the number only; then a buffer that is too small: a prefix, the true number and COMPVHIP_E_OUT_OF_BOUND
    import ctypes as C
    from compv_amd import capi
    exp_rec, _ = fm.fast(view, 20, 9, True)
    assert len(exp_rec) > 4
    n = C.c_size_t(0)
    L = hip_ctx.lib
    assert L.compvhip_fast_u8(hip_ctx.h, view.ctypes.data, W, H, 96, 20, 9, 1, -1, None, 0, None, 0, C.byref(n)) == (capi.E_OUT_OF_BOUND if len(exp_rec) else capi.OK)
    assert n.value == len(exp_rec)
    buf = np.full(6, 0x5a5a5a5a, np.int32).view(capi.CORNER_DTYPE)          # two records
    assert L.compvhip_fast_u8(hip_ctx.h, view.ctypes.data, W, H, 96, 20, 9, 1, -1, None, 0, buf.ctypes.data, 1, C.byref(n)) == capi.E_OUT_OF_BOUND
    assert n.value == len(exp_rec) and buf[:1].tobytes() == exp_rec[:1].tobytes() and int(buf[1]["x"]) == 0x5a5a5a5a


def test_threshold_is_clipped_and_t0_uses_the_integer_formula(hip_ctx):
    img = fm.noise(40, 30, 8)
    for t, eff in ((-5, 0), (0, 0), (300, 255), (255, 255)):
        exp_rec, exp_map = fm.fast(img, eff, 9, False)
        rec, smap = hip_ctx.fast(img, t, 9, False, want_scores=True)
        assert rec.tobytes() == exp_rec.tobytes() and smap.tobytes() == exp_map.tobytes(), t
    rec = hip_ctx.fast(img, 0, 9, False)
    assert len(rec) and int(rec["strength"].min()) >= 0 and (rec["strength"] == fm.score_map(img, 0, 9)[rec["y"], rec["x"]].astype(np.int32) - 1).all()


def test_refusals(hip_ctx):
    from compv_amd import capi

    def code(fn, *a, **k):
        with pytest.raises(capi.CompvHipError) as e:
            fn(*a, **k)
        return e.value.code
    img = np.zeros((40, 40), np.uint8)
    assert code(hip_ctx.fast, img, 20, 10) == capi.E_INVALID_PARAMETER
    assert code(hip_ctx.fast, img, 20, 0) == capi.E_INVALID_PARAMETER
    assert code(hip_ctx.fast, img[:6], 20, 9) == capi.E_INVALID_PARAMETER          # H = 6: no interior pixel
    assert code(hip_ctx.fast, img[:, :6], 20, 9) == capi.E_INVALID_PARAMETER
    assert len(hip_ctx.fast(img[:7, :7], 20, 9)) == 0
    ar = Arena()
    d = ar.new(4 * 16 * 16)
    d_counts = ar.new(8)
    small = capi.Plan(hip_ctx, 6, 9, 8, 1)
    plan = capi.Plan(hip_ctx, 16, 16, 16, 2)
    try:
        assert code(small.fast, ptr(d), 20, 9, True, -1, 0, 0, 0, ptr(d_counts)) == capi.E_INVALID_PARAMETER
        assert code(plan.fast, ptr(d), 20, 11, True, -1, 0, 0, 0, ptr(d_counts)) == capi.E_INVALID_PARAMETER
        assert code(plan.fast, 0, 20, 9, True, -1, 0, 0, 0, ptr(d_counts)) == capi.E_INVALID_PARAMETER
        assert code(plan.fast, ptr(d), 20, 9, True, -1, 0, 0, 0, 0) == capi.E_INVALID_PARAMETER
        assert code(plan.fast, ptr(d), 20, 9, True, -1, 0, 0, 5, ptr(d_counts)) == capi.E_INVALID_PARAMETER              # a capacity without a buffer
        assert code(plan.fast, ptr(d), 20, 9, True, -1, ptr(d) + 256, 0, 0, ptr(d_counts)) == capi.E_INVALID_PARAMETER   # score map inside the frames
        assert code(plan.fast, ptr(d), 20, 9, True, -1, ptr(d) + 512 + 4, 0, 0, ptr(d_counts)) == capi.E_INVALID_PARAMETER   # not 8-byte aligned
        assert code(plan.fast, ptr(d), 20, 9, True, -1, 0, ptr(d) + 512 + 2, 4, ptr(d_counts)) == capi.E_INVALID_PARAMETER   # records not 4-byte aligned
        assert code(plan.fast, ptr(d), 20, 9, True, -1, 0, 0, 0, ptr(d_counts) + 1) == capi.E_INVALID_PARAMETER
        ar.check("refusals")
        assert (d.cpu().numpy() == SENTINEL).all() and (d_counts.cpu().numpy() == SENTINEL).all()
    finally:
        small.close()
        plan.close()


def test_plan_scratch_streams_and_allocations(hip_ctx):
    """the plan's scratch is allocated on first use -- one block of counters, and a score map only for the calls that do not bring one -- is counted by
    compvhip_live_allocations and is released with the plan; a call on a non-default stream"""
    import torch
    torch.cuda.synchronize()
    start = hip_ctx.live_allocations()
    geom = (239, 24, 240, 5)
    exp = expected(geom, 239 + 24, 9, True, 20)
    rig = Rig(hip_ctx, geom, 239 + 24, max(len(e[0]) for e in exp) + 5)
    try:
        base = hip_ctx.live_allocations()
        rig.run(9, True, 20)
        assert hip_ctx.live_allocations() == base + 1
        rig.check("with a score map", exp)
        rig.run(9, True, 20, scores=False)
        assert hip_ctx.live_allocations() == base + 2
        rig.check("without", exp, scores=False)
        rig.run(9, True, 20, max_features=10)
        assert hip_ctx.live_allocations() == base + 2
        rig.check("cut", exp, cut=10)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        rig.run(9, True, 20, stream=st.cuda_stream)
        st.synchronize()
        rig.check("on a stream", exp)
    finally:
        rig.close()
    assert hip_ctx.live_allocations() == start


# ---- the CompV binding ---------------------------------------------------------------------------------------------------------------------
def test_plugin_factory_returns_the_reference_point_list():
    """integration/compv_hip_plugin.cxx re-registers COMPV_FAST_ID: headless_samples runs the reference's built-in detector and the HIP one the
    factory returns afterwards on the same 200 x 258 frame with maxFeatures = -1 and compares the point lists.

    Skipped, before anything runs, when oracle/_ref holds no headless_samples built with the FAST call: the directory is absent, or it was built
    from sources older than the FAST binding (such a program does not hold the text of the report line, ignores the switch and runs its other
    comparisons).  Whatever a program that has the call then does -- any exit code but 0, a crash, a DIFF -- fails the test."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "oracle", "_ref", "headless_samples")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref not built (needs the reference checkout; see oracle/build_ref.sh)")
    with open(exe, "rb") as f:
        if b"fast_corners: %s" not in f.read():
            pytest.skip("oracle/_ref/headless_samples was built before the FAST binding existed (rebuild it with oracle/build_ref.sh where the reference checkout is)")
    out = subprocess.run([exe, "--fast-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "fast_corners: MATCH" in out.stdout, out.stdout[-2000:]
