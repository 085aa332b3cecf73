"""The host (`*_u8`) entry points share one frame -- the cached single-frame plan, the dIn / dOut staging, the record staging, the
count-and-prefix read-back (compv_amd/csrc/api_host.cpp).  One context runs the whole family while the image size changes 96x40 -> 130x70 -> 40x33 (up
across a 64-byte stride boundary, then down: the plan is rebuilt each time, the staging is reused by different calls and is larger than needed at the
last size); every result must equal, byte for byte, that of a fresh context that has only ever seen that size.  At the last size a repeat of the
whole sequence must not allocate; and every list-returning call, given room for one record fewer than there are, must return
COMPVHIP_E_OUT_OF_BOUND, the true count and a correct prefix."""
import ctypes as C

import numpy as np
import pytest

from compv_amd import capi

pytestmark = pytest.mark.gpu

SIZES = [(96, 40), (130, 70), (40, 33)]


def _inputs(W, H):
    rng = np.random.default_rng(1000 * W + H)
    return rng.integers(0, 256, (H, W * 3), dtype=np.uint8), np.ones((3, 3), np.uint8) * 0xff


def _sequence(ctx, W, H):
    """every host call on the cached plan, in a fixed order; the results as a list of (name, array)"""
    rgb, strel = _inputs(W, H)
    out = []
    gray = ctx.grayscale(rgb, capi.FMT_RGB24, W);                                  out.append(("gray", gray))
    out.append(("otsu", np.array([ctx.otsu(gray)])))
    edges = ctx.canny(gray, 60.0, 120.0);                                          out.append(("canny", edges))
    lines, acc = ctx.houghsht(edges, 1.0, 8, max_lines=24, want_acc=True);         out += [("lines", lines), ("acc", acc)]
    segs = ctx.houghsht_segments(edges, lines, 1.0, min_length=2, max_gap=1);      out.append(("segs", segs))
    fits, refined = ctx.houghsht_fit(edges, lines, 1.0, 2, want_refined=True);     out += [("fits", fits), ("refined", refined)]
    out.append(("segfits", ctx.houghsht_fit(edges, lines, 1.0, 2, segs=segs)))
    labels, comps = ctx.components(edges, 8, 1, want_labels=True);                 out += [("labels", labels), ("comps", comps)]
    out.append(("comps_only", ctx.components(edges, 8, 1, want_labels=False)[1]))
    corners, scores = ctx.fast(gray, 20, 9, True, -1, want_scores=True);           out += [("corners", corners), ("scores", scores)]
    out.append(("threshold", ctx.threshold(gray, 127.0)))
    out.append(("close", ctx.morph(gray, strel, capi.MORPH_CLOSE)))
    return out


def _same(got, exp, where):
    assert [n for n, _ in got] == [n for n, _ in exp]
    for (name, g), (_, e) in zip(got, exp):
        assert g.dtype == e.dtype and g.shape == e.shape and g.tobytes() == e.tobytes(), (where, name)


def test_host_calls_across_size_changes_match_fresh_contexts():
    ctx = capi.Context(0)
    try:
        for W, H in SIZES:
            got = _sequence(ctx, W, H)
            fresh = capi.Context(0)
            try:
                exp = _sequence(fresh, W, H)
            finally:
                fresh.close()
            _same(got, exp, (W, H))
            named = dict(got)
            assert len(named["lines"]) >= 2 and len(named["segs"]) >= 2 and len(named["comps"]) >= 2 and len(named["corners"]) >= 2, (W, H)
        # the smallest size last: everything is allocated, the whole sequence again must reuse it
        live = ctx.live_allocations()
        again = _sequence(ctx, *SIZES[-1])
        assert ctx.live_allocations() == live
        _same(again, got, "repeat")

        # one record fewer than there are: E_OUT_OF_BOUND, the true count, a correct prefix
        W, H = SIZES[-1]
        edges, gray, lines, segs = named["canny"], named["gray"], named["lines"], named["segs"]
        lib, n = ctx.lib, C.c_size_t(0)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)

        def short(true, dtype, call):
            cap = len(true) - 1
            rec = np.zeros(cap, dtype)
            n.value = 0
            assert call(ptr(rec), cap) == capi.E_OUT_OF_BOUND, dtype
            assert n.value == len(true) and rec.tobytes() == true[:cap].tobytes(), dtype

        short(lines, capi.LINE_DTYPE, lambda r, cap: lib.compvhip_houghsht_u8(ctx.h, ptr(edges), W, H, W, C.c_float(1.0), C.c_float(1.0), 8, 24, r, cap, C.byref(n), None, 0))
        short(segs, capi.SEGMENT_DTYPE, lambda r, cap: lib.compvhip_houghsht_segments_u8(ctx.h, ptr(edges), W, H, W, C.c_float(1.0), ptr(lines), len(lines), 2, 1, r, cap, C.byref(n)))
        short(named["fits"], capi.LINE_FIT_DTYPE,
              lambda r, cap: lib.compvhip_houghsht_fit_u8(ctx.h, ptr(edges), W, H, W, C.c_float(1.0), ptr(lines), len(lines), 2, None, 0, r, cap, C.byref(n), None))
        short(named["comps"], capi.COMP_DTYPE, lambda r, cap: lib.compvhip_components_u8(ctx.h, ptr(edges), W, H, W, 8, 1, None, W, r, cap, C.byref(n)))
        short(named["corners"], capi.CORNER_DTYPE, lambda r, cap: lib.compvhip_fast_u8(ctx.h, ptr(gray), W, H, W, 20, 9, 1, -1, None, W, r, cap, C.byref(n)))
    finally:
        ctx.close()
