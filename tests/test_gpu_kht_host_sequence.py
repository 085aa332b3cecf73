"""The host KHT calls (compvhip_houghkht_u8, _ex_u8, _kernels_u8: compv_amd/csrc/api_kht.cpp) across changing sizes and content, the way
test_gpu_host_path.py treats the other host calls.  One context goes through 96x40 -> 130x70 -> 40x33; at each size it sees stroke map A, a blank map and
stroke map B, and per map it runs the reference order (against oracle.kht), the canonical order (against kht_canon_model.CanonModel) and the kernel
inspection call (against oracle.kht_kernels).  Every result must equal, byte for byte, that of a fresh context that has only seen that one map; a batched
plan call on the same context in between must change nothing; a repeat at the last size must not allocate; and with room for one record fewer than
there are, every call must return COMPVHIP_E_OUT_OF_BOUND, the true count and a correct prefix."""
import ctypes as C

import numpy as np
import pytest

from compv_amd import capi
from kht_canon_model import CanonModel

pytestmark = pytest.mark.gpu

SIZES = [(96, 40), (130, 70), (40, 33)]
# what the CPU oracle gives for the stroke maps at threshold 1 (and at 5): (A lines, A kernels, B lines, B kernels) in the reference order
ORACLE_COUNTS = {(96, 40): (11, 4, 5, 4), (130, 70): (9, 6, 10, 6), (40, 33): (11, 4, 6, 3)}


def _maps(W, H):
    """stroke map A, blank, stroke map B: 255 on zero.  A: the row H/3, the main diagonal from (4, 4), the column W - 6; B: the row 2H/3, the anti-diagonal
    from (6, H - 5), the column 7.  (The strokes end a few pixels inside the frame: rows at x in [3, W - 3) / [3, W - 5), columns at y in [5, H - 5), the
    diagonals 4 / 5 pixels short of the far borders.)"""
    a, b = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    a[H // 3, 3:W - 3] = 255
    for i in range(min(W, H) - 8):
        a[4 + i, 4 + i] = 255
    a[5:H - 5, W - 6] = 255
    b[2 * H // 3, 3:W - 5] = 255
    i = 0
    while 6 + i < W - 5 and H - 5 - i >= 5:
        b[H - 5 - i, 6 + i] = 255
        i += 1
    b[5:H - 5, 7] = 255
    return [a, np.zeros((H, W), np.uint8), b]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _lines(ctx, e, order, cap=1 << 12):
    """the raw call: (return code, *n, the min(*n, cap) records, GS or None when the call left it alone)"""
    H, W = e.shape
    rec = np.zeros(cap, capi.LINE_DTYPE)
    n, gs = C.c_size_t(0), C.c_double(float("nan"))
    if order == "reference":
        rc = ctx.lib.compvhip_houghkht_u8(ctx.h, _ptr(e), W, H, e.strides[0], 1.0, 1.0, 1, 0, 2.0, 10, 0.002, _ptr(rec), cap, C.byref(n), C.byref(gs))
    else:
        opts = capi.KhtOpts(1.0, 1.0, 1, 0, 2.0, 10, 0.002, 0, capi.KHT_ORDER_CANONICAL)
        rc = ctx.lib.compvhip_houghkht_ex_u8(ctx.h, _ptr(e), W, H, e.strides[0], C.byref(opts), _ptr(rec), cap, C.byref(n), C.byref(gs))
    return rc, n.value, rec[:min(n.value, cap)], (None if np.isnan(gs.value) else gs.value)


def _kernels(ctx, e, cap=1 << 10):
    H, W = e.shape
    out = np.zeros((cap, 7), np.float64)
    n, hmax = C.c_size_t(0), C.c_double(float("nan"))
    rc = ctx.lib.compvhip_houghkht_kernels_u8(ctx.h, _ptr(e), W, H, e.strides[0], 2.0, 10, _ptr(out), cap, C.byref(n), C.byref(hmax))
    return rc, n.value, out[:min(n.value, cap)], hmax.value


def _host(ctx, e):
    """the three host calls on one map: [(name, bytes or value)]"""
    out = []
    for order in ("reference", "canonical"):
        rc, n, rec, gs = _lines(ctx, e, order)
        assert rc == capi.OK and n == len(rec), (order, rc, ctx.last_error())
        if order == "canonical":
            assert ctx.houghkht_stage_ms()[5] == 0
        out += [(order, rec), (order + " gs", gs)]
    rc, n, k, hmax = _kernels(ctx, e)
    assert rc == capi.OK and n == len(k), (rc, ctx.last_error())
    return out + [("kernels", k), ("hmax", hmax)]


def _same(got, exp, where):
    assert [n for n, _ in got] == [n for n, _ in exp]
    for (name, g), (_, e) in zip(got, exp):
        if isinstance(g, np.ndarray):
            assert g.dtype == e.dtype and g.shape == e.shape and g.tobytes() == e.tobytes(), (where, name)
        else:
            assert repr(g) == repr(e), (where, name)


def _f32(v):
    return int(np.float32(v).view(np.uint32))


def _bits(rec):
    """LINE_DTYPE records -> [(rho bits, theta bits, strength, row, col)]"""
    return list(zip(rec["rho"].astype(np.float32).view(np.uint32).tolist(), rec["theta"].astype(np.float32).view(np.uint32).tolist(),
                    rec["strength"].tolist(), rec["row"].tolist(), rec["col"].tolist()))


class Expected:
    """oracle and model results per map, computed once"""

    def __init__(self, oracle):
        self.oracle, self.model, self.memo = oracle, CanonModel(oracle), {}

    def of(self, e):
        key = (e.shape, e.tobytes())
        if key not in self.memo:
            ref, gs = self.oracle.kht(e, 1.0, 1.0, 1)
            canon, cgs, _ = self.model.lines(e)
            kernels, hmax = self.oracle.kht_kernels(e)
            self.memo[key] = (ref, gs, canon, cgs, kernels, hmax)
        return self.memo[key]

    def check_reference(self, rec, gs, e, where):
        ref, egs, _, cgs, _, _ = self.of(e)
        assert [b[:3] for b in _bits(rec)] == [(_f32(l[0]), _f32(l[1]), l[2]) for l in ref], where      # values AND order
        if cgs is None:
            assert gs is None and not ref, where                                                       # no kernel survives: GS is not reported
        else:
            assert repr(gs) == repr(egs), where

    def check_canonical(self, rec, gs, e, where):
        _, _, canon, cgs, _, _ = self.of(e)
        assert _bits(rec) == [(_f32(l[0]), _f32(l[1]), l[2], l[3], l[4]) for l in canon], where
        assert gs == cgs, where

    def check(self, got, e, where):
        named = dict(got)
        self.check_reference(named["reference"], named["reference gs"], e, where)
        self.check_canonical(named["canonical"], named["canonical gs"], e, where)
        _, _, _, _, kernels, hmax = self.of(e)
        assert named["kernels"].shape == kernels.shape and np.array_equal(named["kernels"].view(np.uint64), kernels.view(np.uint64)), where
        assert named["hmax"] == hmax, where


def _fresh(e):
    ctx = capi.Context(0)
    try:
        return _host(ctx, e)
    finally:
        ctx.close()


def _plan_between(ctx, maps, expected):
    """a 3-frame plan on the SAME context, both orders: its lists against the oracle and the model"""
    import torch
    F, (H, W) = len(maps), maps[0].shape
    S = (W + 7) & ~7                                   # a plan's stride is a multiple of 8
    padded = np.zeros((F, H, S), np.uint8)
    padded[:, :, :W] = np.stack(maps)
    d_e = torch.from_numpy(padded).to(torch.device("cuda:0"))
    torch.cuda.synchronize()
    live = ctx.live_allocations()
    plan = capi.Plan(ctx, W, H, S, F, 1.0)
    try:
        ref, rgs = plan.houghkht(d_e.data_ptr(), 1.0, 1.0, 1)
        canon, cgs = plan.houghkht(d_e.data_ptr(), 1.0, 1.0, 1, order="canonical")
        assert plan.houghkht_stage_ms()["stages"]["sort_sweep"] == 0
        for f in range(F):
            expected.check_reference(ref[f], rgs[f], maps[f], ("plan", f))
            expected.check_canonical(canon[f], cgs[f], maps[f], ("plan", f))
    finally:
        plan.close()
    assert ctx.live_allocations() == live


def test_host_kht_calls_across_sizes_and_content_match_fresh_contexts(oracle):
    expected = Expected(oracle)
    ctx = capi.Context(0)
    try:
        assert ctx.live_allocations() == 0
        for W, H in SIZES:
            maps = _maps(W, H)
            got = [_host(ctx, e) for e in maps]
            for i, e in enumerate(maps):
                expected.check(got[i], e, (W, H, i))
                _same(got[i], _fresh(e), (W, H, i))
            a, blank, b = (dict(g) for g in got)
            counts = (len(a["reference"]), len(a["kernels"]), len(b["reference"]), len(b["kernels"]))
            assert counts == ORACLE_COUNTS[(W, H)] and min(counts) >= 2 and min(len(a["canonical"]), len(b["canonical"])) >= 2, (W, H, counts)
            for thr5 in (maps[0], maps[2]):
                assert len(oracle.kht(thr5, 1.0, 1.0, 5)[0]) == len(expected.of(thr5)[0])
            assert len(blank["reference"]) == len(blank["canonical"]) == len(blank["kernels"]) == 0
            assert blank["reference gs"] is None and blank["canonical gs"] is None
            if (W, H) == SIZES[1]:
                _plan_between(ctx, maps, expected)
                for i, e in enumerate(maps):
                    _same(_host(ctx, e), got[i], ("after the plan", i))

        # the smallest size last: everything is allocated, a second pass must reuse it
        live = ctx.live_allocations()
        assert live > 0
        for i, e in enumerate(maps):
            _same(_host(ctx, e), got[i], ("repeat", i))
        assert ctx.live_allocations() == live

        # one record fewer than there are: E_OUT_OF_BOUND, the true count, a correct prefix
        e, named = maps[0], dict(got[0])
        for order in ("reference", "canonical"):
            true = named[order]
            rc, n, rec, gs = _lines(ctx, e, order, cap=len(true) - 1)
            assert rc == capi.E_OUT_OF_BOUND and n == len(true) and rec.tobytes() == true[:-1].tobytes() and repr(gs) == repr(named[order + " gs"]), order
        true = named["kernels"]
        rc, n, k, hmax = _kernels(ctx, e, cap=len(true) - 1)
        assert rc == capi.E_OUT_OF_BOUND and n == len(true) and k.tobytes() == true[:-1].tobytes() and hmax == named["hmax"]
        assert ctx.live_allocations() == live
    finally:
        ctx.close()
    assert ctx.live_allocations() == 0
