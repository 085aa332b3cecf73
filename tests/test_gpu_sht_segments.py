"""Hough line segments on the GPU (compvhip_plan_houghsht_segments, compvhip_houghsht_segments_u8) against the numpy model of the
definition (tests/sht_segments_model.py, pinned on the CPU by tests/test_sht_segments_model.py): the whole segment array and the
counts, bit for bit -- there is no tolerance anywhere in the definition.

Device buffers sit between guards and start filled with a sentinel (the Arena of tests/gpu_support.py); the geometries are
those of tests/plan_geometries.py (ragged widths, padded strides, batches).
"""
import ctypes as C

import numpy as np
import pytest

from gpu_support import LINE_BYTES, SEG_BYTES, SENTINEL, T_HIGH, T_LOW, Arena, frames_view, make_batch, pad_frames, ptr, sht_threshold
from plan_geometries import GEOMETRIES
from sht_segments_model import SEG_DTYPE, frame_segments
from sht_segments_rig import assert_segments, cells_of, lines_of, model_frames, tables

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("W,H,S,F,theta", GEOMETRIES, ids=lambda v: str(v))
def test_segments_geometry_sweep(hip_ctx, oracle, W, H, S, F, theta):
    """Both entry points against the model: the plan's canonical-order lines on its own Canny masks (d_edges == NULL) and on the same
    edge maps passed as bytes -- identical buffers --, and the host entry point on its reference-order lines, rows at stride S."""
    from compv_amd import capi
    seed = W * 7 + H * 3 + F
    rng = np.random.default_rng(seed)
    imgs = make_batch(W, H, F, seed)
    sinQ, cosQ = tables(oracle, W, H, theta)
    thr = sht_threshold(W, H)
    N = max(W, H)
    params = [(1, 0), (5, 2), (1, N + 5), (max(2, N // 8), 1)]
    line_cap, seg_cap = 96, 2048
    A = Arena()
    host_in = pad_frames(imgs, S, rng)
    d_in = A.new(F * H * S, host_in)
    A.keep(d_in, host_in)
    d_e = A.new(F * H * S)
    d_lines = A.new(F * line_cap * LINE_BYTES)
    d_counts = A.new(F * 4)
    d_segs = A.new(F * seg_cap * SEG_BYTES)
    d_sc = A.new(F * 4)
    plan = capi.Plan(hip_ctx, W, H, S, F, theta)
    try:
        plan.canny(ptr(d_in), T_LOW, T_HIGH, ptr(d_e))
        plan.houghsht(0, thr, 0, ptr(d_lines), line_cap, ptr(d_counts))
        A.check("canny + houghsht")
        edges = frames_view(d_e, F, H, S, W).copy()          # bit-exact against the oracle in tests/test_gpu_plan_geometry.py
        A.keep(d_e, d_e.cpu().numpy())
        lines, counts = lines_of(d_lines, d_counts, F, line_cap)
        A.keep(d_lines, d_lines.cpu().numpy()); A.keep(d_counts, d_counts.cpu().numpy())
        exp = model_frames(edges, sinQ, cosQ, lines, params)
        total = 0
        for p in params:
            got = {}
            for how, de in (("masks", 0), ("bytes", ptr(d_e))):
                A.refill(d_segs); A.refill(d_sc)
                plan.houghsht_segments(de, ptr(d_lines), ptr(d_counts), line_cap, 0, p[0], p[1], ptr(d_segs), seg_cap, ptr(d_sc))
                A.check("segments %s %s" % (how, p))
                assert_segments(d_segs, d_sc, F, seg_cap, exp[p], "segments %s %s" % (how, p))
                got[how] = (d_segs.cpu().numpy().tobytes(), d_sc.cpu().numpy().tobytes())
            assert got["masks"] == got["bytes"], p
            total += sum(len(x) for x in exp[p])
        assert total > 0 or max(len(l) for l in lines) == 0
        # everything bridged: one segment per line with edge pixels, and its support is the line's strength
        for f in range(F):
            e = exp[(1, N + 5)][f]
            assert e["line"].tolist() == list(range(len(lines[f]))) and e["support"].tolist() == lines[f]["strength"].tolist(), f

        # host entry point: lines in the reference's order, rows of the caller's map at stride S
        for f in sorted({0, F - 1}):
            padded = np.full((H, S), 255, np.uint8)
            padded[:, :W] = edges[f]
            view = padded[:, :W]
            hl = hip_ctx.houghsht(view, theta, thr)
            for p in params[:2]:
                want = frame_segments(edges[f], sinQ, cosQ, cells_of(hl), p[0], p[1])
                got = hip_ctx.houghsht_segments(view, hl, theta, p[0], p[1], cap=64)      # grows through E_OUT_OF_BOUND when needed
                assert got.tobytes() == want.tobytes(), ("host", f, p)
    finally:
        plan.close()


def test_more_lines_than_one_scan_round(hip_ctx, oracle):
    """More than 1024 lines per frame: the per-frame scan of the segment counts runs a second round and carries the first round's total
    into it (1025 lines: a second round of one element).  The plan reads only row / col of the lines, so they are made up: cells that
    cycle over every theta column and over the accumulator rows -- all of them in the first frame, those the image can reach in the second,
    which so holds more segments per line -- and the frame's strongest cell as its last line (so that the second round of either frame has
    segments to place).  segCap lies below the second frame's total and above where the first frame's second round starts."""
    from compv_amd import capi
    W, H, S, F, theta = 96, 64, 96, 2, 1.0
    line_cap, n_lines = 1300, (1300, 1025)
    rng = np.random.default_rng(964)
    imgs = rng.integers(0, 96, (F, H, W), dtype=np.uint8)                # noise ...
    for f in range(F):                                                   # ... plus strokes
        imgs[f, 10 + 7 * f, 5:90] = 255
        imgs[f, 3:60, 40 + 11 * f] = 255
        i = np.arange(56)
        imgs[f, 4 + i, 20 + i + 5 * f] = 255
        imgs[f, 60 - i, 8 + i] = 255
    R, T, _ = oracle.sht_dims(W, H, theta)
    sinQ, cosQ = tables(oracle, W, H, theta)
    barrier = W + H
    rows = [np.arange(R), np.arange(max(0, barrier - 116), min(R, barrier + 97))]     # rho = barrier - row between -96 and 115: what 96 x 64 pixels vote for
    A = Arena()
    d_in = A.new(F * H * S, imgs)
    d_e = A.new(F * H * S)
    d_sc = A.new(F * 4)
    plan = capi.Plan(hip_ctx, W, H, S, F, theta)
    try:
        plan.canny(ptr(d_in), T_LOW, T_HIGH, ptr(d_e))
        A.check("canny")
        edges = frames_view(d_e, F, H, S, W).copy()          # bit-exact against the oracle in tests/test_gpu_plan_geometry.py
        A.keep(d_e, d_e.cpu().numpy())
        lines = []
        host_lines = np.full((F, line_cap * LINE_BYTES), SENTINEL, np.uint8)
        for f in range(F):
            k = np.arange(n_lines[f])
            ln = np.zeros(n_lines[f], capi.LINE_DTYPE)
            ln["row"] = rows[f][(k * 7 + 3 * f) % len(rows[f])]
            ln["col"] = (k * 11 + f) % T
            acc = oracle.sht_acc(np.ascontiguousarray(edges[f]), theta)
            ln["row"][-1], ln["col"][-1] = np.unravel_index(int(acc.argmax()), acc.shape)
            lines.append(ln)
            host_lines[f, :n_lines[f] * LINE_BYTES] = np.frombuffer(ln.tobytes(), np.uint8)
        d_lines = A.new(F * line_cap * LINE_BYTES, host_lines)
        d_counts = A.new(F * 4, np.array(n_lines, np.int32).view(np.uint8))
        A.keep(d_lines, host_lines); A.keep(d_counts, d_counts.cpu().numpy())
        params = [(1, 0), (5, 2)]
        exp = model_frames(edges, sinQ, cosQ, lines, params)
        for p in params:
            # segments behind line 1024 of both frames: the carry is what places them
            assert all((e["line"] >= 1024).any() for e in exp[p]), p
            seg_cap = len(exp[p][1]) - 3
            assert seg_cap > int(np.searchsorted(exp[p][0]["line"], 1024)), (p, seg_cap)     # ... and the first frame's are among the records written
            d_segs = A.new(F * seg_cap * SEG_BYTES)
            got = {}
            for how, de in (("masks", 0), ("bytes", ptr(d_e))):
                A.refill(d_segs); A.refill(d_sc)
                plan.houghsht_segments(de, ptr(d_lines), ptr(d_counts), line_cap, 0, p[0], p[1], ptr(d_segs), seg_cap, ptr(d_sc))
                A.check("segments %s %s" % (how, p))
                assert_segments(d_segs, d_sc, F, seg_cap, exp[p], "segments %s %s" % (how, p))
                got[how] = d_segs.cpu().numpy().tobytes()
            assert got["masks"] == got["bytes"], p
    finally:
        plan.close()


def _drawn_wide_map(W, H, seed, density):
    """Sparse noise plus a few long drawn lines (horizontal, vertical, two diagonals)."""
    rng = np.random.default_rng(seed)
    e = (rng.random((H, W), dtype=np.float32) < density).astype(np.uint8) * 255
    e[H // 3, W // 8:W - W // 8] = 255
    e[:, W // 2] = 255
    n = min(W, H)
    i = np.arange(n)
    e[i, i + (W - n) // 2] = 255
    e[n - 1 - i, i + (W - n) // 3] = 255
    return e


@pytest.mark.parametrize("W,H,S,thr,density", [(8192, 8192, 8192, 1500, 0.004), (32767, 64, 32768, 40, 0.002)], ids=lambda v: str(v))
def test_wide_geometries_support_is_strength(hip_ctx, oracle, W, H, S, thr, density):
    """x * cosQ + y * sinQ needs 33 bits here: the segment predicate and the vote must still agree.  Sigma support over the (1, N) segments
    of every line equals its strength; the first lines also against the model, record by record."""
    from compv_amd import capi
    theta = 1.0
    e = _drawn_wide_map(W, H, W + H, density)
    host = np.zeros((H, S), np.uint8)
    host[:, :W] = e
    sinQ, cosQ = tables(oracle, W, H, theta)
    A = Arena()
    d_e = A.new(H * S, host)
    A.keep(d_e, host)
    line_cap, seg_cap = 4096, 1 << 16
    d_lines = A.new(line_cap * LINE_BYTES)
    d_counts = A.new(4)
    d_segs = A.new(seg_cap * SEG_BYTES)
    d_sc = A.new(4)
    plan = capi.Plan(hip_ctx, W, H, S, 1, theta)
    try:
        plan.houghsht(ptr(d_e), thr, 0, ptr(d_lines), line_cap, ptr(d_counts))
        (lines,), counts = lines_of(d_lines, d_counts, 1, line_cap)
        assert 3 <= int(counts[0]) <= line_cap, int(counts[0])      # the drawn lines at least (the NMS skips theta column 0)
        plan.houghsht_segments(ptr(d_e), ptr(d_lines), ptr(d_counts), line_cap, 0, 1, max(W, H), ptr(d_segs), seg_cap, ptr(d_sc))
        A.check("segments (1, N)")
        n = int(d_sc.cpu().numpy().view(np.int32)[0])
        assert n == len(lines)
        segs = np.frombuffer(d_segs.cpu().numpy()[:n * SEG_BYTES].tobytes(), SEG_DTYPE)
        assert segs["line"].tolist() == list(range(n))
        assert segs["support"].tolist() == lines["strength"].tolist()
        k = 24
        exp = model_frames([e], sinQ, cosQ, [lines[:k]], [(7, 3)])[(7, 3)]
        A.refill(d_segs); A.refill(d_sc)
        plan.houghsht_segments(ptr(d_e), ptr(d_lines), ptr(d_counts), line_cap, k, 7, 3, ptr(d_segs), seg_cap, ptr(d_sc))
        A.check("segments (7, 3)")
        assert_segments(d_segs, d_sc, 1, seg_cap, exp, "wide (7, 3)")
        assert len(exp[0]) >= 3
    finally:
        plan.close()


def test_support_is_strength_for_every_line_of_a_4k_batch(hip_ctx):
    """One 32 x 4K pipeline step, then the (1, N) segments of every line from the step's own masks: a line's single segment carries its strength."""
    import torch
    from compv_amd import capi
    from oracle_bindings import synth_frame
    W, H, F, theta, thr = 3840, 2160, 32, 1.0, 100
    base = [synth_frame(W, H, 12345 + k) for k in range(4)]
    dev = torch.device("cuda:0")
    d_in = torch.empty((F, H, W), dtype=torch.uint8, device=dev)
    for f in range(F):
        d_in[f] = torch.from_numpy(np.roll(base[f % 4], 37 * (f // 4), axis=1))
    line_cap = 1 << 16          # the benchmark's capacity
    d_e = torch.empty_like(d_in)
    d_lines = torch.zeros(F * line_cap * LINE_BYTES, dtype=torch.uint8, device=dev)
    d_counts = torch.zeros(F, dtype=torch.int32, device=dev)
    d_segs = torch.zeros(F * line_cap * SEG_BYTES, dtype=torch.uint8, device=dev)
    d_sc = torch.zeros(F, dtype=torch.int32, device=dev)
    plan = capi.Plan(hip_ctx, W, H, W, F, theta)
    try:
        plan.pipeline(ptr(d_in), T_LOW, T_HIGH, thr, 0, ptr(d_e), ptr(d_lines), line_cap, ptr(d_counts))
        plan.houghsht_segments(0, ptr(d_lines), ptr(d_counts), line_cap, 0, 1, max(W, H), ptr(d_segs), line_cap, ptr(d_sc))
        torch.cuda.synchronize()
        lines, counts = lines_of(d_lines, d_counts, F, line_cap)
        sc = d_sc.cpu().numpy()
        raw = d_segs.cpu().numpy().reshape(F, line_cap * SEG_BYTES)
        assert int(counts.min()) > 100 and int(counts.max()) <= line_cap, (counts.min(), counts.max())
        for f in range(F):
            n = len(lines[f])
            assert int(sc[f]) == n, f
            segs = np.frombuffer(raw[f][:n * SEG_BYTES].tobytes(), SEG_DTYPE)
            assert (segs["line"] == np.arange(n)).all(), f
            assert (segs["support"] == lines[f]["strength"]).all(), f
            assert ((segs["x0"] >= 0) & (segs["x1"] < W) & (segs["y0"] >= 0) & (segs["y1"] < H) & (segs["y0"] < H) & (segs["x0"] < W)).all(), f
    finally:
        plan.close()


def _busy_empty_busy(hip_ctx, oracle):
    """A 3-frame plan whose middle frame is all zero (no edges, no lines), after Canny + SHT; returns everything a capacity test needs."""
    from compv_amd import capi
    W, H, S, F, theta = 333, 77, 336, 3, 1.0
    from oracle_bindings import synth_frame
    imgs = np.stack([synth_frame(W, H, 5), np.zeros((H, W), np.uint8), synth_frame(W, H, 77)])
    rng = np.random.default_rng(1)
    A = Arena()
    host_in = pad_frames(imgs, S, rng)
    d_in = A.new(F * H * S, host_in)
    d_e = A.new(F * H * S)
    line_cap = 64
    d_lines = A.new(F * line_cap * LINE_BYTES)
    d_counts = A.new(F * 4)
    plan = capi.Plan(hip_ctx, W, H, S, F, theta)
    plan.canny(ptr(d_in), T_LOW, T_HIGH, ptr(d_e))
    plan.houghsht(0, 20, 0, ptr(d_lines), line_cap, ptr(d_counts))
    A.check("setup")
    edges = frames_view(d_e, F, H, S, W).copy()
    lines, counts = lines_of(d_lines, d_counts, F, line_cap)
    assert int(counts[1]) == 0 and int(counts[0]) > 3 and int(counts[2]) > 3
    sinQ, cosQ = tables(oracle, W, H, theta)
    return dict(W=W, H=H, S=S, F=F, theta=theta, A=A, plan=plan, d_in=d_in, d_e=d_e, d_lines=d_lines, d_counts=d_counts, line_cap=line_cap,
                edges=edges, lines=lines, sinQ=sinQ, cosQ=cosQ)


def test_capacity_max_lines_and_empty_frames(hip_ctx, oracle):
    """segCap below the count: the records written are the prefix of the uncapped run and the counts do not change; maxLines cuts the
    line array; a frame without lines between two busy ones counts zero and is not written."""
    k = _busy_empty_busy(hip_ctx, oracle)
    A, plan, F = k["A"], k["plan"], k["F"]
    try:
        p = (3, 1)
        exp = model_frames(k["edges"], k["sinQ"], k["cosQ"], k["lines"], [p])[p]
        assert len(exp[1]) == 0 and min(len(exp[0]), len(exp[2])) > 12
        big = max(len(e) for e in exp) + 5
        for seg_cap in (big, 7, 1):
            d_segs = A.new(F * seg_cap * SEG_BYTES)
            d_sc = A.new(F * 4)
            plan.houghsht_segments(0, ptr(k["d_lines"]), ptr(k["d_counts"]), k["line_cap"], 0, p[0], p[1], ptr(d_segs), seg_cap, ptr(d_sc))
            A.check("segCap %d" % seg_cap)
            assert_segments(d_segs, d_sc, F, seg_cap, exp, "segCap %d" % seg_cap)
        for max_lines in (1, 3, 10 ** 6):
            cut = model_frames(k["edges"], k["sinQ"], k["cosQ"], k["lines"], [p], max_lines=max_lines)[p]
            d_segs = A.new(F * big * SEG_BYTES)
            d_sc = A.new(F * 4)
            plan.houghsht_segments(ptr(k["d_e"]), ptr(k["d_lines"]), ptr(k["d_counts"]), k["line_cap"], max_lines, p[0], p[1], ptr(d_segs), big, ptr(d_sc))
            A.check("maxLines %d" % max_lines)
            assert_segments(d_segs, d_sc, F, big, cut, "maxLines %d" % max_lines)
        assert len(model_frames(k["edges"], k["sinQ"], k["cosQ"], k["lines"], [p], max_lines=1)[p][0]) < len(exp[0])
    finally:
        plan.close()


def test_refusals(hip_ctx, oracle):
    from compv_amd import capi
    k = _busy_empty_busy(hip_ctx, oracle)
    A, plan, F, W, H, S = k["A"], k["plan"], k["F"], k["W"], k["H"], k["S"]
    seg_cap = 512
    d_segs = A.new(F * seg_cap * SEG_BYTES)
    d_sc = A.new(F * 4)

    def call(pl, de, min_length=3, max_gap=1, cap=seg_cap):
        pl.houghsht_segments(de, ptr(k["d_lines"]), ptr(k["d_counts"]), k["line_cap"], 0, min_length, max_gap, ptr(d_segs), cap, ptr(d_sc))

    def refused(code, *a, **kw):
        with pytest.raises(capi.CompvHipError) as err:
            call(*a, **kw)
        assert err.value.code == code, err.value
        A.check("refused call")
        assert (d_segs.cpu().numpy() == SENTINEL).all() and (d_sc.cpu().numpy() == SENTINEL).all()      # a refused call writes nothing

    fresh = capi.Plan(hip_ctx, W, H, S, F, k["theta"])
    try:
        refused(capi.E_INVALID_PARAMETER, plan, 0, min_length=0)
        refused(capi.E_INVALID_PARAMETER, plan, 0, max_gap=-1)
        refused(capi.E_INVALID_PARAMETER, plan, 0, cap=0)
        refused(capi.E_INVALID_PARAMETER, fresh, 0)                     # no Canny ran on this plan: it has no masks
        call(fresh, ptr(k["d_e"]))                                      # ... but it serves explicit edge maps
        A.check("fresh plan, explicit edges")
        want = (d_segs.cpu().numpy().copy(), d_sc.cpu().numpy().copy())
        A.refill(d_segs); A.refill(d_sc)

        # an asynchronous step in flight: refused until it was waited for
        d_e2 = A.new(F * H * S)
        t = plan.pipeline_async(ptr(k["d_in"]), T_LOW, T_HIGH, 20, 0, ptr(d_e2), ptr(k["d_lines"]), k["line_cap"], ptr(k["d_counts"]))
        with pytest.raises(capi.CompvHipError) as err:
            call(plan, 0)
        assert err.value.code == capi.E_INVALID_STATE
        plan.wait(t)
        A.check("async step")
        assert (d_segs.cpu().numpy() == SENTINEL).all()
        call(plan, 0)                                                    # same frames, same thresholds: the same lines and masks as before
        A.check("after wait")
        assert (d_segs.cpu().numpy() == want[0]).all() and (d_sc.cpu().numpy() == want[1]).all()
        exp = model_frames(k["edges"], k["sinQ"], k["cosQ"], k["lines"], [(3, 1)])[(3, 1)]
        assert_segments(d_segs, d_sc, F, seg_cap, exp, "after wait")
    finally:
        fresh.close()
        plan.close()

    # host entry point
    L = hip_ctx.lib
    e0 = np.ascontiguousarray(k["edges"][0])
    R, T, _ = oracle.sht_dims(W, H, k["theta"])
    lines = hip_ctx.houghsht(e0, k["theta"], 20)
    full = hip_ctx.houghsht_segments(e0, lines, k["theta"], 3, 1)
    assert len(full) > 4
    segs = np.zeros(4, SEG_DTYPE)
    n = C.c_size_t(0)

    def host(ln, min_length=3, max_gap=1, cap=4):
        return L.compvhip_houghsht_segments_u8(hip_ctx.h, e0.ctypes.data, W, H, W, k["theta"], ln.ctypes.data, len(ln), min_length, max_gap,
                                               segs.ctypes.data, cap, C.byref(n))
    assert host(lines) == capi.E_OUT_OF_BOUND and n.value == len(full)
    assert segs.tobytes() == full[:4].tobytes()                         # the first cap records were written
    assert host(lines, cap=0) == capi.E_OUT_OF_BOUND and n.value == len(full)
    assert host(lines, min_length=0) == capi.E_INVALID_PARAMETER
    assert host(lines, max_gap=-1) == capi.E_INVALID_PARAMETER
    for field, v in (("row", R), ("row", -1), ("col", T), ("col", -1)):
        bad = lines.copy()
        bad[field][len(bad) // 2] = v
        assert host(bad) == capi.E_INVALID_PARAMETER, (field, v)
    assert host(lines[:0]) == capi.OK and n.value == 0


def test_allocations_go_with_plan_and_context(oracle):
    from compv_amd import capi
    ctx = capi.Context(0)
    try:
        live0 = ctx.live_allocations()
        k = _busy_empty_busy(ctx, oracle)
        A, plan, F = k["A"], k["plan"], k["F"]
        d_segs = A.new(F * 256 * SEG_BYTES)
        d_sc = A.new(F * 4)
        try:
            for line_cap in (16, k["line_cap"]):                         # the per-line scratch grows with the line capacity
                plan.houghsht_segments(0, ptr(k["d_lines"]), ptr(k["d_counts"]), line_cap, 0, 2, 1, ptr(d_segs), 256, ptr(d_sc))
            A.check("segments")
            assert ctx.live_allocations() > live0
        finally:
            plan.close()
        assert ctx.live_allocations() == live0                           # every plan buffer, the segment scratch included
        e0 = np.ascontiguousarray(k["edges"][0])
        lines = ctx.houghsht(e0, k["theta"], 20)
        a = ctx.houghsht_segments(e0, lines, k["theta"], 2, 1)
        live1 = ctx.live_allocations()
        b = ctx.houghsht_segments(e0, lines, k["theta"], 2, 1)
        assert a.tobytes() == b.tobytes() and len(a) > 0
        assert ctx.live_allocations() == live1                           # the staging buffers are reused, not re-allocated
    finally:
        ctx.close()
    assert ctx.h is None
