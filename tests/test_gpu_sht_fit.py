"""Hough line refinement on the GPU (compvhip_plan_houghsht_fit, compvhip_houghsht_fit_u8) against the numpy model of the definition
(tests/sht_fit_model.py, pinned on the CPU by tests/test_sht_fit_model.py).

The bar: `line`, `pixels`, the five moments and the counts bit for bit; nx, ny, rho, rms2 equal as binary64 VALUES (compared with ==, so
the sign of a zero is not part of the contract) -- they are + - * / sqrt on exact integers, rounded once per operation in a fixed order,
so a difference is an operation-order or contraction bug, not a tolerance question.  Only `theta` of a refined line goes through a libm
function (atan2): it must stay within 1 float32 ulp of np.float32(np.arctan2(ny, nx)); the share that is exactly equal is printed.

Device buffers sit between guards and start filled with a sentinel (the Arena of tests/gpu_support.py); the geometries are
those of tests/plan_geometries.py.
"""
import ctypes as C

import numpy as np
import pytest

from gpu_support import FIT_BYTES, LINE_BYTES, SEG_BYTES, SENTINEL, T_HIGH, T_LOW, Arena, frames_view, make_batch, pad_frames, ptr, sht_threshold
from plan_geometries import GEOMETRIES
from sht_fit_model import FIT_DTYPE, frame_fits
from sht_fit_rig import assert_fits, assert_refined, model_fits, same_records, segs_of, tables
from sht_segments_rig import cells_of, lines_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("W,H,S,F,theta", GEOMETRIES, ids=lambda v: str(v))
def test_fit_geometry_sweep(hip_ctx, oracle, W, H, S, F, theta):
    """Both modes and both entry points against the model, b in {0, 1, 8}: the plan's canonical-order lines on its own Canny masks
    (d_edges == NULL) and on the same maps passed as bytes -- identical buffers --, per line (with refined lines) and per segment; the host
    entry point on its reference-order lines, rows at stride S."""
    from compv_amd import capi
    seed = W * 7 + H * 3 + F
    rng = np.random.default_rng(seed)
    imgs = make_batch(W, H, F, seed)
    R, (sinQ, cosQ) = tables(oracle, W, H, theta)
    thr = sht_threshold(W, H)
    line_cap, seg_cap = 40, 512
    A = Arena()
    host_in = pad_frames(imgs, S, rng)
    d_in = A.new(F * H * S, host_in)
    A.keep(d_in, host_in)
    d_e = A.new(F * H * S)
    d_lines = A.new(F * line_cap * LINE_BYTES)
    d_counts = A.new(F * 4)
    d_segs = A.new(F * seg_cap * SEG_BYTES)
    d_sc = A.new(F * 4)
    d_fits = A.new(F * seg_cap * FIT_BYTES)
    d_fc = A.new(F * 4)
    d_ref = A.new(F * line_cap * LINE_BYTES)
    plan = capi.Plan(hip_ctx, W, H, S, F, theta)
    try:
        plan.canny(ptr(d_in), T_LOW, T_HIGH, ptr(d_e))
        plan.houghsht(0, thr, 0, ptr(d_lines), line_cap, ptr(d_counts))
        plan.houghsht_segments(0, ptr(d_lines), ptr(d_counts), line_cap, 0, 3, 1, ptr(d_segs), seg_cap, ptr(d_sc))
        A.check("canny + houghsht + segments")
        edges = frames_view(d_e, F, H, S, W).copy()
        lines, counts = lines_of(d_lines, d_counts, F, line_cap)
        segs = segs_of(d_segs, d_sc, F, seg_cap)
        for d in (d_e, d_lines, d_counts, d_segs, d_sc):
            A.keep(d, d.cpu().numpy())
        total = 0
        for b in (0, 1, 8):
            per_line, valid = model_fits(edges, sinQ, cosQ, R, lines, b)
            per_seg, _ = model_fits(edges, sinQ, cosQ, R, lines, b, segs=segs)
            total += sum(int(v) for vv in valid for v in vv)
            got = {}
            for how, de in (("masks", 0), ("bytes", ptr(d_e))):
                for d in (d_fits, d_fc, d_ref):
                    A.refill(d)
                plan.houghsht_fit(de, ptr(d_lines), ptr(d_counts), line_cap, 0, b, 0, 0, 0, ptr(d_fits), seg_cap, ptr(d_fc), ptr(d_ref))
                A.check("fit per line %s b=%d" % (how, b))
                assert_fits(d_fits, d_fc, F, seg_cap, per_line, "per line %s b=%d" % (how, b))
                raw = d_ref.cpu().numpy().reshape(F, line_cap * LINE_BYTES)
                for f in range(F):
                    n = len(lines[f])
                    assert (raw[f][n * LINE_BYTES:] == SENTINEL).all(), ("refined lines beyond the count were written", f)
                    if n:
                        assert_refined(np.frombuffer(raw[f][:n * LINE_BYTES].tobytes(), capi.LINE_DTYPE), lines[f], per_line[f], valid[f], "refined %s b=%d f=%d" % (how, b, f))
                got[how] = [d_fits.cpu().numpy().tobytes(), d_fc.cpu().numpy().tobytes(), d_ref.cpu().numpy().tobytes()]
                for d in (d_fits, d_fc):
                    A.refill(d)
                plan.houghsht_fit(de, ptr(d_lines), ptr(d_counts), line_cap, 0, b, ptr(d_segs), ptr(d_sc), seg_cap, ptr(d_fits), seg_cap, ptr(d_fc))
                A.check("fit per segment %s b=%d" % (how, b))
                assert_fits(d_fits, d_fc, F, seg_cap, per_seg, "per segment %s b=%d" % (how, b))
                got[how] += [d_fits.cpu().numpy().tobytes(), d_fc.cpu().numpy().tobytes()]
            assert got["masks"] == got["bytes"], b
            if b == 0:
                for f in range(F):
                    assert per_line[f]["pixels"].tolist() == lines[f]["strength"].tolist(), f      # the band of width 0 is the line's support
        assert total > 0 or max(len(l) for l in lines) == 0

        # host entry point: lines in the reference's order, rows of the caller's map at stride S
        for f in sorted({0, F - 1}):
            padded = np.full((H, S), 255, np.uint8)
            padded[:, :W] = edges[f]
            view = padded[:, :W]
            hl = hip_ctx.houghsht(view, theta, thr)
            hs = hip_ctx.houghsht_segments(view, hl, theta, 3, 1)
            for b in (0, 1, 8):
                want, valid = frame_fits(edges[f], sinQ, cosQ, cells_of(hl), b, R)
                got, ref = hip_ctx.houghsht_fit(view, hl, theta, b, want_refined=True)
                same_records(got, want, "host per line f=%d b=%d" % (f, b))
                if len(hl):
                    assert_refined(ref, hl, want, valid, "host refined f=%d b=%d" % (f, b))
                want, _ = frame_fits(edges[f], sinQ, cosQ, cells_of(hl), b, R, segs=hs)
                same_records(hip_ctx.houghsht_fit(view, hl, theta, b, segs=hs), want, "host per segment f=%d b=%d" % (f, b))
    finally:
        plan.close()


def _drawn_map(W, H, seed, density):
    """Sparse noise plus a few long drawn lines (horizontal, vertical, two diagonals) and a slightly tilted one."""
    rng = np.random.default_rng(seed)
    e = (rng.random((H, W), dtype=np.float32) < density).astype(np.uint8) * 255
    e[H // 3, W // 8:W - W // 8] = 255
    e[:, W // 2] = 255
    n = min(W, H)
    i = np.arange(n)
    e[i, i + (W - n) // 2] = 255
    e[n - 1 - i, i + (W - n) // 3] = 255
    x = np.arange(W)
    e[np.clip(H // 5 + (x * 7) // 1000, 0, H - 1), x] = 255
    return e


def test_8192_square_at_the_widest_band(hip_ctx, oracle):
    """The largest geometry the call accepts, b = 8: the sums reach their largest values (int64 central moments, rule 3)."""
    from compv_amd import capi
    W = H = S = 8192
    theta, thr, b = 1.0, 1500, 8
    e = _drawn_map(W, H, W + H, 0.004)
    R, (sinQ, cosQ) = tables(oracle, W, H, theta)
    A = Arena()
    d_e = A.new(H * S, e)
    A.keep(d_e, e)
    line_cap, k = 4096, 24
    d_lines = A.new(line_cap * LINE_BYTES)
    d_counts = A.new(4)
    d_fits = A.new(k * FIT_BYTES)
    d_fc = A.new(4)
    d_ref = A.new(line_cap * LINE_BYTES)
    plan = capi.Plan(hip_ctx, W, H, S, 1, theta)
    try:
        plan.houghsht(ptr(d_e), thr, 0, ptr(d_lines), line_cap, ptr(d_counts))
        (lines,), counts = lines_of(d_lines, d_counts, 1, line_cap)
        assert 4 <= int(counts[0]) <= line_cap, int(counts[0])
        A.keep(d_lines, d_lines.cpu().numpy()); A.keep(d_counts, d_counts.cpu().numpy())
        plan.houghsht_fit(ptr(d_e), ptr(d_lines), ptr(d_counts), line_cap, k, b, 0, 0, 0, ptr(d_fits), k, ptr(d_fc), ptr(d_ref))
        A.check("fit 8192")
        exp, valid = model_fits([e], sinQ, cosQ, R, [lines], b, max_lines=k)
        assert_fits(d_fits, d_fc, 1, k, exp, "8192 x 8192 b=8")
        n = len(exp[0])
        assert n == min(k, len(lines)) and all(valid[0]) and int(exp[0]["pixels"].max()) > 8192
        raw = d_ref.cpu().numpy()
        assert (raw[n * LINE_BYTES:] == SENTINEL).all()
        assert_refined(np.frombuffer(raw[:n * LINE_BYTES].tobytes(), capi.LINE_DTYPE), lines[:n], exp[0], valid[0], "8192 refined")
    finally:
        plan.close()


def test_32_frames_of_4k_from_the_step_masks(hip_ctx, oracle):
    """One 32 x 4K pipeline step, then the fits of every line from the step's own masks: b = 0 counts the strength of every line of every
    frame; b = 2 against the model on the first and the last frame (the strongest lines, and a stride through the rest)."""
    import torch
    from compv_amd import capi
    from oracle_bindings import synth_frame
    W, H, F, theta, thr = 3840, 2160, 32, 1.0, 100
    base = [synth_frame(W, H, 12345 + k) for k in range(4)]
    dev = torch.device("cuda:0")
    d_in = torch.empty((F, H, W), dtype=torch.uint8, device=dev)
    for f in range(F):
        d_in[f] = torch.from_numpy(np.roll(base[f % 4], 37 * (f // 4), axis=1))
    line_cap = 1 << 16
    d_e = torch.empty_like(d_in)
    d_lines = torch.zeros(F * line_cap * LINE_BYTES, dtype=torch.uint8, device=dev)
    d_counts = torch.zeros(F, dtype=torch.int32, device=dev)
    d_fits = torch.zeros(F * line_cap * FIT_BYTES, dtype=torch.uint8, device=dev)
    d_fc = torch.zeros(F, dtype=torch.int32, device=dev)
    R, (sinQ, cosQ) = tables(oracle, W, H, theta)
    plan = capi.Plan(hip_ctx, W, H, W, F, theta)
    try:
        plan.pipeline(ptr(d_in), T_LOW, T_HIGH, thr, 0, ptr(d_e), ptr(d_lines), line_cap, ptr(d_counts))
        plan.houghsht_fit(0, ptr(d_lines), ptr(d_counts), line_cap, 0, 0, 0, 0, 0, ptr(d_fits), line_cap, ptr(d_fc))
        torch.cuda.synchronize()
        lines, counts = lines_of(d_lines, d_counts, F, line_cap)
        fc = d_fc.cpu().numpy()
        raw = d_fits.cpu().numpy().reshape(F, line_cap * FIT_BYTES)
        assert int(counts.min()) > 100 and int(counts.max()) <= line_cap, (counts.min(), counts.max())
        for f in range(F):
            n = len(lines[f])
            assert int(fc[f]) == n, f
            fits = np.frombuffer(raw[f][:n * FIT_BYTES].tobytes(), FIT_DTYPE)
            assert (fits["line"] == np.arange(n)).all() and (fits["pixels"] == lines[f]["strength"]).all(), f
        plan.houghsht_fit(0, ptr(d_lines), ptr(d_counts), line_cap, 0, 2, 0, 0, 0, ptr(d_fits), line_cap, ptr(d_fc))
        torch.cuda.synchronize()
        raw = d_fits.cpu().numpy().reshape(F, line_cap * FIT_BYTES)
        for f in (0, F - 1):
            e = d_e[f].cpu().numpy()
            n = len(lines[f])
            fits = np.frombuffer(raw[f][:n * FIT_BYTES].tobytes(), FIT_DTYPE)
            pick = sorted(set(range(min(n, 12))) | set(range(12, n, max(1, n // 24))))
            want, _ = frame_fits(e, sinQ, cosQ, [cells_of(lines[f])[i] for i in pick], 2, R)
            want["line"] = pick
            same_records(fits[pick], want, "4K frame %d b=2" % f)
    finally:
        plan.close()


def _three_frames(hip_ctx, oracle, kinds):
    """A 3-frame plan after Canny + SHT (or SHT on byte maps given in `kinds`): everything a capacity / content test needs."""
    from compv_amd import capi
    from oracle_bindings import synth_frame
    W, H, S, F, theta = 333, 77, 336, 3, 1.0
    A = Arena()
    line_cap = 64
    d_lines = A.new(F * line_cap * LINE_BYTES)
    d_counts = A.new(F * 4)
    plan = capi.Plan(hip_ctx, W, H, S, F, theta)
    rng = np.random.default_rng(1)
    if kinds == "canny":
        imgs = np.stack([synth_frame(W, H, 5), np.zeros((H, W), np.uint8), synth_frame(W, H, 77)])
        host_in = pad_frames(imgs, S, rng)
        d_in = A.new(F * H * S, host_in)
        d_e = A.new(F * H * S)
        plan.canny(ptr(d_in), T_LOW, T_HIGH, ptr(d_e))
        plan.houghsht(0, 20, 0, ptr(d_lines), line_cap, ptr(d_counts))
    else:
        maps = np.stack([np.full((H, W), 255, np.uint8), np.zeros((H, W), np.uint8), (rng.random((H, W)) < 0.1).astype(np.uint8) * 3])
        host_e = pad_frames(maps, S, rng)         # the padding columns hold random bytes, 255 included: columns >= W are never edges
        d_in = None
        d_e = A.new(F * H * S, host_e)
        plan.houghsht(ptr(d_e), 20, 0, ptr(d_lines), line_cap, ptr(d_counts))
    A.check("setup")
    edges = frames_view(d_e, F, H, S, W).copy()
    lines, counts = lines_of(d_lines, d_counts, F, line_cap)
    R, (sinQ, cosQ) = tables(oracle, W, H, theta)
    return dict(W=W, H=H, S=S, F=F, theta=theta, A=A, plan=plan, d_in=d_in, d_e=d_e, d_lines=d_lines, d_counts=d_counts, line_cap=line_cap, edges=edges,
                lines=lines, counts=counts, sinQ=sinQ, cosQ=cosQ, R=R)


def test_all_foreground_and_empty_frames(hip_ctx, oracle):
    """Every pixel an edge (25 band pixels per position at b = 8), a frame without edges between two busy ones (no lines: count zero,
    nothing written), sparse noise with byte values other than 255."""
    k = _three_frames(hip_ctx, oracle, "maps")
    A, plan, F, cap = k["A"], k["plan"], k["F"], k["line_cap"]
    try:
        assert int(k["counts"][1]) == 0 and int(k["counts"][0]) > 3 and int(k["counts"][2]) > 3
        d_fits = A.new(F * cap * FIT_BYTES)
        d_fc = A.new(F * 4)
        for b in (0, 8):
            exp, valid = model_fits(k["edges"], k["sinQ"], k["cosQ"], k["R"], k["lines"], b)
            A.refill(d_fits); A.refill(d_fc)
            plan.houghsht_fit(ptr(k["d_e"]), ptr(k["d_lines"]), ptr(k["d_counts"]), cap, 0, b, 0, 0, 0, ptr(d_fits), cap, ptr(d_fc))
            A.check("fit b=%d" % b)
            assert_fits(d_fits, d_fc, F, cap, exp, "content b=%d" % b)
            assert len(exp[0]) == min(int(k["counts"][0]), cap) and len(exp[1]) == 0
        assert int(exp[0]["pixels"].max()) > 17 * 77
    finally:
        plan.close()


def test_capacity_is_a_prefix_and_max_lines_cuts(hip_ctx, oracle):
    k = _three_frames(hip_ctx, oracle, "canny")
    A, plan, F, cap = k["A"], k["plan"], k["F"], k["line_cap"]
    try:
        b = 3
        exp, valid = model_fits(k["edges"], k["sinQ"], k["cosQ"], k["R"], k["lines"], b)
        assert len(exp[1]) == 0 and min(len(exp[0]), len(exp[2])) > 8
        for fit_cap in (cap, 5, 1):
            d_fits = A.new(F * fit_cap * FIT_BYTES)
            d_fc = A.new(F * 4)
            plan.houghsht_fit(0, ptr(k["d_lines"]), ptr(k["d_counts"]), cap, 0, b, 0, 0, 0, ptr(d_fits), fit_cap, ptr(d_fc))
            A.check("fitCap %d" % fit_cap)
            assert_fits(d_fits, d_fc, F, fit_cap, exp, "fitCap %d" % fit_cap)
        # counts only
        d_fc = A.new(F * 4)
        plan.houghsht_fit(0, ptr(k["d_lines"]), ptr(k["d_counts"]), cap, 0, b, 0, 0, 0, 0, 0, ptr(d_fc))
        A.check("fitCap 0")
        assert d_fc.cpu().numpy().view(np.int32).tolist() == [len(e) for e in exp]
        for max_lines in (1, 3, 10 ** 6):
            cut, _ = model_fits(k["edges"], k["sinQ"], k["cosQ"], k["R"], k["lines"], b, max_lines=max_lines)
            d_fits = A.new(F * cap * FIT_BYTES)
            d_fc = A.new(F * 4)
            plan.houghsht_fit(ptr(k["d_e"]), ptr(k["d_lines"]), ptr(k["d_counts"]), cap, max_lines, b, 0, 0, 0, ptr(d_fits), cap, ptr(d_fc))
            A.check("maxLines %d" % max_lines)
            assert_fits(d_fits, d_fc, F, cap, cut, "maxLines %d" % max_lines)
        # per segment: segCap clips the segments that are read, fitCap the records that are written
        seg_cap = 256
        d_segs = A.new(F * seg_cap * SEG_BYTES)
        d_sc = A.new(F * 4)
        plan.houghsht_segments(0, ptr(k["d_lines"]), ptr(k["d_counts"]), cap, 0, 3, 1, ptr(d_segs), seg_cap, ptr(d_sc))
        segs = segs_of(d_segs, d_sc, F, seg_cap)
        assert max(len(s) for s in segs) > 12
        for use_cap, fit_cap in ((seg_cap, seg_cap), (9, 256), (seg_cap, 4)):
            want, _ = model_fits(k["edges"], k["sinQ"], k["cosQ"], k["R"], k["lines"], b, segs=[s[:use_cap] for s in segs])
            d_fits = A.new(F * fit_cap * FIT_BYTES)
            d_fc = A.new(F * 4)
            if use_cap == seg_cap:
                plan.houghsht_fit(0, ptr(k["d_lines"]), ptr(k["d_counts"]), cap, 0, b, ptr(d_segs), ptr(d_sc), use_cap, ptr(d_fits), fit_cap, ptr(d_fc))
            else:       # a segment array of capacity 9 per frame: the prefix of each frame's segments, repacked
                packed = np.full((F, use_cap * SEG_BYTES), SENTINEL, np.uint8)
                for f in range(F):
                    raw = segs[f][:use_cap].tobytes()
                    packed[f, :len(raw)] = np.frombuffer(raw, np.uint8)
                d_small = A.new(F * use_cap * SEG_BYTES, packed.reshape(-1))
                plan.houghsht_fit(0, ptr(k["d_lines"]), ptr(k["d_counts"]), cap, 0, b, ptr(d_small), ptr(d_sc), use_cap, ptr(d_fits), fit_cap, ptr(d_fc))
            A.check("per segment caps %d %d" % (use_cap, fit_cap))
            assert_fits(d_fits, d_fc, F, fit_cap, want, "per segment caps %d %d" % (use_cap, fit_cap))
    finally:
        plan.close()


def test_refined_lines_feed_to_cartesian(hip_ctx, oracle):
    """compvhip_plan_to_cartesian on d_refined against the host helper on the same floats.  A refined theta is not a table entry, so the device
    evaluates cos and sin itself: both sides round cos, sin, 1 / sin, W * cos, rho - W * cos and the product by 1 / sin to float32, i.e. at
    most 6 roundings of relative size 2^-24 on quantities bounded by (|rho| + W) / |sin theta|.  The bound below allows 8 on either side;
    the share of bit-equal endpoints is printed."""
    from compv_amd import capi
    k = _three_frames(hip_ctx, oracle, "canny")
    A, plan, F, cap, W, H = k["A"], k["plan"], k["F"], k["line_cap"], k["W"], k["H"]
    try:
        d_ref = A.new(F * cap * LINE_BYTES)
        d_fc = A.new(F * 4)
        d_cart = A.new(F * cap * 16)
        d_cart0 = A.new(F * cap * 16)
        plan.houghsht_fit(0, ptr(k["d_lines"]), ptr(k["d_counts"]), cap, 0, 3, 0, 0, 0, 0, 0, ptr(d_fc), ptr(d_ref))
        plan.to_cartesian(ptr(d_ref), ptr(k["d_counts"]), cap, ptr(d_cart))
        plan.to_cartesian(ptr(k["d_lines"]), ptr(k["d_counts"]), cap, ptr(d_cart0))
        A.check("fit + to_cartesian")
        ref = d_ref.cpu().numpy().reshape(F, cap * LINE_BYTES)
        cart = d_cart.cpu().numpy().view(np.float32).reshape(F, cap, 4)
        cart0 = d_cart0.cpu().numpy().view(np.float32).reshape(F, cap, 4)
        equal = total = moved = 0
        for f in range(F):
            n = len(k["lines"][f])
            assert (d_cart.cpu().numpy().reshape(F, cap * 16)[f][n * 16:] == SENTINEL).all()
            if not n:
                continue
            r = np.frombuffer(ref[f][:n * LINE_BYTES].tobytes(), capi.LINE_DTYPE)
            want = capi.to_cartesian(W, H, [(float(l["rho"]), float(l["theta"])) for l in r])
            # the unrefined lines still take the table path: bit-exact against the host helper, as before
            want0 = capi.to_cartesian(W, H, [(float(l["rho"]), float(l["theta"])) for l in k["lines"][f]])
            assert (cart0[f][:n].view(np.uint32) == want0.view(np.uint32)).all(), f
            rho, th = r["rho"].astype(np.float64), r["theta"].astype(np.float64)
            tol = 16 * 2.0 ** -24 * (np.abs(rho) + W) / np.abs(np.sin(th))
            assert (np.abs(cart[f][:n].astype(np.float64) - want.astype(np.float64)) <= tol[:, None]).all(), f
            equal += int((cart[f][:n].view(np.uint32) == want.view(np.uint32)).all(axis=1).sum())
            total += n
            moved += int((cart[f][:n] != cart0[f][:n]).any(axis=1).sum())
        print("to_cartesian of refined lines: %d of %d bit-equal to the host helper; %d differ from the unrefined lines'" % (equal, total, moved))
        assert total > 8 and moved > 0
    finally:
        plan.close()


def test_refusals(hip_ctx, oracle):
    from compv_amd import capi
    k = _three_frames(hip_ctx, oracle, "canny")
    A, plan, F, W, H, S, cap = k["A"], k["plan"], k["F"], k["W"], k["H"], k["S"], k["line_cap"]
    d_fits = A.new(F * cap * FIT_BYTES)
    d_fc = A.new(F * 4)
    d_ref = A.new(F * cap * LINE_BYTES)
    d_segs = A.new(F * cap * SEG_BYTES, 0)
    d_sc = A.new(F * 4, 0)

    def call(pl, de, b=3, segs=0, sc=0, ref=0, lines=None, line_cap=cap, fits=None, fc=None):
        pl.houghsht_fit(de, ptr(k["d_lines"]) if lines is None else lines, ptr(k["d_counts"]), line_cap, 0, b, segs, sc, cap,
                        ptr(d_fits) if fits is None else fits, cap, ptr(d_fc) if fc is None else fc, ref)

    def refused(code, *a, **kw):
        with pytest.raises(capi.CompvHipError) as err:
            call(*a, **kw)
        assert err.value.code == code, err.value
        A.check("refused call")
        for d in (d_fits, d_fc, d_ref):
            assert (d.cpu().numpy() == SENTINEL).all()      # a refused call writes nothing

    fresh = capi.Plan(hip_ctx, W, H, S, F, k["theta"])
    wide = capi.Plan(hip_ctx, 8193, 16, 8200, F, k["theta"])
    tall = capi.Plan(hip_ctx, 16, 8193, 16, F, k["theta"])
    try:
        refused(capi.E_INVALID_PARAMETER, plan, 0, b=-1)
        refused(capi.E_INVALID_PARAMETER, plan, 0, b=9)
        refused(capi.E_INVALID_PARAMETER, plan, 0, segs=ptr(d_segs), sc=ptr(d_sc), ref=ptr(d_ref))       # refined lines are a per-line result
        refused(capi.E_INVALID_PARAMETER, plan, 0, segs=ptr(d_segs))                                      # segments without their counts
        refused(capi.E_INVALID_PARAMETER, plan, 0, line_cap=0)
        refused(capi.E_INVALID_PARAMETER, plan, 0, lines=0)
        refused(capi.E_INVALID_PARAMETER, plan, 0, fits=0)
        refused(capi.E_INVALID_PARAMETER, plan, 0, fc=0)
        refused(capi.E_INVALID_PARAMETER, fresh, 0)                     # no Canny ran on this plan: it has no masks
        refused(capi.E_NOT_IMPLEMENTED, wide, ptr(k["d_e"]))            # 8193 columns: the central moments could pass 2^63
        refused(capi.E_NOT_IMPLEMENTED, tall, ptr(k["d_e"]))
        call(fresh, ptr(k["d_e"]))                                      # ... but a plan without masks serves explicit edge maps
        A.check("fresh plan, explicit edges")
        want = (d_fits.cpu().numpy().copy(), d_fc.cpu().numpy().copy())
        A.refill(d_fits); A.refill(d_fc)

        # an asynchronous step in flight: refused until it was waited for
        d_e2 = A.new(F * H * S)
        t = plan.pipeline_async(ptr(k["d_in"]), T_LOW, T_HIGH, 20, 0, ptr(d_e2), ptr(k["d_lines"]), cap, ptr(k["d_counts"]))
        with pytest.raises(capi.CompvHipError) as err:
            call(plan, 0)
        assert err.value.code == capi.E_INVALID_STATE
        plan.wait(t)
        A.check("async step")
        assert (d_fits.cpu().numpy() == SENTINEL).all()
        call(plan, 0)                                                    # same frames, same thresholds: the same lines and masks as before
        A.check("after wait")
        assert (d_fits.cpu().numpy() == want[0]).all() and (d_fc.cpu().numpy() == want[1]).all()
        exp, _ = model_fits(k["edges"], k["sinQ"], k["cosQ"], k["R"], k["lines"], 3)
        assert_fits(d_fits, d_fc, F, cap, exp, "after wait")
    finally:
        fresh.close(); wide.close(); tall.close()
        plan.close()

    # host entry point
    L = hip_ctx.lib
    e0 = np.ascontiguousarray(k["edges"][0])
    R, T, _ = oracle.sht_dims(W, H, k["theta"])
    lines = hip_ctx.houghsht(e0, k["theta"], 20)
    full = hip_ctx.houghsht_fit(e0, lines, k["theta"], 3)
    segs = hip_ctx.houghsht_segments(e0, lines, k["theta"], 3, 1)
    assert len(full) == len(lines) > 4 and len(segs) > 4
    fits = np.zeros(4, FIT_DTYPE)
    refined = np.zeros(len(lines), capi.LINE_DTYPE)
    n = C.c_size_t(0)

    def host(ln, b=3, cap=4, sg=None, ref=None, e=e0, w=W, h=H):
        return L.compvhip_houghsht_fit_u8(hip_ctx.h, e.ctypes.data, w, h, w, k["theta"], ln.ctypes.data, len(ln), b, None if sg is None else sg.ctypes.data,
                                          0 if sg is None else len(sg), fits.ctypes.data, cap, C.byref(n), None if ref is None else ref.ctypes.data)
    assert host(lines) == capi.E_OUT_OF_BOUND and n.value == len(full)
    same_records(fits, full[:4], "host prefix")                         # the first cap records were written
    assert host(lines, cap=0) == capi.E_OUT_OF_BOUND and n.value == len(full)
    assert host(lines, sg=segs) == capi.E_OUT_OF_BOUND and n.value == len(segs)
    assert host(lines, b=-1) == capi.E_INVALID_PARAMETER and host(lines, b=9) == capi.E_INVALID_PARAMETER
    assert host(lines, sg=segs, ref=refined) == capi.E_INVALID_PARAMETER
    for field, v in (("row", R), ("row", -1), ("col", T), ("col", -1)):
        bad = lines.copy()
        bad[field][len(bad) // 2] = v
        assert host(bad) == capi.E_INVALID_PARAMETER, (field, v)
    for v in (-1, len(lines)):
        bad = segs.copy()
        bad["line"][1] = v
        assert host(lines, sg=bad) == capi.E_INVALID_PARAMETER, v
    assert host(lines[:0]) == capi.OK and n.value == 0
    big = np.zeros((3, 8193), np.uint8)
    assert host(lines[:1], e=big, w=8193, h=3) == capi.E_NOT_IMPLEMENTED
    big = np.zeros((8193, 3), np.uint8)
    assert host(lines[:1], e=big, w=3, h=8193) == capi.E_NOT_IMPLEMENTED


def test_allocations_go_with_plan_and_context(oracle):
    from compv_amd import capi
    ctx = capi.Context(0)
    try:
        live0 = ctx.live_allocations()
        k = _three_frames(ctx, oracle, "canny")
        A, plan, F, cap = k["A"], k["plan"], k["F"], k["line_cap"]
        d_fits = A.new(F * cap * FIT_BYTES)
        d_fc = A.new(F * 4)
        try:
            live1 = ctx.live_allocations()
            for line_cap in (16, cap):
                plan.houghsht_fit(0, ptr(k["d_lines"]), ptr(k["d_counts"]), line_cap, 0, 2, 0, 0, 0, ptr(d_fits), cap, ptr(d_fc))
            A.check("fit")
            assert ctx.live_allocations() == live1                       # no scratch beyond what the plan's SHT stage owns
        finally:
            plan.close()
        assert ctx.live_allocations() == live0
        e0 = np.ascontiguousarray(k["edges"][0])
        lines = ctx.houghsht(e0, k["theta"], 20)
        a = ctx.houghsht_fit(e0, lines, k["theta"], 2)
        live2 = ctx.live_allocations()
        b = ctx.houghsht_fit(e0, lines, k["theta"], 2)
        assert a.tobytes() == b.tobytes() and len(a) > 0
        assert ctx.live_allocations() == live2                           # the staging buffers are reused, not re-allocated
    finally:
        ctx.close()
    assert ctx.h is None
