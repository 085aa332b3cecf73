"""Connected components on the GPU (compvhip_plan_components, compvhip_components_u8) against the numpy / scipy model of the definition
(tests/components_model.py, pinned on the CPU by tests/test_components_model.py): label map, record array and counts, bit for bit -- the
definition is integer-only and unique, there is no tolerance anywhere and no frame of any case is left out.

Device buffers sit between guards and start filled with a sentinel (the Arena of tests/gpu_support.py); the geometries are those
of tests/plan_geometries.py (ragged widths, padded strides whose padding holds random non-zero bytes, batches).
"""
import ctypes as C

import numpy as np
import pytest

from components_model import COMP_DTYPE, components, summary
from components_rig import Out, assert_result, model
from gpu_support import SENTINEL, T_HIGH, T_LOW, Arena, frames_view, make_batch, pad_frames, ptr
from hysteresis_cases import BASE, maze_frame, spiral_frame
from plan_geometries import GEOMETRIES

pytestmark = pytest.mark.gpu


def dropping_min_pixels(maps, conn):
    """A minPixels that drops some components and keeps some, when the maps allow it."""
    px = np.concatenate([components(e, conn, 1)[1]["pixels"] for e in maps] + [np.zeros(0, np.int32)])
    if len(px) == 0:
        return 3
    if px.min() == px.max():
        return int(px.max()) + 1             # nothing to keep: everything is dropped
    med = int(np.sort(px)[len(px) // 2])
    return med + 1 if med < px.max() else med


@pytest.mark.parametrize("W,H,S,F,theta", GEOMETRIES, ids=lambda v: str(v))
def test_components_geometry_sweep(hip_ctx, W, H, S, F, theta):
    """The plan call on its own Canny masks (d_edges == NULL) and on the same edge maps passed as bytes -- identical buffers --, and the host
    entry point on rows at stride S whose padding is 255; both connectivities, minPixels 1 and a value that drops components, labelStride > W."""
    from compv_amd import capi
    seed = W * 7 + H * 3 + F
    rng = np.random.default_rng(seed)
    imgs = make_batch(W, H, F, seed)
    A = Arena()
    host_in = pad_frames(imgs, S, rng)
    d_in = A.new(F * H * S, host_in)
    A.keep(d_in, host_in)
    d_e = A.new(F * H * S)
    plan = capi.Plan(hip_ctx, W, H, S, F, theta)
    try:
        plan.canny(ptr(d_in), T_LOW, T_HIGH, ptr(d_e))
        A.check("canny")
        edges = frames_view(d_e, F, H, S, W).copy()          # bit-exact against the oracle in tests/test_gpu_plan_geometry.py
        # the byte path must ignore the padding columns, whatever they hold: give them random non-zero bytes
        host_e = pad_frames(edges, S, rng)
        d_eb = A.new(F * H * S, host_e)
        A.keep(d_eb, host_e)
        dropped = 0
        for conn in (8, 4):
            for mp in (1, dropping_min_pixels(edges, conn)):
                exp = model(edges, conn, mp)
                dropped += sum(len(components(e, conn, 1)[1]) - len(x[1]) for e, x in zip(edges, exp))
                cap = max(max(len(x[1]) for x in exp), 1) + 3
                got = {}
                for how, de in (("masks", 0), ("bytes", ptr(d_eb))):
                    out = Out(A, F, H, W + 5 if conn == 8 else W, cap)
                    out.call(plan, de, conn, mp)
                    A.check("components %s %d %d" % (how, conn, mp))
                    assert_result(out, W, exp, "components %s %d %d" % (how, conn, mp))
                    got[how] = out.raw()
                assert got["masks"] == got["bytes"], (conn, mp)
                # host entry point: first and last frame, rows at stride S with 255 in the padding
                for f in sorted({0, F - 1}):
                    padded = np.full((H, S), 255, np.uint8)
                    padded[:, :W] = edges[f]
                    lab, rec = hip_ctx.components(padded[:, :W], conn, mp, cap=2)      # grows through E_OUT_OF_BOUND when needed
                    assert np.array_equal(lab, exp[f][0]) and rec.tobytes() == exp[f][1].tobytes(), ("host", f, conn, mp)
        assert dropped > 0 or sum(len(components(e, 8, 1)[1]) for e in edges) < 2
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------
# adversarial shapes
# ---------------------------------------------------------------------------------------------------------------
def thin_serpentine(W, H):
    """One-pixel rows on every second row, joined alternately at the right and the left end: one component that crosses every tile column."""
    e = np.zeros((H, W), np.uint8)
    e[::2, :] = 1
    for k, y in enumerate(range(1, H - 1, 2)):
        e[y, W - 1 if k % 2 == 0 else 0] = 1
    return e


def combs(W, H):
    """Teeth from the top on every second column that join only in the last row (every tooth's top is a root until the very end), and in the
    lower right a second comb of horizontal teeth that join in its last column."""
    e = np.zeros((H, W), np.uint8)
    h = H // 2
    e[:h, ::2] = 1
    e[h - 1, :] = 1
    e[h + 2::2, : W - 3] = 1
    e[h + 2:, W - 4] = 1
    return e


def diagonals(W, H):
    """One-pixel diagonals, falling in the left half and rising in the right half: lines at 8-connectivity, isolated pixels at 4."""
    y, x = np.mgrid[0:H, 0:W]
    return np.where(x < W // 2, (x + y) % 7 == 0, (x - y) % 5 == 0).astype(np.uint8)


def four_borders(W, H):
    """A one-pixel X from corner to corner plus the frame's outline: one component at 8-connectivity that touches all four borders."""
    e = np.zeros((H, W), np.uint8)
    t = np.arange(max(W, H))
    e[t * (H - 1) // (len(t) - 1), t * (W - 1) // (len(t) - 1)] = 1
    e[(H - 1) - t * (H - 1) // (len(t) - 1), t * (W - 1) // (len(t) - 1)] = 1
    e[0, ::3] = 1; e[-1, ::2] = 1; e[::2, 0] = 1; e[::3, -1] = 1
    return e


def noise_and_lines(W, H, seed, density):
    rng = np.random.default_rng(seed)
    e = (rng.random((H, W), dtype=np.float32) < density).astype(np.uint8)
    e[H // 3, :] = 1
    e[:, W // 2] = 1
    n = min(W, H)
    i = np.arange(n)
    e[i, i + (W - n) // 2] = 1
    return e


def isolated(W, H):
    e = np.zeros((H, W), np.uint8)
    e[::2, ::2] = 255
    return e


ADVERSARIAL = {
    "all_foreground_4k": lambda: np.full((2160, 3840), 255, np.uint8),
    "isolated_4k": lambda: isolated(3840, 2160),
    "diagonals": lambda: diagonals(1031, 600),
    "spiral": lambda: (spiral_frame(2048, 1024) != BASE).astype(np.uint8),
    "serpentine": lambda: (maze_frame(2048, 1024) != BASE).astype(np.uint8),
    "thin_serpentine": lambda: thin_serpentine(1500, 901),
    "combs": lambda: combs(1500, 900),
    "four_borders": lambda: four_borders(1300, 700),
    "w33": lambda: noise_and_lines(33, 200, 3, 0.3),
    "w32767": lambda: noise_and_lines(32767, 64, 4, 0.3),
    "h32767": lambda: noise_and_lines(64, 32767, 5, 0.3),
}


@pytest.mark.parametrize("name", sorted(ADVERSARIAL))
def test_adversarial_shapes(hip_ctx, name):
    from compv_amd import capi
    e = ADVERSARIAL[name]()
    H, W = e.shape
    S = (W + 7) // 8 * 8 + 8
    host = np.full((H, S), 255, np.uint8)
    host[:, :W] = e
    A = Arena()
    d_e = A.new(H * S, host)
    A.keep(d_e, host)
    plan = capi.Plan(hip_ctx, W, H, S, 1, 1.0)
    try:
        for conn in (8, 4):
            for mp in (1, 3):
                exp = model([e], conn, mp)
                cap = len(exp[0][1]) + 2
                out = Out(A, 1, H, W + 3, cap)
                out.call(plan, ptr(d_e), conn, mp)
                A.check("%s %d %d" % (name, conn, mp))
                assert_result(out, W, exp, "%s %d %d" % (name, conn, mp))
                del out
        n8, n4 = len(components(e, 8)[1]), len(components(e, 4)[1])
        if name == "all_foreground_4k":
            assert n8 == n4 == 1 and int(components(e, 4)[1]["pixels"][0]) == W * H
        if name == "isolated_4k":
            assert n8 == n4 == 2073600
        if name == "diagonals":
            assert n8 < 1000 and n4 > 100 * n8           # lines at 8, (nearly) every pixel on its own at 4
        if name in ("thin_serpentine", "spiral", "serpentine"):
            assert n8 == n4 == 1
        if name == "combs":
            assert n8 == n4 == 2
        if name == "four_borders":
            r = components(e, 8)[1][0]
            assert (r["x0"], r["y0"], r["x1"], r["y1"]) == (0, 0, W - 1, H - 1) and n4 > 1000
    finally:
        plan.close()


def _small_batch(hip_ctx):
    """A 3-frame plan whose middle frame is all zero, after Canny."""
    from compv_amd import capi
    from oracle_bindings import synth_frame
    W, H, S, F = 333, 77, 336, 3
    imgs = np.stack([synth_frame(W, H, 5), np.zeros((H, W), np.uint8), synth_frame(W, H, 77)])
    rng = np.random.default_rng(1)
    A = Arena()
    host_in = pad_frames(imgs, S, rng)
    d_in = A.new(F * H * S, host_in)
    d_e = A.new(F * H * S)
    plan = capi.Plan(hip_ctx, W, H, S, F, 1.0)
    plan.canny(ptr(d_in), T_LOW, T_HIGH, ptr(d_e))
    A.check("setup")
    edges = frames_view(d_e, F, H, S, W).copy()
    return dict(W=W, H=H, S=S, F=F, A=A, plan=plan, d_in=d_in, d_e=d_e, edges=edges)


def test_capacity_counts_only_and_replay(hip_ctx):
    """compCap below the count: counts unclipped, the records are the prefix, the slots behind untouched, the label map unchanged; a call
    without records and without labels only counts; calling twice gives identical bytes."""
    k = _small_batch(hip_ctx)
    A, plan, F, W, H = k["A"], k["plan"], k["F"], k["W"], k["H"]
    try:
        exp = model(k["edges"], 8, 2)
        assert len(exp[1][1]) == 0 and min(len(exp[0][1]), len(exp[2][1])) > 1 and max(len(exp[0][1]), len(exp[2][1])) > 7      # caps 7 and 1 clip
        big = max(len(x[1]) for x in exp) + 5
        labels = None
        for cap in (big, 7, 1):
            out = Out(A, F, H, W + 1, cap)
            out.call(plan, 0, 8, 2)
            A.check("compCap %d" % cap)
            assert_result(out, W, exp, "compCap %d" % cap)
            raw = out.raw()
            labels = labels or raw[0]
            assert raw[0] == labels                                         # the label map does not depend on compCap
            out.refill()
            out.call(plan, ptr(k["d_e"]), 8, 2)
            A.check("replay %d" % cap)
            assert out.raw() == raw                                         # again, from bytes: identical buffers
        for labels_wanted in (False, True):
            out = Out(A, F, H, W, 0, labels=labels_wanted)
            out.call(plan, 0, 8, 2)
            A.check("counts only")
            assert_result(out, W, exp, "counts only")
    finally:
        plan.close()


def test_refusals(hip_ctx):
    from compv_amd import capi
    k = _small_batch(hip_ctx)
    A, plan, F, W, H, S = k["A"], k["plan"], k["F"], k["W"], k["H"], k["S"]
    out = Out(A, F, H, W, 64)

    def refused(code, pl, de, conn=8, mp=1, ls=W):
        out.ls = ls
        with pytest.raises(capi.CompvHipError) as err:
            out.call(pl, de, conn, mp)
        out.ls = W
        assert err.value.code == code, err.value
        A.check("refused call")
        assert all((b.cpu().numpy() == SENTINEL).all() for b in (out.d_labels, out.d_comps, out.d_cc))      # a refused call writes nothing

    fresh = capi.Plan(hip_ctx, W, H, S, F, 1.0)
    try:
        for conn in (0, 6, 9, -8):
            refused(capi.E_INVALID_PARAMETER, plan, 0, conn=conn)
        refused(capi.E_INVALID_PARAMETER, plan, 0, mp=0)
        refused(capi.E_INVALID_PARAMETER, plan, 0, mp=-3)
        refused(capi.E_INVALID_PARAMETER, plan, 0, ls=W - 1)
        refused(capi.E_INVALID_PARAMETER, fresh, 0)                     # no Canny ran on this plan: it has no masks
        exp = model(k["edges"], 8, 1)
        out.call(fresh, ptr(k["d_e"]), 8, 1)                            # ... but it serves explicit edge maps
        A.check("fresh plan, explicit edges")
        assert_result(out, W, exp, "fresh plan")
        out.refill()
        # an asynchronous step in flight: refused until it was waited for
        d_e2 = A.new(F * H * S)
        d_lines = A.new(F * 64 * 20)
        d_counts = A.new(F * 4)
        t = plan.pipeline_async(ptr(k["d_in"]), T_LOW, T_HIGH, 20, 0, ptr(d_e2), ptr(d_lines), 64, ptr(d_counts))
        refused(capi.E_INVALID_STATE, plan, 0)
        plan.wait(t)
        out.call(plan, 0, 8, 1)                                         # same frames, same thresholds: the same masks as before
        A.check("after wait")
        assert_result(out, W, exp, "after wait")
    finally:
        fresh.close()
        plan.close()

    # host entry point
    L = hip_ctx.lib
    e0 = np.ascontiguousarray(k["edges"][0])
    lab_full, full = hip_ctx.components(e0, 8, 1)
    assert len(full) > 4 and full.tobytes() == exp[0][1].tobytes()
    comps = np.zeros(4, COMP_DTYPE)
    lab = np.full((H, W + 2), -7, np.int32)
    n = C.c_size_t(0)

    def host(conn=8, mp=1, cap=4, ls=W + 2, labels=True, cp=True):
        return L.compvhip_components_u8(hip_ctx.h, e0.ctypes.data, W, H, W, conn, mp, lab.ctypes.data if labels else None, ls,
                                        comps.ctypes.data if cp else None, cap, C.byref(n))
    assert host() == capi.E_OUT_OF_BOUND and n.value == len(full)
    assert comps.tobytes() == full[:4].tobytes()                        # the first cap records were written
    assert np.array_equal(lab[:, :W], lab_full) and (lab[:, W:] == -7).all()      # the label map is complete, its padding untouched
    assert host(cap=0, cp=False, labels=False) == capi.E_OUT_OF_BOUND and n.value == len(full)
    assert host(conn=5) == capi.E_INVALID_PARAMETER
    assert host(mp=0) == capi.E_INVALID_PARAMETER
    assert host(ls=W - 1) == capi.E_INVALID_PARAMETER
    z = np.zeros((H, W), np.uint8)
    assert L.compvhip_components_u8(hip_ctx.h, z.ctypes.data, W, H, W, 8, 1, None, 0, None, 0, C.byref(n)) == capi.OK and n.value == 0


def test_allocations_go_with_plan_and_context():
    from compv_amd import capi
    ctx = capi.Context(0)
    try:
        live0 = ctx.live_allocations()
        k = _small_batch(ctx)
        A, plan, F, W, H = k["A"], k["plan"], k["F"], k["W"], k["H"]
        try:
            live1 = ctx.live_allocations()
            Out(A, F, H, W, 16).call(plan, 0, 8, 1)                      # label map given: no parent scratch
            live2 = ctx.live_allocations()
            Out(A, F, H, W, 16, labels=False).call(plan, ptr(k["d_e"]), 4, 1)   # bytes, no label map: the mask copy and the parent scratch
            live3 = ctx.live_allocations()
            Out(A, F, H, W, 16, labels=False).call(plan, ptr(k["d_e"]), 4, 1)
            A.check("components")
            assert live1 < live2 < live3 == ctx.live_allocations() and live2 - live1 == 1 and live3 - live2 == 2
        finally:
            plan.close()
        assert ctx.live_allocations() == live0                           # every plan buffer, the component scratch included
        e0 = np.ascontiguousarray(k["edges"][0])
        a = ctx.components(e0, 8, 1)
        live4 = ctx.live_allocations()
        b = ctx.components(e0, 8, 1)
        assert a[1].tobytes() == b[1].tobytes() and np.array_equal(a[0], b[0]) and len(a[1]) > 0
        assert ctx.live_allocations() == live4                           # the staging buffers are reused, not re-allocated
    finally:
        ctx.close()
    assert ctx.h is None


def test_components_of_a_32_x_4k_step(hip_ctx):
    """One 32 x 4K pipeline step on the benchmark's frames, then the components of the step's own masks: all 32 frames against the model, and
    frame f's result equals the single-frame result of the same map."""
    import torch
    from compv_amd import capi
    from oracle_bindings import synth_frame
    W, H, F, thr = 3840, 2160, 32, 100
    dev = torch.device("cuda:0")
    d_in = torch.empty((F, H, W), dtype=torch.uint8, device=dev)
    for f in range(F):
        d_in[f] = torch.from_numpy(synth_frame(W, H, 12345 + f))         # the benchmark's first batch (tools/components_bench.py)
    line_cap = 1 << 16
    d_e = torch.empty_like(d_in)
    d_lines = torch.zeros(F * line_cap * 20, dtype=torch.uint8, device=dev)
    d_counts = torch.zeros(F, dtype=torch.int32, device=dev)
    plan = capi.Plan(hip_ctx, W, H, W, F, 1.0)
    one = capi.Plan(hip_ctx, W, H, W, 1, 1.0)
    A = Arena()
    try:
        plan.pipeline(ptr(d_in), T_LOW, T_HIGH, thr, 0, ptr(d_e), ptr(d_lines), line_cap, ptr(d_counts))
        torch.cuda.synchronize()
        edges = d_e.cpu().numpy()
        for conn, mp in ((8, 1), (8, 10), (4, 1)):
            exp = model(edges, conn, mp)
            cap = max(len(x[1]) for x in exp) + 1
            out = Out(A, F, H, W, cap)
            out.call(plan, 0, conn, mp)
            A.check("4K batch %d %d" % (conn, mp))
            assert_result(out, W, exp, "4K batch %d %d" % (conn, mp))
            if (conn, mp) == (8, 1):
                n, share = summary(exp[0][1], int((edges[0] != 0).sum()))
                assert n > 100 and 0.0 < share <= 1.0
                single = Out(A, 1, H, W, cap)
                lab = out.d_labels.cpu().numpy().reshape(F, -1)
                rec = out.d_comps.cpu().numpy().reshape(F, -1)
                cc = out.d_cc.cpu().numpy().view(np.int32)
                for f in range(F):
                    single.refill()
                    single.call(one, ptr(d_e[f]), conn, mp)
                    A.check("single frame %d" % f)
                    s = single.raw()
                    assert s[0] == lab[f].tobytes() and s[1] == rec[f].tobytes() and np.frombuffer(s[2], np.int32)[0] == cc[f], f
                del single
            del out
            A.bufs.clear()
    finally:
        one.close()
        plan.close()
