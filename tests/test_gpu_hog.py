"""GPU HOG descriptors (compvhip_plan_hog, compvhip_hog_u8) against tests/hog_model.py on every frame and against the fixtures of
tests/golden/golden_hog.* on frame 0, by bit pattern: nothing here is compared with a tolerance.

Harness of tests/gpu_support.py: every device buffer sits between two guards; the descriptors and the cell map start filled with a sentinel, so
every float the definition defines must be written and the floats behind descLen must keep it; the frames' padding columns [W, S) hold seeded random bytes
and the frames must come back unchanged.  Every call is made twice and must repeat itself byte for byte.  Three frames per case, S > W.

A wave of the cells kernel takes nx = min(64, cellsX) adjacent cells of ny = 64 / nx cell rows and stages at most 16 KB of rows; the blocks kernel gives a
block four lanes, 64 blocks to a workgroup.  Shapes are chosen from those numbers: 65 cells across (521 x 19) and 65 cell rows (19 x 521) are one past a
wave's tile in each direction; 40 rows of 96 x 4 cells halve ny (32 lane rows of three staged rows exceed 16 KB) and are staged three rows at a time; two
2740 x 4 cells halve ny, then nx."""
import ctypes as C

import numpy as np
import pytest

import hog_cases as hc
import hog_model as hm
from fixtures import load_golden
from gpu_support import SENTINEL, Arena, ptr
from hog_rig import Rig, bits

pytestmark = pytest.mark.gpu

OTHER = {"noise": ("blocks", 2), "blocks": ("noise", 3), "checkerboard": ("checkerboard", 1), "constant": ("constant", 1)}          # frame 1 of a case, by its kind


@pytest.fixture(scope="module")
def golden_hog():
    meta, arrays = load_golden("golden_hog")
    return {c["id"]: c for c in meta["cases"]}, arrays


def frames_of(c):
    """the golden frame, a frame of another kind, one more noise frame"""
    kind, seed = OTHER[c["kind"]]
    return [hc.case_frame(c), hc.frame(kind, c["W"], c["H"], seed), hc.noise(c["W"], c["H"], 7)]


def model(frames, opts):
    return [hm.hog(f, opts) for f in frames]


@pytest.mark.parametrize("cid", [c["id"] for c in hc.CASES])
def test_cases_against_model_and_golden(hip_ctx, golden_hog, cid):
    """every case of the fixture list: interpolations, norms at counts 9, 15, 36, 6, layouts, 360 and 2 bins, the constant frame (all-zero output), the
    checkerboard, left-out cells, a wave's tile + 1 in both directions, a 64 x 64 cell"""
    by_id, arrays = golden_hog
    c = hc.BY_ID[cid]
    frames = frames_of(c)
    exp = model(frames, c["opts"])
    rig = Rig(hip_ctx, frames, c["opts"])
    try:
        rig.twice(cid, exp)
        desc, cells = rig.outputs(cid)
        if by_id[cid]["stored"]:
            assert desc[0, :rig.desc_len].tobytes() == arrays["desc_" + cid].tobytes()          # frame 0 against the reference's own bytes
        g = rig.g
        if g["validX"] < g["cellsX"] or g["validY"] < g["cellsY"]:          # the left-out cells hold 0
            m = cells.reshape(rig.F, g["cellsY"], g["cellsX"], -1)
            assert not m[:, g["validY"]:].any() and not m[:, :, g["validX"]:].any()
        if c["kind"] == "constant":
            assert not desc[0, :rig.desc_len].any() and not cells[0].any()
    finally:
        rig.close()


@pytest.mark.parametrize("misalign", [1, 2, 3])
def test_frames_that_are_not_dword_aligned(hip_ctx, misalign):
    """the byte-load arm of the staging: same results from frames that start 1, 2, 3 bytes off a dword"""
    for cid in ("b16s8c8_noise37x29", "b12s6c6_noise37x29", "nearest_u_blocks37x29"):
        c = hc.BY_ID[cid]
        frames = frames_of(c)
        rig = Rig(hip_ctx, frames, c["opts"], misalign=misalign)
        try:
            rig.twice("%s at +%d" % (cid, misalign), model(frames, c["opts"]))
        finally:
            rig.close()


@pytest.mark.parametrize("W,H,o", [
    (200, 162, hc.layout((96, 4), (96, 4), (96, 4), norm=hm.NORM_L1)),   # 2 x 40 cells: nx = 2, ny = 32 halves to 16 (3 tiles down); 5 staged rows: 3 cell rows, then 1
    (5500, 8, hc.layout((2740, 4), (2740, 4), (2740, 4), norm=hm.NORM_L2)),   # 2 x 2 cells of 2740 x 4: ny halves to 1, then nx to 1; again 3 rows, then 1
    (130, 70, hc.layout((64, 32), (32, 32), (64, 32), 4)),               # stride = cell / 2 in x only, 64-wide cells
    (96, 40, hc.layout((32, 16), (16, 8), (32, 16), 12, norm=hm.NORM_L1SQRT)),  # stride = cell / 2 on a rectangular cell, 12 bins
])
def test_launch_geometry_arms(hip_ctx, W, H, o):
    assert hm.geometry(W, H, o) is not None
    frames = [hc.noise(W, H, 4), hc.blocks(W, H, 5), hc.noise(W, H, 6)]
    rig = Rig(hip_ctx, frames, o)
    try:
        rig.twice("%dx%d" % (W, H), model(frames, o))
    finally:
        rig.close()


def test_without_a_map_on_a_stream_with_timing(hip_ctx):
    """d_cells == NULL: the plan's own map (allocated on first use, once); a non-default stream; the timing entries; other options on the same plan"""
    import torch
    from compv_amd import capi
    c = hc.BY_ID["b16s8c8_noise37x29"]
    frames = frames_of(c)
    rig = Rig(hip_ctx, frames, c["opts"], desc_pad=0)          # descStride == descLen
    try:
        start = hip_ctx.live_allocations()
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        rig.plan.set_timing(1)
        rig.run(cells=False, stream=st.cuda_stream)
        st.synchronize()
        t = rig.plan.get_timing()
        assert [n for n, _ in t] == ["hog_cells_kernel", "hog_blocks_kernel"] and all(ms >= 0 for _, ms in t)
        rig.plan.set_timing(0)
        first = rig.check("no map, stream", model(frames, c["opts"]), cells=False)
        assert hip_ctx.live_allocations() == start + 1
        rig.run(cells=False, stream=st.cuda_stream)
        st.synchronize()
        assert rig.check("no map, stream (again)", model(frames, c["opts"]), cells=False) == first
        assert hip_ctx.live_allocations() == start + 1          # no call allocates again
        rig.run(cells=True)
        assert rig.check("with a map", model(frames, c["opts"])) == first
        o2 = hc.layout(16, 8, 8, norm=hm.NORM_L1, signed=False, interp=hm.INTERP_NEAREST)          # the same sizes, so the rig's buffers fit
        rig.run(cells=False, opts=capi.HogOpts(**o2))
        assert rig.check("other options on the same plan", model(frames, o2), cells=False) != first
        assert hip_ctx.live_allocations() == start + 1
    finally:
        rig.close()


def test_refusals_write_nothing(hip_ctx):
    from compv_amd import capi
    c = hc.BY_ID["b16s8c8_noise37x29"]
    frames = frames_of(c)
    rig = Rig(hip_ctx, frames, c["opts"])
    lib = hip_ctx.lib

    def code(**kw):
        try:
            rig.run(**kw)
        except capi.CompvHipError as e:
            return e.code
        return capi.OK

    def untouched(what):
        rig.ar.check(what)
        assert (rig.d_desc.cpu().numpy() == SENTINEL).all() and (rig.d_cells.cpu().numpy() == SENTINEL).all(), what

    try:
        start = hip_ctx.live_allocations()
        bad = [capi.HogOpts(block=16, stride=8, cell=6), capi.HogOpts(block=16, stride=4, cell=8), capi.HogOpts(nbins=7), capi.HogOpts(nbins=361), capi.HogOpts(nbins=1),
               capi.HogOpts(nbins=8, signed=False), capi.HogOpts(interp="bilinear_lut"), capi.HogOpts(interp=9), capi.HogOpts(norm=6), capi.HogOpts(block=64),
               capi.HogOpts(block=(16, 32)), capi.HogOpts(gradientSigned=3), capi.HogOpts(cellW=-8)]
        for o in bad:
            assert code(opts=o, cells=False) == capi.E_INVALID_PARAMETER, [getattr(o, f) for f in hm.FIELDS]
            assert hip_ctx.last_error().startswith("HOG")
        wrong_size = capi.HogOpts()
        wrong_size.size = 48
        assert code(opts=wrong_size) == capi.E_INVALID_PARAMETER
        assert code(stride=rig.desc_len - 1) == capi.E_INVALID_PARAMETER          # descStride below descLen
        untouched("refused options")
        o = C.byref(rig.o)
        assert lib.compvhip_plan_hog(rig.plan.h, None, o, None, ptr(rig.d_desc), rig.stride, None) == capi.E_INVALID_PARAMETER          # null frames
        assert lib.compvhip_plan_hog(rig.plan.h, rig.gray_ptr, o, None, None, rig.stride, None) == capi.E_INVALID_PARAMETER              # null descriptors
        assert lib.compvhip_plan_hog(rig.plan.h, rig.gray_ptr, None, None, ptr(rig.d_desc), rig.stride, None) == capi.E_INVALID_PARAMETER   # null options
        assert lib.compvhip_plan_hog(rig.plan.h, rig.gray_ptr, o, None, ptr(rig.d_desc) + 2, rig.stride, None) == capi.E_INVALID_PARAMETER   # misaligned descriptors
        assert lib.compvhip_plan_hog(rig.plan.h, rig.gray_ptr, o, ptr(rig.d_cells) + 1, ptr(rig.d_desc), rig.stride, None) == capi.E_INVALID_PARAMETER
        untouched("refused pointers")
        assert hip_ctx.live_allocations() == start          # a refusal allocates nothing
        rig.twice("after the refusals", model(frames, c["opts"]))
    finally:
        rig.close()


def test_host_form(hip_ctx, golden_hog):
    from compv_amd import capi
    by_id, arrays = golden_hog
    for cid in ("b16s8c8_noise37x29", "rect6u_noise37x29", "norm_l1sqrt_c15_noise37x29", "b8s4c8_noise64x48", "n360_noise16x16", "b8c8_noise8x8"):
        c = hc.BY_ID[cid]
        img = hc.case_frame(c)
        for _ in range(2):
            got = hip_ctx.hog(img, capi.HogOpts(**c["opts"]))
            assert got.dtype == np.float32 and got.tobytes() == arrays["desc_" + cid].tobytes() == hm.hog(img, c["opts"])[0].tobytes(), cid
    img = hc.noise(70, 50, 9)
    wide = np.zeros((50, 90), np.uint8)          # a host stride beyond W
    wide[:, :70] = img
    assert hip_ctx.hog(wide[:, :70]).tobytes() == hm.hog(img)[0].tobytes()          # keywords: none, the defaults
    assert hip_ctx.hog(img, block=8, stride=4, cell=8, nbins=18, norm="l1", signed=True, interp="nearest").tobytes() == \
        hm.hog(img, hc.layout(8, 4, 8, 18, norm=hm.NORM_L1, interp=hm.INTERP_NEAREST))[0].tobytes()
    # cap too small: COMPVHIP_E_OUT_OF_BOUND, *n = descLen, nothing written
    o = capi.HogOpts()
    need = hm.geometry(70, 50)["descLen"]
    buf = np.full(need, 5.0, np.float32)
    n = C.c_size_t(0)
    assert hip_ctx.lib.compvhip_hog_u8(hip_ctx.h, img.ctypes.data, 70, 50, 70, C.byref(o), buf.ctypes.data, need - 1, C.byref(n)) == capi.E_OUT_OF_BOUND
    assert n.value == need and (buf == 5.0).all()
    assert hip_ctx.lib.compvhip_hog_u8(hip_ctx.h, img.ctypes.data, 70, 50, 70, C.byref(o), None, 0, C.byref(n)) == capi.E_OUT_OF_BOUND and n.value == need
    n = C.c_size_t(777)
    assert hip_ctx.lib.compvhip_hog_u8(hip_ctx.h, img.ctypes.data, 70, 50, 70, C.byref(capi.HogOpts(nbins=7)), buf.ctypes.data, need, C.byref(n)) == capi.E_INVALID_PARAMETER
    assert hip_ctx.lib.compvhip_hog_u8(hip_ctx.h, None, 70, 50, 70, C.byref(o), buf.ctypes.data, need, C.byref(n)) == capi.E_INVALID_PARAMETER
    assert hip_ctx.lib.compvhip_hog_u8(hip_ctx.h, img.ctypes.data, 70, 50, 69, C.byref(o), buf.ctypes.data, need, C.byref(n)) == capi.E_INVALID_PARAMETER
    assert n.value == 777 and (buf == 5.0).all()
    assert hip_ctx.lib.compvhip_hog_u8(hip_ctx.h, img.ctypes.data, 70, 50, 70, C.byref(o), buf.ctypes.data, need, C.byref(n)) == capi.OK and n.value == need
    assert buf.tobytes() == hm.hog(img)[0].tobytes()


def test_a_batch_beyond_65535_frames_is_sliced(hip_ctx):
    """65 537 crops of 8 x 8, block = cell = 8: one 9-float block each.  The frames repeat four patterns, so EVERY frame is compared, the last of the first
    slice (65 534), the first of the second (65 535) and the one beyond (65 536) by name"""
    from compv_amd import capi
    F, W, H, S = 65537, 8, 8, 16
    o = hc.layout(8, 8, 8)
    pats = [hc.noise(W, H, 11), hc.blocks(W, H, 12), hc.checkerboard(W, H, 0), hc.noise(W, H, 13)]
    exp = [hm.hog(p, o) for p in pats]
    host = np.empty((F, H, S), np.uint8)
    host[:] = 0x5A
    for k in range(4):
        host[k::4, :, :W] = pats[k]
    ar = Arena()
    d_gray = ar.new(host.size, host.reshape(-1))
    d_desc = ar.new(F * 9 * 4)
    d_cells = ar.new(F * 9 * 4)
    plan = capi.Plan(hip_ctx, W, H, S, F)
    try:
        for rep in range(2):
            ar.refill(d_desc)
            ar.refill(d_cells)
            plan.hog(ptr(d_gray), ptr(d_desc), 9, ptr(d_cells), opts=capi.HogOpts(**o))
            ar.check("65537 frames")
            desc = d_desc.cpu().numpy().view(np.uint32).reshape(F, 9)
            cells = d_cells.cpu().numpy().view(np.uint32).reshape(F, 9)
            for k in range(4):
                assert (desc[k::4] == bits(exp[k][0])[None, :]).all(), "pattern %d" % k
                assert (cells[k::4] == bits(exp[k][1]).reshape(-1)[None, :]).all(), "pattern %d, map" % k
            for f in (0, 65534, 65535, 65536):
                assert desc[f].tobytes() == exp[f % 4][0].tobytes(), f
        assert (d_gray.cpu().numpy() == host.reshape(-1)).all()
    finally:
        plan.close()
