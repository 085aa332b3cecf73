"""GPU tests of the canonical KHT order (compvhip_plan_houghkht_ex / compvhip_houghkht_ex_u8 with COMPVHIP_KHT_ORDER_CANONICAL): every field of every
line, bit for bit and in order, against the CPU model of tests/kht_canon_model.py, and the coexistence of both orders on one plan."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from kht_canon_model import CanonModel, emission, has_tie_neighbour, line_bits, model_line_bits
from oracle_bindings import md5_rows, synth_frame

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LDS_SORT_LINES = 2048      # kKhtCanonSortLds (compv_amd/csrc/kht.hpp): beyond, kht_canon_sort_kernel merges in global memory


@pytest.fixture(scope="module")
def model(oracle):
    return CanonModel(oracle)


def _list_hash(l):
    h = 0
    for r, t, sv in zip(l["rho"].astype(np.float32).view(np.uint32).tolist(), l["theta"].astype(np.float32).view(np.uint32).tolist(), l["strength"].astype(np.int64).tolist()):
        h = (h * 1000003 + r * 7919 + t * 31337 + sv) & ((1 << 64) - 1)
    return h


def _plan_edges(hip_ctx, frames, tl, th):
    """(plan, device edge maps, host copy) for a stack of frames: the plan's Canny makes the edge maps"""
    import torch
    from compv_amd import capi
    F, H, W = frames.shape
    d_in = torch.from_numpy(np.ascontiguousarray(frames)).to(torch.device("cuda:0"))
    d_e = torch.empty_like(d_in)
    plan = capi.Plan(hip_ctx, W, H, W, F, 1.0)
    plan.canny(d_in.data_ptr(), tl, th, d_e.data_ptr())
    torch.cuda.synchronize()
    return plan, d_e, d_e.cpu().numpy()


def _check_against_model(model, lines, gs, edges, **kw):
    exp, egs, rec = model.lines(edges, **kw)
    assert line_bits(lines) == model_line_bits(exp)
    assert gs == egs
    return exp, rec


@pytest.mark.parametrize("F", [9, 32])
def test_canonical_uhd_batch_against_the_model(hip_ctx, model, F):
    """The benchmark's 4K frames (tests/golden/golden_batch_kht.json): every line of every frame, in order, bit for bit against the model; the reference
    order still matches the fixture on the same plan afterwards; at least one frame's canonical list differs from its reference list (ties are exercised)."""
    gk = json.load(open(os.path.join(GOLDEN, "golden_batch_kht.json")))
    frames = np.stack([synth_frame(gk["W"], gk["H"], gk["first_seed"] + f) for f in range(F)])
    plan, d_e, e = _plan_edges(hip_ctx, frames, gk["tLow"], gk["tHigh"])
    try:
        canon, cgs = plan.houghkht(d_e.data_ptr(), gk["rho"], gk["theta_deg"], gk["threshold"], order="canonical")
        st = plan.houghkht_stage_ms()
        assert st["stages"]["sort_sweep"] == 0 and st["stages"]["vote_peaks"] > 0
        ref, rgs = plan.houghkht(d_e.data_ptr(), gk["rho"], gk["theta_deg"], gk["threshold"])
        differs = 0
        for f in range(F):
            g = gk["frames"][f]
            assert md5_rows(e[f]) == g["canny_md5"]
            _check_against_model(model, canon[f], cgs[f], e[f], threshold=gk["threshold"])
            l = ref[f]
            assert (len(l), int(l["strength"].astype(np.int64).sum()), repr(rgs[f]), "%016x" % _list_hash(l)) == \
                (g["lines"], g["sum_strength"], g["gs"], g["list_hash"]), f
            assert cgs[f] == rgs[f]
            differs += line_bits(canon[f]) != line_bits(ref[f])
        assert differs > 0
    finally:
        plan.close()


def test_canonical_host_entry_point_against_the_model(hip_ctx, oracle, model):
    """compvhip_houghkht_ex_u8 on single frames: a 4K benchmark frame, a rhoN % 4 == 3 geometry with records of the scalar remainder (Q6), a maxLines cut
    inside a tie group, a threshold that leaves no record, and a 3 x 2 frame (rhoN <= 4: the non-SIMD scan -- with rho <= 1 so small a frame has no seed,
    so no record)."""
    from compv_amd import capi
    gk = json.load(open(os.path.join(GOLDEN, "golden_batch_kht.json")))
    rc, e = oracle.canny(synth_frame(gk["W"], gk["H"], gk["first_seed"] + 1), gk["tLow"], gk["tHigh"])
    lines, gs = hip_ctx.houghkht(e, 1.0, 1.0, 1, order="canonical")
    exp, rec = _check_against_model(model, lines, gs, e)
    assert hip_ctx.houghkht_stage_ms()[5] == 0
    # maxLines inside a tie group
    cut = next(i for i in range(1, len(exp)) if exp[i - 1][2] == exp[i][2])
    top, _ = hip_ctx.houghkht(e, 1.0, 1.0, 1, max_lines=cut, order="canonical")
    assert line_bits(top) == model_line_bits(exp[:cut]) and len(top) == cut
    # no record at all; GS is still reported (kernels survived)
    none, gsn = hip_ctx.houghkht(e, 1.0, 1.0, 1 << 30, order="canonical")
    assert len(none) == 0 and gsn == gs
    # Q6 geometry
    rc, q = oracle.canny(synth_frame(1282, 720, 7), 0.8, 1.6)
    ax = model.axes(1282, 720)
    assert ax.rhoN % 4 == 3
    lq, gq = hip_ctx.houghkht(q, 1.0, 1.0, 1, order="canonical")
    _, recq = _check_against_model(model, lq, gq, q)
    assert int(((recq[:, 3] - recq[:, 1] * 2 * (ax.rhoN + 2)) >= ax.rhoN + 2).sum()) >= 1
    # rhoN <= 4
    tiny = np.full((2, 3), 255, np.uint8)
    assert model.axes(3, 2).rhoN <= 4
    lt, _ = hip_ctx.houghkht(tiny, 1.0, 1.0, 1, order="canonical")
    assert len(lt) == 0 and len(model.lines(tiny)[0]) == 0
    # unknown order / NULL options through the C ABI
    n = C.c_size_t(0)
    opts = capi.KhtOpts(); opts.order = 7
    assert hip_ctx.lib.compvhip_houghkht_ex_u8(hip_ctx.h, e.ctypes.data_as(C.c_void_p), e.shape[1], e.shape[0], e.shape[1], C.byref(opts), None, 0,
                                               C.byref(n), None) == capi.E_INVALID_PARAMETER
    assert hip_ctx.lib.compvhip_houghkht_ex_u8(hip_ctx.h, e.ctypes.data_as(C.c_void_p), e.shape[1], e.shape[0], e.shape[1], None, None, 0,
                                               C.byref(n), None) == capi.E_INVALID_PARAMETER


def test_canonical_batch_of_13_with_a_blank_frame(hip_ctx, model):
    """13 frames (not a multiple of the group of 8), a blank frame in the middle, and a maxLines cut inside a tie group."""
    F = 13
    frames = np.stack([synth_frame(640, 480, 4000 + f) for f in range(F)])
    frames[6] = 31
    plan, d_e, e = _plan_edges(hip_ctx, frames, 59.0, 119.0)
    try:
        lines, gs = plan.houghkht(d_e.data_ptr(), 1.0, 1.0, 1, order="canonical")
        exps = []
        for f in range(F):
            exp, _ = _check_against_model(model, lines[f], gs[f], e[f])
            exps.append(exp)
        assert len(lines[6]) == 0 and gs[6] is None
        cut = next(i for i in range(1, len(exps[0])) if exps[0][i - 1][2] == exps[0][i][2])
        top, _ = plan.houghkht(d_e.data_ptr(), 1.0, 1.0, 1, max_lines=cut, order="canonical")
        for f in range(F):
            assert line_bits(top[f]) == model_line_bits(exps[f][:cut]), f
    finally:
        plan.close()


def test_canonical_beyond_the_lds_sort(hip_ctx, oracle, model):
    """Dense edge maps with more lines than kht_canon_sort_kernel sorts in LDS: the global-memory merge path, through both entry points."""
    frames = np.stack([synth_frame(1920, 1080, 5), synth_frame(1920, 1080, 6)])
    plan, d_e, e = _plan_edges(hip_ctx, frames, 0.8, 1.6)
    try:
        lines, gs = plan.houghkht(d_e.data_ptr(), 1.0, 1.0, 1, order="canonical", cap=1 << 15)
        for f in range(2):
            exp, _ = _check_against_model(model, lines[f], gs[f], e[f])
            assert len(exp) > LDS_SORT_LINES
        one, g1 = hip_ctx.houghkht(e[0], 1.0, 1.0, 1, order="canonical")
        assert line_bits(one) == line_bits(lines[0]) and g1 == gs[0]
    finally:
        plan.close()
    big = synth_frame(3840, 2160, 3)
    rc, eb = oracle.canny(big, 0.8, 1.6)
    lb, gb = hip_ctx.houghkht(eb, 1.0, 1.0, 1, order="canonical")
    exp, _ = _check_against_model(model, lb, gb, eb)
    assert len(exp) > 2 * LDS_SORT_LINES                                               # more than one merge pass


def test_both_orders_coexist_on_one_plan(hip_ctx, model):
    """Lines whose position has no equal-count record among its 8 neighbours are the same in both orders; GS is the same; the pool size does not change
    the canonical output; too small a cap is E_OUT_OF_BOUND with the needed count; unknown orders are refused; every allocation of the plan goes with it."""
    from compv_amd import capi
    gk = json.load(open(os.path.join(GOLDEN, "golden_batch_kht.json")))
    F = 3
    live0 = hip_ctx.live_allocations()
    frames = np.stack([synth_frame(gk["W"], gk["H"], gk["first_seed"] + f) for f in range(F)])
    plan, d_e, e = _plan_edges(hip_ctx, frames, gk["tLow"], gk["tHigh"])
    try:
        canon, cgs = plan.houghkht(d_e.data_ptr(), 1.0, 1.0, 1, order="canonical", threads=3)
        canon1, cgs1 = plan.houghkht(d_e.data_ptr(), 1.0, 1.0, 1, order="canonical", threads=1)
        ref, rgs = plan.houghkht(d_e.data_ptr(), 1.0, 1.0, 1)
        assert cgs == cgs1 == rgs
        for f in range(F):
            assert line_bits(canon[f]) == line_bits(canon1[f])
            ax, counts, _ = model.vote_map(e[f])
            rec = emission(ax, counts, 1)
            tie = {}
            for (r, t, s, _), flag in zip(rec.tolist(), has_tie_neighbour(rec, ax.rhoN, ax.T).tolist()):
                tie[(r, t, s)] = tie.get((r, t, s), False) or flag
            clear = lambda ls: {x for x in line_bits(ls) if not tie[(x[3], x[4], x[2])]}
            assert clear(canon[f]) == clear(ref[f]) and len(clear(canon[f])) > 0
        # capacity contract
        need = [len(l) for l in canon]
        opts = capi.KhtOpts(); opts.order = capi.KHT_ORDER_CANONICAL
        cap = min(need) - 1
        buf = np.zeros((F, cap), capi.LINE_DTYPE)
        counts = np.zeros(F, np.uint64)
        rc = hip_ctx.lib.compvhip_plan_houghkht_ex(plan.h, d_e.data_ptr(), C.byref(opts), buf.ctypes.data_as(C.c_void_p), cap,
                                                   counts.ctypes.data_as(C.c_void_p), None)
        assert rc == capi.E_OUT_OF_BOUND and counts.tolist() == need
        for f in range(F):
            assert line_bits(buf[f]) == line_bits(canon[f][:cap])
        assert hip_ctx.lib.compvhip_plan_houghkht_ex(plan.h, d_e.data_ptr(), None, buf.ctypes.data_as(C.c_void_p), cap,
                                                     counts.ctypes.data_as(C.c_void_p), None) == capi.E_INVALID_PARAMETER
        opts.order = 2
        assert hip_ctx.lib.compvhip_plan_houghkht_ex(plan.h, d_e.data_ptr(), C.byref(opts), buf.ctypes.data_as(C.c_void_p), cap,
                                                     counts.ctypes.data_as(C.c_void_p), None) == capi.E_INVALID_PARAMETER
        # the reference order after canonical calls: still the fixture
        for f in range(F):
            g = gk["frames"][f]
            l = ref[f]
            assert (len(l), int(l["strength"].astype(np.int64).sum()), repr(rgs[f]), "%016x" % _list_hash(l)) == \
                (g["lines"], g["sum_strength"], g["gs"], g["list_hash"]), f
    finally:
        plan.close()
    assert hip_ctx.live_allocations() == live0
