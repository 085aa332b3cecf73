"""GPU RANSAC line and parabola fits (compvhip_curvefit_*) against tests/curvefit_model.py and the fixture tests/golden/golden_curvefit.*, bit for bit:
nothing here is compared with a tolerance.

Harness of tests/gpu_support.py: every device buffer sits between two guards; outputs start filled with a sentinel that must survive in
every slot the definition leaves unwritten (mask bytes and distances at and behind a set's k); the inputs must come back unchanged, and the point
slots behind a set's count hold seeded junk that is never read.  Every call is made twice on the same handle.

The score kernel gives one workgroup 256 tries and stages 256 points per round, the refit kernel folds 64 partials, the gather scans 256 pixels per
round.  Shapes are chosen from those numbers: k m - 1, m, m + 1, 63, 64, 65, 255, 256, 257, 600; tries 1, 255, 256, 257, maxTries."""
import numpy as np
import pytest

import curvefit_cases as cc
import curvefit_model as cm
from curvefit_rig import REC, SENT64, Rig, label_frame
from fixtures import load_golden
from gpu_support import SENTINEL, Arena, d2h, ptr, u8

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("golden_curvefit")


@pytest.mark.parametrize("model", cm.MODELS)
def test_point_counts_and_try_counts(hip_ctx, model):
    """ten sets of k = m - 1 .. 600 points (30 % outliers) in one handle; tries 1, 255, 256, 257 and maxTries; then the residuals of the planted curves"""
    ks = cc.GPU_KS[model]
    made = [cc.planted(model, k, 0.3, 20 + k) for k in ks]
    rig = Rig(hip_ctx, [p for p, _, _ in made], max(ks), 300)
    try:
        for tries in cc.TRIES + (300,):
            exp = rig.model(model, tries, seed=tries)
            res = rig.twice("model %d, %d tries" % (model, tries), model, tries, exp, seed=tries)
            assert [int(r["k"]) for r in res] == list(ks) and res[0]["status"] == 2
            if tries >= 255:          # the planted inliers, exactly
                for r, (_, inl, _) in zip(res[3:], made[3:]):
                    assert r["status"] == 0 and r["inliers"] == inl.sum()
        rig.twice("no mask", model, 64, rig.model(model, 64, seed=1), mask=False, seed=1)
        rig.check_distances("distances of model %d" % model, model, [coef for _, _, coef in made])
    finally:
        rig.close()


@pytest.mark.parametrize("model", cm.MODELS)
def test_one_three_and_seventy_sets(hip_ctx, model):
    """one set without device counts (k = pointCap = 65); three; seventy with ragged counts: 0, negative, beyond the capacity, m - 1 .. m + 1"""
    pts, _, _ = cc.noisy(model, 65, 0.3, 31)
    rig = Rig(hip_ctx, [pts], 65, 65, counts=None)
    try:
        rig.twice("one set", model, 65, rig.model(model, 65, seed=3), seed=3)
    finally:
        rig.close()
    rig = Rig(hip_ctx, [cc.noisy(model, k, 0.3, 32)[0] for k in (20, 64, 33)], 64, 70)
    try:
        rig.twice("three sets", model, 70, rig.model(model, 70, seed=4), seed=4)
    finally:
        rig.close()
    counts = cc.ragged_counts(70, 40)
    rig = Rig(hip_ctx, [cc.planted(model, 40, 0.3, 100 + s)[0] for s in range(70)], 40, 80, counts=counts.tolist())
    try:
        exp = rig.model(model, 80, seed=0xfffffff0)
        res = rig.twice("seventy sets", model, 80, exp, seed=0xfffffff0)
        assert sorted(set(res["status"].tolist())) == [0, 2] and res["k"].tolist() == np.clip(counts, 0, 40).tolist()
    finally:
        rig.close()


@pytest.mark.parametrize("model", cm.MODELS)
def test_explicit_samples_and_degenerate_sets(hip_ctx, model):
    """d_samples: two equal samples at different t, an index outside [0, k), a repeated index; sets whose every try is rejected; k == m, accepted and
    rejected; a NaN point; then a denormal threshold"""
    m = cm.model_points(model)
    base, inl, _ = cc.planted(model, 12, 0.3, 2)
    bad = base.copy()
    bad[5] = np.nan
    sets = [base, cc.all_equal(12), cc.same_abscissa(model, 12), bad, base[:m], cc.all_equal(m), base[:m - 1], base[:m + 1]]
    rig = Rig(hip_ctx, sets, 12, 8)
    try:
        q = np.array([[0, 1, 2], [3, 4, 5], [0, 1, 2], [0, 12, 1], [-1, 2, 3], [4, 4, 4]], np.int32)[:, :m]
        samples = np.stack([q if len(p) > m + 1 else np.zeros_like(q) for p in sets])
        samples[7] = np.array([[0, 1, 2], [1, 2, 3], [3, 2, 1], [0, 3, 1], [0, 4, 1], [2, 2, 2]], np.int32)[:, :m]          # k = m + 1: index 4 is outside
        exp = rig.model(model, 6, samples=samples)
        res = rig.twice("explicit samples", model, 6, exp, d_samples=rig.buffer(samples))
        assert res["status"].tolist() == [0, 1, 0 if model == cm.LINE else 1, 0, 0, 1, 2, 0]
        assert exp[0]["counts"][0] == exp[0]["counts"][2] and not exp[0]["counts"][3:].any() and res[0]["bestTry"] in (0, 1)
        exp = rig.model(model, 8, seed=9)
        res = rig.twice("generator on degenerate sets", model, 8, exp, seed=9)
        assert res[3]["status"] == 0 and exp[3]["mask"][5] == 0
        rig.twice("denormal threshold", model, 8, rig.model(model, 8, seed=9, threshold=5e-324), seed=9, threshold=5e-324)
    finally:
        rig.close()


@pytest.mark.parametrize("model", cm.MODELS)
def test_fixture_planted_cases(hip_ctx, golden, model):
    """the fixture's noise-free planted sets of one model in ONE batched call, the fixture's own samples through d_samples: records, masks and per-try
    counts as the generator stored them -- there the reference's curve selects the same inliers and lies within 1e-6 px"""
    meta, arr = golden
    cases = [c for c in meta["cases"] if c["kind"] == "planted" and c["model"] == model]
    assert len(cases) == len(cc.KS) * len(cc.SHARES)
    rig = Rig(hip_ctx, [arr["pts_" + c["id"]] for c in cases], max(cc.KS), 200)
    try:
        samples = np.stack([arr["samples_" + c["id"]].astype(np.int32) for c in cases])
        exp = [dict(result=np.frombuffer(arr["result_" + c["id"]].tobytes(), cm.RESULT_DTYPE)[0], mask=arr["mask_" + c["id"]], counts=arr["counts_" + c["id"]]) for c in cases]
        res = rig.twice("fixture, model %d" % model, model, 200, exp, d_samples=rig.buffer(samples), seed=77)
        for c, r in zip(cases, res):
            assert r["status"] == 0 and r["inliers"] == c["planted"], c["id"]
    finally:
        rig.close()


def test_failed_refit_keeps_the_best_trys_model(hip_ctx):
    """abscissas near 1e80: the moments of the refit overflow, its determinant is not finite -- status 3 with the best try's own model"""
    x = np.array([-1e80, 0.0, 1e80, 2e80, 3e80])
    pts = np.stack([x, np.zeros(5)], axis=1)
    rig = Rig(hip_ctx, [pts], 5, 4)
    try:
        q = np.array([[[0, 1, 2]]], np.int32)
        exp = rig.model(cm.PARABOLA, 1, samples=q)
        res = rig.twice("failed refit", cm.PARABOLA, 1, exp, d_samples=rig.buffer(np.concatenate([q.reshape(-1), [0]]).astype(np.int32)))
        assert res[0]["status"] == 3 and res[0]["inliers"] == 5 and res[0]["bestTry"] == 0
    finally:
        rig.close()


# ---- gather ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H,cap", [(37, 29, 16), (300, 40, 200)])
def test_gather_from_label_maps(hip_ctx, W, H, cap):
    """two frames of hand-made label maps; frame 1 reports more components than compCap (clipped) -- the gathered points and counts, then the
    residuals and the fits on them, against the model"""
    from compv_amd import capi
    stride, frames, comp_cap = W + 3, 2, 5
    n = frames * comp_cap
    rng = np.random.default_rng(W)
    lab0, comps0 = label_frame(W, H, stride, cap, rng)
    lab1, comps1 = label_frame(W, H, stride, cap, rng)
    labels = np.stack([lab0, lab1])
    comps = np.zeros((frames, comp_cap), cm.COMP_DTYPE)
    comps[0, :3], comps[1] = comps0[:3], comps1          # frame 0 has 3 records (the slots behind hold junk), frame 1 reports 7 components and has 5 records
    comps[0, 3] = comps[0, 4] = (0, 0, 0, 0, W - 1, H - 1, 99)
    counts = np.array([3, 7], np.int32)
    ar = Arena()
    d_lab, d_comps, d_counts = ar.new(labels.nbytes, u8(labels)), ar.new(comps.nbytes, u8(comps)), ar.new(8, u8(counts))
    for d, h in ((d_lab, labels), (d_comps, comps), (d_counts, counts)):
        ar.keep(d, u8(h))
    d_res, d_mask, d_dist = ar.new(n * REC), ar.new(n * cap), ar.new(n * cap * 8)
    h = capi.Curvefit(hip_ctx, n, cap, 64)
    try:
        exp_pts, exp_k = zip(*[cm.gather(labels[f], W, comps[f], counts[f], comp_cap, cap) for f in range(frames)])
        exp_pts, exp_k = np.concatenate(exp_pts), np.concatenate(exp_k)
        ring = 2 * W + 2 * (H - 2)
        ring_k = -(-ring // -(-ring // cap))
        assert exp_k.tolist() == [ring_k, 1, cap, 0, 0, ring_k, 1, cap, (cap + 2) // 2, cap]          # steps: the ring's, 1, 1; then 2 and 3
        for turn in range(2):
            h.points_from_labels(ptr(d_lab), W, H, stride, ptr(d_comps), comp_cap, ptr(d_counts), frames)
            _, got_k = h.scores(1)
            ar.check("gather %d" % turn)
            assert got_k.tolist() == exp_k.tolist()
            p_pts, _ = h.gathered()
            got = np.frombuffer(d2h(p_pts, n * cap * 16).tobytes(), np.float64).reshape(n, cap, 2)
            for s in range(n):
                assert got[s, :exp_k[s]].tobytes() == exp_pts[s, :exp_k[s]].tobytes(), "set %d gathered points" % s
            for model in cm.MODELS:
                exp = [cm.find(exp_pts[s], exp_k[s], model, 64, seed=6, set_index=s) for s in range(n)]
                d_res.fill_(SENTINEL)
                d_mask.fill_(SENTINEL)
                h.find(0, 0, ptr(d_res), ptr(d_mask), model=model, tries=64, seed=6)
                tries_counts, _ = h.scores(64)
                ar.check("find on gathered points")
                res = np.frombuffer(d_res.cpu().numpy().tobytes(), cm.RESULT_DTYPE)
                mask = d_mask.cpu().numpy().reshape(n, cap)
                for s, e in enumerate(exp):
                    assert res[s].tobytes() == e["result"].tobytes(), (model, s, res[s], e["result"])
                    assert mask[s, :exp_k[s]].tobytes() == e["mask"].tobytes() and (mask[s, exp_k[s]:] == SENTINEL).all()
                    assert e["counts"] is None or tries_counts[s].tolist() == e["counts"].tolist()
            params = np.tile(np.array([1.0, -2.0, 3.0]), (n, 1))
            d_params = ar.new(params.nbytes, u8(params))
            d_dist.fill_(SENTINEL)
            h.distances(0, 0, cm.LINE, ptr(d_params), ptr(d_dist))
            h.scores(1)
            got = np.frombuffer(d_dist.cpu().numpy().tobytes(), np.float64).reshape(n, cap)
            for s in range(n):
                assert got[s, :exp_k[s]].tobytes() == cm.residuals(cm.LINE, 1.0, -2.0, 3.0, exp_pts[s, :exp_k[s]])[0].tobytes()
                assert got[s, exp_k[s]:].tobytes() == np.full(cap - exp_k[s], SENT64).tobytes()
    finally:
        h.close()


def test_chain_components_to_curves(hip_ctx):
    """plan.components -> points_from_labels -> find(d_points = NULL): a line, a parabola and a blob drawn into two 300 x 40 edge maps; the model is fed
    with the label maps and records the plan wrote"""
    from compv_amd import capi
    W, H, S, frames, comp_cap, cap = 300, 40, 304, 2, 6, 96
    edges = np.zeros((frames, H, S), np.uint8)
    x = np.arange(10, 290)
    edges[0, (5 + x // 12), x] = 255                                          # a slanted line
    edges[0, 30:34, 100:110] = 255                                            # a blob
    edges[1, np.clip(35 - ((x - 150) ** 2) // 700, 0, H - 1), x] = 255        # a parabola
    edges[1, 2, 5] = 255                                                      # one pixel
    ar = Arena()
    d_edges = ar.new(edges.nbytes, u8(edges))
    ar.keep(d_edges, u8(edges))
    d_lab, d_comps, d_counts = ar.new(frames * H * W * 4), ar.new(frames * comp_cap * 28), ar.new(frames * 4)
    d_res, d_mask = ar.new(frames * comp_cap * REC), ar.new(frames * comp_cap * cap)
    plan = capi.Plan(hip_ctx, W, H, S, frames)
    h = capi.Curvefit(hip_ctx, frames * comp_cap, cap, 128)
    try:
        for turn in range(2):
            plan.components(ptr(d_edges), 8, 1, ptr(d_lab), W, ptr(d_comps), comp_cap, ptr(d_counts))
            h.points_from_labels(ptr(d_lab), W, H, W, ptr(d_comps), comp_cap, ptr(d_counts), frames)
            h.find(0, 0, ptr(d_res), ptr(d_mask), model=cm.LINE, tries=128, threshold=1.5, seed=8)
            tries_counts, got_k = h.scores(128)
            ar.check("chain %d" % turn)
            labels = np.frombuffer(d_lab.cpu().numpy().tobytes(), np.int32).reshape(frames, H, W)
            comps = np.frombuffer(d_comps.cpu().numpy().tobytes(), cm.COMP_DTYPE).reshape(frames, comp_cap)
            counts = np.frombuffer(d_counts.cpu().numpy().tobytes(), np.int32)
            assert counts.tolist() == [2, 2]
            res = np.frombuffer(d_res.cpu().numpy().tobytes(), cm.RESULT_DTYPE)
            for f in range(frames):
                pts, ks = cm.gather(labels[f], W, comps[f], counts[f], comp_cap, cap)
                for c in range(comp_cap):
                    s = f * comp_cap + c
                    e = cm.find(pts[c], ks[c], cm.LINE, 128, threshold=1.5, seed=8, set_index=s)
                    assert got_k[s] == ks[c] and res[s].tobytes() == e["result"].tobytes(), (s, res[s], e["result"])
                    assert e["counts"] is None or tries_counts[s].tolist() == e["counts"].tolist()
            assert res[0]["status"] == 0 and res[0]["k"] == 94 and res[0]["inliers"] >= 85          # the line's 280 pixels, every third one
            assert res[comp_cap + 0]["k"] == 1 and res[comp_cap]["status"] == 2 and res[2]["status"] == 2 and res[2]["k"] == 0
    finally:
        h.close()
        plan.close()


# ---- stream order ----------------------------------------------------------------------------------------------------------------------------
def test_behind_pending_work_on_the_handles_stream(hip_ctx):
    """a handle created on a side stream: the inputs reach the device on that stream behind a delay, find, distances and the gather follow on it and
    return at once"""
    import torch
    from compv_amd import capi
    side = torch.cuda.Stream()
    model = cm.PARABOLA
    sets = [cc.planted(model, k, 0.3, 50 + k)[0] for k in (65, 40, 3)]
    rig = Rig(hip_ctx, sets, 65, 100, stream=side.cuda_stream, upload=False)          # d_pts holds the sentinel until the copy on the side stream lands
    host = torch.from_numpy(u8(rig.pts).copy()).pin_memory()
    params = np.array([[1.0, 2.0, 3.0]] * 3)
    d_params = rig.buffer(params)
    W, H, cap = 37, 29, 16
    lab, comps = label_frame(W, H, W, cap, np.random.default_rng(1))
    lab_host = torch.from_numpy(u8(lab).copy()).pin_memory()
    d_lab = rig.ar.new(lab.nbytes)
    d_comps, d_n = rig.buffer(comps[:4]), rig.buffer(np.array([4], np.int32))
    g = capi.Curvefit(hip_ctx, 4, cap, 8, stream=side.cuda_stream)
    try:
        exp = rig.model(model, 100, seed=2)
        for turn in range(2):
            rig.d_pts.fill_(SENTINEL)
            d_lab.fill_(SENTINEL)
            rig.ar.refill(rig.d_res)
            rig.ar.refill(rig.d_dist)
            rig.d_mask.fill_(SENTINEL)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                torch.cuda._sleep(20_000_000)          # a few milliseconds of pending work in front of the copies
                rig.d_pts.copy_(host, non_blocking=True)
                d_lab.copy_(lab_host, non_blocking=True)
            rig.h.find(ptr(rig.d_pts), ptr(rig.d_counts), ptr(rig.d_res), ptr(rig.d_mask), model=model, tries=100, seed=2)
            rig.h.distances(ptr(rig.d_pts), ptr(rig.d_counts), model, ptr(d_params), ptr(rig.d_dist))
            g.points_from_labels(ptr(d_lab), W, H, W, ptr(d_comps), 4, ptr(d_n), 1)
            side.synchronize()
            rig.check("behind pending work %d" % turn, model, 100, exp)
            got = np.frombuffer(rig.d_dist.cpu().numpy().tobytes(), np.float64).reshape(3, 65)
            for s in range(3):
                assert got[s, :rig.k(s)].tobytes() == cm.residuals(model, 1.0, 2.0, 3.0, rig.pts[s, :rig.k(s)])[0].tobytes()
            _, got_k = g.scores(1)
            exp_pts, exp_k = cm.gather(lab, W, comps[:4], 4, 4, cap)
            assert got_k.tolist() == exp_k.tolist()
            got_pts = np.frombuffer(d2h(g.gathered()[0], 4 * cap * 16).tobytes(), np.float64).reshape(4, cap, 2)
            for s in range(4):
                assert got_pts[s, :exp_k[s]].tobytes() == exp_pts[s, :exp_k[s]].tobytes()
    finally:
        g.close()
        rig.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(hip_ctx):
    import ctypes as C
    from compv_amd import capi
    lib = hip_ctx.lib
    E = capi.E_INVALID_PARAMETER
    hnd = C.c_void_p(99)
    for d in (capi.CurvefitDesc(0, 8, 8), capi.CurvefitDesc(65536, 8, 8), capi.CurvefitDesc(1, 2, 8), capi.CurvefitDesc(1, 8, 0)):
        assert lib.compvhip_curvefit_create(hip_ctx.h, C.byref(d), C.byref(hnd)) == E and hnd.value is None
    d = capi.CurvefitDesc(1, 8, 8)
    d.size = 20
    assert lib.compvhip_curvefit_create(hip_ctx.h, C.byref(d), C.byref(hnd)) == E and lib.compvhip_curvefit_create(hip_ctx.h, None, C.byref(hnd)) == E
    pts = cc.planted(cm.LINE, 20, 0.3, 1)[0]
    rig = Rig(hip_ctx, [pts, pts], 20, 16)
    try:
        h = rig.h.h
        P, N, R, M, D = ptr(rig.d_pts), ptr(rig.d_counts), ptr(rig.d_res), ptr(rig.d_mask), ptr(rig.d_dist)
        q = rig.buffer(np.zeros((2, 16, 2), np.int32))

        def find(p=P, n=N, o="ok", s=0, r=R, m=M, **kw):
            opts = capi.CurvefitOpts(kw.get("model", 0), kw.get("tries", 16), 0, kw.get("threshold", 1.0))
            opts.size = kw.get("size", opts.size)
            return lib.compvhip_curvefit_find(h, p or None, n or None, C.byref(opts) if o else None, s or None, r or None, m or None)
        assert find() == capi.OK
        rig.ar.refill(rig.d_res)
        rig.d_mask.fill_(SENTINEL)
        rig.ar.refill(rig.d_dist)
        for rc in (find(o=None), find(r=0), find(size=16), find(model=3), find(model=-1), find(tries=0), find(tries=17), find(threshold=0.0), find(threshold=-1.0),
                   find(threshold=float("nan")), find(p=P + 8), find(s=ptr(q) + 8), find(r=R + 4), find(n=N + 2), find(p=0)):
            assert rc in (E, capi.E_INVALID_STATE)
        assert find(p=0) == capi.E_INVALID_STATE          # nothing was gathered on this handle
        prm = rig.buffer(np.ones((2, 3)))
        dist = lib.compvhip_curvefit_distances
        assert dist(h, P, N, 0, ptr(prm), D) == capi.OK
        rig.ar.refill(rig.d_dist)
        for rc in (dist(h, P, N, 3, ptr(prm), D), dist(h, P, N, 0, None, D), dist(h, P, N, 0, ptr(prm), None), dist(h, P + 8, N, 0, ptr(prm), D),
                   dist(h, P, N, 0, ptr(prm) + 4, D), dist(h, P, N, 0, ptr(prm), D + 4), dist(h, P, N + 1, 0, ptr(prm), D)):
            assert rc == E
        gather = lib.compvhip_curvefit_points_from_labels
        lab = rig.buffer(np.zeros((8, 8), np.int32))
        rec = rig.buffer(np.zeros(2, cm.COMP_DTYPE))
        for rc in (gather(h, None, 8, 8, 8, ptr(rec), 2, N, 1), gather(h, ptr(lab), 8, 8, 7, ptr(rec), 2, N, 1), gather(h, ptr(lab), 8, 8, 8, ptr(rec), 1, N, 1),
                   gather(h, ptr(lab), 8, 8, 8, ptr(rec), 2, N, 2), gather(h, ptr(lab) + 2, 8, 8, 8, ptr(rec), 2, N, 1), gather(h, ptr(lab), 8, 8, 8, ptr(rec) + 1, 2, N, 1),
                   gather(h, ptr(lab), 8, 8, 8, ptr(rec), 2, N + 2, 1), gather(h, ptr(lab), 0, 8, 8, ptr(rec), 2, N, 1), gather(h, ptr(lab), 8, 40000, 8, ptr(rec), 2, N, 1)):
            assert rc == E
        assert find(p=0) == capi.E_INVALID_STATE          # a refused gather gathers nothing
        assert lib.compvhip_curvefit_scores(h, 0, None, None) == E and lib.compvhip_curvefit_scores(h, 17, None, None) == E
        rig.ar.check("refusals")          # guards and inputs
        for d in (rig.d_res, rig.d_mask, rig.d_dist):
            assert (d.cpu().numpy() == SENTINEL).all()
        assert hip_ctx.last_error()
    finally:
        rig.close()


def test_host_forms_and_timing(hip_ctx):
    """Context.fit_line / fit_parabola (compvhip_curvefit_find_f64) equal the model; n below m gives status 2; the timing names are the kernels'"""
    from compv_amd import capi
    for model, call in ((cm.LINE, lambda p, **kw: hip_ctx.fit_line(p, **kw)), (cm.PARABOLA, lambda p, **kw: hip_ctx.fit_parabola(p, **kw)),
                        (cm.PARABOLA_SIDEWAYS, lambda p, **kw: hip_ctx.fit_parabola(p, sideways=True, **kw))):
        pts, inl, _ = cc.noisy(model, 129, 0.3, 9)
        for turn in range(2):
            res, mask = call(pts, threshold=1.0, tries=300, seed=12)
            e = cm.find(pts, 129, model, 300, 1.0, seed=12)
            assert res.tobytes() == e["result"].tobytes() and mask.tobytes() == e["mask"].tobytes() and res["status"] == 0
        q = cm.samples(model, 1, 0, 129, 5)
        res, mask = call(pts, tries=5, samples=q)
        assert res.tobytes() == cm.find(pts, 129, model, 5, sample_list=q)["result"].tobytes()
        res, mask = call(pts[:1], tries=5)
        assert res["status"] == 2 and res["k"] == 1 and mask.tolist() == [0]
        res, mask = call(np.zeros((0, 2)), tries=5)
        assert res["status"] == 2 and res["k"] == 0 and len(mask) == 0
    h = capi.Curvefit(hip_ctx, 1, 16, 8)
    try:
        h.set_timing(1)
        ar = Arena()
        p = cc.planted(cm.LINE, 16, 0.0, 1)[0]
        d_p, d_r = ar.new(p.nbytes, u8(p)), ar.new(REC)
        h.find(ptr(d_p), 0, ptr(d_r), 0, tries=8)
        assert [n for n, _ in h.get_timing()] == ["curvefit_score_kernel", "curvefit_refit_kernel"]
    finally:
        h.close()
