"""GPU RANSAC homography (compvhip_homography_*) against tests/homography_model.py and the fixtures of tests/golden/golden_homography.*, bit for bit:
nothing here is compared with a tolerance.

Harness of tests/gpu_support.py: every device buffer sits between two guards; outputs start filled with a sentinel that must survive in
every slot the definition leaves unwritten (mask bytes at and after a pair's k); the inputs must come back unchanged, and the point slots behind a
pair's count hold seeded junk that is never read.

The solve kernel gives one workgroup 64 tries (one per lane), the score kernel 256 tries and 256 staged points per round, the refit kernel folds 64
partials, the gather scans 256 records per round.  Shapes are chosen from those numbers: tries 63, 64, 65 and 255, 256, 257; k 4, 5 (sum64 with one
point per partial), 63, 64, 65 (a second point in partial 0), 129, 255, 256, 257 (a staging round and one more)."""
import numpy as np
import pytest

import homography_cases as hc
import homography_model as hm
import match_model as mm
from fixtures import load_golden
from gpu_support import SENTINEL, Arena, ptr, u8
from homography_rig import REC, Rig
from match_rig import descriptors

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("golden_homography")


@pytest.mark.parametrize("tries", hc.TRIES)
def test_fixture_cases(hip_ctx, golden, tries):
    """every planted fixture case of this try count in ONE batched call (21 pairs: k 4 .. 129 x outlier shares 0, 30, 60 %), the fixture's own quads
    through d_quads: per-try (count, variance bits), records and masks as the generator stored them"""
    meta, arr = golden
    cases = [c for c in meta["cases"] if c["tries"] == tries and c["kind"] == "planted"]
    assert len(cases) == len(hc.KS) * len(hc.SHARES)
    sets = [(arr["src_" + c["points"]], arr["dst_" + c["points"]]) for c in cases]
    quads = [arr["quads_" + c["id"]].astype(np.int32) for c in cases]
    rig = Rig(hip_ctx, sets, max(hc.KS), tries)
    try:
        rig.run(tries, d_quads=rig.quads_buffer(np.stack(quads)), seed=5)
        exp = [dict(result=np.frombuffer(arr["result_" + c["id"]].tobytes(), hm.RESULT_DTYPE)[0], mask=arr["mask_" + c["id"]], counts=arr["counts_" + c["id"]],
                    variances=arr["varbits_" + c["id"]].view(np.float64), rotations=arr["rot_" + c["id"]]) for c in cases]
        res = rig.check("fixtures, %d tries" % tries, tries, exp)
        if tries == 200:
            for c, r in zip(cases, res):          # the planted inliers, exactly
                assert r["status"] == 0 and r["inliers"] == c["planted_inliers"], c["id"]
    finally:
        rig.close()


def test_fixture_edge_cases(hip_ctx, golden):
    """the fixture's collinear quad, repeated-index (singular) quad, out-of-range quad, all-outlier pair, all-collinear pair (no best: status 1) and the
    counts 3, negative and beyond pointCap, one batched call each through the generator or the stored quads"""
    meta, arr = golden
    for c in [c for c in meta["cases"] if c["kind"] != "planted"]:
        s, d = arr["src_" + c["points"]], arr["dst_" + c["points"]]
        quads = arr["quads_" + c["id"]].astype(np.int32) if c["given_quads"] else None
        rig = Rig(hip_ctx, [(s, d)], c["point_cap"], c["tries"], counts=[c["count"]])
        try:
            rig.run(c["tries"], d_quads=rig.quads_buffer(quads) if quads is not None else None, seed=c["seed"], threshold=c["threshold"])
            e = dict(result=np.frombuffer(arr["result_" + c["id"]].tobytes(), hm.RESULT_DTYPE)[0], mask=arr["mask_" + c["id"]], counts=None)
            if c["status"] != 2:
                e.update(counts=arr["counts_" + c["id"]], variances=arr["varbits_" + c["id"]].view(np.float64), rotations=arr["rot_" + c["id"]])
            res = rig.check(c["id"], c["tries"], [e])
            assert res[0]["status"] == c["status"], c["id"]
        finally:
            rig.close()


@pytest.mark.parametrize("tries", [63, 64, 65, 255, 256, 257])
def test_workgroup_boundaries_of_the_tries(hip_ctx, tries):
    """three pairs (k = 9, 65 and 129 with 30 % outliers) at the try counts either side of a solve workgroup (64) and a score workgroup (256), quads
    from the generator on the device, everything against the model"""
    sets = [hc.planted(k, 0.3, 40 + tries)[:2] for k in (9, 65, 129)]
    rig = Rig(hip_ctx, sets, 129, 257)
    try:
        rig.run(tries, seed=tries)
        exp = rig.model(tries, seed=tries)
        rig.check("%d tries" % tries, tries, exp)
        assert all(e["result"]["status"] == 0 for e in exp)
    finally:
        rig.close()


@pytest.mark.parametrize("k", [255, 256, 257])
def test_staging_rounds_of_the_points(hip_ctx, k):
    """k either side of the 256 points the score kernel stages per round (and four rounds of sum64 partials plus a rest), no count array (every pair
    full), no mask"""
    sets = [hc.planted(k, 0.3, 50)[:2], hc.planted(k, 0.0, 51)[:2]]
    rig = Rig(hip_ctx, sets, k, 64, counts=None)
    try:
        rig.run(64, seed=9, mask=False)
        exp = rig.model(64, seed=9)
        rig.check("k %d" % k, 64, exp, mask=False)
        assert exp[0]["result"]["inliers"] == k - int(0.3 * k) and exp[1]["result"]["inliers"] == k
    finally:
        rig.close()


def test_generated_quads_equal_given_quads_and_replay(hip_ctx):
    """the device generator against the same quads through d_quads (from the host entry point), on a stream, twice on the same handle; the timing
    entries; a threshold other than 30"""
    import torch
    from compv_amd import capi
    sets = [hc.planted(k, s, 60)[:2] for k, s in ((5, 0.0), (64, 0.3), (129, 0.6))]
    rig = Rig(hip_ctx, sets, 129, 200)
    try:
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        rig.run(200, seed=77, threshold=12.5, stream=st.cuda_stream)
        st.synchronize()
        exp = rig.model(200, seed=77, threshold=12.5)
        first = rig.check("generated", 200, exp).tobytes()
        quads = np.stack([capi.homography_quads(77, p, rig.k(p), 200) for p in range(3)])
        assert all(quads[p].tolist() == exp[p]["quads"].tolist() for p in range(3))
        rig.run(200, d_quads=rig.quads_buffer(quads), seed=1234, threshold=12.5, stream=st.cuda_stream)          # the seed no longer matters
        st.synchronize()
        assert rig.check("given", 200, exp).tobytes() == first
        rig.h.set_timing(1)
        rig.run(65, seed=77)
        t = rig.h.get_timing()
        assert [n for n, _ in t] == ["homography_solve_kernel", "homography_score_kernel", "homography_refit_kernel"] and all(ms >= 0 for _, ms in t)
        rig.h.set_timing(0)
        rig.check("fewer tries on the same handle", 65, rig.model(65, seed=77))
    finally:
        rig.close()


def test_count_edge_cases(hip_ctx):
    """device counts 3, 0, negative (status 2: zeros, nothing else written), 4 (the quad is the whole set), beyond pointCap (clamped), and a pair whose
    sources all lie on one line (every try scores 0: status 1, H of all points)"""
    cap = 20
    full = hc.planted(cap, 0.3, 70)[:2]
    sets = [full, full, full, hc.planted(4, 0.0, 71)[:2], full, hc.line_case(cap)]
    rig = Rig(hip_ctx, sets, cap, 64, counts=[3, 0, -7, 4, cap + 9, cap])
    try:
        rig.run(64, seed=3)
        exp = rig.model(64, seed=3)
        res = rig.check("counts", 64, exp)
        assert res["status"].tolist() == [2, 2, 2, 0, 0, 1] and res["inliers"][3] == 4 and res["inliers"][5] == 0 and res["rotations"][5] > 0
        assert not res["H"][:3].any() and (res["bestTry"][[0, 1, 2, 5]] == -1).all()
    finally:
        rig.close()


def keypoints(xy):
    k = np.zeros(len(xy), hm.KEYPOINT_DTYPE)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["strength"], k["orient"], k["level"], k["size"] = 50.0, 12.5, 0, 31.0
    return k


@pytest.mark.parametrize("shared", [False, True], ids=["own_train", "shared_train"])
def test_points_gathered_from_a_real_good_list(hip_ctx, shared):
    """Matcher.knn -> Matcher.good (ratio test) -> Homography.points -> find on the gathered points, three pairs: the same records and masks as find
    on the points the model gathers from the downloaded good list, and as the direct form on those points; then a hand-made good list with indices
    outside both capacities, a negative count and a count beyond goodCap, and a pointCap below the good count"""
    from compv_amd import capi
    pairs, qcap, tcap, B = 3, 300, 257, 32
    train_desc = descriptors("uniform", 1 if shared else pairs, tcap, B, B, 90)
    query_desc = descriptors("uniform", pairs, qcap, B, B, 91)
    rng = np.random.default_rng(92)
    train_xy = np.stack([rng.uniform(20, 620, (1 if shared else pairs, tcap)), rng.uniform(20, 460, (1 if shared else pairs, tcap))], axis=2).astype(np.float32)
    query_xy = np.stack([rng.uniform(0, 640, (pairs, qcap)), rng.uniform(0, 480, (pairs, qcap))], axis=2).astype(np.float32)
    for p in range(pairs):
        t = 0 if shared else p
        src_rows = rng.permutation(tcap)[:qcap // 2]          # half the queries are distinct train rows with one bit flipped, placed where H sends them
        query_desc[p, :len(src_rows), :B] = train_desc[t][src_rows, :B]
        flip = rng.integers(0, B, len(src_rows))
        query_desc[p, np.arange(len(src_rows)), flip] ^= np.uint8(1)
        query_xy[p, :len(src_rows)] = (hc.apply(hc.PLANTED_H, train_xy[t][src_rows].astype(np.float64)) + rng.uniform(-0.5, 0.5, (len(src_rows), 2))).astype(np.float32)
    ar = Arena()
    tk = np.stack([keypoints(x) for x in train_xy])
    qk = np.stack([keypoints(x) for x in query_xy])
    d_q, d_t = ar.new(query_desc.size, query_desc), ar.new(train_desc.size, train_desc)
    d_qk, d_tk = ar.new(qk.nbytes, u8(qk)), ar.new(tk.nbytes, u8(tk))
    ar.keep(d_qk, u8(qk))
    ar.keep(d_tk, u8(tk))
    d_matches, d_good, d_gc = ar.new(pairs * 2 * qcap * 16), ar.new(pairs * qcap * 16), ar.new(4 * pairs)
    d_res, d_mask = ar.new(pairs * REC), ar.new(pairs * qcap)
    m = capi.Matcher(hip_ctx, B, qcap, tcap, pairs, 2)
    h = capi.Homography(hip_ctx, pairs, qcap, 100)
    small = capi.Homography(hip_ctx, pairs, 40, 100)
    try:
        m.knn(ptr(d_q), B, 0, ptr(d_t), B, 0, shared, ptr(d_matches))
        m.good(ptr(d_matches), ptr(d_q), B, 0, ptr(d_t), B, 0, shared, ptr(d_good), qcap, ptr(d_gc), ratio=0.7)
        h.set_timing(1)
        h.points(ptr(d_good), qcap, ptr(d_gc), ptr(d_qk), qcap, ptr(d_tk), tcap, shared)
        assert [n for n, _ in h.get_timing()] == ["homography_points_kernel"]
        h.set_timing(0)
        h.find(0, 0, 0, ptr(d_res), ptr(d_mask), tries=100, seed=8)
        ar.check("gathered")
        good = np.frombuffer(d_good.cpu().numpy().tobytes(), mm.MATCH_DTYPE).reshape(pairs, qcap)
        gc = np.frombuffer(d_gc.cpu().numpy().tobytes(), np.int32)
        assert (gc >= qcap // 2 - 5).all() and (gc < qcap).all()
        res = np.frombuffer(d_res.cpu().numpy().tobytes(), hm.RESULT_DTYPE).copy()
        mask = d_mask.cpu().numpy().reshape(pairs, qcap).copy()
        sets = []
        for p in range(pairs):
            s, d = hm.gather(good[p], gc[p], qcap, qcap, qk[p], tk[0 if shared else p])
            sets.append((s, d))
            e = hm.find(s, d, len(s), 100, seed=8, pair=p)
            assert len(s) == gc[p] and res[p].tobytes() == e["result"].tobytes(), (p, res[p], e["result"])
            assert mask[p, :len(s)].tobytes() == e["mask"].tobytes() and (mask[p, len(s):] == SENTINEL).all()
            assert e["result"]["status"] == 0 and e["result"]["inliers"] >= qcap // 2 - 10
        rig = Rig(hip_ctx, sets, qcap, 100)          # the direct form on the same points
        try:
            rig.run(100, seed=8)
            assert np.frombuffer(rig.d_res.cpu().numpy().tobytes(), hm.RESULT_DTYPE).tobytes() == res.tobytes()
        finally:
            rig.close()
        # a hand-made list: records outside either capacity are dropped, the order kept; counts negative, beyond goodCap; pointCap 40 below the count
        bad = good.copy()
        bad[0, 3]["queryIdx"], bad[0, 5]["trainIdx"], bad[0, 6]["queryIdx"], bad[0, 9]["trainIdx"] = -1, tcap, qcap, -2
        counts = np.array([gc[0], -3, qcap + 50], np.int32)
        d_bad, d_bc = ar.new(bad.nbytes, u8(bad)), ar.new(12, u8(counts))
        ar.keep(d_bad, u8(bad))
        ar.refill(d_res)
        small.points(ptr(d_bad), qcap, ptr(d_bc), ptr(d_qk), qcap, ptr(d_tk), tcap, shared)
        small.find(0, 0, 0, ptr(d_res), 0, tries=64, seed=2)
        ar.check("hand-made list")
        res = np.frombuffer(d_res.cpu().numpy().tobytes(), hm.RESULT_DTYPE)
        for p in range(pairs):
            s, d = hm.gather(bad[p], counts[p], qcap, 40, qk[p], tk[0 if shared else p])
            assert len(s) == (36, 0, 40)[p]
            e = hm.find(s, d, len(s), 64, seed=2, pair=p)
            assert res[p].tobytes() == e["result"].tobytes(), (p, res[p], e["result"])
        assert res["status"].tolist() == [0, 2, 0]
    finally:
        m.close()
        h.close()
        small.close()


def test_projection(hip_ctx):
    """compvhip_homography_project: the frame's corners (one shared set) and per-pair points through every pair's H; a status 2 pair (H zeros) gives NaN"""
    sets = [hc.planted(9, 0.0, 80)[:2], hc.planted(65, 0.3, 81)[:2], hc.planted(9, 0.0, 82)[:2]]
    rig = Rig(hip_ctx, sets, 65, 64, counts=[9, 65, 2])
    try:
        rig.run(64, seed=4)
        res = rig.check("find", 64, rig.model(64, seed=4))
        corners = np.array([[0.0, 0.0], [639.0, 0.0], [639.0, 479.0], [0.0, 479.0], [320.5, 240.25]])
        own = np.random.default_rng(83).uniform(0, 640, (3, 300, 2))
        d_c, d_o = rig.ar.new(corners.nbytes, u8(corners)), rig.ar.new(own.nbytes, u8(own))
        rig.ar.keep(d_c, u8(corners))
        rig.ar.keep(d_o, u8(own))
        d_out_c, d_out_o = rig.ar.new(3 * corners.nbytes), rig.ar.new(own.nbytes)
        rig.h.set_timing(1)
        rig.h.project(ptr(rig.d_res), ptr(d_c), len(corners), True, ptr(d_out_c))
        assert [n for n, _ in rig.h.get_timing()] == ["homography_project_kernel"]
        rig.h.project(ptr(rig.d_res), ptr(d_o), 300, False, ptr(d_out_o))
        rig.ar.check("project")
        got_c = np.frombuffer(d_out_c.cpu().numpy().tobytes(), np.float64).reshape(3, -1, 2)
        got_o = np.frombuffer(d_out_o.cpu().numpy().tobytes(), np.float64).reshape(3, 300, 2)
        for p in range(3):
            assert got_c[p].tobytes() == hm.project(res[p]["H"], corners).tobytes() and got_o[p].tobytes() == hm.project(res[p]["H"], own[p]).tobytes(), p
        assert np.isnan(got_c[2]).all() and np.abs(got_c[0] - hc.apply(hc.PLANTED_H, corners)).max() < 5.0
    finally:
        rig.close()


def test_host_form(hip_ctx):
    src, dst, inl = hc.planted(65, 0.3, 85)
    e = hm.find(src, dst, 65, 200, seed=6)
    res, mask = hip_ctx.homography_find(src, dst, tries=200, seed=6)
    assert res.tobytes() == e["result"].tobytes() and mask.tobytes() == e["mask"].tobytes() and (mask != 0).tolist() == inl.tolist()
    q = e["quads"][:7]
    res, mask = hip_ctx.homography_find(src, dst, tries=7, quads=q, want_mask=False)
    assert res.tobytes() == hm.find(src, dst, 65, 7, quad_list=q)["result"].tobytes() and mask is None
    res, mask = hip_ctx.homography_find(src[:3], dst[:3], tries=5)
    assert res["status"] == 2 and not mask.any() and len(mask) == 3
    res, _ = hip_ctx.homography_find(np.zeros((0, 2)), np.zeros((0, 2)), tries=5)
    assert res["status"] == 2


def test_refusals_and_allocations(hip_ctx):
    import torch
    from compv_amd import capi

    def code(fn, *a, **k):
        with pytest.raises(capi.CompvHipError) as e:
            fn(*a, **k)
        return e.value.code
    torch.cuda.synchronize()
    start = hip_ctx.live_allocations()
    for bad in [(0, 8, 8), (1, 3, 8), (1, 8, 0), (65536, 8, 8)]:
        assert code(capi.Homography, hip_ctx, *bad) == capi.E_INVALID_PARAMETER, bad
    assert hip_ctx.live_allocations() == start
    rig = Rig(hip_ctx, [hc.planted(9, 0.0, 86)[:2]], 9, 16)
    try:
        assert hip_ctx.live_allocations() == start + 4          # all scratch at creation: points, counts, the tries' float64 and int32 words
        s, d, c, r, k = ptr(rig.d_src), ptr(rig.d_dst), ptr(rig.d_counts), ptr(rig.d_res), ptr(rig.d_mask)
        f = rig.h.find
        assert code(f, s, d, c, r, k, tries=0) == capi.E_INVALID_PARAMETER
        assert code(f, s, d, c, r, k, tries=17) == capi.E_INVALID_PARAMETER
        assert code(f, s, d, c, r, k, tries=8, threshold=0.0) == capi.E_INVALID_PARAMETER
        assert code(f, s, d, c, r, k, tries=8, threshold=float("nan")) == capi.E_INVALID_PARAMETER
        assert code(f, s, d, c, 0, k, tries=8) == capi.E_INVALID_PARAMETER
        assert code(f, s, 0, c, r, k, tries=8) == capi.E_INVALID_PARAMETER
        assert code(f, s + 8, d, c, r, k, tries=8) == capi.E_INVALID_PARAMETER          # points not 16-byte aligned
        assert code(f, s, d, c + 2, r, k, tries=8) == capi.E_INVALID_PARAMETER
        assert code(f, s, d, c, r + 4, k, tries=8) == capi.E_INVALID_PARAMETER
        assert code(f, s, d, c, r, k, tries=8, d_quads=s + 4) == capi.E_INVALID_PARAMETER
        assert code(f, 0, 0, 0, r, k, tries=8) == capi.E_INVALID_STATE                  # no gathered points yet
        assert code(rig.h.project, 0, s, 4, True, d) == capi.E_INVALID_PARAMETER
        assert code(rig.h.project, r, s + 8, 4, True, d) == capi.E_INVALID_PARAMETER
        assert code(rig.h.points, s, 8, c, 0, 8, d, 8) == capi.E_INVALID_PARAMETER
        assert code(rig.h.points, s + 4, 8, c, s, 8, d, 8) == capi.E_INVALID_PARAMETER
        rig.ar.check("refusals")
        assert (rig.d_res.cpu().numpy() == SENTINEL).all() and (rig.d_mask.cpu().numpy() == SENTINEL).all()
        rig.run(16, seed=1)
        rig.check("after the refusals", 16, rig.model(16, seed=1))
        assert hip_ctx.live_allocations() == start + 4          # no call allocates
        a = np.zeros((9, 2))
        assert code(hip_ctx.homography_find, a, a, tries=0) == capi.E_INVALID_PARAMETER
        assert code(hip_ctx.homography_find, a, a, tries=4, threshold=-1.0) == capi.E_INVALID_PARAMETER
    finally:
        rig.close()
    assert hip_ctx.live_allocations() == start
