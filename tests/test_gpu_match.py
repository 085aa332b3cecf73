"""GPU brute-force Hamming matching (compvhip_matcher_knn / _good and the host form compvhip_match_hamming_u8) against tests/match_model.py, byte
for byte.

Harness of tests/gpu_support.py: every device buffer sits between two guards; outputs start filled with a sentinel that must survive
in every slot the definition leaves unwritten -- match columns >= a pair's query count, good records behind a count --; the descriptors' stride
padding holds seeded random bytes (never read: the model only sees the descBytes in front of it) and the inputs must come back unchanged.

The slice kernel gives one workgroup a QUERY BLOCK of 256 queries (one per lane) and a TRAIN SLICE of 128 train rows; the merge kernel joins the
slices of a pair; the good kernel walks a pair's queries 256 at a time, four waves.  Shapes are chosen from those numbers:
  query caps  1, 63, 64, 65 (a wave and its neighbours), 255, 256, 257 (block - 1, block, block + 1)
  train caps  1, 2, 3 (fewer rows than neighbours asked for), 127, 128, 129 (slice - 1, slice, slice + 1), 257 (2 slices + 1)
  knn         1, 2, 3, 8 (the kernels keep lists of 1, 2, 4, 8), with knn > T
  descBytes   4, 32, 36, 128 (register widths 1, 8, 16 -- nine dwords padded --, 32), stride > descBytes; the widths in between (8, 12, 16, 24, 64 bytes:
              registers 2, 4 padded from three, 4, 8 padded from six, 16) on a reduced grid
The device call returns the canonical (distance, train index) order; the host form returns the reference's own order among equal distances
(match_model.knn_reference) and is held against the records of the compiled reference in tests/golden/golden_match.json directly."""
import hashlib
import json
import os

import numpy as np
import pytest

import match_model as mm
from gpu_support import SENTINEL, Arena, ptr
from match_rig import Rig, derived, descriptors

pytestmark = pytest.mark.gpu

BLOCK, SLICE = 256, 128
QUERY_CAPS = (1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1)
TRAIN_CAPS = (1, 2, 3, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 1)
KNN = (1, 2, 3, 8)
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("desc_bytes,stride", [(4, 8), (32, 48), (36, 40), (128, 132)], ids=lambda v: str(v))
def test_caps_sweep(hip_ctx, desc_bytes, stride):
    """every query cap x every train cap, two full pairs (one uniform, one tie-heavy), knn cycling through 1, 2, 3, 8 so that every cap meets
    every knn somewhere in the four descriptor widths"""
    i = desc_bytes          # start of the knn cycle differs per width
    seen = set()
    for qcap in QUERY_CAPS:
        for tcap in TRAIN_CAPS:
            knn = KNN[i % 4]
            i += 1
            seen.add((knn, knn > tcap))
            query = np.concatenate([descriptors("uniform", 1, qcap, desc_bytes, stride, i), descriptors("ties", 1, qcap, desc_bytes, stride, i + 1)])
            train = np.concatenate([descriptors("uniform", 1, tcap, desc_bytes, stride + 4, i + 2), descriptors("ties", 1, tcap, desc_bytes, stride + 4, i + 3)])
            rig = Rig(hip_ctx, desc_bytes, qcap, tcap, 2, knn, query, train)
            try:
                rig.knn_run()
                rig.knn_check("B %d Q %d T %d knn %d" % (desc_bytes, qcap, tcap, knn))
            finally:
                rig.close()
    assert {k for k, _ in seen} == set(KNN) and any(over for _, over in seen)


@pytest.mark.parametrize("desc_bytes,stride", [(8, 12), (12, 16), (16, 20), (24, 28), (64, 68)], ids=lambda v: str(v))
def test_caps_sweep_remaining_widths(hip_ctx, desc_bytes, stride):
    """the register widths test_caps_sweep leaves out -- match_slice_kernel<2, *>, <4, *> padded from three dwords and unpadded, <8, *> padded
    from six, <16, *> unpadded -- on a reduced grid (a single query, a wave + 1, a block + 1; fewer train rows than neighbours, a slice + 1,
    two slices + 1), knn cycling so that every width meets every knn"""
    i = desc_bytes // 4
    seen = set()
    for qcap in (1, 65, BLOCK + 1):
        for tcap in (3, SLICE + 1, 2 * SLICE + 1):
            knn = KNN[i % 4]
            i += 1
            seen.add(knn)
            query = np.concatenate([descriptors("uniform", 1, qcap, desc_bytes, stride, i), descriptors("ties", 1, qcap, desc_bytes, stride, i + 1)])
            train = np.concatenate([descriptors("uniform", 1, tcap, desc_bytes, stride + 4, i + 2), descriptors("ties", 1, tcap, desc_bytes, stride + 4, i + 3)])
            rig = Rig(hip_ctx, desc_bytes, qcap, tcap, 2, knn, query, train)
            try:
                rig.knn_run()
                rig.knn_check("B %d Q %d T %d knn %d" % (desc_bytes, qcap, tcap, knn))
            finally:
                rig.close()
    assert seen == set(KNN)


@pytest.mark.parametrize("cols", [33, 64, 100, 128])
def test_host_form_wide_descriptors_keep_the_reference_order(hip_ctx, cols):
    """compvhip_match_hamming_u8 above 32 bytes: match_reference_kernel<16, *> (33 and 64 bytes: nine dwords padded, sixteen) and <32, *> (100
    and 128 bytes: 25 dwords padded, 32), every list length, on tie-heavy rows -- the order among equal distances is what this kernel exists for"""
    Q, T = BLOCK + 1, SLICE + 1
    seed = {33: 11000, 64: 3000, 100: 5000, 128: 2000}[cols]          # seeds at which the two orders differ in what the lists keep (most do not show it)
    q, t = mm.content("ties", Q, cols, 300 + cols + seed), mm.content("ties", T, cols, 400 + cols + seed)
    D = mm.distances(q, t)
    differs = False
    for knn in KNN:
        exp = mm.knn_reference(q, t, knn, D)
        got = hip_ctx.match_hamming(q, t, knn)
        assert got.shape == (knn, Q)
        assert got.tobytes() == exp.tobytes(), (cols, knn)
        differs = differs or mm.knn(q, t, knn, D).tobytes() != exp.tobytes()
    assert differs          # the content tells the reference's order from the (distance, train index) order


@pytest.mark.parametrize("tcap", [1, 2, 3])
@pytest.mark.parametrize("knn", [2, 3, 8])
def test_more_neighbours_than_train_rows(hip_ctx, tcap, knn):
    """knn = 2, 3, 8 against T = 1, 2, 3 train rows, crossed, at the query caps either side of the block seam (255, 256, 257) and with the train
    count on the device as well (a cap of 129 -- two slices, the second with one row -- whose count says tcap): rows r >= T hold {q, -1, 0, INT32_MAX}"""
    B, stride = 32, 36
    for qcap in (BLOCK - 1, BLOCK, BLOCK + 1):
        query = np.concatenate([descriptors("uniform", 1, qcap, B, stride, 80 + qcap), descriptors("ties", 1, qcap, B, stride, 81 + qcap)])
        for cap, t_counts in ((tcap, None), (SLICE + 1, [tcap, tcap])):
            train = np.concatenate([descriptors("uniform", 1, cap, B, stride, 82 + tcap), descriptors("ties", 1, cap, B, stride, 83 + tcap)])
            rig = Rig(hip_ctx, B, qcap, cap, 2, knn, query, train, None, t_counts)
            try:
                rig.knn_run()
                rig.knn_check("Q %d T %d of cap %d knn %d" % (qcap, tcap, cap, knn))
                m = mm.knn_device(*rig.sides(0), knn)
                assert m.shape == (knn, qcap)
                if knn > tcap:
                    assert (m[tcap:]["trainIdx"] == -1).all() and (m[tcap:]["distance"] == 0x7fffffff).all() and (m[:tcap]["trainIdx"] >= 0).all()
            finally:
                rig.close()


def ragged(cap):
    return [0, 1, cap, cap + 7, cap // 2 + 3]


@pytest.mark.parametrize("shared", [False, True], ids=["own_train", "shared_train"])
def test_ragged_pairs_and_the_good_list(hip_ctx, shared):
    """5 pairs whose device counts are 0, 1, cap, cap + 7 (clipped) and a middle value, on both sides (the train counts rotated, so that an empty
    query side meets a full train side); then the good list on the same matches: each filter alone, all three, goodCap 0, small and ample.  Pair
    p = 1 of the unshared run has ONE train row under the ratio test; the shared run has one train set and one train count."""
    qcap, tcap, knn, B = BLOCK + 1, 2 * SLICE + 1, 3, 32
    q_counts = ragged(qcap)
    t_counts = [tcap - 5] if shared else ragged(tcap)[2:] + ragged(tcap)[:2]          # cap, cap + 7, mid, 0, 1
    train = descriptors("uniform", 1 if shared else 5, tcap, B, 36, 42)
    query = descriptors("uniform", 5, qcap, B, 48, 41)
    for p in range(5):
        query[p, :, :B] = derived(train[0 if shared else p], qcap, B, 43 + p)
    rig = Rig(hip_ctx, B, qcap, tcap, 5, knn, query, train, q_counts, t_counts, shared, good_cap=qcap)
    try:
        rig.knn_run()
        rig.knn_check("ragged")
        if not shared:
            assert [len(rig.sides(p)[1]) for p in range(5)] == [tcap, tcap, tcap // 2 + 3, 0, 1] and len(rig.sides(4)[0]) == qcap // 2 + 3
        assert 0.7 * 7.0 != 4.9          # the ratio's products are not exactly representable
        filters = [dict(ratio=0.7), dict(max_distance=20), dict(cross_check=True), dict(ratio=0.7, max_distance=20, cross_check=True), dict()]
        totals = []
        for o in filters:
            rig.good_run(**o)
            counts, total = rig.good_check("good %r" % o, **o)
            totals.append(total)
        assert totals[4] > max(totals[:3]) and min(totals[:3]) > totals[3] > 0          # every filter removes something, together they remove more
        o = filters[3]
        rig.good_run(good_cap=0, **o)
        counts, _ = rig.good_check("counts only", good_cap=0, **o)
        small = max(1, int(counts.max()) // 2)
        rig.good_run(good_cap=small, **o)
        rig.good_check("goodCap %d below the count" % small, good_cap=small, **o)
    finally:
        rig.close()


def test_ties_across_every_seam(hip_ctx):
    """64 distinct descriptors repeated with period 64 through the train rows (some with one bit flipped), so that every query has equally distant
    train rows in EVERY slice, and EQUAL rows either side of every train-slice seam (127 | 128, 255 | 256, 383 | 384) and every query-block seam
    (255 | 256, 511 | 512): neighbours 1 and 2 of a query (rows j + 64 and j + 128) lie either side of the first seam at the same distance, knn = 8
    reaches into the third slice, and only the merge's (distance, train index) order tells them apart.  The cross check's reverse run has the
    same ties in (distance, query index)."""
    qcap, tcap, B = 2 * BLOCK + 1, 3 * SLICE + 1, 32
    pool = mm.uniform(64, B, 50)
    rng = np.random.default_rng(53)

    def periodic(sets, cap, stride, seed):
        out = descriptors("uniform", sets, cap, B, stride, seed)
        for s in range(sets):
            out[s, :, :B] = pool[(np.arange(cap) + 7 * s) % 64]
            for i in rng.integers(0, cap, cap // 5):
                out[s, i, rng.integers(0, B)] ^= np.uint8(1 << rng.integers(0, 8))
        return out
    query, train = periodic(2, qcap, 32, 51), periodic(2, tcap, 64, 52)
    for s in range(2):
        for seam in range(SLICE, tcap, SLICE):
            train[s, seam, :B] = train[s, seam - 1, :B]
        for seam in range(BLOCK, qcap, BLOCK):
            query[s, seam, :B] = query[s, seam - 1, :B]
    for knn in (3, 8):
        rig = Rig(hip_ctx, B, qcap, tcap, 2, knn, query, train, good_cap=qcap)
        try:
            rig.knn_run()
            rig.knn_check("seams knn %d" % knn)
            m = mm.knn_device(*rig.sides(0), knn)
            tie = (m[1]["distance"] == m[2]["distance"]) & (m[1]["trainIdx"] // SLICE != m[2]["trainIdx"] // SLICE)
            assert tie.sum() > qcap // 4          # two neighbours of many queries are equally far and come from different slices
            if knn == 8:
                assert (m[5]["trainIdx"] // SLICE == 2).sum() > qcap // 4 and (m[4]["distance"] == m[5]["distance"]).sum() > qcap // 4
            rig.good_run(cross_check=True)
            rig.good_check("seams cross check", cross_check=True)
        finally:
            rig.close()


def test_ratio_is_one_binary64_multiply(hip_ctx):
    """d0 = 55, d1 = 100, ratio 0.55: 0.55 * 100.0 = 55.00000000000001 in binary64, so 55 < ratio * d1 holds although 55 < 55 does not; in binary32
    the product is 55 and the query would fail.  The second pair has ONE train row (count 1): the ratio test passes none there."""
    assert 0.55 * 100.0 > 55.0 and not np.float32(0.55) * np.float32(100.0) > np.float32(55.0)
    B, qcap, tcap = 32, 4, 4
    query = np.zeros((2, qcap, B), np.uint8)
    train = np.full((2, tcap, B), 0xff, np.uint8)
    train[:, 0, :] = 0
    train[:, 0, :7] = [0xff] * 6 + [0x7f]                  # 55 bits
    train[:, 1, :] = 0
    train[:, 1, :13] = [0xff] * 12 + [0x0f]                # 100 bits
    query[:, 1, 31] = 0x01                                 # d0 = 56, d1 = 101: 56 < 55.55 fails
    rig = Rig(hip_ctx, B, qcap, tcap, 2, 2, query, train, [qcap, qcap], [tcap, 1], good_cap=qcap)
    try:
        rig.knn_run()
        rig.knn_check("ratio literal")
        assert mm.knn_device(*rig.sides(0), 2)["distance"][:, 0].tolist() == [55, 100]
        rig.good_run(ratio=0.55)
        counts, _ = rig.good_check("ratio 0.55", ratio=0.55)
        assert counts.tolist() == [3, 0]
    finally:
        rig.close()


def test_host_form_against_the_golden_file(hip_ctx):
    """compvhip_match_hamming_u8 on the fixture's cols = 5 and cols = 32 cases, held against the MD5 recorded from the compiled reference
    directly (no model in between): shape min(knn, T) x Q, the reference's own order among equal distances"""
    with open(os.path.join(HERE, "golden", "golden_match.json")) as f:
        golden = json.load(f)
    n = 0
    cache = {}
    for c in golden["cases"]:
        if c["cols"] not in (5, 32):
            continue
        key = (c["content"], c["cols"], c["Q"], c["T"], c["seed"])
        if key not in cache:
            cache[key] = (mm.content(c["content"], c["Q"], c["cols"], c["seed"]), mm.content(c["content"], c["T"], c["cols"], c["seed"] + 100000))
        q, t = cache[key]
        m = hip_ctx.match_hamming(q, t, c["knn"])
        assert m.shape == (c["rows"], c["Q"]), c
        assert hashlib.md5(np.ascontiguousarray(m).view("<i4").tobytes()).hexdigest() == c["md5"], c
        n += 1
    assert n == 400
    # a strided host view, and a match matrix wider than Q
    rng = np.random.default_rng(3)
    big_q, big_t = rng.integers(0, 256, (70, 40), dtype=np.uint8), rng.integers(0, 256, (9, 40), dtype=np.uint8)
    q, t = big_q[:, :7], big_t[:, :7]
    assert hip_ctx.match_hamming(q, t, 3).tobytes() == mm.knn_reference(q, t, 3).tobytes()


def test_stream_and_determinism(hip_ctx):
    import torch
    qcap, tcap, B = BLOCK + 1, SLICE + 1, 36
    rig = Rig(hip_ctx, B, qcap, tcap, 3, 2, descriptors("ties", 3, qcap, B, 40, 61), descriptors("ties", 3, tcap, B, 40, 62), good_cap=qcap)
    try:
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        rig.knn_run(stream=st.cuda_stream)
        rig.good_run(stream=st.cuda_stream, ratio=0.7, cross_check=True)
        st.synchronize()
        first = rig.knn_check("on a stream")
        rig.good_check("good on a stream", ratio=0.7, cross_check=True)
        good_first = rig.d_good.cpu().numpy().tobytes()
        rig.ar.refill(rig.d_matches)
        rig.knn_run(stream=st.cuda_stream)
        rig.good_run(stream=st.cuda_stream, ratio=0.7, cross_check=True)
        st.synchronize()
        assert rig.knn_check("again") == first and rig.d_good.cpu().numpy().tobytes() == good_first
        rig.m.set_timing(1)
        rig.knn_run()
        assert [n for n, _ in rig.m.get_timing()] == ["match_slice_kernel", "match_merge_kernel"]
        rig.good_run(cross_check=True)
        t = rig.m.get_timing()
        assert [n for n, _ in t] == ["match_reverse_slice_kernel", "match_reverse_merge_kernel", "match_good_kernel"] and all(ms >= 0 for _, ms in t)
        rig.m.set_timing(0)
    finally:
        rig.close()


def test_fast_counts_feed_the_matcher(hip_ctx):
    """compvhip_plan_fast's d_counts -- corners before clipping to cornerCap -- goes straight in as d_queryCounts with queryCap = cornerCap; the
    descriptors are synthetic, indexed by corner.  One frame has more corners than the capacity, one has none."""
    import fast_model as fm
    from compv_amd import capi
    W, H, S, F, cap, B = 64, 48, 64, 3, 40, 32
    frames = np.stack([fm.noise(W, H, 5), np.full((H, W), 9, np.uint8), fm.blocks(W, H, 6)])
    ar = Arena()
    d_in = ar.new(F * H * S, np.ascontiguousarray(frames))
    d_corners = ar.new(F * cap * fm.CORNER_DTYPE.itemsize)
    d_counts = ar.new(4 * F)
    plan = capi.Plan(hip_ctx, W, H, S, F)
    query = descriptors("uniform", F, cap, B, B, 71)
    train = descriptors("uniform", 1, 50, B, B, 72)
    try:
        plan.fast(ptr(d_in), 20, 9, True, -1, 0, ptr(d_corners), cap, ptr(d_counts))
        ar.check("fast")
        counts = np.frombuffer(d_counts.cpu().numpy().tobytes(), np.int32).tolist()
        assert counts == [len(fm.fast(frames[f], 20, 9, True)[0]) for f in range(F)] and counts[0] > cap and counts[1] == 0
        rig = Rig(hip_ctx, B, cap, 50, F, 2, query, train, q_counts=counts, shared=True)
        try:
            rig.m.knn(ptr(rig.d_query), B, ptr(d_counts), ptr(rig.d_train), B, 0, True, ptr(rig.d_matches))          # the FAST call's own count array
            rig.knn_check("chained")
            ar.check("chained")
        finally:
            rig.close()
    finally:
        plan.close()


def test_refusals_and_allocations(hip_ctx):
    import torch
    from compv_amd import capi

    def code(fn, *a, **k):
        with pytest.raises(capi.CompvHipError) as e:
            fn(*a, **k)
        return e.value.code
    torch.cuda.synchronize()
    start = hip_ctx.live_allocations()
    for bad in [(0, 4, 4, 1, 1), (2, 4, 4, 1, 1), (30, 4, 4, 1, 1), (132, 4, 4, 1, 1), (32, 0, 4, 1, 1), (32, 4, 0, 1, 1), (32, 4, 4, 0, 1), (32, 4, 4, 1, 0), (32, 4, 4, 1, 9)]:
        assert code(capi.Matcher, hip_ctx, *bad) == capi.E_INVALID_PARAMETER, bad
    assert hip_ctx.live_allocations() == start
    query, train = descriptors("uniform", 1, 8, 32, 32, 1), descriptors("uniform", 1, 8, 32, 32, 2)
    rig = Rig(hip_ctx, 32, 8, 8, 1, 1, query, train, good_cap=8)
    try:
        assert hip_ctx.live_allocations() == start + 2          # all scratch at creation: the key words and the reverse records
        q, t, mt, g, gc = ptr(rig.d_query), ptr(rig.d_train), ptr(rig.d_matches), ptr(rig.d_good), ptr(rig.d_gc)
        assert code(rig.m.knn, 0, 32, 0, t, 32, 0, False, mt) == capi.E_INVALID_PARAMETER
        assert code(rig.m.knn, q, 32, 0, 0, 32, 0, False, mt) == capi.E_INVALID_PARAMETER
        assert code(rig.m.knn, q, 32, 0, t, 32, 0, False, 0) == capi.E_INVALID_PARAMETER
        assert code(rig.m.knn, q, 28, 0, t, 32, 0, False, mt) == capi.E_INVALID_PARAMETER          # stride below descBytes
        assert code(rig.m.knn, q, 32, 0, t, 34, 0, False, mt) == capi.E_INVALID_PARAMETER          # no multiple of 4
        assert code(rig.m.knn, q, 32, 0, t, 32, 0, False, mt + 4) == capi.E_INVALID_PARAMETER      # records not 16-byte aligned
        assert code(rig.m.knn, q + 2, 32, 0, t, 32, 0, False, mt) == capi.E_INVALID_PARAMETER
        assert code(rig.m.good, mt, q, 32, 0, t, 32, 0, False, g, 8, gc, ratio=0.8) == capi.E_INVALID_PARAMETER          # the ratio test on knn = 1
        assert code(rig.m.good, mt, q, 32, 0, t, 32, 0, False, 0, 8, gc) == capi.E_INVALID_PARAMETER                     # a capacity without a buffer
        assert code(rig.m.good, mt, q, 32, 0, t, 32, 0, False, g, 8, 0) == capi.E_INVALID_PARAMETER
        assert code(rig.m.good, 0, q, 32, 0, t, 32, 0, False, g, 8, gc) == capi.E_INVALID_PARAMETER
        rig.ar.check("refusals")
        assert (rig.d_matches.cpu().numpy() == SENTINEL).all() and (rig.d_good.cpu().numpy() == SENTINEL).all()
        rig.knn_run()
        rig.good_run(cross_check=True, max_distance=200)
        assert hip_ctx.live_allocations() == start + 2          # no call allocates
        rig.knn_check("after the refusals")
        rig.good_check("after the refusals", cross_check=True, max_distance=200)
        a = np.zeros((4, 32), np.uint8)
        assert code(hip_ctx.match_hamming, a, a, 0) == capi.E_INVALID_PARAMETER and code(hip_ctx.match_hamming, a, a, 9) == capi.E_INVALID_PARAMETER
        assert code(hip_ctx.match_hamming, np.zeros((4, 129), np.uint8), np.zeros((4, 129), np.uint8), 1) == capi.E_INVALID_PARAMETER
    finally:
        rig.close()
    assert hip_ctx.live_allocations() == start


# ---- the CompV binding ---------------------------------------------------------------------------------------------------------------------
def test_plugin_factory_returns_the_reference_records():
    """integration/compv_hip_plugin.cxx re-registers COMPV_BRUTEFORCE_ID: headless_samples runs the reference's built-in matcher and the HIP one the
    factory returns afterwards on the same seeded descriptors (KNN 2) and compares the record matrices byte for byte.

    Skipped, before anything runs, when oracle/_ref holds no headless_samples built with the matcher call: the directory is absent, or it was built
    from sources older than the binding (such a program does not hold the text of the report line and ignores the switch).  Whatever a program
    that has the call then does -- any exit code but 0, a crash, a DIFF -- fails the test."""
    import subprocess
    exe = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "headless_samples")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref not built (needs the reference checkout; see oracle/build_ref.sh)")
    with open(exe, "rb") as f:
        if b"bruteforce_matches: %s" not in f.read():
            pytest.skip("oracle/_ref/headless_samples was built before the matcher binding existed (rebuild it with oracle/build_ref.sh where the reference checkout is)")
    for shape in (("300", "257"), ("2000", "2000")):
        out = subprocess.run([exe, "--match-only", *shape], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        assert "bruteforce_matches: MATCH" in out.stdout, out.stdout[-2000:]
