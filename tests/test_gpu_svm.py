"""GPU SVM prediction (compvhip_svm_*) against the fixture the compiled reference made (tests/golden/golden_svm.*, svm_*.model) and tests/svm_model.py,
bit for bit in labels, decision values and kernel values: nothing here is compared with a tolerance.

Harness of tests/gpu_support.py: every device buffer sits between two guards; outputs start filled with a sentinel that must survive in every
element behind n and in every refused call; the queries are staged at a stride above D with a large finite sentinel in the padding, which would show in
any kernel value that read it.

svm_kvalues_kernel gives a workgroup 64 queries x 64 support vectors and stages 32 columns at a time; shapes come from those numbers (tests/svm_cases.py):
D around 16 and 32, 67 = two chunks + 3, 3780; n 1, 63, 64, 65, 257; l up to 67; segment lengths 1, 17, 32."""
import ctypes as C

import numpy as np
import pytest

import svm_cases as sc
import svm_model as sm
from gpu_support import SENTINEL, Arena, ptr, u8
from svm_rig import PAD, Rig

pytestmark = pytest.mark.gpu

CASES = sc.all_cases()
BY_ID = {c["id"]: c for c in CASES}


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["id"])
def test_cases_against_the_fixture(hip_ctx, c):
    _, A = sc.golden()
    cid = c["id"]
    labels, dec, K = A["lab_" + cid], A["dec_" + cid], A["K_" + cid]
    rig = Rig(hip_ctx, c, c["nq"] + 3, from_arrays=CASES.index(c) % 2 == 1)
    try:
        info = rig.h.info()
        assert (info["kernel"], info["nrClass"], info["totalSV"], info["dim"], info["pairs"], info["maxVectors"]) == (rig.m.kernel, rig.m.nr_class, rig.m.l, rig.m.dim, rig.m.pairs,
                                                                                                                         c["nq"] + 3)
        rig.ar.keep(rig.d_x, u8(rig.host_rows(sc.queries(c, rig.m))))
        rig.load(sc.queries(c, rig.m))
        for n in (sc.N_SIZES if c["nq"] == 257 else (c["nq"],)):
            for has_dec, has_k in ((True, True), (False, False), (True, False)):
                rig.run(n, has_dec, has_k)
                rig.check("%s n %d dec %d K %d" % (cid, n, has_dec, has_k), n, labels, dec, K, has_dec, has_k)
    finally:
        rig.close()


def test_one_handle_across_changing_n_and_content(hip_ctx):
    """nothing is carried from call to call: the expectation of every call is the model on that call's own queries"""
    c = BY_ID["rbf_d33_c2"]
    rig = Rig(hip_ctx, c, 257)
    try:
        X = sc.queries(c, rig.m)
        rng = np.random.RandomState(5)
        for turn, n in enumerate((257, 1, 65, 64, 200, 3)):
            x = X[rng.permutation(257)[:n]] if turn % 2 else (X[:n] * np.float32(1.0 + turn / 8)).astype(np.float32)
            labels, dec, K = sm.predict(rig.m, x)
            rig.load(x)
            has_k = turn % 3 != 2
            rig.run(n, has_k, has_k)
            rig.check("turn %d n %d" % (turn, n), n, labels, dec, K, has_k, has_k)
    finally:
        rig.close()


def test_behind_pending_work_on_the_handles_stream(hip_ctx):
    """a handle created on a side stream: the queries reach the device on that stream behind a delay, the call follows on it and returns at once"""
    import torch
    c = BY_ID["hand_l67"]
    _, A = sc.golden()
    side = torch.cuda.Stream()
    rig = Rig(hip_ctx, c, 65, stream=side.cuda_stream)
    try:
        host = torch.from_numpy(u8(rig.host_rows(sc.queries(c, rig.m))).copy()).pin_memory()
        for turn in range(2):
            rig.d_x.fill_(SENTINEL)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                torch.cuda._sleep(20_000_000)          # a few milliseconds of pending work in front of the copy
                rig.d_x.copy_(host, non_blocking=True)
            rig.run(65)
            side.synchronize()
            rig.check("behind pending work %d" % turn, 65, A["lab_hand_l67"], A["dec_hand_l67"], A["K_hand_l67"])
    finally:
        rig.close()


def test_host_form_slices_and_timing(hip_ctx):
    _, A = sc.golden()
    c = BY_ID["lin_d21_c3"]
    m = sc.recorded_model(c)
    X = sc.queries(c, m)
    from compv_amd import capi
    for max_vectors, reps in ((100, 1), (4096, 3)):          # slices of 100; slices of 512
        h = capi.Svm(hip_ctx, sc.model_path(c["id"]), max_vectors)
        try:
            x = np.concatenate([X] * reps)
            wide = sc.padded(x, c["D"] + 2, PAD)
            labels, dec = h.predict_host(wide[:, :c["D"]], want_dec=True)          # a strided view: rows D + 2 apart
            assert labels.tobytes() == np.concatenate([A["lab_" + c["id"]]] * reps).tobytes()
            assert dec.tobytes() == np.concatenate([A["dec_" + c["id"]]] * reps).tobytes()
            assert h.predict_host(x.astype(np.float32)).tobytes() == sm.predict(m, x.astype(np.float32))[0].tobytes()
            h.set_timing(1)
            h.predict_host(x[:7])
            t = h.get_timing()
            assert [n for n, _ in t] == ["svm_kvalues_kernel", "svm_decide_kernel"] and all(ms >= 0 for _, ms in t)
        finally:
            h.close()


def test_allocations_are_made_at_creation_and_returned(hip_ctx):
    c = BY_ID["rbf_d16_c5"]
    _, A = sc.golden()
    start = hip_ctx.live_allocations()
    rig = Rig(hip_ctx, c, c["nq"])
    try:
        made = hip_ctx.live_allocations()
        assert made > start
        x = sc.queries(c, rig.m)
        rig.load(x)
        for _ in range(2):
            rig.run(c["nq"])
            rig.check("allocations", c["nq"], A["lab_" + c["id"]], A["dec_" + c["id"]], A["K_" + c["id"]])
            rig.h.predict_host(x, want_dec=True)
            assert hip_ctx.live_allocations() == made          # no later call allocates
    finally:
        rig.close()
    assert hip_ctx.live_allocations() == start


def test_refusals_leave_everything_untouched(hip_ctx, tmp_path):
    from compv_amd import capi
    lib, E = hip_ctx.lib, capi.E_INVALID_PARAMETER
    start = hip_ctx.live_allocations()
    good = capi.SvmModel.from_file(sc.model_path("rbf_d17_c2"))
    hnd = C.c_void_p(99)

    def create(model_struct, desc):
        hnd.value = 99
        rc = lib.compvhip_svm_create(hip_ctx.h, C.byref(model_struct) if model_struct is not None else None, C.byref(desc) if desc is not None else None, C.byref(hnd))
        assert hnd.value is None
        return rc
    for mv in (0, (1 << 22) + 1, (1 << 31) // good.l + 1):
        assert create(good.struct(), capi.SvmDesc(mv)) == E
    d = capi.SvmDesc(8)
    d.size = 12
    assert create(good.struct(), d) == E and create(good.struct(), None) == E and create(None, capi.SvmDesc(8)) == E
    for field, value in (("size", 64), ("kernel", 1), ("kernel", 3), ("kernel", 4), ("nrClass", 1), ("nrClass", 33), ("totalSV", 0), ("totalSV", good.l + 1), ("dim", 0), ("sv", None),
                         ("label", None)):
        s = good.struct()
        setattr(s, field, value)
        assert create(s, capi.SvmDesc(8)) == E, field
    assert lib.compvhip_svm_create(hip_ctx.h, C.byref(good.struct()), C.byref(capi.SvmDesc(8)), None) == E
    for name in ("poly", "sparse_gap", "epsilon_svr", "truncated_lines"):
        path = str(tmp_path / (name + ".model"))
        sc.write_bad_file(path, name)
        hnd.value = 99
        assert lib.compvhip_svm_create_from_file(hip_ctx.h, path.encode(), C.byref(capi.SvmDesc(8)), C.byref(hnd)) == E and hnd.value is None
    assert hip_ctx.live_allocations() == start          # a refused create leaves nothing behind

    c = BY_ID["rbf_d17_c2"]          # float64 queries
    rig = Rig(hip_ctx, c, 24, max_vectors=20)
    try:
        _, A = sc.golden()
        rig.ar.keep(rig.d_x, u8(rig.host_rows(sc.queries(c, rig.m))))
        rig.load(sc.queries(c, rig.m))
        for b in (rig.d_lab, rig.d_dec, rig.d_k):
            rig.ar.refill(b)
        h, x, lab, dec, k, S = rig.h.h, ptr(rig.d_x), ptr(rig.d_lab), ptr(rig.d_dec), ptr(rig.d_k), rig.stride
        F64, F32 = capi.SVM_F64, capi.SVM_F32
        calls = [(x, F64, 0, S, lab, dec, k), (x, F64, 21, S, lab, dec, k), (x, F64, 8, c["D"] - 1, lab, dec, k), (x, 2, 8, S, lab, dec, k), (x, -1, 8, S, lab, dec, k),
                 (None, F64, 8, S, lab, dec, k), (x, F64, 8, S, None, dec, k),
                 (x + 1, F64, 8, S, lab, dec, k), (x + 4, F64, 8, S, lab, dec, k), (x + 2, F32, 8, S, lab, dec, k), (x + 1, F32, 8, S, lab, dec, k),
                 (x, F64, 8, S, lab + 1, dec, k), (x, F64, 8, S, lab + 2, dec, k), (x, F64, 8, S, lab, dec + 4, k), (x, F64, 8, S, lab, dec + 1, k),
                 (x, F64, 8, S, lab, dec, k + 4), (x, F64, 8, S, lab, dec, k + 2), (x, F64, 8, 1 << 40, lab, dec, k)]
        for args in calls:
            assert lib.compvhip_svm_predict(h, *args) == E, args
            assert hip_ctx.last_error()
        rig.check("refused calls", 0, A["lab_" + c["id"]], A["dec_" + c["id"]], A["K_" + c["id"]])          # every output still holds the sentinel
        labels = np.full(8, 77, np.int32)
        hx = np.zeros((8, c["D"]))
        for args in ((hx.ctypes.data, F64, 0, c["D"], labels.ctypes.data, None), (hx.ctypes.data, F64, 8, c["D"] - 1, labels.ctypes.data, None),
                     (hx.ctypes.data, 5, 8, c["D"], labels.ctypes.data, None), (None, F64, 8, c["D"], labels.ctypes.data, None), (hx.ctypes.data, F64, 8, c["D"], None, None)):
            assert lib.compvhip_svm_predict_host(h, *args) == E
        assert (labels == 77).all()
        s = capi.SvmShape()
        s.size = 36
        assert lib.compvhip_svm_info(h, C.byref(s)) == E and lib.compvhip_svm_info(h, None) == E
        rig.run(20)          # the handle still serves: n == maxVectors, 4-byte aligned float32 rows are another case's business
        rig.check("after the refusals", 20, A["lab_" + c["id"]], A["dec_" + c["id"]], A["K_" + c["id"]])
    finally:
        rig.close()
    assert hip_ctx.live_allocations() == start


def test_hog_descriptors_feed_the_svm_without_a_host_trip(hip_ctx):
    """16 crops of 64 x 128 -> compvhip_plan_hog -> compvhip_svm_predict(F32) on the device buffer, descStride > descLen; equal to the model run on the
    downloaded descriptors"""
    import torch
    from compv_amd import capi
    c = BY_ID["hand_d3780"]
    m = sc.recorded_model(c)
    W, H, F = 64, 128, 16
    assert capi.hog_geometry(W, H)["descLen"] == m.dim == 3780
    stride = 3780 + 4
    rng = np.random.RandomState(3)
    ramp = (np.arange(W)[None, :] * 3 + np.arange(H)[:, None] * 2) % 256
    gray = np.stack([((ramp * (f + 1)) % 256 + rng.randint(0, 64, (H, W))) % 256 for f in range(F)]).astype(np.uint8)
    ar = Arena()
    d_gray = ar.new(gray.size, u8(gray))
    ar.keep(d_gray, u8(gray))
    d_desc = ar.new(F * stride * 4)
    d_desc.copy_(torch.from_numpy(u8(np.full(F * stride, PAD, np.float32)).copy()))          # the padding columns hold the finite sentinel
    d_lab, d_dec, d_k = ar.new(F * 4), ar.new(F * 8), ar.new(F * m.l * 8)
    plan = capi.Plan(hip_ctx, W, H, W, F)
    svm = capi.Svm(hip_ctx, sc.model_path(c["id"]), F)
    try:
        plan.hog(ptr(d_gray), ptr(d_desc), stride)
        svm.predict(ptr(d_desc), capi.SVM_F32, F, stride, ptr(d_lab), ptr(d_dec), ptr(d_k))
        ar.check("hog -> svm")
        desc = np.frombuffer(d_desc.cpu().numpy().tobytes(), np.float32).reshape(F, stride)
        assert (desc[:, 3780:] == np.float32(PAD)).all() and np.isfinite(desc[:, :3780]).all() and desc[:, :3780].any()
        labels, dec, K = sm.predict(m, desc[:, :3780])
        assert np.frombuffer(d_k.cpu().numpy().tobytes(), np.float64).reshape(F, m.l).tobytes() == K.tobytes()
        assert np.frombuffer(d_dec.cpu().numpy().tobytes(), np.float64).reshape(F, 1).tobytes() == dec.tobytes()
        assert np.frombuffer(d_lab.cpu().numpy().tobytes(), np.int32).tobytes() == labels.tobytes()
        assert len({k.tobytes() for k in K}) > 1          # the crops differ, and so do their kernel values
    finally:
        svm.close()
        plan.close()
