"""GPU tests of the PCA projection (include/compv_hip.h, "PCA projection"; docs/kernels/pca.md): compvhip_pca_project, compvhip_mulabt_f32,
compvhip_pca_covariance and compvhip_pca_project_host against the fixture of the compiled reference and tests/pca_model.py (which the fixture generator
holds against the reference), BIT FOR BIT, with sentinels behind `components`, behind row n and in every padding.

Shapes: the smallest at which the kernels can go wrong.  pca_project_kernel owns 32 rows x 32 components and stages 64 columns at a time: n and M at 31,
32, 33; D at 63, 64, 65 and 127, 128, 129 (one and two chunks, a whole group of 16 less, a tail of one); every D of the fixture (1 .. 33 around the groups of
4 and 16, 441, 3780); input paddings hold NaNs, so a read behind `dim` would show in the result."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pca_cases as pc
import pca_fixture as pf
import pca_model as pm
from gpu_support import SENTINEL, Arena, alloc_fill, ptr, u8

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_PAD = np.frombuffer(np.uint32(0x7FC00A5A).tobytes(), np.float32)[0]


def capi_():
    from compv_amd import capi
    return capi


def kernel_constant(name):
    txt = open(os.path.join(ROOT, "compv_amd", "csrc", "kernels.hpp")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, txt).group(1))


def same(a, b):
    return np.shape(a) == np.shape(b) and pm.bits(a).tobytes() == pm.bits(b).tobytes()


def padded(a, stride):
    """(r, c) float32 -> (r, stride) whose padding holds NaNs"""
    out = np.full((a.shape[0], stride), NAN_PAD, np.float32)
    out[:, :a.shape[1]] = a
    return out


class Rig:
    """rows, mean and vectors on the device at the given strides, an output of n + 2 rows full of sentinels"""

    def __init__(self, x, mean, vectors, in_stride=None, vec_stride=None, out_stride=None, arena=None):
        self.ar = arena or Arena()
        self.n, self.D = x.shape
        self.M = vectors.shape[0]
        self.in_stride, self.vec_stride, self.out_stride = in_stride or self.D, vec_stride or self.D, out_stride or self.M
        self.d_in = self.host(padded(x, self.in_stride))
        self.d_vec = self.host(padded(vectors, self.vec_stride))
        self.d_mean = None if mean is None else self.host(np.ascontiguousarray(mean, np.float32))
        self.d_out = self.ar.new((self.n + 2) * self.out_stride * 4)

    def host(self, a):
        b = u8(a).copy()          # (a fixture array is read-only; torch wants a writable one)
        d = self.ar.new(b.size, b)
        self.ar.keep(d, b)
        return d

    def run(self, ctx, stream=0):
        ctx.pca_project_raw(ptr(self.d_mean) if self.d_mean is not None else 0, ptr(self.d_vec), self.vec_stride, self.D, self.M, ptr(self.d_in), self.n, self.in_stride,
                            ptr(self.d_out), self.out_stride, stream=stream)

    def result(self, what):
        """the (n, M) outputs, after checking every guard, every input and every sentinel behind components and behind row n"""
        self.ar.check(what)
        raw = self.d_out.cpu().numpy().reshape(self.n + 2, self.out_stride * 4)
        assert (raw[self.n:] == SENTINEL).all(), "%s: a row behind n was written" % what
        assert (raw[:self.n, self.M * 4:] == SENTINEL).all(), "%s: an element behind components was written" % what
        return np.ascontiguousarray(raw[:self.n, :self.M * 4]).view(np.float32)


def project(ctx, x, mean, vectors, what, **strides):
    rig = Rig(x, mean, vectors, **strides)
    rig.run(ctx)
    return rig.result(what)


@pytest.mark.parametrize("cid", [r["id"] for r in pf.project_cases()])
def test_fixture_cases(hip_ctx, cid):
    """with the mean at padded strides, without it at tight ones; the second run of the same call gives the same bits"""
    rec = next(r for r in pf.project_cases() if r["id"] == cid)
    mean, vectors, _ = pf.model(rec["model"])
    x = pf.case_rows(cid)
    D, M = rec["dim"], rec["components"]
    rig = Rig(x, mean, vectors, in_stride=D + 3, vec_stride=D + 5, out_stride=M + 2)
    rig.run(hip_ctx)
    first = rig.result(cid)
    assert same(first, pf.expected(cid)), "%s: %d of %d outputs differ from the reference" % (cid, int((pm.bits(first) != pm.bits(pf.expected(cid))).sum()), first.size)
    rig.run(hip_ctx)
    assert same(rig.result(cid + " again"), first)
    assert same(project(hip_ctx, x, None, vectors, cid + " without a mean"), pf.expected_raw(cid))
    assert same(project(hip_ctx, x, mean, vectors, cid + " tight"), pf.expected(cid))


def test_mulabt_and_the_denormal_case(hip_ctx):
    _, arrays = pf.golden()
    for a_rows, b_rows, cols in pc.mulabt_cases():
        A, B = pc.mulabt_inputs(a_rows, b_rows, cols)
        ar = Arena()
        dA, dB = ar.new(A.nbytes + 8 * a_rows, u8(padded(A, cols + 2))), ar.new(B.nbytes + 4 * b_rows, u8(padded(B, cols + 1)))
        dR = ar.new((a_rows + 1) * (b_rows + 3) * 4)
        hip_ctx.mulabt(ptr(dA), a_rows, cols + 2, ptr(dB), b_rows, cols + 1, cols, ptr(dR), b_rows + 3)
        ar.check("mulabt")
        raw = dR.cpu().numpy().reshape(a_rows + 1, (b_rows + 3) * 4)
        assert (raw[a_rows:] == SENTINEL).all() and (raw[:, b_rows * 4:] == SENTINEL).all()
        assert same(np.ascontiguousarray(raw[:a_rows, :b_rows * 4]).view(np.float32), arrays["mulabt_%d_%d_%d" % (a_rows, b_rows, cols)]), (a_rows, b_rows, cols)
    x, v = pc.denormal_case()
    got = project(hip_ctx, x, None, v, "denormal", in_stride=40, vec_stride=37, out_stride=4)
    exp = arrays["raw_" + pc.DENORMAL]
    assert same(got, exp) and ((got != 0) & (np.abs(got) < pm.TINY)).any()


def test_tile_edges(hip_ctx):
    """n and M one below, at and one above the tile; D one below, at and one above the chunk and twice the chunk"""
    tile, chunk = kernel_constant("kPcaTile"), kernel_constant("kPcaChunk")
    assert (tile, chunk) == (32, 64)
    x_all, v_all, mean_all = pc.rows(tile + 1, 2 * chunk + 1, 31), pc.rows(tile + 1, 2 * chunk + 1, 32), pc.rows(1, 2 * chunk + 1, 33)[0]
    for D in (chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk, 2 * chunk + 1):
        exp = pm.project(x_all[:, :D], mean_all[:D], v_all[:, :D])          # once per D; the smaller tiles are its corners
        for n in (tile - 1, tile, tile + 1):
            for M in (tile - 1, tile, tile + 1):
                got = project(hip_ctx, np.ascontiguousarray(x_all[:n, :D]), mean_all[:D], np.ascontiguousarray(v_all[:M, :D]), "edges", in_stride=D + 1, out_stride=M + 1)
                assert same(got, exp[:n, :M]), (n, M, D)
    # two tiles of rows and of components and a ragged third
    x, v = pc.rows(2 * tile + 5, 70, 34), pc.rows(2 * tile + 3, 70, 35)
    assert same(project(hip_ctx, x, None, v, "three tiles"), pm.project(x, None, v))


@pytest.mark.parametrize("n,D", pc.COVARIANCE)
def test_covariance(hip_ctx, n, D):
    """mean and covariance bit for bit; symmetric on every bit; the padding of the scratch is neither written nor read"""
    capi = capi_()
    obs, mean, cov = pf.covariance_case(n, D)
    n_pad = (n + 15) // 16 * 16
    assert capi.pca_covariance_scratch(n, D) == D * n_pad * 4
    results = []
    for poison in (SENTINEL, 0x7F):          # 0x7F7F7F7F is a large finite float, 0xA5A5A5A5 a small negative one: either would move a sum
        ar = Arena()
        d_obs = ar.new((D + 2) * n * 4, u8(padded(obs, D + 2)))
        ar.keep(d_obs, u8(padded(obs, D + 2)))
        d_mean, d_cov, d_scratch = ar.new((D + 1) * 4), ar.new((D + 1) * (D + 3) * 4), ar.new(D * n_pad * 4, poison)
        hip_ctx.pca_covariance(ptr(d_obs), n, D + 2, D, ptr(d_mean), ptr(d_cov), D + 3, ptr(d_scratch))
        ar.check("covariance")
        m = d_mean.cpu().numpy()
        assert (m[D * 4:] == SENTINEL).all() and same(m[:D * 4].view(np.float32), mean)
        raw = d_cov.cpu().numpy().reshape(D + 1, (D + 3) * 4)
        assert (raw[D:] == SENTINEL).all() and (raw[:, D * 4:] == SENTINEL).all()
        got = np.ascontiguousarray(raw[:D, :D * 4]).view(np.float32)
        assert same(got, cov) and same(got, got.T), (n, D)
        scratch = d_scratch.cpu().numpy().reshape(D, n_pad * 4)
        assert (scratch[:, n * 4:] == poison).all(), "the padding of the scratch was written"
        assert same(np.ascontiguousarray(scratch[:, :n * 4]).view(np.float32), (obs - mean[None, :]).T)
        results.append(got)
    assert same(results[0], results[1])


def test_host_form_equals_the_device_call(hip_ctx):
    capi = capi_()
    mean, vectors, _ = pf.model("pca_trained_d20_m8")
    model = capi.PcaModel(mean, vectors)
    x_all = pc.rows(1100, 20, 61)
    exp = pm.project(x_all, mean, vectors)
    for n in (1, 512, 513, 1100):
        wide = padded(x_all[:n], 23)
        got = hip_ctx.pca_project_host(model, wide[:, :20])          # a strided host array
        assert same(got, exp[:n]), n
        assert same(project(hip_ctx, x_all[:n], mean, vectors, "device"), got), n
    assert same(hip_ctx.pca_project_host(model, x_all[:70], centre=False), pm.project(x_all[:70], None, vectors))
    assert hip_ctx.pca_project_host(model, x_all[:0]).shape == (0, 8)


def test_hog_to_pca_to_svm_without_a_host_trip(hip_ctx, tmp_path):
    """compvhip_plan_hog on two 64 x 128 crops -> compvhip_pca_project (the composed D = 3780, M = 8 model) -> compvhip_svm_predict (RBF, dim 8): labels,
    decision values and projected vectors equal the numpy models run on the downloaded descriptors"""
    import hog_cases as hc
    import svm_cases as sc
    import svm_model as sm
    capi = capi_()
    W, H, S, F = 64, 128, 64, 2
    name = pc.hand_name(3780, 8)
    mean, vectors, _ = pf.model(name)
    pca = capi.PcaModel(mean * np.float32(0.01), vectors).to_device()          # (descriptor values lie in [0, 1])
    assert capi.hog_geometry(W, H)["descLen"] == pca.dim
    rng = np.random.RandomState(5)
    path = str(tmp_path / "chain.model")
    sm.write_model_file(path, sm.RBF, "0.05", sc._text(rng.uniform(-3.0, 3.0, (7, 8)), 8), sc._text(rng.uniform(-2.0, 2.0, (2, 7)), 16), ["0.1", "-0.2", "0.05"], [2, 3, 2], [4, -1, 9])
    svm_np = sm.parse(path)
    frames = np.stack([hc.noise(W, H, 21), hc.blocks(W, H, 22)])
    ar = Arena()
    d_gray = ar.new(frames.size, u8(frames))
    d_desc, d_proj = ar.new(F * (3780 + 4) * 4), ar.new(F * 9 * 4)
    d_labels, d_dec = ar.new(F * 4), ar.new(F * 3 * 8)
    plan, svm = capi.Plan(hip_ctx, W, H, S, F), capi.Svm(hip_ctx, path, F)
    try:
        plan.hog(ptr(d_gray), ptr(d_desc), 3784)
        hip_ctx.pca_project(pca, ptr(d_desc), F, 3784, ptr(d_proj), 9)
        svm.predict(ptr(d_proj), capi.SVM_F32, F, 9, ptr(d_labels), ptr(d_dec))
        ar.check("chain")
        desc = np.ascontiguousarray(d_desc.cpu().numpy().view(np.float32).reshape(F, 3784)[:, :3780])
        proj = np.ascontiguousarray(d_proj.cpu().numpy().view(np.float32).reshape(F, 9)[:, :8])
        exp_proj = pm.project(desc, pca.mean, vectors)
        assert desc.any() and same(proj, exp_proj)
        labels, dec, _ = sm.predict(svm_np, exp_proj)
        assert d_labels.cpu().numpy().view(np.int32).tolist() == labels.tolist()
        assert d_dec.cpu().numpy().view(np.float64).reshape(F, 3).tobytes() == dec.tobytes()
    finally:
        plan.close()
        svm.close()


@pytest.mark.parametrize("fill", (0xFF, 0x01))
def test_first_use_on_poisoned_allocations(fill):
    """the first calls of a fresh context, whose staging is allocated inside the fill: the host form (it allocates), the device calls (they do not)"""
    capi = capi_()
    mean, vectors, _ = pf.model("pca_trained_d67_m12")
    x = pf.case_rows("pca_trained_d67_m12_n65")
    exp = pf.expected("pca_trained_d67_m12_n65")
    n, D = pc.COVARIANCE[2]
    obs, cmean, cov = pf.covariance_case(n, D)
    with alloc_fill(fill):
        ctx = capi.Context(0)
        try:
            assert same(ctx.pca_project_host(capi.PcaModel(mean, vectors), x), exp)
            assert same(project(ctx, x, mean, vectors, "cold"), exp)
            ar = Arena()
            d_obs, d_mean, d_cov, d_scratch = ar.new(obs.nbytes, u8(obs).copy()), ar.new(D * 4), ar.new(D * D * 4), ar.new(capi.pca_covariance_scratch(n, D), fill)
            ctx.pca_covariance(ptr(d_obs), n, D, D, ptr(d_mean), ptr(d_cov), D, ptr(d_scratch))
            ar.check("cold covariance")
            assert same(d_cov.cpu().numpy().view(np.float32).reshape(D, D), cov) and same(d_mean.cpu().numpy().view(np.float32), cmean)
        finally:
            ctx.close()


def test_behind_pending_work_on_a_side_stream(hip_ctx):
    """the rows reach the device on a side stream behind a delay; the calls follow on it (the descriptor's stream) and return at once"""
    import torch
    side = torch.cuda.Stream()
    cid = "pca_trained_d130_m10_n65"
    mean, vectors, _ = pf.model("pca_trained_d130_m10")
    x = pf.case_rows(cid)
    rig = Rig(x, mean, vectors, in_stride=133)
    n, D = pc.COVARIANCE[3]
    obs, cmean, cov = pf.covariance_case(n, D)
    d_obs, d_mean, d_cov, d_scratch = rig.ar.new(obs.nbytes, 0), rig.ar.new(D * 4), rig.ar.new(D * D * 4), rig.ar.new(capi_().pca_covariance_scratch(n, D))
    host, obs_host = torch.from_numpy(u8(padded(x, 133)).copy()).pin_memory(), torch.from_numpy(u8(obs).copy()).pin_memory()
    rig.d_in.fill_(0)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)          # a few milliseconds of pending work in front of the copies
        rig.d_in.copy_(host, non_blocking=True)
        d_obs.copy_(obs_host, non_blocking=True)
    rig.run(hip_ctx, stream=side.cuda_stream)
    hip_ctx.pca_covariance(ptr(d_obs), n, D, D, ptr(d_mean), ptr(d_cov), D, ptr(d_scratch), stream=side.cuda_stream)
    side.synchronize()
    assert same(rig.result("behind pending work"), pf.expected(cid))
    assert same(d_cov.cpu().numpy().view(np.float32).reshape(D, D), cov) and same(d_mean.cpu().numpy().view(np.float32), cmean)


def test_refusals_write_nothing(hip_ctx):
    capi = capi_()
    lib, E = hip_ctx.lib, capi.E_INVALID_PARAMETER
    D, M, n = 20, 8, 5
    ar = Arena()
    d_mean, d_vec, d_in, d_out = ar.new(D * 4 + 8), ar.new(M * D * 4 + 8), ar.new(n * D * 4 + 8), ar.new(n * M * 4 + 8)
    d_cov, d_scratch = ar.new(D * D * 4 + 8), ar.new(capi.pca_covariance_scratch(n, D) + 16)
    desc = capi.PcaDesc()
    d = C.byref(desc)

    def proj(desc_=d, mean=ptr(d_mean), vec=ptr(d_vec), vs=D, dim=D, comps=M, inp=ptr(d_in), rows=n, ins=D, out=ptr(d_out), outs=M):
        return lib.compvhip_pca_project(hip_ctx.h, desc_, mean, vec, vs, dim, comps, inp, rows, ins, out, outs)

    def cov(obs=ptr(d_in), rows=n, stride=D, dim=D, mean=ptr(d_mean), covar=ptr(d_cov), cs=D, scratch=ptr(d_scratch)):
        return lib.compvhip_pca_covariance(hip_ctx.h, d, obs, rows, stride, dim, mean, covar, cs, scratch)
    wrong = capi.PcaDesc()
    wrong.size = 12
    refused = [proj(desc_=None), proj(desc_=C.byref(wrong)), proj(vec=None), proj(inp=None), proj(out=None), proj(vs=D - 1), proj(ins=D - 1), proj(outs=M - 1),
               proj(dim=0), proj(dim=2 ** 20 + 1, vs=2 ** 20 + 1, ins=2 ** 20 + 1), proj(comps=0), proj(comps=65536, outs=65536), proj(rows=2 ** 31), proj(rows=2 ** 21, ins=2 ** 19),
               cov(obs=None), cov(mean=None), cov(covar=None), cov(scratch=None), cov(rows=0), cov(stride=D - 1), cov(cs=D - 1), cov(dim=0), cov(dim=2 ** 20 + 1),
               cov(scratch=ptr(d_scratch) + 4), cov(scratch=ptr(d_scratch) + 8)]
    for move in (1, 2):
        refused += [proj(mean=ptr(d_mean) + move), proj(vec=ptr(d_vec) + move), proj(inp=ptr(d_in) + move), proj(out=ptr(d_out) + move),
                    cov(obs=ptr(d_in) + move), cov(mean=ptr(d_mean) + move), cov(covar=ptr(d_cov) + move), cov(scratch=ptr(d_scratch) + move),
                    lib.compvhip_mulabt_f32(hip_ctx.h, d, ptr(d_in) + move, n, D, ptr(d_vec), M, D, D, ptr(d_out), M),
                    lib.compvhip_mulabt_f32(hip_ctx.h, d, ptr(d_in), n, D, ptr(d_vec), M, D, D, ptr(d_out) + move, M)]
    refused += [lib.compvhip_mulabt_f32(hip_ctx.h, d, ptr(d_in), 2 ** 20 + 1, D, ptr(d_vec), M, D, D, ptr(d_out), M),
                lib.compvhip_mulabt_f32(hip_ctx.h, d, ptr(d_in), n, D, ptr(d_vec), 0, D, D, ptr(d_out), M)]
    assert refused == [E] * len(refused), refused
    ar.check("refusals")
    for buf in (d_mean, d_vec, d_in, d_out, d_cov, d_scratch):
        assert (buf.cpu().numpy() == SENTINEL).all(), "a refused call wrote"
    assert "pca" in hip_ctx.last_error() or "mulabt" in hip_ctx.last_error()
    # n == 0: success, nothing enqueued, nothing written; a mean of NULL is served
    assert proj(rows=0) == capi.OK and lib.compvhip_mulabt_f32(hip_ctx.h, d, None, 0, D, ptr(d_vec), M, D, D, None, M) == capi.OK
    ar.check("n == 0")
    assert (d_out.cpu().numpy() == SENTINEL).all()
    assert proj(mean=None) == capi.OK
    ar.check("served")


def test_70000_rows(hip_ctx):
    """n = 70 000 rows of D = 5, M = 2: 2188 row tiles in grid x (rows ride in x, where no launch needs slicing)"""
    mean, vectors, _ = pf.model("pca_trained_d5_m2")
    x = pc.rows(70000, 5, 71)
    got = project(hip_ctx, x, mean, vectors, "70000 rows", in_stride=6, out_stride=3)
    exp = pm.project(x, mean, vectors)
    assert same(got, exp), "%d outputs differ, first row %d" % (int((pm.bits(got) != pm.bits(exp)).sum()), int(np.nonzero((pm.bits(got) != pm.bits(exp)).any(axis=1))[0][0]))
