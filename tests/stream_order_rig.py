"""Stream order: every asynchronous call behind pending work (include/compv_hip.h, "Stream order"; the contract table is tests/stream_cases.py, the
coverage table docs/dispatch_coverage.md, "Stream order").

The other stream tests make their call on an idle stream whose inputs were finished long before, where a launch on ANY stream gives the same bits.  Here every
call is queued behind a bounded device delay (torch.cuda._sleep, calibrated once) on a non-blocking torch stream, so that nothing the call needs exists yet
when it returns:

  warm-up   with a decoy content D in the input buffer the call runs on the idle stream; every first-use scratch now exists and holds D's state;
  queue     stall, event, copy X1 -> input, call -> outputs 1, copy X2 -> the SAME input, call (another scalar parameter) -> outputs 2, copy D -> input,
            with no host synchronisation in between; as soon as a call has returned its host arrays and option structs are overwritten with other valid
            values, and for an ASYNC row the event behind the stall must still be pending;
  check     after one stream synchronisation: outputs 1 == f(X1), outputs 2 == f(X2) bit for bit on all frames (f = the model or oracle of the stage's own
            GPU test), the input holds D, the 64-byte sentinel bands around every buffer are intact, compvhip_live_allocations is what it was.

f(D), f(X1) and f(X2) are asserted to differ in every output array before anything is launched: a launch or copy on another stream reads D or D-derived
scratch and shows.  Two calls behind one stall expose a per-call clear on another stream (it would run before call 1 accumulates), the shared input buffer an
order missing between call 1's reads and the next producer, the final copy and the bands a fork that never joins back.

run_cold() is the same queue WITHOUT the warm-up and the stall, for tests/test_gpu_fresh_memory.py: the handle of a case and everything its first use
allocates are blocks filled with a poison byte (gpu_support.alloc_fill), and the first two calls must give f(X1) and f(X2).

STALL_MS is a harness constant, not a tolerance: 50 x the slowest warm enqueue section (docs/dispatch_coverage.md holds the measurements).  An ASYNC case
whose enqueue section takes more than a quarter of it fails with "stall too short", and the event pair around the stall must show at least half of it."""
import ctypes as C
import functools
import time
from types import SimpleNamespace

import numpy as np

import stream_cases as sc
from gpu_support import BAND, COMP_BYTES, FIT_BYTES, SEG_BYTES, SENTINEL, u8

STALL_MS = 85.0          # 50 x the slowest warm enqueue section, rounded up (docs/dispatch_coverage.md, "Stream order")
F = 3
G = (43, 49, 48)          # W, H, S: the first geometry of tests/test_gpu_pointer_alignment.py
THETA = 1.0
SEEDS = (10, 13, 14)      # X1, X2, D: gpu_support.make_batch seeds -- (synth, noise, zero), (text, checker, synth), (checker, synth, noise)
LINE_CAP = 2048
MAX_LINES = 12

CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


# ---- the stall --------------------------------------------------------------------------------------------------------------------------------
class Stall:
    """a bounded device delay on a non-blocking torch stream"""

    def __init__(self):
        import torch
        from compv_amd import capi
        self.torch = torch
        self.stream = torch.cuda.Stream()
        L = capi.load()
        L.hipStreamGetFlags.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
        flags = C.c_uint(99)
        rc = L.hipStreamGetFlags(C.c_void_p(self.stream.cuda_stream), C.byref(flags))
        assert rc == 0, "hipStreamGetFlags returned %d, expected 0" % rc
        assert flags.value & 1, "the test stream must be hipStreamNonBlocking: the legacy default stream would order everything this test looks for"
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):          # cycles of torch.cuda._sleep per millisecond, once
            torch.cuda._sleep(1 << 20)
            self.stream.synchronize()
            n = 1 << 24
            self.e0.record()
            torch.cuda._sleep(n)
            self.e1.record()
            self.stream.synchronize()
        ms = self.e0.elapsed_time(self.e1)
        assert ms > 0.05, ms
        self.cycles = int(n / ms * STALL_MS)

    def enqueue(self):
        """stall + event on the stream; returns the host time"""
        with self.torch.cuda.stream(self.stream):
            self.e0.record()
            self.torch.cuda._sleep(self.cycles)
            self.e1.record()
        return time.perf_counter()

    def pending(self):
        return not self.e1.query()

    def finish(self, what):
        self.stream.synchronize()
        ms = self.e0.elapsed_time(self.e1)
        assert ms >= STALL_MS / 2, "%s: the stall lasted %.1f ms of the intended %.0f" % (what, ms, STALL_MS)


# ---- buffers ------------------------------------------------------------------------------------------------------------------------------------
class Env:
    def __init__(self, ctx, oracle):
        import torch
        self.torch, self.ctx, self.orc = torch, ctx, oracle
        self.dev = torch.device("cuda:0")
        self.bufs, self.handles = [], []

    def buf(self, nbytes, fill=None):
        """a device buffer between two 64-byte sentinel bands"""
        tail = BAND + (-nbytes) % 16
        raw = self.torch.full((BAND + nbytes + tail,), SENTINEL, dtype=self.torch.uint8, device=self.dev)
        body = raw[BAND:BAND + nbytes]
        if fill is not None:
            body.copy_(self.torch.from_numpy(u8(fill)))
        self.bufs.append((raw, nbytes))
        return body

    def stage(self, host):
        return self.torch.from_numpy(u8(host).copy()).to(self.dev)

    def bands(self, what):
        for raw, n in self.bufs:
            assert bool((raw[:BAND] == SENTINEL).all()) and bool((raw[BAND + n:] == SENTINEL).all()), "%s: a sentinel band was written" % what

    def own(self, h):
        self.handles.append(h)
        return h

    def plan(self, g=G, frames=F):
        from compv_amd import capi
        return self.own(capi.Plan(self.ctx, g[0], g[1], g[2], frames, THETA))

    def close(self):
        for h in reversed(self.handles):
            h.close()


def ptrs(d):
    return {k: v.data_ptr() for k, v in d.items()}


def differs(a, b):
    (ia, ma), (ib, mb) = a, b
    return ia.size != ib.size or bool((ma != mb).any()) or bool((ia[ma] != ib[mb]).any())


# ---- the rig -------------------------------------------------------------------------------------------------------------------------------------
def spec(inputs, outputs, call, expect, **kw):
    """inputs: name -> [X1, X2, D] host arrays; outputs: name -> bytes (or one such dict per call); call(k, I, O, stream) with k = 0, 1 (the queued calls)
    or 2 (the warm-up on D), I / O: name -> device address; expect(k) -> name -> (image, mask) of the whole buffer: the sentinel where the call must not write,
    mask False where it may write anything.  Options: scribble() overwrites the host arrays of the row; own_inputs: one input buffer per call, never
    rewritten (a ticketed step, an in-place call: alias maps an output name to the input it shares); finish(): host waits that belong to the case, made
    behind the return checks; growth: call 1 makes the handle reallocate, so it may block and the allocation count may rise; drains: a fresh stall in front
    of each call, no return check; check_host(k, result); after(env): assertions behind the synchronisation; cls: the class this case is checked as where it
    is not the row's (the ticketed form of a call whose plain form waits)"""
    return SimpleNamespace(inputs=inputs, outputs=outputs, call=call, expect=expect, scribble=kw.pop("scribble", None), own_inputs=kw.pop("own_inputs", False),
                           alias=kw.pop("alias", {}), finish=kw.pop("finish", None), growth=kw.pop("growth", False), drains=kw.pop("drains", False),
                           check_host=kw.pop("check_host", None), after=kw.pop("after", None), cls=kw.pop("cls", None), **kw)


def compare(got, exp, others, what):
    img, mask = exp
    assert got.size == img.size, what
    bad = (got != img) & mask
    if bad.any():
        like = [name for name, (oi, om) in others.items() if not ((got != oi) & om).any()]
        raise AssertionError("%s: %d of %d bytes differ, first at %d (got %d, expected %d)%s"
                             % (what, int(bad.sum()), img.size, int(np.flatnonzero(bad)[0]), got[bad][0], img[bad][0], "; it equals " + " and ".join(like) if like else ""))


def buffers(env, cid, s):
    """the staged contents, the banded input and output buffers (the outputs hold the sentinel) and the expectations of a case"""
    names = list(s.inputs)
    stage = {n: [env.stage(a) for a in s.inputs[n]] for n in names}
    sets = 2 if s.own_inputs else 1
    I = [{n: env.buf(stage[n][0].numel()) for n in names} for _ in range(sets)]
    outs = s.outputs if isinstance(s.outputs, list) else [s.outputs, s.outputs]
    O = [{n: (I[k][s.alias[n]] if n in s.alias else env.buf(size)) for n, size in outs[k].items()} for k in range(2)]
    exp = [s.expect(k) for k in range(3)]
    for n in exp[0]:          # f(D), f(X1), f(X2) differ in every output array, before anything is launched
        for a, b in ((0, 1), (0, 2), (1, 2)):
            assert differs(exp[a][n], exp[b][n]), "%s: %s is the same for contents %d and %d: the rig could not tell them apart" % (cid, n, a, b)
    return names, stage, I, O, exp


def check_outputs(cid, s, O, exp, results):
    """outputs 1 == f(X1), outputs 2 == f(X2) bit for bit, and what the calls returned to the host"""
    named = {"f(D)": 2, "f(X1)": 0, "f(X2)": 1}
    for k in range(2):
        for n in exp[k]:
            got = O[k][n].cpu().numpy()
            others = {name: exp[j][n] for name, j in named.items() if j != k}
            compare(got, exp[k][n], others, "%s: %s of call %d" % (cid, n, k + 1))
        if s.check_host:
            s.check_host(k, results[k])


def run_cold(env, stream, cid, s):
    """The FIRST calls of a handle, for tests/test_gpu_fresh_memory.py: `s` was made by CASES[cid](env) inside gpu_support.alloc_fill, and this runs inside
    the same block, so the handle and every scratch buffer its first use allocates are fresh blocks filled with the poison byte.  No warm-up, no stall:
    X1 -> input, call 0 into sentinel-filled outputs, X2 -> input, call 1 (the growth cases reallocate there, into a second filled block), all on the
    non-blocking `stream`; after one synchronisation outputs 1 == f(X1) and outputs 2 == f(X2) bit for bit and the bands are intact.  No return-time
    and no allocation-count assertion: first use allocates, and an allocation under fill waits for the device."""
    torch = env.torch
    if hasattr(s, "custom"):
        s.custom(env, None, cold=stream)
        return
    names, stage, I, O, exp = buffers(env, cid, s)
    torch.cuda.synchronize()
    results = []
    for k in range(2):
        i = I[k if s.own_inputs else 0]
        with torch.cuda.stream(stream):
            for n in names:
                i[n].copy_(stage[n][k], non_blocking=True)
        results.append(s.call(k, ptrs(i), ptrs(O[k]), stream.cuda_stream))
        if s.scribble:
            s.scribble()
    if s.finish:
        s.finish()
    torch.cuda.synchronize()
    check_outputs(cid, s, O, exp, results)
    env.bands(cid)
    if s.after:
        s.after(env)


def run(env, stall, cid, s, stalled=True):
    """stalled=False: the same queue on an IDLE stream, without the return checks -- tools/stream_enqueue_times.py measures with it what STALL_MS is derived
    from, so that what is measured and what is tested is one piece of code.  Returns the host time of the enqueue section."""
    torch, st = env.torch, stall.stream
    cls = s.cls or sc.CASE_ROW[cid].cls
    begin = stall.enqueue if stalled else time.perf_counter
    names, stage, I, O, exp = buffers(env, cid, s)
    # warm-up on D, idle stream
    for i in I:
        for n in names:
            i[n].copy_(stage[n][2])
    torch.cuda.synchronize()
    s.call(2, ptrs(I[0]), ptrs(O[0]), st.cuda_stream)
    if s.finish:
        s.finish()
    torch.cuda.synchronize()
    for k in range(2):
        for n, b in O[k].items():
            if n in s.alias:
                b.copy_(stage[s.alias[n]][2])
            else:
                b.fill_(SENTINEL)
    torch.cuda.synchronize()
    live = env.ctx.live_allocations()
    results, spent = [], 0.0
    if not s.drains:
        t0 = begin()
    for k in range(2):
        if s.drains:
            t0 = begin()
        i = I[k if s.own_inputs else 0]
        with torch.cuda.stream(st):
            for n in names:
                i[n].copy_(stage[n][k], non_blocking=True)
        t1 = time.perf_counter()
        results.append(s.call(k, ptrs(i), ptrs(O[k]), st.cuda_stream))
        t2 = time.perf_counter()
        if s.scribble:
            s.scribble()
        if stalled and cls == sc.ASYNC and not (s.growth and k == 1):
            assert stall.pending(), ("%s: call %d returned only after the stall had ended: an ASYNC call that waits for the stream (the call took %.2f ms, %.2f ms "
                                     "have passed since the stall was enqueued, stall %.0f ms)" % (cid, k + 1, (t2 - t1) * 1e3, (t2 - t0) * 1e3, STALL_MS))
        spent = time.perf_counter() - t0
    if not s.own_inputs:
        with torch.cuda.stream(st):
            for n in names:
                I[0][n].copy_(stage[n][2], non_blocking=True)
        spent = time.perf_counter() - t0
    if stalled and cls == sc.ASYNC and not s.growth:
        assert spent * 1e3 <= STALL_MS / 4, "%s: stall too short: the enqueue section took %.2f ms of a stall of %.0f ms" % (cid, spent * 1e3, STALL_MS)
    if s.finish:
        s.finish()
    if stalled:
        stall.finish(cid)
    torch.cuda.synchronize()
    check_outputs(cid, s, O, exp, results)
    if not s.own_inputs:
        for n in names:
            assert torch.equal(I[0][n], stage[n][2]), "%s: the last copy into %s did not land behind the calls" % (cid, n)
    env.bands(cid)
    if s.after:
        s.after(env)
    if not s.growth:
        assert env.ctx.live_allocations() == live, "%s: %d allocations, %d after the warm-up" % (cid, env.ctx.live_allocations(), live)
    return spent


# ---- content and expectations ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def content(k):
    from gpu_support import make_batch
    out = make_batch(G[0], G[1], F, SEEDS[k])
    out.setflags(write=False)
    return out


_FX = {}


def fx(orc, k):
    """per frame of content k: gpu_support.frame_expectations"""
    if k not in _FX:
        from compv_amd import capi
        from gpu_support import frame_expectations
        _FX[k] = [frame_expectations(orc, img, THETA, True, capi.gauss_kernel_fixedpoint(5, 1.0)) for img in content(k)]
    return _FX[k]


def thr0():
    from gpu_support import sht_threshold
    return sht_threshold(G[0], G[1])


def padded(valid, row_bytes, seed):
    from gpu_support import pad_frames
    return pad_frames(np.ascontiguousarray(valid), row_bytes, np.random.default_rng(seed)).reshape(-1)


def frames_in(valids, bpp=1, S=None):
    """[X1, X2, D] -> three padded batches"""
    S = G[2] if S is None else S
    return [padded(v, S * bpp, 7 + k) for k, v in enumerate(valids)]


def edges_in(maps):
    W, H, S = G
    host = np.full((F, H, S), 255, np.uint8)          # 255 in the padding: columns >= W are never edges
    host[:, :, :W] = np.stack(maps)
    return host.reshape(-1)


def maps_img(maps, strict=False, S=None, elem=1):
    """[F][H][S * elem bytes]: the maps in columns < W; strict: columns >= W keep the sentinel, otherwise they are nobody's business"""
    maps = np.stack([np.ascontiguousarray(m) for m in maps])
    n, H, Wb = maps.shape[0], maps.shape[1], maps.shape[2] * maps.dtype.itemsize
    S = (G[2] if S is None else S) * elem
    img = np.full((n, H, S), SENTINEL, np.uint8)
    img[:, :, :Wb] = maps.view(np.uint8).reshape(n, H, Wb)
    mask = np.ones(img.shape, bool)
    if not strict:
        mask[:, :, Wb:] = False
    return img.reshape(-1), mask.reshape(-1)


def recs_img(per_frame, cap, rec, strict=True):
    """[F][cap] records of `rec` bytes: the first min(n, cap) of every frame, the sentinel behind them (strict) or anything"""
    img = np.full((len(per_frame), cap * rec), SENTINEL, np.uint8)
    mask = np.ones(img.shape, bool)
    for f, r in enumerate(per_frame):
        b = u8(r)[:cap * rec]
        img[f, :b.size] = b
        if not strict:
            mask[f, b.size:] = False
    return img.reshape(-1), mask.reshape(-1)


def full_img(a):
    b = u8(a).copy()
    return b, np.ones(b.size, bool)


def line_recs(lines):
    from compv_amd import capi
    out = np.zeros(len(lines), capi.LINE_DTYPE)
    for i, l in enumerate(lines):
        out[i] = (np.float32(l[0]), np.float32(l[1]), int(l[2]), int(l[3]), int(l[4]))
    return out


def lines_out(per_frame, cap=LINE_CAP):
    """d_lines / d_counts of an SHT: the first min(n, cap) records (the rest is not promised), the uncut totals"""
    assert all(len(l) <= cap for l in per_frame)
    return {"lines": recs_img([line_recs(l) for l in per_frame], cap, 20, strict=False), "counts": full_img(np.array([len(l) for l in per_frame], np.int32))}


def lines_in(per_frame, cap=LINE_CAP):
    from compv_amd import capi
    host = np.zeros((len(per_frame), cap), capi.LINE_DTYPE)
    for f, l in enumerate(per_frame):
        host[f, :len(l)] = line_recs(l)
    return u8(host), u8(np.array([len(l) for l in per_frame], np.int32))


def e3(orc, k):
    from compv_amd import capi
    return [x["canny"][(3, capi.THRESHOLD_COMPARE_TO_GRADIENT)] for x in fx(orc, k)]


def sht_lines(orc, k, thr):
    return [orc.sht_lines_from_acc(x["sht"][0], G[0], G[1], THETA, thr) for x in fx(orc, k)]


def cart_img(orc, per_frame, cap=LINE_CAP):
    out = []
    for l in per_frame:
        r = line_recs(l)
        out.append(np.ascontiguousarray(orc.sht_to_cartesian(G[0], G[1], [(float(a["rho"]), float(a["theta"])) for a in r]), np.float32) if len(l) else np.zeros((0, 4), np.float32))
    return recs_img(out, cap, 16, strict=False)


N_FRAMES = F * G[1] * G[2]
THR = (lambda k: thr0() + (0, 4, 0)[k])          # the SHT threshold of call k: another one for the second queued call


# ---- the Canny / SHT plan --------------------------------------------------------------------------------------------------------------------------
def _canny(env, in_place):
    from compv_amd import capi
    from gpu_support import canny_expect
    plan = env.plan()
    prm = ((59.0, 119.0), (40.0, 90.0), (59.0, 119.0))

    def call(k, I, O, st):
        plan.canny(I["in"], prm[k][0], prm[k][1], O["edges"], 3, capi.THRESHOLD_COMPARE_TO_GRADIENT, st)

    def expect(k):
        return {"edges": maps_img([canny_expect(env.orc, img, 3, capi.THRESHOLD_COMPARE_TO_GRADIENT, *prm[k]) for img in content(k)])}
    kw = dict(own_inputs=True, alias={"edges": "in"}) if in_place else {}
    return spec({"in": frames_in([content(k) for k in range(3)])}, {"edges": N_FRAMES}, call, expect, **kw)


@case
def canny(env):
    return _canny(env, False)


@case
def canny_in_place(env):
    """d_edges == d_in: through tmpOut and a device copy back"""
    return _canny(env, True)


@case
def grayscale(env):
    from compv_amd import capi
    from gpu_support import rgb_of
    plan = env.plan()
    W, H, S = G
    rgb = [np.stack([rgb_of(i).reshape(H, W * 3) for i in content(k)]) for k in range(3)]
    return spec({"in": frames_in(rgb, 3)}, {"gray": N_FRAMES}, lambda k, I, O, st: plan.grayscale(I["in"], capi.FMT_RGB24, O["gray"], st),
                lambda k: {"gray": maps_img([x["rgb"][0] for x in fx(env.orc, k)])})


@case
def otsu(env):
    plan = env.plan()
    return spec({"in": frames_in([content(k) for k in range(3)])}, {"levels": 4 * F}, lambda k, I, O, st: plan.otsu(I["in"], O["levels"], st),
                lambda k: {"levels": full_img(np.array([x["otsu_y"] for x in fx(env.orc, k)], np.int32))})


@case
def convlt1_fixedpoint(env):
    from compv_amd import capi
    plan = env.plan()
    kern = [capi.gauss_kernel_fixedpoint(5, s) for s in (1.0, 2.0, 1.0)]
    vt, hz = np.zeros(5, np.uint16), np.zeros(5, np.uint16)          # the host arrays the call reads: rewritten as soon as it has returned

    def call(k, I, O, st):
        vt[:], hz[:] = kern[k], kern[k]
        plan.convlt_fixedpoint(I["in"], vt, hz, O["out"], st)

    def scribble():
        vt[:], hz[:] = (13107, 13107, 13107, 13107, 13107), (0, 0, 65535, 0, 0)

    def expect(k):
        out = []
        for img in content(k):
            rc, o = env.orc.convlt_fxp(img, kern[k], kern[k])
            assert rc == 0, "oracle convlt_fxp returned %d, expected 0" % rc
            out.append(o)
        return {"out": maps_img(out)}
    return spec({"in": frames_in([content(k) for k in range(3)])}, {"out": N_FRAMES}, call, expect, scribble=scribble)


@case
def to_cartesian(env):
    plan = env.plan()
    lines = [sht_lines(env.orc, k, thr0()) for k in range(3)]
    host = [lines_in(l) for l in lines]
    return spec({"lines": [h[0] for h in host], "counts": [h[1] for h in host]}, {"cart": F * LINE_CAP * 16},
                lambda k, I, O, st: plan.to_cartesian(I["lines"], I["counts"], LINE_CAP, O["cart"], st), lambda k: {"cart": cart_img(env.orc, lines[k])})


def _edge_dete(env, timing):
    from compv_amd import capi
    plan = env.plan()
    # the largest weights first: the per-frame maximum (gmax, cleared by a memset per call) of call 1 is then above call 2's, so a clear that ran early shows
    ops = (capi.OP_SCHARR, capi.OP_SOBEL, capi.OP_PREWITT)
    if timing:
        plan.set_timing(1)

    def after(_):
        names = [n for n, _ in plan.get_timing()]          # waits for the entries, so it comes behind the synchronisation
        assert names == ["edge_dete_kernels"], names
    return spec({"in": frames_in([content(k) for k in range(3)])}, {"out": N_FRAMES}, lambda k, I, O, st: plan.edge_dete(I["in"], ops[k], O["out"], st),
                lambda k: {"out": maps_img([x["dete"][ops[k]] for x in fx(env.orc, k)])}, after=after if timing else None)


@case
def edge_dete(env):
    return _edge_dete(env, False)


@case
def edge_dete_timing(env):
    """compvhip_plan_set_timing on: HIP events around every kernel; the call must stay ASYNC (reading the entries is what waits) and name its kernels"""
    return _edge_dete(env, True)


@case
def houghsht(env):
    plan = env.plan()
    return spec({"edges": [edges_in(e3(env.orc, k)) for k in range(3)]}, {"lines": F * LINE_CAP * 20, "counts": 4 * F},
                lambda k, I, O, st: plan.houghsht(I["edges"], THR(k), 0, O["lines"], LINE_CAP, O["counts"], st),
                lambda k: lines_out(sht_lines(env.orc, k, THR(k))))


@case
def houghsht_line_caps(env):
    """lineCap 16 -> 10 000 behind a pending call.  Both are below the 65 536 key slots a plan keeps per frame at least (kMinLineCap), so nothing is reallocated
    here: the larger line array alone changes, and the case is held to the plain rig -- call 2 may not block, the allocation count may not move"""
    plan = env.plan()
    caps = (16, 10000, 16)

    def expect(k):
        per = sht_lines(env.orc, k, THR(k))
        return {"lines": recs_img([line_recs(l)[:caps[k]] for l in per], caps[k], 20, strict=False), "counts": full_img(np.array([len(l) for l in per], np.int32))}
    return spec({"edges": [edges_in(e3(env.orc, k)) for k in range(3)]}, [{"lines": F * caps[k] * 20, "counts": 4 * F} for k in range(2)],
                lambda k, I, O, st: plan.houghsht(I["edges"], THR(k), 0, O["lines"], caps[k], O["counts"], st), expect)


@case
def houghsht_growth(env):
    """ensureLineCap: lineCap 16 -> 70 000 on a plan whose accumulator has more than 65 536 cells (321 x 241: R * T = 202 500) makes the plan release its key
    buffers, sort scratch and chunk histograms and allocate larger ones while the first call is still pending.  Random edge maps at threshold 1, as the line-sort
    sequence of tests/content_sequences.py draws them: thousands of lines per frame"""
    import content_sequences as cs
    g = cs.SORT_GEOMETRY
    W, H, S = g
    plan = env.plan(g)
    caps = (16, 70000, 16)
    kinds = (("two_chunks", "part_chunk", "none"), ("part_chunk", "three_chunks", "two_chunks"), ("none", "two_chunks", "part_chunk"))
    maps = [np.stack([cs.sort_edge_map(kind, W, H, (40 + k, f)) for f, kind in enumerate(kinds[k])]) for k in range(3)]

    def edges(k):
        host = np.full((F, H, S), 255, np.uint8)
        host[:, :, :W] = maps[k]
        return host.reshape(-1)

    @functools.lru_cache(maxsize=None)
    def lines(k):
        return [env.orc.sht(m, 1.0, 1) for m in maps[k]]

    def expect(k):
        per = lines(k)
        assert all(len(l) <= 65536 for l in per)
        return {"lines": recs_img([line_recs(l[:caps[k]]) for l in per], caps[k], 20, strict=False), "counts": full_img(np.array([len(l) for l in per], np.int32))}
    return spec({"edges": [edges(k) for k in range(3)]}, [{"lines": F * caps[k] * 20, "counts": 4 * F} for k in range(2)],
                lambda k, I, O, st: plan.houghsht(I["edges"], 1, 0, O["lines"], caps[k], O["counts"], st), expect, growth=True)


@case
def houghsht_library_sort(env):
    """a plan on the library-sort fallback (max(W, H) > 4095): the stream-ordered entry point sorts the whole key capacity on the stream (kSortAll) and reads
    nothing back, so it is held to the plain ASYNC rig like every other plan.  Sparse random edge maps at threshold 2"""
    g = (4097, 33, 4104)
    W, H, S = g
    plan = env.plan(g)
    plan.set_timing(1)          # only to see afterwards that the fallback ran: its decode kernel is in the entries
    dens = ((0.004, 0.0, 0.002), (0.001, 0.005, 0.003), (0.003, 0.002, 0.0))
    maps = [np.stack([(np.random.default_rng(8100 + 10 * k + f).random((H, W)) < d).astype(np.uint8) * 255 for f, d in enumerate(dens[k])]) for k in range(3)]
    thr = (2, 3, 2)

    def edges(k):
        host = np.full((F, H, S), 255, np.uint8)
        host[:, :, :W] = maps[k]
        return host.reshape(-1)

    def expect(k):
        per = [env.orc.sht(m, 1.0, thr[k]) for m in maps[k]]
        assert all(len(l) <= 65536 for l in per)
        return {"lines": recs_img([line_recs(l[:LINE_CAP]) for l in per], LINE_CAP, 20, strict=False), "counts": full_img(np.array([len(l) for l in per], np.int32))}
    return spec({"edges": [edges(k) for k in range(3)]}, {"lines": F * LINE_CAP * 20, "counts": 4 * F},
                lambda k, I, O, st: plan.houghsht(I["edges"], thr[k], 0, O["lines"], LINE_CAP, O["counts"], st), expect,
                after=lambda _: _assert_in("sht_decode_kernel", [n for n, _ in plan.get_timing()]))


def _assert_in(name, names):
    assert name in names, (name, names)


def _pipeline_out(env, k, thr):
    out = lines_out(sht_lines(env.orc, k, thr))
    out["edges"] = maps_img(e3(env.orc, k))
    return out


PIPE_OUT = {"edges": N_FRAMES, "lines": F * LINE_CAP * 20, "counts": 4 * F}


@case
def pipeline(env):
    plan = env.plan()
    return spec({"in": frames_in([content(k) for k in range(3)])}, PIPE_OUT,
                lambda k, I, O, st: plan.pipeline(I["in"], 59.0, 119.0, THR(k), 0, O["edges"], O["lines"], LINE_CAP, O["counts"], st),
                lambda k: _pipeline_out(env, k, THR(k)))


@case
def pipeline_async(env):
    """two steps in flight behind the stall, each with its own input (unmodified until its wait) and outputs; the tickets are waited for in order"""
    plan = env.plan()
    tickets = []

    def call(k, I, O, st):
        tickets.append(plan.pipeline_async(I["in"], 59.0, 119.0, THR(k), 0, O["edges"], O["lines"], LINE_CAP, O["counts"], st))

    def finish():
        while tickets:
            plan.wait(tickets.pop(0))
    return spec({"in": frames_in([content(k) for k in range(3)])}, PIPE_OUT, call, lambda k: _pipeline_out(env, k, THR(k)), own_inputs=True, finish=finish)


def _pipeline_ex(env, ticketed):
    """packed RGB24 in, OTSU thresholds, every optional output: gray_kernel, the Otsu histogram, Canny, the SHT and toCartesian in one enqueue"""
    from compv_amd import capi
    from gpu_support import rgb_of, sht_expect
    plan = env.plan()
    W, H, S = G
    rgb = [np.stack([rgb_of(i).reshape(H, W * 3) for i in content(k)]) for k in range(3)]
    opts = capi.PipelineOpts()
    tickets = []

    def call(k, I, O, st):
        opts.tLow, opts.tHigh, opts.threshold, opts.maxLines, opts.ksize = 0.5, 1.0, THR(k), 0, 3
        opts.thresholdType, opts.pixfmt, opts.d_gray, opts.d_otsu, opts.d_cart = capi.THRESHOLD_OTSU, capi.FMT_RGB24, O["gray"], O["otsu"], O["cart"]
        t = C.c_int(-1)
        env.ctx._chk(plan.lib.compvhip_plan_pipeline_ex(plan.h, I["in"], C.byref(opts), O["edges"], O["lines"], LINE_CAP, O["counts"], st, C.byref(t) if ticketed else None))
        if ticketed:
            tickets.append(t.value)

    def scribble():
        opts.tLow, opts.tHigh, opts.threshold, opts.maxLines, opts.ksize = 0.9, 3.0, 1, 2, 5
        opts.thresholdType, opts.pixfmt, opts.d_gray, opts.d_otsu, opts.d_cart = capi.THRESHOLD_COMPARE_TO_GRADIENT, capi.FMT_Y, None, None, None

    def finish():
        while tickets:
            plan.wait(tickets.pop(0))

    def expect(k):
        x = fx(env.orc, k)
        lines = [sht_expect(env.orc, f["rgb"][2], THETA, THR(k))[1] for f in x]
        out = lines_out(lines)
        out.update(edges=maps_img([f["rgb"][2] for f in x]), gray=maps_img([f["rgb"][0] for f in x]), otsu=full_img(np.array([f["rgb"][1] for f in x], np.int32)),
                   cart=cart_img(env.orc, lines))
        return out
    out = dict(PIPE_OUT, gray=N_FRAMES, otsu=4 * F, cart=F * LINE_CAP * 16)
    return spec({"in": frames_in(rgb, 3)}, out, call, expect, scribble=scribble, own_inputs=ticketed, finish=finish if ticketed else None,
                cls=sc.ASYNC if ticketed else None)          # with a ticket the call is ASYNC (the row is the plain form: WAITS)


@case
def pipeline_ex(env):
    return _pipeline_ex(env, False)


@case
def pipeline_ex_ticket(env):
    return _pipeline_ex(env, True)


def _kht(env, order):
    """the edge maps are produced by a device copy queued behind the stall; the call is made at once and must return the lines of those maps"""
    from kht_canon_model import CanonModel
    from kht_canon_model import line_bits, model_line_bits
    plan = env.plan()

    from compv_amd import capi
    cap = 1 << 14
    opts = capi.KhtOpts()          # the host struct compvhip_plan_houghkht_ex reads

    def call(k, I, O, st):
        if order != "canonical":
            return plan.houghkht(I["edges"], 1.0, THETA, 12, order=order)
        opts.rho, opts.thetaDeg, opts.threshold, opts.maxLines, opts.clusterMinDeviation, opts.clusterMinSize = 1.0, THETA, 12, 0, 2.0, 10
        opts.kernelMinHeight, opts.hostThreads, opts.order = 0.002, 0, capi.KHT_ORDER_CANONICAL
        lines, counts, gs = np.zeros((F, cap), capi.LINE_DTYPE), np.zeros(F, np.uint64), np.full(F, np.nan, np.float64)
        env.ctx._chk(plan.lib.compvhip_plan_houghkht_ex(plan.h, I["edges"], C.byref(opts), lines.ctypes.data, cap, counts.ctypes.data, gs.ctypes.data))
        return [lines[f][:int(counts[f])] for f in range(F)], [None if np.isnan(g) else float(g) for g in gs]

    def scribble():
        opts.rho, opts.thetaDeg, opts.threshold, opts.maxLines, opts.order = 0.5, 2.0, 99, 1, capi.KHT_ORDER_REFERENCE

    def check_host(k, res):
        lines, gs = res
        for f, e in enumerate(e3(env.orc, k)):
            if order == "canonical":
                el, egs = CanonModel(env.orc).lines(e, 1.0, THETA, 12)[:2]
                assert line_bits(lines[f]) == model_line_bits(el) and gs[f] == egs, ("canonical kht of call", k + 1, "frame", f)
            else:
                el, egs = fx(env.orc, k)[f]["kht"]
                assert [(float(l["rho"]), float(l["theta"]), int(l["strength"])) for l in lines[f]] == \
                    [(float(np.float32(l[0])), float(np.float32(l[1])), int(l[2])) for l in el], ("kht of call", k + 1, "frame", f)
                assert (gs[f] == egs) if len(el) else (gs[f] is None), ("kht gs of call", k + 1, "frame", f)

    def expect(k):          # no device output: the line lists themselves must differ between the contents
        per = [fx(env.orc, k)[f]["kht"][0] for f in range(F)]
        return {"host lines": full_img(np.array([[float(l[0]), float(l[1]), float(l[2])] for p in per for l in p] + [[len(p) for p in per]], np.float64).reshape(-1))}
    s = spec({"edges": [edges_in(e3(env.orc, k)) for k in range(3)]}, {}, call, lambda k: {}, drains=True, check_host=check_host, scribble=scribble if order == "canonical" else None)
    s.host_expect = expect
    return s


@case
def houghkht(env):
    return _kht(env, "reference")


@case
def houghkht_ex(env):
    return _kht(env, "canonical")


@case
def acc_export(env):
    """the accumulators the SHT queued just before left in the plan, frame by frame"""
    plan = env.plan()
    R, T, _ = env.orc.sht_dims(G[0], G[1], THETA)
    n = R * T * 4

    def call(k, I, O, st):
        plan.houghsht(I["edges"], THR(k), 0, 0, 0, O["counts"], st)
        for f in range(F):
            plan.acc_export(f, O["acc"] + f * n, T, st)
    return spec({"edges": [edges_in(e3(env.orc, k)) for k in range(3)]}, {"acc": F * n, "counts": 4 * F}, call,
                lambda k: {"acc": full_img(np.stack([np.ascontiguousarray(x["sht"][0], np.int32) for x in fx(env.orc, k)])),
                           "counts": full_img(np.array([len(l) for l in sht_lines(env.orc, k, THR(k))], np.int32))})


# ---- features on the plan ----------------------------------------------------------------------------------------------------------------------
def _line_inputs(env):
    lines = [sht_lines(env.orc, k, thr0()) for k in range(3)]
    host = [lines_in(l) for l in lines]
    arrays = [[line_recs(l) for l in per] for per in lines]
    return {"edges": [edges_in(e3(env.orc, k)) for k in range(3)], "lines": [h[0] for h in host], "counts": [h[1] for h in host]}, arrays


SEG_CAP = 64


@case
def houghsht_segments(env):
    import sht_segments_rig as tgs
    plan = env.plan()
    inputs, arrays = _line_inputs(env)
    sinQ, cosQ = tgs.tables(env.orc, G[0], G[1], THETA)
    prm = ((3, 1), (1, 0), (3, 1))

    def expect(k):
        segs = tgs.model_frames(e3(env.orc, k), sinQ, cosQ, arrays[k], [prm[k]], MAX_LINES)[prm[k]]
        return {"segs": recs_img(segs, SEG_CAP, SEG_BYTES), "segCounts": full_img(np.array([len(x) for x in segs], np.int32))}
    return spec(inputs, {"segs": F * SEG_CAP * SEG_BYTES, "segCounts": 4 * F},
                lambda k, I, O, st: plan.houghsht_segments(I["edges"], I["lines"], I["counts"], LINE_CAP, MAX_LINES, prm[k][0], prm[k][1], O["segs"], SEG_CAP, O["segCounts"], st), expect)


@case
def houghsht_fit(env):
    import sht_fit_rig as tgf
    plan = env.plan()
    inputs, arrays = _line_inputs(env)
    R, (sinQ, cosQ) = tgf.tables(env.orc, G[0], G[1], THETA)
    half, cut = (2, 0, 2), (MAX_LINES, 7, MAX_LINES)          # maxLines changes too: the fit counts are the lines walked

    def expect(k):
        fits = tgf.model_fits(e3(env.orc, k), sinQ, cosQ, R, arrays[k], half[k], cut[k])[0]
        return {"fits": recs_img(fits, SEG_CAP, FIT_BYTES), "fitCounts": full_img(np.array([len(x) for x in fits], np.int32))}
    return spec(inputs, {"fits": F * SEG_CAP * FIT_BYTES, "fitCounts": 4 * F},
                lambda k, I, O, st: plan.houghsht_fit(I["edges"], I["lines"], I["counts"], LINE_CAP, cut[k], half[k], 0, 0, 0, O["fits"], SEG_CAP, O["fitCounts"], 0, st), expect)


@case
def components(env):
    import components_rig as tgc
    plan = env.plan()
    W, H, S = G
    ls, cap = W + 3, 512
    prm = ((8, 1), (4, 2), (8, 1))

    def expect(k):
        m = tgc.model(e3(env.orc, k), *prm[k])
        assert all(len(x[1]) <= cap for x in m)
        return {"labels": maps_img([np.ascontiguousarray(x[0], np.int32) for x in m], strict=True, S=ls, elem=4), "comps": recs_img([x[1] for x in m], cap, COMP_BYTES),
                "compCounts": full_img(np.array([len(x[1]) for x in m], np.int32))}
    return spec({"edges": [edges_in(e3(env.orc, k)) for k in range(3)]}, {"labels": F * H * ls * 4, "comps": F * cap * COMP_BYTES, "compCounts": 4 * F},
                lambda k, I, O, st: plan.components(I["edges"], prm[k][0], prm[k][1], O["labels"], ls, O["comps"], cap, O["compCounts"], st), expect)


@case
def threshold(env):
    import morph_model as mm
    plan = env.plan()
    t = (97.0, 150.0, 97.0)
    return spec({"in": frames_in([content(k) for k in range(3)])}, {"out": N_FRAMES}, lambda k, I, O, st: plan.threshold(I["in"], t[k], O["out"], 0, st),
                lambda k: {"out": maps_img([mm.threshold(img, t[k]) for img in content(k)], strict=True)})


def _adaptive(env, in_place):
    import morph_model as mm
    plan = env.plan()
    delta = (7.0, -3.0, 7.0)

    def expect(k):
        img, mask = maps_img([mm.adaptive(i, 9, delta[k], 200.0, True) for i in content(k)], strict=not in_place)
        if in_place:          # columns >= W keep the input's bytes
            keep = frames_in([content(j) for j in range(3)])[k].reshape(F, G[1], G[2])
            img = img.reshape(keep.shape).copy()
            img[:, :, G[0]:] = keep[:, :, G[0]:]
            img, mask = img.reshape(-1), np.ones(img.size, bool)
        return {"out": (img, mask)}
    kw = dict(own_inputs=True, alias={"out": "in"}) if in_place else {}
    return spec({"in": frames_in([content(k) for k in range(3)])}, {"out": N_FRAMES},
                lambda k, I, O, st: plan.threshold_adaptive(I["in"], 9, delta[k], 200.0, True, O["out"], st), expect, **kw)


@case
def threshold_adaptive(env):
    return _adaptive(env, False)


@case
def threshold_adaptive_in_place(env):
    """d_out == d_in: through morphTmp and a device copy back"""
    return _adaptive(env, True)


def _morph(env, kernel, strels):
    import morph_model as mm
    plan = env.plan()
    shape = strels[0].shape
    assert all(s.shape == shape for s in strels)
    se = np.zeros(shape, np.uint8)          # the host array the call reads

    def call(k, I, O, st):
        se[:] = strels[k]
        plan.morph(I["in"], se, mm.CLOSE, mm.BORDER_REPLICATE, O["out"], kernel, st)

    def scribble():
        se[:] = 0
        se[shape[0] // 2, shape[1] // 2] = 255
    return spec({"in": frames_in([content(k) for k in range(3)])}, {"out": N_FRAMES}, call,
                lambda k: {"out": maps_img([mm.morph(i, strels[k], mm.CLOSE, mm.BORDER_REPLICATE) for i in content(k)], strict=True)}, scribble=scribble)


@case
def morph(env):
    """close (two passes through the plan's plane) with a separable element that changes between the calls"""
    import morph_model as mm
    from compv_amd import capi
    return _morph(env, capi.MORPH_KERNEL_AUTO, [mm.strel(mm.RECT, 5, 5), mm.strel(mm.CROSS, 5, 5), mm.strel(mm.RECT, 5, 5)])


@case
def morph_ex(env):
    from compv_amd import capi
    rng = np.random.default_rng(57)
    a, b = ((rng.random((7, 5)) < 0.4).astype(np.uint8) * 255 for _ in range(2))
    return _morph(env, capi.MORPH_KERNEL_GENERAL, [a, b, a])


FAST_CAP = 700


@case
def fast(env):
    import fast_model as fm
    plan = env.plan()
    t = (20, 35, 20)

    def expect(k):
        m = [fm.fast(img, t[k], 9, True) for img in content(k)]
        assert all(len(x[0]) <= FAST_CAP for x in m)
        return {"scores": maps_img([x[1] for x in m], strict=True), "corners": recs_img([x[0] for x in m], FAST_CAP, 12), "counts": full_img(np.array([len(x[0]) for x in m], np.int32))}
    return spec({"in": frames_in([content(k) for k in range(3)])}, {"scores": N_FRAMES, "corners": F * FAST_CAP * 12, "counts": 4 * F},
                lambda k, I, O, st: plan.fast(I["in"], t[k], 9, True, -1, O["scores"], O["corners"], FAST_CAP, O["counts"], st), expect)


def _orb_inputs():
    """frames, corner lists and counts per content: the lists of tests/test_gpu_orb.py, other ones for every content"""
    import orb_model as om
    import orb_rig as go
    W, H, _ = G
    lists = [[go.corner_list(W, H, (5, 3, 6, 4, 2, 7, 3, 5, 4)[3 * k + f], 900 + 10 * k + f) for f in range(F)] for k in range(3)]
    cap = max(len(c) for per in lists for c in per) + 3
    hosts, counts = [], []
    for k in range(3):
        h = np.zeros((F, cap), om.CORNER_DTYPE)
        for f, c in enumerate(lists[k]):
            h[f, :len(c)] = c
        hosts.append(u8(h))
        counts.append(u8(np.array([len(c) for c in lists[k]], np.int32)))
    return lists, cap, hosts, counts


ORB_PRM = ((0, 1.0), (1, 0.83), (0, 1.0))          # level, scale


def _orb_keypoints(env, key_caps):
    import orb_model as om
    plan = env.plan()
    lists, ccap, hosts, counts = _orb_inputs()

    def expect(k):
        m = [om.keypoints(img, lists[k][f], ORB_PRM[k][0], np.float32(ORB_PRM[k][1])) for f, img in enumerate(content(k))]
        cap = key_caps[k]
        return {"keys": recs_img([x[0][:cap] for x in m], cap, 24), "moments": recs_img([x[1][:cap] for x in m], cap, 8), "keyCounts": full_img(np.array([len(x[0]) for x in m], np.int32))}
    return spec({"in": frames_in([content(k) for k in range(3)]), "corners": hosts, "cornerCounts": counts},
                [{"keys": F * key_caps[k] * 24, "moments": F * key_caps[k] * 8, "keyCounts": 4 * F} for k in range(2)],
                lambda k, I, O, st: plan.orb_keypoints(I["in"], I["corners"], ccap, I["cornerCounts"], ORB_PRM[k][0], float(np.float32(ORB_PRM[k][1])), O["keys"], key_caps[k],
                                                       O["keyCounts"], O["moments"], st), expect, growth=key_caps[0] != key_caps[1])


@case
def orb_keypoints(env):
    return _orb_keypoints(env, (16, 16, 16))


@case
def orb_keypoints_growth(env):
    """keyCap 4 -> 4096 behind a pending call: the plan's index list grows with keyCap"""
    return _orb_keypoints(env, (4, 4096, 4))


@case
def orb_describe(env):
    import orb_model as om
    plan = env.plan()
    lists, _, _, _ = _orb_inputs()
    cap = 16
    keys = [[om.keypoints(img, lists[k][f], ORB_PRM[k][0], np.float32(ORB_PRM[k][1]))[0] for f, img in enumerate(content(k))] for k in range(3)]
    assert all(len(x) <= cap for per in keys for x in per)
    hosts = []
    for k in range(3):
        h = np.zeros((F, cap), om.KEYPOINT_DTYPE)
        for f, x in enumerate(keys[k]):
            h[f, :len(x)] = x
        hosts.append(u8(h))

    def expect(k):
        rows = [om.describe(om.blur(img), keys[k][f], np.float32(ORB_PRM[k][1])) for f, img in enumerate(content(k))]
        return {"desc": recs_img(rows, cap, 32)}
    return spec({"in": frames_in([content(k) for k in range(3)]), "keys": hosts, "keyCounts": [u8(np.array([len(x) for x in keys[k]], np.int32)) for k in range(3)]},
                {"desc": F * cap * 32}, lambda k, I, O, st: plan.orb_describe(I["in"], I["keys"], cap, I["keyCounts"], float(np.float32(ORB_PRM[k][1])), O["desc"], 32, True, st), expect)


@case
def scale(env):
    import orb_pyramid_model as pm
    plan = env.plan()
    wo, ho, so = 57, 31, 64
    return spec({"in": frames_in([content(k) for k in range(3)])}, {"out": F * ho * so}, lambda k, I, O, st: plan.scale(I["in"], O["out"], wo, ho, so, st),
                lambda k: {"out": maps_img([pm.scale(i, wo, ho) for i in content(k)], strict=True, S=so)})


REMAP_OUT = (37, 11, 40)


@case
def remap(env):
    import remap_cases as rc
    import remap_model as rm
    from compv_amd import capi
    plan = env.plan()
    W, H, S = G
    wo, ho, so = REMAP_OUT
    maps = [rc.random_map(W, H, wo, ho, 62000 + k) for k in range(3)]
    rois = ((-5.0, 30.25, 3.5, 400.0), (2.0, 40.0, 0.0, 30.0), (-5.0, 30.25, 3.5, 400.0))
    dflt = (9, 77, 9)
    roi = capi.Roi()          # the host struct the call reads

    def call(k, I, O, st):
        roi.left, roi.right, roi.top, roi.bottom = rois[k]
        plan.remap(I["in"], I["x"], I["y"], 1, rm.BILINEAR, O["out"], wo, ho, so, roi, dflt[k], st)

    def scribble():
        roi.left, roi.right, roi.top, roi.bottom = 1.0, 2.0, 1.0, 2.0
    return spec({"in": frames_in([content(k) for k in range(3)]), "x": [u8(np.ascontiguousarray(m[0], np.float32)) for m in maps], "y": [u8(np.ascontiguousarray(m[1], np.float32)) for m in maps]},
                {"out": F * ho * so}, call, lambda k: {"out": maps_img([rm.remap(i, maps[k][0], maps[k][1], rm.BILINEAR, rois[k], dflt[k]) for i in content(k)], strict=True, S=so)},
                scribble=scribble)


def _warp_matrices(wo, ho, n):
    import remap_cases as rc
    base = rc.matrices(G[0], G[1], wo, ho)["affine"]
    out = []
    for j in range(n):
        m = base.copy()
        m[0, 2] += np.float32(1.25 * j)
        m[1, 2] -= np.float32(0.75 * j)
        out.append(m)
    return out


@case
def hog(env):
    import hog_model as hm
    from compv_amd import capi
    plan = env.plan()
    prm = dict(blockW=16, blockH=16, strideW=8, strideH=8, cellW=8, cellH=8, nbins=9, blockNorm=hm.NORM_L2HYS)
    norms = (hm.NORM_L2HYS, hm.NORM_L1, hm.NORM_L2HYS)
    g = hm.geometry(G[0], G[1], hm.resolve(prm))
    stride, cells = g["descLen"] + 5, g["cellsY"] * g["cellsX"] * 9
    o = capi.HogOpts(**hm.resolve(prm))          # the host struct the call reads

    def call(k, I, O, st):
        o.nbins, o.blockNorm, o.cellW = 9, norms[k], 8
        plan.hog(I["in"], O["desc"], stride, O["cells"], opts=o, stream=st)

    def scribble():
        o.nbins, o.blockNorm, o.cellW = 4, hm.NORM_NONE, 16

    def expect(k):
        m = [hm.hog(img, dict(prm, blockNorm=norms[k])) for img in content(k)]
        return {"desc": recs_img([np.ascontiguousarray(x[0], np.float32) for x in m], stride, 4), "cells": full_img(np.stack([np.ascontiguousarray(x[1], np.float32) for x in m]))}
    return spec({"in": frames_in([content(k) for k in range(3)])}, {"desc": F * stride * 4, "cells": F * cells * 4}, call, expect, scribble=scribble)


@case
def hog_growth(env):
    """the plan's own cell map (d_cells NULL): a layout with more cells behind a pending call makes it reallocate"""
    import hog_model as hm
    plan = env.plan()
    prm = [dict(blockW=16, blockH=16, strideW=16, strideH=16, cellW=16, cellH=16, nbins=4, blockNorm=hm.NORM_L2), dict(blockW=8, blockH=8, strideW=4, strideH=4, cellW=4, cellH=4, nbins=18, blockNorm=hm.NORM_L2)]
    prm.append(prm[0])
    lens = [hm.geometry(G[0], G[1], hm.resolve(p))["descLen"] for p in prm]
    return spec({"in": frames_in([content(k) for k in range(3)])}, [{"desc": F * lens[k] * 4} for k in range(2)],
                lambda k, I, O, st: plan.hog(I["in"], O["desc"], lens[k], 0, stream=st, **prm[k]),
                lambda k: {"desc": full_img(np.stack([np.ascontiguousarray(hm.hog(img, prm[k])[0], np.float32) for img in content(k)]))}, growth=True)


def _stats(env, outputs, call, expect):
    plan = env.plan()
    return spec({"in": frames_in([content(k) for k in range(3)])}, outputs, lambda k, I, O, st: call(plan, k, I, O, st), expect)


@case
def integral(env):
    import stats_model as sm
    W, H, _ = G
    stride = W + 3

    def expect(k):
        m = [sm.integral(img) for img in content(k)]
        return {"sum": maps_img([np.ascontiguousarray(x[0], np.float64) for x in m], strict=True, S=stride, elem=8), "sumsq": maps_img([np.ascontiguousarray(x[1], np.float64) for x in m], strict=True, S=stride, elem=8)}
    n = F * (H + 1) * stride * 8
    return _stats(env, {"sum": n, "sumsq": n}, lambda plan, k, I, O, st: plan.integral(I["in"], O["sum"], O["sumsq"], stride, st), expect)


@case
def histogram(env):
    import stats_model as sm
    return _stats(env, {"hist": F * 1024}, lambda plan, k, I, O, st: plan.histogram(I["in"], O["hist"], st),
                  lambda k: {"hist": full_img(np.stack([sm.histogram(img) for img in content(k)]))})


@case
def equalize(env):
    import stats_model as sm
    scales = (0.0, 0.05, 0.0)

    def expect(k):
        m = [sm.equalize(img, None, scales[k]) for img in content(k)]
        return {"out": maps_img([x[0] for x in m]), "lut": full_img(np.stack([np.ascontiguousarray(x[1], np.uint8) for x in m]))}
    return _stats(env, {"out": N_FRAMES, "lut": F * 256}, lambda plan, k, I, O, st: plan.equalize(I["in"], O["out"], 0, scales[k], O["lut"], st), expect)


@case
def projections(env):
    import stats_model as sm
    W, H, _ = G

    def expect(k):
        m = [sm.projections(img) for img in content(k)]
        return {"x": full_img(np.stack([x[0] for x in m])), "y": full_img(np.stack([x[1] for x in m]))}
    return _stats(env, {"x": F * W * 4, "y": F * H * 4}, lambda plan, k, I, O, st: plan.projections(I["in"], O["x"], O["y"], st), expect)


# ---- the ORB pyramid, the matcher, the homography, the colour conversion -------------------------------------------------------------------------------
PYR = (64, 50, 64, 2, 0.83, 400)          # W, H, S, levels, scale factor, maxFeatures
PYR_CAP = 256


@functools.lru_cache(maxsize=None)
def pyr_content(k):
    import fast_model as fm
    W, H = PYR[:2]
    kinds = ((fm.noise, fm.blocks, fm.noise), (fm.blocks, fm.noise, fm.blocks), (fm.noise, fm.noise, fm.blocks))[k]
    return np.stack([fn(W, H, 300 + 10 * k + f) for f, fn in enumerate(kinds)])


@functools.lru_cache(maxsize=None)
def pyr_model(k):
    import orb_pyramid_model as pm
    W, H, S, levels, sf, mf = PYR
    return [pm.detect(img, levels, sf, 20, 9, True, mf, None) for img in pyr_content(k)]


def _pyr(env):
    from compv_amd import capi
    W, H, S, levels, sf, mf = PYR
    return env.own(capi.OrbPyramid(env.ctx, W, H, S, F, capi.OrbPyramidOpts(levels, sf, 20, 9, True, mf), 4096))


@case
def orbpyr_detect(env):
    pyr = _pyr(env)
    levels = PYR[3]

    def expect(k):
        m = pyr_model(k)
        assert all(len(x[0]) <= PYR_CAP for x in m)
        return {"keys": recs_img([x[0] for x in m], PYR_CAP, 24), "keyCounts": full_img(np.array([len(x[0]) for x in m], np.int32)),
                "levelCounts": full_img(np.stack([np.asarray(x[1], np.int32) for x in m])), "levelCorners": full_img(np.stack([np.asarray(x[2], np.int32) for x in m]))}
    return spec({"in": frames_in([pyr_content(k) for k in range(3)], S=PYR[2])}, {"keys": F * PYR_CAP * 24, "keyCounts": 4 * F, "levelCounts": 4 * F * levels, "levelCorners": 4 * F * levels},
                lambda k, I, O, st: pyr.detect(I["in"], O["keys"], PYR_CAP, O["keyCounts"], O["levelCounts"], O["levelCorners"], st), expect)


@case
def orbpyr_describe(env):
    """with rebuilt planes: the scale and blur launches of every level are the call's own"""
    import orb_model as om
    import orb_pyramid_model as pm
    pyr = _pyr(env)
    W, H, S, levels, sf, mf = PYR
    geo = pm.geometry(W, H, levels, sf, mf)
    hosts = []
    for k in range(3):
        h = np.zeros((F, PYR_CAP), om.KEYPOINT_DTYPE)
        for f, x in enumerate(pyr_model(k)):
            h[f, :len(x[0])] = x[0]
        hosts.append(u8(h))
    return spec({"in": frames_in([pyr_content(k) for k in range(3)], S=S), "keys": hosts, "keyCounts": [u8(np.array([len(x[0]) for x in pyr_model(k)], np.int32)) for k in range(3)]},
                {"desc": F * PYR_CAP * 32}, lambda k, I, O, st: pyr.describe(I["in"], I["keys"], PYR_CAP, I["keyCounts"], O["desc"], 32, False, st),
                lambda k: {"desc": recs_img([pm.describe(x[3], geo, x[0]) for x in pyr_model(k)], PYR_CAP, 32)})


MATCH = dict(B=32, qcap=70, tcap=131, pairs=F, knn=2)


@functools.lru_cache(maxsize=None)
def match_sides(k):
    """(query [pairs][qcap][B], train [pairs][tcap][B]): queries derived from train rows, as tests/test_gpu_match.py derives them"""
    import match_rig as gm
    m = MATCH
    train = gm.descriptors("uniform", m["pairs"], m["tcap"], m["B"], m["B"], 40 + k)
    query = np.stack([gm.derived(train[p], m["qcap"], m["B"], 50 + 7 * k + p) for p in range(m["pairs"])])
    return np.ascontiguousarray(query), np.ascontiguousarray(train)


def _matcher(env):
    from compv_amd import capi
    m = MATCH
    return env.own(capi.Matcher(env.ctx, m["B"], m["qcap"], m["tcap"], m["pairs"], m["knn"]))


@case
def matcher_knn(env):
    import match_model as mm
    mt = _matcher(env)
    m = MATCH
    return spec({"query": [match_sides(k)[0] for k in range(3)], "train": [match_sides(k)[1] for k in range(3)]}, {"matches": m["pairs"] * m["knn"] * m["qcap"] * 16},
                lambda k, I, O, st: mt.knn(I["query"], m["B"], 0, I["train"], m["B"], 0, False, O["matches"], st),
                lambda k: {"matches": full_img(np.stack([mm.knn_device(match_sides(k)[0][p], match_sides(k)[1][p], m["knn"]) for p in range(m["pairs"])]))})


MATCH_OPTS = ((0.8, -1, True), (0.6, 60, False), (0.8, -1, True))          # ratio, maxDistance, crossCheck


@case
def matcher_good(env):
    """the good list of the knn records the model gives for the content (crossCheck runs the slice kernels again with the roles swapped)"""
    import match_model as mm
    from compv_amd import capi
    mt = _matcher(env)
    m = MATCH
    knn = [np.stack([mm.knn_device(match_sides(k)[0][p], match_sides(k)[1][p], m["knn"]) for p in range(m["pairs"])]) for k in range(3)]
    o = capi.MatchOpts()          # the host struct the call reads

    def call(k, I, O, st):
        o.ratio, o.maxDistance, o.crossCheck = MATCH_OPTS[k][0], MATCH_OPTS[k][1], int(MATCH_OPTS[k][2])
        env.ctx._chk(mt.lib.compvhip_matcher_good(mt.h, I["matches"], I["query"], m["B"], None, I["train"], m["B"], None, 0, C.byref(o), O["good"], m["qcap"], O["goodCounts"], st))

    def scribble():
        o.ratio, o.maxDistance, o.crossCheck = 0.0, 0, 0

    def expect(k):
        r, d, cc = MATCH_OPTS[k]
        g = [mm.good(match_sides(k)[0][p], match_sides(k)[1][p], m["knn"], ratio=r, max_distance=d, cross_check=cc) for p in range(m["pairs"])]
        return {"good": recs_img(g, m["qcap"], 16), "goodCounts": full_img(np.array([len(x) for x in g], np.int32))}
    return spec({"matches": [u8(x) for x in knn], "query": [match_sides(k)[0] for k in range(3)], "train": [match_sides(k)[1] for k in range(3)]},
                {"good": m["pairs"] * m["qcap"] * 16, "goodCounts": 4 * m["pairs"]}, call, expect, scribble=scribble)


HOM = dict(pairs=F, cap=65, tries=64)
HOM_PRM = ((4, 30.0), (9, 12.5), (4, 30.0))          # seed, threshold


@functools.lru_cache(maxsize=None)
def hom_points(k):
    """(src, dst [pairs][cap][2], counts) of content k: planted models of other sizes and outlier shares"""
    import homography_cases as hc
    rng = np.random.default_rng(70 + k)
    src, dst = rng.uniform(-1e6, 1e6, (HOM["pairs"], HOM["cap"], 2)), rng.uniform(-1e6, 1e6, (HOM["pairs"], HOM["cap"], 2))
    counts = []
    for p in range(HOM["pairs"]):
        n = (9, 65, 33, 40, 12, 65, 20, 50, 9)[3 * k + p]
        s, d = hc.planted(n, (0.0, 0.3, 0.3)[p], 80 + 10 * k + p)[:2]
        src[p, :n], dst[p, :n] = s, d
        counts.append(n)
    return src, dst, counts


@functools.lru_cache(maxsize=None)
def hom_model(k, j=None):
    """homography_model.find of content k with the parameters of call j"""
    import homography_model as hm
    src, dst, counts = hom_points(k)
    seed, thr = HOM_PRM[k if j is None else j]
    return [hm.find(src[p], dst[p], counts[p], HOM["tries"], threshold=thr, seed=seed, pair=p) for p in range(HOM["pairs"])]


def _hom(env):
    from compv_amd import capi
    return env.own(capi.Homography(env.ctx, HOM["pairs"], HOM["cap"], HOM["tries"]))


def _hom_out(k):
    import homography_model as hm
    m = hom_model(k)
    counts = hom_points(k)[2]
    return {"results": full_img(np.array([e["result"] for e in m], hm.RESULT_DTYPE)), "mask": recs_img([np.asarray(e["mask"], np.uint8)[:counts[p]] for p, e in enumerate(m)], HOM["cap"], 1)}


def _hom_inputs():
    return {"src": [u8(hom_points(k)[0]) for k in range(3)], "dst": [u8(hom_points(k)[1]) for k in range(3)], "counts": [u8(np.array(hom_points(k)[2], np.int32)) for k in range(3)]}


@case
def homography_find(env):
    import homography_model as hm
    from compv_amd import capi
    h = _hom(env)
    o = capi.HomographyOpts()          # the host struct the call reads

    def call(k, I, O, st):
        o.tries, o.seed, o.threshold = HOM["tries"], HOM_PRM[k][0], HOM_PRM[k][1]
        env.ctx._chk(h.lib.compvhip_homography_find(h.h, I["src"], I["dst"], I["counts"], C.byref(o), None, O["results"], O["mask"], st))

    def scribble():
        o.tries, o.seed, o.threshold = 1, 999, 1.0
    return spec(_hom_inputs(), {"results": HOM["pairs"] * hm.RESULT_DTYPE.itemsize, "mask": HOM["pairs"] * HOM["cap"]}, call, _hom_out, scribble=scribble)


@case
def homography_scores(env):
    """the per-try scores of the find queued just before, copied to host arrays: the call waits for the stream, and what it returns belongs to that find"""
    import homography_model as hm
    h = _hom(env)

    def call(k, I, O, st):
        h.find(I["src"], I["dst"], I["counts"], O["results"], O["mask"], tries=HOM["tries"], threshold=HOM_PRM[k][1], seed=HOM_PRM[k][0], stream=st)
        return h.scores(HOM["tries"], st)

    def check_host(k, res):
        counts, var, rot = res
        for p, e in enumerate(hom_model(k)):
            assert counts[p].tolist() == np.asarray(e["counts"]).tolist(), ("per-try counts of call", k + 1, "pair", p)
            assert var[p].tobytes() == np.ascontiguousarray(e["variances"], np.float64).tobytes(), ("per-try variances of call", k + 1, "pair", p)
            assert rot[p].tolist() == np.asarray(e["rotations"]).tolist(), ("per-try rotations of call", k + 1, "pair", p)
    return spec(_hom_inputs(), {"results": HOM["pairs"] * hm.RESULT_DTYPE.itemsize, "mask": HOM["pairs"] * HOM["cap"]}, call, _hom_out, check_host=check_host)


@case
def homography_points(env):
    """points gathers into the handle; the find queued behind it (d_src NULL) shows what it gathered"""
    import homography_model as hm
    h = _hom(env)
    cap, pairs, qcap, tcap = HOM["cap"], HOM["pairs"], 80, 90
    data = []
    for k in range(3):
        rng = np.random.default_rng(170 + k)
        src, dst, counts = hom_points(k)
        tk, qk = np.zeros((pairs, tcap), hm.KEYPOINT_DTYPE), np.zeros((pairs, qcap), hm.KEYPOINT_DTYPE)
        good, sets = np.zeros((pairs, cap), hm.MATCH_DTYPE), []
        for p in range(pairs):
            n = counts[p]
            ti, qi = rng.permutation(tcap)[:n], rng.permutation(qcap)[:n]
            tk[p]["x"], tk[p]["y"] = rng.uniform(0, 640, tcap), rng.uniform(0, 480, tcap)
            qk[p]["x"], qk[p]["y"] = rng.uniform(0, 640, qcap), rng.uniform(0, 480, qcap)
            tk[p]["x"][ti], tk[p]["y"][ti] = src[p, :n, 0], src[p, :n, 1]          # float32 positions: the points the model gathers are these, not hom_points'
            qk[p]["x"][qi], qk[p]["y"][qi] = dst[p, :n, 0], dst[p, :n, 1]
            good[p, :n]["queryIdx"], good[p, :n]["trainIdx"] = qi, ti
            sets.append(hm.gather(good[p], n, cap, cap, qk[p], tk[p]))
        data.append((good, np.array(counts, np.int32), qk, tk, sets))

    def call(k, I, O, st):
        h.points(I["good"], cap, I["goodCounts"], I["query"], qcap, I["train"], tcap, False, st)
        h.find(0, 0, 0, O["results"], O["mask"], tries=HOM["tries"], threshold=HOM_PRM[k][1], seed=HOM_PRM[k][0], stream=st)

    def expect(k):
        sets = data[k][4]
        m = [hm.find(s, d, len(s), HOM["tries"], threshold=HOM_PRM[k][1], seed=HOM_PRM[k][0], pair=p) for p, (s, d) in enumerate(sets)]
        return {"results": full_img(np.array([e["result"] for e in m], hm.RESULT_DTYPE)), "mask": recs_img([np.asarray(e["mask"], np.uint8)[:len(sets[p][0])] for p, e in enumerate(m)], cap, 1)}
    return spec({"good": [u8(d[0]) for d in data], "goodCounts": [u8(d[1]) for d in data], "query": [u8(d[2]) for d in data], "train": [u8(d[3]) for d in data]},
                {"results": pairs * hm.RESULT_DTYPE.itemsize, "mask": pairs * cap}, call, expect)


@case
def homography_project(env):
    import homography_model as hm
    h = _hom(env)
    n = 37
    res = [np.array([e["result"] for e in hom_model(k)], hm.RESULT_DTYPE) for k in range(3)]
    pts = [np.random.default_rng(90 + k).uniform(0, 640, (HOM["pairs"], n, 2)) for k in range(3)]
    return spec({"results": [u8(r) for r in res], "points": [u8(p) for p in pts]}, {"out": HOM["pairs"] * n * 16},
                lambda k, I, O, st: h.project(I["results"], I["points"], n, False, O["out"], st),
                lambda k: {"out": full_img(np.stack([hm.project(res[k][p]["H"], pts[k][p]) for p in range(HOM["pairs"])]))})


@case
def convert_frames(env):
    """NV12 -> RGBA32 on padded rows; the two compvhip_image structs are the host data the call reads"""
    import convert_model as cm
    from compv_amd import capi
    W, H = 33, 17
    shapes = cm.plane_shapes(cm.NV12, W, H)
    rb_in = [s[1] + 5 for s in shapes]
    rb_out = W * 4 + 12
    planes = [[[np.random.default_rng(500 + 10 * k + 3 * f + p).integers(0, 256, s, dtype=np.uint8) for p, s in enumerate(shapes)] for f in range(F)] for k in range(3)]

    def packed(k, p):
        out = np.random.default_rng(600 + k).integers(0, 256, (F, shapes[p][0], rb_in[p]), dtype=np.uint8)
        for f in range(F):
            out[f, :, :shapes[p][1]] = planes[k][f][p]
        return out.reshape(-1)
    a, b = capi.Image(cm.NV12, [None, None], rb_in), capi.Image(cm.RGBA32, [None], [rb_out])

    def call(k, I, O, st):
        a.pixfmt, b.pixfmt = cm.NV12, cm.RGBA32
        for p in range(2):
            a.plane[p], a.rowBytes[p], a.frameBytes[p] = I["p%d" % p], rb_in[p], rb_in[p] * shapes[p][0]
        b.plane[0], b.rowBytes[0], b.frameBytes[0] = O["rgba"], rb_out, rb_out * H
        env.ctx.convert_frames(W, H, F, a, b, st)

    def scribble():
        a.pixfmt, b.pixfmt = cm.NV21, cm.RGB24
        for im in (a, b):
            for p in range(3):
                im.plane[p], im.rowBytes[p], im.frameBytes[p] = None, 1, 1
    return spec({"p0": [packed(k, 0) for k in range(3)], "p1": [packed(k, 1) for k in range(3)]}, {"rgba": F * H * rb_out}, call,
                lambda k: {"rgba": maps_img([cm.convert(cm.NV12, cm.RGBA32, planes[k][f], W, H)[0] for f in range(F)], strict=True, S=rb_out)}, scribble=scribble)


def _warp(env, stall, dests, live_stays, stalled=True, cold=None):
    """compvhip_plan_warp_inverse: six calls with six matrices into six destinations behind one stall -- more than the four slots of the staging ring, so the
    fifth call may block on the first one's copy (the documented exception: the return check covers the first four).  M is overwritten after each return.
    cold (a stream, run_cold): no warm-up call, no stall, no return-time or allocation-count assertion; the results and the bands are checked as ever."""
    import remap_model as rm
    if cold is not None:
        stalled = live_stays = False
    torch, st, hip_ctx = env.torch, cold if cold is not None else stall.stream, env.ctx
    plan = env.plan()
    n = len(dests)
    Ms = [_warp_matrices(wo, ho, n)[j] for j, (wo, ho, so) in enumerate(dests)]
    frames = [content(j % 2) for j in range(n)]          # X1, X2 alternate in the one input buffer; D is the decoy
    exp = [maps_img([rm.warp_inverse(i, Ms[j], dests[j][0], dests[j][1], rm.BILINEAR, 9) for i in frames[j]], strict=True, S=dests[j][2]) for j in range(n)]
    decoy = [maps_img([rm.warp_inverse(i, Ms[j], dests[j][0], dests[j][1], rm.BILINEAR, 9) for i in content(2)], strict=True, S=dests[j][2]) for j in range(n)]
    for j in range(n):
        assert differs(exp[j], decoy[j]) and all(differs(exp[j], exp[i]) for i in range(j) if dests[i] == dests[j])
    stage = [env.stage(x) for x in frames_in([content(k) for k in range(3)])]
    d_in = env.buf(N_FRAMES)
    outs = [env.buf(F * ho * so) for wo, ho, so in dests]
    M = np.zeros((2, 3), np.float32)          # the host array the call reads
    d_in.copy_(stage[2])
    torch.cuda.synchronize()
    if cold is None:
        M[:] = Ms[0]
        plan.warp_inverse(d_in.data_ptr(), M, rm.BILINEAR, outs[0].data_ptr(), dests[0][0], dests[0][1], dests[0][2], 9, st.cuda_stream)
        torch.cuda.synchronize()
        outs[0].fill_(SENTINEL)
        torch.cuda.synchronize()
    live = hip_ctx.live_allocations()
    t0 = stall.enqueue() if stalled else time.perf_counter()          # not stalled: only to measure the enqueue section on an idle stream
    for j in range(n):
        with torch.cuda.stream(st):
            d_in.copy_(stage[j % 2], non_blocking=True)
        M[:] = Ms[j]
        plan.warp_inverse(d_in.data_ptr(), M, rm.BILINEAR, outs[j].data_ptr(), dests[j][0], dests[j][1], dests[j][2], 9, st.cuda_stream)
        M[:] = ((0.0, 1.0, 5.0), (1.0, 0.0, -3.0))
        if stalled and live_stays and j < 4:
            assert stall.pending(), "warp_inverse: call %d returned only after the stall had ended (%.2f ms since it was enqueued)" % (j + 1, (time.perf_counter() - t0) * 1e3)
            assert (time.perf_counter() - t0) * 1e3 <= STALL_MS / 4, "warp_inverse: stall too short"
    with torch.cuda.stream(st):
        d_in.copy_(stage[2], non_blocking=True)
    spent = time.perf_counter() - t0
    if stalled:
        stall.finish("warp_inverse")
    torch.cuda.synchronize()
    for j in range(n):
        others = {"the decoy's": decoy[j]}
        others.update({"matrix %d's" % (i + 1): exp[i] for i in range(n) if i != j and dests[i] == dests[j]})
        compare(outs[j].cpu().numpy(), exp[j], others, "warp_inverse: destination of call %d" % (j + 1))
    assert torch.equal(d_in, stage[2]), "warp_inverse: the last copy into the input did not land behind the calls"
    env.bands("warp_inverse")
    if live_stays:
        assert hip_ctx.live_allocations() == live, "warp_inverse: %d allocations, %d after the warm-up" % (hip_ctx.live_allocations(), live)
    return spent


@case
def warp_inverse(env):
    """six matrices behind one stall"""
    return SimpleNamespace(custom=lambda e, stall, **kw: _warp(e, stall, [REMAP_OUT] * 6, True, **kw))


@case
def warp_inverse_growth(env):
    """a larger destination makes the plan's table buffer reallocate while the first call is still pending; blocking is allowed, both results must be right"""
    return SimpleNamespace(custom=lambda e, stall, **kw: _warp(e, stall, [REMAP_OUT, (201, 150, 208)], False, **kw))
