"""The GPU tests' shared kit: guarded and poisoned device buffers, frame generators, the oracle's expectations of a frame, the comparers, and the sizes of
the C records.  Not a test module, so its asserts are not rewritten: each carries its own message.  Importing it loads neither torch nor
libcompv_hip.so and touches no device (tests/test_support_layout.py): both are imported inside the functions that need them."""
import concurrent.futures as cf
import contextlib

import numpy as np

from hysteresis_cases import BAND, text_frame   # BAND: also the width of the sentinel bands of the stream-order and pointer-alignment buffers
from oracle_bindings import synth_frame

LINE_BYTES, SEG_BYTES, FIT_BYTES, COMP_BYTES = 20, 24, 80, 28          # the C records of include/compv_hip.h: line, segment, line fit, component


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


GUARD = 4096
SENTINEL = 0xA5
LINE_CAP = 4096
KEY_CAP = 65536          # lines beyond max(lineCap, 65536) per frame make the plan's line set an arbitrary subset (compv_hip.h)
T_LOW, T_HIGH = 59.0, 119.0


# ---------------------------------------------------------------------------------------------------------------
# guarded, poisoned device buffers
# ---------------------------------------------------------------------------------------------------------------
class Arena:
    """Device buffers as uint8 tensors with a guard pattern before and after; check() verifies every guard and every input
    registered with keep() (which must be unchanged)."""

    def __init__(self):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.pattern = ((torch.arange(GUARD, dtype=torch.int32) * 167 + 89) & 0xff).to(torch.uint8).to(self.dev)
        self.bufs = []
        self.kept = []

    def new(self, nbytes, fill=SENTINEL):
        raw = self.torch.empty(nbytes + 2 * GUARD, dtype=self.torch.uint8, device=self.dev)
        raw[:GUARD] = self.pattern
        raw[GUARD + nbytes:] = self.pattern
        body = raw[GUARD:GUARD + nbytes]
        if isinstance(fill, np.ndarray):
            assert fill.dtype == np.uint8 and fill.size == nbytes, "fill: %s, %d bytes for a buffer of %d" % (fill.dtype, fill.size, nbytes)
            body.copy_(self.torch.from_numpy(np.ascontiguousarray(fill).reshape(-1)))
        else:
            body.fill_(fill)
        self.bufs.append(raw)
        return body

    def keep(self, body, host):
        self.kept.append((body, np.ascontiguousarray(host).reshape(-1).copy()))

    def refill(self, body, fill=SENTINEL):
        body.fill_(fill)

    def reload(self, body, host):
        """new content for a buffer registered with keep(): the device bytes, and the copy check() holds them against"""
        h = np.ascontiguousarray(host).view(np.uint8).reshape(-1).copy()
        assert h.size == body.numel() and any(b is body for b, _ in self.kept), "reload: %d bytes for a kept buffer of %d" % (h.size, body.numel())
        body.copy_(self.torch.from_numpy(h))
        self.torch.cuda.synchronize()
        self.kept = [(b, h if b is body else old) for b, old in self.kept]

    def check(self, what):
        self.torch.cuda.synchronize()
        for raw in self.bufs:
            assert self.torch.equal(raw[:GUARD], self.pattern), "%s: guard before a buffer overwritten" % what
            assert self.torch.equal(raw[-GUARD:], self.pattern), "%s: guard after a buffer overwritten" % what
        for body, host in self.kept:
            assert (body.cpu().numpy() == host).all(), "%s: input modified" % what


@contextlib.contextmanager
def alloc_fill(byte):
    """compvhip_debug_alloc_fill for the length of the block: every device or pinned block the library allocates inside it is filled with `byte`
    (None: the hook is left alone).  The hook is process-wide; the previous value is restored whatever happens inside"""
    if byte is None:
        yield
        return
    from compv_amd import capi
    L = capi.load()
    prev = L.compvhip_debug_alloc_fill(int(byte))
    assert -1 <= prev <= 255, "compvhip_debug_alloc_fill(%r) returned %d" % (byte, prev)
    try:
        yield
    finally:
        L.compvhip_debug_alloc_fill(prev)


def ptr(t):
    return t.data_ptr()


def frames_view(body, F, H, S, W):
    """(F, H, W) host copy of the valid region of a [F][H][S] device buffer."""
    return body.cpu().numpy().reshape(F, H, S)[:, :, :W]


def d2h(dptr, nbytes):
    """Device -> host copy of memory the plan owns (the edge counts)."""
    import ctypes as C
    import torch
    from compv_amd import capi
    L = capi.load()
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(nbytes, np.uint8)
    torch.cuda.synchronize()
    rc = L.hipMemcpy(out.ctypes.data, dptr, nbytes, 2)          # hipMemcpyDeviceToHost
    assert rc == 0, "hipMemcpy returned %d, expected 0" % rc
    return out


def pad_frames(valid, row_bytes, rng):
    """[F][H][Wb] valid bytes -> [F][H][row_bytes] whose padding holds seeded random bytes, with a 255 in one padding column of every row."""
    F, H, Wb = valid.shape
    out = rng.integers(0, 256, (F, H, row_bytes), dtype=np.uint8)
    if row_bytes > Wb:
        out[:, :, Wb + rng.integers(0, row_bytes - Wb)] = 255
    out[:, :, :Wb] = valid
    return out


# ---------------------------------------------------------------------------------------------------------------
# frame content
# ---------------------------------------------------------------------------------------------------------------
def checker_frame(W, H, seed):
    c = 3 + seed % 7
    x = np.arange(W)[None, :] // c
    y = np.arange(H)[:, None] // c
    return (((x + y) & 1) * 255).astype(np.uint8)


KINDS = ("synth", "noise", "zero", "text", "checker")   # the all-zero frame sits between two dense ones


def make_frame(kind, W, H, seed):
    if kind == "synth":
        return synth_frame(W, H, seed)
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)
    if kind == "zero":
        return np.zeros((H, W), np.uint8)
    if kind == "text":
        return text_frame(W, H, seed)
    return checker_frame(W, H, seed)


def make_batch(W, H, F, seed):
    return np.stack([make_frame(KINDS[(seed + f) % len(KINDS)], W, H, seed * 1000 + f) for f in range(F)])


def rgb_of(img):
    b = img.astype(np.int32)
    return np.stack([np.clip(b + 20, 0, 255), b * 3 // 4, 255 - b], axis=-1).astype(np.uint8)


def rgb565le_of(img):
    b = img.astype(np.uint16)
    v = ((b >> 3) << 11) | ((b >> 2) << 5) | ((255 - b) >> 3)
    return np.stack([v & 0xff, v >> 8], axis=-1).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------
# oracle side, one frame at a time on a thread pool (ctypes releases the GIL inside the oracle)
# ---------------------------------------------------------------------------------------------------------------
def pool():
    from compv_amd import capi
    return cf.ThreadPoolExecutor(max_workers=max(1, min(16, capi.host_cpu_budget())))


def canny_expect(orc, img, ksize, mode, tl, th):
    from compv_amd import capi
    if mode == capi.THRESHOLD_OTSU:
        lo, hi = orc.otsu_canny_thresholds(orc.otsu(img), tl, th)
        rc, e = orc.canny(img, float(lo), float(hi), ksize)
    else:
        rc, e = orc.canny(img, tl, th, ksize, mode)
    assert rc == 0, rc
    return e


def sht_expect(orc, edges, theta, thr):
    H, W = edges.shape
    acc = orc.sht_acc(edges, theta)
    return acc, orc.sht_lines_from_acc(acc, W, H, theta, thr)


def canny_modes():
    from compv_amd import capi
    return [(3, capi.THRESHOLD_COMPARE_TO_GRADIENT, T_LOW, T_HIGH), (3, capi.THRESHOLD_PERCENT_OF_MEAN, 0.68, 1.36), (3, capi.THRESHOLD_OTSU, 0.5, 1.0),
            (5, capi.THRESHOLD_COMPARE_TO_GRADIENT, 400.0, 900.0), (5, capi.THRESHOLD_PERCENT_OF_MEAN, 0.68, 1.36), (5, capi.THRESHOLD_OTSU, 0.5, 1.0)]


def sht_threshold(W, H):
    return max(3, min(W, H) // 2)


def frame_expectations(orc, img, theta, want_kht, gauss):
    from compv_amd import capi
    H, W = img.shape
    thr = sht_threshold(W, H)
    x = {"dete": {op: orc.edge_dete(img, op)[0] for op in (capi.OP_SOBEL, capi.OP_SCHARR, capi.OP_PREWITT)}}
    x["canny"] = {m[:2]: canny_expect(orc, img, *m) for m in canny_modes()}
    e3 = x["canny"][(3, capi.THRESHOLD_COMPARE_TO_GRADIENT)]
    x["sht"] = sht_expect(orc, e3, theta, thr)
    x["sht5"] = sht_expect(orc, x["canny"][(5, capi.THRESHOLD_PERCENT_OF_MEAN)], theta, thr)[1]
    x["otsu_y"] = int(orc.otsu(img))
    gray = orc.grayscale(rgb_of(img).reshape(H, W * 3), capi.FMT_RGB24, W)
    lo, hi = orc.otsu_canny_thresholds(orc.otsu(gray), 0.5, 1.0)
    rc, eg = orc.canny(gray, float(lo), float(hi))
    assert rc == 0, "oracle canny returned %d, expected 0" % rc
    x["rgb"] = (gray, int(orc.otsu(gray)), eg, sht_expect(orc, eg, theta, thr)[1])
    g565 = orc.grayscale(rgb565le_of(img).reshape(H, W * 2), capi.FMT_RGB565LE, W)
    x["565"] = (g565, int(orc.otsu(g565)))
    rc, x["gauss"] = orc.convlt_fxp(img, gauss, gauss)
    assert rc == 0, "oracle convlt_fxp returned %d, expected 0" % rc
    if want_kht:
        x["kht"] = orc.kht(e3, 1.0, theta, 12)
    return x


def lines_of(raw_f, n):
    from compv_amd import capi
    return np.frombuffer(raw_f[:n].tobytes(), dtype=capi.LINE_DTYPE)


def assert_lines(raw, counts, exp, what):
    """raw: (F, cap, 20) bytes; counts: int32[F]; exp: per-frame oracle lines in canonical order."""
    for f, e in enumerate(exp):
        assert int(counts[f]) == len(e), (what, f, int(counts[f]), len(e))
        assert len(e) <= KEY_CAP, (what, f, len(e))                      # otherwise the test itself would be out of contract
        n = min(len(e), raw.shape[1])
        got = lines_of(raw[f], n)
        assert [(float(l["rho"]), float(l["theta"]), int(l["strength"]), int(l["row"]), int(l["col"])) for l in got] == \
               [(float(np.float32(l[0])), float(np.float32(l[1])), int(l[2]), int(l[3]), int(l[4])) for l in e[:n]], (what, f)


def assert_maps(got, exp, what):
    for f, e in enumerate(exp):
        if not (got[f] == e).all():
            ys, xs = np.nonzero(got[f] != e)
            raise AssertionError("%s: frame %d differs at %d pixels, first (y=%d, x=%d): got %d, expected %d"
                                 % (what, f, len(ys), ys[0], xs[0], got[f][ys[0], xs[0]], e[ys[0], xs[0]]))


def check_accs(plan, arena, F, R, T, exp_accs, what):
    d_acc = arena.new(R * T * 4)
    for f in range(F):
        arena.refill(d_acc)
        plan.acc_export(f, ptr(d_acc), T)
        arena.check("%s acc_export %d" % (what, f))
        got = d_acc.cpu().numpy().view(np.int32).reshape(R, T)
        assert (got == exp_accs[f]).all(), (what, f, int((got != exp_accs[f]).sum()))


def edge_counts(plan, F):
    """compvhip_plan_edge_counts: counted by the SHT's voting kernel, so meaningful after an SHT or a pipeline step."""
    return d2h(plan.edge_counts_ptr(), 4 * F).view(np.int32)
