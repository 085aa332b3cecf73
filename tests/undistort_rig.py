"""The undistortion GPU tests' rig (tests/test_gpu_undistort.py, tests/test_gpu_fresh_memory.py): a handle between guarded buffers, the model's windows
and the whole-buffer comparison.  Not a test module: every assert carries its own message."""
import numpy as np

import undistort_cases as uc
import undistort_model as um
from gpu_support import SENTINEL, Arena, ptr, u8

F32_OUT = (2, 5)          # COMPVHIP_INTERP_BILINEAR_FLOAT32, _BICUBIC_FLOAT32
_MODEL = {}


def model_image(c, interp, k=0, K=None, d=None):
    """the model's window of frame k of the case (computed once per process)"""
    key = (c["id"], interp, k, None if K is None else np.asarray(K).tobytes() + np.asarray(d).tobytes())
    if key not in _MODEL:
        wo, ho = c["size"][2:]
        _MODEL[key] = um.undistort(uc.frame(c, k), c["K"] if K is None else K, c["d"] if d is None else d, wo, ho, *c["origin"], interp=interp, roi=c["roi"], default=c["default"])
    return _MODEL[key]


def padded_frames(c, count, S, seed=5):
    """[count][H][S] with seeded random padding"""
    w, h = c["size"][:2]
    out = np.random.default_rng(seed).integers(0, 256, (count, h, S), dtype=np.uint8)
    for k in range(count):
        out[k, :, :w] = uc.frame(c, k)
    return out


def expect_buffer(planes, Sout):
    """the bytes of [F][Hout][Sout] elements: the planes, and the sentinel wherever nothing may be written"""
    Ho, Wo = planes[0].shape
    item = planes[0].itemsize
    buf = np.full((len(planes), Ho, Sout * item), SENTINEL, np.uint8)
    for f, p in enumerate(planes):
        buf[f, :, :Wo * item] = np.ascontiguousarray(p).view(np.uint8).reshape(Ho, Wo * item)
    return buf.reshape(-1)


def same_bytes(body, exp, what):
    got = body.cpu().numpy()
    bad = np.flatnonzero(got != exp)
    assert not bad.size, "%s: %d bytes differ, first at %d: got %d, expected %d" % (what, bad.size, bad[0], got[bad[0]], exp[bad[0]])


class Rig:
    """An undistort handle over `count` frames of a case, its guarded source and a destination with room for any layout"""

    def __init__(self, ctx, c, count=1, pad=7, stream=0, max_sets=0, max_points=0):
        from compv_amd import capi
        self.capi, self.c, self.count = capi, c, count
        w, h, wo, ho = c["size"]
        self.S = max(w + pad, 4)
        self.ar = Arena()
        self.src = padded_frames(c, count, self.S)
        self.d_in = self.ar.new(self.src.size, u8(self.src))
        self.ar.keep(self.d_in, u8(self.src))
        self.d_out = self.ar.new(count * ho * (wo + 16) * 4 + 32)
        self.h = capi.Undistort(ctx, w, h, self.S, count, wo, ho, *c["origin"], max_sets=max_sets, max_points=max_points, stream=stream)

    def run(self, interp, K, d, Sout, offset=0, roi="case", default=None):
        c = self.c
        self.ar.refill(self.d_out)
        self.h.undistort(ptr(self.d_in), K, d, interp, ptr(self.d_out) + offset, Sout, c["roi"] if roi == "case" else roi, c["default"] if default is None else default)

    def check(self, what, planes, Sout, offset=0):
        self.ar.check(what)          # (synchronises the device)
        exp = np.full(self.d_out.numel(), SENTINEL, np.uint8)
        body = expect_buffer(planes, Sout)
        exp[offset:offset + body.size] = body
        same_bytes(self.d_out, exp, what)

    def close(self):
        self.h.close()


def layouts(wo, interp):
    """(name, Sout, byte offset of the destination): one that takes the vector stores, one that cannot"""
    if interp in F32_OUT:
        return (("vector", (wo + 3) // 4 * 4 + 4, 0), ("element", wo + 1, 4))
    return (("vector", (wo + 3) // 4 * 4 + 4, 0), ("element", wo + 3, 1))


def maps_of(rig, K, d, count, T, ar, offset=0):
    """compvhip_undistort_maps into fresh guarded buffers -> (x bytes, y bytes, the device tensors)"""
    wo, ho = rig.c["size"][2:]
    n = count * wo * ho * np.dtype(T).itemsize
    dx, dy = ar.new(n + 64), ar.new(n + 64)
    rig.h.maps(K, d, ptr(dx) + offset, ptr(dy) + offset, rig.capi.UNDISTORT_F32 if T is np.float32 else rig.capi.UNDISTORT_F64)
    ar.check("maps")
    for t in (dx, dy):
        raw = t.cpu().numpy()
        assert (raw[:offset] == SENTINEL).all() and (raw[offset + n:] == SENTINEL).all(), "the map call wrote outside its planes"
    return dx.cpu().numpy()[offset:offset + n], dy.cpu().numpy()[offset:offset + n], dx, dy


def point_rig(hip_ctx, max_sets, max_points, stream=0):
    return Rig(hip_ctx, uc.case("one"), max_sets=max_sets, max_points=max_points, stream=stream)
