"""What the ORB-pyramid GPU test shares with the content-sequence test: the frame batch of a geometry, and the pyramid handle with its guarded buffers
and its checks against tests/orb_pyramid_model.py."""
import functools

import numpy as np

import fast_model as fm
import orb_model as om
from fixtures import load_golden
from gpu_support import SENTINEL, Arena, d2h, pad_frames, ptr

G, A = load_golden("golden_orb_pyramid")
GOLD_100x90 = next(i for i, c in enumerate(G["pyramids"]) if (c["W"], c["H"]) == (100, 90))
KREC = om.KEYPOINT_DTYPE.itemsize
F = 3
THRESHOLD = 20


@functools.lru_cache(maxsize=None)
def batch(W, H):
    seed0 = G["pyramids"][GOLD_100x90]["seed"] if (W, H) == (100, 90) else 600 + W          # frame 0 of 100 x 90 is the golden case's frame
    v = np.stack([fm.noise(W, H, seed0), fm.blocks(W, H, seed0 + 1), om.constant(W, H, 97)])
    v.setflags(write=False)
    return v


def opts_of(levels, sf, mf, threshold=THRESHOLD):
    from compv_amd import capi
    return capi.OrbPyramidOpts(levels, sf, threshold, 9, True, mf)


class Rig:
    def __init__(self, hip_ctx, geom, key_cap, corner_cap=8192, desc_stride=32, threshold=THRESHOLD):
        from compv_amd import capi
        W, H, S, levels, sf, mf = geom
        self.geom, self.key_cap, self.desc_stride, self.levels = geom, key_cap, desc_stride, levels
        self.ar = Arena()
        self.valid = batch(W, H)
        self.host_in = pad_frames(self.valid, S, np.random.default_rng(W + H))
        self.d_in = self.ar.new(self.host_in.size, self.host_in.reshape(-1))
        self.ar.keep(self.d_in, self.host_in)
        self.d_keys = self.ar.new(F * key_cap * KREC)
        self.d_kcounts = self.ar.new(4 * F)
        self.d_lcounts = self.ar.new(4 * F * levels)
        self.d_lcorners = self.ar.new(4 * F * levels)
        self.d_desc = self.ar.new(F * key_cap * desc_stride)
        self.pyr = capi.OrbPyramid(hip_ctx, W, H, S, F, opts_of(levels, sf, mf, threshold), corner_cap)

    def set_content(self, valid, rng):
        """other frames [F][H][W] for the next calls on the same handle"""
        self.valid = valid
        self.host_in = pad_frames(valid, self.geom[2], rng)
        self.ar.reload(self.d_in, self.host_in)

    def close(self):
        self.pyr.close()

    def detect(self, key_cap=None, stream=0):
        cap = self.key_cap if key_cap is None else key_cap
        self.pyr.detect(ptr(self.d_in), ptr(self.d_keys) if cap else 0, cap, ptr(self.d_kcounts), ptr(self.d_lcounts), ptr(self.d_lcorners), stream)

    def ints(self, t, shape):
        return np.frombuffer(t.cpu().numpy().tobytes(), np.int32).reshape(shape)

    def check_detect(self, what, exp, key_cap=None):
        cap = self.key_cap if key_cap is None else key_cap
        self.ar.check(what)
        raw = self.d_keys.cpu().numpy().tobytes()
        counts, lc, lk = self.ints(self.d_kcounts, F), self.ints(self.d_lcounts, (F, self.levels)), self.ints(self.d_lcorners, (F, self.levels))
        for f in range(F):
            keys, e_lc, e_lk, _ = exp[f]
            assert lk[f].tolist() == e_lk.tolist(), "%s: frame %d FAST counts per level" % (what, f)
            assert lc[f].tolist() == e_lc.tolist(), "%s: frame %d survivors per level" % (what, f)
            assert counts[f] == len(keys) == e_lc.sum(), "%s: frame %d count %d, model %d" % (what, f, counts[f], len(keys))
            n = min(len(keys), cap)
            lo = f * cap * KREC
            assert raw[lo:lo + n * KREC] == keys[:n].tobytes(), "%s: frame %d records" % (what, f)
            assert raw[lo + n * KREC:lo + cap * KREC] == bytes([SENTINEL]) * ((cap - n) * KREC), "%s: frame %d wrote behind its records" % (what, f)

    def rows(self, t=None):
        return (self.d_desc if t is None else t).cpu().numpy().reshape(F, self.key_cap, self.desc_stride)

    def check_rows(self, what, got, exp_rows, counts):
        for f in range(F):
            n = min(counts[f], self.key_cap)
            assert (got[f, :n, :32] == exp_rows[f][:n]).all(), "%s: frame %d rows" % (what, f)
            assert (got[f, :n, 32:] == SENTINEL).all() and (got[f, n:] == SENTINEL).all(), "%s: frame %d wrote outside its rows" % (what, f)

    def level_planes(self, l, geo, blurred=False):
        g = geo[l]
        S = self.geom[2] if l == 0 else g["S"]
        return d2h(self.pyr.plane(l, blurred), F * g["H"] * S).reshape(F, g["H"], S)[:, :, :g["W"]]
