"""What the ORB GPU test shares with the content-sequence and stream-order tests: the frame batches, the made-up corner lists, and the plan with its
guarded buffers and its checks against tests/orb_model.py."""
import functools

import numpy as np

import fast_model as fm
import orb_model as om
from gpu_support import SENTINEL, Arena, pad_frames, ptr

SURVIVORS = (257, 1, 0, 63, 64, 65)
KREC, CREC = om.KEYPOINT_DTYPE.itemsize, om.CORNER_DTYPE.itemsize
KINDS = ("noise", "blocks", "constant", "ramp", "mirrored")


def make_frame(kind, W, H, seed):
    if kind == "noise":
        return fm.noise(W, H, seed)
    if kind == "blocks":
        return fm.blocks(W, H, seed)
    if kind == "constant":
        return om.constant(W, H, 40 + seed % 200)
    if kind == "ramp":
        return om.ramp(W, H)
    return om.mirrored(fm.noise(W, H, seed))


@functools.lru_cache(maxsize=None)
def batch(W, H, F, seed):
    v = np.stack([make_frame(KINDS[f % len(KINDS)], W, H, seed * 100 + f) for f in range(F)])
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def blurred_batch(W, H, F, seed):
    v = np.stack([om.blur(img) for img in batch(W, H, F, seed)])
    v.setflags(write=False)
    return v


def corner_list(W, H, survivors, seed):
    """`survivors` admissible corners in a list that also holds inadmissible ones, in a seeded order"""
    rng = np.random.default_rng(seed)
    b = om.BORDER
    good = [(b, b), (W - b - 1, b), (b, H - b - 1), (W - b - 1, H - b - 1), (W // 2, H // 2), (W // 2, b)]
    bad = [(b - 1, H // 2), (W - b, H // 2), (W // 2, b - 1), (W // 2, H - b), (0, 0), (W - 1, H - 1), (b - 1, b - 1)]
    while len(good) < survivors:
        good.append((int(rng.integers(b, W - b)), int(rng.integers(b, H - b))))
    good = good[:survivors]
    for _ in range(survivors // 3):
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        if not om.admissible(x, y, W, H):
            bad.append((x, y))
    pts = [(p, True) for p in good] + [(p, False) for p in bad]
    order = rng.permutation(len(pts))
    c = np.zeros(len(pts), om.CORNER_DTYPE)
    for i, j in enumerate(order):
        c[i] = (pts[j][0][0], pts[j][0][1], int(rng.integers(0, 255)))
    admitted = int(om.admissible(c["x"], c["y"], W, H).sum())
    assert admitted == survivors, "corner_list: %d admissible corners, %d wanted" % (admitted, survivors)
    return c


def u8(a):
    """the bytes of an array as a writable uint8 array"""
    return np.frombuffer(a.tobytes(), np.uint8).copy()


class Rig:
    """a plan with guarded frames, corner lists and counts, keypoints, key counts, moments and descriptor rows of one geometry"""

    def __init__(self, hip_ctx, geom, seed, key_cap, desc_stride=32):
        from compv_amd import capi
        W, H, S, F = geom
        self.geom, self.key_cap, self.desc_stride = geom, key_cap, desc_stride
        self.ar = Arena()
        self.valid = batch(W, H, F, seed)
        self.host_in = pad_frames(self.valid, S, np.random.default_rng(seed + 1))
        self.d_in = self.ar.new(F * H * S, self.host_in)
        self.ar.keep(self.d_in, self.host_in)
        self.lists = [corner_list(W, H, SURVIVORS[(f + W) % len(SURVIVORS)], seed * 1000 + f) for f in range(F)]
        self.corner_cap = max(len(c) for c in self.lists) + 3
        host_c = np.zeros((F, self.corner_cap), om.CORNER_DTYPE)
        rng = np.random.default_rng(seed + 2)
        host_c["x"], host_c["y"] = rng.integers(0, W, host_c.shape), rng.integers(0, H, host_c.shape)          # behind a list: corners that must not be read
        counts = np.zeros(F, np.int32)
        for f, c in enumerate(self.lists):
            host_c[f, :len(c)] = c
            counts[f] = len(c)
        if F >= 5:          # a count above cornerCap (the whole row is the list) and a negative one (an empty list)
            self.lists[F - 2] = host_c[F - 2].copy()
            counts[F - 2] = self.corner_cap + 50
            self.lists[F - 1] = host_c[F - 1, :0].copy()
            counts[F - 1] = -5
        self.d_corners = self.ar.new(host_c.nbytes, u8(host_c))
        self.ar.keep(self.d_corners, u8(host_c))
        self.d_ccounts = self.ar.new(4 * F, u8(counts))
        self.ar.keep(self.d_ccounts, u8(counts))
        self.d_keys = self.ar.new(F * key_cap * KREC)
        self.d_kcounts = self.ar.new(4 * F)
        self.d_moments = self.ar.new(F * key_cap * 8)
        self.d_desc = self.ar.new(F * key_cap * desc_stride)
        self.plan = capi.Plan(hip_ctx, W, H, S, F)

    def set_content(self, valid, rng, corner_counts=None):
        """other frames [F][H][W] (and device corner counts: a prefix of every frame's list) for the next calls on the same plan"""
        self.valid = valid
        self.host_in = pad_frames(valid, self.geom[2], rng)
        self.ar.reload(self.d_in, self.host_in)
        if corner_counts is not None:
            if not hasattr(self, "full_lists"):
                self.full_lists = [c.copy() for c in self.lists]
            self.lists = [c[:n] for c, n in zip(self.full_lists, corner_counts)]
            self.ar.reload(self.d_ccounts, np.asarray([len(c) for c in self.lists], np.int32))

    def expected(self, level, scale):
        return [om.keypoints(self.valid[f], self.lists[f], level, scale) for f in range(self.geom[3])]

    def keypoints(self, level, scale, moments=True, key_cap=None, stream=0):
        cap = self.key_cap if key_cap is None else key_cap
        self.plan.orb_keypoints(ptr(self.d_in), ptr(self.d_corners), self.corner_cap, ptr(self.d_ccounts), level, float(scale), ptr(self.d_keys) if cap else 0, cap,
                                ptr(self.d_kcounts), ptr(self.d_moments) if moments else 0, stream)

    def check_keypoints(self, what, exp, moments=True, key_cap=None):
        cap = self.key_cap if key_cap is None else key_cap
        self.ar.check(what)
        F = self.geom[3]
        raw, mom = self.d_keys.cpu().numpy().tobytes(), self.d_moments.cpu().numpy().tobytes()
        counts = np.frombuffer(self.d_kcounts.cpu().numpy().tobytes(), np.int32)
        for f in range(F):
            keys, m = exp[f]
            assert counts[f] == len(keys), "%s: frame %d count %d, model %d" % (what, f, counts[f], len(keys))
            n = min(len(keys), cap)
            lo = f * cap * KREC
            assert raw[lo:lo + n * KREC] == keys[:n].tobytes(), "%s: frame %d records" % (what, f)
            assert raw[lo + n * KREC:lo + cap * KREC] == bytes([SENTINEL]) * ((cap - n) * KREC), "%s: frame %d wrote behind its records" % (what, f)
            if moments:
                assert mom[f * cap * 8:f * cap * 8 + n * 8] == m[:n].tobytes(), "%s: frame %d moments" % (what, f)
                assert mom[f * cap * 8 + n * 8:(f + 1) * cap * 8] == bytes([SENTINEL]) * ((cap - n) * 8), "%s: frame %d wrote behind its moments" % (what, f)
        if not moments:
            assert mom == bytes([SENTINEL]) * len(mom), "%s: moments written although none were asked for" % what
        if not cap:
            assert raw == bytes([SENTINEL]) * len(raw), "%s: %d bytes of the record buffer written although its capacity is 0" % (what, sum(b != SENTINEL for b in raw))
        return raw, counts

    def describe(self, scale, blur=True, d_gray=None, stream=0):
        self.plan.orb_describe(ptr(self.d_in if d_gray is None else d_gray), ptr(self.d_keys), self.key_cap, ptr(self.d_kcounts), float(scale), ptr(self.d_desc),
                               self.desc_stride, blur, stream)

    def check_desc(self, what, keys_per_frame, scale, seed):
        """keys_per_frame[f]: the records that lie in d_keys for frame f (at most key_cap of them)"""
        self.ar.check(what)
        W, H, S, F = self.geom
        blurred = blurred_batch(W, H, F, seed)
        rows = self.d_desc.cpu().numpy().reshape(F, self.key_cap, self.desc_stride)
        for f in range(F):
            exp = om.describe(blurred[f], keys_per_frame[f][:self.key_cap], scale)
            n = len(exp)
            assert rows[f, :n, :32].tobytes() == exp.tobytes(), "%s: frame %d rows %s" % (what, f, np.nonzero((rows[f, :n, :32] != exp).any(axis=1))[0][:8])
            assert (rows[f, n:] == SENTINEL).all(), "%s: frame %d wrote behind its rows" % (what, f)
        assert (rows[:, :, 32:] == SENTINEL).all(), "%s: row padding written" % what
        return rows.copy()

    def refill(self):
        for b in (self.d_keys, self.d_kcounts, self.d_moments, self.d_desc):
            self.ar.refill(b)

    def close(self):
        self.plan.close()
