"""What the RANSAC-homography GPU test shares with the content-sequence test: the handle with its guarded buffers and its checks against
tests/homography_model.py."""
import numpy as np

import homography_model as hm
from gpu_support import SENTINEL, Arena, ptr, u8

REC = hm.RESULT_DTYPE.itemsize


class Rig:
    """A homography handle and its guarded buffers.  sets: per pair (src [k][2], dst [k][2]); counts: the device counts (None: a NULL pointer)."""

    def __init__(self, hip_ctx, sets, point_cap, max_tries, counts="own", quads=None):
        from compv_amd import capi
        self.pairs, self.cap, self.max_tries = len(sets), point_cap, max_tries
        rng = np.random.default_rng(point_cap * 7 + len(sets))
        self.src = rng.uniform(-1e6, 1e6, (self.pairs, point_cap, 2))          # junk behind every pair's points
        self.dst = rng.uniform(-1e6, 1e6, (self.pairs, point_cap, 2))
        for p, (s, d) in enumerate(sets):
            n = min(len(s), point_cap)
            self.src[p, :n], self.dst[p, :n] = s[:n], d[:n]
        self.counts = [len(s) for s, _ in sets] if isinstance(counts, str) else counts
        self.ar = Arena()
        self.d_src, self.d_dst = self.ar.new(self.src.nbytes, u8(self.src)), self.ar.new(self.dst.nbytes, u8(self.dst))
        self.ar.keep(self.d_src, u8(self.src))
        self.ar.keep(self.d_dst, u8(self.dst))
        self.d_counts = None
        if self.counts is not None:
            h = u8(np.asarray(self.counts, np.int32))
            self.d_counts = self.ar.new(h.size, h)
            self.ar.keep(self.d_counts, h)
        self.d_res = self.ar.new(self.pairs * REC)
        self.d_mask = self.ar.new(self.pairs * point_cap)
        self.h = capi.Homography(hip_ctx, self.pairs, point_cap, max_tries)

    def set_points(self, src, dst, counts):
        """other points and device counts for the next calls on the same handle: src, dst [pairs][pointCap][2] (a rig made with a count array)"""
        self.src, self.dst, self.counts = src, dst, list(counts)
        self.ar.reload(self.d_src, u8(src))
        self.ar.reload(self.d_dst, u8(dst))
        self.ar.reload(self.d_counts, u8(np.asarray(counts, np.int32)))

    def k(self, p):
        return self.cap if self.counts is None else max(0, min(int(self.counts[p]), self.cap))

    def quads_buffer(self, quads):
        h = u8(np.asarray(quads, np.int32))
        d = self.ar.new(h.size, h)
        self.ar.keep(d, h)
        return d

    def run(self, tries, d_quads=None, stream=0, mask=True, **opts):
        self.ar.refill(self.d_res)
        self.ar.refill(self.d_mask)
        self.h.find(ptr(self.d_src), ptr(self.d_dst), ptr(self.d_counts) if self.d_counts is not None else 0, ptr(self.d_res), ptr(self.d_mask) if mask else 0,
                    tries=tries, d_quads=ptr(d_quads) if d_quads is not None else 0, stream=stream, **opts)

    def outputs(self, what, tries):
        self.ar.check(what)
        res = np.frombuffer(self.d_res.cpu().numpy().tobytes(), hm.RESULT_DTYPE)
        mask = self.d_mask.cpu().numpy().reshape(self.pairs, self.cap)
        return res, mask, self.h.scores(tries)

    def check(self, what, tries, expected, mask=True):
        """expected: per pair a dict as homography_model.find returns (result, mask, counts, variances, rotations)"""
        res, got_mask, (counts, var, rot) = self.outputs(what, tries)
        for p, e in enumerate(expected):
            k = self.k(p)
            assert res[p].tobytes() == e["result"].tobytes(), "%s: pair %d record %r, model %r" % (what, p, res[p], e["result"])
            if mask:
                assert got_mask[p, :k].tobytes() == np.asarray(e["mask"], np.uint8).tobytes(), "%s: pair %d mask" % (what, p)
                assert (got_mask[p, k:] == SENTINEL).all(), "%s: pair %d wrote mask bytes at or after k" % (what, p)
            else:
                assert (got_mask[p] == SENTINEL).all(), "%s: pair %d: %d mask bytes written although no mask was passed" % (what, p, int((got_mask[p] != SENTINEL).sum()))
            if e["counts"] is not None:
                assert counts[p].tolist() == np.asarray(e["counts"]).tolist(), "%s: pair %d per-try counts" % (what, p)
                assert var[p].tobytes() == np.ascontiguousarray(e["variances"], np.float64).tobytes(), "%s: pair %d per-try variance bits" % (what, p)
                assert rot[p].tolist() == np.asarray(e["rotations"]).tolist(), "%s: pair %d per-try rotations" % (what, p)
        return res

    def model(self, tries, quads=None, **opts):
        return [hm.find(self.src[p], self.dst[p], self.k(p), tries, pair=p, quad_list=None if quads is None else quads[p], **opts) for p in range(self.pairs)]

    def close(self):
        self.h.close()
