"""What the FAST GPU test shares with the content-sequence test: the frame batch, and the plan with its guarded buffers and its checks against
tests/fast_model.py."""
import numpy as np

import fast_model as fm
from gpu_support import SENTINEL, Arena, pad_frames, ptr

REC = fm.CORNER_DTYPE.itemsize


def batch(W, H, F, seed):
    kinds = (fm.noise, fm.blocks, fm.seam_noise, lambda w, h, s: np.full((h, w), (37 * s) & 0xff, np.uint8), fm.tied_arcs)
    return np.stack([kinds[(seed + f) % 5](W, H, seed * 100 + f) for f in range(F)])


class Rig:
    """A plan, a guarded input batch, a guarded score map, record array and count array of one geometry."""

    def __init__(self, hip_ctx, geom, seed, cap):
        from compv_amd import capi
        W, H, S, F = geom
        self.geom, self.cap = geom, cap
        self.ar = Arena()
        self.valid = batch(W, H, F, seed)
        self.host_in = pad_frames(self.valid, S, np.random.default_rng(seed + 1))
        self.d_in = self.ar.new(F * H * S, self.host_in)
        self.ar.keep(self.d_in, self.host_in)
        self.d_scores = self.ar.new(F * H * S)
        self.d_rec = self.ar.new(max(F * cap * REC, 8))
        self.d_counts = self.ar.new(4 * F)
        self.plan = capi.Plan(hip_ctx, W, H, S, F)

    def set_content(self, valid, rng):
        """other frames [F][H][W] for the next calls on the same plan; the padding columns get bytes of rng"""
        self.valid = valid
        self.host_in = pad_frames(valid, self.geom[2], rng)
        self.ar.reload(self.d_in, self.host_in)

    def run(self, N, nonmax, t, max_features=-1, scores=True, cap=None, stream=0):
        cap = self.cap if cap is None else cap
        self.plan.fast(ptr(self.d_in), t, N, nonmax, max_features, ptr(self.d_scores) if scores else 0, ptr(self.d_rec) if cap else 0, cap, ptr(self.d_counts), stream)

    def fetch(self, what):
        self.ar.check(what)
        W, H, S, F = self.geom
        return (self.d_scores.cpu().numpy().reshape(F, H, S), self.d_rec.cpu().numpy().tobytes(), np.frombuffer(self.d_counts.cpu().numpy().tobytes(), np.int32))

    def check(self, what, exp, scores=True, cap=None, cut=-1):
        """exp[f] = (records, score map) of the model without a cut; `cut` applies the canonical cut to the records"""
        cap = self.cap if cap is None else cap
        W, H, S, F = self.geom
        smap, raw, counts = self.fetch(what)
        for f in range(F):
            rec = fm.cut(exp[f][0], cut)
            assert counts[f] == len(rec), "%s: frame %d count %d, model %d" % (what, f, counts[f], len(rec))
            n = min(len(rec), cap)
            lo = f * cap * REC
            assert raw[lo:lo + n * REC] == rec[:n].tobytes(), "%s: frame %d records" % (what, f)
            assert raw[lo + n * REC:lo + cap * REC] == bytes([SENTINEL]) * ((cap - n) * REC), "%s: frame %d wrote behind its records" % (what, f)
            if scores:
                assert smap[f, :, :W].tobytes() == exp[f][1].tobytes(), "%s: frame %d score map" % (what, f)
        if scores:
            assert (smap[:, :, W:] == SENTINEL).all(), "%s: padding columns of the score map written" % what
        else:
            assert (smap == SENTINEL).all(), "%s: score map written although none was asked for" % what
        if not cap:
            assert raw == bytes([SENTINEL]) * len(raw), "%s: %d bytes of the record buffer written although its capacity is 0" % (what, sum(b != SENTINEL for b in raw))
        self.ar.refill(self.d_scores)
        self.ar.refill(self.d_rec)
        self.ar.refill(self.d_counts)
        return raw, counts

    def close(self):
        self.plan.close()
