"""The curve-fit GPU tests' rig (tests/test_gpu_curvefit.py, tests/test_gpu_fresh_memory.py): a handle between guarded buffers, and the hand-made
label maps of the gather.  Not a test module: every assert carries its own message where it needs one."""
import numpy as np

import curvefit_model as cm
from gpu_support import SENTINEL, Arena, ptr, u8

REC = cm.RESULT_DTYPE.itemsize
SENT64 = np.frombuffer(bytes([SENTINEL] * 8), np.float64)[0]


class Rig:
    """A curve-fit handle and its guarded buffers.  sets: per set its points [k][2]; counts: "own" (the device counts are the sets' sizes), a list, or
    None (a NULL pointer: every set has pointCap points)."""

    def __init__(self, hip_ctx, sets, point_cap, max_tries, counts="own", stream=0, upload=True):
        from compv_amd import capi
        self.n, self.cap, self.max_tries = len(sets), point_cap, max_tries
        rng = np.random.default_rng(point_cap * 7 + len(sets))
        self.pts = rng.uniform(-1e6, 1e6, (self.n, point_cap, 2))          # junk behind every set's points
        for s, p in enumerate(sets):
            n = min(len(p), point_cap)
            self.pts[s, :n] = np.asarray(p, np.float64).reshape(-1, 2)[:n]
        self.counts = [len(p) for p in sets] if isinstance(counts, str) else counts
        self.ar = Arena()
        self.d_pts = self.ar.new(self.pts.nbytes, u8(self.pts) if upload else SENTINEL)
        self.ar.keep(self.d_pts, u8(self.pts))
        self.d_counts = None
        if self.counts is not None:
            h = u8(np.asarray(self.counts, np.int32))
            self.d_counts = self.ar.new(h.size, h)
            self.ar.keep(self.d_counts, h)
        self.d_res = self.ar.new(self.n * REC)
        self.d_mask = self.ar.new(self.n * point_cap + 3)[3:]          # ANY BYTE: the mask starts at an odd address
        self.d_dist = self.ar.new(self.n * point_cap * 8)
        self.h = capi.Curvefit(hip_ctx, self.n, point_cap, max_tries, stream=stream)

    def k(self, s):
        return self.cap if self.counts is None else max(0, min(int(self.counts[s]), self.cap))

    def buffer(self, host):
        h = u8(host)
        d = self.ar.new(h.size, h)
        self.ar.keep(d, h)
        return d

    def run(self, model, tries, d_samples=None, mask=True, **opts):
        self.ar.refill(self.d_res)
        self.d_mask.fill_(SENTINEL)
        self.h.find(ptr(self.d_pts), ptr(self.d_counts) if self.d_counts is not None else 0, ptr(self.d_res), ptr(self.d_mask) if mask else 0, model=model, tries=tries,
                    d_samples=ptr(d_samples) if d_samples is not None else 0, **opts)

    def check(self, what, model, tries, expected, mask=True):
        """expected: per set a dict as curvefit_model.find returns (result, mask, counts)"""
        counts, _ = self.h.scores(tries)          # (waits for the handle's stream)
        self.ar.check(what)
        res = np.frombuffer(self.d_res.cpu().numpy().tobytes(), cm.RESULT_DTYPE)
        got_mask = self.d_mask.cpu().numpy().reshape(self.n, self.cap)
        for s, e in enumerate(expected):
            k = self.k(s)
            assert res[s].tobytes() == e["result"].tobytes(), "%s: set %d record %r, model %r" % (what, s, res[s], e["result"])
            if mask:
                assert got_mask[s, :k].tobytes() == np.asarray(e["mask"], np.uint8).tobytes(), "%s: set %d mask" % (what, s)
                assert (got_mask[s, k:] == SENTINEL).all(), "%s: set %d wrote mask bytes at or behind k" % (what, s)
            else:
                assert (got_mask[s] == SENTINEL).all(), "%s: set %d wrote mask bytes of a NULL mask's stand-in" % (what, s)
            if e["counts"] is not None:
                assert counts[s].tolist() == np.asarray(e["counts"]).tolist(), "%s: set %d per-try counts" % (what, s)
        return res

    def model(self, model, tries, samples=None, **opts):
        return [cm.find(self.pts[s], self.k(s), model, tries, set_index=s, sample_list=None if samples is None else samples[s], **opts) for s in range(self.n)]

    def twice(self, what, model, tries, expected, d_samples=None, mask=True, **opts):
        for turn in range(2):
            self.run(model, tries, d_samples=d_samples, mask=mask, **opts)
            res = self.check("%s, call %d" % (what, turn), model, tries, expected, mask)
        return res

    def check_distances(self, what, model, params, turns=2):
        d_params = self.buffer(np.asarray(params, np.float64))
        for turn in range(turns):
            self.ar.refill(self.d_dist)
            self.h.distances(ptr(self.d_pts), ptr(self.d_counts) if self.d_counts is not None else 0, model, ptr(d_params), ptr(self.d_dist))
            self.h.scores(1)
            self.ar.check(what)
            got = np.frombuffer(self.d_dist.cpu().numpy().tobytes(), np.float64).reshape(self.n, self.cap)
            for s in range(self.n):
                k = self.k(s)
                exp = cm.residuals(model, params[s][0], params[s][1], params[s][2], self.pts[s, :k])[0]
                assert got[s, :k].tobytes() == exp.tobytes(), "%s: set %d distances, call %d" % (what, s, turn)
                assert got[s, k:].tobytes() == np.full(self.cap - k, SENT64).tobytes(), "%s: set %d wrote distances at or behind k" % (what, s)

    def close(self):
        self.h.close()


def label_frame(W, H, stride, cap, rng):
    """a label map with components of 1, cap, cap + 1 and 3 * cap - 1 pixels (steps 1, 1, 2, 3), one whose box spans the frame (the border ring, the
    others inside its box), and junk in the padding columns; -> labels [H][stride], records, count"""
    lab = np.zeros((H, stride), np.int32)
    lab[:, W:] = rng.integers(1, 6, (H, stride - W))          # never read: columns >= W
    lab[0, :W] = lab[H - 1, :W] = 1
    lab[:, 0] = lab[:, W - 1] = 1          # id 1: the ring
    sizes = [1, cap, cap + 1, 3 * cap - 1]
    y = 2
    for i, n in enumerate(sizes):          # ids 2 .. 5: runs of rows of width W - 6 from column 3, two rows apart
        left = n
        while left:
            run = min(left, W - 6)
            lab[y, 3:3 + run] = i + 2
            left -= run
            y += 1
        y += 1
    assert y < H - 1, "label_frame: %d rows do not hold the components" % H
    comps = np.zeros(5, cm.COMP_DTYPE)
    for i in range(5):
        ys, xs = np.nonzero(lab[:, :W] == i + 1)
        comps[i] = (xs[0], ys[0], xs.min(), ys.min(), xs.max(), ys.max(), len(ys))
    return lab, comps


def gather_case(W, H, cap):
    """the two hand-made frames of test_gpu_curvefit.py::test_gather_from_label_maps: frame 0 has 3 records (the slots behind hold junk), frame 1 reports
    7 components and has 5 records -> labels [2][H][W + 3], records [2][5], counts, and the model's gathered points and counts"""
    stride, frames, comp_cap = W + 3, 2, 5
    rng = np.random.default_rng(W)
    lab0, comps0 = label_frame(W, H, stride, cap, rng)
    lab1, comps1 = label_frame(W, H, stride, cap, rng)
    labels = np.stack([lab0, lab1])
    comps = np.zeros((frames, comp_cap), cm.COMP_DTYPE)
    comps[0, :3], comps[1] = comps0[:3], comps1
    comps[0, 3] = comps[0, 4] = (0, 0, 0, 0, W - 1, H - 1, 99)
    counts = np.array([3, 7], np.int32)
    exp_pts, exp_k = zip(*[cm.gather(labels[f], W, comps[f], counts[f], comp_cap, cap) for f in range(frames)])
    exp_pts, exp_k = np.concatenate(exp_pts), np.concatenate(exp_k)
    ring = 2 * W + 2 * (H - 2)
    ring_k = -(-ring // -(-ring // cap))
    assert exp_k.tolist() == [ring_k, 1, cap, 0, 0, ring_k, 1, cap, (cap + 2) // 2, cap], "gather_case: the model's counts"          # steps: the ring's, 1, 1; then 2 and 3
    return labels, comps, counts, exp_pts, exp_k
