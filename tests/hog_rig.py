"""What the HOG GPU test shares with the content-sequence test: the plan with its guarded buffers and its checks against tests/hog_model.py."""
import numpy as np

import hog_model as hm
from gpu_support import SENTINEL, Arena, pad_frames, ptr


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Rig:
    """A plan of len(frames) frames of one size and its guarded buffers"""

    def __init__(self, hip_ctx, frames, opts, desc_pad=5, misalign=0):
        from compv_amd import capi
        self.F, (self.H, self.W) = len(frames), frames[0].shape
        self.S = (self.W + 7) // 8 * 8 + 8          # S > W, and S % 8 == 0 as a plan asks
        self.opts = hm.resolve(opts)
        self.o = capi.HogOpts(**self.opts)
        self.g = hm.geometry(self.W, self.H, self.opts)
        self.desc_len, self.stride = self.g["descLen"], self.g["descLen"] + desc_pad
        self.map_len = self.g["cellsY"] * self.g["cellsX"] * self.opts["nbins"]
        host = pad_frames(np.stack(frames), self.S, np.random.default_rng(self.W * 31 + self.H))
        self.ar = Arena()
        # misalign: the frames start that many bytes into their buffer (the bytes in front and behind are junk), so no row is dword aligned
        raw = np.concatenate([np.full(misalign, 0xEE, np.uint8), host.reshape(-1), np.full((8 - misalign) % 8, 0xEE, np.uint8)])
        self.d_raw = self.ar.new(raw.size, raw)
        self.ar.keep(self.d_raw, raw)
        self.gray_ptr = ptr(self.d_raw) + misalign
        self.d_desc = self.ar.new(self.F * self.stride * 4)
        self.d_cells = self.ar.new(self.F * self.map_len * 4)
        self.plan = capi.Plan(hip_ctx, self.W, self.H, self.S, self.F)

    def close(self):
        self.plan.close()

    def set_content(self, frames, opts, rng):
        """other frames and options for the next calls on the same plan; the descriptor stride stays, so descLen may not exceed it.  Without misalign only."""
        from compv_amd import capi
        self.opts = hm.resolve(opts)
        self.o = capi.HogOpts(**self.opts)
        self.g = hm.geometry(self.W, self.H, self.opts)
        self.desc_len = self.g["descLen"]
        assert self.desc_len <= self.stride, "descLen %d exceeds the descriptor stride %d of this rig" % (self.desc_len, self.stride)
        self.ar.reload(self.d_raw, pad_frames(np.stack(frames), self.S, rng))

    def run(self, cells=True, stream=0, opts=None, stride=None):
        self.ar.refill(self.d_desc)
        self.ar.refill(self.d_cells)
        self.plan.hog(self.gray_ptr, ptr(self.d_desc), self.stride if stride is None else stride, ptr(self.d_cells) if cells else 0, opts=self.o if opts is None else opts,
                      stream=stream)

    def outputs(self, what):
        self.ar.check(what)
        desc = self.d_desc.cpu().numpy().view(np.uint32).reshape(self.F, self.stride)
        cells = self.d_cells.cpu().numpy().view(np.uint32).reshape(self.F, self.map_len)
        return desc, cells

    def check(self, what, expected, cells=True):
        """expected: per frame (desc, cell map) of the model.  Returns the descriptors' bytes."""
        desc, got_cells = self.outputs(what)
        pad = np.frombuffer(bytes([SENTINEL]) * 4, np.uint32)[0]
        for f, (e_desc, e_cells) in enumerate(expected):
            bad = np.nonzero(desc[f, :self.desc_len] != bits(e_desc))[0]
            assert bad.size == 0, "%s: frame %d, %d of %d descriptor floats differ, first at %d" % (what, f, bad.size, self.desc_len, bad[0])
            assert (desc[f, self.desc_len:] == pad).all(), "%s: frame %d wrote behind descLen" % (what, f)
            if cells:
                bad = np.nonzero(got_cells[f] != bits(e_cells).reshape(-1))[0]
                assert bad.size == 0, "%s: frame %d, %d of %d map floats differ, first at %d" % (what, f, bad.size, self.map_len, bad[0])
            else:
                assert (got_cells[f] == pad).all(), "%s: the caller's map was written without being passed" % what
        return desc.tobytes()

    def twice(self, what, expected, **kw):
        self.run(**kw)
        first = self.check(what, expected, cells=kw.get("cells", True))
        self.run(**kw)
        assert self.check(what + " (again)", expected, cells=kw.get("cells", True)) == first, "%s: the second call's descriptors differ from the first call's" % what
        return first
