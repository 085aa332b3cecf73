"""The SVM GPU tests' rig (tests/test_gpu_svm.py, tests/test_gpu_fresh_memory.py): a handle and its guarded buffers.  Not a test module: every assert
carries its own message."""
import numpy as np

import svm_cases as sc
from gpu_support import SENTINEL, Arena, ptr, u8

PAD = 7e30          # finite in float32 and float64: (PAD - sv)^2 would swamp any kernel value


class Rig:
    """An SVM handle and its guarded buffers for up to `cap` queries of the case's type at stride D + extra"""

    def __init__(self, hip_ctx, c, cap, from_arrays=False, stream=0, extra=5, max_vectors=None):
        from compv_amd import capi
        self.capi, self.c, self.cap = capi, c, cap
        self.m = sc.recorded_model(c)
        self.stride = c["D"] + extra
        self.dtype = np.float32 if c["qtype"] == "f32" else np.float64
        self.vtype = capi.SVM_F32 if c["qtype"] == "f32" else capi.SVM_F64
        self.ar = Arena()
        self.d_x = self.ar.new(cap * self.stride * self.dtype().itemsize)
        self.d_lab = self.ar.new(cap * 4)
        self.d_dec = self.ar.new(cap * self.m.pairs * 8)
        self.d_k = self.ar.new(cap * self.m.l * 8)
        src = capi.SvmModel.from_file(sc.model_path(c["id"])) if from_arrays else sc.model_path(c["id"])
        self.h = capi.Svm(hip_ctx, src, cap if max_vectors is None else max_vectors, stream=stream)

    def host_rows(self, x):
        rows = sc.padded(np.ascontiguousarray(x, self.dtype), self.stride, PAD)
        full = np.full((self.cap, self.stride), PAD, self.dtype)
        full[:len(rows)] = rows
        return full

    def load(self, x):
        import torch
        self.d_x.copy_(torch.from_numpy(u8(self.host_rows(x)).copy()))
        torch.cuda.synchronize()

    def run(self, n, dec=True, kv=True):
        for b in (self.d_lab, self.d_dec, self.d_k):
            self.ar.refill(b)
        self.h.predict(ptr(self.d_x), self.vtype, n, self.stride, ptr(self.d_lab), ptr(self.d_dec) if dec else 0, ptr(self.d_k) if kv else 0)

    def check(self, what, n, labels, dec, K, has_dec=True, has_k=True):
        self.ar.check(what)          # (synchronises the device)
        got_lab = np.frombuffer(self.d_lab.cpu().numpy().tobytes(), np.int32)
        got_dec = np.frombuffer(self.d_dec.cpu().numpy().tobytes(), np.float64).reshape(self.cap, self.m.pairs)
        got_k = np.frombuffer(self.d_k.cpu().numpy().tobytes(), np.float64).reshape(self.cap, self.m.l)
        sent32, sent64 = np.frombuffer(bytes([SENTINEL] * 4), np.int32)[0], bytes([SENTINEL] * 8)
        assert got_lab[:n].tobytes() == labels[:n].tobytes(), "%s: labels %r, expected %r" % (what, got_lab[:n], labels[:n])
        assert (got_lab[n:] == sent32).all(), "%s: labels behind n written" % what
        for name, got, exp, present in (("dec", got_dec, dec, has_dec), ("K", got_k, K, has_k)):
            k = n if present else 0
            if present:
                bad = np.argwhere(got[:n].view(np.uint64) != np.ascontiguousarray(exp[:n]).view(np.uint64))
                assert not len(bad), "%s: %s differs in %d elements, first at %s: %r, expected %r" % (what, name, len(bad), bad[0], got[tuple(bad[0])], exp[tuple(bad[0])])
            assert got[k:].tobytes() == sent64 * (got[k:].size), "%s: %s written behind n (or into a NULL output's stand-in)" % (what, name)

    def close(self):
        self.h.close()
