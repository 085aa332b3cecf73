"""What the Hamming-matcher GPU test shares with the tests that run the matcher among others (homography, content sequences, stream order): the
descriptor generators, and the matcher with its guarded buffers and its checks against tests/match_model.py."""
import numpy as np

import match_model as mm
from gpu_support import SENTINEL, Arena, ptr

REC = mm.MATCH_DTYPE.itemsize


def clip(count, cap):
    return max(0, min(int(count), cap))


def descriptors(kind, sets, cap, desc_bytes, stride, seed):
    """[sets][cap][stride] uint8: content in the first desc_bytes of a row, seeded random bytes (a 255 among them) in the stride padding"""
    rng = np.random.default_rng(seed + 9)
    out = rng.integers(0, 256, (sets, cap, stride), dtype=np.uint8)
    if stride > desc_bytes:
        out[:, :, desc_bytes] = 255
    for s in range(sets):
        out[s, :, :desc_bytes] = mm.content(kind, cap, desc_bytes, seed * 100 + s)
    return out


def derived(train_rows, n, desc_bytes, seed):
    """n query rows: copies of random train rows with 0..40 random bits flipped -- a clear best neighbour for most, several queries per train row"""
    rng = np.random.default_rng(seed)
    out = train_rows[rng.integers(0, len(train_rows), n), :desc_bytes].copy()
    for i in range(n):
        for b in rng.integers(0, desc_bytes * 8, rng.integers(0, 41)):
            out[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return out


class Rig:
    """A matcher and its guarded buffers.  q_counts / t_counts: None (a NULL pointer: every pair full) or a list of device counts."""

    def __init__(self, hip_ctx, desc_bytes, qcap, tcap, pairs, knn, query, train, q_counts=None, t_counts=None, shared=False, good_cap=0):
        from compv_amd import capi
        self.ctx = hip_ctx
        self.B, self.qcap, self.tcap, self.pairs, self.knn, self.shared, self.good_cap = desc_bytes, qcap, tcap, pairs, knn, shared, good_cap
        self.query, self.train = query, train
        self.qs, self.ts = query.shape[2], train.shape[2]
        self.q_counts, self.t_counts = q_counts, t_counts
        self.ar = Arena()
        self.d_query = self.ar.new(query.size, query)
        self.d_train = self.ar.new(train.size, train)
        self.ar.keep(self.d_query, query)
        self.ar.keep(self.d_train, train)
        self.d_qc = self.d_tc = None
        if q_counts is not None:
            h = np.asarray(q_counts, np.int32).view(np.uint8)
            self.d_qc = self.ar.new(h.size, h)
            self.ar.keep(self.d_qc, h)
        if t_counts is not None:
            h = np.asarray(t_counts, np.int32).view(np.uint8)
            self.d_tc = self.ar.new(h.size, h)
            self.ar.keep(self.d_tc, h)
        self.d_matches = self.ar.new(pairs * knn * qcap * REC)
        self.d_good = self.ar.new(max(pairs * good_cap * REC, 16))
        self.d_gc = self.ar.new(4 * pairs)
        self.m = capi.Matcher(hip_ctx, desc_bytes, qcap, tcap, pairs, knn)

    def set_counts(self, q_counts, t_counts):
        """other device counts for the next calls on the same handle (a rig made with count arrays)"""
        self.ar.reload(self.d_qc, np.asarray(q_counts, np.int32))
        self.ar.reload(self.d_tc, np.asarray(t_counts, np.int32))
        self.q_counts, self.t_counts = list(q_counts), list(t_counts)

    def sides(self, p):
        """the valid descriptor rows of pair p: (query rows, train rows)"""
        Q = self.qcap if self.q_counts is None else clip(self.q_counts[p], self.qcap)
        tp = 0 if self.shared else p
        T = self.tcap if self.t_counts is None else clip(self.t_counts[tp], self.tcap)
        return self.query[p, :Q, :self.B], self.train[tp, :T, :self.B]

    def args(self):
        return (ptr(self.d_query), self.qs, ptr(self.d_qc) if self.d_qc is not None else 0, ptr(self.d_train), self.ts,
                ptr(self.d_tc) if self.d_tc is not None else 0, self.shared)

    def knn_run(self, stream=0):
        self.m.knn(*self.args(), ptr(self.d_matches), stream=stream)

    def knn_check(self, what):
        self.ar.check(what)
        raw = self.d_matches.cpu().numpy().reshape(self.pairs, self.knn, self.qcap * REC)
        for p in range(self.pairs):
            q, t = self.sides(p)
            exp = mm.knn_device(q, t, self.knn)
            for r in range(self.knn):
                got = raw[p, r].tobytes()
                assert got[:len(q) * REC] == exp[r].tobytes(), "%s: pair %d neighbour %d" % (what, p, r)
                assert got[len(q) * REC:] == bytes([SENTINEL]) * ((self.qcap - len(q)) * REC), "%s: pair %d row %d wrote columns behind its query count" % (what, p, r)
        return raw.tobytes()

    def good_run(self, good_cap=None, stream=0, **opts):
        cap = self.good_cap if good_cap is None else good_cap
        self.ar.refill(self.d_good)
        self.ar.refill(self.d_gc)
        self.m.good(ptr(self.d_matches), *self.args(), ptr(self.d_good) if cap else 0, cap, ptr(self.d_gc), stream=stream, **opts)

    def good_check(self, what, good_cap=None, **opts):
        cap = self.good_cap if good_cap is None else good_cap
        self.ar.check(what)
        counts = np.frombuffer(self.d_gc.cpu().numpy().tobytes(), np.int32)
        raw = self.d_good.cpu().numpy().tobytes()
        total = 0
        for p in range(self.pairs):
            q, t = self.sides(p)
            exp = mm.good(q, t, self.knn, **opts)
            assert counts[p] == len(exp), "%s: pair %d good count %d, model %d" % (what, p, counts[p], len(exp))
            n = min(len(exp), cap)
            lo = p * cap * REC
            assert raw[lo:lo + n * REC] == exp[:n].tobytes(), "%s: pair %d good records" % (what, p)
            assert raw[lo + n * REC:lo + cap * REC] == bytes([SENTINEL]) * ((cap - n) * REC), "%s: pair %d wrote behind its good records" % (what, p)
            total += len(exp)
        if not cap:
            assert raw == bytes([SENTINEL]) * len(raw), "%s: %d bytes of the record buffer written although its capacity is 0" % (what, sum(b != SENTINEL for b in raw))
        return counts, total

    def close(self):
        self.m.close()
