"""What the connected-components GPU test shares with the tests that run the call among others (content sequences, pointer alignment, stream order):
the output buffers of a plan call, the comparer and the model of a batch."""
import numpy as np

from components_model import COMP_DTYPE, components
from gpu_support import COMP_BYTES, SENTINEL, ptr

SENT32 = np.frombuffer(bytes([SENTINEL] * 4), np.int32)[0]


class Out:
    """The three output buffers of a plan call, in an Arena."""

    def __init__(self, A, F, H, ls, cap, labels=True):
        self.F, self.H, self.ls, self.cap = F, H, ls, cap
        self.d_labels = A.new(F * H * ls * 4) if labels else None
        self.d_comps = A.new(F * cap * COMP_BYTES) if cap else None
        self.d_cc = A.new(F * 4)
        self.A = A

    def refill(self):
        for b in (self.d_labels, self.d_comps, self.d_cc):
            if b is not None:
                self.A.refill(b)

    def call(self, plan, d_edges, conn, mp, stream=0):
        plan.components(d_edges, conn, mp, ptr(self.d_labels) if self.d_labels is not None else 0, self.ls,
                        ptr(self.d_comps) if self.d_comps is not None else 0, self.cap, ptr(self.d_cc), stream)

    def raw(self):
        return tuple(None if b is None else b.cpu().numpy().tobytes() for b in (self.d_labels, self.d_comps, self.d_cc))


def assert_result(out, W, exp, what):
    """exp[f] = (labels, records) of the model.  Counts are the unclipped totals; the first min(count, cap) records equal the model's and the
    slots behind them still hold the sentinel; the label map equals the model's and its columns >= W still hold the sentinel."""
    F, H, ls, cap = out.F, out.H, out.ls, out.cap
    counts = out.d_cc.cpu().numpy().view(np.int32)
    for f in range(F):
        assert int(counts[f]) == len(exp[f][1]), (what, f, int(counts[f]), len(exp[f][1]))
    if out.d_comps is not None:
        raw = out.d_comps.cpu().numpy().reshape(F, cap * COMP_BYTES)
        for f in range(F):
            want = exp[f][1]
            n = min(len(want), cap)
            got = np.frombuffer(raw[f][:n * COMP_BYTES].tobytes(), COMP_DTYPE)
            if got.tobytes() != want[:n].tobytes():
                bad = int(np.flatnonzero(got != want[:n])[0])
                raise AssertionError("%s: frame %d record %d: got %s, expected %s" % (what, f, bad, got[bad], want[bad]))
            assert (raw[f][n * COMP_BYTES:] == SENTINEL).all(), (what, f, "records beyond the count were written")
    if out.d_labels is not None:
        lab = out.d_labels.cpu().numpy().view(np.int32).reshape(F, H, ls)
        for f in range(F):
            if not np.array_equal(lab[f, :, :W], exp[f][0]):
                ys, xs = np.nonzero(lab[f, :, :W] != exp[f][0])
                raise AssertionError("%s: frame %d: %d labels differ, first at (x %d, y %d): got %d, expected %d"
                                     % (what, f, len(ys), xs[0], ys[0], lab[f, ys[0], xs[0]], exp[f][0][ys[0], xs[0]]))
            assert (lab[f, :, W:] == SENT32).all(), (what, f, "label columns >= W were written")


def model(maps, conn, mp):
    return [components(e, conn, mp) for e in maps]
