"""What the Hough line-refinement GPU test shares with the tests that run the call among others (content sequences, pointer alignment, stream order):
the segments a plan wrote, the model of a batch and the comparers of the fit records and of the refined lines."""
import numpy as np

from gpu_support import FIT_BYTES, SEG_BYTES, SENTINEL
from sht_fit_model import FIT_DTYPE, frame_fits, refine_lines
from sht_segments_model import SEG_DTYPE
from sht_segments_rig import cells_of

INTS = ("line", "pixels", "sx", "sy", "sxx", "sxy", "syy")
DOUBLES = ("nx", "ny", "rho", "rms2")


def tables(oracle, W, H, theta):
    R, T, _ = oracle.sht_dims(W, H, theta)
    return R, oracle.sht_tables(theta, T)


def segs_of(d_segs, d_sc, F, cap):
    counts = d_sc.cpu().numpy().view(np.int32).copy()
    raw = d_segs.cpu().numpy().reshape(F, cap * SEG_BYTES)
    return [np.frombuffer(raw[f][:min(int(counts[f]), cap) * SEG_BYTES].tobytes(), SEG_DTYPE) for f in range(F)]


def same_records(got, exp, what):
    assert got.dtype == FIT_DTYPE and exp.dtype == FIT_DTYPE and len(got) == len(exp), what
    for k in INTS:
        if not (got[k] == exp[k]).all():
            i = int(np.flatnonzero(got[k] != exp[k])[0])
            raise AssertionError("%s: record %d field %s: got %s, expected %s" % (what, i, k, got[i], exp[i]))
    for k in DOUBLES:
        if not (got[k] == exp[k]).all():
            i = int(np.flatnonzero(~(got[k] == exp[k]))[0])
            raise AssertionError("%s: record %d field %s: got %r, expected %r (%s vs %s)" % (what, i, k, float(got[k][i]), float(exp[k][i]), got[i], exp[i]))


def assert_fits(d_fits, d_fc, F, fit_cap, exp, what):
    """Counts are the unclipped totals; the first min(count, fit_cap) records equal the model's; the slots behind them were not written."""
    counts = d_fc.cpu().numpy().view(np.int32)
    raw = d_fits.cpu().numpy().reshape(F, fit_cap * FIT_BYTES)
    for f in range(F):
        assert int(counts[f]) == len(exp[f]), (what, f, int(counts[f]), len(exp[f]))
        n = min(len(exp[f]), fit_cap)
        got = np.frombuffer(raw[f][:n * FIT_BYTES].tobytes(), FIT_DTYPE)
        same_records(got, exp[f][:n], "%s frame %d" % (what, f))
        assert (raw[f][n * FIT_BYTES:] == SENTINEL).all(), (what, f, "records beyond the count were written")


THETA_STATS = {"n": 0, "equal": 0}


def assert_refined(got, lines, fits, valid, what):
    """rho (a conversion), strength, row, col: exact.  theta: within 1 float32 ulp of np.float32(np.arctan2(ny, nx)) -- the device atan2 may
    differ from libm's by a few binary64 ulp, which moves a float32 rounding by at most one step."""
    exp = refine_lines(lines, fits, valid)
    assert len(got) == len(exp), what
    for k in ("rho", "strength", "row", "col"):
        assert got[k].tobytes() == exp[k].tobytes(), (what, k)
    v = np.array(valid, bool)
    assert got["theta"][~v].tobytes() == lines["theta"][~v].tobytes(), what
    g, e = got["theta"][v], exp["theta"][v]
    lo, hi = np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf))
    assert ((g >= lo) & (g <= hi)).all(), (what, g[(g < lo) | (g > hi)][:4], e[(g < lo) | (g > hi)][:4])
    THETA_STATS["n"] += int(v.sum())
    THETA_STATS["equal"] += int((g == e).sum())
    print("%s: refined theta exactly equal to float32(arctan2) on %d of %d lines (running: %d of %d)"
          % (what, int((g == e).sum()), int(v.sum()), THETA_STATS["equal"], THETA_STATS["n"]))


def model_fits(edge_maps, sinQ, cosQ, R, lines, b, max_lines=0, segs=None):
    out, valid = [], []
    for f, (e, ln) in enumerate(zip(edge_maps, lines)):
        r, v = frame_fits(e, sinQ, cosQ, cells_of(ln), b, R, max_lines, None if segs is None else segs[f])
        out.append(r)
        valid.append(v)
    return out, valid
