"""What the Hough-segments GPU test shares with the tests that run the call among others (line refinement, content sequences, pointer alignment, stream
order): the lines a plan wrote, the model of a batch and the comparer."""
import numpy as np

from gpu_support import LINE_BYTES, SEG_BYTES, SENTINEL
from sht_segments_model import SEG_DTYPE, line_occupancy, line_segments


def tables(oracle, W, H, theta):
    R, T, _ = oracle.sht_dims(W, H, theta)
    return oracle.sht_tables(theta, T)


def lines_of(d_lines, d_counts, F, cap):
    """Per frame: the LINE_DTYPE array of the min(count, cap) lines the plan wrote, and the raw counts."""
    from compv_amd import capi
    counts = d_counts.cpu().numpy().view(np.int32).copy()
    raw = d_lines.cpu().numpy().reshape(F, cap * LINE_BYTES)
    return [np.frombuffer(raw[f][:min(int(counts[f]), cap) * LINE_BYTES].tobytes(), capi.LINE_DTYPE) for f in range(F)], counts


def cells_of(lines):
    return list(zip(lines["row"].tolist(), lines["col"].tolist()))


def model_frames(edge_maps, sinQ, cosQ, lines, params, max_lines=0):
    """{(minLength, maxGap): [SEG_DTYPE array of frame f]}; the occupancy of a line is computed once for all parameter pairs."""
    out = {p: [] for p in params}
    for e, ln in zip(edge_maps, lines):
        cells = cells_of(ln)
        if max_lines > 0:
            cells = cells[:max_lines]
        occ = [line_occupancy(e, sinQ, cosQ, r, c) for r, c in cells]
        for p in params:
            recs = []
            for i, (cnt, first, xm) in enumerate(occ):
                recs += line_segments(cnt, first, xm, i, p[0], p[1])
            out[p].append(np.array(recs, SEG_DTYPE) if recs else np.zeros(0, SEG_DTYPE))
    return out


def assert_segments(d_segs, d_seg_counts, F, seg_cap, exp, what):
    """Counts are the unclipped totals; the first min(count, seg_cap) records equal the model's; the slots behind them were not written."""
    counts = d_seg_counts.cpu().numpy().view(np.int32)
    raw = d_segs.cpu().numpy().reshape(F, seg_cap * SEG_BYTES)
    for f in range(F):
        assert int(counts[f]) == len(exp[f]), (what, f, int(counts[f]), len(exp[f]))
        n = min(len(exp[f]), seg_cap)
        got = np.frombuffer(raw[f][:n * SEG_BYTES].tobytes(), SEG_DTYPE)
        if got.tobytes() != exp[f][:n].tobytes():
            bad = int(np.flatnonzero(got != exp[f][:n])[0])
            raise AssertionError("%s: frame %d record %d: got %s, expected %s" % (what, f, bad, got[bad], exp[f][bad]))
        assert (raw[f][n * SEG_BYTES:] == SENTINEL).all(), (what, f, "records beyond the count were written")
