"""Hough line segments in plain numpy: the definition of include/compv_hip.h (compvhip_segment) restated, the yardstick of
tests/test_gpu_sht_segments.py.  It shares no code with the kernel; tests/test_sht_segments_model.py pins it against the
oracle's accumulator, a brute-force scan of the whole image and hand-drawn maps.

The Q16 tables come from oracle_bindings.Oracle.sht_tables (the vote's tables); all arithmetic is int64, so wide geometries
(W, H up to 32767) need no special case.
"""
import numpy as np

SEG_DTYPE = np.dtype([("line", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("support", "<i4")])


def line_occupancy(edges, sinQ, cosQ, row, col):
    """Rules 1-3 for the accumulator cell (row, col): (cnt[N], first[N], x_major).  cnt[p] = support pixels at position p that are
    inside the image and edges, first[p] = the smallest minor coordinate among them (-1 where cnt[p] == 0)."""
    H, W = edges.shape
    rho, s, c = (W + H) - int(row), int(sinQ[col]), int(cosQ[col])
    x_major = s >= abs(c)
    N, Nm = (W, H) if x_major else (H, W)
    cp, cm = (c, s) if x_major else (s, c)          # coefficient of the position / of the minor coordinate
    p = np.arange(N, dtype=np.int64)
    est = np.floor_divide((rho << 16) - p * cp, cm)
    cnt = np.zeros(N, np.int64)
    first = np.full(N, -1, np.int64)
    e = edges != 0
    for k in (2, 1, 0, -1):                         # descending: the smallest minor coordinate is written last
        m = est + k
        ok = (((p * cp + m * cm) >> 16) == rho) & (m >= 0) & (m < Nm)
        mi = np.clip(m, 0, Nm - 1)
        ok &= e[mi, p] if x_major else e[p, mi]
        cnt += ok
        first[ok] = m[ok]
    return cnt, first, x_major


def line_segments(cnt, first, x_major, line, min_length, max_gap):
    """Rules 4-5: the (line, x0, y0, x1, y1, support) records of one line, p0 ascending."""
    on = np.flatnonzero(cnt)
    if not len(on):
        return []
    brk = np.flatnonzero(np.diff(on) > max_gap + 1)
    starts = on[np.concatenate([[0], brk + 1])]
    ends = on[np.concatenate([brk, [len(on) - 1]])]
    csum = np.concatenate([[0], np.cumsum(cnt)])
    out = []
    for a, b in zip(starts.tolist(), ends.tolist()):
        if b - a + 1 >= min_length:
            (x0, y0), (x1, y1) = ((a, int(first[a])), (b, int(first[b]))) if x_major else ((int(first[a]), a), (int(first[b]), b))
            out.append((line, x0, y0, x1, y1, int(csum[b + 1] - csum[a])))
    return out


def frame_segments(edges, sinQ, cosQ, cells, min_length, max_gap, max_lines=0):
    """Rule 6 for one frame: cells = [(row, col)] in the order of the frame's line array; returns a SEG_DTYPE array (all segments,
    unclipped: the first min(count, segCap) of them are what a capacity segCap holds)."""
    n = len(cells) if max_lines <= 0 else min(len(cells), max_lines)
    out = []
    for i in range(n):
        cnt, first, xm = line_occupancy(edges, sinQ, cosQ, cells[i][0], cells[i][1])
        out += line_segments(cnt, first, xm, i, min_length, max_gap)
    return np.array(out, SEG_DTYPE) if out else np.zeros(0, SEG_DTYPE)
