"""Exact CPU model of the canonical KHT order (COMPVHIP_KHT_ORDER_CANONICAL, include/compv_hip.h), built from the oracle's stage exports only.

The oracle's stages (oracle/kht_oracle.c) give the smoothed-count records of CompVHoughKht::process; their emission order is restated here in numpy
(the reference's SSE2 scan + scalar remainder, quirk Q6: what kht_peaks_kernel does); a STABLE sort by count descending is the canonical order; the
oracle's visited-map sweep (orc_kht_peak_lines, correct for any input order) then picks the lines.  local_lines() is the per-record rule the GPU applies
instead of the sweep.  Test infrastructure only."""
import ctypes as C

import numpy as np

from oracle_bindings import KhtLine

sz = C.c_size_t


class Axes(C.Structure):
    _fields_ = [("dRho", C.c_double), ("dTheta_rad", C.c_double), ("dTheta_deg", C.c_double), ("r", C.c_double),
                ("rhoN", sz), ("T", sz), ("W", sz), ("H", sz)]


class Cell(C.Structure):
    _fields_ = [("rho_index", sz), ("theta_index", sz), ("count", C.c_int32)]


KERNEL_DOUBLES = 7   # orc_kht_kernel: rho, theta, h, sigma_theta_square, sigma_rho_square, m2, sigma_rho_times_theta


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class CanonModel:
    def __init__(self, oracle):
        self.L = L = oracle.lib
        L.orc_kht_axes.argtypes = [sz, sz, C.c_float, C.c_float, C.POINTER(Axes)]
        L.orc_kht_link.argtypes = [C.c_void_p, sz, sz, sz, sz, C.POINTER(C.c_void_p), C.POINTER(sz), C.POINTER(C.c_void_p), C.POINTER(sz)]
        L.orc_kht_clusters.argtypes = [C.c_void_p, C.c_void_p, sz, sz, C.c_double, C.POINTER(C.c_void_p), C.POINTER(sz)]
        L.orc_kht_kernels.argtypes = [C.c_void_p, C.c_void_p, sz, C.c_void_p, C.POINTER(C.c_double)]
        L.orc_kht_prune_gs.argtypes = [C.c_void_p, C.POINTER(sz), C.c_double, C.c_double, C.POINTER(C.c_double)]
        L.orc_kht_vote.argtypes = [C.POINTER(Axes), C.c_void_p, sz, C.c_double, C.c_void_p, sz]
        L.orc_kht_peak_votes.argtypes = [C.POINTER(Axes), C.c_void_p, sz, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(sz)]
        L.orc_kht_peak_lines.argtypes = [C.POINTER(Axes), C.c_void_p, sz, C.c_int, C.c_void_p, sz, C.POINTER(sz)]
        L.orc_free.argtypes = [C.c_void_p]

    def axes(self, W, H, rho=1.0, theta_deg=1.0):
        ax = Axes()
        assert self.L.orc_kht_axes(W, H, rho, theta_deg, C.byref(ax)) == 0
        return ax

    def vote_map(self, edges, rho=1.0, theta_deg=1.0, min_dev=2.0, min_size=10, min_height=0.002):
        """-> (axes, int32 count map [(T + 2), (rhoN + 2)] or None when no kernel survives, GS or None)"""
        L = self.L
        H, W = edges.shape
        edges = np.ascontiguousarray(edges)
        ax = self.axes(W, H, rho, theta_deg)
        poss, strings, clusters = C.c_void_p(), C.c_void_p(), C.c_void_p()
        npos, ns, nc = sz(0), sz(0), sz(0)
        assert L.orc_kht_link(_p(edges), W, H, edges.strides[0], min_size, C.byref(poss), C.byref(npos), C.byref(strings), C.byref(ns)) == 0
        try:
            if not ns.value:
                return ax, None, None
            assert L.orc_kht_clusters(poss, strings, ns.value, min_size, min_dev, C.byref(clusters), C.byref(nc)) == 0
            if not nc.value:
                return ax, None, None
            kernels = np.zeros((nc.value, KERNEL_DOUBLES), np.float64)
            hmax = C.c_double(0.0)
            assert L.orc_kht_kernels(poss, clusters, nc.value, _p(kernels), C.byref(hmax)) == 0
            nk, gs = sz(nc.value), C.c_double(1.0)
            assert L.orc_kht_prune_gs(_p(kernels), C.byref(nk), hmax.value, min_height, C.byref(gs)) == 0
            if not nk.value:
                return ax, None, None
            counts = np.zeros((ax.T + 2, ax.rhoN + 2), np.int32)
            assert L.orc_kht_vote(C.byref(ax), _p(kernels), nk.value, gs.value, _p(counts), ax.rhoN + 2) == 0
            return ax, counts, gs.value
        finally:
            for q in (poss, strings, clusters):
                if q.value:
                    L.orc_free(q)

    def oracle_votes(self, ax, counts, threshold):
        """orc_kht_peak_votes: the records in the reference's sorted order, as an [n, 3] array of (rho_index, theta_index, count)"""
        v, n = C.c_void_p(), sz(0)
        assert self.L.orc_kht_peak_votes(C.byref(ax), _p(counts), ax.rhoN + 2, threshold, C.byref(v), C.byref(n)) == 0
        try:
            cells = C.cast(v, C.POINTER(Cell))
            return np.array([(cells[i].rho_index, cells[i].theta_index, cells[i].count) for i in range(n.value)], np.int64).reshape(-1, 3)
        finally:
            if v.value:
                self.L.orc_free(v)

    def sweep(self, ax, records, max_lines=0):
        """orc_kht_peak_lines (the reference's visited-map sweep) on records [n, 3] = (rho_index, theta_index, count) in the given order"""
        n = len(records)
        cells = (Cell * max(n, 1))()
        for i, (r, t, c) in enumerate(records.tolist()):
            cells[i].rho_index, cells[i].theta_index, cells[i].count = r, t, c
        buf = (KhtLine * max(n, 1))()
        nl = sz(0)
        assert self.L.orc_kht_peak_lines(C.byref(ax), cells, n, max_lines, buf, max(n, 1), C.byref(nl)) == 0
        return [(buf[i].rho, buf[i].theta, buf[i].strength, buf[i].rho_index, buf[i].theta_index) for i in range(nl.value)]

    def lines(self, edges, rho=1.0, theta_deg=1.0, threshold=1, max_lines=0, min_dev=2.0, min_size=10, min_height=0.002):
        """The canonical list: ([(rho, theta, strength, rho_index, theta_index)], GS or None, records [n, 4] in canonical order)"""
        ax, counts, gs = self.vote_map(edges, rho, theta_deg, min_dev, min_size, min_height)
        if counts is None:
            return [], None, np.zeros((0, 4), np.int64)
        rec = canonical(emission(ax, counts, threshold))
        return self.sweep(ax, rec[:, :3], max_lines), gs, rec


def scan(rhoN):
    """(main-scan columns [1, main_end), sign test of the main scan, Q6 column or None): the reference's peak scan (:1166-1187, intrin_sse2.cxx:20-96)"""
    if rhoN <= 4:
        return rhoN, False, None
    sse_end = rhoN - 3
    main_end = 1 + 4 * ((sse_end - 1 + 3) // 4)
    consumed = (rhoN & ~3) + 1
    remains = max(rhoN - consumed, 0)
    return main_end, True, (consumed + 1 if remains >= 2 else None)   # remains <= 2: one Q6 column at most (position 1)


def emission(ax, counts, threshold):
    """The records in the reference's emission order: [n, 4] int64 of (rho_index, theta_index, count, emission key)"""
    rhoN, T = ax.rhoN, ax.T
    c = counts.astype(np.int64)
    s = (c[:-2, :-2] + 2 * c[:-2, 1:-1] + c[:-2, 2:] + 2 * c[1:-1, :-2] + 4 * c[1:-1, 1:-1] + 2 * c[1:-1, 2:]
         + c[2:, :-2] + 2 * c[2:, 1:-1] + c[2:, 2:]).astype(np.int32).astype(np.int64)   # smooth3x3 of map cell (t, r) = s[t - 1, r - 1], int32 arithmetic
    vs = rhoN + 2
    main_end, positive, q6 = scan(rhoN)
    v = counts[1:T, 1:main_end]
    m = ((v > 0) if positive else (v != 0)) & (s[0:T - 1, 0:main_end - 1] >= threshold)
    tt, rr = np.nonzero(m)
    t, r = tt + 1, rr + 1
    parts = [np.stack([r, t, s[tt, rr], t * 2 * vs + r], axis=1)]
    if q6 is not None:
        mq = (counts[1:T, q6] != 0) & (s[0:T - 1, q6 - 1] >= threshold)
        tq = np.nonzero(mq)[0] + 1
        parts.append(np.stack([np.ones_like(tq), tq, s[tq - 1, q6 - 1], tq * 2 * vs + vs + 1], axis=1))
    rec = np.concatenate(parts).astype(np.int64).reshape(-1, 4)
    return rec[np.argsort(rec[:, 3], kind="stable")]


def canonical(rec):
    """stable sort of the emission list by count descending (= count descending, emission key ascending)"""
    return rec[np.argsort(-rec[:, 2], kind="stable")]


def _neighbour_records(rec, rhoN, T):
    """for every record, the (count, key) of the records at the 8 OTHER positions around it (count 0: no record): two [n, k] arrays"""
    vs = rhoN + 2
    R, Tt, S, E = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]
    q6 = (E - Tt * 2 * vs) >= vs
    Sm = np.zeros((T + 2, rhoN + 2), np.int64); Em = np.zeros_like(Sm)
    Sm[Tt[~q6], R[~q6]] = S[~q6]; Em[Tt[~q6], R[~q6]] = E[~q6]
    Sq = np.zeros(T + 2, np.int64); Eq = np.zeros_like(Sq)
    Sq[Tt[q6]] = S[q6]; Eq[Tt[q6]] = E[q6]
    s2, e2 = [], []
    for dt in (-1, 0, 1):
        for dr in (-1, 0, 1):
            if dt or dr:
                s2.append(Sm[Tt + dt, R + dr]); e2.append(Em[Tt + dt, R + dr])
                at1 = (R + dr) == 1                                            # a Q6 record sits at position (t, 1)
                s2.append(np.where(at1, Sq[Tt + dt], 0)); e2.append(np.where(at1, Eq[Tt + dt], 0))
    return np.stack(s2, axis=1), np.stack(e2, axis=1)


def local_lines(rec, rhoN, T):
    """The local rule: record r is a line iff no record at another position of its 8-neighbourhood has a larger count, or the same count and a smaller
    emission key.  rec: [n, 4] (rho_index, theta_index, count, key) in any order -> boolean mask"""
    if not len(rec):
        return np.zeros(0, bool)
    s2, e2 = _neighbour_records(rec, rhoN, T)
    S, E = rec[:, 2:3], rec[:, 3:4]
    return ~((s2 > S) | ((s2 == S) & (e2 < E))).any(axis=1)


def has_tie_neighbour(rec, rhoN, T):
    """per record: some record at another position of its 8-neighbourhood has the same count"""
    if not len(rec):
        return np.zeros(0, bool)
    s2, _ = _neighbour_records(rec, rhoN, T)
    return (s2 == rec[:, 2:3]).any(axis=1)


def line_bits(lines):
    """LINE_DTYPE array -> [(rho bits, theta bits, strength, row, col)]"""
    return list(zip(lines["rho"].astype(np.float32).view(np.uint32).tolist(), lines["theta"].astype(np.float32).view(np.uint32).tolist(),
                    lines["strength"].tolist(), lines["row"].tolist(), lines["col"].tolist()))


def model_line_bits(lines):
    return [(int(np.float32(l[0]).view(np.uint32)), int(np.float32(l[1]).view(np.uint32)), l[2], l[3], l[4]) for l in lines]
