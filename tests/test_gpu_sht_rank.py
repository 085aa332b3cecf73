"""The line sort's rank kernel (sht_sort_kernels.hip) on edge maps built for ties: the full ordered line list of every frame against the CPU oracle's canonical
order (strength descending, ties in emission order), element by element.

Isolated points on a lattice at threshold 1 give thousands of lines of strength 2, 3, 4 ...: equal strengths in one row of 64 lines, in adjacent rows, rows apart
and on both sides of every chunk boundary.  Every input's line count is checked on the CPU first (tests/sht_rank_cases.py names what each was found for), and no
frame exceeds the plan's 65 536 key slots.  The model of what the kernels compute is tests/test_sht_rank_model.py."""
import numpy as np
import pytest

import sht_rank_cases as rc
import gpu_support as pg
from gpu_support import Arena, ptr

pytestmark = pytest.mark.gpu

F = 3
S = 528                # row pitch of the 512-wide maps: padding columns hold random bytes
BIG_CAP = 1 << 15      # a caller's capacity above every frame's count here


@pytest.fixture(scope="module")
def frames(oracle):
    """name -> (edge map, oracle lines in canonical order), computed once; the counts each map was chosen for are asserted here"""
    out = {}
    for name, (_, _, count) in rc.LATTICE_FRAMES.items():
        m = rc.lattice_frame(name)
        lines = lines_tuple(oracle.sht(m, 1.0, 1))
        assert len(lines) == count, (name, len(lines), count)
        assert len(lines) <= rc.KEY_CAP
        out[name] = (m, lines)
    return out


def lines_tuple(lines):
    return [(float(np.float32(l[0])), float(np.float32(l[1])), int(l[2]), int(l[3]), int(l[4])) for l in lines]


def got_lines(raw_f, n):
    return [(float(l["rho"]), float(l["theta"]), int(l["strength"]), int(l["row"]), int(l["col"])) for l in pg.lines_of(raw_f, n)]


def run_sht(hip_ctx, maps, exp, cap, max_lines=0, what="", row_pitch=S):
    """one plan, one compvhip_plan_houghsht call at threshold 1 on `maps`; every frame's count and its first min(count, cap, maxLines) lines against `exp`"""
    from compv_amd import capi
    n_frames, H, W = maps.shape
    A = Arena()
    host = pg.pad_frames(maps, row_pitch, np.random.default_rng(W + cap))
    d_maps = A.new(host.size, host)
    A.keep(d_maps, host)
    d_lines = A.new(n_frames * cap * 20)
    d_counts = A.new(n_frames * 4)
    plan = capi.Plan(hip_ctx, W, H, row_pitch, n_frames, 1.0)
    try:
        for call in range(2):                                  # the second call on the live plan finds the first one's histograms and rank words
            A.refill(d_lines); A.refill(d_counts)
            plan.houghsht(ptr(d_maps), 1, max_lines, ptr(d_lines), cap, ptr(d_counts))
            A.check(what)
            counts = d_counts.cpu().numpy().view(np.int32)
            raw = d_lines.cpu().numpy().reshape(n_frames, cap, 20)
            for f, e in enumerate(exp):
                assert int(counts[f]) == len(e), (what, call, "line count", f, int(counts[f]), len(e))
                n = min(len(e), cap, max_lines if max_lines > 0 else cap)
                got = got_lines(raw[f], n)
                if got != e[:n]:
                    bad = next(i for i in range(n) if got[i] != e[i])
                    raise AssertionError((what, call, "frame", f, "first wrong slot", bad, got[bad], e[bad]))
    finally:
        plan.close()


def batch(frames, names):
    return np.stack([frames[n][0] for n in names]), [frames[n][1] for n in names]


def test_inputs_have_the_ties_they_were_built_for(frames):
    """on the CPU: equal strengths inside a row of 64 lines, in adjacent rows and 64 rows apart; one strength on both sides of both chunk boundaries"""
    for name in ("one_chunk", "one_chunk_and_a_line", "three_chunks"):
        s = [l[2] for l in rc.emission_order(frames[name][1])]
        assert rc.tie_distances(s) == {"row": True, "adjacent": True, "far": True}, name
    s = [l[2] for l in rc.emission_order(frames["three_chunks"][1])]
    assert len(s) > 2 * rc.CHUNK
    for edge in (rc.CHUNK, 2 * rc.CHUNK):
        near = set(s[edge - rc.ROW:edge]) & set(s[edge:edge + rc.ROW])
        assert near, edge                                      # a run of one strength across the boundary, within a row either side
        assert s[edge - 1] in s[edge:edge + rc.ROW] or s[edge] in s[edge - rc.ROW:edge], edge


def test_one_chunk_one_more_and_three_chunks_in_one_batch(hip_ctx, frames):
    """a batch of 3 frames of different counts: exactly one chunk of lines, one chunk + 1, more than two chunks"""
    maps, exp = batch(frames, ("one_chunk", "one_chunk_and_a_line", "three_chunks"))
    run_sht(hip_ctx, maps, exp, BIG_CAP, what="chunk boundaries")


def test_a_frame_without_lines_between_frames_with_lines(hip_ctx, frames):
    maps, exp = batch(frames, ("three_chunks", "none", "one_chunk_and_a_line"))
    run_sht(hip_ctx, maps, exp, BIG_CAP, what="empty frame in the middle")


def test_line_cap_below_the_line_count(hip_ctx, frames):
    """the caller's lineCap cuts every frame's sorted list, in the three-chunk frame inside its second chunk's worth of slots"""
    maps, exp = batch(frames, ("one_chunk_and_a_line", "three_chunks", "one_chunk"))
    cap = 5000
    assert all(len(e) > cap for e in exp)
    run_sht(hip_ctx, maps, exp, cap, what="lineCap 5000")
    cap = rc.CHUNK + 100
    assert len(exp[1]) > cap >= len(exp[0])
    run_sht(hip_ctx, maps, exp, cap, what="lineCap one chunk + 100")


def test_max_lines_cuts_inside_a_tie_run(hip_ctx, frames):
    maps, exp = batch(frames, ("three_chunks", "one_chunk", "one_chunk_and_a_line"))
    for max_lines in (7000, rc.CHUNK + 3):
        for e in exp:
            if len(e) > max_lines:
                assert e[max_lines - 1][2] == e[max_lines][2], max_lines      # the cut falls between two lines of one strength
        assert len(exp[0]) > max_lines
        run_sht(hip_ctx, maps, exp, BIG_CAP, max_lines, what="maxLines %d" % max_lines)


@pytest.mark.parametrize("W", [4095, 4097], ids=["13_strength_bits", "14_bits_library_sort"])
def test_widest_frame_of_the_device_sort_and_the_first_beyond(hip_ctx, oracle, W):
    """max(W, H) = 4095 is the last size whose strengths fit 13 bits; 4097 keeps the library sort, whose lists must be what they were"""
    H = 48
    maps = np.stack([rc.lattice_map(W, H, 16), rc.lattice_map(W, H, 16, 500, 5)])
    exp = [lines_tuple(oracle.sht(m, 1.0, 1)) for m in maps]
    assert len(exp[0]) > rc.CHUNK > len(exp[1]) > 0 and len(exp[0]) <= rc.KEY_CAP, [len(e) for e in exp]
    run_sht(hip_ctx, maps, exp, BIG_CAP, what="W = %d" % W, row_pitch=(W + 7) & ~7)


def test_two_asynchronous_steps_in_flight_on_two_plans(hip_ctx, oracle):
    """compvhip_plan_pipeline_async on two plans, both tickets enqueued before either is waited for: Canny -> SHT at threshold 1 on 512 x 512 frames of two
    and three chunks of lines, with an all-zero frame between them"""
    from compv_amd import capi
    W = H = 512
    kinds = ((("synth", 1), ("zero", 0), ("noise", 1)), (("text", 1), ("checker", 1), ("synth", 2)))
    A = Arena()
    rigs = []
    for k, ks in enumerate(kinds):
        imgs = np.stack([pg.make_frame(kind, W, H, seed) for kind, seed in ks])
        edges = [pg.canny_expect(oracle, img, 3, capi.THRESHOLD_COMPARE_TO_GRADIENT, pg.T_LOW, pg.T_HIGH) for img in imgs]
        exp = [lines_tuple(oracle.sht(e, 1.0, 1)) for e in edges]
        assert all(len(e) <= rc.KEY_CAP for e in exp)
        host = pg.pad_frames(imgs, S, np.random.default_rng(k))
        d_in = A.new(host.size, host)
        A.keep(d_in, host)
        rigs.append(dict(exp=exp, edges=edges, d_in=d_in, d_edges=A.new(F * H * S), d_lines=A.new(F * BIG_CAP * 20), d_counts=A.new(F * 4),
                         plan=capi.Plan(hip_ctx, W, H, S, F, 1.0)))
    counts = [[len(e) for e in r["exp"]] for r in rigs]
    assert counts[0][1] == 0 and counts[0][0] > 2 * rc.CHUNK and all(c > rc.CHUNK for c in (counts[0][2], counts[1][0], counts[1][1], counts[1][2])), counts
    try:
        for order in ((0, 1), (1, 0)):
            for r in rigs:
                A.refill(r["d_edges"]); A.refill(r["d_lines"]); A.refill(r["d_counts"])
            tickets = [r["plan"].pipeline_async(ptr(r["d_in"]), pg.T_LOW, pg.T_HIGH, 1, 0, ptr(r["d_edges"]), ptr(r["d_lines"]), BIG_CAP, ptr(r["d_counts"]))
                       for r in rigs]
            for i in order:
                rigs[i]["plan"].wait(tickets[i])
            A.check("two plans, waited in order %s" % (order,))
            for k, r in enumerate(rigs):
                pg.assert_maps(pg.frames_view(r["d_edges"], F, H, S, W), r["edges"], "plan %d: edges" % k)
                got_counts = r["d_counts"].cpu().numpy().view(np.int32)
                raw = r["d_lines"].cpu().numpy().reshape(F, BIG_CAP, 20)
                for f, e in enumerate(r["exp"]):
                    assert int(got_counts[f]) == len(e), (k, f, int(got_counts[f]), len(e))
                    assert got_lines(raw[f], len(e)) == e, ("plan", k, "frame", f, "order", order)
    finally:
        for r in rigs:
            r["plan"].close()
