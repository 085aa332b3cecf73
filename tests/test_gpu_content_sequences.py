"""Handles across changing content: nothing carried between calls.

The rest of the suite checks replays by making the same call twice, which is blind to stale state: what the first call left behind is exactly what the second
is supposed to produce.  Here one handle lives through a sequence of DIFFERENT contents and parameters (tests/content_sequences.py; its properties are checked
on the CPU by tests/test_content_sequences.py), the way a video and bench.py use it.  The driver is the same for every stage (drive()):

  - the handle is created once;
  - before each call every output buffer is refilled with a sentinel;
  - after the call every output of every frame is compared with the model or oracle of THAT STEP ALONE, bit for bit -- no tolerances, as in the rest of the suite;
  - where include/compv_hip.h promises that slots beyond a count are not written, those slots must still hold the sentinel (the checkers of the stage tests,
    reused here, assert that);
  - after the last step the first one runs again and must match its model again;
  - the whole sequence runs twice, and compvhip_live_allocations after the second pass equals the count after the first.

Every test runs in two passes of the module (the autouse fixture fresh_allocations): `as_allocated`, on blocks as hipMalloc hands them out, and `filled_ff`,
where every block the library allocates is filled with 0xFF first -- step 0 of a sequence is a handle's FIRST call, and nothing may depend on what a fresh
block holds.

Which buffer each sequence watches is tabled in docs/dispatch_coverage.md ("State a handle keeps between calls", "Fresh allocations").
"""
import numpy as np
import pytest

import content_sequences as cs
import gpu_support as pg
from gpu_support import FIT_BYTES, SEG_BYTES, SENTINEL, Arena, ptr

pytestmark = pytest.mark.gpu

LINE_CAP = 4096


PASSES = {None: 2, 0xFF: 2}          # fill byte of the module's pass -> times drive() runs a sequence through


@pytest.fixture(autouse=True, params=[None, 0xFF], ids=["as_allocated", "filled_ff"])
def fresh_allocations(request):
    """Every test of this module runs twice: on blocks as hipMalloc hands them out (in a young process: zeros), and with every block the library allocates
    filled with 0xFF (gpu_support.alloc_fill) -- NaN, 65 535, -1, every flag set.  Step 0 of a sequence is a handle's first call, at the geometries where
    scratch is shared across workgroups; an autouse fixture is set up before the ones a test names, so the handles those create are created under the fill
    too (docs/dispatch_coverage.md, "Fresh allocations")."""
    PASSES["now"] = PASSES[request.param]
    with pg.alloc_fill(request.param):
        yield request.param


def drive(ctx, steps, call, passes=None):
    """call(k, what) makes step k's call on the live handle and checks it: every step, then the first again; twice; no allocation may be left over"""
    live = []
    for p in range(PASSES["now"] if passes is None else passes):
        for i, k in enumerate(cs.run_order(steps)):
            call(k, "pass %d call %d (step %d)" % (p, i, k))
        live.append(ctx.live_allocations())
    assert live[-1] == live[0], live


def lines_tuple(lines):
    return [(float(np.float32(l[0])), float(np.float32(l[1])), int(l[2]), int(l[3]), int(l[4])) for l in lines]


def got_lines(raw_f, n):
    return [(float(l["rho"]), float(l["theta"]), int(l["strength"]), int(l["row"]), int(l["col"])) for l in pg.lines_of(raw_f, n)]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (a) Canny, SHT and the pipeline on one plan
# ---------------------------------------------------------------------------------------------------------------------------------------------
def plan_expectations(oracle, W, H):
    """per step: [(edges, acc, lines)] per frame, from the oracle on that step's frames and parameters alone"""
    out = []
    for frames, prm in cs.plan_sequence(W, H):
        per = []
        for img in frames:
            e = pg.canny_expect(oracle, img, prm["ksize"], prm["mode"], prm["tl"], prm["th"])
            acc, lines = pg.sht_expect(oracle, e, 1.0, prm["thr"])
            per.append((e, acc, lines_tuple(lines)))
        out.append(per)
    return out


class PlanRig:
    """one plan and one set of guarded buffers for a whole sequence"""

    def __init__(self, hip_ctx, oracle, W, H, S, line_cap=LINE_CAP):
        from compv_amd import capi
        self.capi, self.ctx, self.oracle = capi, hip_ctx, oracle
        self.W, self.H, self.S, self.cap = W, H, S, line_cap
        self.steps = cs.plan_sequence(W, H)
        self.exp = plan_expectations(oracle, W, H)
        self.R, self.T, _ = oracle.sht_dims(W, H, 1.0)
        self.A = Arena()
        self.n = cs.F * H * S
        self.rng = np.random.default_rng(W + H)
        self.inputs = [self.device_frames(frames) for frames, _ in self.steps]
        self.outs = [self.outputs() for _ in range(2)]
        self.d_acc = self.A.new(self.R * self.T * 4)
        self.plan = capi.Plan(hip_ctx, W, H, S, cs.F, 1.0)

    def device_frames(self, frames, pad=None):
        """[F][H][S] device copy whose padding columns hold seeded random bytes (or `pad`), registered as an input that must come back unchanged"""
        host = pg.pad_frames(frames, self.S, self.rng)
        if pad is not None:
            host[:, :, self.W:] = pad
        d = self.A.new(self.n, host)
        self.A.keep(d, host)
        return d

    def outputs(self):
        return dict(edges=self.A.new(self.n), lines=self.A.new(cs.F * self.cap * 20), counts=self.A.new(cs.F * 4))

    def refill(self, o):
        for b in o.values():
            self.A.refill(b)

    def close(self):
        self.plan.close()

    # -- calls --
    def canny(self, k, o):
        prm = self.steps[k][1]
        self.plan.canny(ptr(self.inputs[k]), prm["tl"], prm["th"], ptr(o["edges"]), prm["ksize"], prm["mode"])

    def sht(self, k, o, d_edges=0):
        prm = self.steps[k][1]
        self.plan.houghsht(d_edges, prm["thr"], prm["max_lines"], ptr(o["lines"]), self.cap, ptr(o["counts"]))

    def pipeline(self, k, o, asynchronous=False):
        prm = self.steps[k][1]
        a = (ptr(self.inputs[k]), prm["tl"], prm["th"], prm["thr"], prm["max_lines"], ptr(o["edges"]), ptr(o["lines"]), self.cap, ptr(o["counts"]))
        if prm["ksize"] == 3 and prm["mode"] == cs.GRADIENT:
            return self.plan.pipeline_async(*a) if asynchronous else self.plan.pipeline(*a)
        return self.plan.pipeline_ex(*a, ksize=prm["ksize"], threshold_type=prm["mode"], asynchronous=asynchronous)

    # -- checks: every output against step k's expectation --
    def check_edges(self, k, o, what):
        self.A.check(what)
        pg.assert_maps(pg.frames_view(o["edges"], cs.F, self.H, self.S, self.W), [x[0] for x in self.exp[k]], what + ": edges")

    def check_lines(self, k, o, what, exp=None):
        """counts are the uncut totals; the records are the strongest min(count, lineCap, maxLines) in the canonical order"""
        self.A.check(what)
        exp = [x[2] for x in self.exp[k]] if exp is None else exp
        max_lines = self.steps[k][1]["max_lines"]
        counts = o["counts"].cpu().numpy().view(np.int32)
        raw = o["lines"].cpu().numpy().reshape(cs.F, self.cap, 20)
        for f, e in enumerate(exp):
            assert int(counts[f]) == len(e), (what, "line count", f, int(counts[f]), len(e))
            n = min(len(e), self.cap, max_lines if max_lines > 0 else self.cap)
            assert got_lines(raw[f], n) == e[:n], (what, "lines", f)

    def check_sht_state(self, k, what, edges=None, accs=None):
        """the plan's own edge counts and its whole accumulator, cell by cell"""
        edges = [x[0] for x in self.exp[k]] if edges is None else edges
        accs = [x[1] for x in self.exp[k]] if accs is None else accs
        assert pg.edge_counts(self.plan, cs.F).tolist() == [int((m != 0).sum()) for m in edges], what + ": edge counts"
        for f in range(cs.F):
            self.A.refill(self.d_acc)
            self.plan.acc_export(f, ptr(self.d_acc), self.T)
            self.A.check("%s acc_export %d" % (what, f))
            got = self.d_acc.cpu().numpy().view(np.int32).reshape(self.R, self.T)
            assert (got == accs[f]).all(), (what, "accumulator", f, int((got != accs[f]).sum()))


@pytest.fixture(params=cs.PLAN_GEOMETRIES, ids=lambda g: "%dx%d_S%d" % g)
def plan_rig(request, hip_ctx, oracle):
    rig = PlanRig(hip_ctx, oracle, *request.param)
    yield rig
    rig.close()


def test_plan_pipeline_sequence(plan_rig):
    """compvhip_plan_pipeline / _ex, synchronous: noise, bars with tile columns of 256 and more (partHi, colFlag), a constant frame, the bars shifted -- rotated over
    the frames -- while ksize, the threshold mode, the SHT threshold and maxLines change from call to call.  Watches the accumulator and NMS flag planes that are
    zeroed once, colFlag / partHi, the counters the tile kernel clears, the per-frame threshold scratch (thrDev, sums, hist)."""
    r, o = plan_rig, plan_rig.outs[0]

    def call(k, what):
        r.refill(o)
        r.pipeline(k, o)
        r.check_edges(k, o, what)
        r.check_lines(k, o, what)
        r.check_sht_state(k, what)

    drive(r.ctx, r.steps, call)


def test_plan_canny_then_sht_on_the_masks_sequence(plan_rig):
    """compvhip_plan_canny, then compvhip_plan_houghsht(NULL) on its bit masks: the same sequence as two calls per step (the SHT relies on the counters the Canny
    tile kernel cleared: countersFresh)."""
    r, o = plan_rig, plan_rig.outs[0]

    def call(k, what):
        r.refill(o)
        r.canny(k, o)
        r.check_edges(k, o, what + " canny")
        r.sht(k, o)
        r.check_lines(k, o, what + " houghsht(masks)")
        r.check_sht_state(k, what + " houghsht(masks)")

    drive(r.ctx, r.steps, call)


def test_plan_sht_on_foreign_bytes_between_canny_steps(plan_rig):
    """compvhip_plan_houghsht on the caller's edge bytes between two Canny steps: the foreign maps are the oracle's edges of the step two further on (another class
    for every frame), 255 in their padding.  The foreign call overwrites the plan's bit masks (bitsValid drops) and finds the counters used (countersFresh is
    false: it clears them itself); the Canny after it must leave nothing of either behind."""
    r, o = plan_rig, plan_rig.outs[0]
    K = len(r.steps)
    foreign = []
    for k in range(K):
        thr = r.steps[k][1]["thr"]
        maps = [x[0] for x in r.exp[(k + 2) % K]]
        accs = [x[1] for x in r.exp[(k + 2) % K]]
        lines = [lines_tuple(r.oracle.sht_lines_from_acc(a, r.W, r.H, 1.0, thr)) for a in accs]
        foreign.append((r.device_frames(np.stack(maps), pad=255), maps, accs, lines))

    def call(k, what):
        r.refill(o)
        r.canny(k, o)
        r.check_edges(k, o, what + " canny")
        r.sht(k, o)
        r.check_lines(k, o, what + " houghsht(masks)")
        r.check_sht_state(k, what + " houghsht(masks)")
        d_fe, maps, accs, lines = foreign[k]
        r.A.refill(o["lines"]); r.A.refill(o["counts"])
        r.sht(k, o, ptr(d_fe))
        r.check_lines(k, o, what + " houghsht(foreign)", lines)
        r.check_sht_state(k, what + " houghsht(foreign)", maps, accs)

    drive(r.ctx, r.steps, call)


def test_plan_pipeline_async_two_tickets_in_flight(plan_rig):
    """compvhip_plan_pipeline_async / _ex with a ticket: steps k and k + 1 (every frame of another class) in flight on separate buffers, waited in issue order for
    even k and in reverse for odd k.  Edges, counts and lines of both tickets, and the plan's accumulator and edge counts, which belong to the step that ran
    last: step k + 1 whenever the tickets were waited in issue order (a replay in compvhip_plan_wait runs the later step again too)."""
    r = plan_rig
    K = len(r.steps)

    def call(k, what):
        ks = (k, (k + 1) % K)
        for o in r.outs:
            r.refill(o)
        tickets = [r.pipeline(j, o, asynchronous=True) for j, o in zip(ks, r.outs)]
        in_order = k % 2 == 0
        for i in ((0, 1) if in_order else (1, 0)):
            r.plan.wait(tickets[i])
        for j, o in zip(ks, r.outs):
            r.check_edges(j, o, "%s ticket of step %d" % (what, j))
            r.check_lines(j, o, "%s ticket of step %d" % (what, j))
        # the plan's accumulator and edge counts are those of the step that ran last: step k + 1, or -- when compvhip_plan_wait replayed step k after it, which
        # only the reverse order allows -- step k; wholly one of the two, never a mixture
        try:
            r.check_sht_state(ks[1], what)
        except AssertionError:
            if in_order:
                raise
            r.check_sht_state(ks[0], what + " (step %d replayed last)" % ks[0])

    drive(r.ctx, r.steps, call)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (b) the line sort on a live plan
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_line_sort_sequence_and_the_move_to_the_library_sort(hip_ctx, oracle):
    """The device-sized line sort (sht_sort_kernels.hip) on one plan: frames of more than two chunks of 4096 lines, less than one, none, more than one -- rotated
    over the frames, so that chunks which return at once keep the histograms of the call before -- while the caller's line capacity goes 16, 10 000, 16, 10 000 (the
    plan keeps its larger key buffers).  Then one call with a capacity above 32 chunks takes the plan off the device sort for good (ensureLineCap releases chunkHist
    and strengthStart; key slots past the sorted range hold an earlier call's pairs), and the whole sequence runs again on the library sort.  Every list against
    the oracle's canonical order, element by element; counts are the uncut totals."""
    from compv_amd import capi
    W, H, S = cs.SORT_GEOMETRY
    steps = cs.sort_sequence()
    exp = [[lines_tuple(oracle.sht(m, 1.0, 1)) for m in maps] for maps, _ in steps]
    A = Arena()
    rng = np.random.default_rng(W)
    d_maps = []
    for maps, _ in steps:
        host = pg.pad_frames(maps, S, rng)
        d = A.new(host.size, host)
        A.keep(d, host)
        d_maps.append(d)
    caps = sorted(set(p["line_cap"] for _, p in steps) | {cs.SORT_BIG_CAP})
    d_lines = {c: A.new(cs.F * c * 20) for c in caps}
    d_counts = A.new(cs.F * 4)
    plan = capi.Plan(hip_ctx, W, H, S, cs.F, 1.0)

    def run(k, cap, what):
        A.refill(d_lines[cap]); A.refill(d_counts)
        plan.houghsht(ptr(d_maps[k]), 1, 0, ptr(d_lines[cap]), cap, ptr(d_counts))
        A.check(what)
        counts = d_counts.cpu().numpy().view(np.int32)
        raw = d_lines[cap].cpu().numpy().reshape(cs.F, cap, 20)
        for f, e in enumerate(exp[k]):
            assert int(counts[f]) == len(e), (what, "line count", f, int(counts[f]), len(e))
            n = min(len(e), cap)
            assert got_lines(raw[f], n) == e[:n], (what, "lines", f)

    try:
        drive(hip_ctx, steps, lambda k, what: run(k, steps[k][1]["line_cap"], "device sort, " + what))
        run(0, cs.SORT_BIG_CAP, "the capacity that leaves the device sort")
        drive(hip_ctx, steps, lambda k, what: run(k, steps[k][1]["line_cap"], "library sort, " + what))
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (e) the matcher
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True], ids=["own_train", "shared_train"])
def test_matcher_sequence_of_device_counts(hip_ctx, shared):
    """One matcher whose trainCap AND queryCap span three slices of 128, device counts that change between calls: every slice used, one slice, no train row, no
    query, every slice again, a mixed step -- ragged and rotated over the pairs.  A slice beyond a pair's train count returns before it writes its partial list,
    so the lists of the call before stay in the handle: the merge must read the slices that ran, no others.  The cross check runs the same kernels with the roles
    swapped (the QUERY count decides which reverse slices run): under crossCheck the query counts go three slices -> one -> none -> two / three / one, with a
    smaller non-zero train count, and crossCheck is off in between, so the reverse lists and `reverse` are stale in their own rhythm.
    The knn records and the good list against tests/match_model.py, byte for byte; columns behind a query count and records behind a good count keep the
    sentinel (Rig.knn_check / good_check)."""
    import match_rig as gm
    m = cs.MATCH
    steps = cs.match_steps(shared)
    query, train = cs.match_descriptors(shared)
    rig = gm.Rig(hip_ctx, m["desc_bytes"], m["qcap"], m["tcap"], m["pairs"], m["knn"], query, train, steps[0]["q"], steps[0]["t"], shared, good_cap=m["qcap"])

    def call(k, what):
        s = steps[k]
        rig.set_counts(s["q"], s["t"])
        rig.ar.refill(rig.d_matches)
        rig.knn_run()
        rig.knn_check(what + " knn")
        o = dict(ratio=s["ratio"], max_distance=s["max_distance"], cross_check=s["cross_check"])
        rig.good_run(**o)
        rig.good_check(what + " good", **o)

    try:
        drive(hip_ctx, steps, call)
    finally:
        rig.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (f) the homography handle
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_homography_sequence_of_point_sets(hip_ctx):
    """One handle: a planted model with k = 129, k = 3 (status 2: nothing written but the record), every quad collinear (status 1: no try stores a hypothesis, so the
    hypotheses of the call before must not be scored -- the per-try counts, variances and rotations are compared too), k = 4, another planted model; rotated over
    three pairs while tries goes 257 <-> 63, the quads come from the generator, then from the caller, then from the generator, and the mask is given or NULL.
    Against tests/homography_model.py, bit for bit; the points behind a pair's count are what the step before left there."""
    import homography_rig as gh
    import homography_model as hm
    from compv_amd import capi
    h = cs.HOMOGRAPHY
    steps = cs.homography_sequence()
    rig = gh.Rig(hip_ctx, steps[0][0], h["point_cap"], h["max_tries"])
    exp, quads = [], []
    src, dst = rig.src.copy(), rig.dst.copy()
    hosts = []
    for sets, prm in steps:                                    # the host image of every step: its points over what the steps before left behind them
        for p, (s, d) in enumerate(sets):
            src[p, :len(s)], dst[p, :len(s)] = s, d
        counts = [len(s) for s, _ in sets]
        q = None
        if prm["given_quads"]:                                 # another seed's quads for the pair's own k (zeros for k < 4: never read)
            q = np.stack([capi.homography_quads(prm["seed"] + 100, p, k, prm["tries"]) if k >= 4 else np.zeros((prm["tries"], 4), np.int32) for p, k in enumerate(counts)])
        hosts.append((src.copy(), dst.copy(), counts, None if q is None else rig.quads_buffer(q)))
        exp.append([hm.find(src[p], dst[p], counts[p], prm["tries"], seed=prm["seed"], pair=p, quad_list=None if q is None else q[p]) for p in range(h["pairs"])])

    def call(k, what):
        prm = steps[k][1]
        s, d, counts, d_quads = hosts[k]
        rig.set_points(s, d, counts)
        rig.run(prm["tries"], d_quads=d_quads, mask=prm["mask"], seed=prm["seed"])
        res = rig.check(what, prm["tries"], exp[k], mask=prm["mask"])
        want = {"planted_large": 0, "planted_other": 0, "four_points": 0, "three_points": 2, "collinear": 1}
        assert res["status"].tolist() == [want[kind] for kind in prm["kinds"]], what

    try:
        drive(hip_ctx, steps, call)
    finally:
        rig.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (d) FAST
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", cs.FAST_GEOMETRIES, ids=lambda g: "%dx%d_S%d_F%d" % g)
def test_fast_sequence(hip_ctx, geom):
    """compvhip_plan_fast on one plan: many corners, none, a handful at other positions, tied arcs -- rotated over the frames -- while the threshold, N 9 <-> 12,
    nonmax and maxFeatures (a cut that falls at a tie included) change, the score map alternates between the caller's and the plan's (fastScores), and the records
    alternate with counts only.  Watches fastScores, the sums FAST clears per call and the corner lists; score map, counts and records against tests/fast_model.py;
    records behind a count and an unrequested score map keep the sentinel (Rig.check)."""
    import fast_model as fm
    import fast_rig as gf
    W, H, S, F = geom
    steps = cs.fast_sequence(W, H)
    exp = [[fm.fast(fr[f], p["t"], p["N"], p["nonmax"]) for f in range(F)] for fr, p in steps]
    cap = max(len(e[0]) for ex in exp for e in ex) + 5
    rig = gf.Rig(hip_ctx, geom, 1, cap)
    rng = np.random.default_rng(W)

    def call(k, what):
        fr, p = steps[k]
        rig.set_content(fr, rng)
        c = cap if p["records"] else 0
        rig.run(p["N"], p["nonmax"], p["t"], max_features=p["max_features"], scores=p["scores"], cap=c)
        rig.check(what, exp[k], scores=p["scores"], cap=c, cut=p["max_features"])

    try:
        drive(hip_ctx, steps, call)
    finally:
        rig.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (g) calls that look stateless and own scratch
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_otsu_sequence(hip_ctx, oracle):
    """compvhip_plan_otsu: its partial histograms (hist, plan-owned) are sums and preproc_kernels.hip has no memset, so every chunk must be written whole by every
    call.  Frames with quite different histograms in a row -- noise, a constant frame (one bin), a dark and a bright bimodal frame."""
    from compv_amd import capi
    W, H, S = cs.SCRATCH_GEOMETRY
    steps = cs.otsu_sequence()
    exp = [[int(oracle.otsu(f)) for f in fr] for fr, _ in steps]
    A = Arena()
    rng = np.random.default_rng(W)
    d_in = [A.new(cs.F * H * S, pg.pad_frames(fr, S, rng)) for fr, _ in steps]
    for d in d_in:
        A.keep(d, d.cpu().numpy())
    d_otsu = A.new(cs.F * 4)
    plan = capi.Plan(hip_ctx, W, H, S, cs.F)

    def call(k, what):
        A.refill(d_otsu)
        plan.otsu(ptr(d_in[k]), ptr(d_otsu))
        A.check(what)
        assert d_otsu.cpu().numpy().view(np.int32).tolist() == exp[k], what

    try:
        drive(hip_ctx, steps, call)
    finally:
        plan.close()


def test_morph_and_in_place_adaptive_share_their_scratch(hip_ctx):
    """Open and close (two passes through morphTmp) and the in-place adaptive threshold (which also goes through morphTmp) alternate on one plan while the
    structuring element, the border, the block size and the content change: morphTmp is plan-owned and never cleared, so each call must write every byte of it
    that it reads.  Against tests/morph_model.py; the padding columns of the output keep the sentinel for the out-of-place calls."""
    import morph_model as mm
    from compv_amd import capi
    W, H, S = cs.SCRATCH_GEOMETRY
    steps = cs.morph_sequence()
    A = Arena()
    rng = np.random.default_rng(H)
    hosts = [pg.pad_frames(fr, S, rng) for fr, _ in steps]
    d_in = [A.new(h.size, h) for h in hosts]
    for d, h in zip(d_in, hosts):
        A.keep(d, h)
    d_out = A.new(cs.F * H * S)
    exp = []
    for fr, p in steps:
        if p["call"] == "morph":
            se = mm.strel(*p["strel"])
            exp.append([mm.morph(f, se, p["op"], p["border"]) for f in fr])
        else:
            exp.append([mm.adaptive(f, p["block"], p["delta"], 255.0, p["invert"]) for f in fr])
    plan = capi.Plan(hip_ctx, W, H, S, cs.F)

    def call(k, what):
        fr, p = steps[k]
        if p["call"] == "morph":
            A.refill(d_out)
            plan.morph(ptr(d_in[k]), mm.strel(*p["strel"]), p["op"], p["border"], ptr(d_out))
        else:                                                   # in place: the output buffer holds the input
            d_out.copy_(d_in[k])
            plan.threshold_adaptive(ptr(d_out), p["block"], p["delta"], 255.0, p["invert"], ptr(d_out))
        A.check(what)
        got = d_out.cpu().numpy().reshape(cs.F, H, S)
        if p["call"] == "morph":
            assert (got[:, :, W:] == SENTINEL).all(), what + ": padding columns written"
        for f in range(cs.F):
            assert got[f, :, :W].tobytes() == exp[k][f].tobytes(), (what, p["call"], f)

    try:
        drive(hip_ctx, steps, call)
    finally:
        plan.close()


def test_hog_options_change_on_the_plans_own_cell_map(hip_ctx):
    """compvhip_plan_hog with d_cells NULL: the cell map is the plan's (hogCells, allocated once at the size of the largest call) while bin count, cell size and
    norm -- and with them the map's layout -- and the content change between calls.  Descriptors against tests/hog_model.py by bit pattern; the floats behind
    descLen keep the sentinel."""
    import hog_model as hm
    import hog_rig as gh
    steps = cs.hog_sequence()
    W, H = cs.HOG_SIZE
    geo = [hm.geometry(W, H, hm.resolve(p["opts"])) for _, p in steps]
    big = max(range(len(steps)), key=lambda k: geo[k]["descLen"])
    rig = gh.Rig(hip_ctx, steps[big][0], steps[big][1]["opts"])          # buffers of the largest descriptor; the stride stays
    exp = [[hm.hog(f, p["opts"]) for f in fr] for fr, p in steps]
    rng = np.random.default_rng(W)

    def call(k, what):
        fr, p = steps[k]
        rig.set_content(fr, p["opts"], rng)
        rig.run(cells=False)
        rig.check(what, exp[k], cells=False)

    try:
        drive(hip_ctx, steps, call)
    finally:
        rig.close()


def test_pure_functions_of_their_inputs_one_step_each(hip_ctx, oracle):
    """Grayscale, the bilinear scale and the inverse warp carry nothing from call to call: each is one launch that reads the caller's frames and writes the caller's
    output, with no counter and no plan-owned plane in between (the warp's running-sum tables are the only plan-owned bytes, computed on the host and uploaded
    whole by every call), so a sequence could only repeat what tests/test_gpu_preproc.py, test_gpu_scale.py and test_gpu_remap.py check at every geometry.  One
    step each, on a plan that has just run other content through its scratch-owning calls, shows that those leave them alone."""
    import orb_pyramid_model as pm
    import remap_model as rm
    from compv_amd import capi
    W, H, S = cs.SCRATCH_GEOMETRY
    fr = cs.otsu_sequence()[0][0]
    A = Arena()
    rng = np.random.default_rng(3)
    d_in = A.new(cs.F * H * S, pg.pad_frames(fr, S, rng))
    A.keep(d_in, d_in.cpu().numpy())
    rgb = np.stack([pg.rgb_of(f).reshape(H, W * 3) for f in fr])
    d_rgb = A.new(cs.F * H * S * 3, pg.pad_frames(rgb, S * 3, rng))
    A.keep(d_rgb, d_rgb.cpu().numpy())
    d_gray = A.new(cs.F * H * S)
    d_otsu = A.new(cs.F * 4)
    ow, oh, os_ = 131, 37, 136
    d_scaled = A.new(cs.F * oh * os_)
    plan = capi.Plan(hip_ctx, W, H, S, cs.F)
    try:
        plan.otsu(ptr(d_in), ptr(d_otsu))                       # scratch-owning calls first
        plan.morph(ptr(d_in), np.full((3, 3), 255, np.uint8), capi.MORPH_OPEN, capi.BORDER_REPLICATE, ptr(d_gray))
        A.refill(d_gray)
        plan.grayscale(ptr(d_rgb), capi.FMT_RGB24, ptr(d_gray))
        A.check("grayscale")
        pg.assert_maps(pg.frames_view(d_gray, cs.F, H, S, W), [oracle.grayscale(r, capi.FMT_RGB24, W) for r in rgb], "grayscale")
        A.refill(d_scaled)
        plan.scale(ptr(d_in), ptr(d_scaled), ow, oh, os_)
        A.check("scale")
        got = d_scaled.cpu().numpy().reshape(cs.F, oh, os_)
        assert (got[:, :, ow:] == SENTINEL).all(), "scale: columns >= Wout written"
        for f in range(cs.F):
            assert got[f, :, :ow].tobytes() == pm.scale(fr[f], ow, oh).tobytes(), ("scale", f)
        M = np.array([[1.02, 0.03, -2.0], [-0.01, 0.98, 1.5]], np.float32)
        A.refill(d_scaled)
        plan.warp_inverse(ptr(d_in), M, capi.INTERP_BILINEAR, ptr(d_scaled), ow, oh, os_, default=9)
        A.check("warp_inverse")
        got = d_scaled.cpu().numpy().reshape(cs.F, oh, os_)
        assert (got[:, :, ow:] == SENTINEL).all(), "warp_inverse: columns >= Wout written"
        for f in range(cs.F):
            assert got[f, :, :ow].tobytes() == rm.warp_inverse(fr[f], M, ow, oh, rm.BILINEAR, 9).tobytes(), ("warp_inverse", f)
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (c) segments, fits and components behind every step of (a)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_plan_segments_fits_and_components_after_each_step(plan_rig):
    """After every pipeline step of sequence (a): the segments of its first lines, their fits per line and per segment, and the connected components, on the plan's own masks and on the
    caller's bytes of another class than the masks hold (the oracle's edges of the step two further on), while minLength, maxGap, halfWidth, connectivity 4 <-> 8
    and minPixels change, compCap goes 0 -> 64, and d_labels goes NULL (the plan's compParent) -> given -> NULL.  A dense frame comes before an empty one in every
    frame slot, so segPerLine, compRows, compBits and compParent hold large stale numbers when the empty frame is walked.  Against tests/sht_segments_model.py,
    tests/sht_fit_model.py and tests/components_model.py; records behind a count and label columns >= W keep the sentinel (the stage tests' checkers)."""
    import components_rig as gc
    import sht_fit_rig as gfit
    import sht_segments_rig as gseg
    r, o = plan_rig, plan_rig.outs[0]
    capi = r.capi
    K = len(r.steps)
    sinQ, cosQ = gseg.tables(r.oracle, r.W, r.H, 1.0)
    seg_cap = fit_cap = 16384          # above every segment count of the sequence, so the per-segment fits see every segment
    d_segs, d_sc = r.A.new(cs.F * seg_cap * SEG_BYTES), r.A.new(cs.F * 4)
    d_fits, d_fc = r.A.new(cs.F * fit_cap * FIT_BYTES), r.A.new(cs.F * 4)
    outs = [gc.Out(r.A, cs.F, r.H, r.W + 3, cap, labels=lab) for lab, cap in cs.FEATURE_OUTPUTS]
    foreign, exp = [], []
    for k in range(K):
        prm, fp = r.steps[k][1], cs.FEATURE_PARAMS[k]
        cut = min(cs.FEATURE_LINES, prm["max_lines"]) if prm["max_lines"] > 0 else cs.FEATURE_LINES
        lines = [np.array(x[2][:min(len(x[2]), r.cap)], capi.LINE_DTYPE) for x in r.exp[k]]
        own = [x[0] for x in r.exp[k]]
        other = [x[0] for x in r.exp[(k + 2) % K]]
        foreign.append(r.device_frames(np.stack(other), pad=255))
        per = {}
        for how, maps in (("masks", own), ("bytes", other)):
            sp = (fp["min_length"], fp["max_gap"])
            segs = gseg.model_frames(maps, sinQ, cosQ, lines, [sp], cut)[sp]
            assert max(len(x) for x in segs) <= seg_cap
            per[how] = dict(segs=segs, fits=gfit.model_fits(maps, sinQ, cosQ, r.R, lines, fp["half_width"], cut)[0],
                            seg_fits=gfit.model_fits(maps, sinQ, cosQ, r.R, lines, fp["half_width"], cut, segs=segs)[0],
                            comps=gc.model(maps, fp["conn"], fp["min_pixels"]))
        exp.append((cut, per))

    def call(k, what):
        fp = cs.FEATURE_PARAMS[k]
        cut, per = exp[k]
        out = outs[k % len(outs)]
        r.refill(o)
        r.pipeline(k, o)
        r.check_lines(k, o, what)
        for how, de in (("masks", 0), ("bytes", ptr(foreign[k]))):
            w = "%s, %s" % (what, how)
            for d in (d_segs, d_sc, d_fits, d_fc):
                r.A.refill(d)
            out.refill()
            r.plan.houghsht_segments(de, ptr(o["lines"]), ptr(o["counts"]), r.cap, cut, fp["min_length"], fp["max_gap"], ptr(d_segs), seg_cap, ptr(d_sc))
            r.plan.houghsht_fit(de, ptr(o["lines"]), ptr(o["counts"]), r.cap, cut, fp["half_width"], 0, 0, 0, ptr(d_fits), fit_cap, ptr(d_fc))
            out.call(r.plan, de, fp["conn"], fp["min_pixels"])
            r.A.check(w)
            gseg.assert_segments(d_segs, d_sc, cs.F, seg_cap, per[how]["segs"], w + " segments")
            gfit.assert_fits(d_fits, d_fc, cs.F, fit_cap, per[how]["fits"], w + " fits")
            gc.assert_result(out, r.W, per[how]["comps"], w + " components")
            r.A.refill(d_fits); r.A.refill(d_fc)          # per segment, on the segments the plan has just written
            r.plan.houghsht_fit(de, ptr(o["lines"]), ptr(o["counts"]), r.cap, cut, fp["half_width"], ptr(d_segs), ptr(d_sc), seg_cap, ptr(d_fits), fit_cap, ptr(d_fc))
            r.A.check(w + " fits per segment")
            gfit.assert_fits(d_fits, d_fc, cs.F, fit_cap, per[how]["seg_fits"], w + " fits per segment")

    drive(r.ctx, r.steps, call)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (h) KHT on a plan
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_plan_houghkht_sequence_in_both_orders(hip_ctx, oracle, monkeypatch):
    """compvhip_plan_houghkht and _ex (canonical) alternate on one plan over edge maps that are busy, empty, then busy with other lines -- rotated over the frames --
    while COMPVHIP_KHT_GROUP splits the batch into three groups, two, or leaves it whole.  The pooled per-group buffers (strings, clusters, kernels, vote maps,
    the canonical peak lists) grow on demand and are never cleared; an empty frame after a busy one must return no line and leave its GS untouched.  The reference
    order against the oracle, the canonical order against tests/kht_canon_model.py, as tests/test_gpu_kht_canonical.py compares them."""
    import kht_canon_model as gk
    from compv_amd import capi
    from kht_canon_model import CanonModel
    W, H, S = cs.KHT_GEOMETRY
    steps = cs.kht_sequence()
    model = CanonModel(oracle)
    exp = []
    for maps, p in steps:
        if p["order"] == "canonical":
            exp.append([model.lines(e, threshold=p["threshold"])[:2] for e in maps])
        else:
            exp.append([oracle.kht(e, 1.0, 1.0, p["threshold"]) for e in maps])
    A = Arena()
    rng = np.random.default_rng(H)
    hosts = [pg.pad_frames(maps, S, rng) for maps, _ in steps]
    d_maps = [A.new(h.size, h) for h in hosts]
    for d, h in zip(d_maps, hosts):
        A.keep(d, h)
    plan = capi.Plan(hip_ctx, W, H, S, cs.F, 1.0)

    def call(k, what):
        p = steps[k][1]
        if p["group"] is None:
            monkeypatch.delenv("COMPVHIP_KHT_GROUP", raising=False)
        else:
            monkeypatch.setenv("COMPVHIP_KHT_GROUP", str(p["group"]))
        lines, gs = plan.houghkht(ptr(d_maps[k]), 1.0, 1.0, p["threshold"], order=p["order"])
        A.check(what)
        for f in range(cs.F):
            el, egs = exp[k][f]
            if p["order"] == "canonical":
                assert gk.line_bits(lines[f]) == gk.model_line_bits(el), (what, f)
                assert gs[f] == egs, (what, f)
            else:
                assert [(float(l["rho"]), float(l["theta"]), int(l["strength"])) for l in lines[f]] == \
                       [(float(np.float32(l[0])), float(np.float32(l[1])), int(l[2])) for l in el], (what, f)
                assert (gs[f] == egs) if len(el) else (gs[f] is None), (what, "gs", f)

    try:
        drive(hip_ctx, steps, call)
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (d) ORB and the ORB pyramid
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", cs.ORB_GEOMETRIES, ids=lambda g: "%dx%d_S%d_F%d" % g)
def test_orb_keypoints_and_describe_sequence(hip_ctx, geom):
    """compvhip_plan_orb_keypoints and _describe on one plan: the content goes many corners -> none -> a handful, the device corner counts go the whole list ->
    none -> three, both rotated over the frames, while level and scale change, keyCap alternates 0 with > 0 and blur alternates 1 (the plan's orbBlur plane)
    with 0 (the caller's blurred frames).  Watches orbIndex (the survivors' indices, never cleared) and orbBlur; counts, records, moments and rows against
    tests/orb_model.py, and nothing behind a list or a row is written."""
    import orb_model as om
    import orb_rig as go
    W, H, S, F = geom
    steps = cs.orb_sequence(W, H)
    rig = go.Rig(hip_ctx, geom, 7, 260)
    full = [len(c) for c in rig.lists]
    rng = np.random.default_rng(W)
    d_blurred = [rig.ar.new(F * H * S, pg.pad_frames(np.stack([om.blur(f) for f in fr]), S, rng)) for fr, _ in steps]

    def call(k, what):
        fr, p = steps[k]
        rig.set_content(fr, rng, [full[f] if c == "all" else 0 if c == "none" else min(c, full[f]) for f, c in enumerate(p["counts"])])
        rig.refill()
        cap = rig.key_cap if p["records"] else 0
        exp = rig.expected(p["level"], np.float32(p["scale"]))
        rig.keypoints(p["level"], np.float32(p["scale"]), moments=p["moments"], key_cap=cap)
        rig.check_keypoints(what, exp, moments=p["moments"], key_cap=cap)
        if not cap:
            return
        rig.describe(np.float32(p["scale"]), blur=p["blur"], d_gray=None if p["blur"] else d_blurred[k])
        rig.ar.check(what + " describe")
        rows = rig.d_desc.cpu().numpy().reshape(F, rig.key_cap, rig.desc_stride)
        for f in range(F):
            e = om.describe(om.blur(fr[f]), exp[f][0][:rig.key_cap], np.float32(p["scale"]))
            assert rows[f, :len(e), :32].tobytes() == e.tobytes(), (what, "rows", f)
            assert (rows[f, len(e):] == SENTINEL).all(), (what, "wrote behind its rows", f)

    try:
        drive(hip_ctx, steps, call)
    finally:
        rig.close()


def test_orb_pyramid_sequence(hip_ctx):
    """One compvhip_orbpyr of five levels: detect, then describe with rebuilt planes, on content that goes many corners -> none -> a handful at other positions,
    rotated over the frames.  The level planes (plain and blurred), the per-level FAST scratch and corner lists and the keypoint staging are the handle's and are
    never cleared.  Every level's plane, FAST count, survivor count and record, and every row, against tests/orb_pyramid_model.py."""
    import orb_model as om
    import orb_pyramid_model as pm
    import orb_pyramid_rig as gp
    geom = cs.ORBPYR_GEOMETRY
    W, H, S, levels, sf, mf = geom
    steps = cs.orbpyr_sequence()
    geo = pm.geometry(W, H, levels, sf, mf)
    assert levels >= 4 and not any(g["empty"] for g in geo)
    exp = [[pm.detect(img, levels, sf, gp.THRESHOLD, 9, True, mf, None) for img in fr] for fr, _ in steps]
    rig = gp.Rig(hip_ctx, geom, key_cap=max(len(e[0]) for ex in exp for e in ex) + 7, desc_stride=36)
    rng = np.random.default_rng(W)

    def call(k, what):
        fr, _ = steps[k]
        rig.set_content(fr, rng)
        for d in (rig.d_keys, rig.d_kcounts, rig.d_lcounts, rig.d_lcorners, rig.d_desc):
            rig.ar.refill(d)
        rig.detect()
        rig.check_detect(what + " detect", exp[k])
        for l in range(levels):
            got = rig.level_planes(l, geo)
            for f in range(gp.F):
                assert (got[f] == exp[k][f][3][l]).all(), (what, "plane of level", l, f)
        rig.pyr.describe(ptr(rig.d_in), ptr(rig.d_keys), rig.key_cap, ptr(rig.d_kcounts), ptr(rig.d_desc), rig.desc_stride, reuse_planes=False)
        rig.ar.check(what + " describe")
        rig.check_rows(what + " rows", rig.rows(), [pm.describe(e[3], geo, e[0]) for e in exp[k]], [len(e[0]) for e in exp[k]])
        for l in range(levels):
            got = rig.level_planes(l, geo, blurred=True)
            for f in range(gp.F):
                assert (got[f] == om.blur(exp[k][f][3][l])).all(), (what, "blurred plane of level", l, f)

    try:
        drive(hip_ctx, steps, call)
    finally:
        rig.close()
