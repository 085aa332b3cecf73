"""The Canny hysteresis (canny_resolve_kernel, and the speculative rounds / replay / flag-slot wrap of api.cpp) on adversarial chains,
heterogeneous batches and replays, bit for bit against the oracle.

The cases come from tests/hysteresis_cases.py; tests/test_hysteresis_cases.py proves on the CPU what each of them crosses and how many
launches it needs at least.  Every device buffer sits between guard pages and every output starts filled with a sentinel (the Arena of
tests/gpu_support.py).  A test that claims extra rounds or a replay shows that they happened: with plan.set_timing(1) the
timeline of the last synchronous call (or of the replay inside compvhip_plan_wait, which runs as a synchronous step) holds one
"canny_resolve_kernel" entry per launch; COMPVHIP_TRACE_ROUNDS=1 (read when a plan is made) prints what an asynchronous
ticket saw."""
import numpy as np
import pytest

import hysteresis_cases as hc
from oracle_bindings import synth_frame
from gpu_support import (LINE_CAP, Arena, assert_lines, assert_maps, check_accs, edge_counts, frames_view, pad_frames, pool, ptr,
                                    sht_expect)

pytestmark = pytest.mark.gpu

ROWS = [(c["name"], ks) for c in hc.CASES for ks in c["ksizes"]]
EASY = (59.0, 119.0)
DEEP = "zigzag-chunk-k26"      # 2300 x 330: two cell columns, six bands, 26 crossings of x = 2048


def stride_for(W):
    return (W + 7) // 8 * 8 + 8


def resolve_launches(plan):
    return sum(1 for name, _ in plan.get_timing(4096) if name == "canny_resolve_kernel")


def oracle_maps(oracle, imgs, tl, th, ksize=3):
    def one(img):
        rc, e = oracle.canny(img, tl, th, ksize)
        assert rc == 0
        return e
    with pool() as ex:
        return list(ex.map(one, imgs))


def min_launches(oracle, img, tl, th, ksize=3):
    """Launches the GPU needs at least on this frame: the productive ones of the topological bound plus the one that confirms."""
    rc, _, g = oracle.canny(img, tl, th, ksize, 0, want_gnms=True)
    rc, lo, hi = oracle.canny_thresholds(tl, th, 0)
    weak, strong = hc.masks(g, lo, hi)
    k, cells = hc.crossing_depth(weak, strong)
    return hc.launches_lower_bound(k, cells) + 1 if k >= 0 else 1


class Batch:
    """A guarded input batch with padded rows and the output buffers of a plan."""

    def __init__(self, imgs, seed=1, lines=False, keep_input=True):
        self.imgs = imgs = np.stack(imgs)
        self.F, self.H, self.W = imgs.shape
        self.S = stride_for(self.W)
        self.A = Arena()
        self.n = self.F * self.H * self.S
        self.host_in = pad_frames(imgs, self.S, np.random.default_rng(seed))
        self.d_in = self.A.new(self.n, self.host_in)
        if keep_input:                                              # in-place callers overwrite it
            self.A.keep(self.d_in, self.host_in)
        self.d_out = self.A.new(self.n)
        if lines:
            self.d_lines = self.A.new(self.F * LINE_CAP * 20)
            self.d_counts = self.A.new(self.F * 4)

    def plan(self, ctx, timing=True):
        from compv_amd import capi
        p = capi.Plan(ctx, self.W, self.H, self.S, self.F, 1.0)
        if timing:
            p.set_timing(1)
        return p

    def out(self, buf=None):
        return frames_view(self.d_out if buf is None else buf, self.F, self.H, self.S, self.W)

    def refill(self):
        self.A.refill(self.d_out)
        if hasattr(self, "d_lines"):
            self.A.refill(self.d_lines); self.A.refill(self.d_counts)

    def counts(self):
        return self.d_counts.cpu().numpy().view(np.int32)

    def raw_lines(self):
        return self.d_lines.cpu().numpy().reshape(self.F, LINE_CAP, 20)


def sht_threshold(W, H):
    return max(3, min(W, H) // 2)


def check_step(b, plan, oracle, exp, what, accs=True):
    """Edge maps, line records in order, line counts, per-frame edge counts and accumulators of every frame of a pipeline step."""
    thr = sht_threshold(b.W, b.H)
    b.A.check(what)
    assert_maps(b.out(), exp, what)
    with pool() as ex:
        sx = list(ex.map(lambda e: sht_expect(oracle, e, 1.0, thr), exp))
    assert_lines(b.raw_lines(), b.counts(), [x[1] for x in sx], what)
    assert edge_counts(plan, b.F).tolist() == [int((e != 0).sum()) for e in exp], what
    if accs:
        R, T, _ = oracle.sht_dims(b.W, b.H, 1.0)
        check_accs(plan, b.A, b.F, R, T, [x[0] for x in sx], what)


# ---------------------------------------------------------------------------------------------------------------
# every row of the table: host entry and batched plan, in all eight orientations
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ksize", ROWS, ids=lambda v: str(v))
def test_case_through_host_entry(hip_ctx, oracle, name, ksize):
    case = hc.BY_NAME[name]
    tl, th = hc.thresholds_for(case, ksize)
    same, transposed = hc.variants(case["gen"]())
    imgs = same + transposed
    for i, (img, e) in enumerate(zip(imgs, oracle_maps(oracle, same, tl, th, ksize) + oracle_maps(oracle, transposed, tl, th, ksize))):
        got = hip_ctx.canny(img, tl, th, ksize)
        assert_maps([got], [e], "%s variant %d" % (name, i))


@pytest.mark.parametrize("name,ksize", ROWS, ids=lambda v: str(v))
def test_case_through_plan_batch(hip_ctx, oracle, name, ksize):
    """The row's frame and its three flips in one launch, the four transposed ones in a second plan."""
    case = hc.BY_NAME[name]
    tl, th = hc.thresholds_for(case, ksize)
    for group, imgs in enumerate(hc.variants(case["gen"]())):
        exp = oracle_maps(oracle, imgs, tl, th, ksize)
        need = max(min_launches(oracle, img, tl, th, ksize) for img in imgs)
        b = Batch(imgs, seed=len(name) + group)
        plan = b.plan(hip_ctx)
        try:
            plan.canny(ptr(b.d_in), tl, th, ptr(b.d_out), ksize)
            b.A.check(name)
            assert_maps(b.out(), exp, "%s group %d" % (name, group))
            n = resolve_launches(plan)
            print("%s ksize %d group %d: %d resolve launches, at least %d needed" % (name, ksize, group, n, need))
            assert n >= need, (n, need)
        finally:
            plan.close()


# ---------------------------------------------------------------------------------------------------------------
# one deep frame among easy ones
# ---------------------------------------------------------------------------------------------------------------
def hetero_batch(name, F, pos):
    case = hc.BY_NAME[name]
    deep = case["gen"]()
    H, W = deep.shape
    return [deep if f == pos else synth_frame(W, H, 70 + f) for f in range(F)]


@pytest.mark.parametrize("name,F,pos", [(DEEP, 2, 0), (DEEP, 9, 4), ("zigzag-band-k18", 33, 32), ("spiral", 2, 1)], ids=lambda v: str(v))
def test_one_deep_frame_in_a_batch(hip_ctx, oracle, name, F, pos):
    """canny and the synchronous pipeline on a batch in which one frame needs many rounds and the others none: the replayed Hough tail
    must not count the converged frames twice (edge counts, accumulators, line counts)."""
    imgs = hetero_batch(name, F, pos)
    tl, th = hc.T_LOW, hc.T_HIGH
    exp = oracle_maps(oracle, imgs, tl, th)
    need = min_launches(oracle, imgs[pos], tl, th)
    assert need > hc.SPEC_ROUNDS
    b = Batch(imgs, seed=F, lines=True)
    plan = b.plan(hip_ctx)
    try:
        plan.canny(ptr(b.d_in), tl, th, ptr(b.d_out))
        b.A.check("canny")
        assert_maps(b.out(), exp, "canny")
        n = resolve_launches(plan)
        assert n >= need and n > hc.SPEC_ROUNDS, (n, need)
        b.refill()
        thr = sht_threshold(b.W, b.H)
        plan.pipeline(ptr(b.d_in), tl, th, thr, 0, ptr(b.d_out), ptr(b.d_lines), LINE_CAP, ptr(b.d_counts))
        n2 = resolve_launches(plan)
        print("%s F %d pos %d: canny %d launches, pipeline %d (at least %d)" % (name, F, pos, n, n2, need))
        assert n2 >= need and n2 > hc.SPEC_ROUNDS, (n2, need)       # more than the blind rounds: the tail was replayed
        check_step(b, plan, oracle, exp, "pipeline", accs=F <= 9)
        if F > 9:
            R, T, _ = oracle.sht_dims(b.W, b.H, 1.0)
            sub = sorted({0, pos, F // 2, F - 2})
            for f in sub:
                d_acc = b.A.new(R * T * 4)
                plan.acc_export(f, ptr(d_acc), T)
                assert (d_acc.cpu().numpy().view(np.int32).reshape(R, T) == oracle.sht_acc(exp[f], 1.0)).all(), ("acc", f)
    finally:
        plan.close()


def test_in_place_canny_after_extra_rounds(hip_ctx, oracle):
    """d_edges == d_in on a deep batch: the scratch map goes back to the caller's buffer after the extra rounds."""
    imgs = hetero_batch(DEEP, 3, 1)
    exp = oracle_maps(oracle, imgs, hc.T_LOW, hc.T_HIGH)
    b = Batch(imgs, seed=3, lines=True, keep_input=False)
    plan = b.plan(hip_ctx)
    try:
        plan.canny(ptr(b.d_in), hc.T_LOW, hc.T_HIGH, ptr(b.d_in))
        b.A.check("canny in place")
        assert_maps(b.out(b.d_in), exp, "canny in place")
        n = resolve_launches(plan)
        assert n > hc.SPEC_ROUNDS, n
        # the synchronous step in place: its copy back runs again after the rounds the first check asked for
        b.d_in.copy_(b.A.torch.from_numpy(b.host_in.reshape(-1)))
        thr = sht_threshold(b.W, b.H)
        plan.pipeline(ptr(b.d_in), hc.T_LOW, hc.T_HIGH, thr, 0, ptr(b.d_in), ptr(b.d_lines), LINE_CAP, ptr(b.d_counts))
        b.A.check("pipeline in place")
        n2 = resolve_launches(plan)
        print("in place: canny %d launches, pipeline %d" % (n, n2))
        assert n2 > hc.SPEC_ROUNDS, n2
        assert_maps(b.out(b.d_in), exp, "pipeline in place")
        assert edge_counts(plan, b.F).tolist() == [int((e != 0).sum()) for e in exp]
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------
# asynchronous steps
# ---------------------------------------------------------------------------------------------------------------
def async_fixture(oracle, F=4, pos=2):
    deep = hetero_batch(DEEP, F, pos)
    H, W = deep[0].shape
    easy = [synth_frame(W, H, 300 + f) for f in range(F)]
    return deep, easy, oracle_maps(oracle, deep, hc.T_LOW, hc.T_HIGH), oracle_maps(oracle, easy, *EASY)


def trace_lines(capfd):
    return [l for l in capfd.readouterr().err.splitlines() if "rounds enqueued" in l]


def needed_of(line):
    return int(line.split("needed ")[1].split()[0])


def test_async_deep_step_second_with_shared_outputs(hip_ctx, oracle, monkeypatch, capfd):
    """Two tickets in flight on ONE set of output buffers, the deep step second (the existing test has it first).  Step 0 converges
    within its blind rounds; wait(1) must complete the deep step by a replay, after which the shared buffers hold its results."""
    monkeypatch.setenv("COMPVHIP_TRACE_ROUNDS", "1")
    deep, easy, exp_deep, exp_easy = async_fixture(oracle)
    b = Batch(easy, seed=5, lines=True)
    d_deep = b.A.new(b.n, pad_frames(np.stack(deep), b.S, np.random.default_rng(6)))
    plan = b.plan(hip_ctx)
    thr = sht_threshold(b.W, b.H)
    try:
        t0 = plan.pipeline_async(ptr(b.d_in), EASY[0], EASY[1], thr, 0, ptr(b.d_out), ptr(b.d_lines), LINE_CAP, ptr(b.d_counts))
        t1 = plan.pipeline_async(ptr(d_deep), hc.T_LOW, hc.T_HIGH, thr, 0, ptr(b.d_out), ptr(b.d_lines), LINE_CAP, ptr(b.d_counts))
        plan.wait(t0)
        plan.wait(t1)
        n = resolve_launches(plan)
        tr = trace_lines(capfd)
        print("async shared, deep second: replay with %d launches; trace: %s" % (n, tr))
        assert len(tr) == 2 and needed_of(tr[0]) <= hc.SPEC_ROUNDS and needed_of(tr[1]) > hc.SPEC_ROUNDS, tr
        assert n > 2 * hc.SPEC_ROUNDS, n                          # more than the blind rounds of both tickets: only a replay gives that
        check_step(b, plan, oracle, exp_deep, "deep step second")
    finally:
        plan.close()


def test_async_deep_step_first_with_shared_outputs(hip_ctx, oracle, monkeypatch, capfd):
    """The batch form of the existing shared-buffer test: the deep step first, an easy step behind it on the same output buffers.
    wait(0) replays step 0 after step 1 ran; wait(1) must then bring step 1's results back."""
    monkeypatch.setenv("COMPVHIP_TRACE_ROUNDS", "1")
    deep, easy, exp_deep, exp_easy = async_fixture(oracle, pos=1)
    b = Batch(deep, seed=14, lines=True)
    d_easy = b.A.new(b.n, pad_frames(np.stack(easy), b.S, np.random.default_rng(15)))
    plan = b.plan(hip_ctx)
    thr = sht_threshold(b.W, b.H)
    try:
        t0 = plan.pipeline_async(ptr(b.d_in), hc.T_LOW, hc.T_HIGH, thr, 0, ptr(b.d_out), ptr(b.d_lines), LINE_CAP, ptr(b.d_counts))
        t1 = plan.pipeline_async(ptr(d_easy), EASY[0], EASY[1], thr, 0, ptr(b.d_out), ptr(b.d_lines), LINE_CAP, ptr(b.d_counts))
        plan.wait(t0)
        n = resolve_launches(plan)
        tr = trace_lines(capfd)
        print("async shared, deep first: replay with %d launches; trace: %s" % (n, tr))
        assert len(tr) == 1 and needed_of(tr[0]) > hc.SPEC_ROUNDS, tr
        assert n > 2 * hc.SPEC_ROUNDS, n                          # more than the blind rounds of both tickets: only a replay gives that
        check_step(b, plan, oracle, exp_deep, "deep step first")
        plan.wait(t1)
        check_step(b, plan, oracle, exp_easy, "easy step behind a replayed one")
    finally:
        plan.close()


def test_async_separate_buffers_waited_in_reverse(hip_ctx, oracle, monkeypatch, capfd):
    """Two tickets with their own buffers, the deep step first, waited for in the order 1, 0."""
    monkeypatch.setenv("COMPVHIP_TRACE_ROUNDS", "1")
    deep, easy, exp_deep, exp_easy = async_fixture(oracle, pos=0)
    bd = Batch(deep, seed=7, lines=True)
    be = Batch(easy, seed=8, lines=True)
    plan = bd.plan(hip_ctx)
    thr = sht_threshold(bd.W, bd.H)
    try:
        t0 = plan.pipeline_async(ptr(bd.d_in), hc.T_LOW, hc.T_HIGH, thr, 0, ptr(bd.d_out), ptr(bd.d_lines), LINE_CAP, ptr(bd.d_counts))
        t1 = plan.pipeline_async(ptr(be.d_in), EASY[0], EASY[1], thr, 0, ptr(be.d_out), ptr(be.d_lines), LINE_CAP, ptr(be.d_counts))
        plan.wait(t1)
        be.A.check("easy step")
        assert_maps(be.out(), exp_easy, "easy step, waited first")
        plan.wait(t0)
        n = resolve_launches(plan)
        tr = trace_lines(capfd)
        print("async separate, wait 1 then 0: replay with %d launches; trace: %s" % (n, tr))
        assert len(tr) == 2 and needed_of(tr[1]) > hc.SPEC_ROUNDS, tr
        assert n > 2 * hc.SPEC_ROUNDS, n                          # more than the blind rounds of both tickets: only a replay gives that
        check_step(bd, plan, oracle, exp_deep, "deep step, waited last")
        # the easy step's own buffers are untouched by the deep step's replay
        assert_maps(be.out(), exp_easy, "easy step after the replay")
        with pool() as ex:
            sx = list(ex.map(lambda e: sht_expect(oracle, e, 1.0, thr), exp_easy))
        assert_lines(be.raw_lines(), be.counts(), [x[1] for x in sx], "easy step after the replay")
    finally:
        plan.close()


def test_async_batch_learns_two_rounds_then_recovers(hip_ctx, oracle, monkeypatch, capfd):
    """Six easy steps teach the plan two blind rounds; the deep batch then needs a replay; an easy step after it is right again."""
    monkeypatch.setenv("COMPVHIP_TRACE_ROUNDS", "1")
    deep, easy, exp_deep, exp_easy = async_fixture(oracle, pos=3)
    b = Batch(easy, seed=9, lines=True)
    d_deep = b.A.new(b.n, pad_frames(np.stack(deep), b.S, np.random.default_rng(10)))
    plan = b.plan(hip_ctx)
    thr = sht_threshold(b.W, b.H)
    seq = [(b.d_in, EASY, exp_easy)] * 6 + [(d_deep, (hc.T_LOW, hc.T_HIGH), exp_deep), (b.d_in, EASY, exp_easy)]
    try:
        for i, (d_in, (tl, th), exp) in enumerate(seq):
            b.refill()
            plan.wait(plan.pipeline_async(ptr(d_in), tl, th, thr, 0, ptr(b.d_out), ptr(b.d_lines), LINE_CAP, ptr(b.d_counts)))
            check_step(b, plan, oracle, exp, "step %d" % i, accs=(i >= 6))
            if i == 6:
                n = resolve_launches(plan)
                assert n > 7 * hc.SPEC_ROUNDS, n                  # more than the blind rounds of all seven tickets so far
        tr = trace_lines(capfd)
        print("async sequence: replay with %d launches; trace: %s" % (n, tr))
        assert len(tr) == 8
        enq = int(tr[6].split("rounds enqueued ")[1].split(",")[0])
        assert needed_of(tr[6]) == enq + 1, tr[6]                       # every blind round of the deep step changed something
        assert all(needed_of(l) <= hc.SPEC_ROUNDS for l in tr[:6] + tr[7:]), tr
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------
# per-frame thresholds
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,factors", [("mean", (0.3, 2.0)), ("otsu", (0.3, 1.5))])
def test_per_frame_thresholds_keep_and_drop_the_same_chain(hip_ctx, oracle, mode, factors):
    """Frames that differ in brightness only get different thresholds under PERCENT_OF_MEAN and OTSU: the deep chain is kept in one frame
    and dropped in its neighbour."""
    from compv_amd import capi
    base = hc.BY_NAME["zigzag-band-k18"]["gen"]()
    bright = np.clip(base.astype(np.int32) + 100, 0, 255).astype(np.uint8)
    imgs = [base, bright, base, bright, base]
    thr, exp = [], []
    for img in imgs:
        if mode == "mean":
            rc, lo, hi = oracle.canny_thresholds(factors[0], factors[1], 1, int(img.sum(dtype=np.int64)), img.shape[1], img.shape[0])
            assert rc == 0
            rc, e = oracle.canny(img, factors[0], factors[1], 3, 1)
        else:
            lo, hi = oracle.otsu_canny_thresholds(oracle.otsu(img), *factors)
            rc, e = oracle.canny(img, float(lo), float(hi))
        assert rc == 0
        thr.append((lo, hi)); exp.append(e)
    assert thr[0] != thr[1] and thr[0][0] < thr[1][0]
    kept = [int((e != 0).sum()) for e in exp]
    assert kept[0] > 3000 and kept[1] < 200, kept                  # the chain is kept in the dark frames only
    b = Batch(imgs, seed=11)
    plan = b.plan(hip_ctx)
    try:
        plan.canny(ptr(b.d_in), factors[0], factors[1], ptr(b.d_out), 3, capi.THRESHOLD_PERCENT_OF_MEAN if mode == "mean" else capi.THRESHOLD_OTSU)
        b.A.check(mode)
        assert_maps(b.out(), exp, mode)
        n = resolve_launches(plan)
        print("per-frame thresholds (%s): %d resolve launches" % (mode, n))
        assert n > hc.SPEC_ROUNDS, n
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------
# more rounds than flag slots
# ---------------------------------------------------------------------------------------------------------------
def test_flag_slot_wrap_with_two_cell_columns_and_three_frames(oracle, monkeypatch):
    """COMPVHIP_RESOLVE_WRAP=8 (read when a plan is made): a 26-crossing chain over the chunk border, its mirror image and an easy frame
    in one batch; canny and the pipeline, twice each on the same plan."""
    from compv_amd import capi
    deep = hc.BY_NAME[DEEP]["gen"]()
    imgs = [deep, synth_frame(deep.shape[1], deep.shape[0], 5), np.ascontiguousarray(deep[::-1, ::-1])]
    tl, th = hc.T_LOW, hc.T_HIGH
    exp = oracle_maps(oracle, imgs, tl, th)
    need = max(min_launches(oracle, imgs[0], tl, th), min_launches(oracle, imgs[2], tl, th))
    monkeypatch.setenv("COMPVHIP_RESOLVE_WRAP", str(hc.WRAP_SLOTS))
    ctx = capi.Context(0)
    try:
        b = Batch(imgs, seed=12, lines=True)
        plan = b.plan(ctx)
        thr = sht_threshold(b.W, b.H)
        try:
            for rep in range(2):
                b.refill()
                plan.canny(ptr(b.d_in), tl, th, ptr(b.d_out))
                b.A.check("canny")
                n = resolve_launches(plan)
                assert n > hc.WRAP_SLOTS and n >= need, (n, need)       # the slots were reused
                assert_maps(b.out(), exp, "canny with wrap, run %d" % rep)
                b.refill()
                plan.pipeline(ptr(b.d_in), tl, th, thr, 0, ptr(b.d_out), ptr(b.d_lines), LINE_CAP, ptr(b.d_counts))
                n2 = resolve_launches(plan)
                print("wrap run %d: canny %d launches, pipeline %d (at least %d)" % (rep, n, n2, need))
                assert n2 > hc.WRAP_SLOTS, n2
                check_step(b, plan, oracle, exp, "pipeline with wrap, run %d" % rep, accs=(rep == 1))
        finally:
            plan.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# all-or-nothing twins side by side
# ---------------------------------------------------------------------------------------------------------------
def test_seeded_and_unseeded_mazes_alternate_in_one_batch(hip_ctx, oracle):
    """Eight frames, alternately the seeded maze (every weak pixel kept) and its twin without the seed (nothing kept): any leak between
    frames -- mask stride, per-frame dirty offset, the shared flag -- shows in tens of thousands of pixels."""
    a, z = hc.BY_NAME["maze-seeded"]["gen"](), hc.BY_NAME["maze-unseeded"]["gen"]()
    imgs = [a, z, z, a, a[::-1].copy(), z, a[:, ::-1].copy(), z]
    tl, th = hc.T_LOW, hc.T_HIGH
    exp = oracle_maps(oracle, imgs, tl, th)
    assert [bool(e.any()) for e in exp] == [True, False, False, True, True, False, True, False]
    b = Batch(imgs, seed=13, lines=True)
    plan = b.plan(hip_ctx)
    thr = sht_threshold(b.W, b.H)
    try:
        plan.canny(ptr(b.d_in), tl, th, ptr(b.d_out))
        b.A.check("canny")
        assert_maps(b.out(), exp, "canny")
        n = resolve_launches(plan)
        assert n > hc.SPEC_ROUNDS, n
        b.refill()
        plan.pipeline(ptr(b.d_in), tl, th, thr, 0, ptr(b.d_out), ptr(b.d_lines), LINE_CAP, ptr(b.d_counts))
        n2 = resolve_launches(plan)
        check_step(b, plan, oracle, exp, "pipeline")
        b.refill()
        plan.wait(plan.pipeline_async(ptr(b.d_in), tl, th, thr, 0, ptr(b.d_out), ptr(b.d_lines), LINE_CAP, ptr(b.d_counts)))
        n3 = resolve_launches(plan)
        print("maze twins: canny %d launches, pipeline %d, async replay %d" % (n, n2, n3))
        assert n2 > hc.SPEC_ROUNDS and n3 > hc.SPEC_ROUNDS, (n2, n3)
        check_step(b, plan, oracle, exp, "pipeline_async")
    finally:
        plan.close()
