"""First calls on fresh, poisoned allocations (docs/dispatch_coverage.md, "Fresh allocations").

hipMalloc and hipHostMalloc promise nothing about the content of a block, and the library's kernels clear as little as possible: apart from a handful of
buffers cleared where they are allocated, every scratch buffer rests on "written whole before it is read".  The other GPU tests create their handles in a
young process, where a large fresh block holds zeros, and the content sequences check those arguments against what a previous VALID call left.  Here
compvhip_debug_alloc_fill (gpu_support.alloc_fill) makes every device and pinned block the library allocates hold one byte, every handle and context is
created inside such a block of the test's own, and its first calls are held bit for bit against the model or oracle of the stage's own GPU test.

Two bytes, for complementary reasons.  0xFF is NaN in every float, 65 535 in every accumulator cell, every flag and mask bit set and -1 in every int32 --
which `max(count, 0)` hides, hence 0x01: 16 843 009, a positive count that clamps to the capacity and then reads garbage records, and small non-zero
sums.  Nothing here is compared with a tolerance."""
import pytest

import fresh_memory_cases as fc
import stream_order_rig as rig
from gpu_support import alloc_fill

pytestmark = pytest.mark.gpu

FILLS = pytest.mark.parametrize("fill", fc.FILLS, ids=[fc.FILL_IDS[f] for f in fc.FILLS])


def hip_failure(e):
    return getattr(e, "code", None) == -7 or "HIP error" in str(e)


def guarded(what, fn):
    """a HIP error (the binding's or torch's) ends the module: nothing more is started on a device that has faulted"""
    try:
        fn()
    except RuntimeError as e:
        if hip_failure(e):
            pytest.exit("%s: %s" % (what, e), returncode=3)
        raise


@pytest.fixture(scope="module")
def stream():
    import torch
    return torch.cuda.Stream()          # non-blocking: it does not order against the null stream, on which an allocation is filled


@pytest.fixture
def own_ctx():
    """a context of the test's own, for what is created under fill and counted in it; never the session's, whose staging was allocated long ago"""
    from compv_amd import capi
    made = []

    def make():
        made.append(capi.Context(0))
        return made[-1]
    yield make
    for c in made:
        c.close()


@FILLS
@pytest.mark.parametrize("cid", sorted(rig.CASES))
def test_first_call_on_filled_memory(hip_ctx, oracle, stream, cid, fill):
    """every case of the stream-order rig without its warm-up: the handle, and whatever its first use and (the growth cases) its second allocate, are
    filled blocks.  The session's context only counts the allocations: the rig's calls take none of its staging"""
    env = rig.Env(hip_ctx, oracle)

    def body():
        with alloc_fill(fill):
            s = rig.CASES[cid](env)
            rig.run_cold(env, stream, cid, s)
    try:
        guarded(cid, body)
    finally:
        env.close()


@FILLS
@pytest.mark.parametrize("name", sorted(fc.FAMILIES))
def test_first_call_of_the_descriptor_stream_handles(own_ctx, name, fill):
    def body():
        with alloc_fill(fill):
            fc.FAMILIES[name](own_ctx())
    guarded(name, body)


@FILLS
@pytest.mark.parametrize("name", sorted(fc.HOST_CALLS))
def test_first_host_call_on_a_fresh_context(own_ctx, oracle, name, fill):
    """one entry family, twice, at two sizes, as the first and only user of a context created under fill: its stream's staging, the cached single-frame
    plan and that plan's first-use scratch are allocated at the first size and reallocated at the second"""
    def body():
        with alloc_fill(fill):
            ctx = own_ctx()
            for k, (W, H) in enumerate(fc.SIZES):
                fc.HOST_CALLS[name](ctx, oracle, W, H, k)
    guarded(name, body)


def test_the_hook(hip_ctx):
    from compv_amd import capi
    lib = hip_ctx.lib
    assert lib.compvhip_debug_alloc_fill(-1) == -1          # off by default, and off again behind every test above
    assert lib.compvhip_debug_alloc_fill(256) == capi.E_INVALID_PARAMETER and lib.compvhip_debug_alloc_fill(-2) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_debug_alloc_fill(-1) == -1          # a refusal changes nothing
    assert lib.compvhip_debug_alloc_fill(0) == -1 and lib.compvhip_debug_alloc_fill(255) == 0 and lib.compvhip_debug_alloc_fill(-1) == 255
    live = hip_ctx.live_allocations()
    with alloc_fill(0xFF):
        plan = capi.Plan(hip_ctx, 43, 49, 48, 3)
        assert hip_ctx.live_allocations() > live
        plan.close()
        assert hip_ctx.live_allocations() == live          # a filled block is counted once and returned once
        with alloc_fill(0x01):
            assert lib.compvhip_debug_alloc_fill(0x01) == 0x01
        assert lib.compvhip_debug_alloc_fill(0xFF) == 0xFF          # the inner block put the outer one's byte back
    assert lib.compvhip_debug_alloc_fill(-1) == -1
    with pytest.raises(ZeroDivisionError):
        with alloc_fill(7):
            assert lib.compvhip_debug_alloc_fill(7) == 7
            raise ZeroDivisionError
    assert lib.compvhip_debug_alloc_fill(-1) == -1          # restored behind an exception
    with pytest.raises(AssertionError):
        with alloc_fill(256):
            pass
    assert lib.compvhip_debug_alloc_fill(-1) == -1
