"""Stream order: every asynchronous call behind pending work (include/compv_hip.h, "Stream order").  The rig, the content and the table of cases are
tests/stream_order_rig.py, whose docstring describes the method; the contract table is tests/stream_cases.py, the coverage table
docs/dispatch_coverage.md, "Stream order"."""
import pytest

import stream_cases as sc
from stream_order_rig import CASES, Env, Stall, differs, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def stall(hip_ctx):
    return Stall()


@pytest.mark.parametrize("cid", sorted(CASES))
def test_behind_pending_work(hip_ctx, oracle, stall, cid):
    env = Env(hip_ctx, oracle)
    try:
        s = CASES[cid](env)
        if hasattr(s, "custom"):
            print("%s: enqueue section %.3f ms" % (cid, s.custom(env, stall) * 1e3))
            return
        if hasattr(s, "host_expect"):          # a call whose results are the host's: the expected lists themselves must differ between the contents
            h = [s.host_expect(k) for k in range(3)]
            assert all(differs(h[a]["host lines"], h[b]["host lines"]) for a, b in ((0, 1), (0, 2), (1, 2))), cid
        spent = run(env, stall, cid, s)
        print("%s: enqueue section %.3f ms" % (cid, spent * 1e3))
    except RuntimeError as e:          # a HIP error (the binding's or torch's) ends the module: nothing more is started on a device that has faulted
        if getattr(e, "code", None) == -7 or "HIP error" in str(e):
            pytest.exit("%s: %s" % (cid, e), returncode=3)
        raise
    finally:
        env.close()


def test_the_case_list_matches_the_table():
    assert set(CASES) == set(sc.CASE_ROW)
