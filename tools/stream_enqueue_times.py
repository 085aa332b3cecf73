"""Warm host time of the enqueue section of every case of tests/stream_order_rig.py on an IDLE stream: the figures STALL_MS is derived from
(docs/dispatch_coverage.md, "Stream order").  It runs the test's own rig with stalled=False, so what is measured is what is tested.  Needs a GPU.

    python tools/stream_enqueue_times.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import stream_order_rig as t               # noqa: E402
from compv_amd import capi                 # noqa: E402
from oracle_bindings import Oracle         # noqa: E402


def main():
    ctx, orc, stall, ms = capi.Context(0), Oracle(), t.Stall(), {}
    for cid in sorted(t.CASES):
        for rep in range(2):          # the second pass is the warm one
            env = t.Env(ctx, orc)
            try:
                s = t.CASES[cid](env)
                ms[cid] = (s.custom(env, stall, stalled=False) if hasattr(s, "custom") else t.run(env, stall, cid, s, stalled=False)) * 1e3
            finally:
                env.close()
        print("%-30s %.3f ms" % (cid, ms[cid]), flush=True)
    slow = max(ms, key=ms.get)
    print("slowest: %s, %.3f ms; 50 x = %.1f ms" % (slow, ms[slow], 50 * ms[slow]))
    ctx.close()


if __name__ == "__main__":
    main()
