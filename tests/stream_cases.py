"""The stream-order contract of every export that enqueues on a caller's stream (include/compv_hip.h, "Stream order"): one row per export with a `void* stream`
parameter, plus the two batched KHT calls, which take no stream and drain the device.  Importable without a GPU; tests/test_stream_cases.py holds it against the
header, tests/test_gpu_stream_order.py against the library.

Classes
  ASYNC   everything the call does on the device is ordered on `stream`; on a warm handle it returns without waiting for the stream; host arrays and option
          structs may be changed as soon as it returns.
  WAITS   the same ordering, but the call may wait for the stream before it returns.
  DRAINS  no stream parameter: the call drains the whole device first.

`host`: the host arrays and structs the call reads (the GPU case overwrites each of them as soon as the call has returned).
`cases`: ids of tests/stream_order_rig.py::CASES; the first is the plain rig of the row, the others are the runs that need more (growth behind pending
work, in place, a ticket, timing mode)."""
from collections import namedtuple

ASYNC, WAITS, DRAINS = "ASYNC", "WAITS", "DRAINS"
CLASSES = (ASYNC, WAITS, DRAINS)
Row = namedtuple("Row", "export cls host cases")


def _row(export, cls, host=(), cases=None):
    short = export[len("compvhip_"):]
    for prefix in ("plan_",):
        if short.startswith(prefix):
            short = short[len(prefix):]
    return Row(export, cls, tuple(host), tuple(cases) if cases else (short,))


ROWS = (
    # ---- the Canny / SHT plan (api.cpp, api_kht.cpp)
    _row("compvhip_plan_canny", WAITS, cases=("canny", "canny_in_place")),
    _row("compvhip_plan_grayscale", ASYNC),
    _row("compvhip_plan_otsu", ASYNC),
    _row("compvhip_plan_convlt1_fixedpoint", ASYNC, host=("vtKern", "hzKern")),
    _row("compvhip_plan_to_cartesian", ASYNC),
    _row("compvhip_plan_edge_dete", ASYNC, cases=("edge_dete", "edge_dete_timing")),
    _row("compvhip_plan_houghsht", ASYNC, cases=("houghsht", "houghsht_line_caps", "houghsht_growth", "houghsht_library_sort")),
    _row("compvhip_plan_pipeline", WAITS),
    _row("compvhip_plan_pipeline_async", ASYNC),
    _row("compvhip_plan_pipeline_ex", WAITS, host=("opts",), cases=("pipeline_ex", "pipeline_ex_ticket")),
    _row("compvhip_plan_houghkht", DRAINS),
    _row("compvhip_plan_houghkht_ex", DRAINS, host=("opts",)),
    _row("compvhip_plan_acc_export", ASYNC),
    # ---- features on the plan (api_features.cpp)
    _row("compvhip_plan_houghsht_segments", ASYNC),
    _row("compvhip_plan_houghsht_fit", ASYNC),
    _row("compvhip_plan_components", ASYNC),
    _row("compvhip_plan_threshold", ASYNC),
    _row("compvhip_plan_threshold_adaptive", ASYNC, cases=("threshold_adaptive", "threshold_adaptive_in_place")),
    _row("compvhip_plan_morph", ASYNC, host=("strel",)),
    _row("compvhip_plan_morph_ex", ASYNC, host=("strel",)),
    _row("compvhip_plan_fast", ASYNC),
    _row("compvhip_plan_orb_keypoints", ASYNC, cases=("orb_keypoints", "orb_keypoints_growth")),
    _row("compvhip_plan_orb_describe", ASYNC),
    _row("compvhip_plan_scale", ASYNC),
    _row("compvhip_plan_remap", ASYNC, host=("roi",)),
    _row("compvhip_plan_warp_inverse", ASYNC, host=("M",), cases=("warp_inverse", "warp_inverse_growth")),
    _row("compvhip_plan_hog", ASYNC, host=("opts",), cases=("hog", "hog_growth")),
    _row("compvhip_plan_integral", ASYNC),
    _row("compvhip_plan_histogram", ASYNC),
    _row("compvhip_plan_equalize", ASYNC),
    _row("compvhip_plan_projections", ASYNC),
    # ---- the ORB pyramid, the matcher, the homography, the colour conversion
    _row("compvhip_orbpyr_detect", ASYNC),
    _row("compvhip_orbpyr_describe", ASYNC),
    _row("compvhip_matcher_knn", ASYNC),
    _row("compvhip_matcher_good", ASYNC, host=("opts",)),
    _row("compvhip_homography_points", ASYNC),
    _row("compvhip_homography_find", ASYNC, host=("opts",)),
    _row("compvhip_homography_project", ASYNC),
    _row("compvhip_homography_scores", WAITS),
    _row("compvhip_convert_frames", ASYNC, host=("in", "out")),
)

BY_EXPORT = {r.export: r for r in ROWS}
assert len(BY_EXPORT) == len(ROWS), "an export has two rows"
CASE_ROW = {c: r for r in ROWS for c in r.cases}
assert len(CASE_ROW) == sum(len(r.cases) for r in ROWS), "a case belongs to two rows"
