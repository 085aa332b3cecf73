"""The alignment contract of every device pointer of the plan, pyramid, matcher and homography calls (include/compv_hip.h, "Alignment of device
pointers"): one row per (export, d_* pointer parameter).  Importable without a GPU; tests/test_alignment_cases.py holds it against the header,
tests/test_gpu_pointer_alignment.py against the library.

Classes
  SERVED   a uint8 frame, edge map or plane that may start at any byte: same bits as at an aligned pointer, nothing else written.  n = 1.
  REFUSED  below n bytes (4, 8 or 16) the call returns E_INVALID_PARAMETER before it allocates, enqueues or writes anything.
  HOST     a HOST pointer that receives a device address (two stars in the header): no device access, nothing to align.  n = 0.

`n_f32`: a void* destination that is uint8 (SERVED) or, with INTERP_BILINEAR_FLOAT32, float32 (REFUSED below n_f32).
`test`: where the row's refusal is launched: "here" = tests/test_gpu_pointer_alignment.py::test_refused_pointer, which is every row today (the
refusal tests the newer calls came with move only some of their pointers alone; docs/dispatch_coverage.md, "Pointer alignment", names them); a later
row may name another test id instead, and test_every_refused_row_has_a_call_here then has to learn about it."""
from collections import namedtuple

SERVED, REFUSED, HOST = "served", "refused", "host"
Row = namedtuple("Row", "export param cls n n_f32 test")
FAMILIES = ("compvhip_plan_", "compvhip_orbpyr_", "compvhip_matcher_", "compvhip_homography_")
HERE = "here"


def _rows(export, served=(), host=(), test=HERE, f32=(), **refused):
    """refused: r4 / r8 / r16 = names refused below 4 / 8 / 16 bytes"""
    out = [Row(export, p, SERVED, 1, 4 if p in f32 else 0, test) for p in served]
    out += [Row(export, p, HOST, 0, 0, None) for p in host]
    for key, names in refused.items():
        out += [Row(export, p, REFUSED, int(key[1:]), 0, test) for p in names]
    return out


ROWS = (
    # ---- the Canny / SHT plan (api.cpp, api_kht.cpp)
    _rows("compvhip_plan_canny", served=("d_in", "d_edges"))
    + _rows("compvhip_plan_grayscale", served=("d_in", "d_gray"))
    + _rows("compvhip_plan_otsu", served=("d_gray",), r4=("d_thresholds",))
    + _rows("compvhip_plan_convlt1_fixedpoint", served=("d_in", "d_out"))
    + _rows("compvhip_plan_to_cartesian", r4=("d_lines", "d_counts", "d_cart"))
    + _rows("compvhip_plan_edge_dete", served=("d_in", "d_out"))
    + _rows("compvhip_plan_houghsht", served=("d_edges",), r4=("d_lines", "d_counts"))
    + _rows("compvhip_plan_pipeline", served=("d_in", "d_edges"), r4=("d_lines", "d_counts"))
    + _rows("compvhip_plan_pipeline_async", served=("d_in", "d_edges"), r4=("d_lines", "d_counts"))
    + _rows("compvhip_plan_pipeline_ex", served=("d_in", "d_edges"), r4=("d_lines", "d_counts"))
    + _rows("compvhip_plan_houghkht", served=("d_edges",))
    + _rows("compvhip_plan_houghkht_ex", served=("d_edges",))
    + _rows("compvhip_plan_acc", host=("d_acc",))
    + _rows("compvhip_plan_acc_export", r4=("d_out",))
    + _rows("compvhip_plan_edge_counts", host=("d_edge_counts",))
    # ---- features on the plan (api_features.cpp)
    + _rows("compvhip_plan_houghsht_segments", served=("d_edges",), r4=("d_lines", "d_counts", "d_segs", "d_segCounts"))
    + _rows("compvhip_plan_houghsht_fit", served=("d_edges",), r4=("d_lines", "d_counts", "d_segs", "d_segCounts", "d_fitCounts", "d_refined"), r8=("d_fits",))
    + _rows("compvhip_plan_components", served=("d_edges",), r4=("d_labels", "d_comps", "d_compCounts"))
    + _rows("compvhip_plan_threshold", served=("d_in", "d_out"), r4=("d_levels",))
    + _rows("compvhip_plan_threshold_adaptive", served=("d_in", "d_out"))
    + _rows("compvhip_plan_morph", served=("d_in", "d_out"))
    + _rows("compvhip_plan_morph_ex", served=("d_in", "d_out"))
    + _rows("compvhip_plan_fast", r8=("d_gray", "d_scores"), r4=("d_corners", "d_counts"))
    + _rows("compvhip_plan_orb_keypoints", r4=("d_gray", "d_corners", "d_cornerCounts", "d_keypoints", "d_keyCounts", "d_moments"))
    + _rows("compvhip_plan_orb_describe", r4=("d_gray", "d_keypoints", "d_keyCounts", "d_desc"))
    + _rows("compvhip_plan_scale", served=("d_in", "d_out"))
    + _rows("compvhip_plan_remap", served=("d_in", "d_out"), f32=("d_out",), r4=("d_mapX", "d_mapY"))
    + _rows("compvhip_plan_warp_inverse", served=("d_in", "d_out"), f32=("d_out",))
    + _rows("compvhip_plan_hog", served=("d_gray",), r4=("d_cells", "d_desc"))
    + _rows("compvhip_plan_integral", served=("d_gray",), r8=("d_sum", "d_sumsq"))
    + _rows("compvhip_plan_histogram", served=("d_gray",), r4=("d_hist",))
    + _rows("compvhip_plan_equalize", served=("d_gray", "d_out", "d_lut"), r4=("d_hist",))
    + _rows("compvhip_plan_projections", served=("d_gray",), r4=("d_projX", "d_projY"))
    # ---- the ORB pyramid, the matcher, the homography
    + _rows("compvhip_orbpyr_plane", host=("d_plane",))
    + _rows("compvhip_orbpyr_detect", r8=("d_gray",), r4=("d_keypoints", "d_keyCounts", "d_levelCounts", "d_levelCorners"))
    + _rows("compvhip_orbpyr_describe", r8=("d_gray",), r4=("d_keypoints", "d_keyCounts", "d_desc"))
    + _rows("compvhip_matcher_knn", r4=("d_query", "d_queryCounts", "d_train", "d_trainCounts"), r16=("d_matches",))
    + _rows("compvhip_matcher_good", r4=("d_query", "d_queryCounts", "d_train", "d_trainCounts", "d_goodCounts"), r16=("d_matches", "d_good"))
    + _rows("compvhip_homography_points", r4=("d_goodCounts", "d_query", "d_train"), r16=("d_good",))
    + _rows("compvhip_homography_find", served=("d_mask",), r4=("d_counts",), r8=("d_results",), r16=("d_src", "d_dst", "d_quads"))
    + _rows("compvhip_homography_project", r8=("d_results",), r16=("d_points", "d_out"))
)

BY_KEY = {(r.export, r.param): r for r in ROWS}
assert len(BY_KEY) == len(ROWS), "a pointer has two rows"


def refused_rows():
    return [r for r in ROWS if r.cls == REFUSED] + [r._replace(cls=REFUSED, n=r.n_f32) for r in ROWS if r.n_f32]


def moves(n):
    """byte offsets that break an alignment of n and nothing coarser: 1 always, n / 2 for 8 and 16"""
    return (1,) if n == 4 else (1, n // 2)
