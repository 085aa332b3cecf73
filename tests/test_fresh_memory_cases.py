"""The table of cold cases of tests/test_gpu_fresh_memory.py (tests/fresh_memory_cases.py), checked without a GPU: every opaque handle type the header
declares is created by at least one cold case, and every host entry point of the header belongs to a family that has one."""
import os
import re

import fresh_memory_cases as fc
import stream_order_rig as rig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "compv_hip.h")) as f:
        return f.read()


def test_every_handle_type_of_the_header_has_a_cold_case():
    cases = fc.handle_cases(rig.CASES)
    assert fc.handle_types(header()) == sorted(["ctx", "plan", "matcher", "orbpyr", "homography", "curvefit", "svm", "undistort"])
    assert fc.handles_without_a_case(header(), cases) == []
    assert all(cases[t] for t in cases), cases
    # every id names something that runs: a host call, a family, a case of the rig
    for ids in cases.values():
        for i in ids:
            kind, name = i.split(":")
            assert name in {"host": fc.HOST_CALLS, "family": fc.FAMILIES, "rig": rig.CASES}[kind], i


def test_a_handle_type_without_a_cold_case_is_found():
    """the check on a copy of the header's text with one more handle type, and on a table that lost one"""
    more = header() + "\ntypedef struct compvhip_tracker compvhip_tracker;   /* a handle nobody tests yet */\n"
    cases = fc.handle_cases(rig.CASES)
    assert fc.handles_without_a_case(more, cases) == ["tracker"]
    assert fc.handles_without_a_case(header(), {k: v for k, v in cases.items() if k != "svm"}) == ["svm"]
    assert fc.handles_without_a_case(header(), dict(cases, matcher=[])) == ["matcher"]
    assert fc.handle_types("typedef struct compvhip_a compvhip_b;") == []          # not an opaque handle's declaration


def test_every_host_entry_point_belongs_to_a_family_with_a_cold_case():
    """the exports that take host pointers end in _u8 or _f64 (svm's predict_host runs in its family): each is reached by a HOST_CALLS entry"""
    declared = set(re.findall(r"COMPVHIP_API\s+[\w\s\*]+?\b(compvhip_\w+?)\s*\(", header()))
    host = sorted(s for s in declared if s.endswith(("_u8", "_f64")) and not s.startswith(("compvhip_undistort_coeffs", "compvhip_undistort_map_", "compvhip_svm_exp")))
    reached = {
        "canny": ["compvhip_canny_u8"], "edge_dete": ["compvhip_edge_dete_u8"], "grayscale": ["compvhip_grayscale_u8"], "otsu": ["compvhip_otsu_u8"],
        "convlt_fixedpoint": ["compvhip_convlt1_fixedpoint_u8"], "houghsht": ["compvhip_houghsht_u8"], "houghkht": ["compvhip_houghkht_u8", "compvhip_houghkht_ex_u8"],
        "houghsht_segments": ["compvhip_houghsht_segments_u8"], "houghsht_fit": ["compvhip_houghsht_fit_u8"], "components": ["compvhip_components_u8"],
        "threshold": ["compvhip_threshold_u8"], "threshold_adaptive": ["compvhip_threshold_adaptive_u8"], "morph": ["compvhip_morph_u8"], "fast": ["compvhip_fast_u8"],
        "orb": ["compvhip_orb_u8"], "orb_pyramid": ["compvhip_orb_pyramid_u8"], "scale": ["compvhip_scale_u8"], "remap": ["compvhip_remap_u8"],
        "warp_inverse": ["compvhip_warp_inverse_u8"], "hog": ["compvhip_hog_u8"], "integral": ["compvhip_integral_u8"], "histogram": ["compvhip_histogram_u8"],
        "equalize": ["compvhip_equalize_u8"], "projections": ["compvhip_projections_u8"], "convert": ["compvhip_convert_u8"], "match_hamming": ["compvhip_match_hamming_u8"],
        "homography_find_f64": ["compvhip_homography_find_f64"], "curvefit_find_f64": ["compvhip_curvefit_find_f64"], "undistort_u8": ["compvhip_undistort_u8"],
    }
    assert sorted(reached) == sorted(fc.HOST_CALLS)
    covered = {s for v in reached.values() for s in v}
    # stage inspection of the KHT (kernels, link): the same group state as compvhip_houghkht_u8, which has its case
    assert [s for s in host if s not in covered] == ["compvhip_houghkht_kernels_u8", "compvhip_houghkht_link_u8"]


def test_the_sizes_make_the_second_call_reallocate():
    (w0, h0), (w1, h1) = fc.SIZES
    assert w1 > w0 and h1 > h0 and (w1 + 7) // 8 * 8 * h1 > 2 * ((w0 + 7) // 8 * 8 * h0)
    assert fc.FILLS == (0xFF, 0x01)
