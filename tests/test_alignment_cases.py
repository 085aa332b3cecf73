"""CPU check of tests/alignment_cases.py against include/compv_hip.h: every d_* pointer parameter of a plan, pyramid, matcher or homography export has
exactly one row, no row names a parameter that is gone, and a row's class fits the parameter's type -- so a later call cannot arrive without an
alignment contract."""
import os
import re

import alignment_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_pointers(txt):
    """{(export, parameter): type} of the d_* pointer parameters of the four families"""
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    out = {}
    for name, params in re.findall(r"COMPVHIP_API\s+[\w\s\*]+?\b(compvhip_\w+)\s*\(([^)]*)\)\s*;", txt):
        if not name.startswith(ac.FAMILIES):
            continue
        for prm in params.split(","):
            m = re.match(r"\s*(.*?)(\bd_\w+)\s*$", prm.strip())
            if m and "*" in m.group(1):
                out[(name, m.group(2))] = " ".join(m.group(1).split())
    return out


def header_text():
    return open(os.path.join(ROOT, "include", "compv_hip.h")).read()


def problems(rows, pointers):
    keys = {(r.export, r.param) for r in rows}
    bad = ["no row: %s(%s)" % k for k in sorted(set(pointers) - keys)]
    bad += ["row without a parameter: %s(%s)" % k for k in sorted(keys - set(pointers))]
    return bad


def test_the_parser_finds_the_pointers():
    ptrs = header_pointers(header_text())
    assert ptrs[("compvhip_plan_canny", "d_edges")] == "uint8_t*"
    assert ptrs[("compvhip_plan_houghsht_fit", "d_fits")] == "compvhip_line_fit*"
    assert ptrs[("compvhip_plan_acc", "d_acc")] == "const uint16_t**"
    assert ptrs[("compvhip_plan_remap", "d_out")] == "void*"
    assert ("compvhip_plan_houghkht", "lines") not in ptrs and ("compvhip_plan_create", "plan") not in ptrs
    assert len({e for e, _ in ptrs}) >= 40 and len(ptrs) >= 120


def test_every_device_pointer_has_a_row_and_every_row_a_pointer():
    assert problems(ac.ROWS, header_pointers(header_text())) == []


def test_the_check_notices_a_missing_and_a_stale_row():
    ptrs = header_pointers(header_text())
    for victim in (("compvhip_plan_canny", "d_in"), ("compvhip_plan_acc_export", "d_out"), ("compvhip_homography_find", "d_mask")):
        rows = [r for r in ac.ROWS if (r.export, r.param) != victim]
        assert problems(rows, ptrs) == ["no row: %s(%s)" % victim]
    stale = ac.ROWS + [ac.Row("compvhip_plan_canny", "d_gone", ac.SERVED, 1, 0, ac.HERE)]
    assert problems(stale, ptrs) == ["row without a parameter: compvhip_plan_canny(d_gone)"]
    later = dict(ptrs)
    later[("compvhip_plan_new_call", "d_thing")] = "float*"
    assert problems(ac.ROWS, later) == ["no row: compvhip_plan_new_call(d_thing)"]


NATURAL = {"int32_t": 4, "uint32_t": 4, "float": 4, "double": 8, "compvhip_line": 4, "compvhip_segment": 4, "compvhip_component": 4, "compvhip_corner": 4,
           "compvhip_keypoint": 4, "compvhip_line_fit": 8, "compvhip_homography_result": 8, "compvhip_match": 4}


def test_classes_fit_the_types():
    """SERVED only for uint8 (or the void* destinations that may be uint8); a typed array REFUSED at its natural alignment at least; two stars = HOST"""
    for (export, param), typ in header_pointers(header_text()).items():
        r = ac.BY_KEY[(export, param)]
        base = typ.replace("const", "").replace("*", "").strip()
        what = "%s(%s): %s" % (export, param, typ)
        if typ.count("*") == 2:
            assert r.cls == ac.HOST, what
        elif r.cls == ac.SERVED:
            assert base == "uint8_t" or (base == "void" and r.n_f32 == 4), what
        else:
            assert r.cls == ac.REFUSED and r.n in (4, 8, 16), what
            assert base == "uint8_t" or r.n >= NATURAL[base], what


def test_moves():
    assert ac.moves(4) == (1,) and ac.moves(8) == (1, 4) and ac.moves(16) == (1, 8)
    assert all(r.n in (4, 8, 16) for r in ac.refused_rows())
