"""CPU check of tests/stream_cases.py against include/compv_hip.h and against the case list of tests/stream_order_rig.py: every export with a `void* stream`
parameter (and the two batched KHT calls) has exactly one row, no row names an export that is gone, the class word beside the declaration in the header is the
row's, the host arrays a row names are parameters of the export, and every case id exists -- so a later call cannot arrive without a stream-order contract and
a GPU run behind pending work."""
import os
import re

import stream_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_STREAM = ("compvhip_plan_houghkht", "compvhip_plan_houghkht_ex")          # DRAINS: the two calls of the table that take no stream


def header_text():
    return open(os.path.join(ROOT, "include", "compv_hip.h")).read()


def header_exports(txt):
    """{export: (parameter names, class word beside it or None)} of the exports with a `void* stream` parameter and of NO_STREAM.  The class word is the last
    "Stream order: WORD" between the end of the declaration before and the export's own declaration."""
    out = {}
    last = 0
    for m in re.finditer(r"COMPVHIP_API\s+[\w\s\*]+?\b(compvhip_\w+)\s*\(([^)]*)\)\s*;", txt):
        name, params = m.group(1), [p.strip() for p in m.group(2).split(",")]
        between = txt[last:m.start()]
        last = m.end()
        if not any(re.fullmatch(r"void\s*\*\s*stream", p) for p in params) and name not in NO_STREAM:
            continue
        words = re.findall(r"Stream order:\s*(\w+)", between)
        out[name] = ([re.search(r"(\w+)\s*(\[\d*\])?$", p).group(1) for p in params], words[-1] if words else None)
    return out


def case_ids():
    import stream_order_rig as gso          # importable without torch or a device: everything heavy is imported inside its functions
    return set(gso.CASES)


def problems(rows, exports, cases):
    by = {r.export: r for r in rows}
    bad = ["no row: %s" % e for e in sorted(set(exports) - set(by))]
    bad += ["row without an export: %s" % e for e in sorted(set(by) - set(exports))]
    for e in sorted(set(by) & set(exports)):
        params, word = exports[e]
        if word != by[e].cls:
            bad.append("%s: the header says %s, the row %s" % (e, word, by[e].cls))
        bad += ["%s: no parameter %s" % (e, h) for h in by[e].host if h not in params]
        bad += ["%s: no GPU case %s" % (e, c) for c in by[e].cases if c not in cases]
    listed = {c for r in rows for c in r.cases}
    bad += ["GPU case without a row: %s" % c for c in sorted(cases - listed)]
    return bad


def test_the_parser_finds_the_exports():
    ex = header_exports(header_text())
    assert ex["compvhip_plan_canny"][1] == sc.WAITS and ex["compvhip_plan_edge_dete"][1] == sc.ASYNC and ex["compvhip_plan_houghkht_ex"][1] == sc.DRAINS
    assert "strel" in ex["compvhip_plan_morph_ex"][0] and "M" in ex["compvhip_plan_warp_inverse"][0] and "opts" in ex["compvhip_homography_find"][0]
    assert "compvhip_plan_wait" not in ex and "compvhip_canny_u8" not in ex and "compvhip_plan_houghkht_stage_ms" not in ex
    assert len(ex) >= 40 and all(w in sc.CLASSES for _, w in ex.values())


def test_every_export_has_a_row_a_class_and_a_case():
    assert problems(sc.ROWS, header_exports(header_text()), case_ids()) == []


def test_rows_are_well_formed():
    for r in sc.ROWS:
        assert r.cls in sc.CLASSES and r.cases, r
        assert (r.cls == sc.DRAINS) == (r.export in NO_STREAM), r


def test_the_check_notices_a_missing_row_a_new_export_another_class_and_a_missing_case():
    txt = header_text()
    ex, cases = header_exports(txt), case_ids()
    for victim in ("compvhip_plan_canny", "compvhip_homography_scores", "compvhip_convert_frames", "compvhip_plan_houghkht"):
        rows = [r for r in sc.ROWS if r.export != victim]
        got = problems(rows, ex, cases)
        assert got[0] == "no row: %s" % victim and all(g.startswith("GPU case without a row") for g in got[1:]), got
    stale = sc.ROWS + (sc.Row("compvhip_plan_gone", sc.ASYNC, (), ("edge_dete",)),)
    assert problems(stale, ex, cases) == ["row without an export: compvhip_plan_gone"]
    # an export with a stream parameter added to a copy of the header: without a class word, then with one
    later = txt.replace("COMPVHIP_API int compvhip_plan_set_timing(", "COMPVHIP_API int compvhip_plan_new_call(compvhip_plan* plan, const uint8_t* d_in, void* stream);\n"
                        "COMPVHIP_API int compvhip_plan_set_timing(")
    assert later != txt and problems(sc.ROWS, header_exports(later), cases) == ["no row: compvhip_plan_new_call"]
    assert header_exports(later)["compvhip_plan_new_call"] == (["plan", "d_in", "stream"], None)
    # a class word in the header that differs from the row
    other = txt.replace("Stream order: ASYNC: compvhip_plan_wait", "Stream order: WAITS: compvhip_plan_wait")
    assert other != txt and problems(sc.ROWS, header_exports(other), cases) == ["compvhip_plan_pipeline_async: the header says WAITS, the row ASYNC"]
    # a row whose case does not exist, a case nobody lists, a host array that is no parameter
    assert problems(sc.ROWS, ex, cases - {"otsu"}) == ["compvhip_plan_otsu: no GPU case otsu"]
    assert problems(sc.ROWS, ex, cases | {"brand_new"}) == ["GPU case without a row: brand_new"]
    rows = tuple(r._replace(host=("kernel9",)) if r.export == "compvhip_plan_morph" else r for r in sc.ROWS)
    assert problems(rows, ex, cases) == ["compvhip_plan_morph: no parameter kernel9"]
