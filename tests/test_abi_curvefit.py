"""CPU tests of the curve-fit boundary: the library exports the compvhip_curvefit_* calls, the Python binding lists and binds them with the header's
argument counts, the record, descriptor and option layouts are the C structs', compvhip_curvefit_samples (host arithmetic) equals the model exactly,
and the refusals that precede any HIP call answer without a GPU and leave the outputs untouched.  (Without a device no context can be made, so the
parameter refusals that need a handle are exercised by tests/test_gpu_curvefit.py.)"""
import ctypes as C
import inspect
import os
import re

import numpy as np

import curvefit_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"compvhip_curvefit_create": 3, "compvhip_curvefit_destroy": 1, "compvhip_curvefit_points_from_labels": 9, "compvhip_curvefit_find": 7,
           "compvhip_curvefit_distances": 6, "compvhip_curvefit_scores": 4, "compvhip_curvefit_gathered": 3, "compvhip_curvefit_set_timing": 2,
           "compvhip_curvefit_get_timing": 4, "compvhip_curvefit_samples": 6, "compvhip_curvefit_find_f64": 7}


def header():
    return open(os.path.join(ROOT, "include", "compv_hip.h")).read()


def test_symbols_are_exported_and_bound():
    from compv_amd import capi
    lib = capi.load()
    txt = header()
    declared = set(re.findall(r"COMPVHIP_API \w+ (compvhip_curvefit_\w+)\(", txt))
    assert declared == set(SYMBOLS)
    for s, nargs in SYMBOLS.items():
        assert s in capi.EXPORTS and hasattr(lib, s), s
        assert len(getattr(lib, s).argtypes) == nargs, s
        decl = re.search(r"COMPVHIP_API \w+ %s\((.*?)\);" % s, txt, re.S).group(1)
        assert decl.count(",") + 1 == nargs, s          # the binding's argument count is the header's


def test_no_call_of_the_family_takes_a_stream_parameter():
    """the stream travels in the descriptor (the header says why); a `void* stream` parameter would need a row in tests/stream_cases.py"""
    for s in SYMBOLS:
        decl = re.search(r"COMPVHIP_API \w+ %s\((.*?)\);" % s, header(), re.S).group(1)
        assert "stream" not in decl, s
    body = re.search(r"typedef struct compvhip_curvefit_desc \{(.*?)\} compvhip_curvefit_desc;", header(), re.S).group(1)
    assert re.search(r"void\*\s*stream;", body)


def test_python_signatures():
    from compv_amd import capi
    assert list(inspect.signature(capi.Curvefit.__init__).parameters) == ["self", "ctx", "sets", "point_cap", "max_tries", "stream"]
    assert list(inspect.signature(capi.Curvefit.find).parameters) == ["self", "d_points", "d_counts", "d_results", "d_mask", "model", "tries", "threshold", "seed", "d_samples"]
    assert list(inspect.signature(capi.Curvefit.points_from_labels).parameters) == ["self", "d_labels", "W", "H", "label_stride", "d_comps", "comp_cap", "d_comp_counts",
                                                                                     "frames"]
    assert list(inspect.signature(capi.Curvefit.distances).parameters) == ["self", "d_points", "d_counts", "model", "d_params", "d_out"]
    assert list(inspect.signature(capi.Context.fit_line).parameters) == ["self", "points", "threshold", "tries", "seed", "samples", "want_mask"]
    assert list(inspect.signature(capi.Context.fit_parabola).parameters) == ["self", "points", "threshold", "tries", "seed", "sideways", "samples", "want_mask"]
    for name in ("scores", "gathered", "set_timing", "get_timing", "close"):
        assert hasattr(capi.Curvefit, name)
    assert (capi.CURVEFIT_LINE, capi.CURVEFIT_PARABOLA, capi.CURVEFIT_PARABOLA_SIDEWAYS) == cm.MODELS
    enum = re.search(r"enum \{\s*COMPVHIP_CURVEFIT_LINE = 0,\s*COMPVHIP_CURVEFIT_PARABOLA = 1,[^\n]*\n\s*COMPVHIP_CURVEFIT_PARABOLA_SIDEWAYS = 2", header())
    assert enum


def fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip().split(" ", 1)[-1].replace("*", " "))]


def test_layouts_are_the_c_structs():
    from compv_amd import capi
    assert capi.CURVEFIT_RESULT_DTYPE == cm.RESULT_DTYPE and cm.RESULT_DTYPE.itemsize == 40
    assert fields("compvhip_curvefit_result") == list(cm.RESULT_DTYPE.names) == ["A", "B", "C", "inliers", "bestTry", "status", "k"]
    assert [cm.RESULT_DTYPE.fields[n][1] for n in cm.RESULT_DTYPE.names] == [0, 8, 16, 24, 28, 32, 36]
    assert fields("compvhip_curvefit_desc") == [f[0] for f in capi.CurvefitDesc._fields_] == ["size", "sets", "pointCap", "maxTries", "stream"]
    assert C.sizeof(capi.CurvefitDesc) == 24 and capi.CurvefitDesc.stream.offset == 16
    assert fields("compvhip_curvefit_opts") == [f[0] for f in capi.CurvefitOpts._fields_] == ["size", "model", "tries", "seed", "threshold"]
    assert C.sizeof(capi.CurvefitOpts) == 24 and capi.CurvefitOpts.threshold.offset == 16
    o = capi.CurvefitOpts()
    assert (o.size, o.model, o.tries, o.seed, o.threshold) == (24, 0, 2000, 0, 1.0)
    d = capi.CurvefitDesc(7, 100, 50)
    assert (d.size, d.sets, d.pointCap, d.maxTries, d.stream) == (24, 7, 100, 50, None)
    assert cm.COMP_DTYPE == capi.COMP_DTYPE


def test_samples_on_the_host_equal_the_model():
    """compvhip_curvefit_samples needs no GPU: every k from m + 1 (every try ends in the fill-up or a permutation) through the wave and block sizes, seeds
    and sets that wrap; each sample holds m distinct indices below k"""
    from compv_amd import capi
    for model in cm.MODELS:
        m = cm.model_points(model)
        for seed, s, k, tries in [(0, 0, m + 1, 300), (1, 0, 5, 300), (0xffffffff, 65534, 9, 200), (12345, 7, 63, 200), (77, 1, 64, 65), (77, 2, 65, 65), (5, 3, 257, 200),
                                  (0x80000000, 31, 2000, 2000), (9, 0, 1 << 22, 64)]:
            q = capi.curvefit_samples(model, seed, s, k, tries)
            assert q.dtype == np.int32 and q.shape == (tries, m)
            assert q.tolist() == cm.samples(model, seed, s, k, tries).tolist(), (model, seed, s, k)
            assert (q >= 0).all() and (q < k).all() and all(len(set(r)) == m for r in q.tolist())
        assert capi.curvefit_samples(model, 3, 0, 50, 100).tolist() != capi.curvefit_samples(model, 3, 1, 50, 100).tolist()          # the set enters the hash
        assert capi.curvefit_samples(model, 3, 0, 50, 100).tolist() != capi.curvefit_samples(model, 4, 0, 50, 100).tolist()


def test_refusals_before_any_hip_call():
    from compv_amd import capi
    lib = capi.load()
    q = np.full((4, 3), 77, np.int32)
    assert lib.compvhip_curvefit_samples(cm.LINE, 0, 0, 2, 4, q.ctypes.data) == capi.E_INVALID_PARAMETER          # k == m: no generator runs on such a set
    assert lib.compvhip_curvefit_samples(cm.PARABOLA, 0, 0, 3, 4, q.ctypes.data) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_curvefit_samples(3, 0, 0, 9, 4, q.ctypes.data) == capi.E_INVALID_PARAMETER                # an unknown model
    assert lib.compvhip_curvefit_samples(-1, 0, 0, 9, 4, q.ctypes.data) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_curvefit_samples(cm.LINE, 0, 0, 9, 4, None) == capi.E_INVALID_PARAMETER and (q == 77).all()
    h = C.c_void_p(1234)
    d = capi.CurvefitDesc(1, 8, 8)
    assert lib.compvhip_curvefit_create(None, C.byref(d), C.byref(h)) == capi.E_INVALID_PARAMETER and h.value == 1234
    pts = np.zeros((8, 2))
    res = np.zeros(1, capi.CURVEFIT_RESULT_DTYPE)
    res["status"] = 55
    o = capi.CurvefitOpts(cm.LINE, 8, 0, 1.0)
    assert lib.compvhip_curvefit_find_f64(None, pts.ctypes.data, 8, C.byref(o), None, res.ctypes.data, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_curvefit_find(None, pts.ctypes.data, None, C.byref(o), None, res.ctypes.data, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_curvefit_distances(None, pts.ctypes.data, None, cm.LINE, pts.ctypes.data, pts.ctypes.data) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_curvefit_points_from_labels(None, pts.ctypes.data, 4, 4, 4, pts.ctypes.data, 1, pts.ctypes.data, 1) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_curvefit_scores(None, 8, None, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_curvefit_gathered(None, None, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_curvefit_set_timing(None, 1) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_curvefit_get_timing(None, None, None, 0) == capi.E_INVALID_PARAMETER
    assert res["status"][0] == 55 and not pts.any()
    lib.compvhip_curvefit_destroy(None)          # a no-op
