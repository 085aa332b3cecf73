"""CPU tests of the homography boundary: the library exports the compvhip_homography_* calls, the Python binding lists and binds them with the header's
argument counts, the record dtype is the C struct's, compvhip_homography_quads (host arithmetic) equals the model exactly, and the refusals that
precede any HIP call answer without a GPU and leave the outputs untouched.  (Without a device no context can be made, so the parameter refusals that
need a handle are exercised by tests/test_gpu_homography.py.)"""
import ctypes as C
import inspect
import os
import re

import numpy as np

import homography_model as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"compvhip_homography_create": 5, "compvhip_homography_destroy": 1, "compvhip_homography_points": 10, "compvhip_homography_find": 9,
           "compvhip_homography_project": 7, "compvhip_homography_quads": 5, "compvhip_homography_find_f64": 8, "compvhip_homography_scores": 6,
           "compvhip_homography_set_timing": 2, "compvhip_homography_get_timing": 4}


def test_symbols_are_exported_and_bound():
    from compv_amd import capi
    lib = capi.load()
    txt = open(os.path.join(ROOT, "include", "compv_hip.h")).read()
    for s, nargs in SYMBOLS.items():
        assert s in capi.EXPORTS and hasattr(lib, s), s
        assert len(getattr(lib, s).argtypes) == nargs, s
        decl = re.search(r"COMPVHIP_API \w+ %s\((.*?)\);" % s, txt, re.S).group(1)
        assert decl.count(",") + 1 == nargs, s          # the binding's argument count is the header's


def test_python_signatures():
    from compv_amd import capi
    assert list(inspect.signature(capi.Homography.__init__).parameters) == ["self", "ctx", "pairs", "point_cap", "max_tries"]
    assert list(inspect.signature(capi.Homography.find).parameters) == ["self", "d_src", "d_dst", "d_counts", "d_results", "d_mask", "tries", "threshold", "seed", "d_quads",
                                                                         "stream"]
    assert list(inspect.signature(capi.Homography.points).parameters) == ["self", "d_good", "good_cap", "d_good_counts", "d_query", "query_cap", "d_train", "train_cap",
                                                                           "train_shared", "stream"]
    assert list(inspect.signature(capi.Homography.project).parameters) == ["self", "d_results", "d_points", "n", "shared", "d_out", "stream"]
    assert list(inspect.signature(capi.Context.homography_find).parameters) == ["self", "src", "dst", "tries", "threshold", "seed", "quads", "want_mask"]
    assert inspect.signature(capi.Context.homography_find).parameters["threshold"].default == 30.0          # COMPV_HOMOGRAPHY_OUTLIER_THRESHOLD
    for name in ("scores", "set_timing", "get_timing", "close"):
        assert hasattr(capi.Homography, name)


def test_record_dtype_is_the_c_struct():
    from compv_amd import capi
    assert capi.HOMOGRAPHY_RESULT_DTYPE == hm.RESULT_DTYPE and capi.HOMOGRAPHY_RESULT_DTYPE.itemsize == 96
    txt = open(os.path.join(ROOT, "include", "compv_hip.h")).read()
    body = re.search(r"typedef struct compvhip_homography_result \{(.*?)\} compvhip_homography_result;", txt, re.S).group(1)
    assert re.findall(r"\b(\w+)(?:\[9\])?\s*[,;]", body) == ["H", "variance", "inliers", "bestTry", "status", "rotations"]
    assert [hm.RESULT_DTYPE.fields[n][1] for n in hm.RESULT_DTYPE.names] == [0, 72, 80, 84, 88, 92]
    assert C.sizeof(capi.HomographyOpts) == 16 and capi.HomographyOpts.seed.offset == 4 and capi.HomographyOpts.threshold.offset == 8
    o = capi.HomographyOpts()
    assert (o.tries, o.seed, o.threshold) == (2000, 0, 30.0)


def test_quads_on_the_host_equal_the_model():
    """compvhip_homography_quads needs no GPU: every k from 4 (every try ends in the fill-up or a permutation) through the wave and block sizes, seeds
    and pairs that wrap, 2000 tries; each quad holds four distinct indices below k"""
    from compv_amd import capi
    for seed, pair, k, tries in [(0, 0, 4, 300), (1, 0, 5, 300), (0xffffffff, 65534, 9, 200), (12345, 7, 63, 200), (77, 1, 64, 65), (77, 2, 65, 65), (5, 3, 129, 200),
                                 (0x80000000, 31, 2000, 2000), (9, 0, 1 << 22, 64)]:
        q = capi.homography_quads(seed, pair, k, tries)
        assert q.dtype == np.int32 and q.shape == (tries, 4)
        assert q.tolist() == hm.quads(seed, pair, k, tries).tolist(), (seed, pair, k)
        assert (q >= 0).all() and (q < k).all() and all(len(set(r)) == 4 for r in q.tolist())
    assert capi.homography_quads(3, 0, 50, 100).tolist() != capi.homography_quads(3, 1, 50, 100).tolist()          # the pair enters the hash
    assert capi.homography_quads(3, 0, 50, 100).tolist() != capi.homography_quads(4, 0, 50, 100).tolist()


def test_refusals_before_any_hip_call():
    from compv_amd import capi
    lib = capi.load()
    q = np.full((4, 4), 77, np.int32)
    assert lib.compvhip_homography_quads(0, 0, 3, 4, q.ctypes.data) == capi.E_INVALID_PARAMETER and (q == 77).all()          # k < 4
    assert lib.compvhip_homography_quads(0, 0, 9, 4, None) == capi.E_INVALID_PARAMETER
    h = C.c_void_p(1234)
    assert lib.compvhip_homography_create(None, 1, 8, 8, C.byref(h)) == capi.E_INVALID_PARAMETER and h.value == 1234
    pts = np.zeros((8, 2))
    res = np.zeros(1, capi.HOMOGRAPHY_RESULT_DTYPE)
    res["status"] = 55
    o = capi.HomographyOpts(8, 0, 30.0)
    assert lib.compvhip_homography_find_f64(None, pts.ctypes.data, pts.ctypes.data, 8, C.byref(o), None, res.ctypes.data, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_homography_find(None, pts.ctypes.data, pts.ctypes.data, None, C.byref(o), None, res.ctypes.data, None, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_homography_points(None, None, 0, None, pts.ctypes.data, 8, pts.ctypes.data, 8, 0, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_homography_project(None, res.ctypes.data, pts.ctypes.data, 8, 0, pts.ctypes.data, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_homography_scores(None, 8, None, None, None, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_homography_set_timing(None, 1) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_homography_get_timing(None, None, None, 0) == capi.E_INVALID_PARAMETER
    assert res["status"][0] == 55 and not pts.any()
    lib.compvhip_homography_destroy(None)          # a no-op
