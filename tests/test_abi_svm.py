"""CPU tests of the SVM boundary: the library exports the compvhip_svm_* calls, the Python binding lists and binds them with the header's argument counts,
the model, descriptor and shape layouts are the C structs', no call takes a stream parameter, compvhip_svm_exp_f64 and compvhip_svm_model_parse (host
arithmetic) equal the model and the fixture exactly, and the refusals that precede any HIP call answer without a GPU and leave the outputs untouched.
(Without a device no context can be made, so the parameter refusals that need a handle are exercised by tests/test_gpu_svm.py.)"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import svm_cases as sc
import svm_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"compvhip_svm_create": 4, "compvhip_svm_create_from_file": 4, "compvhip_svm_destroy": 1, "compvhip_svm_info": 2, "compvhip_svm_predict": 8,
           "compvhip_svm_predict_host": 7, "compvhip_svm_set_timing": 2, "compvhip_svm_get_timing": 4, "compvhip_svm_exp_f64": 3, "compvhip_svm_model_parse": 7}


def header():
    return open(os.path.join(ROOT, "include", "compv_hip.h")).read()


def test_symbols_are_exported_and_bound():
    from compv_amd import capi
    lib = capi.load()
    txt = header()
    declared = set(re.findall(r"COMPVHIP_API \w+ (compvhip_svm_\w+)\(", txt))
    assert declared == set(SYMBOLS)
    for s, nargs in SYMBOLS.items():
        assert s in capi.EXPORTS and hasattr(lib, s), s
        assert len(getattr(lib, s).argtypes) == nargs, s
        decl = re.search(r"COMPVHIP_API \w+ %s\((.*?)\);" % s, txt, re.S).group(1)
        assert decl.count(",") + 1 == nargs, s          # the binding's argument count is the header's


def test_no_call_of_the_family_takes_a_stream_parameter():
    """the stream travels in the descriptor, as the curve-fit handle's; a `void* stream` parameter would need a row in tests/stream_cases.py"""
    for s in SYMBOLS:
        decl = re.search(r"COMPVHIP_API \w+ %s\((.*?)\);" % s, header(), re.S).group(1)
        assert "stream" not in decl, s
        assert not s.startswith(("compvhip_plan_", "compvhip_matcher_", "compvhip_homography_", "compvhip_orbpyr_"))
    body = re.search(r"typedef struct compvhip_svm_desc \{(.*?)\} compvhip_svm_desc;", header(), re.S).group(1)
    assert re.search(r"void\*\s*stream;", body)


def test_python_signatures():
    from compv_amd import capi
    assert list(inspect.signature(capi.Svm.__init__).parameters) == ["self", "ctx", "model_or_path", "max_vectors", "stream"]
    assert list(inspect.signature(capi.Svm.predict).parameters) == ["self", "d_vectors", "vtype", "n", "stride", "d_labels", "d_dec", "d_kvalues"]
    assert list(inspect.signature(capi.Svm.predict_host).parameters) == ["self", "vectors", "want_dec"]
    for name in ("info", "set_timing", "get_timing", "close"):
        assert hasattr(capi.Svm, name)
    assert hasattr(capi.SvmModel, "from_file")
    assert (capi.SVM_KERNEL_LINEAR, capi.SVM_KERNEL_RBF) == (sm.LINEAR, sm.RBF) == (0, 2) and (capi.SVM_F32, capi.SVM_F64) == (0, 1)
    assert re.search(r"COMPVHIP_SVM_KERNEL_LINEAR = 0,[^\n]*\n\s*COMPVHIP_SVM_KERNEL_RBF = 2", header())
    assert re.search(r"COMPVHIP_SVM_F32 = 0,\s*COMPVHIP_SVM_F64 = 1", header())


def fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip().split(" ", 1)[-1].replace("*", " ").replace("const double", "").replace("const int32_t", ""))]


def test_layouts_are_the_c_structs():
    from compv_amd import capi
    assert fields("compvhip_svm_model") == [f[0] for f in capi.SvmModelStruct._fields_] == ["size", "kernel", "nrClass", "totalSV", "dim", "reserved", "gamma", "sv", "svCoef",
                                                                                         "rho", "nSV", "label"]
    assert C.sizeof(capi.SvmModelStruct) == 72 and capi.SvmModelStruct.gamma.offset == 24 and capi.SvmModelStruct.sv.offset == 32 and capi.SvmModelStruct.label.offset == 64
    assert fields("compvhip_svm_desc") == [f[0] for f in capi.SvmDesc._fields_] == ["size", "maxVectors", "stream"]
    assert C.sizeof(capi.SvmDesc) == 16 and capi.SvmDesc.stream.offset == 8
    assert fields("compvhip_svm_shape") == [f[0] for f in capi.SvmShape._fields_] == ["size", "kernel", "nrClass", "totalSV", "dim", "pairs", "maxVectors", "reserved", "gamma"]
    assert C.sizeof(capi.SvmShape) == 40 and capi.SvmShape.gamma.offset == 32
    d = capi.SvmDesc(4096)
    assert (d.size, d.maxVectors, d.stream) == (16, 4096, None)
    assert capi.SvmShape().size == 40


def test_exp_on_the_host_equals_the_model_and_the_reference():
    from compv_amd import capi
    _, A = sc.golden()
    x = sc.exp_inputs()
    got = capi.svm_exp(x)
    assert got.tobytes() == sm.exp_ref(x).tobytes() == A["exp_out"].tobytes()
    assert capi.svm_exp(np.zeros(0)).size == 0


@pytest.mark.parametrize("c", sc.all_cases(), ids=lambda c: c["id"])
def test_parse_on_the_host_equals_the_fixture(c):
    from compv_amd import capi
    rec = sc.recorded_model(c)
    m = capi.SvmModel.from_file(sc.model_path(c["id"]))
    assert (m.kernel, m.nr_class, m.l, m.dim, m.pairs) == (rec.kernel, rec.nr_class, rec.l, rec.dim, rec.pairs)
    assert np.float64(m.gamma).tobytes() == np.float64(rec.gamma).tobytes()
    for got, exp in ((m.sv, rec.sv), (m.sv_coef, rec.sv_coef), (m.rho, rec.rho), (m.n_sv, rec.n_sv), (m.label, rec.label)):
        assert got.dtype == exp.dtype and got.shape == exp.shape and got.tobytes() == exp.tobytes()


@pytest.mark.parametrize("name", sorted(sc.BAD_FILES) + ["missing"])
def test_parse_refuses_bad_files_and_writes_nothing(tmp_path, name):
    from compv_amd import capi
    lib = capi.load()
    path = str(tmp_path / (name + ".model"))
    if name != "missing":
        sc.write_bad_file(path, name)
    s = capi.SvmShape()
    s.kernel, s.dim = 77, 78
    sv = np.full(4096, 7.0)
    nsv = np.full(32, 9, np.int32)
    assert lib.compvhip_svm_model_parse(os.fsencode(path), C.byref(s), sv.ctypes.data, sv.ctypes.data, sv.ctypes.data, nsv.ctypes.data, nsv.ctypes.data) == capi.E_INVALID_PARAMETER
    assert (s.kernel, s.dim) == (77, 78) and (sv == 7.0).all() and (nsv == 9).all()
    with pytest.raises(capi.CompvHipError):
        capi.SvmModel.from_file(path)


def test_refusals_before_any_hip_call():
    from compv_amd import capi
    lib = capi.load()
    good = os.fsencode(sc.model_path("rbf_d17_c2"))
    s = capi.SvmShape()
    s.kernel = 55
    assert lib.compvhip_svm_model_parse(None, C.byref(s), None, None, None, None, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_svm_model_parse(good, None, None, None, None, None, None) == capi.E_INVALID_PARAMETER
    s.size = 39
    assert lib.compvhip_svm_model_parse(good, C.byref(s), None, None, None, None, None) == capi.E_INVALID_PARAMETER and s.kernel == 55
    out = np.full(4, 3.0)
    assert lib.compvhip_svm_exp_f64(None, out.ctypes.data, 4) == capi.E_INVALID_PARAMETER and lib.compvhip_svm_exp_f64(out.ctypes.data, None, 4) == capi.E_INVALID_PARAMETER
    assert (out == 3.0).all()
    h = C.c_void_p(1234)
    d = capi.SvmDesc(8)
    m = capi.SvmModel.from_file(sc.model_path("rbf_d17_c2")).struct()
    assert lib.compvhip_svm_create(None, C.byref(m), C.byref(d), C.byref(h)) == capi.E_INVALID_PARAMETER and h.value == 1234
    assert lib.compvhip_svm_create_from_file(None, good, C.byref(d), C.byref(h)) == capi.E_INVALID_PARAMETER and h.value == 1234
    labels = np.full(8, 77, np.int32)
    x = np.zeros((8, 17))
    assert lib.compvhip_svm_predict(None, x.ctypes.data, capi.SVM_F64, 8, 17, labels.ctypes.data, None, None) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_svm_predict_host(None, x.ctypes.data, capi.SVM_F64, 8, 17, labels.ctypes.data, None) == capi.E_INVALID_PARAMETER
    s = capi.SvmShape()
    s.dim = 91
    assert lib.compvhip_svm_info(None, C.byref(s)) == capi.E_INVALID_PARAMETER and s.dim == 91
    assert lib.compvhip_svm_set_timing(None, 1) == capi.E_INVALID_PARAMETER
    assert lib.compvhip_svm_get_timing(None, None, None, 0) == capi.E_INVALID_PARAMETER
    assert (labels == 77).all() and not x.any()
    lib.compvhip_svm_destroy(None)          # a no-op
