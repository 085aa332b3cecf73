#!/usr/bin/env python
"""Generate tests/golden/golden_svm.json, golden_svm.npz and the trained model files tests/golden/svm_*.model from tests/svm_cases.py, held against the
COMPILED REFERENCE (oracle/_ref, built by oracle/build_ref.sh).  Run in the build container only: it compiles the small shim below (our own code: it only
CALLS the reference -- CompVCpu::flagsDisable, CompVMachineLearningSVM::newObj / train / save / rbf, svm_load_model, svm_makeSVs_SIMD_frienly,
svm_predict_values, CompVMathExp::exp) into a temporary directory and links it against oracle/_ref/libcompv_ref.so.  The reference runs on one thread
with every CPU flag disabled BEFORE any model is loaded (the leaves are hooked at load time): its plain C leaves are the definition.

Two kinds of model: the trained ones (the reference trains on small synthetic clusters and saves the file) and the hand-composed files of
svm_cases.hand_models().  For EVERY query of EVERY model the generator asserts that tests/svm_model.py, fed the file through its own parser, equals the
reference byte for byte in the decision values and the label, and -- for RBF models, where CompVMachineLearningSVM::rbf hands out the row -- in the kernel
values (the reference has no call that returns a LINEAR model's kernel values; they are pinned through the decision values).  exp_ref alone is held
against CompVMathExp::exp.  One mismatch fails the generator; nothing is skipped or retried.
Stored: per case K, dec and the labels, a trained file's parsed arrays, a hand-composed file's SHA-256 (the file itself is composed again on use); the queries are drawn again from the case's seed by svm_cases.queries()."""
import ctypes as C
import json, os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle_bindings import RefShim  # noqa: E402
import svm_model as sm  # noqa: E402
import svm_cases as sc  # noqa: E402

SHIM = r"""
#include <compv/base/compv_base.h>
#include <compv/base/compv_cpu.h>
#include <compv/base/compv_mat.h>
#include <compv/base/math/compv_math_exp.h>
#include <compv/base/ml/compv_base_ml_svm.h>
#include <compv/base/ml/libsvm-322/libsvm.h>
#include <vector>
using namespace compv;
extern "C" {
int svmshim_plain_c(void) { return COMPV_ERROR_CODE_IS_NOK(CompVCpu::flagsDisable(kCpuFlagAll)) ? -1 : 0; }
// CompVMachineLearningSVM::newObj / train / save on n vectors of D float64 values
int svmshim_train(const double* x, const int32_t* y, size_t n, size_t D, int kernel, double gamma, double cost, const char* path)
{
	CompVMachineLearningSVMParams params;
	params.svm_type = COMPV_SVM_TYPE_C_SVC; params.kernel_type = kernel; params.gamma = gamma; params.C = cost;
	CompVMachineLearningSVMPtr svm;
	if (COMPV_ERROR_CODE_IS_NOK(CompVMachineLearningSVM::newObj(&svm, params))) return -1;
	CompVMatPtr labels, vectors;
	if (COMPV_ERROR_CODE_IS_NOK(CompVMat::newObjAligned<int32_t>(&labels, 1, n)) || COMPV_ERROR_CODE_IS_NOK(CompVMat::newObjAligned<compv_float64_t>(&vectors, n, D))) return -2;
	for (size_t i = 0; i < n; ++i) {
		*labels->ptr<int32_t>(0, i) = y[i];
		for (size_t j = 0; j < D; ++j) *vectors->ptr<compv_float64_t>(i, j) = x[i * D + j];
	}
	if (COMPV_ERROR_CODE_IS_NOK(svm->train(labels, vectors))) return -3;
	return COMPV_ERROR_CODE_IS_NOK(svm->save(path)) ? -4 : 0;
}
// svm_load_model, and for RBF svm_makeSVs_SIMD_frienly as CompVMachineLearningSVM::load does; dims: kernel, nr_class, l, D
void* svmshim_load(const char* path, int* dims)
{
	svm_model* m = svm_load_model(path);
	if (!m) return nullptr;
	size_t D = 0;
	for (const svm_node* p = m->SV[0]; p->index != -1; ++p) ++D;
	if (m->param.kernel_type == RBF && COMPV_ERROR_CODE_IS_NOK(svm_makeSVs_SIMD_frienly(m, D))) return nullptr;
	dims[0] = m->param.kernel_type; dims[1] = m->nr_class; dims[2] = m->l; dims[3] = (int)D;
	return m;
}
void svmshim_free(void* model) { svm_model* m = (svm_model*)model; svm_free_and_destroy_model(&m); }
// svm_predict_values with a NODE_TYPE_MAT node (RBF) or an indexed node (LINEAR); K (RBF only): CompVMachineLearningSVM::rbf
int svmshim_predict(void* model, const double* x, size_t D, double* dec, double* K, int32_t* label)
{
	const svm_model* m = (const svm_model*)model;
	if (m->param.kernel_type == RBF) {
		CompVMatPtr v, k;
		if (COMPV_ERROR_CODE_IS_NOK(CompVMat::newObjAligned<compv_float64_t>(&v, 1, D))) return -1;
		for (size_t j = 0; j < D; ++j) *v->ptr<compv_float64_t>(0, j) = x[j];
		const svm_node_base node(NODE_TYPE_MAT, &v);
		*label = (int32_t)svm_predict_values(m, &node, dec);
		if (!K) return 0;
		if (COMPV_ERROR_CODE_IS_NOK(CompVMat::newObjAligned<compv_float64_t>(&k, 1, (size_t)m->l))) return -2;
		if (COMPV_ERROR_CODE_IS_NOK(CompVMachineLearningSVM::rbf(v, m->SVMat, (size_t)m->l, m->param.gamma, k, m))) return -3;
		for (int i = 0; i < m->l; ++i) K[i] = *k->ptr<const compv_float64_t>(0, i);
		return 0;
	}
	std::vector<svm_node> nodes(D + 1);
	for (size_t j = 0; j < D; ++j) { nodes[j].index = (int)j + 1; nodes[j].value = x[j]; }
	nodes[D].index = -1;
	const svm_node_base node(NODE_TYPE_INDEXED, nodes.data());
	*label = (int32_t)svm_predict_values(m, &node, dec);
	return 0;
}
int svmshim_exp(const double* in, double* out, size_t n)
{
	CompVMatPtr a, b;
	if (COMPV_ERROR_CODE_IS_NOK(CompVMat::newObjAligned<compv_float64_t>(&a, 1, n))) return -1;
	for (size_t i = 0; i < n; ++i) *a->ptr<compv_float64_t>(0, i) = in[i];
	if (COMPV_ERROR_CODE_IS_NOK(CompVMathExp::exp(a, &b))) return -2;
	for (size_t i = 0; i < n; ++i) out[i] = *b->ptr<const compv_float64_t>(0, i);
	return 0;
}
}
"""


def build_shim(tmp, ref="/root/reference", plain_c=True):          # ref: the default of oracle/build_ref.sh; plain_c=False (tools/svm_bench.py): the SIMD leaves stay
    src = os.path.join(tmp, "svm_shim.cxx")
    so = os.path.join(tmp, "libsvm_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.check_call(["g++", "-include", "limits", "-std=c++11", "-O2", "-fPIC", "-w", "-DCOMPV_ASM=0", "-I%s/base/include" % ref, "-shared", "-o", so, src,
                           "-L" + refdir, "-lcompv_ref", "-Wl,-rpath," + refdir, "-ldl", "-lpthread"])
    L = C.CDLL(so)
    vp, sz = C.c_void_p, C.c_size_t
    L.svmshim_train.argtypes = [vp, vp, sz, sz, C.c_int, C.c_double, C.c_double, C.c_char_p]
    L.svmshim_load.argtypes = [C.c_char_p, vp]
    L.svmshim_load.restype = vp
    L.svmshim_free.argtypes = [vp]
    L.svmshim_free.restype = None
    L.svmshim_predict.argtypes = [vp, vp, sz, vp, vp, vp]
    L.svmshim_exp.argtypes = [vp, vp, sz]
    if plain_c:
        assert L.svmshim_plain_c() == 0
    return L


def reference(L, path, X):
    """-> (labels, dec, K or None) of the reference on the file's model"""
    dims = np.zeros(4, np.int32)
    h = L.svmshim_load(path.encode(), dims.ctypes.data)
    assert h, path
    kernel, nc, l, D = (int(v) for v in dims)
    assert D == X.shape[1]
    P = nc * (nc - 1) // 2
    labels, dec, K = np.zeros(len(X), np.int32), np.zeros((len(X), P)), np.zeros((len(X), l))
    X64 = np.ascontiguousarray(X.astype(np.float64))          # CompVMachineLearningSVM::predict casts a float32 vector first
    for i in range(len(X)):
        lab = np.zeros(1, np.int32)
        assert L.svmshim_predict(h, X64[i].ctypes.data, D, dec[i].ctypes.data, K[i].ctypes.data, lab.ctypes.data) == 0
        labels[i] = lab[0]
    L.svmshim_free(h)
    return labels, dec, (K if kernel == sm.RBF else None)


def reference_time(L, path, X):
    """seconds the reference needs for svm_predict_values on every row of X (float64), the model loaded beforehand (tools/svm_bench.py)"""
    import time
    dims = np.zeros(4, np.int32)
    h = L.svmshim_load(path.encode(), dims.ctypes.data)
    assert h, path
    nc, l, D = int(dims[1]), int(dims[2]), int(dims[3])
    dec, lab = np.zeros(nc * (nc - 1) // 2), np.zeros(1, np.int32)
    t0 = time.perf_counter()
    for i in range(len(X)):
        assert L.svmshim_predict(h, X[i].ctypes.data, D, dec.ctypes.data, None, lab.ctypes.data) == 0
    t = time.perf_counter() - t0
    L.svmshim_free(h)
    return t


def main():
    RefShim(threads=1)          # refshim_init(1): the reference on one thread
    meta = {"cases": []}
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        L = build_shim(tmp, *sys.argv[1:2])
        # exp_ref alone
        x = sc.exp_inputs()
        ref = np.zeros_like(x)
        assert L.svmshim_exp(x.ctypes.data, ref.ctypes.data, x.size) == 0
        got = sm.exp_ref(x)
        assert got.tobytes() == ref.tobytes(), ("exp_ref", int((got.view(np.uint64) != ref.view(np.uint64)).sum()))
        arrays["exp_out"] = ref
        meta["exp_inputs"] = int(x.size)
        for c in sc.all_cases():
            path = sc.model_path(c["id"])          # a hand-composed file: written into a temporary directory, only its SHA-256 is stored
            if "sv_text" not in c:
                tx, ty = sc.training_set(c)
                assert L.svmshim_train(np.ascontiguousarray(tx).ctypes.data, ty.ctypes.data, len(tx), c["D"], c["kernel"], c["gamma"], 4.0, path.encode()) == 0, c["id"]
            m = sm.parse(path)
            assert (m.kernel, m.dim, m.nr_class) == (c["kernel"], c["D"], c["classes"]), c["id"]
            X = sc.queries(c, m)
            labels, dec, K = sm.predict(m, X)
            rl, rd, rk = reference(L, path, X)
            assert labels.tobytes() == rl.tobytes(), (c["id"], "labels", int((labels != rl).sum()))
            assert dec.tobytes() == rd.tobytes(), (c["id"], "dec", int((dec.view(np.uint64) != rd.view(np.uint64)).sum()))
            if rk is not None:
                assert K.tobytes() == rk.tobytes(), (c["id"], "K", int((K.view(np.uint64) != rk.view(np.uint64)).sum()))
            cid = c["id"]
            arrays["K_" + cid], arrays["dec_" + cid], arrays["lab_" + cid] = K, dec, labels
            if "sv_text" not in c:          # the parsed arrays of the files that are kept
                arrays["sv_" + cid], arrays["coef_" + cid], arrays["rho_" + cid] = m.sv, m.sv_coef, m.rho
                arrays["nsv_" + cid], arrays["label_" + cid] = m.n_sv, m.label
            meta["cases"].append(dict(id=cid, kernel=m.kernel, dim=m.dim, classes=m.nr_class, l=m.l, gamma=float(m.gamma).hex(), nq=len(X), qtype=c["qtype"],
                                      trained="sv_text" not in c, sha256=sc.file_sha256(path), labels_seen=sorted({int(v) for v in labels}), bytes=os.path.getsize(path)))
            print("%-22s l %3d  labels %s  file %d bytes" % (cid, m.l, meta["cases"][-1]["labels_seen"], meta["cases"][-1]["bytes"]))
    with open(os.path.join(HERE, "golden_svm.json"), "w") as f:
        json.dump(meta, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "golden_svm.npz"), **arrays)
    print("wrote %d cases, %d exp inputs" % (len(meta["cases"]), x.size))


if __name__ == "__main__":
    main()
