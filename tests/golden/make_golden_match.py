#!/usr/bin/env python
"""Generate tests/golden/golden_match.json from the COMPILED REFERENCE (oracle/_ref, built by oracle/build_ref.sh): shape and MD5 of the int32
record matrix CompVMatcherBruteForce::process returns, on descriptors any box can regenerate (tests/match_model.py: numpy default_rng seeds).
Run in the build container only: it compiles the small shim below (our own code: it only CALLS the reference's public API --
CompVMatcher::newObj(COMPV_BRUTEFORCE_ID), setInt, process) into a temporary directory and links it against oracle/_ref/libcompv_ref.so.
The reference runs on one thread (refshim_init(1)); one large case is run again on several threads to record that its answer does not depend
on the thread count.

cols = 5: the reference cannot be asked.  Its scalar popcount loop (base/math/compv_math_distance.cxx:207, `i <= width - 8` on an unsigned width)
underflows for every width below 8 and reads until it faults.  Those cases are put to the reference with each row padded to 8 bytes with zeros
(recorded as "ref_cols": 8) -- which leaves every distance as it is, and is what compvhip_match_hamming_u8 does on its way to the device."""
import ctypes as C
import hashlib, json, os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle_bindings import RefShim  # noqa: E402
import match_model as mm  # noqa: E402

SHIM = r"""
#include <compv/base/compv_base.h>
#include <compv/base/compv_matchers.h>
#include <compv/base/compv_mat.h>
#include <cstring>
using namespace compv;
extern "C" {
int matchshim_enums(int* v)
{
	v[0] = COMPV_BRUTEFORCE_ID; v[1] = COMPV_BRUTEFORCE_SET_INT_KNN; v[2] = COMPV_BRUTEFORCE_SET_INT_NORM; v[3] = COMPV_BRUTEFORCE_NORM_HAMMING;
	v[4] = (int)sizeof(CompVDMatch);
	return 0;
}
// -> rows of the match matrix (its columns are Q), or < 0; out receives rows * Q records of 4 int32
long matchshim_process(const uint8_t* query, size_t Q, const uint8_t* train, size_t T, size_t cols, int knn, int32_t* out, size_t capRows)
{
	CompVMatPtr q, t, m;
	if (COMPV_ERROR_CODE_IS_NOK(CompVMat::newObjAligned<uint8_t>(&q, Q, cols))) return -1;
	if (COMPV_ERROR_CODE_IS_NOK(CompVMat::newObjAligned<uint8_t>(&t, T, cols))) return -1;
	for (size_t j = 0; j < Q; ++j) memcpy(q->ptr<uint8_t>(j), query + j * cols, cols);
	for (size_t j = 0; j < T; ++j) memcpy(t->ptr<uint8_t>(j), train + j * cols, cols);
	CompVMatcherPtr matcher;
	if (COMPV_ERROR_CODE_IS_NOK(CompVMatcher::newObj(&matcher, COMPV_BRUTEFORCE_ID))) return -3;
	if (COMPV_ERROR_CODE_IS_NOK(matcher->setInt(COMPV_BRUTEFORCE_SET_INT_KNN, knn))) return -4;
	if (COMPV_ERROR_CODE_IS_NOK(matcher->setInt(COMPV_BRUTEFORCE_SET_INT_NORM, COMPV_BRUTEFORCE_NORM_HAMMING))) return -4;
	if (COMPV_ERROR_CODE_IS_NOK(matcher->process(q, t, &m))) return -5;
	if (m->cols() != Q || m->rows() > capRows) return -6;
	for (size_t r = 0; r < m->rows(); ++r) memcpy(out + r * Q * 4, m->ptr<const CompVDMatch>(r), Q * sizeof(CompVDMatch));
	return (long)m->rows();
}
}
"""

SIZES = (1, 2, 3, 65, 300)
COLS = (32, 8, 5)          # the reference takes a separate 32-byte path
KNN = (1, 2, 3, 8)
CONTENT = ("uniform", "ties")
BIG = {"Q": 2000, "T": 500, "cols": 32, "knn": 2, "content": "uniform", "seed": 424242, "threads": 4}


def build_shim(tmp):
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"          # the default of oracle/build_ref.sh
    src = os.path.join(tmp, "match_shim.cxx")
    so = os.path.join(tmp, "libmatch_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.check_call(["g++", "-include", "limits", "-std=c++11", "-O2", "-fPIC", "-w", "-DCOMPV_ASM=0", "-I%s/base/include" % ref, "-I%s/core/include" % ref,
                           "-shared", "-o", so, src, "-L" + refdir, "-lcompv_ref", "-Wl,-rpath," + refdir, "-ldl", "-lpthread"])
    return C.CDLL(so)


REF_MIN_COLS = 8          # below it the reference's popcount loop underflows (see above)


def padded(rows):
    if rows.shape[1] >= REF_MIN_COLS:
        return rows
    out = np.zeros((len(rows), REF_MIN_COLS), np.uint8)
    out[:, :rows.shape[1]] = rows
    return out


def run(L, query, train, knn):
    query, train = padded(query), padded(train)
    Q, cols = query.shape
    T = len(train)
    buf = np.zeros((max(knn, 1), Q, 4), np.int32)
    rows = L.matchshim_process(np.ascontiguousarray(query).ctypes.data, Q, np.ascontiguousarray(train).ctypes.data, T, cols, knn, buf.ctypes.data, len(buf))
    assert rows == min(knn, T), (rows, knn, T)
    return buf[:rows]


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a, "<i4").tobytes()).hexdigest()


def main():
    shim = RefShim(threads=1)          # refshim_init(1): the reference on one thread
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    with tempfile.TemporaryDirectory() as tmp:
        L = build_shim(tmp)
        L.matchshim_process.argtypes = [vp, sz, vp, sz, sz, i, vp, sz]
        L.matchshim_process.restype = C.c_long
        L.matchshim_enums.argtypes = [vp]
        ev = np.zeros(5, np.int32)
        L.matchshim_enums(ev.ctypes.data)
        out = {"enums": dict(zip(("BRUTEFORCE_ID", "SET_INT_KNN", "SET_INT_NORM", "NORM_HAMMING", "sizeof_CompVDMatch"), map(int, ev))), "cases": []}
        seed = 31000
        for kind in CONTENT:
            for cols in COLS:
                for Q in SIZES:
                    for T in SIZES:
                        seed += 1
                        query, train = mm.content(kind, Q, cols, seed), mm.content(kind, T, cols, seed + 100000)
                        for knn in KNN:
                            m = run(L, query, train, knn)
                            out["cases"].append({"Q": Q, "T": T, "cols": cols, "knn": knn, "content": kind, "seed": seed, "rows": int(len(m)), "md5": md5(m),
                                                 "ref_cols": max(cols, REF_MIN_COLS)})
        b = dict(BIG)
        query, train = mm.content(b["content"], b["Q"], b["cols"], b["seed"]), mm.content(b["content"], b["T"], b["cols"], b["seed"] + 100000)
        b["md5"] = md5(run(L, query, train, b["knn"]))
        shim.reinit(b["threads"])
        b["threads_used"] = int(shim.threads)
        b["md5_threads"] = md5(run(L, query, train, b["knn"]))
        shim.reinit(1)
        assert b["md5"] == b["md5_threads"], "the reference's answer depends on its thread count"
        out["big"] = b
    with open(os.path.join(HERE, "golden_match.json"), "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote %d cases; big case on %d threads: %s" % (len(out["cases"]), b["threads_used"], "same MD5"))


if __name__ == "__main__":
    main()
