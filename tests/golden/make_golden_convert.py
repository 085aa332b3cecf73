#!/usr/bin/env python
"""Generate tests/golden/golden_convert.json (+ golden_convert.npz) from tests/convert_model.py, held against the COMPILED REFERENCE (oracle/_ref, built by
oracle/build_ref.sh).  Run in the build container only: it compiles the small shim below (our own code: it only CALLS CompVImage::wrap, CompVImage::convert
and CompVCpu::flagsDisable / flagsEnable) into a temporary directory and links it against oracle/_ref/libcompv_ref.so.  The reference runs on one thread.

The parity target is the reference with every SIMD CPU flag switched off: the plain leaves, which are the definition the source states.  Asserted before
anything is written: for every case of tests/convert_cases.py and every destination its source is served to, model == reference (flags off) byte for byte,
stride padding excluded.  Only a case with an odd W or H may miss that (the reference's leaves derive chroma strides from the luma stride): it is stored as
"model only" with the reason.  Every case is also run with the flags on: for the integer conversions the fixture records per pair whether that path agrees
with the plain one; for RGB24 -> HSV on the exhaustive frame it records how many of the 2^24 triples differ and by how much (the AVX2 leaf uses an
approximate reciprocal whose result depends on the CPU model: a measurement, asserted nowhere).
Stored: an MD5 of every output plane of every case, the planes themselves for frames of up to convert_cases.STORE_LIMIT pixels."""
import ctypes as C
import hashlib
import json, os, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle_bindings import RefShim  # noqa: E402
import convert_model as cm  # noqa: E402
import convert_cases as cc  # noqa: E402

SHIM = r"""
#include <compv/base/compv_base.h>
#include <compv/base/compv_cpu.h>
#include <compv/base/compv_mat.h>
#include <compv/base/image/compv_image.h>
#include <cstring>
using namespace compv;
static bool subtype(int fmt, COMPV_SUBTYPE* s)
{
	static const COMPV_SUBTYPE k[18] = { COMPV_SUBTYPE_PIXELS_RGBA32, COMPV_SUBTYPE_PIXELS_ARGB32, COMPV_SUBTYPE_PIXELS_BGRA32, COMPV_SUBTYPE_PIXELS_RGB24,
		COMPV_SUBTYPE_PIXELS_BGR24, COMPV_SUBTYPE_PIXELS_RGB565LE, COMPV_SUBTYPE_PIXELS_RGB565BE, COMPV_SUBTYPE_PIXELS_BGR565LE, COMPV_SUBTYPE_PIXELS_BGR565BE,
		COMPV_SUBTYPE_PIXELS_YUYV422, COMPV_SUBTYPE_PIXELS_UYVY422, COMPV_SUBTYPE_PIXELS_Y, COMPV_SUBTYPE_PIXELS_NV12, COMPV_SUBTYPE_PIXELS_NV21,
		COMPV_SUBTYPE_PIXELS_YUV420P, COMPV_SUBTYPE_PIXELS_YUV422P, COMPV_SUBTYPE_PIXELS_YUV444P, COMPV_SUBTYPE_PIXELS_HSV };
	if (fmt < 0 || fmt >= 18) return false;
	*s = k[fmt];
	return true;
}
extern "C" {
int convshim_simd(int on)
{
	return COMPV_ERROR_CODE_IS_NOK(on ? CompVCpu::flagsEnable(kCpuFlagAll) : CompVCpu::flagsDisable(kCpuFlagAll)) ? -1 : 0;
}
// data: the source's planes one behind the other, plane 0 with dataStride samples per row.  out: the destination's planes one behind the other, dense;
// planes / rowBytes / rows describe them.  < 0: the reference refused.
int convshim_convert(int inFmt, const uint8_t* data, size_t W, size_t H, size_t dataStride, int outFmt, uint8_t* out, size_t outCap, int* planes,
                     size_t* rowBytes, size_t* rows)
{
	COMPV_SUBTYPE si, so;
	if (!subtype(inFmt, &si) || !subtype(outFmt, &so)) return -1;
	CompVMatPtr in, o;
	if (COMPV_ERROR_CODE_IS_NOK(CompVImage::wrap(si, data, W, H, dataStride, &in))) return -2;
	if (COMPV_ERROR_CODE_IS_NOK(CompVImage::convert(in, so, &o)) || !o) return -3;
	if (o->cols() != W || o->rows() != H) return -4;
	*planes = static_cast<int>(o->planeCount());
	size_t off = 0;
	for (int p = 0; p < *planes; ++p) {
		rowBytes[p] = o->rowInBytes(p); rows[p] = o->rows(p);
		if (off + rowBytes[p] * rows[p] > outCap) return -5;
		for (size_t j = 0; j < rows[p]; ++j, off += rowBytes[p]) memcpy(out + off, o->ptr<const uint8_t>(j, 0, p), rowBytes[p]);
	}
	return 0;
}
}
"""


def build_shim(tmp, ref="/root/reference"):          # the default of oracle/build_ref.sh
    src = os.path.join(tmp, "convert_shim.cxx")
    so = os.path.join(tmp, "libconvert_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    refdir = os.path.join(ROOT, "oracle", "_ref")
    subprocess.check_call(["g++", "-include", "limits", "-std=c++11", "-O2", "-fPIC", "-w", "-DCOMPV_ASM=0", "-I%s/base/include" % ref, "-shared", "-o", so, src,
                           "-L" + refdir, "-lcompv_ref", "-Wl,-rpath," + refdir, "-ldl", "-lpthread"])
    L = C.CDLL(so)
    vp, sz = C.c_void_p, C.c_size_t
    L.convshim_simd.argtypes = [C.c_int]
    L.convshim_convert.argtypes = [C.c_int, vp, sz, sz, sz, C.c_int, vp, sz, vp, vp, vp]
    return L


def reference(L, c, planes, dst):
    """the compiled reference's dense output planes with the CPU flags as convshim_simd left them, or a string: why it gave none"""
    W, H = c["W"], c["H"]
    data = np.concatenate([p.reshape(-1) for p in planes])
    stride = 2 * ((W + 1) // 2) if c["src"] in (cm.YUYV422, cm.UYVY422) else W          # packed 4:2:2 rows hold whole pairs
    out = np.zeros(4 * W * H + 64, np.uint8)
    n, rb, rows = C.c_int(0), (C.c_size_t * 3)(), (C.c_size_t * 3)()
    rc = L.convshim_convert(c["src"], data.ctypes.data, W, H, stride, dst, out.ctypes.data, out.size, C.byref(n), rb, rows)
    if rc:
        return "the reference refused (shim code %d)" % rc
    want = cm.plane_shapes(dst, W, H)
    got = [(rows[p], rb[p]) for p in range(n.value)]
    if got != want:
        return "the reference's planes are %r, the layout's %r" % (got, want)
    res, off = [], 0
    for r, b in got:
        res.append(out[off:off + r * b].reshape(r, b).copy())
        off += r * b
    return res


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    RefShim(threads=1)          # refshim_init(1): the reference on one thread
    meta = {"cases": [], "simd_agrees": {}, "hsv_simd": {}}
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        L = build_shim(tmp, *sys.argv[1:2])
        for c in cc.CASES:
            planes = cc.case_planes(c)
            odd = bool((c["W"] | c["H"]) & 1)
            stored = c["W"] * c["H"] <= cc.STORE_LIMIT
            rec = dict(id=c["id"], src=cm.NAMES[c["src"]], W=c["W"], H=c["H"], kind=c["kind"], stored=stored, frame_md5=[md5(p) for p in planes], md5={}, checked={})
            for dst in cc.destinations(c["src"]):
                m = cm.convert(c["src"], dst, planes, c["W"], c["H"])
                assert L.convshim_simd(0) == 0
                plain = reference(L, c, planes, dst)
                assert L.convshim_simd(1) == 0
                simd = reference(L, c, planes, dst)
                name = cm.NAMES[dst]
                why = plain if isinstance(plain, str) else None
                if why is None and not all(a.tobytes() == b.tobytes() for a, b in zip(m, plain)):
                    bad = sum(int((a != b).sum()) for a, b in zip(m, plain))
                    why = "the reference (SIMD off) differs from the model in %d bytes" % bad
                if why is not None:
                    assert odd, "%s -> %s: %s" % (c["id"], name, why)          # only odd-sized cases may be model only
                    rec["checked"][name] = "model only: " + why
                else:
                    rec["checked"][name] = "reference"
                    if not isinstance(simd, str):
                        agree = all(a.tobytes() == b.tobytes() for a, b in zip(plain, simd))
                        if dst == cm.HSV:
                            if c["kind"] == "exhaustive" and c["src"] == cm.RGB24:
                                d = np.abs(plain[0].astype(np.int16) - simd[0].astype(np.int16)).reshape(-1, 3)
                                meta["hsv_simd"] = dict(triples=int(d.shape[0]), differ=int((d.max(axis=1) > 0).sum()), max_abs_diff=[int(v) for v in d.max(axis=0)])
                        else:
                            k = cm.pair_name(c["src"], dst)
                            meta["simd_agrees"][k] = bool(meta["simd_agrees"].get(k, True) and agree)
                rec["md5"][name] = [md5(p) for p in m]
                if stored:
                    for i, p in enumerate(m):
                        arrays[cc.key(c, dst, i)] = p
            meta["cases"].append(rec)
            print(c["id"], rec["checked"], flush=True)
    for c in meta["cases"]:          # every even-sized case and both exhaustive frames are reference-checked
        assert ((c["W"] | c["H"]) & 1) or all(v == "reference" for v in c["checked"].values()), c["id"]
    with open(os.path.join(HERE, "golden_convert.json"), "w") as f:
        json.dump(meta, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "golden_convert.npz"), **arrays)
    only = sum(1 for c in meta["cases"] for v in c["checked"].values() if v != "reference")
    print("wrote %d cases; %d outputs are model only; SIMD disagreements: %s; HSV, SIMD against plain: %s"
          % (len(meta["cases"]), only, sorted(k for k, v in meta["simd_agrees"].items() if not v), meta["hsv_simd"]))


if __name__ == "__main__":
    main()
