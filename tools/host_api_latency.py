"""Latency of the host (drop-in) entry points: mean ms per call, including H2D/D2H and synchronisation.  One call of every framing of the host forms: the
cached-plan calls (sobel, canny, sht, adaptive threshold), the list calls (fast, components), the plan-less planes (remap, integral, grayscale, moments), KHT,
and -- on the committed fixtures, once, their size does not follow the image's -- the sliced calls (PCA, SVM) and the temporary-handle call (homography).
capi only: the same file runs against any build of the library."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from compv_amd import capi
from oracle_bindings import synth_frame
GOLDEN = os.path.join(ROOT, "tests", "golden")
ctx = capi.Context(0)
def t(fn, n=20):
    fn(); fn()
    t0 = time.perf_counter()
    for _ in range(n): fn()
    return (time.perf_counter() - t0) / n * 1e3
for (W, H) in [(1280, 720), (1920, 1080), (3840, 2160)]:
    img = synth_frame(W, H)
    e = ctx.canny(img, 59., 119.)
    print("%dx%d  sobel %.3f ms  canny %.3f ms  sht %.3f ms  kht %.3f ms" % (
        W, H, t(lambda: ctx.edge_dete(img)), t(lambda: ctx.canny(img, 59., 119.)), t(lambda: ctx.houghsht(e, 1.0, 100)), t(lambda: ctx.houghkht(e), 5)), flush=True)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    map_x, map_y = xs * 0.98 + 3.25, ys * 0.97 + 1.5
    rgb = np.ascontiguousarray(np.repeat(img, 3, axis=1))          # (H, 3 W): RGB24 rows
    cap = len(ctx.fast(img))                                       # no call below is repeated for a buffer that was too small
    ncomp = len(ctx.components(e, want_labels=False)[1])
    print("%dx%d  fast %.3f ms  adaptive %.3f ms  remap %.3f ms  integral %.3f ms  gray %.3f ms  components %.3f ms  moments %.3f ms" % (
        W, H, t(lambda: ctx.fast(img, cap=max(cap, 1))), t(lambda: ctx.threshold_adaptive(img, 15, 5.0)), t(lambda: ctx.remap(img, map_x, map_y)),
        t(lambda: ctx.integral(img)), t(lambda: ctx.grayscale(rgb, capi.FMT_RGB24, W)), t(lambda: ctx.components(e, cap=max(ncomp, 1))),
        t(lambda: ctx.moments(img))), flush=True)
rng = np.random.default_rng(1)
pca = capi.PcaModel.from_file(os.path.join(GOLDEN, "pca_trained_d130_m10.json"))
rows = rng.standard_normal((1024, pca.dim)).astype(np.float32)     # two slices of the host form
svm = capi.Svm(ctx, os.path.join(GOLDEN, "svm_rbf_d36_c2.model"), 1024)
vectors = rng.standard_normal((1024, svm.dim))
src = rng.uniform(0, 1000, (512, 2))
dst = src * 1.01 + rng.normal(0, 0.5, src.shape) + 7.0
print("fixtures  pca %.3f ms  svm %.3f ms  homography %.3f ms" % (
    t(lambda: ctx.pca_project_host(pca, rows)), t(lambda: svm.predict_host(vectors, want_dec=True)), t(lambda: ctx.homography_find(src, dst, tries=256))), flush=True)
svm.close()
