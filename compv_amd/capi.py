"""ctypes binding of the C ABI in include/compv_hip.h (compv_amd/lib/libcompv_hip.so).

This is plumbing for tests and bench.py: the product is the shared library itself, which a CompV build binds
directly from C++.  There is NO CPU fallback: importing works without a GPU (so that the
symbol-export test can run), but creating a context without a GPU, or loading without the built library, fails loudly.
"""
import ctypes as C
import importlib.util
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libcompv_hip.so")

OK = 0
E_NOT_IMPLEMENTED = -1
E_NOT_INITIALIZED = -2
E_INVALID_STATE = -3
E_INVALID_PARAMETER = -4
E_OUT_OF_MEMORY = -5
E_OUT_OF_BOUND = -6
E_HIP = -7

OP_SOBEL, OP_SCHARR, OP_PREWITT = 0, 2, 3
THRESHOLD_COMPARE_TO_GRADIENT, THRESHOLD_PERCENT_OF_MEAN, THRESHOLD_OTSU = 0, 1, 2
(FMT_RGBA32, FMT_ARGB32, FMT_BGRA32, FMT_RGB24, FMT_BGR24, FMT_RGB565LE, FMT_RGB565BE, FMT_BGR565LE, FMT_BGR565BE,
 FMT_YUYV422, FMT_UYVY422, FMT_Y) = range(12)
FMT_BYTES = [4, 4, 4, 3, 3, 2, 2, 2, 2, 2, 2, 1]
FMT_NV12, FMT_NV21, FMT_YUV420P, FMT_YUV422P, FMT_YUV444P, FMT_HSV = range(12, 18)   # formats of the colour conversion calls only
MORPH_ERODE, MORPH_DILATE, MORPH_OPEN, MORPH_CLOSE = 0, 1, 2, 3
STREL_RECT, STREL_DIAMOND, STREL_CROSS = 0, 1, 2
BORDER_ZERO, BORDER_REPLICATE = 0, 2
MORPH_KERNEL_AUTO, MORPH_KERNEL_GENERAL, MORPH_KERNEL_SEPARABLE = 0, 1, 2
INTERP_NEAREST, INTERP_BILINEAR, INTERP_BILINEAR_FLOAT32 = 0, 1, 2
INTERP_BICUBIC, INTERP_BICUBIC_FLOAT32 = 4, 5                    # 3 is unassigned
CORNER_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("strength", "<i4")])   # compvhip_corner
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("strength", "<f4"), ("orient", "<f4"), ("level", "<i4"), ("size", "<f4")])   # compvhip_keypoint = CompVInterestPoint
MATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imageIdx", "<i4"), ("distance", "<i4")])   # compvhip_match = CompVDMatch
HOG_NORM_NONE, HOG_NORM_L1, HOG_NORM_L1SQRT, HOG_NORM_L2, HOG_NORM_L2HYS = 1, 2, 3, 4, 5          # COMPVHIP_HOG_NORM_* (0: the default, L2HYS)
HOG_GRADIENT_SIGNED, HOG_GRADIENT_UNSIGNED = 1, 2                                              # COMPVHIP_HOG_GRADIENT_* (0: the default, signed)
HOG_INTERP_NEAREST, HOG_INTERP_BILINEAR, HOG_INTERP_BILINEAR_LUT = 1, 2, 3                     # COMPVHIP_HOG_INTERP_* (0: the default, BILINEAR; _LUT is refused)
HOMOGRAPHY_RESULT_DTYPE = np.dtype([("H", "<f8", (9,)), ("variance", "<f8"), ("inliers", "<i4"), ("bestTry", "<i4"), ("status", "<i4"), ("rotations", "<i4")])   # compvhip_homography_result
CURVEFIT_LINE, CURVEFIT_PARABOLA, CURVEFIT_PARABOLA_SIDEWAYS = 0, 1, 2                         # COMPVHIP_CURVEFIT_*
SVM_KERNEL_LINEAR, SVM_KERNEL_RBF = 0, 2                                                       # COMPVHIP_SVM_KERNEL_* (libsvm's kernel_type numbers)
SVM_F32, SVM_F64 = 0, 1                                                                        # COMPVHIP_SVM_F32 / _F64
UNDISTORT_F32, UNDISTORT_F64 = 0, 1                                                            # COMPVHIP_UNDISTORT_F32 / _F64
UNDISTORT_COEFFS = 14                                                                          # values of a camera's coefficient record
MOMENTS_VALUE, MOMENTS_UNIT = 0, 1                                                             # COMPVHIP_MOMENTS_VALUE / _UNIT
MOMENTS_ORIGIN_FRAME, MOMENTS_ORIGIN_BOX = 0, 1                                                # COMPVHIP_MOMENTS_ORIGIN_*
MOMENTS_DTYPE = np.dtype([(k, "<u8") for k in ("m00", "m01", "m10", "m11", "m02", "m20")])     # compvhip_moments
MOMENTS_SHAPE_DTYPE = np.dtype([(k, "<f8") for k in ("xbar", "ybar", "u20", "u02", "u11", "skew", "cs", "sn")] + [("status", "<i4"), ("pad", "<i4")])   # compvhip_moments_shape
CURVEFIT_RESULT_DTYPE = np.dtype([("A", "<f8"), ("B", "<f8"), ("C", "<f8"), ("inliers", "<i4"), ("bestTry", "<i4"), ("status", "<i4"), ("k", "<i4")])   # compvhip_curvefit_result

# every symbol include/compv_hip.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "compvhip_device_count", "compvhip_ctx_create", "compvhip_ctx_destroy", "compvhip_last_error",
    "compvhip_live_allocations", "compvhip_debug_alloc_fill", "compvhip_edge_dete_u8", "compvhip_canny_u8", "compvhip_houghsht_u8",
    "compvhip_houghsht_dims", "compvhip_houghsht_vote_grid", "compvhip_plan_create", "compvhip_plan_destroy", "compvhip_plan_canny",
    "compvhip_plan_houghsht", "compvhip_plan_pipeline", "compvhip_plan_acc", "compvhip_plan_edge_counts",
    "compvhip_plan_set_timing", "compvhip_plan_get_timing", "compvhip_plan_acc_export", "compvhip_plan_edge_dete",
    "compvhip_houghkht_u8", "compvhip_grayscale_u8", "compvhip_otsu_u8", "compvhip_plan_grayscale", "compvhip_plan_otsu",
    "compvhip_gauss_kernel_fixedpoint", "compvhip_convlt1_fixedpoint_u8", "compvhip_plan_convlt1_fixedpoint", "compvhip_plan_to_cartesian",
    "compvhip_plan_pipeline_async", "compvhip_plan_wait", "compvhip_houghsht_to_cartesian", "compvhip_houghkht_to_cartesian",
    "compvhip_houghkht_kernels_u8", "compvhip_houghkht_stage_ms", "compvhip_convlt1_8u16s16s", "compvhip_convlt1_16s16s16s",
    "compvhip_plan_pipeline_ex", "compvhip_plan_houghkht", "compvhip_plan_houghkht_stage_ms", "compvhip_houghkht_link_u8",
    "compvhip_houghkht_dims", "compvhip_host_cpu_budget", "compvhip_plan_houghkht_ex", "compvhip_houghkht_ex_u8",
    "compvhip_plan_houghsht_segments", "compvhip_houghsht_segments_u8",
    "compvhip_plan_houghsht_fit", "compvhip_houghsht_fit_u8",
    "compvhip_plan_components", "compvhip_components_u8",
    "compvhip_threshold_u8", "compvhip_plan_threshold", "compvhip_threshold_adaptive_u8", "compvhip_plan_threshold_adaptive",
    "compvhip_morph_strel", "compvhip_morph_u8", "compvhip_plan_morph", "compvhip_plan_morph_ex",
    "compvhip_plan_fast", "compvhip_fast_u8",
    "compvhip_plan_orb_keypoints", "compvhip_plan_orb_describe", "compvhip_orb_u8",
    "compvhip_matcher_create", "compvhip_matcher_destroy", "compvhip_matcher_knn", "compvhip_matcher_good", "compvhip_match_hamming_u8",
    "compvhip_matcher_set_timing", "compvhip_matcher_get_timing",
    "compvhip_orbpyr_create", "compvhip_orbpyr_destroy", "compvhip_orbpyr_geometry", "compvhip_orbpyr_plane", "compvhip_orbpyr_detect", "compvhip_orbpyr_describe",
    "compvhip_plan_scale", "compvhip_scale_u8", "compvhip_orb_pyramid_u8", "compvhip_orbpyr_set_timing", "compvhip_orbpyr_get_timing",
    "compvhip_warp_tables", "compvhip_plan_remap", "compvhip_plan_warp_inverse", "compvhip_remap_u8", "compvhip_warp_inverse_u8",
    "compvhip_homography_create", "compvhip_homography_destroy", "compvhip_homography_points", "compvhip_homography_find", "compvhip_homography_project",
    "compvhip_homography_quads", "compvhip_homography_find_f64", "compvhip_homography_scores", "compvhip_homography_set_timing", "compvhip_homography_get_timing",
    "compvhip_curvefit_create", "compvhip_curvefit_destroy", "compvhip_curvefit_points_from_labels", "compvhip_curvefit_find", "compvhip_curvefit_distances",
    "compvhip_curvefit_scores", "compvhip_curvefit_gathered", "compvhip_curvefit_set_timing", "compvhip_curvefit_get_timing", "compvhip_curvefit_samples",
    "compvhip_curvefit_find_f64",
    "compvhip_hog_geometry", "compvhip_plan_hog", "compvhip_hog_u8",
    "compvhip_integral_dims", "compvhip_plan_integral", "compvhip_integral_u8", "compvhip_plan_histogram", "compvhip_histogram_u8", "compvhip_plan_equalize",
    "compvhip_equalize_u8", "compvhip_plan_projections", "compvhip_projections_u8",
    "compvhip_convert_layout", "compvhip_convert_frames", "compvhip_convert_u8",
    "compvhip_svm_create", "compvhip_svm_create_from_file", "compvhip_svm_destroy", "compvhip_svm_info", "compvhip_svm_predict", "compvhip_svm_predict_host",
    "compvhip_svm_set_timing", "compvhip_svm_get_timing", "compvhip_svm_exp_f64", "compvhip_svm_model_parse",
    "compvhip_undistort_coeffs_f32", "compvhip_undistort_coeffs_f64", "compvhip_undistort_map_f32", "compvhip_undistort_map_f64",
    "compvhip_undistort_create", "compvhip_undistort_destroy", "compvhip_undistort_frames", "compvhip_undistort_maps", "compvhip_undistort_points",
    "compvhip_undistort_project", "compvhip_undistort_u8", "compvhip_undistort_set_timing", "compvhip_undistort_get_timing",
    "compvhip_moments_frames", "compvhip_moments_components", "compvhip_moments_shapes", "compvhip_moments_shape_host", "compvhip_moments_fits", "compvhip_moments_host",
    "compvhip_pca_project", "compvhip_mulabt_f32", "compvhip_pca_covariance", "compvhip_pca_covariance_scratch", "compvhip_pca_project_host", "compvhip_pca_model_parse",
    "compvhip_pca_dot_host",
]

KHT_ORDER_REFERENCE, KHT_ORDER_CANONICAL = 0, 1
KHT_ORDERS = {"reference": KHT_ORDER_REFERENCE, "canonical": KHT_ORDER_CANONICAL}


class Line(C.Structure):
    _fields_ = [("rho", C.c_float), ("theta", C.c_float), ("strength", C.c_int32), ("row", C.c_int32), ("col", C.c_int32)]


LINE_DTYPE = np.dtype([("rho", "<f4"), ("theta", "<f4"), ("strength", "<i4"), ("row", "<i4"), ("col", "<i4")])


class Segment(C.Structure):
    """compvhip_segment (include/compv_hip.h): a piece of an SHT line between the pixels (x0, y0) and (x1, y1)"""
    _fields_ = [("line", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32), ("support", C.c_int32)]


SEGMENT_DTYPE = np.dtype([("line", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("support", "<i4")])


class LineFit(C.Structure):
    """compvhip_line_fit (include/compv_hip.h): the band's pixel count and moments, the fitted unit normal (nx, ny), rho and mean squared distance"""
    _fields_ = [("line", C.c_int32), ("pixels", C.c_int32), ("sx", C.c_int64), ("sy", C.c_int64), ("sxx", C.c_int64), ("sxy", C.c_int64), ("syy", C.c_int64),
                ("nx", C.c_double), ("ny", C.c_double), ("rho", C.c_double), ("rms2", C.c_double)]


LINE_FIT_DTYPE = np.dtype([("line", "<i4"), ("pixels", "<i4"), ("sx", "<i8"), ("sy", "<i8"), ("sxx", "<i8"), ("sxy", "<i8"), ("syy", "<i8"),
                           ("nx", "<f8"), ("ny", "<f8"), ("rho", "<f8"), ("rms2", "<f8")])


class Component(C.Structure):
    """compvhip_component (include/compv_hip.h): root (x, y), inclusive bounding box, pixel count of a connected component"""
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32), ("pixels", C.c_int32)]


COMP_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("pixels", "<i4")])


class PipelineOpts(C.Structure):
    """compvhip_pipeline_opts (include/compv_hip.h)"""
    _fields_ = [("tLow", C.c_float), ("tHigh", C.c_float), ("threshold", C.c_int), ("maxLines", C.c_int), ("ksize", C.c_int),
                ("thresholdType", C.c_int), ("pixfmt", C.c_int), ("d_gray", C.c_void_p), ("d_otsu", C.c_void_p), ("d_cart", C.c_void_p)]


class KhtOpts(C.Structure):
    """compvhip_kht_opts (include/compv_hip.h): a zero field takes the default"""
    _fields_ = [("rho", C.c_float), ("thetaDeg", C.c_float), ("threshold", C.c_int), ("maxLines", C.c_int), ("clusterMinDeviation", C.c_double),
                ("clusterMinSize", C.c_size_t), ("kernelMinHeight", C.c_double), ("hostThreads", C.c_int), ("order", C.c_int)]


def _kht_order(order):
    if order not in KHT_ORDERS:
        raise ValueError("order must be one of %s, not %r" % (sorted(KHT_ORDERS), order))
    return KHT_ORDERS[order]


class Keypoint(C.Structure):
    """compvhip_keypoint (include/compv_hip.h): CompVInterestPoint's layout, 24 bytes"""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("strength", C.c_float), ("orient", C.c_float), ("level", C.c_int32), ("size", C.c_float)]


class MatchOpts(C.Structure):
    """compvhip_match_opts (include/compv_hip.h): ratio <= 0 / maxDistance < 0 / crossCheck == 0 switch a test off"""
    _fields_ = [("ratio", C.c_double), ("maxDistance", C.c_int), ("crossCheck", C.c_int)]


class HomographyOpts(C.Structure):
    """compvhip_homography_opts (include/compv_hip.h); the reference's outlier threshold is 30"""
    _fields_ = [("tries", C.c_int32), ("seed", C.c_uint32), ("threshold", C.c_double)]

    def __init__(self, tries=2000, seed=0, threshold=30.0):
        super().__init__(int(tries), int(seed) & 0xffffffff, float(threshold))


class CurvefitDesc(C.Structure):
    """compvhip_curvefit_desc (include/compv_hip.h): the handle's capacities and the stream all its calls run on"""
    _fields_ = [("size", C.c_uint32), ("sets", C.c_uint32), ("pointCap", C.c_uint32), ("maxTries", C.c_uint32), ("stream", C.c_void_p)]

    def __init__(self, sets=1, point_cap=3, max_tries=2000, stream=0):
        super().__init__(C.sizeof(CurvefitDesc), int(sets), int(point_cap), int(max_tries), stream or None)


class CurvefitOpts(C.Structure):
    """compvhip_curvefit_opts (include/compv_hip.h)"""
    _fields_ = [("size", C.c_uint32), ("model", C.c_int32), ("tries", C.c_int32), ("seed", C.c_uint32), ("threshold", C.c_double)]

    def __init__(self, model=CURVEFIT_LINE, tries=2000, seed=0, threshold=1.0):
        super().__init__(C.sizeof(CurvefitOpts), int(model), int(tries), int(seed) & 0xffffffff, float(threshold))


class SvmModelStruct(C.Structure):
    """compvhip_svm_model (include/compv_hip.h): host arrays, copied by compvhip_svm_create"""
    _fields_ = [("size", C.c_uint32), ("kernel", C.c_int32), ("nrClass", C.c_int32), ("totalSV", C.c_int32), ("dim", C.c_int32), ("reserved", C.c_int32),
                ("gamma", C.c_double), ("sv", C.c_void_p), ("svCoef", C.c_void_p), ("rho", C.c_void_p), ("nSV", C.c_void_p), ("label", C.c_void_p)]


class SvmDesc(C.Structure):
    """compvhip_svm_desc (include/compv_hip.h): the handle's capacity and the stream all its calls run on"""
    _fields_ = [("size", C.c_uint32), ("maxVectors", C.c_uint32), ("stream", C.c_void_p)]

    def __init__(self, max_vectors=1, stream=0):
        super().__init__(C.sizeof(SvmDesc), int(max_vectors), stream or None)


class SvmShape(C.Structure):
    """compvhip_svm_shape (include/compv_hip.h)"""
    _fields_ = [("size", C.c_uint32), ("kernel", C.c_int32), ("nrClass", C.c_int32), ("totalSV", C.c_int32), ("dim", C.c_int32), ("pairs", C.c_int32),
                ("maxVectors", C.c_uint32), ("reserved", C.c_uint32), ("gamma", C.c_double)]

    def __init__(self):
        super().__init__(C.sizeof(SvmShape))


class UndistortDesc(C.Structure):
    """compvhip_undistort_desc (include/compv_hip.h): the geometry of the fused form, the caps of the point calls and the stream all calls run on"""
    _fields_ = [("size", C.c_uint32), ("W", C.c_uint32), ("H", C.c_uint32), ("S", C.c_uint32), ("frames", C.c_uint32), ("Wout", C.c_uint32), ("Hout", C.c_uint32),
                ("x0", C.c_uint32), ("y0", C.c_uint32), ("maxSets", C.c_uint32), ("maxPoints", C.c_uint32), ("reserved", C.c_uint32), ("stream", C.c_void_p)]

    def __init__(self, W=0, H=0, S=0, frames=0, Wout=0, Hout=0, x0=0, y0=0, max_sets=0, max_points=0, stream=0):
        super().__init__(C.sizeof(UndistortDesc), W, H, S, frames, Wout, Hout, x0, y0, max_sets, max_points, 0, stream or None)


class MomentsDesc(C.Structure):
    """compvhip_moments_desc (include/compv_hip.h): how a pixel counts, the origin of the coordinates and the stream the device calls run on"""
    _fields_ = [("size", C.c_uint32), ("weights", C.c_int32), ("origin", C.c_int32), ("hipStream", C.c_void_p)]

    def __init__(self, weights=MOMENTS_VALUE, origin=MOMENTS_ORIGIN_FRAME, stream=0):
        super().__init__(C.sizeof(MomentsDesc), weights, origin, stream or None)


class PcaDesc(C.Structure):
    """compvhip_pca_desc (include/compv_hip.h): the stream the device calls run on"""
    _fields_ = [("size", C.c_uint32), ("reserved", C.c_uint32), ("hipStream", C.c_void_p)]

    def __init__(self, stream=0):
        super().__init__(C.sizeof(PcaDesc), 0, stream or None)


def curvefit_model_points(model):
    """m of a COMPVHIP_CURVEFIT_* model: 2 for a line, 3 for a parabola"""
    return 2 if model == CURVEFIT_LINE else 3


class HogOpts(C.Structure):
    """compvhip_hog_opts (include/compv_hip.h): a zero field takes the reference's default -- block 16 x 16, stride 8 x 8, cell 8 x 8, 9 bins, L2HYS, signed,
    BILINEAR.  Keywords: block / stride / cell (a number, or (w, h)), nbins, norm (HOG_NORM_* or its name), signed, interp (HOG_INTERP_* or its name), or the
    struct's own field names."""
    _fields_ = [("size", C.c_uint32), ("blockW", C.c_int32), ("blockH", C.c_int32), ("strideW", C.c_int32), ("strideH", C.c_int32), ("cellW", C.c_int32),
                ("cellH", C.c_int32), ("nbins", C.c_int32), ("blockNorm", C.c_int32), ("gradientSigned", C.c_int32), ("interp", C.c_int32)]
    NORMS = {"none": HOG_NORM_NONE, "l1": HOG_NORM_L1, "l1sqrt": HOG_NORM_L1SQRT, "l2": HOG_NORM_L2, "l2hys": HOG_NORM_L2HYS}
    INTERPS = {"nearest": HOG_INTERP_NEAREST, "bilinear": HOG_INTERP_BILINEAR, "bilinear_lut": HOG_INTERP_BILINEAR_LUT}

    def __init__(self, block=0, stride=0, cell=0, nbins=0, norm=0, signed=None, interp=0, **fields):
        pair = lambda v: (int(v), int(v)) if np.isscalar(v) else (int(v[0]), int(v[1]))          # noqa: E731
        (bw, bh), (sw, sh), (cw, ch) = pair(block), pair(stride), pair(cell)
        super().__init__(C.sizeof(HogOpts), bw, bh, sw, sh, cw, ch, int(nbins), self.NORMS.get(norm, norm), 0 if signed is None else (HOG_GRADIENT_SIGNED if signed else HOG_GRADIENT_UNSIGNED),
                         self.INTERPS.get(interp, interp))
        for k, v in fields.items():
            if k not in dict(self._fields_) or k == "size":
                raise TypeError("HogOpts has no field %r" % k)
            setattr(self, k, int(v))


def _hog_opts(opts, kw):
    """a HogOpts, or the keywords of one"""
    if opts is not None and kw:
        raise TypeError("pass a HogOpts or keywords, not both")
    return opts if opts is not None else HogOpts(**kw)


class Roi(C.Structure):
    """compvhip_roi (include/compv_hip.h): the source rectangle of a remap, inclusive"""
    _fields_ = [("left", C.c_float), ("right", C.c_float), ("top", C.c_float), ("bottom", C.c_float)]


def _roi(roi):
    """None, a Roi or (left, right, top, bottom) -> what ctypes passes for a const compvhip_roi*"""
    if roi is None:
        return None
    return C.byref(roi if isinstance(roi, Roi) else Roi(*roi))


class OrbPyramidOpts(C.Structure):
    """compvhip_orbpyr_opts (include/compv_hip.h); the defaults are CompVCornerDeteORB's"""
    _fields_ = [("levels", C.c_int), ("scaleFactor", C.c_float), ("threshold", C.c_int), ("fastType", C.c_int), ("nonmax", C.c_int), ("maxFeatures", C.c_int)]

    def __init__(self, levels=8, scale_factor=0.83, threshold=20, fast_type=9, nonmax=True, max_features=2000):
        super().__init__(levels, scale_factor, threshold, fast_type, int(bool(nonmax)), max_features)


class Image(C.Structure):
    """compvhip_image (include/compv_hip.h): `frames` images of one format -- plane pointers, bytes from row to row and from frame to frame"""
    _fields_ = [("pixfmt", C.c_int), ("plane", C.c_void_p * 3), ("rowBytes", C.c_size_t * 3), ("frameBytes", C.c_size_t * 3)]

    def __init__(self, pixfmt, planes, row_bytes, frame_bytes=()):
        """planes: addresses (int or None); row_bytes / frame_bytes: one value per plane"""
        super().__init__()
        self.pixfmt = pixfmt
        for i, p in enumerate(planes):
            self.plane[i] = p
        for i, v in enumerate(row_bytes):
            self.rowBytes[i] = v
        for i, v in enumerate(frame_bytes):
            self.frameBytes[i] = v


class CompvHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("compvhip error %d: %s" % (code, msg))
        self.code = code


_lib = None


def _share_hip_runtime_with_torch():
    """PyTorch wheels bundle their own libamdhip64.so (same soname as /opt/rocm's).  Device pointers are only
    interchangeable inside ONE HIP runtime, so when torch is installed its copy is loaded first and the loader
    resolves libcompv_hip.so's DT_NEEDED libamdhip64.so.7 to it (no torch import needed, no dependency on torch)."""
    try:
        spec = importlib.util.find_spec("torch")
    except Exception:
        spec = None
    if spec and spec.submodule_search_locations:
        p = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(p):
            C.CDLL(p, mode=C.RTLD_GLOBAL)


def load():
    """Load the HIP library; raises if it was not built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("compv_amd: %s is missing -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(the HIP extension is mandatory; there is no CPU fallback)" % LIB_PATH)
    _share_hip_runtime_with_torch()
    L = C.CDLL(LIB_PATH)
    sz, vp, i32 = C.c_size_t, C.c_void_p, C.c_int
    L.compvhip_device_count.restype = i32
    L.compvhip_ctx_create.argtypes = [C.POINTER(vp), i32]
    L.compvhip_ctx_destroy.argtypes = [vp]
    L.compvhip_ctx_destroy.restype = None
    L.compvhip_last_error.argtypes = [vp]
    L.compvhip_last_error.restype = C.c_char_p
    L.compvhip_live_allocations.argtypes = [vp]
    L.compvhip_live_allocations.restype = C.c_long
    L.compvhip_debug_alloc_fill.argtypes = [C.c_int]
    L.compvhip_debug_alloc_fill.restype = C.c_int
    L.compvhip_edge_dete_u8.argtypes = [vp, vp, sz, sz, sz, i32, vp, sz]
    L.compvhip_canny_u8.argtypes = [vp, vp, sz, sz, sz, C.c_float, C.c_float, i32, i32, vp, sz]
    L.compvhip_houghsht_u8.argtypes = [vp, vp, sz, sz, sz, C.c_float, C.c_float, i32, i32, vp, sz, C.POINTER(sz), vp, sz]
    L.compvhip_houghkht_kernels_u8.argtypes = [vp, vp, sz, sz, sz, C.c_double, sz, vp, sz, C.POINTER(sz), C.POINTER(C.c_double)]
    L.compvhip_houghkht_stage_ms.argtypes = [vp, vp]
    L.compvhip_houghkht_u8.argtypes = [vp, vp, sz, sz, sz, C.c_float, C.c_float, i32, i32, C.c_double, sz, C.c_double, vp, sz, C.POINTER(sz),
                                       C.POINTER(C.c_double)]
    L.compvhip_houghsht_dims.argtypes = [sz, sz, C.c_float, C.POINTER(sz), C.POINTER(sz), C.POINTER(C.c_float)]
    L.compvhip_houghsht_vote_grid.argtypes = [sz, sz, C.c_float, sz, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.compvhip_plan_create.argtypes = [vp, sz, sz, sz, sz, C.c_float, C.POINTER(vp)]
    L.compvhip_plan_destroy.argtypes = [vp]
    L.compvhip_plan_destroy.restype = None
    L.compvhip_plan_canny.argtypes = [vp, vp, C.c_float, C.c_float, i32, i32, vp, vp]
    L.compvhip_plan_houghsht.argtypes = [vp, vp, i32, i32, vp, sz, vp, vp]
    L.compvhip_plan_edge_dete.argtypes = [vp, vp, i32, vp, vp]
    L.compvhip_grayscale_u8.argtypes = [vp, vp, i32, sz, sz, sz, vp, sz]
    L.compvhip_otsu_u8.argtypes = [vp, vp, sz, sz, sz, C.POINTER(C.c_double)]
    L.compvhip_plan_grayscale.argtypes = [vp, vp, i32, vp, vp]
    L.compvhip_plan_otsu.argtypes = [vp, vp, vp, vp]
    L.compvhip_plan_to_cartesian.argtypes = [vp, vp, vp, sz, vp, vp]
    L.compvhip_gauss_kernel_fixedpoint.argtypes = [sz, C.c_float, vp]
    L.compvhip_convlt1_fixedpoint_u8.argtypes = [vp, vp, sz, sz, sz, vp, vp, sz, vp, sz]
    L.compvhip_plan_convlt1_fixedpoint.argtypes = [vp, vp, vp, vp, sz, vp, vp]
    L.compvhip_convlt1_8u16s16s.argtypes = [vp, vp, sz, sz, sz, vp, vp, sz, vp, sz]
    L.compvhip_convlt1_16s16s16s.argtypes = [vp, vp, sz, sz, sz, vp, vp, sz, vp, sz]
    L.compvhip_plan_pipeline.argtypes = [vp, vp, C.c_float, C.c_float, i32, i32, vp, vp, sz, vp, vp]
    L.compvhip_plan_pipeline_async.argtypes = [vp, vp, C.c_float, C.c_float, i32, i32, vp, vp, sz, vp, vp, C.POINTER(i32)]
    L.compvhip_plan_wait.argtypes = [vp, i32]
    L.compvhip_plan_houghkht.argtypes = [vp, vp, C.c_float, C.c_float, i32, i32, C.c_double, sz, C.c_double, vp, sz, vp, vp, i32]
    L.compvhip_plan_houghkht_stage_ms.argtypes = [vp, vp, C.POINTER(C.c_double), C.POINTER(i32)]
    L.compvhip_plan_houghkht_ex.argtypes = [vp, vp, C.POINTER(KhtOpts), vp, sz, vp, vp]
    L.compvhip_houghkht_ex_u8.argtypes = [vp, vp, sz, sz, sz, C.POINTER(KhtOpts), vp, sz, C.POINTER(sz), C.POINTER(C.c_double)]
    L.compvhip_plan_pipeline_ex.argtypes = [vp, vp, C.POINTER(PipelineOpts), vp, vp, sz, vp, vp, C.POINTER(i32)]
    L.compvhip_plan_houghsht_segments.argtypes = [vp, vp, vp, vp, sz, i32, i32, i32, vp, sz, vp, vp]
    L.compvhip_houghsht_segments_u8.argtypes = [vp, vp, sz, sz, sz, C.c_float, vp, sz, i32, i32, vp, sz, C.POINTER(sz)]
    L.compvhip_plan_houghsht_fit.argtypes = [vp, vp, vp, vp, sz, i32, i32, vp, vp, sz, vp, sz, vp, vp, vp]
    L.compvhip_houghsht_fit_u8.argtypes = [vp, vp, sz, sz, sz, C.c_float, vp, sz, i32, vp, sz, vp, sz, C.POINTER(sz), vp]
    L.compvhip_plan_components.argtypes = [vp, vp, i32, i32, vp, sz, vp, sz, vp, vp]
    L.compvhip_components_u8.argtypes = [vp, vp, sz, sz, sz, i32, i32, vp, sz, vp, sz, C.POINTER(sz)]
    f64 = C.c_double
    L.compvhip_threshold_u8.argtypes = [vp, vp, sz, sz, sz, f64, vp, sz]
    L.compvhip_plan_threshold.argtypes = [vp, vp, f64, vp, vp, vp]
    L.compvhip_threshold_adaptive_u8.argtypes = [vp, vp, sz, sz, sz, sz, f64, f64, i32, vp, sz]
    L.compvhip_plan_threshold_adaptive.argtypes = [vp, vp, sz, f64, f64, i32, vp, vp]
    L.compvhip_morph_strel.argtypes = [i32, sz, sz, vp]
    L.compvhip_morph_u8.argtypes = [vp, vp, sz, sz, sz, vp, sz, sz, i32, i32, vp, sz]
    L.compvhip_plan_morph.argtypes = [vp, vp, vp, sz, sz, i32, i32, vp, vp]
    L.compvhip_plan_morph_ex.argtypes = [vp, vp, vp, sz, sz, i32, i32, i32, vp, vp]
    L.compvhip_plan_fast.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, sz, vp, vp]
    L.compvhip_fast_u8.argtypes = [vp, vp, sz, sz, sz, i32, i32, i32, i32, vp, sz, vp, sz, C.POINTER(sz)]
    L.compvhip_plan_orb_keypoints.argtypes = [vp, vp, vp, sz, vp, i32, C.c_float, vp, sz, vp, vp, vp]
    L.compvhip_plan_orb_describe.argtypes = [vp, vp, vp, sz, vp, C.c_float, i32, vp, sz, vp]
    L.compvhip_orb_u8.argtypes = [vp, vp, sz, sz, sz, vp, sz, i32, C.c_float, vp, vp, sz, C.POINTER(sz)]
    L.compvhip_matcher_create.argtypes = [vp, sz, sz, sz, sz, i32, C.POINTER(vp)]
    L.compvhip_matcher_destroy.argtypes = [vp]
    L.compvhip_matcher_destroy.restype = None
    L.compvhip_matcher_knn.argtypes = [vp, vp, sz, vp, vp, sz, vp, i32, vp, vp]
    L.compvhip_matcher_good.argtypes = [vp, vp, vp, sz, vp, vp, sz, vp, i32, C.POINTER(MatchOpts), vp, sz, vp, vp]
    L.compvhip_match_hamming_u8.argtypes = [vp, vp, sz, sz, vp, sz, sz, sz, i32, vp, sz, C.POINTER(sz)]
    L.compvhip_matcher_set_timing.argtypes = [vp, i32]
    L.compvhip_matcher_get_timing.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), i32]
    L.compvhip_orbpyr_create.argtypes = [vp, sz, sz, sz, sz, C.POINTER(OrbPyramidOpts), sz, C.POINTER(vp)]
    L.compvhip_orbpyr_destroy.argtypes = [vp]
    L.compvhip_orbpyr_destroy.restype = None
    L.compvhip_orbpyr_geometry.argtypes = [vp, i32, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), C.POINTER(C.c_float), C.POINTER(i32)]
    L.compvhip_orbpyr_plane.argtypes = [vp, i32, i32, C.POINTER(vp)]
    L.compvhip_orbpyr_detect.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp]
    L.compvhip_orbpyr_describe.argtypes = [vp, vp, i32, vp, sz, vp, vp, sz, vp]
    L.compvhip_plan_scale.argtypes = [vp, vp, vp, sz, sz, sz, vp]
    L.compvhip_scale_u8.argtypes = [vp, vp, sz, sz, sz, vp, sz, sz, sz]
    L.compvhip_warp_tables.argtypes = [vp, i32, sz, sz, vp, vp, vp, vp, vp, vp]
    L.compvhip_plan_remap.argtypes = [vp, vp, vp, vp, sz, i32, C.POINTER(Roi), C.c_uint8, vp, sz, sz, sz, vp]
    L.compvhip_plan_warp_inverse.argtypes = [vp, vp, vp, i32, sz, i32, C.c_uint8, vp, sz, sz, sz, vp]
    L.compvhip_remap_u8.argtypes = [vp, vp, sz, sz, sz, vp, vp, i32, C.POINTER(Roi), C.c_uint8, vp, sz, sz, sz]
    L.compvhip_warp_inverse_u8.argtypes = [vp, vp, sz, sz, sz, vp, i32, i32, C.c_uint8, vp, sz, sz, sz]
    L.compvhip_orb_pyramid_u8.argtypes = [vp, vp, sz, sz, sz, C.POINTER(OrbPyramidOpts), vp, vp, sz, sz, C.POINTER(sz)]
    L.compvhip_orbpyr_set_timing.argtypes = [vp, i32]
    L.compvhip_orbpyr_get_timing.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), i32]
    L.compvhip_homography_create.argtypes = [vp, sz, sz, sz, C.POINTER(vp)]
    L.compvhip_homography_destroy.argtypes = [vp]
    L.compvhip_homography_destroy.restype = None
    L.compvhip_homography_points.argtypes = [vp, vp, sz, vp, vp, sz, vp, sz, i32, vp]
    L.compvhip_homography_find.argtypes = [vp, vp, vp, vp, C.POINTER(HomographyOpts), vp, vp, vp, vp]
    L.compvhip_homography_project.argtypes = [vp, vp, vp, sz, i32, vp, vp]
    L.compvhip_homography_quads.argtypes = [C.c_uint32, sz, sz, sz, vp]
    L.compvhip_homography_find_f64.argtypes = [vp, vp, vp, sz, C.POINTER(HomographyOpts), vp, vp, vp]
    L.compvhip_homography_scores.argtypes = [vp, sz, vp, vp, vp, vp]
    L.compvhip_homography_set_timing.argtypes = [vp, i32]
    L.compvhip_homography_get_timing.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), i32]
    L.compvhip_curvefit_create.argtypes = [vp, C.POINTER(CurvefitDesc), C.POINTER(vp)]
    L.compvhip_curvefit_destroy.argtypes = [vp]
    L.compvhip_curvefit_destroy.restype = None
    L.compvhip_curvefit_points_from_labels.argtypes = [vp, vp, sz, sz, sz, vp, sz, vp, sz]
    L.compvhip_curvefit_find.argtypes = [vp, vp, vp, C.POINTER(CurvefitOpts), vp, vp, vp]
    L.compvhip_curvefit_distances.argtypes = [vp, vp, vp, i32, vp, vp]
    L.compvhip_curvefit_scores.argtypes = [vp, sz, vp, vp]
    L.compvhip_curvefit_gathered.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.compvhip_curvefit_set_timing.argtypes = [vp, i32]
    L.compvhip_curvefit_get_timing.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), i32]
    L.compvhip_curvefit_samples.argtypes = [i32, C.c_uint32, sz, sz, sz, vp]
    L.compvhip_curvefit_find_f64.argtypes = [vp, vp, sz, C.POINTER(CurvefitOpts), vp, vp, vp]
    L.compvhip_hog_geometry.argtypes = [sz, sz, C.POINTER(HogOpts), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    L.compvhip_plan_hog.argtypes = [vp, vp, C.POINTER(HogOpts), vp, vp, sz, vp]
    L.compvhip_hog_u8.argtypes = [vp, vp, sz, sz, sz, C.POINTER(HogOpts), vp, sz, C.POINTER(sz)]
    L.compvhip_integral_dims.argtypes = [sz, sz, C.POINTER(sz), C.POINTER(sz)]
    L.compvhip_plan_integral.argtypes = [vp, vp, vp, vp, sz, vp]
    L.compvhip_integral_u8.argtypes = [vp, vp, sz, sz, sz, vp, vp, sz]
    L.compvhip_plan_histogram.argtypes = [vp, vp, vp, vp]
    L.compvhip_histogram_u8.argtypes = [vp, vp, sz, sz, sz, vp]
    L.compvhip_plan_equalize.argtypes = [vp, vp, vp, C.c_double, vp, vp, vp]
    L.compvhip_equalize_u8.argtypes = [vp, vp, sz, sz, sz, vp, C.c_double, vp, sz, vp]
    L.compvhip_plan_projections.argtypes = [vp, vp, vp, vp, vp]
    L.compvhip_projections_u8.argtypes = [vp, vp, sz, sz, sz, vp, vp]
    L.compvhip_convert_layout.argtypes = [i32, sz, sz, C.POINTER(i32), C.POINTER(sz), C.POINTER(sz)]
    L.compvhip_convert_frames.argtypes = [vp, sz, sz, sz, C.POINTER(Image), C.POINTER(Image), vp]
    L.compvhip_convert_u8.argtypes = [vp, sz, sz, C.POINTER(Image), C.POINTER(Image)]
    L.compvhip_svm_create.argtypes = [vp, C.POINTER(SvmModelStruct), C.POINTER(SvmDesc), C.POINTER(vp)]
    L.compvhip_svm_create_from_file.argtypes = [vp, C.c_char_p, C.POINTER(SvmDesc), C.POINTER(vp)]
    L.compvhip_svm_destroy.argtypes = [vp]
    L.compvhip_svm_destroy.restype = None
    L.compvhip_svm_info.argtypes = [vp, C.POINTER(SvmShape)]
    L.compvhip_svm_predict.argtypes = [vp, vp, i32, sz, sz, vp, vp, vp]
    L.compvhip_svm_predict_host.argtypes = [vp, vp, i32, sz, sz, vp, vp]
    L.compvhip_svm_set_timing.argtypes = [vp, i32]
    L.compvhip_svm_get_timing.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), i32]
    L.compvhip_svm_exp_f64.argtypes = [vp, vp, sz]
    L.compvhip_svm_model_parse.argtypes = [C.c_char_p, C.POINTER(SvmShape), vp, vp, vp, vp, vp]
    for f in (L.compvhip_undistort_coeffs_f32, L.compvhip_undistort_coeffs_f64):
        f.argtypes = [vp, vp, i32, vp]
    for f in (L.compvhip_undistort_map_f32, L.compvhip_undistort_map_f64):
        f.argtypes = [vp, vp, i32, sz, sz, sz, sz, vp, vp]
    L.compvhip_undistort_create.argtypes = [vp, C.POINTER(UndistortDesc), C.POINTER(vp)]
    L.compvhip_undistort_destroy.argtypes = [vp]
    L.compvhip_undistort_destroy.restype = None
    L.compvhip_undistort_frames.argtypes = [vp, vp, vp, vp, i32, sz, i32, C.POINTER(Roi), C.c_uint8, vp, sz]
    L.compvhip_undistort_maps.argtypes = [vp, vp, vp, i32, sz, i32, vp, vp]
    L.compvhip_undistort_points.argtypes = [vp, vp, vp, i32, sz, i32, vp, sz, sz, vp, vp]
    L.compvhip_undistort_project.argtypes = [vp, vp, vp, i32, sz, vp, vp, sz, sz, vp, vp]
    L.compvhip_undistort_u8.argtypes = [vp, vp, sz, sz, sz, vp, vp, i32, sz, sz, i32, C.POINTER(Roi), C.c_uint8, vp, sz, sz, sz]
    L.compvhip_undistort_set_timing.argtypes = [vp, i32]
    L.compvhip_undistort_get_timing.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), i32]
    L.compvhip_moments_frames.argtypes = [vp, C.POINTER(MomentsDesc), vp, sz, sz, sz, sz, vp, vp]
    L.compvhip_moments_components.argtypes = [vp, C.POINTER(MomentsDesc), vp, sz, sz, sz, vp, sz, vp, sz, vp, sz, vp, vp]
    L.compvhip_moments_shapes.argtypes = [vp, C.POINTER(MomentsDesc), vp, sz, vp]
    L.compvhip_moments_shape_host.argtypes = [vp, sz, vp]
    L.compvhip_moments_fits.argtypes = [sz, sz, i32]
    L.compvhip_moments_host.argtypes = [vp, C.POINTER(MomentsDesc), vp, sz, sz, sz, vp, vp]
    L.compvhip_pca_project.argtypes = [vp, C.POINTER(PcaDesc), vp, vp, sz, sz, sz, vp, sz, sz, vp, sz]
    L.compvhip_mulabt_f32.argtypes = [vp, C.POINTER(PcaDesc), vp, sz, sz, vp, sz, sz, sz, vp, sz]
    L.compvhip_pca_covariance.argtypes = [vp, C.POINTER(PcaDesc), vp, sz, sz, sz, vp, vp, sz, vp]
    L.compvhip_pca_covariance_scratch.argtypes = [sz, sz, C.POINTER(sz)]
    L.compvhip_pca_project_host.argtypes = [vp, C.POINTER(PcaDesc), vp, vp, sz, sz, sz, vp, sz, sz, vp, sz]
    L.compvhip_pca_model_parse.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, vp, vp]
    L.compvhip_pca_dot_host.argtypes = [vp, vp, sz, C.POINTER(C.c_float)]
    L.compvhip_plan_acc.argtypes = [vp, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    L.compvhip_plan_acc_export.argtypes = [vp, sz, vp, sz, vp]
    L.compvhip_plan_edge_counts.argtypes = [vp, C.POINTER(vp)]
    L.compvhip_plan_set_timing.argtypes = [vp, i32]
    L.compvhip_plan_get_timing.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), i32]
    _lib = L
    return L


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def warp_tables(M, out_w, out_h):
    """compvhip_warp_tables (host arithmetic, no GPU): the running-sum tables of a (2, 3) or (3, 3) float32 matrix -> (ac, df, gi, by, ey, hy); gi and hy are
    None for two rows"""
    L = load()
    M = np.ascontiguousarray(M, np.float32)
    assert M.ndim == 2 and M.shape[1] == 3
    rows = M.shape[0]
    ac, df, gi = (np.zeros(out_w, np.float32) for _ in range(3))
    by, ey, hy = (np.zeros(out_h, np.float32) for _ in range(3))
    rc = L.compvhip_warp_tables(_ptr(M), rows, out_w, out_h, _ptr(ac), _ptr(df), _ptr(gi) if rows == 3 else None, _ptr(by), _ptr(ey), _ptr(hy) if rows == 3 else None)
    if rc != OK:
        raise CompvHipError(rc, "compvhip_warp_tables")
    return (ac, df, gi, by, ey, hy) if rows == 3 else (ac, df, None, by, ey, None)


def _cameras(K, d, dtype):
    """K (3, 3) or (count, 3, 3), d (nd,) or (count, nd), nd in 2 .. 4 -> contiguous K, d of `dtype`, nd, count (shapes are not judged here: the C ABI refuses)"""
    K, d = np.ascontiguousarray(K, dtype), np.ascontiguousarray(d, dtype)
    assert K.shape[-2:] == (3, 3) and K.ndim in (2, 3) and d.ndim == K.ndim - 1
    count = 1 if K.ndim == 2 else K.shape[0]
    assert K.ndim == 2 or d.shape[0] == count
    return K, d, int(d.shape[-1]), count


def undistort_coeffs(K, d, dtype=np.float32):
    """compvhip_undistort_coeffs_f32 / _f64 (host arithmetic, no GPU): the 14-value coefficient record of one camera -- fx, fy, cx, cy, skew, k1, k2, p1, p2,
    kinv11, kinv21, kinv31, kinv22, kinv32 -- in `dtype`"""
    L = load()
    dtype = np.dtype(dtype)
    assert dtype in (np.float32, np.float64)
    K, d = np.ascontiguousarray(K, dtype), np.ascontiguousarray(d, dtype).ravel()
    assert K.shape == (3, 3)
    out = np.zeros(UNDISTORT_COEFFS, dtype)
    fn = L.compvhip_undistort_coeffs_f32 if dtype == np.float32 else L.compvhip_undistort_coeffs_f64
    rc = fn(_ptr(K), _ptr(d), d.size, _ptr(out))
    if rc != OK:
        raise CompvHipError(rc, "compvhip_undistort_coeffs")
    return out


def undistort_map(K, d, out_w, out_h, x0=0, y0=0, dtype=np.float32):
    """compvhip_undistort_map_f32 / _f64 (host arithmetic, no GPU): CompVCalibUtils::initUndistMap -> map_x, map_y (out_h, out_w) of `dtype`"""
    L = load()
    dtype = np.dtype(dtype)
    assert dtype in (np.float32, np.float64)
    K, d = np.ascontiguousarray(K, dtype), np.ascontiguousarray(d, dtype).ravel()
    assert K.shape == (3, 3)
    mx, my = np.zeros((max(out_h, 0), max(out_w, 0)), dtype), np.zeros((max(out_h, 0), max(out_w, 0)), dtype)
    fn = L.compvhip_undistort_map_f32 if dtype == np.float32 else L.compvhip_undistort_map_f64
    rc = fn(_ptr(K), _ptr(d), d.size, x0, y0, out_w, out_h, _ptr(mx), _ptr(my))
    if rc != OK:
        raise CompvHipError(rc, "compvhip_undistort_map")
    return mx, my


def moments_fits(W, H, weights=MOMENTS_VALUE):
    """compvhip_moments_fits (host arithmetic, no GPU): may a frame of W x H be given with these weights (no sum can reach 2^64)"""
    return bool(load().compvhip_moments_fits(W, H, weights))


def moments_shape_host(raw):
    """compvhip_moments_shape_host (host arithmetic, no GPU): raw records (MOMENTS_DTYPE, or an (n, 6) array of integers) -> MOMENTS_SHAPE_DTYPE records"""
    L = load()
    if not isinstance(raw, np.ndarray):
        raw = np.array([[int(v) for v in r] for r in raw], dtype=np.uint64)          # (Python integers up to 2^64 - 1, without a trip through float64)
    raw = np.ascontiguousarray(raw)
    if raw.dtype != MOMENTS_DTYPE:
        raw = np.ascontiguousarray(raw, np.uint64).reshape(-1, 6).view(MOMENTS_DTYPE).reshape(-1)
    raw = raw.reshape(-1)
    out = np.zeros(raw.size, MOMENTS_SHAPE_DTYPE)
    rc = L.compvhip_moments_shape_host(_ptr(raw), raw.size, _ptr(out))
    if rc != OK:
        raise CompvHipError(rc, "compvhip_moments_shape_host")
    return out


def homography_quads(seed, pair, k, tries):
    """compvhip_homography_quads (host arithmetic, no GPU): int32 (tries, 4), the point indices of every try of pair `pair` among k >= 4 points"""
    L = load()
    out = np.zeros((tries, 4), np.int32)
    rc = L.compvhip_homography_quads(int(seed) & 0xffffffff, pair, k, tries, _ptr(out))
    if rc != OK:
        raise CompvHipError(rc, "compvhip_homography_quads")
    return out


def curvefit_samples(model, seed, set_index, k, tries):
    """compvhip_curvefit_samples (host arithmetic, no GPU): int32 (tries, m), the point indices of every try of set `set_index` among k > m points"""
    L = load()
    out = np.zeros((tries, curvefit_model_points(model)), np.int32)
    rc = L.compvhip_curvefit_samples(int(model), int(seed) & 0xffffffff, set_index, k, tries, _ptr(out))
    if rc != OK:
        raise CompvHipError(rc, "compvhip_curvefit_samples")
    return out


def svm_exp(x):
    """compvhip_svm_exp_f64 (host arithmetic, no GPU): the reference's table exponential of a float64 array"""
    L = load()
    x = np.ascontiguousarray(x, np.float64)
    out = np.zeros_like(x)
    rc = L.compvhip_svm_exp_f64(_ptr(x), _ptr(out), x.size)
    if rc != OK:
        raise CompvHipError(rc, "compvhip_svm_exp_f64")
    return out


class SvmModel:
    """A C-SVC model as host arrays: kernel (SVM_KERNEL_*), gamma, sv (l, dim), sv_coef (nr_class - 1, l), rho (pairs,), n_sv and label (nr_class,)."""

    def __init__(self, kernel, gamma, sv, sv_coef, rho, n_sv, label):
        self.kernel, self.gamma = int(kernel), float(gamma)
        self.sv = np.ascontiguousarray(sv, np.float64)
        self.sv_coef = np.ascontiguousarray(sv_coef, np.float64)
        self.rho = np.ascontiguousarray(rho, np.float64)
        self.n_sv = np.ascontiguousarray(n_sv, np.int32)
        self.label = np.ascontiguousarray(label, np.int32)
        self.nr_class, (self.l, self.dim) = len(self.label), self.sv.shape
        self.pairs = self.nr_class * (self.nr_class - 1) // 2

    @classmethod
    def from_file(cls, path):
        """compvhip_svm_model_parse (host, no GPU): a libsvm model file; CompvHipError where compvhip_svm_create_from_file would refuse it"""
        L = load()
        s = SvmShape()
        rc = L.compvhip_svm_model_parse(os.fsencode(path), C.byref(s), None, None, None, None, None)
        if rc != OK:
            raise CompvHipError(rc, "compvhip_svm_model_parse")
        sv, coef = np.zeros((s.totalSV, s.dim)), np.zeros((s.nrClass - 1, s.totalSV))
        rho, n_sv, label = np.zeros(s.pairs), np.zeros(s.nrClass, np.int32), np.zeros(s.nrClass, np.int32)
        rc = L.compvhip_svm_model_parse(os.fsencode(path), C.byref(s), _ptr(sv), _ptr(coef), _ptr(rho), _ptr(n_sv), _ptr(label))
        if rc != OK:
            raise CompvHipError(rc, "compvhip_svm_model_parse")
        return cls(s.kernel, s.gamma, sv, coef, rho, n_sv, label)

    def struct(self):
        return SvmModelStruct(C.sizeof(SvmModelStruct), self.kernel, self.nr_class, self.l, self.dim, 0, self.gamma, self.sv.ctypes.data, self.sv_coef.ctypes.data,
                              self.rho.ctypes.data, self.n_sv.ctypes.data, self.label.ctypes.data)


def pca_dot(a, b):
    """compvhip_pca_dot_host (host arithmetic, no GPU): the sixteen-accumulator float32 dot product of CompVMath::mulABt"""
    L = load()
    a, b = np.ascontiguousarray(a, np.float32).ravel(), np.ascontiguousarray(b, np.float32).ravel()
    assert a.size == b.size
    out = C.c_float()
    rc = L.compvhip_pca_dot_host(_ptr(a) if a.size else None, _ptr(b) if b.size else None, a.size, C.byref(out))
    if rc != OK:
        raise CompvHipError(rc, "compvhip_pca_dot_host")
    return np.float32(out.value)


def pca_covariance_scratch(n, dim):
    """compvhip_pca_covariance_scratch (host arithmetic, no GPU): the bytes compvhip_pca_covariance needs for n observations of dim dimensions"""
    b = C.c_size_t(0)
    rc = load().compvhip_pca_covariance_scratch(n, dim, C.byref(b))
    if rc != OK:
        raise CompvHipError(rc, "compvhip_pca_covariance_scratch")
    return b.value


class PcaModel:
    """A PCA model: mean (dim,) or None, vectors (components, dim) -- the eigenvectors as rows -- and values (components,) or None, float32 host arrays;
    to_device() uploads mean and vectors with torch and keeps the tensors (d_mean, d_vectors)."""

    def __init__(self, mean, vectors, values=None):
        self.vectors = np.ascontiguousarray(vectors, np.float32)
        assert self.vectors.ndim == 2
        self.components, self.dim = self.vectors.shape
        self.mean = None if mean is None else np.ascontiguousarray(mean, np.float32).reshape(self.dim)
        self.values = None if values is None else np.ascontiguousarray(values, np.float32).reshape(self.components)
        self.d_mean = self.d_vectors = None

    @classmethod
    def from_file(cls, path):
        """compvhip_pca_model_parse (host, no GPU): a model file as CompVMathPCA::write produces it; CompvHipError where the file is refused"""
        L = load()
        d, m = C.c_int32(0), C.c_int32(0)
        rc = L.compvhip_pca_model_parse(os.fsencode(path), C.byref(d), C.byref(m), None, None, None)
        if rc != OK:
            raise CompvHipError(rc, "compvhip_pca_model_parse")
        mean, vectors, values = np.zeros(d.value, np.float32), np.zeros((m.value, d.value), np.float32), np.zeros(m.value, np.float32)
        rc = L.compvhip_pca_model_parse(os.fsencode(path), C.byref(d), C.byref(m), _ptr(mean), _ptr(vectors), _ptr(values))
        if rc != OK:
            raise CompvHipError(rc, "compvhip_pca_model_parse")
        return cls(mean, vectors, values)

    def to_device(self, device="cuda:0"):
        import torch
        self.d_vectors = torch.from_numpy(self.vectors).to(device)
        self.d_mean = None if self.mean is None else torch.from_numpy(self.mean).to(device)
        return self


def hog_geometry(W, H, opts=None, **kw):
    """compvhip_hog_geometry (host arithmetic, no GPU): -> dict(cellsX, cellsY, blocksX, blocksY, descLen) of a W x H frame; CompvHipError where the device calls
    would refuse the parameters"""
    L = load()
    o = _hog_opts(opts, kw)
    v = [C.c_size_t(0) for _ in range(5)]
    rc = L.compvhip_hog_geometry(W, H, C.byref(o), *[C.byref(x) for x in v])
    if rc != OK:
        raise CompvHipError(rc, "compvhip_hog_geometry")
    return dict(zip(("cellsX", "cellsY", "blocksX", "blocksY", "descLen"), (x.value for x in v)))


def integral_dims(W, H):
    """compvhip_integral_dims (host arithmetic, no GPU): -> (rows, cols) = (H + 1, W + 1) of the integral images of a W x H frame; CompvHipError for W = 0,
    H = 0, a side beyond 32 767 or 2^31 pixels and more -- what the device calls refuse"""
    L = load()
    rows, cols = C.c_size_t(0), C.c_size_t(0)
    rc = L.compvhip_integral_dims(W, H, C.byref(rows), C.byref(cols))
    if rc != OK:
        raise CompvHipError(rc, "compvhip_integral_dims")
    return rows.value, cols.value


def convert_layout(pixfmt, W, H):
    """compvhip_convert_layout (host arithmetic, no GPU): -> (planes, minRowBytes[3], rows[3]) of a W x H image of the format; CompvHipError for an unknown
    format or a zero size"""
    L = load()
    n, rb, rows = C.c_int(0), (C.c_size_t * 3)(), (C.c_size_t * 3)()
    rc = L.compvhip_convert_layout(pixfmt, W, H, C.byref(n), rb, rows)
    if rc != OK:
        raise CompvHipError(rc, "compvhip_convert_layout")
    return n.value, list(rb), list(rows)


class Context:
    """One GPU context (compvhip_ctx)."""

    def __init__(self, device=-1):
        self.lib = load()
        h = C.c_void_p()
        rc = self.lib.compvhip_ctx_create(C.byref(h), device)
        if rc != OK:
            raise CompvHipError(rc, "compvhip_ctx_create failed (no usable GPU? the HIP path is mandatory)")
        self.h = h

    def close(self):
        if self.h:
            self.lib.compvhip_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return self.lib.compvhip_last_error(self.h).decode()

    def live_allocations(self):
        return self.lib.compvhip_live_allocations(self.h)

    def _chk(self, rc):
        if rc != OK:
            raise CompvHipError(rc, self.last_error())

    # ---- host entry points (numpy in / numpy out) ----
    def edge_dete(self, img, op=OP_SOBEL):
        H, W = img.shape
        out = np.empty((H, W), np.uint8)
        self._chk(self.lib.compvhip_edge_dete_u8(self.h, _ptr(img), W, H, img.strides[0], op, _ptr(out), W))
        return out

    def grayscale(self, packed, pixfmt, W):
        """packed: (H, S*bpp) uint8 array, rows of S samples; returns the (H, W) luma plane (CompVImage::convertGrayscale)."""
        H = packed.shape[0]
        bpp = FMT_BYTES[pixfmt]
        S = packed.strides[0] // bpp
        out = np.empty((H, W), np.uint8)
        self._chk(self.lib.compvhip_grayscale_u8(self.h, _ptr(packed), pixfmt, W, H, S, _ptr(out), W))
        return out

    def convert(self, planes, pixfmt_in, pixfmt_out, W, H):
        """compvhip_convert_u8: planes -- the source's planes as 2-D uint8 arrays (rows contiguous, any row stride at or above the layout's minimum); returns
        the destination's dense planes, rows x minRowBytes each (convert_layout)."""
        n_in, _, _ = convert_layout(pixfmt_in, W, H)
        n_out, rb, rows = convert_layout(pixfmt_out, W, H)
        assert len(planes) == n_in and all(p.dtype == np.uint8 and p.ndim == 2 and p.strides[1] == 1 for p in planes)
        out = [np.empty((rows[p], rb[p]), np.uint8) for p in range(n_out)]
        src = Image(pixfmt_in, [p.ctypes.data for p in planes], [p.strides[0] for p in planes])
        dst = Image(pixfmt_out, [p.ctypes.data for p in out], [p.strides[0] for p in out])
        self._chk(self.lib.compvhip_convert_u8(self.h, W, H, C.byref(src), C.byref(dst)))
        return out

    def convert_frames(self, W, H, frames, src, dst, stream=0):
        """compvhip_convert_frames on device memory: src, dst -- Image descriptions of `frames` images; asynchronous on `stream`"""
        self._chk(self.lib.compvhip_convert_frames(self.h, W, H, frames, C.byref(src), C.byref(dst), stream))

    def convlt_fixedpoint(self, img, vt, hz):
        """CompVMathConvlt::convlt1FixedPoint (vt/hz: uint16 Q16 weights)."""
        H, W = img.shape
        vt = np.ascontiguousarray(vt, np.uint16); hz = np.ascontiguousarray(hz, np.uint16)
        out = np.empty((H, W), np.uint8)
        self._chk(self.lib.compvhip_convlt1_fixedpoint_u8(self.h, _ptr(img), W, H, img.strides[0], _ptr(vt), _ptr(hz), len(vt), _ptr(out), W))
        return out

    def convlt1_i16(self, img, vt, hz):
        """CompVMathConvlt::convlt1<u8|s16, s16, s16>: separable integer correlation, int16 out (img: uint8 or int16, C-contiguous rows)."""
        H, W = img.shape
        vt = np.ascontiguousarray(vt, np.int16); hz = np.ascontiguousarray(hz, np.int16)
        assert len(vt) == len(hz)
        out = np.zeros((H, W), np.int16)
        fn = self.lib.compvhip_convlt1_8u16s16s if img.dtype == np.uint8 else self.lib.compvhip_convlt1_16s16s16s
        assert img.dtype in (np.uint8, np.int16)
        self._chk(fn(self.h, _ptr(img), W, H, img.strides[0] // img.itemsize, _ptr(vt), _ptr(hz), len(vt), _ptr(out), W))
        return out

    def otsu(self, img):
        """CompVImage::thresholdOtsu: the Otsu level (a double holding an integer, like the reference)."""
        H, W = img.shape
        t = C.c_double(0)
        self._chk(self.lib.compvhip_otsu_u8(self.h, _ptr(img), W, H, img.strides[0], C.byref(t)))
        return t.value

    def canny(self, img, tLow, tHigh, ksize=3, threshold_type=THRESHOLD_COMPARE_TO_GRADIENT, out=None):
        H, W = img.shape
        if out is None:
            out = np.empty((H, W), np.uint8)
        self._chk(self.lib.compvhip_canny_u8(self.h, _ptr(img), W, H, img.strides[0], tLow, tHigh, ksize, threshold_type,
                                             _ptr(out), out.strides[0]))
        return out

    def houghsht_dims(self, W, H, theta_deg=1.0):
        R, T, st = C.c_size_t(), C.c_size_t(), C.c_float()
        rc = self.lib.compvhip_houghsht_dims(W, H, theta_deg, C.byref(R), C.byref(T), C.byref(st))
        self._chk(rc)
        return R.value, T.value, st.value

    def houghsht(self, edges, theta_deg=1.0, threshold=100, max_lines=0, rho=1.0, cap=1 << 16, want_acc=False):
        H, W = edges.shape
        lines = np.zeros(cap, LINE_DTYPE)
        n = C.c_size_t(0)
        acc = None
        accp, accs = None, 0
        if want_acc:
            R, T, _ = self.houghsht_dims(W, H, theta_deg)
            acc = np.zeros((R, T), np.int32)
            accp, accs = _ptr(acc), T
        rc = self.lib.compvhip_houghsht_u8(self.h, _ptr(edges), W, H, edges.strides[0], rho, theta_deg, threshold, max_lines,
                                           _ptr(lines), cap, C.byref(n), accp, accs)
        if rc == E_OUT_OF_BOUND and n.value > cap:
            return self.houghsht(edges, theta_deg, threshold, max_lines, rho, cap=n.value, want_acc=want_acc)
        self._chk(rc)
        lines = lines[:n.value]
        return (lines, acc) if want_acc else lines

    def houghsht_segments(self, edges, lines, theta_deg=1.0, min_length=1, max_gap=0, cap=1 << 12):
        """compvhip_houghsht_segments_u8: the segments (SEGMENT_DTYPE array) of caller-held SHT lines (a LINE_DTYPE array, e.g. what houghsht()
        returned for the same edge map and theta_deg; only row / col are read) -- where along each line its edge pixels are."""
        H, W = edges.shape
        lines = np.ascontiguousarray(lines, LINE_DTYPE)
        segs = np.zeros(max(cap, 1), SEGMENT_DTYPE)
        n = C.c_size_t(0)
        rc = self.lib.compvhip_houghsht_segments_u8(self.h, _ptr(edges), W, H, edges.strides[0], theta_deg, _ptr(lines), len(lines), min_length, max_gap,
                                                    _ptr(segs), cap, C.byref(n))
        if rc == E_OUT_OF_BOUND and n.value > cap:
            return self.houghsht_segments(edges, lines, theta_deg, min_length, max_gap, cap=n.value)
        self._chk(rc)
        return segs[:n.value]

    def houghsht_fit(self, edges, lines, theta_deg=1.0, half_width=3, segs=None, want_refined=False):
        """compvhip_houghsht_fit_u8: the least-squares fits (LINE_FIT_DTYPE array) through the edge pixels within half_width rho cells of
        caller-held SHT lines (a LINE_DTYPE array; only row / col are read) -- one record per line, or per segment of segs (a SEGMENT_DTYPE
        array of those lines).  want_refined (per line only): returns (fits, lines with the fitted rho / theta)."""
        H, W = edges.shape
        lines = np.ascontiguousarray(lines, LINE_DTYPE)
        if segs is not None:
            segs = np.ascontiguousarray(segs, SEGMENT_DTYPE)
        cap = len(lines) if segs is None else len(segs)
        fits = np.zeros(max(cap, 1), LINE_FIT_DTYPE)
        refined = np.zeros(max(len(lines), 1), LINE_DTYPE) if want_refined else None
        n = C.c_size_t(0)
        self._chk(self.lib.compvhip_houghsht_fit_u8(self.h, _ptr(edges), W, H, edges.strides[0], theta_deg, _ptr(lines), len(lines), half_width,
                                                    None if segs is None else _ptr(segs), 0 if segs is None else len(segs), _ptr(fits), cap, C.byref(n),
                                                    _ptr(refined) if want_refined else None))
        return (fits[:n.value], refined[:len(lines)]) if want_refined else fits[:n.value]

    def components(self, edges, connectivity=8, min_pixels=1, want_labels=True, cap=1 << 12):
        """compvhip_components_u8: (labels, records) of one edge map -- the int32 label map (None without want_labels) and the COMP_DTYPE
        array of the components with at least min_pixels pixels, in ascending order of their root's raster index."""
        H, W = edges.shape
        labels = np.zeros((H, W), np.int32) if want_labels else None
        comps = np.zeros(max(cap, 1), COMP_DTYPE)
        n = C.c_size_t(0)
        rc = self.lib.compvhip_components_u8(self.h, _ptr(edges), W, H, edges.strides[0], connectivity, min_pixels,
                                             _ptr(labels) if want_labels else None, W, _ptr(comps), cap, C.byref(n))
        if rc == E_OUT_OF_BOUND and n.value > cap:
            return self.components(edges, connectivity, min_pixels, want_labels, cap=n.value)
        self._chk(rc)
        return labels, comps[:n.value]

    def threshold(self, img, threshold):
        """compvhip_threshold_u8 (CompVImageThreshold::global): img > round(clip(threshold)) ? 255 : 0."""
        H, W = img.shape
        out = np.empty((H, W), np.uint8)
        self._chk(self.lib.compvhip_threshold_u8(self.h, _ptr(img), W, H, img.strides[0], threshold, _ptr(out), W))
        return out

    def threshold_adaptive(self, img, block_size, delta, max_val=255.0, invert=False):
        """compvhip_threshold_adaptive_u8 (CompVImageThreshold::adaptive with the Q16 mean kernel)."""
        H, W = img.shape
        out = np.empty((H, W), np.uint8)
        self._chk(self.lib.compvhip_threshold_adaptive_u8(self.h, _ptr(img), W, H, img.strides[0], block_size, delta, max_val, int(bool(invert)), _ptr(out), W))
        return out

    def morph(self, img, strel, op, border=BORDER_REPLICATE):
        """compvhip_morph_u8 (CompVMathMorph::process): strel is a 2-D uint8 array, non-zero = member."""
        H, W = img.shape
        strel = np.ascontiguousarray(strel, np.uint8)
        out = np.empty((H, W), np.uint8)
        self._chk(self.lib.compvhip_morph_u8(self.h, _ptr(img), W, H, img.strides[0], _ptr(strel), strel.shape[1], strel.shape[0], op, border, _ptr(out), W))
        return out

    def fast(self, img, threshold=20, fast_type=9, nonmax=True, max_features=-1, want_scores=False, cap=4096):
        """compvhip_fast_u8 (CompVCornerDeteFAST::process): -> corners (CORNER_DTYPE, raster order) [, score map].  The call is repeated with a
        larger buffer when `cap` was too small."""
        H, W = img.shape
        scores = np.empty((H, W), np.uint8) if want_scores else None
        n = C.c_size_t(0)
        while True:
            rec = np.zeros(cap, CORNER_DTYPE)
            rc = self.lib.compvhip_fast_u8(self.h, _ptr(img), W, H, img.strides[0], threshold, fast_type, int(bool(nonmax)), max_features,
                                           _ptr(scores) if want_scores else None, W, _ptr(rec) if cap else None, cap, C.byref(n))
            if rc != E_OUT_OF_BOUND:
                break
            cap = n.value
        self._chk(rc)
        return (rec[:n.value], scores) if want_scores else rec[:n.value]

    def orb(self, img, corners, level=0, scale=1.0):
        """compvhip_orb_u8: corners (CORNER_DTYPE, e.g. fast()'s) of one pyramid level -> (keypoints KEYPOINT_DTYPE, descriptors (n, 32) uint8): the corners
        18 pixels from every border, in their order, with the intensity-centroid orientation, and their rotated BRIEF-256/31 rows."""
        H, W = img.shape
        corners = np.ascontiguousarray(corners, CORNER_DTYPE)
        n = len(corners)
        keys = np.zeros(n, KEYPOINT_DTYPE)
        desc = np.zeros((n, 32), np.uint8)
        kept = C.c_size_t(0)
        self._chk(self.lib.compvhip_orb_u8(self.h, _ptr(img), W, H, img.strides[0], _ptr(corners) if n else None, n, level, scale, _ptr(keys) if n else None,
                                           _ptr(desc) if n else None, 32, C.byref(kept)))
        return keys[:kept.value], desc[:kept.value]

    def hog(self, img, opts=None, **kw):
        """compvhip_hog_u8 (CompVHOG, COMPV_HOGS_ID): the float32 descriptor of one gray frame; opts: a HogOpts, or its keywords (block=16, stride=8, cell=8,
        nbins=9, norm="l2hys", signed=True, interp="bilinear")"""
        H, W = img.shape
        o = _hog_opts(opts, kw)
        desc = np.zeros(hog_geometry(W, H, o)["descLen"], np.float32)
        n = C.c_size_t(0)
        self._chk(self.lib.compvhip_hog_u8(self.h, _ptr(img), W, H, img.strides[0], C.byref(o), _ptr(desc), desc.size, C.byref(n)))
        return desc[:n.value]

    def integral(self, img, want_sum=True, want_sumsq=True, sum_stride=None):
        """compvhip_integral_u8 (CompVImage::integral): -> (sum, sumsq), float64 (H + 1, W + 1) views of rows of sum_stride elements; None for one not wanted"""
        H, W = img.shape
        stride = W + 1 if sum_stride is None else sum_stride
        s = np.zeros((H + 1, stride), np.float64) if want_sum else None
        q = np.zeros((H + 1, stride), np.float64) if want_sumsq else None
        self._chk(self.lib.compvhip_integral_u8(self.h, _ptr(img), W, H, img.strides[0], _ptr(s) if want_sum else None, _ptr(q) if want_sumsq else None, stride))
        return (s[:, :W + 1] if want_sum else None), (q[:, :W + 1] if want_sumsq else None)

    def histogram(self, img):
        """compvhip_histogram_u8 (CompVImage::histogramBuild): -> uint32[256]"""
        H, W = img.shape
        hist = np.zeros(256, np.uint32)
        self._chk(self.lib.compvhip_histogram_u8(self.h, _ptr(img), W, H, img.strides[0], _ptr(hist)))
        return hist

    def equalize(self, img, hist=None, scale=0.0, out_stride=None):
        """compvhip_equalize_u8 (CompVImage::histogramEqualiz): -> (out, lut); hist: None (the frame's own) or uint32[256]; scale <= 0: 255 / (W * H)"""
        H, W = img.shape
        So = W if out_stride is None else out_stride
        out = np.zeros((H, So), np.uint8)
        lut = np.zeros(256, np.uint8)
        if hist is not None:
            hist = np.ascontiguousarray(hist, np.uint32)
            assert hist.size == 256
        self._chk(self.lib.compvhip_equalize_u8(self.h, _ptr(img), W, H, img.strides[0], _ptr(hist) if hist is not None else None, float(scale), _ptr(out), So, _ptr(lut)))
        return out[:, :W], lut

    def projections(self, img, want_x=True, want_y=True):
        """compvhip_projections_u8 (CompVImage::histogramBuildProjectionX / Y): -> (projX int32[W], projY int32[H]); None for one not wanted"""
        H, W = img.shape
        px = np.zeros(W, np.int32) if want_x else None
        py = np.zeros(H, np.int32) if want_y else None
        self._chk(self.lib.compvhip_projections_u8(self.h, _ptr(img), W, H, img.strides[0], _ptr(px) if want_x else None, _ptr(py) if want_y else None))
        return px, py

    def scale(self, img, out_w, out_h):
        """compvhip_scale_u8 (CompVImage::scale, bilinear): -> the (out_h, out_w) plane"""
        H, W = img.shape
        out = np.empty((out_h, out_w), np.uint8)
        self._chk(self.lib.compvhip_scale_u8(self.h, _ptr(img), W, H, img.strides[0], _ptr(out), out_w, out_h, out_w))
        return out

    def remap(self, img, map_x, map_y, interp=INTERP_BILINEAR, roi=None, default=0):
        """compvhip_remap_u8 (CompVImageRemap::process): map_x, map_y (out_h, out_w) float32 -> the (out_h, out_w) plane, uint8 or (INTERP_BILINEAR_FLOAT32,
        INTERP_BICUBIC_FLOAT32) float32.  interp: INTERP_NEAREST, _BILINEAR, _BICUBIC or one of the two _FLOAT32 forms.  roi: None, a Roi or (left, right, top, bottom)."""
        H, W = img.shape
        map_x, map_y = np.ascontiguousarray(map_x, np.float32), np.ascontiguousarray(map_y, np.float32)
        assert map_x.ndim == 2 and map_x.shape == map_y.shape
        out_h, out_w = map_x.shape
        out = np.empty((out_h, out_w), np.float32 if interp in (INTERP_BILINEAR_FLOAT32, INTERP_BICUBIC_FLOAT32) else np.uint8)
        self._chk(self.lib.compvhip_remap_u8(self.h, _ptr(img), W, H, img.strides[0], _ptr(map_x), _ptr(map_y), interp, _roi(roi), default, _ptr(out), out_w, out_h, out_w))
        return out

    def warp_inverse(self, img, M, out_w, out_h, interp=INTERP_BILINEAR, default=0):
        """compvhip_warp_inverse_u8 (CompVImage::warpInverse): M (2, 3) or (3, 3) float32, destination to source -> the (out_h, out_w) plane, uint8 or
        (INTERP_BILINEAR_FLOAT32, INTERP_BICUBIC_FLOAT32) float32"""
        H, W = img.shape
        M = np.ascontiguousarray(M, np.float32)
        assert M.ndim == 2 and M.shape[1] == 3
        out = np.empty((out_h, out_w), np.float32 if interp in (INTERP_BILINEAR_FLOAT32, INTERP_BICUBIC_FLOAT32) else np.uint8)
        self._chk(self.lib.compvhip_warp_inverse_u8(self.h, _ptr(img), W, H, img.strides[0], _ptr(M), M.shape[0], interp, default, _ptr(out), out_w, out_h, out_w))
        return out

    def moments(self, img, weights=MOMENTS_VALUE):
        """compvhip_moments_host (CompVMathMoments::rawSecondOrder, skewness, orientation): one (H, W) uint8 plane from 1 x 1 on -> (raw, shape), one
        MOMENTS_DTYPE and one MOMENTS_SHAPE_DTYPE record"""
        H, W = img.shape
        raw, shape = np.zeros(1, MOMENTS_DTYPE), np.zeros(1, MOMENTS_SHAPE_DTYPE)
        desc = MomentsDesc(weights)
        self._chk(self.lib.compvhip_moments_host(self.h, C.byref(desc), _ptr(img), W, H, img.strides[0], _ptr(raw), _ptr(shape)))
        return raw[0], shape[0]

    # ---- image moments on device memory (stateless on the context; asynchronous on `stream`) ----
    def moments_frames(self, d_gray, W, H, S, frames, d_raw, d_shape=0, weights=MOMENTS_VALUE, stream=0):
        """compvhip_moments_frames: d_gray [frames][H][S] -> d_raw [frames] (and d_shape [frames]) records"""
        desc = MomentsDesc(weights, MOMENTS_ORIGIN_FRAME, stream)
        self._chk(self.lib.compvhip_moments_frames(self.h, C.byref(desc), d_gray or None, W, H, S, frames, d_raw or None, d_shape or None))

    def moments_components(self, d_labels, W, H, label_stride, d_comps, comp_cap, d_counts, frames, d_raw, d_shape=0, d_gray=0, S=0, weights=MOMENTS_VALUE,
                           origin=MOMENTS_ORIGIN_FRAME, stream=0):
        """compvhip_moments_components: the label map, records and counts of compvhip_plan_components (and optional gray planes [frames][H][S]) -> d_raw (and
        d_shape) [frames][comp_cap]; records at and behind min(max(count, 0), comp_cap) are not written"""
        desc = MomentsDesc(weights, origin, stream)
        self._chk(self.lib.compvhip_moments_components(self.h, C.byref(desc), d_labels or None, W, H, label_stride, d_gray or None, S, d_comps or None, comp_cap,
                                                       d_counts or None, frames, d_raw or None, d_shape or None))

    def moments_shapes(self, d_raw, n, d_shape, stream=0):
        """compvhip_moments_shapes: d_shape[k] of d_raw[k], k < n"""
        desc = MomentsDesc(stream=stream)
        self._chk(self.lib.compvhip_moments_shapes(self.h, C.byref(desc), d_raw or None, n, d_shape or None))

    # ---- PCA projection on device memory (stateless on the context; asynchronous on `stream`) ----
    def pca_project(self, model, d_in, n, in_stride, d_out, out_stride, centre=True, stream=0):
        """compvhip_pca_project: d_in [n][in_stride] float32 -> d_out [n][out_stride], with a PcaModel after to_device(); centre=False: the mean is not subtracted"""
        assert model.d_vectors is not None, "PcaModel.to_device() first"
        d_mean = model.d_mean.data_ptr() if centre and model.d_mean is not None else None
        desc = PcaDesc(stream)
        self._chk(self.lib.compvhip_pca_project(self.h, C.byref(desc), d_mean, model.d_vectors.data_ptr(), model.dim, model.dim, model.components, d_in or None, n, in_stride,
                                                d_out or None, out_stride))

    def pca_project_raw(self, d_mean, d_vectors, vec_stride, dim, components, d_in, n, in_stride, d_out, out_stride, stream=0):
        """compvhip_pca_project on raw device addresses (d_mean = 0: do not centre)"""
        desc = PcaDesc(stream)
        self._chk(self.lib.compvhip_pca_project(self.h, C.byref(desc), d_mean or None, d_vectors or None, vec_stride, dim, components, d_in or None, n, in_stride, d_out or None,
                                                out_stride))

    def mulabt(self, d_A, a_rows, a_stride, d_B, b_rows, b_stride, cols, d_R, r_stride, stream=0):
        """compvhip_mulabt_f32 (CompVMath::mulABt): d_R [a_rows][r_stride] = d_A [a_rows][a_stride] times the transpose of d_B [b_rows][b_stride], float32"""
        desc = PcaDesc(stream)
        self._chk(self.lib.compvhip_mulabt_f32(self.h, C.byref(desc), d_A or None, a_rows, a_stride, d_B or None, b_rows, b_stride, cols, d_R or None, r_stride))

    def pca_covariance(self, d_obs, n, obs_stride, dim, d_mean, d_covar, cov_stride, d_scratch, stream=0):
        """compvhip_pca_covariance: the mean [dim] and the covariance [dim][cov_stride] of n row-based observations; d_scratch: pca_covariance_scratch(n, dim) bytes"""
        desc = PcaDesc(stream)
        self._chk(self.lib.compvhip_pca_covariance(self.h, C.byref(desc), d_obs or None, n, obs_stride, dim, d_mean or None, d_covar or None, cov_stride, d_scratch or None))

    def pca_project_host(self, model, rows, centre=True):
        """compvhip_pca_project_host: (n, dim) float32 host rows -> (n, components); the model's host arrays are used"""
        rows = np.asarray(rows, np.float32)
        assert rows.ndim == 2 and rows.shape[1] == model.dim and rows.strides[1] == 4 and rows.strides[0] % 4 == 0
        out = np.zeros((rows.shape[0], model.components), np.float32)
        desc = PcaDesc()
        mean = _ptr(model.mean) if centre and model.mean is not None else None
        self._chk(self.lib.compvhip_pca_project_host(self.h, C.byref(desc), mean, _ptr(model.vectors), model.dim, model.dim, model.components, _ptr(rows) if rows.size else None,
                                                     rows.shape[0], rows.strides[0] // 4 if rows.shape[0] > 1 else model.dim, _ptr(out) if out.size else None, model.components))
        return out

    def undistort(self, img, K, d, out_w=None, out_h=None, x0=0, y0=0, interp=INTERP_BILINEAR, roi=None, default=0):
        """compvhip_undistort_u8 (CompVCalibUtils::undist2DImage): one camera K (3, 3), d (2 .. 4) float32 -> the (out_h, out_w) window at origin (x0, y0) of the
        undistorted frame, uint8 or (the two _FLOAT32 interpolations) float32.  out_w, out_h default to the image's."""
        H, W = img.shape
        out_w, out_h = W if out_w is None else out_w, H if out_h is None else out_h
        K, d = np.ascontiguousarray(K, np.float32), np.ascontiguousarray(d, np.float32).ravel()
        assert K.shape == (3, 3)
        out = np.empty((out_h, out_w), np.float32 if interp in (INTERP_BILINEAR_FLOAT32, INTERP_BICUBIC_FLOAT32) else np.uint8)
        self._chk(self.lib.compvhip_undistort_u8(self.h, _ptr(img), W, H, img.strides[0], _ptr(K), _ptr(d), d.size, x0, y0, interp, _roi(roi), default, _ptr(out),
                                                 out_w, out_h, out_w))
        return out

    def orb_pyramid(self, img, opts=None, cap=4096):
        """compvhip_orb_pyramid_u8 (CompVCornerDeteORB::process + CompVCornerDescORB::process): -> (keypoints KEYPOINT_DTYPE in level order, descriptors
        (n, 32) uint8).  opts: OrbPyramidOpts or None for the defaults.  The call is repeated with a larger buffer when `cap` was too small."""
        H, W = img.shape
        n = C.c_size_t(0)
        while True:
            keys = np.zeros(cap, KEYPOINT_DTYPE)
            desc = np.zeros((cap, 32), np.uint8)
            rc = self.lib.compvhip_orb_pyramid_u8(self.h, _ptr(img), W, H, img.strides[0], C.byref(opts) if opts is not None else None, _ptr(keys) if cap else None,
                                                  _ptr(desc) if cap else None, 32, cap, C.byref(n))
            if rc != E_OUT_OF_BOUND:
                break
            cap = n.value
        self._chk(rc)
        return keys[:n.value], desc[:n.value]

    def match_hamming(self, query, train, knn=2):
        """compvhip_match_hamming_u8 (CompVMatcherBruteForce::process): query (Q, cols) and train (T, cols) uint8 rows -> (min(knn, T), Q) MATCH_DTYPE
        records, neighbour r of query q at [r, q], distances ascending.  Among equal distances the records follow the REFERENCE's insertion order
        (tests/match_model.py: knn_reference; docs/kernels/match.md), not the (distance, train index) order of Matcher.knn: on ties the two calls
        return different train indices, never different distances."""
        assert query.dtype == np.uint8 and train.dtype == np.uint8 and query.ndim == 2 and train.ndim == 2 and query.shape[1] == train.shape[1]
        assert query.strides[1] == 1 and train.strides[1] == 1
        Q, cols = query.shape
        T = train.shape[0]
        out = np.zeros((max(knn, 1), max(Q, 1)), MATCH_DTYPE)
        rows = C.c_size_t(0)
        self._chk(self.lib.compvhip_match_hamming_u8(self.h, _ptr(query), Q, query.strides[0], _ptr(train), T, train.strides[0], cols, knn, _ptr(out), out.shape[1],
                                                     C.byref(rows)))
        return out[:rows.value, :Q]

    def homography_find(self, src, dst, tries=2000, threshold=30.0, seed=0, quads=None, want_mask=True):
        """compvhip_homography_find_f64 (CompVHomography<double>::find, every try run): src, dst (n, 2) float64 correspondences src -> dst ->
        (HOMOGRAPHY_RESULT_DTYPE scalar, uint8 inlier mask of n or None).  quads: None or int32 (tries, 4), replacing the generator."""
        src, dst = np.ascontiguousarray(src, np.float64).reshape(-1, 2), np.ascontiguousarray(dst, np.float64).reshape(-1, 2)
        assert src.shape == dst.shape
        n = len(src)
        o = HomographyOpts(tries, seed, threshold)
        q = None if quads is None else np.ascontiguousarray(quads, np.int32).reshape(tries, 4)
        res = np.zeros(1, HOMOGRAPHY_RESULT_DTYPE)
        mask = np.zeros(max(n, 1), np.uint8) if want_mask else None
        self._chk(self.lib.compvhip_homography_find_f64(self.h, _ptr(src) if n else None, _ptr(dst) if n else None, n, C.byref(o), _ptr(q) if q is not None else None,
                                                        _ptr(res), _ptr(mask) if want_mask else None))
        return res[0], (mask[:n] if want_mask else None)

    def _curvefit(self, model, points, threshold, tries, seed, samples, want_mask):
        points = np.ascontiguousarray(points, np.float64).reshape(-1, 2)
        n = len(points)
        o = CurvefitOpts(model, tries, seed, threshold)
        q = None if samples is None else np.ascontiguousarray(samples, np.int32).reshape(tries, curvefit_model_points(model))
        res = np.zeros(1, CURVEFIT_RESULT_DTYPE)
        mask = np.zeros(max(n, 1), np.uint8) if want_mask else None
        self._chk(self.lib.compvhip_curvefit_find_f64(self.h, _ptr(points) if n else None, n, C.byref(o), _ptr(q) if q is not None else None, _ptr(res),
                                                      _ptr(mask) if want_mask else None))
        return res[0], (mask[:n] if want_mask else None)

    def fit_line(self, points, threshold=1.0, tries=2000, seed=0, samples=None, want_mask=True):
        """compvhip_curvefit_find_f64 with the LINE model (CompVMathStatsFit::line, every try run): points (n, 2) float64 ->
        (CURVEFIT_RESULT_DTYPE scalar with Ax + By + C = 0, uint8 inlier mask of n or None).  samples: None or int32 (tries, 2), replacing the generator."""
        return self._curvefit(CURVEFIT_LINE, points, threshold, tries, seed, samples, want_mask)

    def fit_parabola(self, points, threshold=1.0, tries=2000, seed=0, sideways=False, samples=None, want_mask=True):
        """compvhip_curvefit_find_f64 with a PARABOLA model (CompVMathStatsFit::parabola): y = Ax^2 + Bx + C, or x = Ay^2 + By + C with sideways.
        samples: None or int32 (tries, 3)."""
        return self._curvefit(CURVEFIT_PARABOLA_SIDEWAYS if sideways else CURVEFIT_PARABOLA, points, threshold, tries, seed, samples, want_mask)

    def houghkht(self, edges, rho=1.0, theta_deg=1.0, threshold=1, max_lines=0, min_dev=2.0, min_size=10, min_height=0.002, cap=1 << 14, order="reference"):
        """Returns (lines, GS); lines['row'] / ['col'] hold the rho / theta indices.  order: "reference" (compvhip_houghkht_u8: the reference's tie
        order) or "canonical" (compvhip_houghkht_ex_u8: count descending, ties by emission key, peaks found and sorted on the GPU)."""
        H, W = edges.shape
        o = _kht_order(order)
        lines = np.zeros(cap, LINE_DTYPE)
        n = C.c_size_t(0)
        gs = C.c_double(1.0)
        if o == KHT_ORDER_REFERENCE:
            rc = self.lib.compvhip_houghkht_u8(self.h, _ptr(edges), W, H, edges.strides[0], rho, theta_deg, threshold, max_lines, min_dev, min_size,
                                               min_height, _ptr(lines), cap, C.byref(n), C.byref(gs))
        else:
            opts = KhtOpts(rho, theta_deg, threshold, max_lines, min_dev, min_size, min_height, 0, o)
            rc = self.lib.compvhip_houghkht_ex_u8(self.h, _ptr(edges), W, H, edges.strides[0], C.byref(opts), _ptr(lines), cap, C.byref(n), C.byref(gs))
        if rc == E_OUT_OF_BOUND and n.value > cap:
            return self.houghkht(edges, rho, theta_deg, threshold, max_lines, min_dev, min_size, min_height, cap=n.value, order=order)
        self._chk(rc)
        return lines[:n.value], gs.value


    def houghkht_kernels(self, edges, min_dev=2.0, min_size=10, cap=1 << 16):
        """Stage inspection: (kernels[n, 7] float64 in CompVHoughKhtKernel field order, before the height pruning; hmax)."""
        H, W = edges.shape
        out = np.zeros((cap, 7), np.float64)
        n = C.c_size_t(0)
        hmax = C.c_double(0.0)
        rc = self.lib.compvhip_houghkht_kernels_u8(self.h, _ptr(edges), W, H, edges.strides[0], min_dev, min_size, _ptr(out), cap, C.byref(n), C.byref(hmax))
        if rc == E_OUT_OF_BOUND and n.value > cap:
            return self.houghkht_kernels(edges, min_dev, min_size, cap=n.value)
        self._chk(rc)
        return out[:n.value], hmax.value

    def houghkht_stage_ms(self):
        """Milliseconds of the six stages of the last houghkht() call: link, subdivide, statistics, prune, vote + peaks, sort + sweep."""
        ms = np.zeros(6, np.float64)
        self._chk(self.lib.compvhip_houghkht_stage_ms(self.h, _ptr(ms)))
        return ms


class Plan:
    """Batched device-resident pipeline (compvhip_plan). Pointers are raw device addresses (e.g. torch .data_ptr())."""

    def __init__(self, ctx, W, H, S, frames, theta_deg=1.0):
        self.ctx = ctx
        self.lib = ctx.lib
        h = C.c_void_p()
        ctx._chk(self.lib.compvhip_plan_create(ctx.h, W, H, S, frames, theta_deg, C.byref(h)))
        self.h = h
        self.W, self.H, self.S, self.frames = W, H, S, frames
        self.timing_mode = 0

    def close(self):
        if self.h:
            self.lib.compvhip_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def canny(self, d_in, tLow, tHigh, d_edges, ksize=3, threshold_type=THRESHOLD_COMPARE_TO_GRADIENT, stream=0):
        self.ctx._chk(self.lib.compvhip_plan_canny(self.h, d_in, tLow, tHigh, ksize, threshold_type, d_edges, stream))

    def edge_dete(self, d_in, op, d_out, stream=0):
        self.ctx._chk(self.lib.compvhip_plan_edge_dete(self.h, d_in, op, d_out, stream))

    def grayscale(self, d_in, pixfmt, d_gray, stream=0):
        self.ctx._chk(self.lib.compvhip_plan_grayscale(self.h, d_in, pixfmt, d_gray, stream))

    def convlt_fixedpoint(self, d_in, vt, hz, d_out, stream=0):
        vt = np.ascontiguousarray(vt, np.uint16); hz = np.ascontiguousarray(hz, np.uint16)
        self.ctx._chk(self.lib.compvhip_plan_convlt1_fixedpoint(self.h, d_in, _ptr(vt), _ptr(hz), len(vt), d_out, stream))

    def to_cartesian(self, d_lines, d_counts, line_cap, d_cart, stream=0):
        self.ctx._chk(self.lib.compvhip_plan_to_cartesian(self.h, d_lines, d_counts, line_cap, d_cart, stream))

    def otsu(self, d_gray, d_thresholds, stream=0):
        self.ctx._chk(self.lib.compvhip_plan_otsu(self.h, d_gray, d_thresholds, stream))

    def houghsht(self, d_edges, threshold, max_lines, d_lines, line_cap, d_counts, stream=0):
        self.ctx._chk(self.lib.compvhip_plan_houghsht(self.h, d_edges, threshold, max_lines, d_lines, line_cap, d_counts, stream))

    def houghsht_segments(self, d_edges, d_lines, d_counts, line_cap, max_lines, min_length, max_gap, d_segs, seg_cap, d_seg_counts, stream=0):
        """compvhip_plan_houghsht_segments: segments of the device line arrays of houghsht() / pipeline(); d_edges = 0 reads the 1-bit masks of
        the plan's last Canny.  d_segs: frames * seg_cap Segment records, d_seg_counts: frames int32 (found, before clipping)."""
        self.ctx._chk(self.lib.compvhip_plan_houghsht_segments(self.h, d_edges or None, d_lines, d_counts, line_cap, max_lines, min_length, max_gap,
                                                               d_segs, seg_cap, d_seg_counts, stream))

    def houghsht_fit(self, d_edges, d_lines, d_counts, line_cap, max_lines, half_width, d_segs, d_seg_counts, seg_cap, d_fits, fit_cap, d_fit_counts,
                     d_refined=0, stream=0):
        """compvhip_plan_houghsht_fit: least-squares fits of the device line arrays of houghsht() / pipeline(), per line (d_segs = 0) or per
        segment of houghsht_segments(); d_edges = 0 reads the 1-bit masks of the plan's last Canny.  d_fits: frames * fit_cap LineFit
        records, d_fit_counts: frames int32 (records, before clipping), d_refined: 0 or frames * line_cap Line records."""
        self.ctx._chk(self.lib.compvhip_plan_houghsht_fit(self.h, d_edges or None, d_lines, d_counts, line_cap, max_lines, half_width, d_segs or None,
                                                          d_seg_counts or None, seg_cap, d_fits or None, fit_cap, d_fit_counts, d_refined or None, stream))

    def components(self, d_edges, connectivity, min_pixels, d_labels, label_stride, d_comps, comp_cap, d_comp_counts, stream=0):
        """compvhip_plan_components: connected components of every frame; d_edges = 0 reads the 1-bit masks of the plan's last Canny.
        d_labels: frames * H * label_stride int32 (0: no label map), d_comps: frames * comp_cap Component records (0 with comp_cap 0:
        counts only), d_comp_counts: frames int32 (found, before clipping)."""
        self.ctx._chk(self.lib.compvhip_plan_components(self.h, d_edges or None, connectivity, min_pixels, d_labels or None, label_stride,
                                                        d_comps or None, comp_cap, d_comp_counts, stream))

    def threshold(self, d_in, threshold, d_out, d_levels=0, stream=0):
        """compvhip_plan_threshold: d_levels = 0 cuts every frame at `threshold`, otherwise frame f at d_levels[f] (what otsu() wrote)."""
        self.ctx._chk(self.lib.compvhip_plan_threshold(self.h, d_in, threshold, d_levels or None, d_out, stream))

    def threshold_adaptive(self, d_in, block_size, delta, max_val, invert, d_out, stream=0):
        self.ctx._chk(self.lib.compvhip_plan_threshold_adaptive(self.h, d_in, block_size, delta, max_val, int(bool(invert)), d_out, stream))

    def morph(self, d_in, strel, op, border, d_out, kernel=MORPH_KERNEL_AUTO, stream=0):
        """compvhip_plan_morph (kernel = MORPH_KERNEL_AUTO) / compvhip_plan_morph_ex: strel is a 2-D uint8 HOST array, non-zero = member."""
        strel = np.ascontiguousarray(strel, np.uint8)
        sh, sw = strel.shape
        if kernel == MORPH_KERNEL_AUTO:
            self.ctx._chk(self.lib.compvhip_plan_morph(self.h, d_in, _ptr(strel), sw, sh, op, border, d_out, stream))
        else:
            self.ctx._chk(self.lib.compvhip_plan_morph_ex(self.h, d_in, _ptr(strel), sw, sh, op, border, kernel, d_out, stream))

    def fast(self, d_gray, threshold, fast_type, nonmax, max_features, d_scores, d_corners, corner_cap, d_counts, stream=0):
        """compvhip_plan_fast: d_scores = 0 for no score map, d_corners = 0 with corner_cap = 0 for counts only."""
        self.ctx._chk(self.lib.compvhip_plan_fast(self.h, d_gray, threshold, fast_type, int(bool(nonmax)), max_features, d_scores or None,
                                                  d_corners or None, corner_cap, d_counts, stream))

    def orb_keypoints(self, d_gray, d_corners, corner_cap, d_corner_counts, level, scale, d_keypoints, key_cap, d_key_counts, d_moments=0, stream=0):
        """compvhip_plan_orb_keypoints: d_corners / d_corner_counts as fast() wrote them; d_moments = 0 or [frames][key_cap][2] int32 = {m01, m10}."""
        self.ctx._chk(self.lib.compvhip_plan_orb_keypoints(self.h, d_gray, d_corners or None, corner_cap, d_corner_counts or None, level, scale, d_keypoints or None,
                                                           key_cap, d_key_counts or None, d_moments or None, stream))

    def orb_describe(self, d_gray, d_keypoints, key_cap, d_key_counts, scale, d_desc, desc_stride=32, blur=True, stream=0):
        """compvhip_plan_orb_describe: 32-byte rows at d_desc + (f * key_cap + q) * desc_stride; blur=False takes d_gray as already blurred."""
        self.ctx._chk(self.lib.compvhip_plan_orb_describe(self.h, d_gray, d_keypoints or None, key_cap, d_key_counts or None, scale, int(bool(blur)), d_desc or None,
                                                          desc_stride, stream))

    def hog(self, d_gray, d_desc, desc_stride, d_cells=0, opts=None, stream=0, **kw):
        """compvhip_plan_hog: the plan's frames -> float32 descriptors [frames][desc_stride] (desc_stride >= hog_geometry()'s descLen, in floats) and, with d_cells,
        the cell map [frames][cellsY][cellsX][nbins]; opts: a HogOpts, or its keywords"""
        o = _hog_opts(opts, kw)
        self.ctx._chk(self.lib.compvhip_plan_hog(self.h, d_gray or None, C.byref(o), d_cells or None, d_desc or None, desc_stride, stream))

    def integral(self, d_gray, d_sum, d_sumsq, sum_stride, stream=0):
        """compvhip_plan_integral: the plan's frames -> float64 integral images [frames][H + 1][sum_stride] of the pixels (d_sum) and of their squares (d_sumsq);
        either may be 0, sum_stride >= W + 1 in elements"""
        self.ctx._chk(self.lib.compvhip_plan_integral(self.h, d_gray or None, d_sum or None, d_sumsq or None, sum_stride, stream))

    def histogram(self, d_gray, d_hist, stream=0):
        """compvhip_plan_histogram: the plan's frames -> uint32 [frames][256]"""
        self.ctx._chk(self.lib.compvhip_plan_histogram(self.h, d_gray or None, d_hist or None, stream))

    def equalize(self, d_gray, d_out, d_hist=0, scale=0.0, d_lut=0, stream=0):
        """compvhip_plan_equalize: d_out [frames][H][S] (may be d_gray) = lut[d_gray]; d_hist: 0 (each frame's own histogram) or uint32 [frames][256]; scale <= 0:
        255 / (W * H); d_lut: 0 or [frames][256] bytes"""
        self.ctx._chk(self.lib.compvhip_plan_equalize(self.h, d_gray or None, d_hist or None, float(scale), d_out or None, d_lut or None, stream))

    def projections(self, d_gray, d_proj_x, d_proj_y, stream=0):
        """compvhip_plan_projections: the plan's frames -> int32 column sums [frames][W] and row sums [frames][H]; either may be 0"""
        self.ctx._chk(self.lib.compvhip_plan_projections(self.h, d_gray or None, d_proj_x or None, d_proj_y or None, stream))

    def scale(self, d_in, d_out, out_w, out_h, out_stride, stream=0):
        """compvhip_plan_scale: the plan's frames [frames][H][S] -> d_out [frames][out_h][out_stride], bilinear"""
        self.ctx._chk(self.lib.compvhip_plan_scale(self.h, d_in or None, d_out or None, out_w, out_h, out_stride, stream))

    def remap(self, d_in, d_map_x, d_map_y, map_count, interp, d_out, out_w, out_h, out_stride, roi=None, default=0, stream=0):
        """compvhip_plan_remap: the plan's frames -> d_out [frames][out_h][out_stride] (uint8, or float32 with out_stride in elements) through the device maps
        [map_count][out_h * out_w] float32, map_count 1 (shared) or frames.  roi: None, a Roi or (left, right, top, bottom)."""
        self.ctx._chk(self.lib.compvhip_plan_remap(self.h, d_in or None, d_map_x or None, d_map_y or None, map_count, interp, _roi(roi), default, d_out or None,
                                                   out_w, out_h, out_stride, stream))

    def warp_inverse(self, d_in, M, interp, d_out, out_w, out_h, out_stride, default=0, stream=0):
        """compvhip_plan_warp_inverse: M is a HOST array (rows, 3) for all frames or (frames, rows, 3), rows 2 or 3, float32"""
        M = np.ascontiguousarray(M, np.float32)
        assert M.ndim in (2, 3) and M.shape[-1] == 3
        count = 1 if M.ndim == 2 else M.shape[0]
        self.ctx._chk(self.lib.compvhip_plan_warp_inverse(self.h, d_in or None, _ptr(M), M.shape[-2], count, interp, default, d_out or None, out_w, out_h, out_stride, stream))

    def pipeline(self, d_in, tLow, tHigh, threshold, max_lines, d_edges, d_lines, line_cap, d_counts, stream=0):
        self.ctx._chk(self.lib.compvhip_plan_pipeline(self.h, d_in, tLow, tHigh, threshold, max_lines, d_edges, d_lines, line_cap,
                                                      d_counts, stream))

    def pipeline_async(self, d_in, tLow, tHigh, threshold, max_lines, d_edges, d_lines, line_cap, d_counts, stream=0):
        """Enqueue one step without waiting for its hysteresis flag; returns the ticket for wait()."""
        t = C.c_int(-1)
        self.ctx._chk(self.lib.compvhip_plan_pipeline_async(self.h, d_in, tLow, tHigh, threshold, max_lines, d_edges, d_lines, line_cap,
                                                            d_counts, stream, C.byref(t)))
        return t.value

    def pipeline_ex(self, d_in, tLow, tHigh, threshold, max_lines, d_edges, d_lines, line_cap, d_counts, ksize=3,
                    threshold_type=THRESHOLD_COMPARE_TO_GRADIENT, pixfmt=FMT_Y, d_gray=0, d_otsu=0, d_cart=0, stream=0, asynchronous=False):
        """[grayscale ->] Canny (any kernel size / threshold mode) -> SHT [-> toCartesian] as one enqueue; returns the ticket when asynchronous."""
        o = PipelineOpts(tLow, tHigh, threshold, max_lines, ksize, threshold_type, pixfmt, d_gray or None, d_otsu or None, d_cart or None)
        t = C.c_int(-1)
        self.ctx._chk(self.lib.compvhip_plan_pipeline_ex(self.h, d_in, C.byref(o), d_edges, d_lines, line_cap, d_counts, stream,
                                                         C.byref(t) if asynchronous else None))
        return t.value if asynchronous else None

    def houghkht(self, d_edges, rho=1.0, theta_deg=1.0, threshold=1, max_lines=0, min_dev=2.0, min_size=10, min_height=0.002, cap=1 << 14, threads=0,
                 order="reference"):
        """CompVHoughKht::process on the plan's device edge maps; returns ([lines of frame f as a LINE_DTYPE array], [GS of frame f or None]).
        order: "reference" (compvhip_plan_houghkht) or "canonical" (compvhip_plan_houghkht_ex: peaks found and sorted on the GPU)."""
        F = self.frames
        o = _kht_order(order)
        lines = np.zeros((F, cap), LINE_DTYPE)
        counts = np.zeros(F, np.uint64)
        gs = np.full(F, np.nan, np.float64)
        if o == KHT_ORDER_REFERENCE:
            self.ctx._chk(self.lib.compvhip_plan_houghkht(self.h, d_edges, rho, theta_deg, threshold, max_lines, min_dev, min_size, min_height,
                                                          _ptr(lines), cap, _ptr(counts), _ptr(gs), threads))
        else:
            opts = KhtOpts(rho, theta_deg, threshold, max_lines, min_dev, min_size, min_height, threads, o)
            self.ctx._chk(self.lib.compvhip_plan_houghkht_ex(self.h, d_edges, C.byref(opts), _ptr(lines), cap, _ptr(counts), _ptr(gs)))
        return [lines[f][:int(counts[f])] for f in range(F)], [None if np.isnan(g) else float(g) for g in gs]

    def houghkht_stage_ms(self):
        ms = (C.c_double * 6)(); wall = C.c_double(0); th = C.c_int(0)
        self.ctx._chk(self.lib.compvhip_plan_houghkht_stage_ms(self.h, ms, C.byref(wall), C.byref(th)))
        names = ["link", "subdivide", "statistics", "prune_gmin", "vote_peaks", "sort_sweep"]
        F = max(1, self.frames)
        host = ms[0] + ms[3] + ms[5]
        return {"stages": {n: round(ms[i] / F, 4) for i, n in enumerate(names)}, "wall_ms": wall.value, "threads": th.value,
                "host_share": round(host / max(sum(ms), 1e-9), 3)}

    def wait(self, ticket):
        self.ctx._chk(self.lib.compvhip_plan_wait(self.h, ticket))

    def acc(self, frame):
        p, R, T, pitch = C.c_void_p(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        self.ctx._chk(self.lib.compvhip_plan_acc(self.h, frame, C.byref(p), C.byref(R), C.byref(T), C.byref(pitch)))
        return p.value, R.value, T.value, pitch.value

    def acc_export(self, frame, d_out, out_stride, stream=0):
        self.ctx._chk(self.lib.compvhip_plan_acc_export(self.h, frame, d_out, out_stride, stream))

    def edge_counts_ptr(self):
        p = C.c_void_p()
        self.ctx._chk(self.lib.compvhip_plan_edge_counts(self.h, C.byref(p)))
        return p.value

    def set_timing(self, mode=1):
        """0/False = off, 1/True = HIP events around every kernel, 2 = only around the two roofline kernels."""
        self.ctx._chk(self.lib.compvhip_plan_set_timing(self.h, int(mode)))
        self.timing_mode = int(mode)

    def get_timing(self, cap=256):
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        n = self.lib.compvhip_plan_get_timing(self.h, names, ms, cap)
        return [(names[i].decode(), ms[i]) for i in range(max(n, 0))]


class Matcher:
    """Batched device-resident brute-force Hamming matcher (compvhip_matcher).  Pointers are raw device addresses; 0 stands for NULL."""

    def __init__(self, ctx, desc_bytes, query_cap, train_cap, pairs=1, knn=2):
        self.ctx = ctx
        self.lib = ctx.lib
        h = C.c_void_p()
        ctx._chk(self.lib.compvhip_matcher_create(ctx.h, desc_bytes, query_cap, train_cap, pairs, knn, C.byref(h)))
        self.h = h
        self.desc_bytes, self.query_cap, self.train_cap, self.pairs, self.knn_rows = desc_bytes, query_cap, train_cap, pairs, knn

    def close(self):
        if self.h:
            self.lib.compvhip_matcher_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def knn(self, d_query, query_stride, d_query_counts, d_train, train_stride, d_train_counts, train_shared, d_matches, stream=0):
        """compvhip_matcher_knn: d_matches = [pairs][knn][query_cap] MATCH_DTYPE records; d_*_counts = 0: every pair is full."""
        self.ctx._chk(self.lib.compvhip_matcher_knn(self.h, d_query or None, query_stride, d_query_counts or None, d_train or None, train_stride,
                                                    d_train_counts or None, int(bool(train_shared)), d_matches or None, stream))

    def good(self, d_matches, d_query, query_stride, d_query_counts, d_train, train_stride, d_train_counts, train_shared, d_good, good_cap, d_good_counts,
             ratio=0.0, max_distance=-1, cross_check=False, stream=0):
        """compvhip_matcher_good: the good list of what knn() wrote; d_good = [pairs][good_cap] records (0 with good_cap 0: counts only)."""
        o = MatchOpts(ratio, max_distance, int(bool(cross_check)))
        self.ctx._chk(self.lib.compvhip_matcher_good(self.h, d_matches or None, d_query or None, query_stride, d_query_counts or None, d_train or None, train_stride,
                                                     d_train_counts or None, int(bool(train_shared)), C.byref(o), d_good or None, good_cap, d_good_counts or None, stream))

    def set_timing(self, mode=1):
        self.ctx._chk(self.lib.compvhip_matcher_set_timing(self.h, int(mode)))

    def get_timing(self, cap=16):
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        n = self.lib.compvhip_matcher_get_timing(self.h, names, ms, cap)
        return [(names[i].decode(), ms[i]) for i in range(max(n, 0))]


class Homography:
    """Batched device-resident RANSAC homography (compvhip_homography).  Pointers are raw device addresses; 0 stands for NULL."""

    def __init__(self, ctx, pairs, point_cap, max_tries=2000):
        self.ctx = ctx
        self.lib = ctx.lib
        h = C.c_void_p()
        ctx._chk(self.lib.compvhip_homography_create(ctx.h, pairs, point_cap, max_tries, C.byref(h)))
        self.h = h
        self.pairs, self.point_cap, self.max_tries = pairs, point_cap, max_tries

    def close(self):
        if self.h:
            self.lib.compvhip_homography_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def points(self, d_good, good_cap, d_good_counts, d_query, query_cap, d_train, train_cap, train_shared=False, stream=0):
        """compvhip_homography_points: gathers src = train positions, dst = query positions of the good records into the handle"""
        self.ctx._chk(self.lib.compvhip_homography_points(self.h, d_good or None, good_cap, d_good_counts or None, d_query or None, query_cap, d_train or None,
                                                          train_cap, int(bool(train_shared)), stream))

    def find(self, d_src, d_dst, d_counts, d_results, d_mask=0, tries=None, threshold=30.0, seed=0, d_quads=0, stream=0):
        """compvhip_homography_find: d_src = 0 takes the gathered points; d_results = [pairs] HOMOGRAPHY_RESULT_DTYPE records"""
        o = HomographyOpts(self.max_tries if tries is None else tries, seed, threshold)
        self.ctx._chk(self.lib.compvhip_homography_find(self.h, d_src or None, d_dst or None, d_counts or None, C.byref(o), d_quads or None, d_results or None,
                                                        d_mask or None, stream))

    def project(self, d_results, d_points, n, shared, d_out, stream=0):
        """compvhip_homography_project: n points ([pairs][n] or one shared set [n] of {x, y} float64) through every pair's H"""
        self.ctx._chk(self.lib.compvhip_homography_project(self.h, d_results or None, d_points or None, n, int(bool(shared)), d_out or None, stream))

    def scores(self, tries, stream=0):
        """compvhip_homography_scores (test hook): per pair and try the inlier count, variance and rotation count the last find() left -> three (pairs, tries) arrays"""
        counts, var, rot = np.zeros((self.pairs, tries), np.int32), np.zeros((self.pairs, tries), np.float64), np.zeros((self.pairs, tries), np.int32)
        self.ctx._chk(self.lib.compvhip_homography_scores(self.h, tries, _ptr(counts), _ptr(var), _ptr(rot), stream))
        return counts, var, rot

    def set_timing(self, mode=1):
        self.ctx._chk(self.lib.compvhip_homography_set_timing(self.h, int(mode)))

    def get_timing(self, cap=16):
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        n = self.lib.compvhip_homography_get_timing(self.h, names, ms, cap)
        return [(names[i].decode(), ms[i]) for i in range(max(n, 0))]


class Curvefit:
    """Batched device-resident RANSAC line / parabola fits (compvhip_curvefit).  Every call runs on the stream given here.  Pointers are raw device
    addresses; 0 stands for NULL."""

    def __init__(self, ctx, sets, point_cap, max_tries=2000, stream=0):
        self.ctx = ctx
        self.lib = ctx.lib
        h = C.c_void_p()
        d = CurvefitDesc(sets, point_cap, max_tries, stream)
        ctx._chk(self.lib.compvhip_curvefit_create(ctx.h, C.byref(d), C.byref(h)))
        self.h = h
        self.sets, self.point_cap, self.max_tries, self.stream = sets, point_cap, max_tries, stream

    def close(self):
        if self.h:
            self.lib.compvhip_curvefit_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def points_from_labels(self, d_labels, W, H, label_stride, d_comps, comp_cap, d_comp_counts, frames):
        """compvhip_curvefit_points_from_labels: every component of compvhip_plan_components' label maps becomes a point set of the handle"""
        self.ctx._chk(self.lib.compvhip_curvefit_points_from_labels(self.h, d_labels or None, W, H, label_stride, d_comps or None, comp_cap, d_comp_counts or None, frames))

    def find(self, d_points, d_counts, d_results, d_mask=0, model=CURVEFIT_LINE, tries=None, threshold=1.0, seed=0, d_samples=0):
        """compvhip_curvefit_find: d_points = 0 takes the gathered points; d_results = [sets] CURVEFIT_RESULT_DTYPE records"""
        o = CurvefitOpts(model, self.max_tries if tries is None else tries, seed, threshold)
        self.ctx._chk(self.lib.compvhip_curvefit_find(self.h, d_points or None, d_counts or None, C.byref(o), d_samples or None, d_results or None, d_mask or None))

    def distances(self, d_points, d_counts, model, d_params, d_out):
        """compvhip_curvefit_distances: the residual of every point under its set's {A, B, C}"""
        self.ctx._chk(self.lib.compvhip_curvefit_distances(self.h, d_points or None, d_counts or None, int(model), d_params or None, d_out or None))

    def scores(self, tries):
        """compvhip_curvefit_scores (test hook): (sets, tries) inlier counts of the last find(), (sets,) gathered point counts; waits for the stream"""
        counts, gathered = np.zeros((self.sets, tries), np.int32), np.zeros(self.sets, np.int32)
        self.ctx._chk(self.lib.compvhip_curvefit_scores(self.h, tries, _ptr(counts), _ptr(gathered)))
        return counts, gathered

    def gathered(self):
        """compvhip_curvefit_gathered: device addresses of the gathered points [sets][pointCap][2] float64 and of their counts [sets] int32"""
        p, c = C.c_void_p(), C.c_void_p()
        self.ctx._chk(self.lib.compvhip_curvefit_gathered(self.h, C.byref(p), C.byref(c)))
        return p.value, c.value

    def set_timing(self, mode=1):
        self.ctx._chk(self.lib.compvhip_curvefit_set_timing(self.h, int(mode)))

    def get_timing(self, cap=16):
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        n = self.lib.compvhip_curvefit_get_timing(self.h, names, ms, cap)
        return [(names[i].decode(), ms[i]) for i in range(max(n, 0))]


class Svm:
    """Batched device-resident C-SVC prediction (compvhip_svm): RBF and LINEAR.  Every call runs on the stream given here.  Pointers are raw device
    addresses; 0 stands for NULL."""

    def __init__(self, ctx, model_or_path, max_vectors, stream=0):
        self.ctx = ctx
        self.lib = ctx.lib
        h = C.c_void_p()
        d = SvmDesc(max_vectors, stream)
        if isinstance(model_or_path, SvmModel):
            m = model_or_path.struct()
            ctx._chk(self.lib.compvhip_svm_create(ctx.h, C.byref(m), C.byref(d), C.byref(h)))
        else:
            ctx._chk(self.lib.compvhip_svm_create_from_file(ctx.h, os.fsencode(model_or_path), C.byref(d), C.byref(h)))
        self.h = h
        self.max_vectors, self.stream = max_vectors, stream
        i = self.info()
        self.dim, self.l, self.pairs = i["dim"], i["totalSV"], i["pairs"]

    def close(self):
        if self.h:
            self.lib.compvhip_svm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """compvhip_svm_info: dict(kernel, nrClass, totalSV, dim, pairs, maxVectors, gamma)"""
        s = SvmShape()
        self.ctx._chk(self.lib.compvhip_svm_info(self.h, C.byref(s)))
        return {k: getattr(s, k) for k in ("kernel", "nrClass", "totalSV", "dim", "pairs", "maxVectors", "gamma")}

    def predict(self, d_vectors, vtype, n, stride, d_labels, d_dec=0, d_kvalues=0):
        """compvhip_svm_predict: d_vectors [n][stride] float32 (SVM_F32) or float64 (SVM_F64) -> d_labels [n] int32, d_dec [n][pairs], d_kvalues [n][totalSV]"""
        self.ctx._chk(self.lib.compvhip_svm_predict(self.h, d_vectors or None, int(vtype), n, stride, d_labels or None, d_dec or None, d_kvalues or None))

    def predict_host(self, vectors, want_dec=False):
        """compvhip_svm_predict_host: vectors (n, >= dim) float32 or float64 with contiguous rows -> int32 labels (n,) [, float64 decision values (n, pairs)]"""
        v = np.asarray(vectors)
        if v.dtype not in (np.float32, np.float64):
            v = v.astype(np.float64)
        if v.ndim != 2 or v.strides[1] != v.itemsize or v.strides[0] % v.itemsize:
            v = np.ascontiguousarray(v).reshape(len(v), -1)
        labels = np.zeros(len(v), np.int32)
        dec = np.zeros((len(v), self.pairs)) if want_dec else None
        self.ctx._chk(self.lib.compvhip_svm_predict_host(self.h, _ptr(v), SVM_F32 if v.dtype == np.float32 else SVM_F64, len(v), v.strides[0] // v.itemsize, _ptr(labels),
                                                         _ptr(dec) if want_dec else None))
        return (labels, dec) if want_dec else labels

    def set_timing(self, mode=1):
        self.ctx._chk(self.lib.compvhip_svm_set_timing(self.h, int(mode)))

    def get_timing(self, cap=16):
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        n = self.lib.compvhip_svm_get_timing(self.h, names, ms, cap)
        return [(names[i].decode(), ms[i]) for i in range(max(n, 0))]


class Undistort:
    """Batched device-resident lens undistortion (compvhip_undistort): the fused image form, maps, points and projection.  Every call runs on the stream
    given here.  Cameras (K, d) and poses are HOST arrays per call; pointers are raw device addresses, 0 stands for NULL."""

    def __init__(self, ctx, W, H, S, frames, out_w=None, out_h=None, x0=0, y0=0, max_sets=0, max_points=0, stream=0):
        self.ctx = ctx
        self.lib = ctx.lib
        out_w, out_h = W if out_w is None else out_w, H if out_h is None else out_h
        h = C.c_void_p()
        desc = UndistortDesc(W, H, S, frames, out_w, out_h, x0, y0, max_sets, max_points, stream)
        ctx._chk(self.lib.compvhip_undistort_create(ctx.h, C.byref(desc), C.byref(h)))
        self.h = h
        self.W, self.H, self.S, self.frames, self.out_w, self.out_h, self.x0, self.y0 = W, H, S, frames, out_w, out_h, x0, y0
        self.max_sets, self.max_points, self.stream = max_sets, max_points, stream

    def close(self):
        if self.h:
            self.lib.compvhip_undistort_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def undistort(self, d_in, K, d, interp, d_out, out_stride, roi=None, default=0):
        """compvhip_undistort_frames: d_in [frames][H][S] -> d_out [frames][out_h][out_stride] (uint8, or float32 with out_stride in elements); K (3, 3) with d (nd,)
        for all frames, or K (frames, 3, 3) with d (frames, nd), float32"""
        K, d, nd, count = _cameras(K, d, np.float32)
        self.ctx._chk(self.lib.compvhip_undistort_frames(self.h, d_in or None, _ptr(K), _ptr(d), nd, count, interp, _roi(roi), default, d_out or None, out_stride))

    def maps(self, K, d, d_map_x, d_map_y, mtype=UNDISTORT_F32):
        """compvhip_undistort_maps: d_map_x, d_map_y [count][out_h * out_w] float32 (UNDISTORT_F32) or float64 (UNDISTORT_F64); count 1 or frames"""
        K, d, nd, count = _cameras(K, d, np.float32 if mtype == UNDISTORT_F32 else np.float64)
        self.ctx._chk(self.lib.compvhip_undistort_maps(self.h, _ptr(K), _ptr(d), nd, count, int(mtype), d_map_x or None, d_map_y or None))

    def points(self, K, d, d_in, sets, n, d_out, ptype=UNDISTORT_F32, d_counts=0):
        """compvhip_undistort_points: d_in, d_out [sets][n] {x, y} of ptype; d_counts 0 or [sets] int32; one camera, or one per set"""
        K, d, nd, count = _cameras(K, d, np.float32 if ptype == UNDISTORT_F32 else np.float64)
        self.ctx._chk(self.lib.compvhip_undistort_points(self.h, _ptr(K), _ptr(d), nd, count, int(ptype), d_in or None, sets, n, d_counts or None, d_out or None))

    def project(self, K, d, Rt, d_in, sets, n, d_out, d_counts=0):
        """compvhip_undistort_project: d_in [sets][n] {x, y, z} -> d_out [sets][n] {u, v}, float64; Rt HOST (sets, 12): R row-major, then t"""
        K, d, nd, count = _cameras(K, d, np.float64)
        Rt = np.ascontiguousarray(Rt, np.float64)
        assert Rt.size == sets * 12
        self.ctx._chk(self.lib.compvhip_undistort_project(self.h, _ptr(K), _ptr(d), nd, count, _ptr(Rt), d_in or None, sets, n, d_counts or None, d_out or None))

    def set_timing(self, mode=1):
        self.ctx._chk(self.lib.compvhip_undistort_set_timing(self.h, int(mode)))

    def get_timing(self, cap=16):
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        n = self.lib.compvhip_undistort_get_timing(self.h, names, ms, cap)
        return [(names[i].decode(), ms[i]) for i in range(max(n, 0))]


class OrbPyramid:
    """Batched device-resident ORB scale pyramid (compvhip_orbpyr): multi-level detect and describe.  Pointers are raw device addresses; 0 stands for NULL."""

    def __init__(self, ctx, W, H, S, frames, opts=None, corner_cap=4096):
        self.ctx = ctx
        self.lib = ctx.lib
        self.opts = opts if opts is not None else OrbPyramidOpts()
        h = C.c_void_p()
        ctx._chk(self.lib.compvhip_orbpyr_create(ctx.h, W, H, S, frames, C.byref(self.opts), corner_cap, C.byref(h)))
        self.h = h
        self.W, self.H, self.S, self.frames, self.levels, self.corner_cap = W, H, S, frames, self.opts.levels, corner_cap

    def close(self):
        if self.h:
            self.lib.compvhip_orbpyr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def geometry(self, level):
        """-> (W, H, S, scale, quota) of a level; S == 0: the level is empty"""
        W, H, S, sf, q = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_float(), C.c_int()
        self.ctx._chk(self.lib.compvhip_orbpyr_geometry(self.h, level, C.byref(W), C.byref(H), C.byref(S), C.byref(sf), C.byref(q)))
        return W.value, H.value, S.value, np.float32(sf.value), q.value

    def plane(self, level, blurred=False):
        """device address of the level's plane [frames][H_l][S_l] as the last call built it"""
        p = C.c_void_p()
        self.ctx._chk(self.lib.compvhip_orbpyr_plane(self.h, level, int(bool(blurred)), C.byref(p)))
        return p.value

    def detect(self, d_gray, d_keypoints, key_cap, d_key_counts, d_level_counts=0, d_level_corners=0, stream=0):
        """compvhip_orbpyr_detect: d_keypoints [frames][key_cap] KEYPOINT_DTYPE in level order, d_key_counts [frames]; optional [frames][levels] int32 arrays"""
        self.ctx._chk(self.lib.compvhip_orbpyr_detect(self.h, d_gray or None, d_keypoints or None, key_cap, d_key_counts or None, d_level_counts or None,
                                                      d_level_corners or None, stream))

    def describe(self, d_gray, d_keypoints, key_cap, d_key_counts, d_desc, desc_stride=32, reuse_planes=False, stream=0):
        """compvhip_orbpyr_describe: every keypoint on the plane of its own level; reuse_planes: the planes of the preceding detect() on the same d_gray"""
        self.ctx._chk(self.lib.compvhip_orbpyr_describe(self.h, d_gray or None, int(bool(reuse_planes)), d_keypoints or None, key_cap, d_key_counts or None,
                                                        d_desc or None, desc_stride, stream))

    def set_timing(self, mode=1):
        self.ctx._chk(self.lib.compvhip_orbpyr_set_timing(self.h, int(mode)))

    def get_timing(self, cap=128):
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        n = self.lib.compvhip_orbpyr_get_timing(self.h, names, ms, cap)
        return [(names[i].decode(), ms[i]) for i in range(max(n, 0))]


def houghkht_link(edges, min_size=10):
    """The host stage of KHT alone (compvhip_houghkht_link_u8, no device): (points[n, 2] int32 as (x, y), string end indices)."""
    lib = load()
    e = np.ascontiguousarray(edges, dtype=np.uint8)
    H, W = e.shape
    sz = C.c_size_t
    lib.compvhip_houghkht_link_u8.argtypes = [C.c_void_p, sz, sz, sz, sz, C.c_void_p, sz, C.c_void_p, C.c_void_p, sz, C.c_void_p]
    n_set = int((e != 0).sum())
    xy = np.zeros((max(n_set, 1), 2), np.int32)
    ends = np.zeros(max(n_set, 1), np.uint32)
    npts, nstr = sz(0), sz(0)
    rc = lib.compvhip_houghkht_link_u8(_ptr(e), W, H, e.strides[0], min_size, _ptr(xy), len(xy), C.byref(npts), _ptr(ends), len(ends), C.byref(nstr))
    if rc:
        raise CompvHipError(rc, "compvhip_houghkht_link_u8")
    return xy[:npts.value].copy(), ends[:nstr.value].copy()


def host_cpu_budget():
    """CPUs this process may really use at once: min(hardware threads, affinity mask, cgroup quota) (compvhip_host_cpu_budget)."""
    lib = load()
    lib.compvhip_host_cpu_budget.restype = C.c_int
    return int(lib.compvhip_host_cpu_budget())


def houghsht_vote_grid(W, H, theta_deg=1.0, frames=1):
    """(nx, ny, window rows) of the voting kernel's image-tile grid for a plan of `frames` W x H frames (compvhip_houghsht_vote_grid)."""
    lib = load()
    nx = C.c_int(0); ny = C.c_int(0); rw = C.c_int(0)
    rc = lib.compvhip_houghsht_vote_grid(W, H, theta_deg, frames, C.byref(nx), C.byref(ny), C.byref(rw))
    if rc:
        raise CompvHipError(rc, "compvhip_houghsht_vote_grid")
    return nx.value, ny.value, rw.value


def houghkht_dims(W, H, rho=1.0, theta_deg=1.0):
    """(T, rhoN) of the KHT vote map for a W x H image (compvhip_houghkht_dims)."""
    lib = load()
    r = C.c_size_t(0); t = C.c_size_t(0)
    lib.compvhip_houghkht_dims.argtypes = [C.c_size_t, C.c_size_t, C.c_float, C.c_float, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    rc = lib.compvhip_houghkht_dims(W, H, rho, theta_deg, C.byref(r), C.byref(t))
    if rc:
        raise CompvHipError(rc, "compvhip_houghkht_dims")
    return int(t.value), int(r.value)


def to_cartesian(W, H, lines, kht=False):
    """CompVHoughSht / CompVHoughKht::toCartesian for (rho, theta) pairs: (n, 4) float32 a.x, a.y, b.x, b.y (host arithmetic, no GPU needed)."""
    L = load()
    n = len(lines)
    buf = np.zeros(max(n, 1), LINE_DTYPE)
    for i, l in enumerate(lines):
        buf[i]["rho"] = l[0]; buf[i]["theta"] = l[1]
    out = np.zeros((max(n, 1), 4), np.float32)
    fn = L.compvhip_houghkht_to_cartesian if kht else L.compvhip_houghsht_to_cartesian
    fn.argtypes = [C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    rc = fn(W, H, _ptr(buf), n, _ptr(out))
    if rc != OK:
        raise CompvHipError(rc, "invalid toCartesian parameters")
    return out[:n]


def morph_strel(kind, w, h):
    """CompVMathMorph::buildStructuringElement (host arithmetic, no GPU needed): (h, w) uint8, 0xff marks a member."""
    s = np.zeros((max(h, 0), max(w, 0)), np.uint8)
    rc = load().compvhip_morph_strel(kind, w, h, _ptr(s) if s.size else None)
    if rc != OK:
        raise CompvHipError(rc, "compvhip_morph_strel")
    return s


def gauss_kernel_fixedpoint(size, sigma):
    """CompVMathGauss::kernelDim1FixedPoint (host arithmetic, no GPU needed)."""
    k = np.zeros(size, np.uint16)
    rc = load().compvhip_gauss_kernel_fixedpoint(size, sigma, _ptr(k))
    if rc != OK:
        raise CompvHipError(rc, "invalid Gaussian kernel parameters")
    return k
