"""The inputs of the PCA tests, shared by the fixture generator (tests/golden/make_golden_pca.py), the CPU tests and the GPU tests.  Everything is made
from integer arithmetic on uint64 arrays (no random generator whose stream could change between library versions), so every process composes the same
bytes; the fixture stores digests of what must not move."""
import hashlib

import numpy as np

# models the reference trains and writes itself: (D, M, n observations)
TRAINED = [(5, 2, 40), (17, 5, 33), (20, 8, 40), (36, 3, 7), (67, 12, 100), (130, 10, 50)]
# mean and covariance: (n, D), each trained through the reference with M = min(2, D - 1) components
COVARIANCE = [(1, 5), (2, 5), (33, 17), (100, 67), (50, 130)]
# hand-composed model files read through the reference's read: (D, M)
HAND = [(1, 2), (3, 2), (4, 3), (15, 3), (16, 3), (19, 3), (31, 3), (32, 3), (33, 3), (7, 1), (7, 63), (7, 64), (7, 65)]
# composed again in every process instead of being stored (their SHA-256 is in the fixture): the HOG descriptor of a 64 x 128 crop, and the shape of the
# reference's own tests/math/pca.cxx
COMPOSED = [(3780, 8), (441, 92)]
ROWS = (1, 2, 63, 64, 65, 100)          # observation rows of the projection cases, dealt round the models
DENORMAL = "denormal_d37_m3"


def uniform(shape, seed):
    """float32 in [-1, 1) with 24 random bits each, from a splitmix64 of the element's index"""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        x = np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        x ^= x >> np.uint64(30); x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27); x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return (((x >> np.uint64(40)).astype(np.int64) - (1 << 23)).astype(np.float32) / np.float32(1 << 23)).reshape(shape)


def observations(n, D, seed):
    """n correlated observations of D dimensions: four latent factors, an offset per dimension and noise"""
    k = min(4, D)
    latent = uniform((n, k), seed) * np.float32(3)
    mix = uniform((k, D), seed + 1)
    obs = (latent.astype(np.float64) @ mix.astype(np.float64)).astype(np.float32)
    return np.ascontiguousarray(obs + uniform((n, D), seed + 2) * np.float32(0.25) + uniform((1, D), seed + 3) * np.float32(5))


def rows(n, D, seed):
    """n rows to project: values of mixed magnitude"""
    return np.ascontiguousarray(uniform((n, D), seed) * (np.float32(1) + np.float32(7) * np.abs(uniform((n, D), seed + 1))))


def reference_rows(n=100, D=441):
    """the features of the reference's own tests/math/pca.cxx: ((i * 398 + i) * (+-1) * 4.95f) * (j + 0.5f)"""
    i = np.arange(D, dtype=np.int32)
    a = ((i * 398 + i) * np.where(i & 1, 1, -1)).astype(np.float32) * np.float32(4.95)
    return np.ascontiguousarray(a[None, :] * (np.arange(n, dtype=np.int32).astype(np.float32) + np.float32(0.5))[:, None])


def number_text(v, style):
    """one value as JSON text: an integer, an exponent form or a 17-digit decimal"""
    if style == 0:
        return "%d" % int(round(v * 8))
    if style == 1:
        return ("%.6e" % v).replace("e", "E") if v < 0 else "%.6e" % v
    return "%.17g" % v


def compose_text(D, M, seed):
    """the text of a hand-composed model file: members out of order, one unknown member, all three number styles"""
    def mat(r, c, s, scale):
        vals = uniform((r * c,), s).astype(np.float64) * scale + uniform((r * c,), s + 7).astype(np.float64) * 1e-9
        body = ",".join(number_text(float(v), (k + s) % 3) for k, v in enumerate(vals))
        return r, c, body
    parts = {}
    for name, (r, c, s, scale) in {"mean": (1, D, seed, 2.0), "vectors": (M, D, seed + 1, 1.0), "values": (1, M, seed + 2, 50.0)}.items():
        r, c, body = mat(r, c, s, scale)
        if name == "vectors":
            parts[name] = '"vectors" : {"data":[%s],\n "size":[%d, %d], "type":"32f"}' % (body, r, c)
        elif name == "mean":
            parts[name] = '"mean":{"type":"32f","note":{"by":["hand",1,true,null],"x":-1.5e2},"size":[%d,%d],"data":[%s]}' % (r, c, body)
        else:
            parts[name] = '"values":{"size":[%d,%d],"type":"32f","data":[ %s ]}' % (r, c, body)
    return '{ "comment": "composed by tests/pca_cases.py", %s,\n%s,\t%s }\n' % (parts["values"], parts["vectors"], parts["mean"])


def sha256(data):
    return hashlib.sha256(data if isinstance(data, bytes) else np.ascontiguousarray(data).tobytes()).hexdigest()


def hand_name(D, M):
    return "pca_hand_d%d_m%d" % (D, M)


def trained_name(D, M):
    return "pca_trained_d%d_m%d" % (D, M)


def denormal_case():
    """rows and vectors scaled so that products (about 1e-40) and their partial sums are float32 denormals; no mean"""
    D, M, n = 37, 3, 5
    return np.ascontiguousarray(uniform((n, D), 901) * np.float32(1e-20)), np.ascontiguousarray(uniform((M, D), 902) * np.float32(3e-20))


def mulabt_cases():
    """(aRows, bRows, cols) with A != B"""
    return [(1, 1, 1), (3, 65, 17), (65, 3, 36), (64, 64, 67)]


def mulabt_inputs(a_rows, b_rows, cols):
    return rows(a_rows, cols, 1000 + a_rows + cols), rows(b_rows, cols, 2000 + b_rows + cols)
