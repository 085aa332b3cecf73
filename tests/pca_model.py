"""The PCA projection of include/compv_hip.h ("PCA projection", items B - G) restated in numpy float32: every array operation below is one IEEE binary32
operation per element (numpy neither fuses nor reorders elementwise float32 arithmetic, and the host keeps denormals), in the order the definition
gives.  Beside the definition: three deliberately different evaluations (left to right, fused multiply-add, flush to zero) that the fixture generator
uses to show that the stored cases tell the orders apart."""
import json

import numpy as np

F = np.float32
TINY = np.finfo(np.float32).tiny


def centre(x, mean):
    """item B"""
    x = np.asarray(x, F)
    return x if mean is None else x - np.asarray(mean, F)[None, :]


def dot16(A, B, fused=False, ftz=False):
    """item C for every pair of rows: A (n, D), B (M, D) -> (n, M).  fused: v += a * b rounded once (through float64: the product of two float32 is exact
    there; the one sum is then rounded twice, to float64 and to float32, which differs from a true fused operation only in rare ties).  ftz: denormal
    inputs, products and sums are flushed to zero."""
    A, B = np.asarray(A, F), np.asarray(B, F)
    n, D = A.shape
    M = B.shape[0]
    assert B.shape[1] == D

    def flush(x):
        return np.where(np.abs(x) < TINY, F(0), x).astype(F) if ftz else x
    A, B = flush(A), flush(B)

    def madd(v, a, b):
        if fused:
            return (v.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(F)
        return flush(v + flush(a * b))
    v = np.zeros((n, M, 16), F)
    k = 0
    while k + 16 <= D:
        v = madd(v, A[:, None, k:k + 16], B[None, :, k:k + 16])
        k += 16
    while k + 4 <= D:
        v[:, :, 0:4] = madd(v[:, :, 0:4], A[:, None, k:k + 4], B[None, :, k:k + 4])
        k += 4
    add = (lambda x, y: flush(x + y))
    v[:, :, 0:4] = add(v[:, :, 0:4], v[:, :, 4:8])
    v[:, :, 8:12] = add(v[:, :, 8:12], v[:, :, 12:16])
    v[:, :, 0:4] = add(v[:, :, 0:4], v[:, :, 8:12])
    v[:, :, 0:2] = add(v[:, :, 0:2], v[:, :, 2:4])
    v[:, :, 0] = add(v[:, :, 0], v[:, :, 1])
    while k < D:
        v[:, :, 0] = madd(v[:, :, 0], A[:, None, k], B[None, :, k])
        k += 1
    return np.ascontiguousarray(v[:, :, 0])


def dot_left_to_right(A, B):
    """the same products summed into one accumulator in column order"""
    A, B = np.asarray(A, F), np.asarray(B, F)
    v = np.zeros((A.shape[0], B.shape[0]), F)
    for k in range(A.shape[1]):
        v = v + A[:, None, k] * B[None, :, k]
    return v


def project(x, mean, vectors, **how):
    """items B and D"""
    return dot16(centre(x, mean), vectors, **how)


def mulabt(A, B):
    """item E"""
    return dot16(A, B)


def mean_of(obs):
    """item F: the binary64 sum in row order, times 1.0 / n, rounded to float32"""
    obs = np.asarray(obs, F)
    s = np.zeros(obs.shape[1], np.float64)
    for row in obs:
        s = s + row.astype(np.float64)
    return (s * (1.0 / float(obs.shape[0]))).astype(F)


def covariance(obs):
    """item F: (mean, covar)"""
    obs = np.asarray(obs, F)
    n = obs.shape[0]
    m = mean_of(obs)
    c = np.ascontiguousarray((obs - m[None, :]).T)
    cov = dot16(c, c)
    if n > 1:
        cov = cov * (F(1) / F(n - 1))
    return m, cov


def parse_text(text):
    """item G with Python's json (strtod semantics for reals, integers exact): -> (mean (D,), vectors (M, D), values (M,)) float32"""
    root = json.loads(text)
    out = []
    for name in ("mean", "vectors", "values"):
        m = root[name]
        assert m["type"] == "32f"
        r, c = m["size"]
        a = np.array([float(v) for v in m["data"]], np.float64).astype(F)
        assert a.size == r * c
        out.append(a.reshape(r, c))
    mean, vectors, values = out
    assert mean.shape[0] == 1 and values.shape[0] == 1 and vectors.shape == (values.shape[1], mean.shape[1])
    return mean[0], vectors, values[0]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)
