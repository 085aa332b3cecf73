"""The definition of the brute-force Hamming matcher (include/compv_hip.h, docs/kernels/match.md) in numpy: distance matrix, stable argsort,
good list; and the reference's own insertion order (knn_reference), which differs from the stable order among equal distances.  What the GPU tests compare with byte for byte, and what tests/test_match_model.py holds against the records of the compiled
reference (tests/golden/golden_match.json)."""
import numpy as np

MATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imageIdx", "<i4"), ("distance", "<i4")])   # CompVDMatch
INT32_MAX = 0x7fffffff
POP8 = np.array([bin(v).count("1") for v in range(256)], np.int32)


def distances(query, train):
    """(Q, T) int32: popcount of the XOR of the rows"""
    Q, T = len(query), len(train)
    out = np.empty((Q, T), np.int32)
    step = max(1, (1 << 22) // max(1, T * query.shape[1]))
    for q0 in range(0, Q, step):
        out[q0:q0 + step] = POP8[query[q0:q0 + step, None, :] ^ train[None, :, :]].sum(axis=2)
    return out


def knn(query, train, k, D=None):
    """(min(k, T), Q) records: neighbour r of query q = the r-th train row in ascending (distance, train index) order -- the reference's shape"""
    D = distances(query, train) if D is None else D
    Q, T = D.shape
    rows = min(k, T)
    order = np.argsort(D, axis=1, kind="stable")[:, :rows]          # stable: the lower train index first among equal distances
    out = np.zeros((rows, Q), MATCH_DTYPE)
    out["queryIdx"] = np.arange(Q, dtype=np.int32)[None, :]
    out["trainIdx"] = order.T
    out["distance"] = np.take_along_axis(D, order, axis=1).T
    return out


def knn_reference(query, train, k, D=None):
    """(min(k, T), Q) records as the REFERENCE leaves them (core/matchers/compv_core_matcher_bruteforce.cxx:196-225, and :168-195, which is the
    same procedure for two rows): t walks upward; the candidate walks down the list and swaps with every entry whose DISTANCE is larger, the
    displaced entry walks on.  The distances of a column are the same as knn()'s; among equal distances the train indices may differ (an entry
    displaced from the head of a run of equal distances lands behind the run, or falls off the list).  What compvhip_match_hamming_u8 returns."""
    D = distances(query, train) if D is None else D
    Q, T = D.shape
    rows = min(k, T)
    bd = np.full((rows, Q), INT32_MAX, np.int64)
    bt = np.full((rows, Q), -1, np.int64)
    for t in range(T):
        cd, ct = D[:, t].astype(np.int64), np.full(Q, t, np.int64)
        for r in range(rows):
            lt = cd < bd[r]
            if not lt.any():
                continue
            od, ot = bd[r].copy(), bt[r].copy()
            bd[r], bt[r] = np.where(lt, cd, od), np.where(lt, ct, ot)
            cd, ct = np.where(lt, od, cd), np.where(lt, ot, ct)
    out = np.zeros((rows, Q), MATCH_DTYPE)
    out["queryIdx"] = np.arange(Q, dtype=np.int32)[None, :]
    out["trainIdx"] = bt
    out["distance"] = bd
    return out


def knn_device(query, train, k, D=None):
    """(k, Q) records, the device form: rows r >= T hold {q, -1, 0, INT32_MAX}"""
    Q, T = len(query), len(train)
    out = np.zeros((k, Q), MATCH_DTYPE)
    out["queryIdx"] = np.arange(Q, dtype=np.int32)[None, :]
    out["trainIdx"] = -1
    out["distance"] = INT32_MAX
    if Q and T:
        m = knn(query, train, k, D)
        out[:len(m)] = m
    return out


def good(query, train, k, ratio=0.0, max_distance=-1, cross_check=False, D=None):
    """matches[0][q] of the queries that pass every enabled test, ascending q"""
    Q, T = len(query), len(train)
    if not Q or not T:
        return np.zeros(0, MATCH_DTYPE)
    D = distances(query, train) if D is None else D
    m = knn_device(query, train, k, D)
    ok = np.ones(Q, bool)
    if ratio > 0:
        assert k >= 2
        # one binary64 multiply, one compare
        ok &= (m[0]["distance"].astype(np.float64) < np.float64(ratio) * m[1]["distance"].astype(np.float64)) if T >= 2 else False
    if max_distance >= 0:
        ok &= m[0]["distance"] <= max_distance
    if cross_check:
        best_query = np.argmin(D, axis=0)          # the first minimum: the smallest (distance, query index)
        ok &= best_query[m[0]["trainIdx"]] == np.arange(Q)
    return m[0][ok].copy()


# ---- content any box can regenerate ---------------------------------------------------------------------------------------------------------
def uniform(n, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, cols), dtype=np.uint8)


def tie_heavy(n, cols, seed, pool_seed=77):
    """rows drawn from a pool of 6 distinct descriptors (the pool depends on pool_seed and cols only, so the query and the train side share it);
    every third row differs from its pool member in one bit: nearly every query has several train rows at equal distance"""
    pool = np.random.default_rng(pool_seed * 1000 + cols).integers(0, 256, size=(6, cols), dtype=np.uint8)
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, 6, size=n)
    out = pool[pick].copy()
    flip = rng.integers(0, 3, size=n) == 0
    bit = rng.integers(0, cols * 8, size=n)
    for i in np.nonzero(flip)[0]:
        out[i, bit[i] >> 3] ^= np.uint8(1 << (bit[i] & 7))
    return out


def content(kind, n, cols, seed):
    return uniform(n, cols, seed) if kind == "uniform" else tie_heavy(n, cols, seed)
