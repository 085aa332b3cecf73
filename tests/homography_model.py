"""The RANSAC homography of include/compv_hip.h ("RANSAC homography", items A - H) in numpy: the definition the device equals bit for bit.

Elementwise float64 operations only -- every +, -, *, /, sqrt below is ONE IEEE binary64 operation on arrays, in the order the definition gives; no
np.sum, no np.dot, no fused multiply-add, no transcendental function.  Everything is vectorised over hypotheses (the tries of a pair), so a case
of 200 tries and 129 points takes well under a second."""
import numpy as np

EPS = 2.0 ** -52
SQRT2 = 1.4142135623730950488016887242097
COS_PI_4 = 0.70710678118654757
MAX_ROTATIONS = 9 * 9 * 30
QUAD_DRAWS = 64
DBL_MAX = float(np.finfo(np.float64).max)
DEFAULT_THRESHOLD = 30.0

RESULT_DTYPE = np.dtype([("H", "<f8", (9,)), ("variance", "<f8"), ("inliers", "<i4"), ("bestTry", "<i4"), ("status", "<i4"), ("rotations", "<i4")])   # compvhip_homography_result
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("strength", "<f4"), ("orient", "<f4"), ("level", "<i4"), ("size", "<f4")])
MATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imageIdx", "<i4"), ("distance", "<i4")])

_QUIET = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


# ---- A. quads ------------------------------------------------------------------------------------------------------------------------------
def lowbias32(x):
    x = np.asarray(x, np.uint32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7feb352d)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846ca68b)
        x ^= x >> np.uint32(16)
    return x


def quads(seed, pair, k, tries):
    """int32 [tries][4]: the four indices of every try of pair `pair` among k >= 4 points"""
    assert k >= 4
    t = np.arange(tries, dtype=np.uint32)
    with np.errstate(over="ignore"):
        base = lowbias32(lowbias32(np.uint32(seed) ^ np.uint32(pair)) + t)
    out = np.full((tries, 4), -1, np.int64)
    filled = np.zeros(tries, np.int64)
    rows = np.arange(tries)
    for c in range(QUAD_DRAWS):
        if (filled == 4).all():
            break
        with np.errstate(over="ignore"):
            u = lowbias32(base + np.uint32(c))
        idx = ((u.astype(np.uint64) * np.uint64(k)) >> np.uint64(32)).astype(np.int64)
        take = (filled < 4) & ~(out == idx[:, None]).any(axis=1)
        out[rows[take], filled[take]] = idx[take]
        filled[take] += 1
    for r in np.nonzero(filled < 4)[0]:          # 64 draws did not fill the slots: the smallest unused indices
        idx = 0
        while filled[r] < 4:
            if idx not in out[r, :filled[r]]:
                out[r, filled[r]] = idx
                filled[r] += 1
            idx += 1
    return out.astype(np.int32)


# ---- B. collinearity -----------------------------------------------------------------------------------------------------------------------
def collinear(x, y):
    """x, y: [n][4] source coordinates of n quads -> bool [n]"""
    with np.errstate(**_QUIET):
        vertical = x[:, 0] == x[:, 1]
        slope = (y[:, 1] - y[:, 0]) / (x[:, 1] - x[:, 0])
        intercept = y[:, 0] - slope * x[:, 0]
        line = (y[:, 2] == slope * x[:, 2] + intercept) & (y[:, 3] == slope * x[:, 3] + intercept)
    return np.where(vertical, (x[:, 0] == x[:, 2]) & (x[:, 0] == x[:, 3]), line)


# ---- C. sums, normalisation, S -------------------------------------------------------------------------------------------------------------
def sum64(v):
    """v: [..., N] -> [...]: point i adds to partial i mod 64 in ascending i; the partials fold with p[l] += p[l + stride], stride 32 .. 1"""
    n = v.shape[-1]
    rounds = (n + 63) // 64
    pad = np.zeros(v.shape[:-1] + (rounds * 64,))
    pad[..., :n] = v
    part = np.zeros(v.shape[:-1] + (64,))
    for r in range(rounds):
        part = part + pad[..., 64 * r:64 * r + 64]
    stride = 32
    while stride:
        part = part[..., :stride] + part[..., stride:2 * stride]
        stride //= 2
    return part[..., 0]


def total(v):
    """the sum over the last axis as computeH takes it: index order for 4 terms, sum64 for more"""
    if v.shape[-1] == 4:
        return ((v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3]
    return sum64(v)


def hartley(x, y):
    """x, y: [n][N] -> tx, ty, s of [n]"""
    inv = np.float64(1.0) / np.float64(x.shape[-1])
    tx = total(x) * inv
    ty = total(y) * inv
    a = x - tx[:, None]
    b = y - ty[:, None]
    mean = total(np.sqrt(a * a + b * b)) * inv
    with np.errstate(**_QUIET):
        s = np.where(mean != 0.0, SQRT2 / mean, SQRT2)
    return tx, ty, s


def normalised(v, t, s):
    return s[:, None] * v + (-(t * s))[:, None]


def build_s(x, y, X, Y):
    """normalised points [n][N] -> S = MtM [n][9][9]: per entry, per point, row0[a] * row0[b] then row1[a] * row1[b]"""
    n, N = x.shape
    zero, one = np.zeros((n, N)), np.ones((n, N))
    m0 = np.stack([-x, -y, -one, zero, zero, zero, X * x, X * y, X], axis=1)          # [n][9][N]
    m1 = np.stack([zero, zero, zero, -x, -y, -one, Y * x, Y * y, Y], axis=1)
    S = np.zeros((n, 9, 9))
    for a in range(9):
        for b in range(a + 1):
            p0 = m0[:, a] * m0[:, b]
            p1 = m1[:, a] * m1[:, b]
            if N == 4:
                acc = np.zeros(n)
                for i in range(4):
                    acc = acc + p0[:, i]
                    acc = acc + p1[:, i]
            else:                      # partial i mod 64 takes point i's two products in turn; then the fold
                rounds = (N + 63) // 64
                q0 = np.zeros((n, rounds * 64))
                q1 = np.zeros((n, rounds * 64))
                q0[:, :N] = p0
                q1[:, :N] = p1
                part = np.zeros((n, 64))
                for r in range(rounds):
                    part = part + q0[:, 64 * r:64 * r + 64]
                    part = part + q1[:, 64 * r:64 * r + 64]
                stride = 32
                while stride:
                    part = part[:, :stride] + part[:, stride:2 * stride]
                    stride //= 2
                acc = part[:, 0]
            S[:, a, b] = acc
            S[:, b, a] = acc
    return S


# ---- D. Jacobi -----------------------------------------------------------------------------------------------------------------------------
def jacobi(S):
    """S: [n][9][9] -> D, Qt (rows = vectors), rotations [n]"""
    D = S.copy()
    n = D.shape[0]
    Q = np.zeros((n, 9, 9))
    Q[:, np.arange(9), np.arange(9)] = 1.0
    rot = np.zeros(n, np.int32)
    active = np.ones(n, bool)
    with np.errstate(**_QUIET):
        while True:
            best = np.abs(D[:, 1, 0])
            pr = np.ones(n, np.int64)
            pc = np.zeros(n, np.int64)
            for r in range(1, 9):
                for c in range(r):
                    v = np.abs(D[:, r, c])
                    b = v > best
                    best = np.where(b, v, best)
                    pr = np.where(b, r, pr)
                    pc = np.where(b, c, pc)
            active = active & (best > EPS) & (rot < MAX_ROTATIONS)
            idx = np.nonzero(active)[0]
            if not len(idx):
                break
            r, c = pr[idx], pc[idx]
            Ds, Qs = D[idx], Q[idx]
            ar = np.arange(len(idx))
            drr, dcc = Ds[ar, r, r], Ds[ar, c, c]
            y = 2.0 * Ds[ar, r, c]
            x = dcc - drr
            rho = np.sqrt(x * x + y * y)
            c2 = x / rho
            s2 = y / rho
            cos_a = np.sqrt((1.0 + c2) * 0.5)
            sin_a = s2 / (2.0 * cos_a)
            mag = np.sqrt((1.0 - c2) * 0.5)
            sin_b = np.where((s2 == 0.0) | (s2 > 0.0), mag, -mag)
            cos_b = s2 / (2.0 * sin_b)
            same = drr == dcc
            cs = np.where(same, COS_PI_4, np.where(c2 >= 0.0, cos_a, cos_b))[:, None]
            sn = np.where(same, COS_PI_4, np.where(c2 >= 0.0, sin_a, sin_b))[:, None]
            for A in (Qs, Ds):          # mulGA(A, r, c, cos, -sin) on the rows
                ri, rj = A[ar, r, :].copy(), A[ar, c, :].copy()
                A[ar, r, :] = ri * cs + (-sn) * rj
                A[ar, c, :] = ri * sn + cs * rj
            ri, rj = Ds[ar, :, r].copy(), Ds[ar, :, c].copy()          # the same formula on the columns of D
            Ds[ar, :, r] = ri * cs + (-sn) * rj
            Ds[ar, :, c] = ri * sn + cs * rj
            D[idx], Q[idx] = Ds, Qs
            rot[idx] += 1
    return D, Q, rot


def dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def compute_h(src, dst, promote):
    """src, dst: [n][N][2] (n hypotheses of N >= 4 correspondences each) -> H [n][9], rotations [n]"""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    n = src.shape[0]
    with np.errstate(**_QUIET):
        atx, aty, as_ = hartley(src[:, :, 0], src[:, :, 1])
        btx, bty, bs = hartley(dst[:, :, 0], dst[:, :, 1])
        S = build_s(normalised(src[:, :, 0], atx, as_), normalised(src[:, :, 1], aty, as_),
                    normalised(dst[:, :, 0], btx, bs), normalised(dst[:, :, 1], bty, bs))
        D, Q, rot = jacobi(S)
        idx = np.full(n, 8, np.int64)
        least = D[:, 8, 8].copy()
        for j in range(7, -1, -1):
            b = D[:, j, j] < least
            least = np.where(b, D[:, j, j], least)
            idx = np.where(b, j, idx)
        hn = Q[np.arange(n), idx, :]
        zero, one = np.zeros(n), np.ones(n)
        t1 = [as_, zero, zero, zero, as_, zero, -atx * as_, -aty * as_, one]
        m = [[dot3(t1[3 * i], t1[3 * i + 1], t1[3 * i + 2], hn[:, 3 * j], hn[:, 3 * j + 1], hn[:, 3 * j + 2]) for j in range(3)] for i in range(3)]
        inv = 1.0 / bs
        t2 = [inv, zero, btx, zero, inv, bty, zero, zero, one]
        H = np.stack([dot3(t2[3 * i], t2[3 * i + 1], t2[3 * i + 2], m[j][0], m[j][1], m[j][2]) for i in range(3) for j in range(3)], axis=1)
        if promote:
            H[:, :8] = np.where(np.abs(H[:, :8]) <= EPS, 0.0, H[:, :8])
        scale = np.where(H[:, 8] != 0.0, 1.0 / H[:, 8], 1.0)
        H = np.where((H[:, 8] != 0.0)[:, None], H * scale[:, None], H)
    return H, rot


# ---- E. inverse, distance, score -----------------------------------------------------------------------------------------------------------
def inverse3(a):
    """a: [n][9] -> inverse [n][9], ok [n] (False: a determinant of exactly 0)"""
    with np.errstate(**_QUIET):
        det = (a[:, 0] * (a[:, 4] * a[:, 8] - a[:, 7] * a[:, 5]) - a[:, 3] * (a[:, 1] * a[:, 8] - a[:, 7] * a[:, 2])) + a[:, 6] * (a[:, 1] * a[:, 5] - a[:, 4] * a[:, 2])
        d = 1.0 / det
        r = np.stack([((a[:, 4] * a[:, 8]) - (a[:, 7] * a[:, 5])) * d, ((a[:, 2] * a[:, 7]) - (a[:, 8] * a[:, 1])) * d, ((a[:, 1] * a[:, 5]) - (a[:, 4] * a[:, 2])) * d,
                      ((a[:, 5] * a[:, 6]) - (a[:, 8] * a[:, 3])) * d, ((a[:, 0] * a[:, 8]) - (a[:, 6] * a[:, 2])) * d, ((a[:, 2] * a[:, 3]) - (a[:, 5] * a[:, 0])) * d,
                      ((a[:, 3] * a[:, 7]) - (a[:, 6] * a[:, 4])) * d, ((a[:, 1] * a[:, 6]) - (a[:, 7] * a[:, 0])) * d, ((a[:, 0] * a[:, 4]) - (a[:, 3] * a[:, 1])) * d], axis=1)
    return r, ~(det == 0.0)


def mse_through(A, ax, ay, bx, by):
    """A: [n][9]; points [k] -> [n][k]"""
    one = np.ones_like(ax)
    c = [A[:, j][:, None] for j in range(9)]
    with np.errstate(**_QUIET):
        X = dot3(c[0], c[1], c[2], ax, ay, one)
        Y = dot3(c[3], c[4], c[5], ax, ay, one)
        Z = dot3(c[6], c[7], c[8], ax, ay, one)
        scale = 1.0 / Z
        ex = X * scale - bx
        ey = Y * scale - by
        return ex * ex + ey * ey


def distances(H, Hinv, src, dst):
    """[n][k]: mse(H src, dst) + mse(Hinv dst, src)"""
    with np.errstate(**_QUIET):
        return mse_through(H, src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]) + mse_through(Hinv, dst[:, 0], dst[:, 1], src[:, 0], src[:, 1])


def score(d, live, threshold):
    """d: [n][k] distances; live: [n] (False: the try scores 0) -> count int32 [n], variance [n], inlier flags [n][k]"""
    n, k = d.shape
    inl = (d < threshold) & live[:, None]
    count = np.zeros(n, np.int32)
    s = np.zeros(n)
    for i in range(k):
        s = np.where(inl[:, i], s + d[:, i], s)
        count = count + inl[:, i]
    with np.errstate(**_QUIET):
        mean = np.where(count > 0, s / np.maximum(count, 1), 0.0)
        var = np.zeros(n)
        for i in range(k):
            dev = d[:, i] - mean
            var = np.where(inl[:, i], var + dev * dev, var)
        variance = np.where(count >= 2, var / np.maximum(count - 1, 1), DBL_MAX)
    return count.astype(np.int32), variance, inl


def better(cb, vb, tb, ca, va, ta):
    """item F: does (count, variance, try) b beat a"""
    if cb < 4:
        return False
    if ca < 4:
        return True
    if cb != ca:
        return cb > ca
    if vb < va:
        return True
    if va < vb:
        return False
    return tb < ta


# ---- the whole call for one pair -----------------------------------------------------------------------------------------------------------
def find(src, dst, count, tries, threshold=DEFAULT_THRESHOLD, seed=0, pair=0, quad_list=None):
    """src, dst: [pointCap][2]; count: the pair's (clamped here) -> dict(result (RESULT_DTYPE scalar), mask uint8 [k], counts, variances, rotations per try,
    quads)"""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    k = max(0, min(int(count), len(src)))
    res = np.zeros((), RESULT_DTYPE)
    res["variance"], res["bestTry"] = DBL_MAX, -1
    if k < 4:
        res["status"] = 2
        return dict(result=res, mask=np.zeros(k, np.uint8), counts=None, variances=None, rotations=None, quads=None, k=k)
    src, dst = src[:k], dst[:k]
    q = quads(seed, pair, k, tries) if quad_list is None else np.asarray(quad_list, np.int32).reshape(tries, 4)
    in_range = ((q >= 0) & (q < k)).all(axis=1)
    qs = np.where(in_range[:, None], q, 0)
    col = collinear(src[qs, 0], src[qs, 1])
    solve = in_range & ~col
    H = np.zeros((tries, 9))
    Hinv = np.zeros((tries, 9))
    rot = np.zeros(tries, np.int32)
    live = np.zeros(tries, bool)
    si = np.nonzero(solve)[0]
    if len(si):
        H[si], rot[si] = compute_h(src[qs[si]], dst[qs[si]], False)
        Hinv[si], live[si] = inverse3(H[si])
    d = np.full((tries, k), np.inf)
    li = np.nonzero(live)[0]
    if len(li):
        d[li] = distances(H[li], Hinv[li], src, dst)
    counts, variances, inl = score(d, live, threshold)
    bc, bv, bt = 0, DBL_MAX, -1
    for t in range(tries):
        if better(int(counts[t]), float(variances[t]), t, bc, bv, bt):
            bc, bv, bt = int(counts[t]), float(variances[t]), t
    mask = np.zeros(k, np.uint8)
    if bc >= 4:
        mask = inl[bt].astype(np.uint8)
        sel = np.nonzero(inl[bt])[0]
        Hf, rf = compute_h(src[sel][None], dst[sel][None], True)
        res["variance"], res["inliers"], res["bestTry"], res["status"] = bv, bc, bt, 0
    else:
        Hf, rf = compute_h(src[None], dst[None], True)
        res["status"] = 1
    res["H"], res["rotations"] = Hf[0], rf[0]
    return dict(result=res, mask=mask, counts=counts, variances=variances, rotations=rot, quads=q, k=k, distances=d, inlier_sets=inl)


# ---- H. projection -------------------------------------------------------------------------------------------------------------------------
def project(H, pts):
    """H: [9]; pts: [n][2] -> [n][2]"""
    H, pts = np.asarray(H, np.float64).reshape(9), np.asarray(pts, np.float64)
    x, y, one = pts[:, 0], pts[:, 1], np.ones(len(pts))
    with np.errstate(**_QUIET):
        X = dot3(H[0], H[1], H[2], x, y, one)
        Y = dot3(H[3], H[4], H[5], x, y, one)
        Z = dot3(H[6], H[7], H[8], x, y, one)
        s = 1.0 / Z
        return np.stack([X * s, Y * s], axis=1)


# ---- gathering the points of a good list ----------------------------------------------------------------------------------------------------
def gather(good, good_count, good_cap, point_cap, query, train):
    """good: MATCH_DTYPE [goodCap]; query / train: KEYPOINT_DTYPE [cap] -> src [k][2], dst [k][2] float64"""
    n = min(max(int(good_count), 0), good_cap, point_cap)
    g = good[:n]
    ok = (g["queryIdx"] >= 0) & (g["queryIdx"] < len(query)) & (g["trainIdx"] >= 0) & (g["trainIdx"] < len(train))
    g = g[ok]
    src = np.stack([train["x"][g["trainIdx"]].astype(np.float64), train["y"][g["trainIdx"]].astype(np.float64)], axis=1).reshape(-1, 2)
    dst = np.stack([query["x"][g["queryIdx"]].astype(np.float64), query["y"][g["queryIdx"]].astype(np.float64)], axis=1).reshape(-1, 2)
    return src, dst
