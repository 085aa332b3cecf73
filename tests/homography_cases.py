"""Seeded point sets for the RANSAC homography tests: a known H maps k points of a 640 x 480 frame; inliers carry uniform noise of at most NOISE (0.05) px per
coordinate, outliers land somewhere else in the frame, at least 60 px from where H sends them.  Only numpy's default_rng integers / uniform doubles
and plain arithmetic: any box regenerates the same bits.  (The golden file stores its inputs anyway.)"""
import numpy as np

W, H_ = 640, 480
# a mild perspective: rotation about 8 degrees, scale 0.9, a shift, two small projective terms (literal entries: no libm on the way)
PLANTED_H = np.array([[0.8912, -0.1253, 31.5], [0.1253, 0.8912, -12.25], [0.00011, -0.00007, 1.0]])
KS = (4, 5, 9, 63, 64, 65, 129)
SHARES = (0.0, 0.3, 0.6)
TRIES = (1, 63, 64, 65, 200)
# Inlier noise per coordinate, px.  Well below the 0.5 px the cases may carry: the fixture generator demands that no distance of any try lies within 0.1 % of
# the threshold, and with 0.5 px the quads that extrapolate badly scatter their distances through the threshold in every large case.
NOISE = 0.05


def apply(Hm, pts):
    z = Hm[2, 0] * pts[:, 0] + Hm[2, 1] * pts[:, 1] + Hm[2, 2]
    return np.stack([(Hm[0, 0] * pts[:, 0] + Hm[0, 1] * pts[:, 1] + Hm[0, 2]) / z, (Hm[1, 0] * pts[:, 0] + Hm[1, 1] * pts[:, 1] + Hm[1, 2]) / z], axis=1)


def planted(k, share, seed):
    """-> src [k][2], dst [k][2] float64, planted inlier flags bool [k].  Unless share == 1 (all outliers) at least 5 inliers stay (all 4 when k == 4): a
    quad always fits its own four points, so a planted set of four could not be told from any other quad."""
    rng = np.random.default_rng([seed, k, int(round(share * 100))])
    src = np.stack([rng.uniform(20.0, W - 20.0, k), rng.uniform(20.0, H_ - 20.0, k)], axis=1)
    true = apply(PLANTED_H, src)
    dst = true + rng.uniform(-NOISE, NOISE, (k, 2))
    n_out = k if share >= 1.0 else max(0, min(int(share * k), k - 5))
    inl = np.ones(k, bool)
    if n_out:
        out = np.sort(rng.permutation(k)[:n_out])
        inl[out] = False
        for i in out:
            while True:
                cand = np.array([rng.uniform(0.0, W), rng.uniform(0.0, H_)])
                if np.abs(cand - true[i]).max() >= 60.0:
                    break
            dst[i] = cand
    return src, dst, inl


def edge_quads(k):
    """quads for the parity hook on a planted case of k >= 9 points: an ordinary one, one with a repeated index (a singular system), one out of range"""
    return np.array([[0, 1, 2, 3], [4, 4, 5, 6], [0, 1, 2, k], [5, 6, 7, 8], [-1, 2, 3, 4]], np.int32)


def collinear_case():
    """9 points whose first four sources lie exactly on y = 2 x + 1 (small integers: every product is exact), the rest planted"""
    src, dst, inl = planted(9, 0.0, 77)
    src[:4] = [[10.0, 21.0], [20.0, 41.0], [35.0, 71.0], [50.0, 101.0]]
    dst[:4] = apply(PLANTED_H, src[:4])
    return src, dst, inl


def line_case(k):
    """k points whose sources all lie exactly on y = 2 x + 1 (integers: slope and products are exact), so that EVERY quad is collinear and no try
    scores: the path on which the result is computeH of all points (status 1)"""
    src, dst, _ = planted(k, 0.0, 78)
    src[:, 0] = 10.0 + 7.0 * np.arange(k)
    src[:, 1] = 2.0 * src[:, 0] + 1.0
    return src, dst
