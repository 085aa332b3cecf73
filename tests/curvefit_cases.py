"""Point sets of the curve-fit tests (tests/test_curvefit_*.py, tests/test_gpu_curvefit.py, tests/golden/make_golden_curvefit.py): deterministic
functions of their arguments, so that every test and the fixture generator see the same sets.

planted(): points of a curve with INTEGER coefficients at INTEGER abscissas -- every coordinate is exactly representable, and so is every term of the
curve's value -- plus `share` outliers that lie at least 4 x threshold from the curve.  noisy(): the same with float abscissas and inliers moved by at
most 0.3 x threshold."""
import numpy as np

import curvefit_model as cm

THRESHOLD = 1.0
KS = (9, 63, 64, 65, 129, 257)          # sum64 partials and the 256-point LDS round
SHARES = (0.0, 0.3)
GPU_KS = {cm.LINE: (1, 2, 3, 63, 64, 65, 255, 256, 257, 600), cm.PARABOLA: (2, 3, 4, 63, 64, 65, 255, 256, 257, 600)}
GPU_KS[cm.PARABOLA_SIDEWAYS] = GPU_KS[cm.PARABOLA]
TRIES = (1, 255, 256, 257)


def curve(model, rng):
    """integer coefficients: a line y = a x + b as (A, B, C) = (a, -1, b); a parabola y = a x^2 + b x + c"""
    if model == cm.LINE:
        return float(rng.randint(-3, 4)), -1.0, float(rng.randint(0, 50))
    return float(rng.choice([-2, -1, 1, 2])), float(rng.randint(-5, 6)), float(rng.randint(-20, 21))


def value(model, coef, x):
    """the curve's ordinate at the abscissa x (every term an exact integer for integer x)"""
    if model == cm.LINE:
        return coef[0] * x + coef[2]
    return (coef[0] * x) * x + coef[1] * x + coef[2]


def assemble(model, x, y):
    """[k][2] points from the model's abscissas and ordinates (a sideways parabola has them exchanged)"""
    return np.stack([y, x], axis=1) if model == cm.PARABOLA_SIDEWAYS else np.stack([x, y], axis=1)


def planted(model, k, share, seed, threshold=THRESHOLD, noise=0.0):
    """-> points float64 [k][2], inlier flags bool [k], the curve's coefficients.  Distinct abscissas; the outliers are spread over the set."""
    rng = np.random.RandomState(1000 * seed + 7 * k + model)
    coef = curve(model, rng)
    span = 60 if model != cm.LINE else 400
    x = rng.permutation(np.arange(-span, span + 1) if k <= 2 * span + 1 else np.arange(-k, k + 1))[:k].astype(np.float64)
    if noise:
        x = x + rng.uniform(-0.25, 0.25, k)
    y = value(model, coef, x)
    n_out = int(round(k * share))
    inl = np.ones(k, bool)
    inl[rng.permutation(k)[:n_out]] = False
    # a line's residual is the perpendicular distance dy / sqrt(1 + a^2); a parabola's is dy itself
    least = 4.0 * threshold * (np.sqrt(1.0 + coef[0] * coef[0]) if model == cm.LINE else 1.0)
    off = np.ceil(least) + 1.0 + rng.randint(0, 40, k)
    off = np.where(rng.randint(0, 2, k) == 1, off, -off)
    y = np.where(inl, y + (rng.uniform(-noise, noise, k) if noise else 0.0), y + off)
    return assemble(model, x, y), inl, coef


def noisy(model, k, share, seed, threshold=THRESHOLD):
    return planted(model, k, share, seed, threshold, noise=0.3 * threshold)


def all_equal(k):
    """every try of every model is rejected"""
    return np.full((k, 2), 7.0)


def same_abscissa(model, k):
    """all x equal (all y for the sideways parabola): every parabola try is rejected; a line fits"""
    t = np.arange(k, dtype=np.float64)
    return assemble(model, np.full(k, 3.0), t)


def ragged_counts(sets, cap, seed=5):
    """int32 [sets]: 0, a negative count, one beyond the capacity, m - 1 .. m + 1 and random sizes"""
    rng = np.random.RandomState(seed)
    c = rng.randint(0, cap + 1, sets).astype(np.int32)
    c[:7] = [0, -3, cap + 9, 1, 2, 3, 4][:min(7, sets)]
    return c
