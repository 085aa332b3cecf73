"""The inputs of the image-moments fixture and tests, written out or regenerated from seeds: tests/golden/make_golden_moments.py runs the compiled
reference on them, the tests run the model, the host code and the GPU on them.  tests/golden/golden_moments.json / .npz hold the OUTPUTS only.

Frame cases: noise, text-like blobs, 0 / 1 planes, all-zero, all-255, one pixel in each corner, W or H of 1, up to 2048 x 2048, and 8192 x 256 filled
with 255 -- the one whose m20 (1.2e16) lies above 2^53, where the reference's double sums round and the library's integers do not.
Component cases: frames of text-like blobs labelled by tests/components_model.py, with and without gray planes, both origins."""
import numpy as np

import moments_model as mm

BIG = "full8192"


def blobs(w, h, seed, count=None):
    """text-like blobs: filled strokes of random size and gray level on a zero ground, some touching, some with holes of zeros"""
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w), np.uint8)
    for _ in range(count if count is not None else max(3, w * h // 400)):
        bw, bh = int(rng.integers(1, max(2, w // 4))), int(rng.integers(1, max(2, h // 4)))
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        img[y:y + bh, x:x + bw] = rng.integers(1, 256, (min(bh, h - y), min(bw, w - x)), dtype=np.uint8)
        if bw > 2 and bh > 2 and y + 1 < h and x + 1 < w:
            img[y + 1, x + 1] = 0
    return img


def frame_cases():
    """dicts: id, size (W, H), kind, seed, weights: the modes the case runs with"""
    both = (mm.VALUE, mm.UNIT)
    out = [
        {"id": "noise61", "size": (61, 37), "kind": "noise", "seed": 81000, "weights": both},
        {"id": "noise1025", "size": (1025, 19), "kind": "noise", "seed": 81001, "weights": both},
        {"id": "sparse203", "size": (203, 97), "kind": "sparse", "seed": 81002, "weights": both},
        {"id": "text203", "size": (203, 97), "kind": "blobs", "seed": 81003, "weights": both},
        {"id": "text640", "size": (640, 360), "kind": "blobs", "seed": 81004, "weights": both},
        {"id": "bin64", "size": (64, 48), "kind": "bin01", "seed": 81005, "weights": both},
        {"id": "zeros17", "size": (17, 9), "kind": "zeros", "seed": 0, "weights": both},
        {"id": "full40", "size": (40, 40), "kind": "full", "seed": 0, "weights": both},
        {"id": "corner_tl", "size": (33, 21), "kind": "pixel", "seed": 0, "at": (0, 0), "weights": (mm.VALUE,)},
        {"id": "corner_tr", "size": (33, 21), "kind": "pixel", "seed": 0, "at": (32, 0), "weights": (mm.VALUE,)},
        {"id": "corner_bl", "size": (33, 21), "kind": "pixel", "seed": 0, "at": (0, 20), "weights": (mm.VALUE,)},
        {"id": "corner_br", "size": (33, 21), "kind": "pixel", "seed": 0, "at": (32, 20), "weights": both},
        {"id": "col57", "size": (1, 57), "kind": "noise", "seed": 81006, "weights": both},
        {"id": "row300", "size": (300, 1), "kind": "noise", "seed": 81007, "weights": both},
        {"id": "one", "size": (1, 1), "kind": "full", "seed": 0, "weights": both},
        {"id": "noise2048", "size": (2048, 2048), "kind": "noise", "seed": 81008, "weights": (mm.VALUE,)},
        {"id": BIG, "size": (8192, 256), "kind": "full", "seed": 0, "weights": (mm.VALUE,)},
    ]
    return out


def frame_case(cid):
    return next(c for c in frame_cases() if c["id"] == cid)


def frame(c):
    """(H, W) uint8"""
    w, h = c["size"]
    rng = np.random.default_rng(c["seed"])
    kind = c["kind"]
    if kind == "noise":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "sparse":          # three pixels in four are zero
        return (rng.integers(0, 256, (h, w), dtype=np.uint8) * (rng.integers(0, 4, (h, w)) == 0)).astype(np.uint8)
    if kind == "blobs":
        return blobs(w, h, c["seed"])
    if kind == "bin01":
        return rng.integers(0, 2, (h, w), dtype=np.uint8)
    if kind == "zeros":
        return np.zeros((h, w), np.uint8)
    if kind == "full":
        return np.full((h, w), 255, np.uint8)
    assert kind == "pixel", kind
    img = np.zeros((h, w), np.uint8)
    img[c["at"][1], c["at"][0]] = 201
    return img


def component_cases():
    """dicts: id, size (W, H), seed, connectivity, min_pixels, gray (are gray planes given), weights, origin"""
    out = []
    for cid, size, seed, conn, mp in (("blobs97", (97, 61), 82000, 8, 1), ("blobs203", (203, 97), 82001, 4, 3)):
        for gray, weights in ((False, mm.VALUE), (True, mm.VALUE), (True, mm.UNIT)):
            for origin in (mm.ORIGIN_FRAME, mm.ORIGIN_BOX):
                out.append({"id": "%s_%s_%s" % (cid, "mask" if not gray else ("value", "unit")[weights], ("frame", "box")[origin]), "size": size, "seed": seed,
                            "connectivity": conn, "min_pixels": mp, "gray": gray, "weights": weights, "origin": origin})
    return out


def component_frame(c):
    """(the binary map the labeller gets, the gray plane): the gray plane has zeros INSIDE blobs (a fifth of their pixels) and noise outside them"""
    w, h = c["size"]
    fg = blobs(w, h, c["seed"]) != 0
    rng = np.random.default_rng(c["seed"] + 1)
    gray = rng.integers(1, 256, (h, w), dtype=np.uint8)
    gray[rng.integers(0, 5, (h, w)) == 0] = 0
    return (fg * 255).astype(np.uint8), gray


def labelled(c):
    """(labels (H, W) int32, records) of the case by the components model"""
    from components_model import components
    return components(component_frame(c)[0], c["connectivity"], c["min_pixels"])
