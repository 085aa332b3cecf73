"""CPU tests that pin the numpy / scipy model of the connected-component definition (tests/components_model.py) before the GPU is compared
with it (tests/test_gpu_components.py): against a plain breadth-first flood fill, on hand-drawn maps whose answer is written out, through
the invariants of the definition, on Canny output tied to the C oracle, and the C ABI of the two entry points."""
import ctypes
import os
import re
from collections import deque

import numpy as np
import pytest

from components_model import COMP_DTYPE, components, summary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N8 = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
N4 = [(-1, 0), (0, -1), (0, 1), (1, 0)]


def flood(e, connectivity, min_pixels):
    """The definition, literally: raster scan, breadth-first fill from every unvisited foreground pixel (which is its component's root)."""
    H, W = e.shape
    seen = np.zeros((H, W), bool)
    lab = np.zeros((H, W), np.int32)
    recs = []
    nb = N8 if connectivity == 8 else N4
    for y in range(H):
        for x in range(W):
            if not e[y, x] or seen[y, x]:
                continue
            q = deque([(y, x)])
            seen[y, x] = True
            px = []
            while q:
                cy, cx = q.popleft()
                px.append((cy, cx))
                for dy, dx in nb:
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < H and 0 <= nx < W and e[ny, nx] and not seen[ny, nx]:
                        seen[ny, nx] = True
                        q.append((ny, nx))
            if len(px) < min_pixels:
                continue
            ys = [p[0] for p in px]; xs = [p[1] for p in px]
            recs.append((x, y, min(xs), min(ys), max(xs), max(ys), len(px)))
            for cy, cx in px:
                lab[cy, cx] = len(recs)
    return lab, np.array(recs, COMP_DTYPE) if recs else np.zeros(0, COMP_DTYPE)


def check_invariants(e, connectivity, min_pixels, lab, rec):
    H, W = e.shape
    fg = e != 0
    assert lab.dtype == np.int32 and lab.shape == (H, W) and rec.dtype == COMP_DTYPE
    assert int(rec["pixels"].sum()) == int((lab > 0).sum())
    assert not (lab[~fg] != 0).any()
    full_lab, full = components(e, connectivity, 1)
    # label > 0 exactly on the pixels of the survivors
    big = np.zeros(len(full) + 1, bool)
    big[1:] = full["pixels"] >= min_pixels
    assert ((lab > 0) == big[full_lab]).all()
    roots = rec["y"].astype(np.int64) * W + rec["x"]
    assert (np.diff(roots) > 0).all()                                  # roots ascend
    for i, r in enumerate(rec):
        ys, xs = np.nonzero(lab == i + 1)
        assert len(ys) == r["pixels"] >= min_pixels
        assert lab[r["y"], r["x"]] == i + 1 and int((ys * W + xs).min()) == int(roots[i])    # the root carries the id and is the smallest index
        assert (xs.min(), ys.min(), xs.max(), ys.max()) == (r["x0"], r["y0"], r["x1"], r["y1"])   # the box is tight


def test_model_against_flood_fill():
    rng = np.random.default_rng(2024)
    n = 0
    for it in range(300):
        H, W = int(rng.integers(1, 24)), int(rng.integers(1, 40))
        e = (rng.random((H, W)) < rng.choice([0.05, 0.2, 0.4, 0.6, 0.9])).astype(np.uint8) * int(rng.integers(1, 256))
        for c in (4, 8):
            for mp in (1, 2, 5, 17):
                lab, rec = components(e, c, mp)
                flab, frec = flood(e, c, mp)
                assert (lab == flab).all() and rec.tobytes() == frec.tobytes(), (it, c, mp)
                n += len(rec)
        if it % 10 == 0:
            check_invariants(e, 8, 2, *components(e, 8, 2))
            check_invariants(e, 4, 1, *components(e, 4, 1))
    assert n > 1000


def _map(rows):
    return np.array([[1 if ch == "#" else 0 for ch in r] for r in rows], np.uint8)


def _recs(*t):
    return np.array(list(t), COMP_DTYPE)


def test_hand_drawn_maps():
    # two pixels touching by a corner: one component at 8, two at 4
    e = _map(["#.", ".#"])
    lab, rec = components(e, 8)
    assert lab.tolist() == [[1, 0], [0, 1]] and rec.tobytes() == _recs((0, 0, 0, 0, 1, 1, 2)).tobytes()
    lab, rec = components(e, 4)
    assert lab.tolist() == [[1, 0], [0, 2]] and rec.tobytes() == _recs((0, 0, 0, 0, 0, 0, 1), (1, 1, 1, 1, 1, 1, 1)).tobytes()
    # a U whose arms meet only in the last row: the root is the left arm's top, the right arm's top carries the same id
    e = _map(["#..#", "#..#", "####"])
    for c in (4, 8):
        lab, rec = components(e, c)
        assert lab.tolist() == [[1, 0, 0, 1], [1, 0, 0, 1], [1, 1, 1, 1]] and rec.tobytes() == _recs((0, 0, 0, 0, 3, 2, 8)).tobytes()
    # a frame-sized ring around an isolated pixel
    e = np.zeros((7, 9), np.uint8)
    e[0, :] = e[-1, :] = e[:, 0] = e[:, -1] = 255
    e[3, 4] = 7
    lab, rec = components(e, 8)
    assert rec.tobytes() == _recs((0, 0, 0, 0, 8, 6, 28), (4, 3, 4, 3, 4, 3, 1)).tobytes() and lab[3, 4] == 2 and lab[6, 8] == 1
    lab, rec = components(e, 8, 2)
    assert rec.tobytes() == _recs((0, 0, 0, 0, 8, 6, 28)).tobytes() and lab[3, 4] == 0 and int((lab == 1).sum()) == 28
    # empty map, 1 x 1, 1 x N, N x 1
    lab, rec = components(np.zeros((5, 6), np.uint8), 8)
    assert not lab.any() and len(rec) == 0 and summary(rec, 0) == (0, 0.0)
    lab, rec = components(np.ones((1, 1), np.uint8), 4)
    assert lab.tolist() == [[1]] and rec.tobytes() == _recs((0, 0, 0, 0, 0, 0, 1)).tobytes()
    assert len(components(np.zeros((1, 1), np.uint8), 4)[1]) == 0
    row = _map(["##.#..###"])
    lab, rec = components(row, 8)
    assert lab.tolist() == [[1, 1, 0, 2, 0, 0, 3, 3, 3]]
    assert rec.tobytes() == _recs((0, 0, 0, 0, 1, 0, 2), (3, 0, 3, 0, 3, 0, 1), (6, 0, 6, 0, 8, 0, 3)).tobytes()
    lab, rec = components(row.T.copy(), 4, 2)
    assert lab.ravel().tolist() == [1, 1, 0, 0, 0, 0, 2, 2, 2]
    assert rec.tobytes() == _recs((0, 0, 0, 0, 0, 1, 2), (0, 6, 0, 6, 0, 8, 3)).tobytes()
    assert summary(rec, 6) == (2, 0.5)
    with pytest.raises(ValueError):
        components(row, 6)
    with pytest.raises(ValueError):
        components(row, 8, 0)


def test_every_component_of_a_canny_map_holds_a_strong_pixel(oracle):
    """Tie to the oracle: hysteresis keeps exactly the weak components that hold a strong pixel, so every 8-connected component of the edge map
    must hold a pixel whose NMS gradient is above the high threshold."""
    from oracle_bindings import synth_frame
    for W, H, seed in ((640, 360, 12345), (333, 77, 5)):
        img = synth_frame(W, H, seed)
        rc, edges, gnms = oracle.canny(img, 59.0, 119.0, want_gnms=True)
        assert rc == 0
        rc, lo, hi = oracle.canny_thresholds(59.0, 119.0)
        assert rc == 0
        lab, rec = components(edges, 8)
        assert len(rec) > 3
        strong = (gnms > hi) & (edges != 0)
        assert sorted(set(np.unique(lab[strong]).tolist()) - {0}) == list(range(1, len(rec) + 1))
        check_invariants(edges, 8, 1, lab, rec)
        n, share = summary(rec, int((edges != 0).sum()))
        assert n == len(rec) and 0.0 < share <= 1.0


def test_abi_of_the_component_calls():
    """Both names are declared in the header, listed in capi.EXPORTS and exported by the built library; the record is 28 bytes."""
    from compv_amd import capi
    names = ["compvhip_plan_components", "compvhip_components_u8"]
    txt = open(os.path.join(ROOT, "include", "compv_hip.h")).read()
    declared = set(re.findall(r"COMPVHIP_API\s+[\w\s\*]+?\b(compvhip_\w+)\s*\(", txt))
    lib = capi.load()
    for s in names:
        assert s in declared and s in capi.EXPORTS and hasattr(lib, s), s
    assert "typedef struct compvhip_component" in txt
    assert ctypes.sizeof(capi.Component) == 28 == capi.COMP_DTYPE.itemsize == COMP_DTYPE.itemsize
    assert capi.COMP_DTYPE == COMP_DTYPE
    assert [f[0] for f in capi.Component._fields_] == list(COMP_DTYPE.names)
