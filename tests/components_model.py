"""The definition of the connected-component call (include/compv_hip.h, docs/kernels/components.md) in numpy / scipy; what the GPU is compared
with bit for bit (tests/test_gpu_components.py), pinned on the CPU by tests/test_components_model.py.

  components: maximal sets of foreground (non-zero) pixels connected by 8- (or 4-) neighbour steps
  root:       the pixel of a component with the smallest raster index y * W + x
  survivors:  components with at least min_pixels pixels; ids 1, 2, ... in ascending order of the root's raster index
  label map:  int32, 0 for background and dropped components, otherwise the id
  record:     root (x, y), inclusive bounding box (x0, y0, x1, y1), pixel count -- stored at index id - 1
"""
import numpy as np
from scipy import ndimage

COMP_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("pixels", "<i4")])

STRUCTURE = {8: np.ones((3, 3), np.int32), 4: np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.int32)}


def components(edges, connectivity=8, min_pixels=1):
    """(labels int32 [H][W], records COMP_DTYPE [survivors]) of one edge map (any integer / bool array, foreground = non-zero)."""
    if connectivity not in STRUCTURE:
        raise ValueError("connectivity must be 4 or 8")
    if min_pixels < 1:
        raise ValueError("min_pixels must be >= 1")
    fg = np.asarray(edges) != 0
    H, W = fg.shape
    lab, n = ndimage.label(fg, structure=STRUCTURE[connectivity], output=np.int32)
    if n == 0:
        return np.zeros((H, W), np.int32), np.zeros(0, COMP_DTYPE)
    flat = lab.ravel()
    idx = np.flatnonzero(flat)                       # raster indices of the foreground pixels, ascending
    l = flat[idx].astype(np.int64)                   # their scipy labels, 1 .. n
    pixels = np.bincount(l, minlength=n + 1)
    # root = the first (smallest) raster index of a label
    root = np.full(n + 1, -1, np.int64)
    first = np.unique(l, return_index=True)[1]       # idx is ascending: the first occurrence is the minimum
    root[l[first]] = idx[first]
    ys, xs = idx // W, idx % W
    x0 = np.full(n + 1, W, np.int64); y0 = np.full(n + 1, H, np.int64)
    x1 = np.full(n + 1, -1, np.int64); y1 = np.full(n + 1, -1, np.int64)
    np.minimum.at(x0, l, xs); np.minimum.at(y0, l, ys)
    np.maximum.at(x1, l, xs); np.maximum.at(y1, l, ys)
    keep = np.flatnonzero(pixels[1:] >= min_pixels) + 1
    keep = keep[np.argsort(root[keep], kind="stable")]       # roots are distinct
    new_id = np.zeros(n + 1, np.int32)
    new_id[keep] = np.arange(1, len(keep) + 1, dtype=np.int32)
    rec = np.zeros(len(keep), COMP_DTYPE)
    rec["x"] = root[keep] % W; rec["y"] = root[keep] // W
    rec["x0"] = x0[keep]; rec["y0"] = y0[keep]; rec["x1"] = x1[keep]; rec["y1"] = y1[keep]
    rec["pixels"] = pixels[keep]
    return new_id[lab], rec


def summary(rec, edge_pixels):
    """(component count, share of the edge pixels that the largest component holds) -- the statistics DESIGN.md 7 argues with."""
    if len(rec) == 0 or edge_pixels == 0:
        return 0, 0.0
    return len(rec), float(rec["pixels"].max()) / float(edge_pixels)
