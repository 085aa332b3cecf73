"""CPU check of the hysteresis case table (tests/hysteresis_cases.py): the plain fixed-point model equals the oracle on every row, every
row has the properties it claims on the oracle's own masks, the round model respects the topological lower bound, and the table as a
whole keeps reaching every border class, direction, depth threshold and width class the GPU tests (tests/test_gpu_hysteresis.py) exist
for -- so that trimming it later says what was dropped."""
import numpy as np
import pytest

import hysteresis_cases as hc

ROWS = [(c["name"], ks) for c in hc.CASES for ks in c["ksizes"]]
_cache = {}


def measured(oracle, name, ksize, variant=0):
    key = (name, ksize, variant)
    if key not in _cache:
        case = hc.BY_NAME[name]
        img = hc.variants(case["gen"]())[0][variant]
        tl, th = hc.thresholds_for(case, ksize)
        rc, e, g = oracle.canny(img, tl, th, ksize, 0, want_gnms=True)
        assert rc == 0
        rc, lo, hi = oracle.canny_thresholds(tl, th, 0)
        assert rc == 0
        _cache[key] = (img, e, g, lo, hi, hc.measure(img, g, lo, hi))
    return _cache[key]


@pytest.mark.parametrize("name,ksize", ROWS, ids=lambda v: str(v))
def test_case_row(oracle, name, ksize):
    case = hc.BY_NAME[name]
    claims = case["claims"]
    img, e, g, lo, hi, m = measured(oracle, name, ksize)
    assert img.shape == (case["H"], case["W"])
    # the fixed point by definition equals the oracle's stack-based flood, pixel for pixel
    keep = hc.expected_edges(g, lo, hi)
    assert (keep == (e != 0)).all(), int((keep != (e != 0)).sum())
    assert set(np.unique(e).tolist()) <= {0, 255}
    assert m["kept"] == claims["kept"], (m["kept"], claims["kept"])
    if "rpg" in claims:
        assert hc.rows_per_group(case["W"], case["H"]) == claims["rpg"]
    for cls in claims.get("borders", ()):
        assert m["links"][cls], "no kept link crosses a %s border" % cls
    if ksize == 3:
        for cls in claims.get("diag", ()):
            # local and causal: with these border links cut, kept pixels beyond the border are lost
            assert hc.lost_without(m["weak"], m["strong"], cls) > 20, "nothing hangs on the %s links" % cls
    # the cell-synchronous model reaches the same fixed point; its productive rounds are k + 1 and respect the lower bound
    weak, strong = hc.masks(g, lo, hi)
    rounds, E = hc.cell_rounds(weak, strong)
    assert (E == keep).all()
    if keep.any():
        assert rounds == m["k"] + 1, (rounds, m["k"])
    if claims.get("k") is not None:
        assert m["k"] >= claims["k"], (m["k"], claims["k"])
        if claims.get("cells"):
            assert m["cells"] == claims["cells"], m["cells"]
        lower = hc.launches_lower_bound(m["k"], m["cells"])
        assert rounds >= lower >= 1
        if claims.get("cells") == 2:
            assert lower >= -(-claims["k"] // 2)                # the ceil(k / 2) of a zigzag over one border


def test_widths_claimed_are_real():
    for c in hc.CASES:
        W, H = c["W"], c["H"]
        for w in c["claims"].get("widths", ()):
            ok = {"nc2": W > hc.CHUNK, "cw56": W == 3840 and hc.chunk_words(W, 1) == 56, "cw1": W > hc.CHUNK and hc.chunk_words(W, W // hc.CHUNK) == 1,
                  "lastband": 0 < H % hc.BAND < 8}[w]
            assert ok, (c["name"], w)


def test_table_reaches_every_case(oracle):
    missing = []
    # border class x direction, over the rows and the flips of the rows marked symmetric (their borders map onto themselves)
    dirs = {cls: set() for cls in ("rowgroup", "word", "band", "chunk", "corner")}
    for c in hc.CASES:
        if not c["claims"].get("borders"):
            continue
        for v in range(4 if c["claims"].get("symmetric") or c["name"].startswith("cross") else 1):
            m = measured(oracle, c["name"], 3, v)[5]
            for cls in dirs:
                dirs[cls] |= hc.directions(m["links"].get(cls, []))
    for cls in ("rowgroup", "band"):
        for d in [(dy, dx) for dy in (-1, 1) for dx in (-1, 0, 1)]:
            if d not in dirs[cls]:
                missing.append("%s border crossed in direction %s" % (cls, d))
    for cls in ("word", "chunk"):
        for d in [(dy, dx) for dx in (-1, 1) for dy in (-1, 0, 1)]:
            if d not in dirs[cls]:
                missing.append("%s border crossed in direction %s" % (cls, d))
    for d in [(dy, dx) for dy in (-1, 1) for dx in (-1, 1)]:
        if d not in dirs["corner"]:
            missing.append("corner crossed in direction %s" % (d,))
    claims = [c["claims"] for c in hc.CASES]
    for rpg in (1, 5, 8):
        if not any(c.get("rpg") == rpg and "rowgroup" in c.get("borders", ()) for c in claims):
            missing.append("row-group crossing with rpg = %d" % rpg)
    for cls in ("band", "chunk", "corner", "bandword"):
        if not any(cls in c.get("diag", ()) for c in claims):
            missing.append("a chain that hangs on a diagonal %s link" % cls)
    slides = sorted(int(c["name"][6:]) for c in hc.CASES if c["name"].startswith("corner"))
    if slides != [-2, -1, 0, 1]:
        missing.append("corner crossing at x = 2046 .. 2049")
    for border in ("band", "chunk"):
        for t in hc.DEPTH_THRESHOLDS:
            need = t + 1 if border == "band" else (hc.TICKET_FLAGS + 1 if t < hc.WRAP_SLOTS else None)
            if need is not None and not any(c.get("cells") == 2 and border in c.get("borders", ()) and -(-c["k"] // 2) >= need for c in claims):
                missing.append("a two-cell zigzag over the %s border with ceil(k / 2) > %d" % (border, t))
    if not any("chunk" in c.get("borders", ()) and (c.get("k") or 0) >= 2 * hc.WRAP_SLOTS + 1 for c in claims):
        missing.append("a chain with more than 2 x %d crossings of the chunk border" % hc.WRAP_SLOTS)
    if not any(c["name"] == "spiral" for c in hc.CASES):
        missing.append("the spiral")
    for w in ("nc2", "cw56", "cw1", "lastband"):
        if not any(w in c.get("widths", ()) for c in claims):
            missing.append("width class " + w)
    for kept in ("all", "none", "some"):
        if not any(c["kept"] == kept for c in claims):
            missing.append("a row whose weak pixels are kept: " + kept)
    if not any(5 in c["ksizes"] and (c["claims"].get("k") or 0) > 2 * hc.WRAP_SLOTS for c in hc.CASES):
        missing.append("a deep row at kernel size 5")
    assert not missing, "the hysteresis case table no longer reaches: " + "; ".join(missing)


def test_all_or_nothing_pair_differs_everywhere(oracle):
    a = measured(oracle, "maze-seeded", 3)[1]
    b = measured(oracle, "maze-unseeded", 3)[1]
    assert not b.any() and int((a != 0).sum()) > 50000
    ia, ib = hc.BY_NAME["maze-seeded"]["gen"](), hc.BY_NAME["maze-unseeded"]["gen"]()
    assert int((ia != ib).sum()) < 400                          # the twins differ in the seed ramp only
